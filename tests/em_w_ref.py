"""Reference and error bounds for ONE weighted dense EM pass (csrc/em.hip em_cp_vec_k / em_cp_k under EmWeighted, DESIGN.md section
4.5.1).  Shared by tests/test_em_w_host.py (which checks the bounds against an emulation of the kernel's fp32 arithmetic on
the CPU) and tests/test_gpu_em_w_pass.py (which compares the device pass with them).  The manner is that of tests/em_ref.py.

The pass, per entry of a block with data X0, weights W in [0, 1] and the current Xhat (xh), for the model M of the
current factors:
    q = xh - w x0                                (= (1 - w) m_old: no factor snapshot is needed)
    obs_res += w (x0 - m)^2 ; obs_x2 += w x0^2 ; num += ((1 - w) m - q)^2 ; den += q^2
    xh <- w x0 + (1 - w) m                       (update only)
stats = (num, den, obs_res, obs_x2), the order of csrc/readback.h EmStat.

Reference: everything in np.longdouble from the fp64 factors and from X0, W and Xhat AS THE DEVICE HOLDS THEM (the test
data is exact in fp32: X0 is rounded to fp32 as em_ref.make_data does and the weights are multiples of 1/256; Xhat is what
the upload's reset or an earlier pass left, which the caller passes in).

Bounds.  Derived from the kernel's arithmetic, first order in u (u = 2^-24 for fp32, 2^-53 for fp64), not measured, and
not to be widened.  beta is em_ref.beta, the bound on the device's model value m_dev; its (R + 4) u against the (R + 2) u
of the derivation leaves 2 u sum_r |a b c| >= 2 u |M| of room, which covers the second-order terms dropped below.
  * The new value.  The kernel forms  omw = fl(1 - w),  p_dev = fl(omw * m_dev),  xh_new = fl(w x0 + p_dev)  (one FMA):
    three roundings, of relative size u, on p (twice) and on the result.  With p = (1 - w) M:
        |xh_new_dev - (w x0 + p)| <= |1 - w| beta + u (2 |p| + |w x0 + p|)
  * q.  The kernel forms  wx = fl(w x0)  and  q_dev = fl(xh - wx).  xh and w x0 nearly cancel where w is close to 1, and
    what the cancellation leaves is the rounding of wx, u |w x0| (at most u (|xh| + |q|)), however small q is; the
    subtraction adds u |q|:
        |q_dev - q| <= e_q = u (|w x0| + |q|)
  * den = sum q^2:        rel <= 2 rho + rho^2 + 80 u,   rho = ||e_q|| / ||q||          (2-norms over the block)
  * num = sum (p - q)^2:  rel <= 2 rho + rho^2 + 80 u,   rho = || |1 - w| beta + 2 u |p| + e_q || / ||p - q||
  * obs_res = sum w d^2 (d = x0 - M):  rel <= 2 rho + rho^2 + 80 u,   rho = ||sqrt(w) beta|| / ||sqrt(w) d||
  * obs_x2 = sum w x0^2:  rel <= 80 u
    The 80 is em_ref's: the roundings of one term (here at most three: the difference, the product with w, the fused
    multiply-add), 64 terms per accumulator lane per 64-column tile in the tensor's precision, then the lane, wave and
    block sums in fp64.
A sum whose reference terms are all exactly 0 (num and den under W = 1, obs_res and obs_x2 under W = 0) must be exactly 0.
"""
import numpy as np

import em_ref
from em_ref import SUM_TERMS, U_OF

STAT_NAMES = em_ref.STAT_NAMES


def make_weights(dims, rng, kind='uniform'):
    """Weights that are exact in fp32 and fp64: 'uniform' multiples of 1/256 in [0, 1] with a tenth of the entries at 0,
    'boolean' (40 % zeros), 'ones', 'zeros'."""
    if kind == 'ones':
        return np.ones(dims, order='F')
    if kind == 'zeros':
        return np.zeros(dims, order='F')
    if kind == 'boolean':
        return np.asfortranarray((rng.random(dims) >= 0.4).astype(np.float64))
    W = rng.integers(0, 257, size=dims).astype(np.float64) / 256.0
    W[rng.random(dims) < 0.1] = 0.0
    return np.asfortranarray(W)


def reset(X0, W, prec):
    """Xhat as the upload and the start of a solve leave it: W o X0 rounded once to the block's precision."""
    p = np.asarray(W, dtype=np.float64) * np.asarray(X0, dtype=np.float64)          # exact in fp64 for this module's inputs
    return np.asfortranarray(p.astype(np.float32).astype(np.float64) if prec == 'f32' else p)


class EmWRef:
    """One weighted pass in longdouble.  X0, W, Xh: data, weights and the Xhat the pass starts from, as the device holds
    them; U: the fp64 factors; M: their longdouble model when the caller has it already."""

    def __init__(self, X0, W, Xh, U, M=None):
        ld = np.longdouble
        self.X0 = np.asarray(X0, dtype=np.float64)
        self.W = np.asarray(W, dtype=np.float64)
        self.Xh = np.asarray(Xh, dtype=np.float64)
        self.U = [np.asarray(u, dtype=np.float64) for u in U]
        self.M = em_ref.model(self.U) if M is None else M
        w, x0, xh = self.W.astype(ld), self.X0.astype(ld), self.Xh.astype(ld)
        self.wx = w * x0
        self.q = xh - self.wx
        self.p = (1 - w) * self.M
        self.d = x0 - self.M
        self.n = self.p - self.q
        self.X_new_ld = self.wx + self.p
        self.X_new = np.asfortranarray(self.X_new_ld.astype(np.float64))
        self.stats = np.array([float((self.n ** 2).sum()), float((self.q ** 2).sum()),
                               float((w * self.d ** 2).sum()), float((w * x0 ** 2).sum())])

    def beta(self, prec):
        return em_ref.beta(self.U, prec)

    def entry_bound(self, prec):
        """Per-entry bound on the new Xhat (module docstring)."""
        u = U_OF[prec]
        return (np.abs(1.0 - self.W) * self.beta(prec)
                + u * (2 * np.abs(self.p) + np.abs(self.X_new_ld)).astype(np.float64))

    def entry_ratio(self, data, prec):
        """max over the entries of |data - Xhat_new| / bound; entries whose bound is 0 must be exact."""
        err = np.abs(np.asarray(data, dtype=np.longdouble) - self.X_new_ld).astype(np.float64)
        b = self.entry_bound(prec)
        if np.any((b == 0) & (err > 0)):
            return np.inf
        return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0

    def stat_bounds(self, prec):
        """Relative bounds on (num, den, obs_res, obs_x2); 0 where the reference sum is exactly 0."""
        u = U_OF[prec]
        f = lambda a: np.asarray(a, dtype=np.float64)
        b = self.beta(prec)
        e_q = u * (np.abs(f(self.wx)) + np.abs(f(self.q)))
        e_n = np.abs(1.0 - self.W) * b + 2 * u * np.abs(f(self.p)) + e_q
        sw = np.sqrt(self.W)
        out = np.zeros(4)
        for k, (e, t) in enumerate(((e_n, f(self.n)), (e_q, f(self.q)), (sw * b, sw * f(self.d)))):
            nt = float(np.linalg.norm(t))
            if self.stats[k] > 0 and nt > 0:
                rho = float(np.linalg.norm(e)) / nt
                out[k] = 2 * rho + rho * rho + SUM_TERMS * u
        out[3] = SUM_TERMS * u if self.stats[3] > 0 else 0.0
        return out

    def stat_ratios(self, stats, prec):
        """|stats - reference| / (bound * reference) per statistic; 0 where both agree exactly, inf where the reference is
        exactly 0 and the statistic is not."""
        bnd = self.stat_bounds(prec)
        out = np.zeros(4)
        for k in range(4):
            err = abs(float(stats[k]) - self.stats[k])
            if err == 0.0:
                continue
            out[k] = err / (bnd[k] * self.stats[k]) if bnd[k] * self.stats[k] > 0 else np.inf
        return out


# ---- the kernel's fp32 arithmetic in numpy ------------------------------------------------------------------------------
def _fma32(a, b, c):
    """float32(a * b + c) from fp32 arrays: the product is exact in fp64, so this is the fused multiply-add up to a double
    rounding (em_ref.emulate_f32_pass)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_f32_pass(X0, W, Xh, U, tile=64):
    """The weighted strip kernel's arithmetic for a 3-way block walked along mode 2, in numpy: the model value as
    em_ref.emulate_f32_pass forms it, then em_w_entry's products and differences rounded one by one in fp32 and its fused
    multiply-adds, the four sums per row and per `tile` columns in fp32, then in fp64.  Returns (Xhat_new as a float32
    array, stats)."""
    A, B, C = [np.asarray(u, dtype=np.float64) for u in U]
    I, J, K = A.shape[0], B.shape[0], C.shape[0]
    ac = (A[:, None, :] * C[None, :, :]).astype(np.float32)          # [i, k, r]
    b = B.astype(np.float32)                                         # [j, r]
    m = np.zeros((I, J, K), dtype=np.float32)
    for r in range(A.shape[1]):
        m = _fma32(np.broadcast_to(ac[:, None, :, r], m.shape), np.broadcast_to(b[None, :, None, r], m.shape), m)
    x0, w, xh = [np.asarray(a, dtype=np.float32) for a in (X0, W, Xh)]
    wx = w * x0
    q = xh - wx
    p = (np.float32(1) - w) * m
    d = x0 - m
    wd = w * d
    n = p - q
    xn = np.where(w == 1, x0, _fma32(w, x0, p))                    # the data itself where w = 1, as the kernel selects
    stats = np.zeros(4)
    for k, (a, c) in enumerate(((n, n), (q, q), (wd, d), (wx, x0))):
        total = 0.0
        for j0 in range(0, J, tile):
            s = np.zeros((I, K), dtype=np.float32)
            for j in range(j0, min(j0 + tile, J)):
                s = _fma32(a[:, j, :], c[:, j, :], s)
            total += float(s.astype(np.float64).sum())
        stats[k] = total
    return xn, stats
