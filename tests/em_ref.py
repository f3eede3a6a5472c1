"""Reference and error bounds for ONE dense EM pass (csrc/em.hip; functions/cmtf_fun_AOADMM.m:408-441, :1224-1226,
:1249-1252).  Shared by tests/test_em_pass_host.py (which checks the bounds against an emulation of the kernel's fp32
arithmetic on the CPU) and tests/test_gpu_em_pass.py (which compares the device pass with them).

The pass, per entry of a block with data X and mask (1 = observed), for the model M of the current factors:
    observed:  obs_res += (x - m)^2 ; obs_x2 += x^2
    missing :  num += (m - x)^2 ; den += x^2 ; x <- m            (update only)
stats = (num, den, obs_res, obs_x2), the order of csrc/readback.h EmStat.

Reference: M in np.longdouble from the fp64 factors, the four sums in longdouble, X_new = where(observed, X, M).

Bounds.  They are derived from the kernel's arithmetic, not measured, and are not to be widened.
  * An imputed value.  The strip kernel rounds A(i,r)*F(f,r) (F the factor of the fixed mode) once to the tensor's
    precision, rounds the walked factor's row once, then runs an R-term FMA chain in that precision:
        |m_dev - M| <= beta = (R + 4) u sum_r |A_ir B_jr C_kr|,     u = 2^-24 (fp32), 2^-53 (fp64)
    (two roundings of the inputs plus gamma_R of the chain is (R + 2) u + O(u^2); the kernel for R > 32 and the PARAFAC2
    kernel multiply and add separately, which stays below the same figure; the merged Khatri-Rao factor of an N-way
    block is one more fp64 rounding per merged mode).
  * obs_res and num.  With d the exact residuals over the entries the sum runs over and rho = |beta| / |d| (2-norms over
    those entries):   rel <= 2 rho + rho^2 + 80 u.   The 80: one rounding of x - m, 64 terms per accumulator lane per
    64-column tile in the tensor's precision, then the lane, wave and block sums in fp64.
  * obs_x2 and den:  rel <= 80 u.
"""
import numpy as np

U_OF = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
SUM_TERMS = 80                    # see above
STAT_NAMES = ('num', 'den', 'obs_res', 'obs_x2')


def kr_rest(U):
    """Khatri-Rao product of U[1:] with the rows in column-major order of modes 2..N (mode 2 fastest)."""
    K = U[1]
    for F in U[2:]:
        K = (F[:, None, :] * K[None, :, :]).reshape(-1, K.shape[1])
    return K


def model(U, dtype=np.longdouble):
    """sum_r prod_n U_n(i_n, r) as an array of the block's shape."""
    U = [np.asarray(u, dtype=dtype) for u in U]
    dims = tuple(u.shape[0] for u in U)
    return np.asarray(U[0] @ kr_rest(U).T).reshape(dims, order='F')


def beta(U, prec):
    """Per-entry bound on an imputed value (module docstring), fp64 array of the block's shape."""
    R = np.asarray(U[0]).shape[1]
    return (R + 4) * U_OF[prec] * model([np.abs(np.asarray(u, dtype=np.float64)) for u in U], np.float64)


def random_factors(dims, R, rng):
    return [rng.standard_normal((n, R)) for n in dims]


def make_data(dims, R, rng, fill='nonzero'):
    """(X, U): X = a rank-R model from factors OTHER than U plus 10 % noise, rounded to fp32 so that the stored value is
    exact in both precisions; the residual X - model(U) is O(|X|).  The values at the missing positions are whatever X
    holds there (non-zero); fill = 'zero' is applied by EmRef from the mask."""
    V = random_factors(dims, R, rng)
    X = model(V, np.float64)
    N = rng.standard_normal(dims)
    X = X + 0.1 * np.linalg.norm(X) / np.linalg.norm(N) * N
    X = np.asfortranarray(X.astype(np.float32).astype(np.float64))
    return X, random_factors(dims, R, rng)


class EmRef:
    """One EM pass in longdouble.  X: the uploaded data (values exact in fp32), observed: boolean array of X's shape,
    U: the fp64 factors; M: their longdouble model when the caller has it already."""

    def __init__(self, X, observed, U, M=None):
        self.X = np.asarray(X, dtype=np.float64)
        self.obs = np.asarray(observed, dtype=bool)
        self.U = [np.asarray(u, dtype=np.float64) for u in U]
        self.R = self.U[0].shape[1]
        self.M = model(self.U) if M is None else M               # longdouble
        self.d = self.X.astype(np.longdouble) - self.M
        miss = ~self.obs
        x2 = self.X.astype(np.longdouble) ** 2
        d2 = self.d ** 2
        self.stats = np.array([float(d2[miss].sum()), float(x2[miss].sum()), float(d2[self.obs].sum()),
                               float(x2[self.obs].sum())])
        self.X_new = np.asfortranarray(np.where(self.obs, self.X, self.M.astype(np.float64)))

    def beta(self, prec):
        return beta(self.U, prec)

    def stat_bounds(self, prec):
        """Relative bounds on (num, den, obs_res, obs_x2); a sum over no entry (or of exact zeros) must be exactly 0,
        its bound is 0."""
        u = U_OF[prec]
        b = self.beta(prec)
        miss = ~self.obs
        out = np.zeros(4)
        for q, sel in ((0, miss), (2, self.obs)):
            nd = float(np.sqrt((self.d[sel] ** 2).sum()))
            if nd > 0:
                rho = float(np.linalg.norm(b[sel])) / nd
                out[q] = 2 * rho + rho * rho + SUM_TERMS * u
        out[1] = SUM_TERMS * u if self.stats[1] > 0 else 0.0
        out[3] = SUM_TERMS * u if self.stats[3] > 0 else 0.0
        return out

    def stat_ratios(self, stats, prec):
        """|stats - reference| / (bound * reference) per statistic; 0 where both are exactly 0, inf where only the
        reference is."""
        bnd = self.stat_bounds(prec)
        out = np.zeros(4)
        for q in range(4):
            err = abs(float(stats[q]) - self.stats[q])
            if err == 0.0:
                continue
            out[q] = err / (bnd[q] * self.stats[q]) if bnd[q] * self.stats[q] > 0 else np.inf
        return out

    def entry_ratio(self, data, prec, scale=1.0):
        """max over the missing entries of |data - M| / (scale * beta); 0 without missing entries."""
        miss = ~self.obs
        if not miss.any():
            return 0.0
        err = np.abs(np.asarray(data, dtype=np.longdouble) - self.M)[miss]
        b = self.beta(prec)[miss] * scale
        return float((err / np.maximum(b, np.finfo(np.float64).tiny)).max())

    def mttkrp(self, n):
        from oracle.tensor_ops import mttkrp as o_mttkrp
        return o_mttkrp(self.X_new, self.U, n)


# ---- the kernel's fp32 arithmetic in numpy ------------------------------------------------------------------------------
def emulate_f32_pass(X, observed, U, tile=64):
    """The strip kernel's arithmetic for a 3-way block walked along mode 2, in numpy: float32(A*C) and float32(B), a
    sequential fp32 multiply-add over r (the product of two fp32 numbers is exact in fp64, so float32(fp64 sum) is the
    fused multiply-add up to a double rounding), squares accumulated per row and per `tile` columns in fp32, then in
    fp64.  Returns (m as a float32 array, stats)."""
    A, B, C = [np.asarray(u, dtype=np.float64) for u in U]
    I, J, K = A.shape[0], B.shape[0], C.shape[0]
    R = A.shape[1]
    ac = (A[:, None, :] * C[None, :, :]).astype(np.float32)          # [i, k, r]
    b = B.astype(np.float32)                                         # [j, r]
    m = np.zeros((I, J, K), dtype=np.float32)
    for r in range(R):
        prod = ac[:, None, :, r].astype(np.float64) * b[None, :, None, r].astype(np.float64)
        m = (prod + m.astype(np.float64)).astype(np.float32)
    x = np.asarray(X, dtype=np.float32)
    obs = np.asarray(observed, dtype=bool)
    d = x - m                                                        # fp32
    zero = np.float32(0)
    terms = [np.where(~obs, d, zero), np.where(~obs, x, zero), np.where(obs, d, zero), np.where(obs, x, zero)]
    stats = np.zeros(4)
    for q, t in enumerate(terms):
        total = 0.0
        for j0 in range(0, J, tile):
            s = np.zeros((I, K), dtype=np.float32)
            for j in range(j0, min(j0 + tile, J)):
                v = t[:, j, :]
                s = (v.astype(np.float64) * v.astype(np.float64) + s.astype(np.float64)).astype(np.float32)
            total += float(s.astype(np.float64).sum())
        stats[q] = total
    return m, stats
