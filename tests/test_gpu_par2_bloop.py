"""GPU: every kernel class of the PARAFAC2 B_k loop (ADMM_B_Parafac2, cmtf_fun_AOADMM.m:509-589, csrc/par2.hip), run as
the solver runs it (`Engine.par2_b_loop` -> aoadmm_op_par2_b_loop -> par2_b_loop: slab systems, the loop on the path
par2_b_path() names, Gram matrices), against a numpy fp64 loop.

Reference (`RefLoop`): oracle/aoadmm.py ADMM_B_Parafac2 line for line -- Cholesky solve, P_k = U V' of the economy SVD,
the rho-weighted DeltaB, the dual update, prox from oracle.prox, the four residual means (the dual coupling residual
without a zero check) -- with rho_k and L_k as cmtf_fun_AOADMM.m:194-212 builds them.

Every case asserts: the path (folded, slab kernel class, in_lds, par2_b_dual_fold_k class) against LITERALS of the case
table (a moved threshold turns the case red: pick a new shape), the iteration count, B / P / mu / DeltaB / Z / muZ
(largest relative Frobenius distance over the slabs), rho, L, the four residuals, and GB against the host B_k'B_k of the
returned B_k.

Bar: the device takes the polar factor by one-sided Jacobi, the reference by SVD.  The same kind of difference exists
between two host formulations, so each case also runs the numpy loop with P_k = W V diag(lambda^-1/2) V' from
eigh(W'W); the largest distance of the two host results over all compared outputs is the case's floor and its bar is
max(1e-11, 10 x floor) (the rule of tests/test_gpu_admm.py).  The bar is never taken from the device.  Largest floor
over the cases of this file: LARGEST_FLOOR below.
Residuals: a residual is a mean of ratios ||x - y|| / ||z||; x and y carry an error of bar * ||x|| each and z one of
bar * ||z||, so the bound is bar * (mean(||x|| + ||y||) / ||z|| + residual).  GB: each entry is a sum of J_k products in
four partial sums, |error| <= (J_k / 4 + 3) eps sqrt(G_rr G_qq), hence ||error||_F <= (J_k / 4 + 3) eps trace(G).

Inputs (`make_inputs`) keep the polar factor well conditioned: DeltaB has singular values in [0.7, 1.6],
B_true_k = Q_k DeltaB with Q_k orthonormal, Ak = w B_true_k (D_k GA D_k) + 5 % noise, P starts as a perturbed Q_k, mu
and muZ at 0.05 x noise.  The primal coupling residual then falls by 0.6-0.8 per iteration from the second on.

Early exit: k* comes from the reference history with tolerances 0; the tolerance is the geometric mean of the residual
at k* and the smallest earlier one, asserted on the reference alone to sit >= 10 % from every residual up to k*.

Class -> case (ids as pytest prints them):
  folded, par2_b_slab_fold_regs_k<1|2|4>    regs-R{1..4}-J{64|65|128|129|256} (a slab with J_k = R in each, J_k = 1 at R = 1)
  folded, par2_b_slab_fold_k<4>             lds4-R4-J257, lds4-R1-J257; in_lds = 0: nolds-R3-J2100
  folded, par2_b_slab_fold_k<8>             lds8-R{5,6,7,8}-J70; in_lds edge: lds8-R8-J760 (1), lds8-R8-J761 (0), nolds-R8-J800
  par2_b_dual_fold_k<16|64>                 R <= 4 | R in 5..8 of the above; second round of the unrolled sum: K257-R3, K129-R6
  par2_b_head lane stride                   K1-R3, K64-R3, K65-R3
  four-launch, par2_b_slab_k<16|64>         four-R9, four-R16 | four-R17, four-R48 (ew 16 in par2_deltab_combine_k),
                                            four-R64 (65 536 B of dynamic LDS), four-R9-K300 (ksum_tile: slabs > groups)
  four-launch constrained                   nn-regs1 / regs2 / regs4 / lds4 / lds8 / lds16, unimodal-regs2,
                                            tpar2-K2, tpar2-K64; refused: tPARAFAC2 at K = 65 and with ragged J_k
  loop control                              inner1-* / inner6-* (parity into par2_b_close_k; 5 is the default of every case),
                                            exit-pc-odd / exit-pc-even / exit-dc (folded), exit-four-{pc,pz,dc,dz}
  degenerate                                sc0 (muZ stays 0: unscaled dual constraint residual), a zero row of C (not PD)
  exact                                     exact-folded, exact-four (array_equal), asym-folded, asym-four (at the bar)
"""
import functools
import zlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from oracle import prox as OP

pytestmark = pytest.mark.gpu

REGS1, REGS2, REGS4, LDS4, LDS8, LDS16, LDS64 = range(7)      # AOADMM_P2SLAB_* (include/aoadmm_hip.h)
SLAB_NAME = ['regs<1>', 'regs<2>', 'regs<4>', 'lds<4>', 'lds<8>', 'lds<16>', 'lds<64>']

# Largest distance between the two host formulations (SVD / eigh(W'W) polar factor) over every case of this file (host
# only, no device involved): 2.3e-13 (sc0; 1.2e-13 at regs-R3-J128 with one inner iteration).  Every case is required to
# stay below MAX_FLOOR, so every case runs at the 1e-11 bar.
LARGEST_FLOOR = 2.3e-13
MAX_FLOOR = 1e-12

NONNEG = ('non-negativity',)
UNIMODAL = ('unimodality', True)
TPAR2 = ('tPARAFAC2', 0.3)
WEIGHT = 0.7
EXIT_INNER = 10
INF = float('inf')


def case(cid, R, J, path, con=None, inner=5, kind='random', rho_scale=1.0):
    return dict(id=cid, R=R, J=tuple(J), path=path, con=con, inner=inner, kind=kind, rho_scale=rho_scale)


def ragged(Jmax, R):
    """Jmax, a slab with J_k = R, and J_k mod 4 taking all four values; J_k R on both sides of a multiple of 128."""
    return [R, Jmax] + [max(R, Jmax - d) for d in (1, 2, 3)] + [max(R, Jmax // 2 + 1)]


def tall(Jmax, R):
    """The same without the square slab: every J_k >= 2 R."""
    return [Jmax - d for d in (0, 1, 2, 3)] + [2 * R, 2 * R + 5]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_inputs(c):
    rng = np.random.default_rng(zlib.crc32(c['id'].split('|')[0].encode()))
    R, J, con, kind = c['R'], c['J'], c['con'], c['kind']
    K = len(J)
    w = WEIGHT
    Cm = rng.random((K, R)) + 0.5
    if kind == 'random':
        if con == NONNEG:
            # a truth the constraint agrees with: Q_k >= 0 (columns on disjoint rows), DeltaB >= 0
            DeltaB = np.diag(np.linspace(0.8, 1.3, R)) + 0.3 / R
        else:
            U, _ = np.linalg.qr(rng.standard_normal((R, R)))
            V, _ = np.linalg.qr(rng.standard_normal((R, R)))
            sv = np.linspace(0.7, 1.6, R) if R > 1 else np.array([1.1])
            DeltaB = (U * sv) @ V.T
        sv = np.linalg.svd(DeltaB, compute_uv=False)
        assert 0.7 - 1e-12 <= sv.min() and sv.max() <= 1.6 + 1e-12
        nF = 4 * R + 20
        F = rng.standard_normal((nF, R))
        GA = F.T @ F / nF
        Ak, P, mu, Z, muZ = [], [], [], [], []
        for k, j in enumerate(J):
            if con == NONNEG:
                Q = np.zeros((j, R))
                rows = rng.permutation(j)
                Q[rows, np.arange(j) % R] = rng.random(j) + 0.2
                Q /= np.linalg.norm(Q, axis=0)
            else:
                Q, _ = np.linalg.qr(rng.standard_normal((j, R)))
            Bt = Q @ DeltaB
            sig = w * Bt @ (Cm[k][:, None] * GA * Cm[k][None, :])
            Ak.append(sig + 0.05 * rng.standard_normal((j, R)))
            P.append(np.linalg.qr(Q + 0.1 / np.sqrt(j) * rng.standard_normal((j, R)))[0])
            mu.append(0.05 * rng.standard_normal((j, R)))
            Z.append(Bt + 0.05 * rng.standard_normal((j, R)))
            muZ.append(0.05 * rng.standard_normal((j, R)))
    elif kind == 'positive':
        # everything positive, diagonal systems, mu = muZ = 0: B_k > 0 after one iteration, so Z_k = B_k and muZ stays 0
        GA = 1.3 * np.eye(R)
        DeltaB = rng.random((R, R)) + 0.2
        Ak = [rng.random((j, R)) + 0.5 for j in J]
        P = [rng.random((j, R)) / np.sqrt(j) for j in J]
        Z = [rng.random((j, R)) + 0.1 for j in J]
        mu = [np.zeros((j, R)) for j in J]
        muZ = [np.zeros((j, R)) for j in J]
    elif kind in ('exact', 'asym'):
        # C = 1, mu = 0, P made of unit vectors.  exact: GA = 2 I and w = 1.5 give rho_k = 2, system 4 I, L_k = 2 I;
        # column r of Ak + P is 4 (r + 1) on rows 4r..4r+3 and zero elsewhere, so B_k = (r + 1) there, W_k = B_k has
        # orthogonal columns of norm 2 (r + 1) (no rotation), P_k = 1/2 there, DeltaB = diag(2 (r + 1)), mu = 0: all exact.
        # asym: L_k and DeltaB without symmetry (GA tridiagonal, DeltaB unit upper bidiagonal), integer Ak.
        w = 1.5
        Cm = np.ones((K, R))
        P = []
        for j in J:
            Pk = np.zeros((j, R))
            Pk[(4 if kind == 'exact' else 1) * np.arange(R), np.arange(R)] = 1.0
            P.append(Pk)
        mu = [np.zeros((j, R)) for j in J]
        Z, muZ = None, None
        if kind == 'exact':
            GA = 2.0 * np.eye(R)
            DeltaB = np.eye(R)
            Ak = []
            for k, j in enumerate(J):
                A = np.zeros((j, R))
                for r in range(R):
                    A[4 * r:4 * r + 4, r] = 4.0 * (r + 1)
                Ak.append(A - P[k])
        else:
            GA = 4.0 * np.eye(R) + np.eye(R, k=1) + np.eye(R, k=-1)
            DeltaB = np.eye(R) + 0.5 * np.eye(R, k=1)
            Ak = [rng.integers(-3, 4, size=(j, R)).astype(np.float64) for j in J]
    else:
        raise ValueError(kind)
    if con is None:
        Z = muZ = None
    inp = dict(R=R, J=J, K=K, w=w, rho_scale=c['rho_scale'], con=con, GA=GA, C=Cm, DeltaB=DeltaB, Ak=Ak, P=P, mu=mu,
               Z=Z, muZ=muZ)
    for v in inp.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return inp


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def polar_svd(W):
    U, _, Vt = np.linalg.svd(W, full_matrices=False)
    return U @ Vt                                                               # :534


def polar_eigh(W):
    lam, V = np.linalg.eigh(W.T @ W)
    return W @ ((V / np.sqrt(lam)) @ V.T)


class RefLoop:
    """ADMM_B_Parafac2 in numpy (oracle/aoadmm.py:433-477).  Iterates are computed once and kept, so the runs with
    tolerances walk the same `while` over the same states."""

    def __init__(self, inp, polar):
        self.i, self.polar = inp, polar
        R, K, w = inp['R'], inp['K'], inp['w']
        self.rho = np.zeros(K)
        self.L = []
        for k in range(K):
            Dk = np.diag(inp['C'][k])
            Ck = Dk @ inp['GA'] @ Dk                                            # :194
            self.rho[k] = inp['rho_scale'] * (np.trace(Ck) / R)                 # :195-198
            Bs = w * Ck + self.rho[k] / 2 * np.eye(R)                           # :199-200
            if inp['con'] is not None:
                Bs = Bs + self.rho[k] / 2 * np.eye(R)                           # :210
            self.L.append(np.linalg.cholesky(Bs))                               # :212
        self.prox = None
        if inp['con'] is not None:
            self.prox = OP.constraints_to_prox([1], [inp['con']], [list(inp['J'])])[0][0]
        self.states = [dict(B=None, P=inp['P'], mu=inp['mu'], DeltaB=inp['DeltaB'], Z=inp['Z'], muZ=inp['muZ'],
                            res=(np.inf,) * 4, scale=None)]

    def _step(self):
        i, s = self.i, self.states[-1]
        K, rho, con = i['K'], self.rho, i['con']
        D = s['DeltaB']
        B, P = [], []
        for k in range(K):
            A_inner = i['Ak'][k] + rho[k] / 2 * (s['P'][k] @ D - s['mu'][k])                    # :526
            if con is not None:
                A_inner = A_inner + rho[k] / 2 * (s['Z'][k] - s['muZ'][k])                      # :527-529
            Bk = OA._solve_llt_right(A_inner, self.L[k])                                        # :530
            B.append(Bk)
            P.append(self.polar((Bk + s['mu'][k]) @ D.T))                                       # :532-534
        newD = np.zeros_like(D)
        for k in range(K):
            newD = newD + rho[k] * P[k].T @ (B[k] + s['mu'][k])                                 # :541
        newD = newD / np.sum(rho)                                                               # :544
        mu = [s['mu'][k] + B[k] - P[k] @ newD for k in range(K)]                                # :546
        pz = dz = 0.0
        Z, muZ = None, None
        sz = sdz = 0.0
        with np.errstate(invalid='ignore', divide='ignore'):
            if con is not None:
                V = [B[k] + s['muZ'][k] for k in range(K)]
                if con[0] == 'tPARAFAC2':                                                       # :553
                    Z = list(self.prox(V, rho))
                else:
                    Z = [self.prox(V[k], float(rho[k])) for k in range(K)]                      # :568
                muZ = [s['muZ'][k] + B[k] - Z[k] for k in range(K)]                             # :569
                for k in range(K):
                    nb = OA._fro(B[k])
                    pz += OA._fro(B[k] - Z[k]) / nb / K                                         # :571
                    scaling = OA._fro(muZ[k])
                    d = OA._fro(s['Z'][k] - Z[k])
                    dz += (d / scaling if scaling > 0 else d) / K                               # :572-577
                    sz += (nb + OA._fro(Z[k])) / nb / K
                    sdz += (OA._fro(s['Z'][k]) + OA._fro(Z[k])) / (scaling if scaling > 0 else 1.0) / K
            pc = dc = sdc = 0.0
            for k in range(K):                                                                  # :582-585
                PD = P[k] @ newD
                pc += OA._fro(B[k] - PD) / OA._fro(B[k]) / K
                dc += OA._fro(s['P'][k] @ D - PD) / OA._fro(mu[k]) / K
                sdc += (OA._fro(s['P'][k] @ D) + OA._fro(PD)) / OA._fro(mu[k]) / K
        # what each residual is a ratio of (see the module docstring): the scale of its error bound
        scale = (2.0, sz, sdc, sdz)
        self.states.append(dict(B=B, P=P, mu=mu, DeltaB=newD, Z=Z, muZ=muZ,
                                res=(float(pc), float(pz), float(dc), float(dz)), scale=scale))

    def run(self, max_inner, tol=(0.0, 0.0, 0.0, 0.0)):
        it, res = 0, (np.inf,) * 4
        while it < max_inner and any(r > t for r, t in zip(res, tol)):                          # :520
            it += 1
            if len(self.states) <= it:
                self._step()
            res = self.states[it]['res']
        out = dict(self.states[it])
        out['inner_iters'] = it
        out['GB'] = np.stack([b.T @ b for b in out['B']])
        return out

    def history(self, n):
        self.run(n)
        return [[s['res'][q] for s in self.states[1:n + 1]] for q in range(4)]


def _key(c):
    return (c['id'].split('|')[0], c['R'], c['J'], c['con'], c['kind'], c['rho_scale'])


@functools.lru_cache(maxsize=None)
def _reference(key):
    cid, R, J, con, kind, rho_scale = key
    inp = make_inputs(dict(id=cid, R=R, J=J, con=con, kind=kind, rho_scale=rho_scale))
    return inp, RefLoop(inp, polar_svd), RefLoop(inp, polar_eigh)


def reference(c):
    """(inputs, SVD loop, eigh loop) of a case; computed once, shared, never modified."""
    return _reference(_key(c))


STATE = ('B', 'P', 'mu', 'Z', 'muZ')


def slab_dist(a, b):
    """Largest relative Frobenius distance over the slabs."""
    return max(float(np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)) for x, y in zip(a, b))


def distances(out, ref, loop):
    d = {k: slab_dist(out[k], ref[k]) for k in STATE if ref[k] is not None}
    if len(loop.rho) == 1:
        # K = 1: P_1 spans the columns of B_1 + mu_1 and DeltaB = P_1'(B_1 + mu_1), so mu_1 + B_1 - P_1 DeltaB = 0 in exact
        # arithmetic: mu is rounding noise.  Its error is measured on the scale of what it is the difference of, B_1.
        d['mu'] = float(np.linalg.norm(out['mu'][0] - ref['mu'][0]) / np.linalg.norm(ref['B'][0]))
    d['DeltaB'] = slab_dist([out['DeltaB']], [ref['DeltaB']])
    d['rho'] = slab_dist([np.asarray(out.get('rho', loop.rho))], [loop.rho])
    d['L'] = slab_dist(list(out.get('L', loop.L)), loop.L)
    return d


def _res_close(dev, ref, bound):
    if not np.isfinite(ref):
        return bool(dev == ref or (np.isnan(ref) and np.isnan(dev)))
    return abs(dev - ref) <= bound


def res_compared(loop):
    """K = 1: the dual coupling residual is ||...|| / ||mu_1||, a ratio to rounding noise (see distances): no digits."""
    return (0, 1, 3) if len(loop.rho) == 1 else (0, 1, 2, 3)


def host_floor(c, max_inner, tol):
    _, loop, alt = reference(c)
    ref, other = loop.run(max_inner, tol), alt.run(max_inner, tol)
    assert other['inner_iters'] == ref['inner_iters'], 'the two host formulations stop at different iterations'
    d = distances(other, ref, loop)
    for q in res_compared(loop):
        if np.isfinite(ref['res'][q]) and ref['scale'][q] > 0:
            d['res%d' % q] = abs(other['res'][q] - ref['res'][q]) / (ref['scale'][q] + ref['res'][q])
    return ref, max(d.values())


def check_case(eng, c, tol=(0.0, 0.0, 0.0, 0.0), expect_iters=None):
    inp, loop, _ = reference(c)
    max_inner = c['inner']
    ref, floor = host_floor(c, max_inner, tol)
    assert floor < MAX_FLOOR, ('the two host formulations differ by %.2e: the input sits on a tie of a discontinuous prox '
                               'or has an ill-conditioned polar factor; pick another input' % floor)
    bar = max(1e-11, 10 * floor)
    if expect_iters is not None:
        assert ref['inner_iters'] == expect_iters
    out = eng.par2_b_loop(inp['J'], inp['R'], inp['Ak'], inp['GA'], inp['C'], inp['w'], inp['rho_scale'], inp['con'],
                          max_inner, tol, inp['P'], inp['mu'], inp['DeltaB'], inp['Z'], inp['muZ'])
    d = distances(out, ref, loop)
    print('%s R %d K %d Jmax %d inner %d: path %s its %d/%d floor %.2e bar %.2e %s res dev %s ref %s'
          % (c['id'], inp['R'], inp['K'], max(inp['J']), max_inner, out['path'], out['inner_iters'], ref['inner_iters'],
             floor, bar, ' '.join('%s %.2e' % kv for kv in d.items()), ' '.join('%.15e' % v for v in out['res']),
             ' '.join('%.15e' % v for v in ref['res'])))
    assert out['path'] == c['path'], ('dispatch runs (folded %d, %s, in_lds %d, dual_fold %d) here, the case is meant '
                                      'for (folded %d, %s, in_lds %d, dual_fold %d): pick a new shape'
                                      % (out['path'][0], SLAB_NAME[out['path'][1]], out['path'][2], out['path'][3],
                                         c['path'][0], SLAB_NAME[c['path'][1]], c['path'][2], c['path'][3]))
    assert out['inner_iters'] == ref['inner_iters']
    for k, v in d.items():
        assert v < bar, (k, v, bar)
    for q in res_compared(loop):
        name = ('pr_coupl', 'pr_constr', 'du_coupl', 'du_constr')[q]
        bound = bar * (ref['scale'][q] + ref['res'][q]) if np.isfinite(ref['res'][q]) else 0.0
        assert _res_close(out['res'][q], ref['res'][q], bound), (name, out['res'][q], ref['res'][q], bound)
    eps = np.finfo(np.float64).eps
    for k, j in enumerate(inp['J']):
        G = out['B'][k].T @ out['B'][k]
        assert np.linalg.norm(out['GB'][k] - G) <= (j / 4 + 3) * eps * np.trace(G), (k, j)
    return out, ref


# ---------------------------------------------------------------------------------------------------------------------
# kernel classes, tolerances 0, five inner iterations
# ---------------------------------------------------------------------------------------------------------------------
def _regs_cases():
    out = []
    for Jmax, slab in ((64, REGS1), (65, REGS2), (128, REGS2), (129, REGS4), (256, REGS4)):
        for R in (1, 2, 3, 4):
            J = ragged(Jmax, R) + ([1] if R == 1 else [])
            out.append(case('regs-R%d-J%d' % (R, Jmax), R, J, (1, slab, 1, 16)))
    return out


FOLDED_CASES = _regs_cases() + [
    case('lds4-R4-J257', 4, ragged(257, 4), (1, LDS4, 1, 16)),
    case('lds4-R1-J257', 1, ragged(257, 1), (1, LDS4, 1, 16)),
    case('lds8-R5-J70', 5, ragged(70, 5), (1, LDS8, 1, 64)),
    case('lds8-R6-J70', 6, ragged(70, 6), (1, LDS8, 1, 64)),
    case('lds8-R7-J70', 7, ragged(70, 7), (1, LDS8, 1, 64)),                 # ng = 1 with 49 live lanes
    case('lds8-R8-J70', 8, ragged(70, 8), (1, LDS8, 1, 64)),                 # R*R = 64: one wave in the dual kernel
    # in_lds: R*R*8 + Jmax*R*8 <= 48 KB; at R = 8 that is Jmax <= 760
    case('lds8-R8-J760', 8, [760, 70, 33], (1, LDS8, 1, 64)),
    case('lds8-R8-J761', 8, [761, 70, 33], (1, LDS8, 0, 64)),
    case('nolds-R8-J800', 8, [800, 71, 34], (1, LDS8, 0, 64)),
    case('nolds-R3-J2100', 3, [2100, 70, 35], (1, LDS4, 0, 16)),
    case('K1-R3', 3, [50], (1, REGS1, 1, 16)),
    case('K64-R3', 3, [20 + (7 * k) % 23 for k in range(64)], (1, REGS1, 1, 16)),
    case('K65-R3', 3, [20 + (7 * k) % 23 for k in range(65)], (1, REGS1, 1, 16)),
    case('K257-R3', 3, [61 + (7 * k) % 60 for k in range(257)], (1, REGS2, 1, 16)),
    case('K129-R6', 6, [12 + (5 * k) % 31 for k in range(129)], (1, LDS8, 1, 64)),
    case('rhoscale-R3', 3, ragged(100, 3), (1, REGS2, 1, 16), rho_scale=2.5),
]

FOUR_CASES = [
    # (no slab with J_k = R from here on: a square W_k under 5 % noise is close to singular at these ranks, and the polar
    # factor of such a slab has no digits to compare -- the two host formulations differ by 1e-10 there)
    case('four-R9', 9, tall(70, 9), (0, LDS16, 1, 0)),
    case('four-R16', 16, tall(70, 16), (0, LDS16, 1, 0)),
    case('four-R17', 17, tall(70, 17), (0, LDS64, 1, 0)),
    case('four-R48', 48, tall(150, 48), (0, LDS64, 0, 0)),
    case('four-R64', 64, tall(200, 64), (0, LDS64, 0, 0)),                   # 2*R*R*8 = 65 536 B of dynamic LDS
    case('four-R9-K300', 9, [61 + (7 * k) % 60 for k in range(300)], (0, LDS16, 1, 0)),
]

CONSTRAINED_CASES = [
    case('nn-regs1', 3, ragged(64, 3), (0, REGS1, 1, 0), NONNEG),
    case('nn-regs2', 3, ragged(128, 3), (0, REGS2, 1, 0), NONNEG),
    case('nn-regs4', 4, ragged(256, 4), (0, REGS4, 1, 0), NONNEG),
    case('nn-lds4', 4, ragged(257, 4), (0, LDS4, 1, 0), NONNEG),
    case('nn-lds8', 6, ragged(70, 6), (0, LDS8, 1, 0), NONNEG),
    case('nn-lds16', 9, tall(70, 9), (0, LDS16, 1, 0), NONNEG),
    case('unimodal-regs2', 3, ragged(100, 3), (0, REGS2, 1, 0), UNIMODAL),
    case('tpar2-K2', 3, [20, 20], (0, REGS1, 1, 0), TPAR2),
    case('tpar2-K64', 3, [20] * 64, (0, REGS1, 1, 0), TPAR2),
]


def _params(cases):
    return [pytest.param(c, id=c['id']) for c in cases]


@pytest.mark.parametrize('c', _params(FOLDED_CASES))
def test_folded_loop(eng, c):
    check_case(eng, c)


@pytest.mark.parametrize('c', _params(FOUR_CASES))
def test_four_launch_loop(eng, c):
    check_case(eng, c)


@pytest.mark.parametrize('c', _params(CONSTRAINED_CASES))
def test_four_launch_constrained_loop(eng, c):
    check_case(eng, c)


@pytest.mark.parametrize('J', [pytest.param([20] * 65, id='K65'), pytest.param([20, 21, 20], id='ragged')])
def test_tparafac2_refuses_what_it_cannot_run(eng, pkg, J):
    """More than 64 slabs, or slabs of different sizes: an error before anything runs, the state untouched."""
    c = case('tpar2-refused', 3, J, None, TPAR2)
    inp = make_inputs(c)
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.par2_b_loop(inp['J'], 3, inp['Ak'], inp['GA'], inp['C'], inp['w'], 1.0, TPAR2, 5, (0.0,) * 4, inp['P'],
                        inp['mu'], inp['DeltaB'], inp['Z'], inp['muZ'])
    assert not isinstance(ei.value, pkg.NotPositiveDefinite)
    assert 'tPARAFAC2' in str(ei.value)


# ---------------------------------------------------------------------------------------------------------------------
# loop control
# ---------------------------------------------------------------------------------------------------------------------
def _with(c, suffix, **kw):
    """The same inputs (the seed comes from the id before '|') under another loop setting."""
    d = dict(c)
    d.update(kw)
    d['id'] = c['id'] + '|' + suffix
    return d


_BY_ID = {c['id']: c for c in FOLDED_CASES + FOUR_CASES + CONSTRAINED_CASES}
PARITY_BASES = ['regs-R3-J128', 'lds8-R5-J70', 'nolds-R3-J2100', 'four-R9', 'nn-regs2']


@pytest.mark.parametrize('c', _params([_with(_BY_ID[b], 'inner%d' % n, inner=n) for b in PARITY_BASES for n in (1, 6)]))
def test_runs_to_max_inner(eng, c):
    """max_inner = 1 and 6 with tolerances 0 (5 is what every class case runs): an odd and an even count into
    par2_b_close_k, which swaps the DeltaB pair after an odd one."""
    check_case(eng, c, expect_iters=c['inner'])


def pick_exit(series):
    """Iterations k in 2..9 (1-based) whose residual is below 0.8 x the smallest earlier one -> [(k, tolerance)]; the
    tolerance is the geometric mean of the two, > 10 % away from both."""
    out = []
    for k in range(2, EXIT_INNER):
        lo = min(series[:k - 1])
        if 0 < series[k - 1] < 0.8 * lo:
            out.append((k, float(np.sqrt(series[k - 1] * lo))))
    return out


def assert_margin(hist, kstar, tol):
    """The reference stops at k*, and up to k* no residual comes within 10 % of a finite tolerance."""
    assert 1 < kstar < EXIT_INNER
    for k in range(1, kstar + 1):
        for q in range(4):
            if np.isfinite(tol[q]):
                assert abs(hist[q][k - 1] / tol[q] - 1.0) > 0.1, (
                    'residual %d = %.3e within 10 %% of the tolerance %.3e at iteration %d' % (q, hist[q][k - 1], tol[q], k))
        go = any(hist[q][k - 1] > tol[q] for q in range(4))
        assert go == (k < kstar)


def exit_case(eng, c, which, parity=None):
    c = _with(c, 'exit%d%s' % (which, parity or ''), inner=EXIT_INNER)
    _, loop, _ = reference(c)
    hist = loop.history(EXIT_INNER)
    picks = [p for p in pick_exit(hist[which]) if parity is None or p[0] % 2 == (1 if parity == 'odd' else 0)]
    assert picks, '%s no longer has such an exit iteration in 2..9 with the 0.8 gap: pick another input' % c['id']
    kstar, t = picks[len(picks) // 2]
    tol = tuple(t if q == which else INF for q in range(4))
    assert_margin(hist, kstar, tol)
    out, _ = check_case(eng, c, tol, expect_iters=kstar)
    last = loop.run(EXIT_INNER)                      # the state of iteration k*, not of iteration 10
    assert slab_dist(out['B'], last['B']) > 1e-6 or slab_dist(out['mu'], last['mu']) > 1e-6
    return kstar


EXIT_FOLDED = ['regs-R3-J128', 'regs-R4-J256', 'lds8-R5-J70', 'nolds-R3-J2100', 'K257-R3']


@pytest.mark.parametrize('base', EXIT_FOLDED)
@pytest.mark.parametrize('parity', ['odd', 'even'])
def test_folded_exit_primal_residual(eng, base, parity):
    """The while test rides at the head of the next slab kernel; after an odd count par2_b_close_k swaps the DeltaB pair,
    after an even one it must not."""
    k = exit_case(eng, _BY_ID[base], 0, parity)
    assert k % 2 == (1 if parity == 'odd' else 0)


@pytest.mark.parametrize('base', EXIT_FOLDED)
def test_folded_exit_dual_residual(eng, base):
    """Primal tolerance infinite: the dual coupling residual alone ends the loop."""
    exit_case(eng, _BY_ID[base], 2)


@pytest.mark.parametrize('base', ['four-R9', 'four-R17'])
@pytest.mark.parametrize('which', [0, 2], ids=['pc', 'dc'])
def test_four_launch_exit_unconstrained(eng, base, which):
    exit_case(eng, _BY_ID[base], which)


@pytest.mark.parametrize('base', ['nn-regs2', 'nn-lds16'])
@pytest.mark.parametrize('which', [0, 1, 2, 3], ids=['pc', 'pz', 'dc', 'dz'])
def test_four_launch_exit_each_residual(eng, base, which):
    """par2_b_finalize_k: each of the four residuals alone ends the constrained loop."""
    exit_case(eng, _BY_ID[base], which)


# ---------------------------------------------------------------------------------------------------------------------
# degenerate and exact inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_constraint_dual_takes_the_unscaled_residual(eng):
    """Non-negativity, muZ = 0 and B_k > 0 after the one iteration: Z_k = B_k, muZ stays exactly 0, ||muZ_k|| = 0 and
    the dual constraint residual is the unscaled ||Z_k - Zold_k|| (:572-577, the sc == 0 branch of par2_b_finalize_k)."""
    c = case('sc0', 3, ragged(100, 3), (0, REGS2, 1, 0), NONNEG, inner=1, kind='positive')
    _, loop, _ = reference(c)
    ref = loop.run(1)
    assert all((b > 0).all() for b in ref['B']) and all(not m.any() for m in ref['muZ'])
    out, _ = check_case(eng, c, expect_iters=1)
    assert all(not m.any() for m in out['muZ'])
    assert all(np.array_equal(z, b) for z, b in zip(out['Z'], out['B']))
    assert out['res'][1] == 0.0 and out['res'][3] > 0.1


@pytest.mark.parametrize('base', ['regs-R3-J128', 'four-R9', 'nn-lds8'])
def test_zero_row_of_C_is_not_positive_definite(eng, pkg, base):
    """C(k,:) = 0: C_k = 0, rho_k = 0, the slab's system is the zero matrix and chol fails (notpd of par2_b_system_k)."""
    c = _BY_ID[base]
    inp, _, _ = reference(c)
    Cm = inp['C'].copy()
    Cm[1, :] = 0.0
    with pytest.raises(pkg.NotPositiveDefinite):
        eng.par2_b_loop(inp['J'], inp['R'], inp['Ak'], inp['GA'], Cm, inp['w'], 1.0, inp['con'], 2, (0.0,) * 4, inp['P'],
                        inp['mu'], inp['DeltaB'], inp['Z'], inp['muZ'])


EXACT_CASES = [
    case('exact-folded', 3, [12, 13, 16, 70], (1, REGS2, 1, 16), inner=1, kind='exact'),
    case('exact-four', 9, [36, 40, 50, 37], (0, LDS16, 1, 0), inner=1, kind='exact'),
]


@pytest.mark.parametrize('c', _params(EXACT_CASES))
def test_exact_small_integers(eng, c):
    """Every intermediate of one iteration is an exactly representable number (see make_inputs): the device must return
    B_k, P_k, DeltaB, mu_k, rho_k, L_k and GB_k to the last bit.  A swapped index pair, a wrong row or a wrong slab
    offset cannot hide behind a tolerance here."""
    inp, _, _ = reference(c)
    R, J = inp['R'], inp['J']
    out = eng.par2_b_loop(J, R, inp['Ak'], inp['GA'], inp['C'], inp['w'], 1.0, None, 1, (0.0,) * 4, inp['P'], inp['mu'],
                          inp['DeltaB'])
    assert out['path'] == c['path']
    assert out['inner_iters'] == 1
    assert np.array_equal(out['rho'], np.full(len(J), 2.0))
    assert all(np.array_equal(Lk, 2.0 * np.eye(R)) for Lk in out['L'])
    for k, j in enumerate(J):
        B = (inp['Ak'][k] + inp['P'][k]) / 4.0
        assert np.array_equal(out['B'][k], B)
        assert np.array_equal(out['P'][k], np.where(B != 0, 0.5, 0.0))
        assert not out['mu'][k].any()
        assert np.array_equal(out['GB'][k], np.diag(4.0 * np.arange(1, R + 1) ** 2))
    assert np.array_equal(out['DeltaB'], np.diag(2.0 * np.arange(1, R + 1)))
    assert out['res'][0] == 0.0 and out['res'][2] == INF        # ||B_k - P_k DeltaB|| = 0 and ||mu_k|| = 0


@pytest.mark.parametrize('c', _params([
    case('asym-folded', 3, [12, 13, 16, 70], (1, REGS2, 1, 16), inner=2, kind='asym'),
    case('asym-lds8', 6, [12, 13, 16, 70], (1, LDS8, 1, 64), inner=2, kind='asym'),
    case('asym-four', 9, [36, 40, 50, 37], (0, LDS16, 1, 0), inner=2, kind='asym'),
]))
def test_asymmetric_small_integers(eng, c):
    """L_k lower bidiagonal and DeltaB upper bidiagonal, integer right-hand sides: an r/q swap in either changes the
    result at the first digit."""
    check_case(eng, c)
