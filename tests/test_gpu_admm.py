"""GPU: every kernel family of ADMM_constrained_only (cmtf_fun_AOADMM.m:591-623), run as the solver runs it
(`Engine.admm_mode` -> aoadmm_op_admm_mode: system from sys_build, kernels from admm_path), against a numpy fp64 loop.

Reference (`RefLoop`): rho = trace(C)/R, L = chol(C + rho/2 I), fac = (A_inner/L')/L, Z = prox(fac + mu, rho) from
oracle.prox, mu += fac - Z, residuals and while condition of eval_res_ADMM_constr / ADMM_constrained_only.

Every case asserts: the path code (so a retuned dispatch says "pick a new shape"), inner_iters, fac / Z / mu, the two
residuals (rtol 1e-9), the Gram matrix against the host fac'fac of the returned fac (1e-13) and the row-major copy
(bitwise).

Bar on fac, Z, mu: the solver-path kernels multiply by the explicit inverse inv(L L') where the reference solves with
the triangular factor.  The same difference exists between two host formulations, so each case also runs the numpy
loop with fac = A_inner @ inv(L L'); the relative Frobenius distance of the two host results is the case's floor and
its bar is max(1e-11, 10 x floor) -- 10 for a different summation order over at most 64 terms.  The bar is never
taken from the device.  Largest floor seen over the cases of this file: see LARGEST_FLOOR below.

Early exit: the exit iteration k* comes from the reference run with tolerances 0.  k* is an iteration 2..9 whose
residual lies below 0.8 x the smallest earlier one; the tolerance is the geometric mean of the two, so the decision
sits >= 10 % away from the threshold at every iteration (asserted, never skipped).  The device must stop at exactly
k* and leave the state of iteration k*.

Class -> case (ids as pytest prints them):
  admm_loop_wg_k   RMAX 4          wg-*-65x1, -65x4, -256x1, -256x4
                   RMAX 8          wg-*-65x5, -65x8, -256x5, -256x8, rows 1 / 63 / 64 / 255 at R 5
                   RMAX 16         wg-*-65x9, -65x16, -256x9, -256x16, every constraint at 255x9, every row count at R 16
                   column-norm     wg-l2-ball / non-negative l2-ball / non-negative l2-sphere / l2 regularization -255x9
                   thresholds      edge-257x16 (-> MFMA), edge-256x17 (-> MFMA), edge-l2-ball-257x9 (-> column prox)
  admm_rows_mfma_k KS 1            mfma-*-x1, x4        KS 2   x5, x8       KS 3   x9, x12     KS 4 (MT 1)  x13, x16
                   KS 5 (MT 2)     x17, x20             KS 6   x21, x24     KS 8   x25, x28 (padded), x29, x32
                   rows            257 / 271 (ragged tile), 272 (full), 2000 (headline 2000x20)
                   thresholds      thr-4096x8 (256 tiles, kSpecPartJ full), thr-3264x10, thr-2000x10, mfma-inner1
  admm_rows_k      CPW 1           rows-simplex-300x3 (not EXACT), rows-simplex-300x4 (EXACT), rows-*-70001x3
                   CPW 2           rows-simplex-300x8 (EXACT), col-*-x6 (not EXACT)
                   CPW 3 / 4       rows-simplex-300x9 / x13 (not EXACT), thr-4096x9 (R 12 EXACT) / thr-2000x11 (R 16 EXACT)
                   CPW 5 / 6 / 8   rows-simplex-300x17 / x21 / x29 (not EXACT), x20 / x24 / x32 (EXACT), col-*-x20 (CPW 5)
                   CPW 12          rows-non-negativity-300x33 / x36 (not EXACT), x48 (EXACT)
                   CPW 16          x49, x60 (not EXACT), x61 (dynamic LDS, not EXACT), x64 (EXACT, dynamic LDS)
                   grid-stride     rows-non-negativity-70001x3, rows-simplex row-wise-70001x3 (1024 blocks of 64 rows)
                   thresholds      thr-4096x9, thr-4112x5, thr-3280x10, thr-2000x11
  + column prox    col-<constraint>-300x6 / 300x20 / 4097x6 / 4097x20 (primal kernel, prox_apply, dual_update_k)
  + fused TV       tv-300 (256 threads), tv-1025 (1024 threads), tv-6400 (largest LDS form), tv-6401 (hybrid),
                   tv-12001 (workspace form)
  early exit       exit-du-* / exit-pr-* / exit-both-* on every path class
  degenerate       zero-* (A = Z = mu = 0: 0/0 primal residual), ident-* (mu = 0 throughout: unscaled dual residual)
"""
import functools
import zlib

import numpy as np
import pytest

from helpers import rel_fro
from oracle import aoadmm as OA
from oracle import prox as OP
from prox_ref import gl_banded as _gl_banded

pytestmark = pytest.mark.gpu

WG, MFMA, ROWS, COLPROX, TV, ROWL = range(6)          # AOADMM_PATH_* (include/aoadmm_hip.h)
PATH_NAME = ['one-workgroup', 'MFMA two-launch', 'admm_rows_k fused', 'admm_rows_k + column prox',
             'admm_rows_k + fused TV', 'admm_rowL_k']

# Largest distance between the two host formulations (triangular solve / explicit inverse) over every case of this
# file (host only, no device involved): 1.3e-14 (l1 regularization 256 x 16; 1.1e-14 at 300 x 60), so every case runs
# at the 1e-11 bar.
LARGEST_FLOOR = 1.3e-14


def _quad_L(rows, sym):
    rng = np.random.default_rng(1234 + rows)
    M = rng.standard_normal((rows, rows)) / np.sqrt(rows)
    return M.T @ M if sym else M.T @ M + 0.3 * np.triu(rng.standard_normal((rows, rows)), 1) / np.sqrt(rows)


# name -> constraint cell.  Parameters put the prox in its active regime for the inputs below (rho ~ 133,
# entries of fac + mu of order 1).
CONSTRAINTS = {
    'non-negativity': ('non-negativity',),
    'box': ('box', 0.1, 0.6),
    'l1 regularization': ('l1 regularization', 20.0),
    'l0 regularization': ('l0 regularization', 5.0),
    'ridge': ('ridge', 30.0),
    'simplex row-wise': ('simplex row-wise', 1.0),
    'l2-ball': ('l2-ball', 1.0),
    'non-negative l2-ball': ('non-negative l2-ball', 1.0),
    'non-negative l2-sphere': ('non-negative l2-sphere', 1),
    'l2 regularization': ('l2 regularization', 50.0),
    'simplex column-wise': ('simplex column-wise', 1.0),
    'l1-ball': ('l1-ball', 1.0),
    'non-decreasing': ('non-decreasing',),
    'unimodality': ('unimodality', True),
    'GL smoothness': ('GL smoothness', 50.0),
    'orthonormal': ('orthonormal',),
    'quadratic sym': ('quadratic regularization', 20.0, 'sym'),
    'quadratic nonsym': ('quadratic regularization', 20.0, 'nonsym'),
    'TV regularization': ('TV regularization', 5.0),
    'wide box': ('box', -1e3, 1e3),
}
# Seed changes (at most one per constraint): unimodality and l0 are discontinuous; a seed is kept only when the two
# host formulations agree (asserted in every case through the floor).  None was needed.
SEED_BUMP = {}


def constraint_cell(name, rows):
    c = CONSTRAINTS[name]
    if c[0] == 'quadratic regularization':
        return (c[0], c[1], _quad_L(rows, c[2] == 'sym'))
    return c


def host_prox(name, rows):
    """prox(x, rho) of oracle.prox.  Above 1000 rows two of them are restated, the same operations in a form that
    takes milliseconds instead of many seconds, each pinned to oracle.prox in test_fast_host_prox_is_the_oracle_prox:
    GL smoothness solves the same tridiagonal system (2 eta/rho L + I) x = v banded instead of dense; simplex row-wise
    runs the sort-based projection of oracle.prox._simplex_vec on all rows at once instead of row by row."""
    c = constraint_cell(name, rows)
    if c[0] == 'GL smoothness' and rows > 1000:
        return functools.partial(_gl_banded, eta=c[1])
    if c[0] == 'simplex row-wise' and rows > 1000:
        return functools.partial(_simplex_rows, eta=c[1])
    return OP.constraints_to_prox([1], [c], [rows])[0][0]


def _simplex_rows(x, rho, eta):
    n = x.shape[1]
    u = -np.sort(-x, axis=1)
    css = np.cumsum(u, axis=1) - eta
    cond = u - css / np.arange(1, n + 1) > 0
    last = n - 1 - np.argmax(cond[:, ::-1], axis=1)
    tau = css[np.arange(x.shape[0]), last] / (last + 1.0)
    return np.maximum(x - tau[:, None], 0.0)


def make_inputs(name, rows, R, kind='random'):
    """A standard normal; fac, Z, mu uniform; C = F'F with F uniform 400 x R; seed from the constraint name."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + SEED_BUMP.get(name, 0))
    F = rng.random((400, R))
    C = F.T @ F
    A = rng.standard_normal((rows, R))
    fac, Z, mu = rng.random((rows, R)), rng.random((rows, R)), rng.random((rows, R))
    if kind == 'zero':                               # ||fac|| = 0 after the first solve: primal residual 0/0
        A, Z, mu = np.zeros_like(A), np.zeros_like(Z), np.zeros_like(mu)
    elif kind == 'ident':                            # prox = identity on the data and mu = 0: mu stays exactly 0
        mu = np.zeros_like(mu)
    return A, C, fac, Z, mu


class RefLoop:
    """ADMM_constrained_only in numpy.  Iterates are computed once and kept, so that the runs with tolerances (early
    exit) walk the same `while` over the same states.  solve: 'chol' (the reference's triangular solves) or 'inv'
    (multiplication by inv(L L'), what the solver-path kernels do)."""

    def __init__(self, A, C, prox, fac, Z, mu, solve='chol'):
        R = C.shape[0]
        self.A, self.prox = A, prox
        self.rho = float(np.trace(C) / R)
        self.L = np.linalg.cholesky(C + self.rho / 2 * np.eye(R))
        self.Binv = np.linalg.inv(self.L @ self.L.T) if solve == 'inv' else None
        self.states = [(fac, Z, mu, np.inf, np.inf)]

    def _step(self):
        _, Z, mu, _, _ = self.states[-1]
        A_inner = self.A + self.rho / 2 * (Z - mu)                          # :608
        fac = A_inner @ self.Binv if self.Binv is not None else OA._solve_llt_right(A_inner, self.L)   # :609
        Zn = self.prox(fac + mu, self.rho)                                  # :1425
        mun = mu + fac - Zn                                                 # :1428
        with np.errstate(invalid='ignore', divide='ignore'):
            pr = OA._fro(fac - Zn) / OA._fro(fac)                           # :1085
        scaling = OA._fro(mun)
        d = OA._fro(Zn - Z)
        du = d / scaling if scaling > 0 else d                              # :1087-1092
        self.states.append((fac, Zn, mun, float(pr), float(du)))

    def run(self, max_inner, tol_pr=0.0, tol_du=0.0):
        it, pr, du = 0, np.inf, np.inf
        while it < max_inner and (pr > tol_pr or du > tol_du):              # :600
            it += 1
            if len(self.states) <= it:
                self._step()
            pr, du = self.states[it][3:]
        fac, Z, mu = self.states[it][:3]
        return dict(fac=fac, Z=Z, mu=mu, inner_iters=it, pr=pr, du=du)

    def history(self, max_inner):
        self.run(max_inner)
        return ([s[3] for s in self.states[1:max_inner + 1]], [s[4] for s in self.states[1:max_inner + 1]])


@functools.lru_cache(maxsize=None)
def reference(name, rows, R, kind='random'):
    """(inputs, triangular-solve loop, explicit-inverse loop) of a case; computed once, shared, never modified."""
    A, C, fac, Z, mu = make_inputs(name, rows, R, kind)
    for x in (A, C, fac, Z, mu):
        x.setflags(write=False)
    prox = host_prox(name, rows)
    return (A, C, fac, Z, mu), RefLoop(A, C, prox, fac, Z, mu, 'chol'), RefLoop(A, C, prox, fac, Z, mu, 'inv')


def floor_of(ref, alt):
    return max(rel_fro(alt[k], ref[k]) for k in ('fac', 'Z', 'mu'))


def _res_close(dev, ref):
    if np.isnan(ref):
        return bool(np.isnan(dev))
    return abs(dev - ref) <= 1e-9 * abs(ref)


def check_case(eng, name, rows, R, max_inner, path, tol_pr=0.0, tol_du=0.0, kind='random', expect_iters=None):
    (A, C, fac, Z, mu), loop, loop_inv = reference(name, rows, R, kind)
    ref = loop.run(max_inner, tol_pr, tol_du)
    alt = loop_inv.run(max_inner, tol_pr, tol_du)
    assert alt['inner_iters'] == ref['inner_iters'], 'the two host formulations stop at different iterations'
    floor = floor_of(ref, alt)
    assert floor < 1e-9, ('the two host formulations differ by %.2e: the input sits on a tie of a discontinuous prox; '
                          'change the seed of %r (one change per constraint)' % (floor, name))
    bar = max(1e-11, 10 * floor)
    if expect_iters is not None:
        assert ref['inner_iters'] == expect_iters
    out = eng.admm_mode(A, C, constraint_cell(name, rows), fac, Z, mu, max_inner, tol_pr, tol_du)
    errs = {k: rel_fro(out[k], ref[k]) for k in ('fac', 'Z', 'mu')}
    print('%s %dx%d inner %d: path %d its %d/%d floor %.2e bar %.2e fac %.2e Z %.2e mu %.2e pr %.15e/%.15e du %.15e/%.15e'
          % (name, rows, R, max_inner, out['path'], out['inner_iters'], ref['inner_iters'], floor, bar, errs['fac'],
             errs['Z'], errs['mu'], out['pr'], ref['pr'], out['du'], ref['du']))
    assert out['path'] == path, ('dispatch runs %s here, the case is meant for %s: pick a new shape'
                                 % (PATH_NAME[out['path']], PATH_NAME[path]))
    assert out['inner_iters'] == ref['inner_iters']
    for k in ('fac', 'Z', 'mu'):
        assert errs[k] < bar, (k, errs[k], bar)
    assert _res_close(out['pr'], ref['pr']), (out['pr'], ref['pr'])
    assert _res_close(out['du'], ref['du']), (out['du'], ref['du'])
    G = out['fac'].T @ out['fac']
    assert np.linalg.norm(out['gram'] - G) <= 1e-13 * np.linalg.norm(G), rel_fro(out['gram'], G)
    assert np.array_equal(out['facT'], out['fac']), 'row-major copy differs from the factor'
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rank and row classes, tolerances 0
# ---------------------------------------------------------------------------------------------------------------------
ELEMENTWISE = ['non-negativity', 'box', 'l1 regularization', 'l0 regularization', 'ridge']
COLNORM = ['l2-ball', 'non-negative l2-ball', 'non-negative l2-sphere', 'l2 regularization']
WG_CONSTRAINTS = ELEMENTWISE + ['simplex row-wise'] + COLNORM
COLUMN_PROX = ['l2-ball', 'non-negative l2-sphere', 'simplex column-wise', 'l1-ball', 'non-decreasing', 'unimodality',
               'GL smoothness', 'orthonormal']


def _cid(prefix, name, rows, R):
    return '%s-%s-%dx%d' % (prefix, name, rows, R)


def _wg_cases():
    cases = []
    for i, R in enumerate([1, 4, 5, 8, 9, 16]):                # every R at rows 65 and 256
        cases += [(WG_CONSTRAINTS[i % 10], 65, R), (WG_CONSTRAINTS[(i + 6) % 10], 256, R)]
    for i, rows in enumerate([1, 63, 64, 65, 255, 256]):       # every row count at R 5 and 16
        cases += [(WG_CONSTRAINTS[(i + 2) % 10], rows, 5), (WG_CONSTRAINTS[(i + 7) % 10], rows, 16)]
    cases += [(c, 255, 9) for c in WG_CONSTRAINTS]             # every constraint at (255, 9)
    cases += [('non-negativity', 256, 1), ('non-negativity', 256, 4), ('simplex row-wise', 65, 4), ('simplex row-wise', 256, 16)]
    # (no simplex at R = 1: every row projects to eta, the primal residual is rounding noise and has no digits to compare)
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(pytest.param(*c, id=_cid('wg', *c)))
    return out


@pytest.mark.parametrize('name,rows,R', _wg_cases())
def test_one_workgroup_loop(eng, name, rows, R):
    check_case(eng, name, rows, R, 5, WG)


@pytest.mark.parametrize('name,rows,R,path', [
    pytest.param('non-negativity', 257, 16, MFMA, id='edge-257x16'),
    pytest.param('box', 256, 17, MFMA, id='edge-256x17'),
    pytest.param('l2-ball', 257, 9, COLPROX, id='edge-l2-ball-257x9'),
    pytest.param('simplex row-wise', 257, 16, ROWS, id='edge-simplex-257x16'),
    pytest.param('l2 regularization', 256, 17, COLPROX, id='edge-l2reg-256x17'),
])
def test_one_workgroup_threshold(eng, name, rows, R, path):
    """kWgLoopRows = 256 and R <= 16: one row or one column more takes another family."""
    check_case(eng, name, rows, R, 5, path)


MFMA_RANKS = [1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32]
MFMA_ROWS = [257, 271, 272, 2000]


def _mfma_cases():
    cases = []
    for i, R in enumerate(MFMA_RANKS):                         # every rank at a ragged and at a full last tile
        cases += [(ELEMENTWISE[i % 5], 271, R), (ELEMENTWISE[(i + 2) % 5], 272, R)]
    for i, R in enumerate([1, 13, 20, 28, 32]):                # one rank per MT / padding class at 257 and 2000 rows
        cases += [(ELEMENTWISE[(i + 1) % 5], 257, R), (ELEMENTWISE[(i + 3) % 5], 2000, R)]
    cases += [(c, 2000, 20) for c in ELEMENTWISE]              # every constraint at the headline shape
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(pytest.param(*c, id=_cid('mfma', *c)))
    return out


@pytest.mark.parametrize('name,rows,R', _mfma_cases())
def test_mfma_two_launch_loop(eng, name, rows, R):
    check_case(eng, name, rows, R, 5, MFMA)


@pytest.mark.parametrize('rows,R,max_inner,path', [
    pytest.param(4096, 8, 8, MFMA, id='thr-4096x8'),           # 256 tiles x 8 = all 2 * kMaxParts slots, kSpecPartJ full
    pytest.param(4096, 12, 9, ROWS, id='thr-4096x9'),          # 256 x 9 slots do not fit
    pytest.param(4112, 8, 5, ROWS, id='thr-4112x5'),           # 257 tiles > 64 * kSpecPartJ
    pytest.param(3264, 20, 10, MFMA, id='thr-3264x10'),        # 204 tiles x 10 = 2040 <= 2048
    pytest.param(3280, 20, 10, ROWS, id='thr-3280x10'),        # 205 x 10 = 2050
    pytest.param(2000, 20, 10, MFMA, id='thr-2000x10'),        # kSpecMaxInner
    pytest.param(2000, 16, 11, ROWS, id='thr-2000x11'),
    pytest.param(271, 20, 1, MFMA, id='mfma-inner1'),          # max_inner = 1: the clamped itc loads of pass 2
    pytest.param(2000, 32, 5, MFMA, id='thr-2000xR32'),
    pytest.param(300, 33, 5, ROWS, id='thr-300xR33'),          # R <= 32
])
def test_mfma_dispatch_thresholds(eng, rows, R, max_inner, path):
    """admm_path: tiles <= 64 * kSpecPartJ, max_inner <= kSpecMaxInner, max_inner * tiles <= 2 * kMaxParts, R <= 32."""
    check_case(eng, 'non-negativity', rows, R, max_inner, path)


@pytest.mark.parametrize('name,rows,R', [pytest.param('non-negativity', 300, R, id=_cid('rows', 'non-negativity', 300, R))
                                         for R in (33, 36, 48, 49, 60, 61, 64)] +
                         [pytest.param('simplex row-wise', 300, R, id=_cid('rows', 'simplex', 300, R))
                          for R in (3, 4, 8, 9, 13, 17, 20, 21, 24, 29, 32)] +
                         [pytest.param(c, 70001, 3, id=_cid('rows', c, 70001, 3))
                          for c in ('non-negativity', 'simplex row-wise')])
def test_rows_fused_loop(eng, name, rows, R):
    """admm_rows_k with the prox inside: CPW classes, EXACT and not, dynamic LDS at R = 61..64, and at 70 001 rows the
    grid-stride loop with the grid clamped to kMaxParts blocks."""
    check_case(eng, name, rows, R, 5, ROWS)


def _colprox_cases():
    # (the python isotonic regression of the unimodal projection takes ~1 s per 4097 x 20 call: R = 6 only there)
    cases = [(c, rows, R) for c in COLUMN_PROX for rows in (300, 4097) for R in (6, 20)
             if (c, rows, R) != ('unimodality', 4097, 20)]
    cases += [(c, 300, R) for c in ('quadratic sym', 'quadratic nonsym') for R in (6, 20)]
    return [pytest.param(*c, id=_cid('col', *c)) for c in cases]


@pytest.mark.parametrize('name,rows,R', _colprox_cases())
def test_rows_column_prox_loop(eng, name, rows, R):
    check_case(eng, name, rows, R, 5, COLPROX)


@pytest.mark.parametrize('rows', [300, 1025, 6400, 6401, 12001])
def test_rows_fused_tv_loop(eng, rows):
    """256-thread, 1024-thread, largest LDS-resident, hybrid and workspace forms of the TV prox, each warm-started from
    Z and with the dual update inside."""
    check_case(eng, 'TV regularization', rows, 3, 5, TV)


# ---------------------------------------------------------------------------------------------------------------------
# early exit
# ---------------------------------------------------------------------------------------------------------------------
EXIT_INNER = 10


def pick_exit(series):
    """Iterations k in 2..9 (1-based) whose residual is below 0.8 x the smallest earlier one -> [(k, tolerance)]; the
    tolerance is the geometric mean of the two, > 10 % away from both."""
    out = []
    for k in range(2, EXIT_INNER):
        lo = min(series[:k - 1])
        if series[k - 1] < 0.8 * lo and series[k - 1] > 0:
            out.append((k, float(np.sqrt(series[k - 1] * lo))))
    return out


def assert_margin(pr, du, kstar, tol_pr, tol_du):
    """The loop stops at k* and at no iteration up to k* does a residual come within 10 % of a finite tolerance."""
    assert 1 < kstar < EXIT_INNER
    for k in range(1, kstar + 1):
        for v, tol in ((pr[k - 1], tol_pr), (du[k - 1], tol_du)):
            if np.isfinite(tol):
                assert abs(v / tol - 1.0) > 0.1, ('residual %.3e within 10 %% of the tolerance %.3e at iteration %d' % (v, tol, k))
        go = pr[k - 1] > tol_pr or du[k - 1] > tol_du
        assert go == (k < kstar)


def exit_case(eng, name, rows, R, path, which):
    _, loop, _ = reference(name, rows, R)
    pr, du = loop.history(EXIT_INNER)
    picks = pick_exit(du if which == 'du' else pr)
    assert picks, ('%s %dx%d no longer has a %s-driven exit iteration in 2..9 with the 0.8 gap: pick another input'
                   % (name, rows, R, which))
    kstar, tol = picks[len(picks) // 2]
    tol_pr, tol_du = (np.inf, tol) if which == 'du' else (tol, np.inf)
    assert_margin(pr, du, kstar, tol_pr, tol_du)
    out = check_case(eng, name, rows, R, EXIT_INNER, path, tol_pr, tol_du, expect_iters=kstar)
    # the state of iteration k*, not of iteration 10
    last = loop.run(EXIT_INNER)
    assert rel_fro(out['fac'], last['fac']) > 1e-6 or rel_fro(out['mu'], last['mu']) > 1e-6


EXIT_SHAPES = ([('non-negativity', 255, 9, WG), ('l2-ball', 255, 9, WG), ('simplex row-wise', 64, 5, WG),
                ('l1 regularization', 271, 13, MFMA), ('non-negativity', 2000, 20, MFMA), ('box', 3264, 8, MFMA),
                ('non-negativity', 300, 33, ROWS), ('simplex row-wise', 300, 8, ROWS), ('non-negativity', 70001, 3, ROWS),
                ('simplex row-wise', 70001, 3, ROWS)] +
               [(c, 300, 6, COLPROX) for c in COLUMN_PROX + ['quadratic sym', 'quadratic nonsym']] +
               [('l2-ball', 4097, 20, COLPROX), ('non-decreasing', 4097, 6, COLPROX),
                ('TV regularization', 300, 3, TV), ('TV regularization', 1025, 3, TV), ('TV regularization', 6401, 3, TV),
                ('TV regularization', 12001, 3, TV)])


@pytest.mark.parametrize('name,rows,R,path', [pytest.param(*c, id=_cid('exit-du', *c[:3])) for c in EXIT_SHAPES])
def test_early_exit_dual_residual(eng, name, rows, R, path):
    exit_case(eng, name, rows, R, path, 'du')


# the inputs that have a primal-residual-driven k* (found on the CPU; the simplex, l1-ball and orthonormal families
# have none: their primal residual does not fall by 20 % within 9 iterations)
EXIT_PR_SHAPES = ([('ridge', 255, 9, WG), ('non-negativity', 255, 9, WG), ('l2-ball', 255, 9, WG), ('l2 regularization', 255, 9, WG),
                   ('ridge', 271, 13, MFMA), ('l1 regularization', 271, 13, MFMA), ('non-negativity', 2000, 20, MFMA),
                   ('ridge', 300, 33, ROWS), ('non-negativity', 300, 33, ROWS), ('simplex row-wise', 70001, 3, ROWS)] +
                  [(c, 300, 6, COLPROX) for c in ('l2-ball', 'non-negative l2-sphere', 'non-decreasing', 'unimodality',
                                                  'GL smoothness', 'quadratic sym', 'quadratic nonsym')] +
                  [('TV regularization', 300, 3, TV), ('TV regularization', 6401, 3, TV)])


@pytest.mark.parametrize('name,rows,R,path', [pytest.param(*c, id=_cid('exit-pr', *c[:3])) for c in EXIT_PR_SHAPES])
def test_early_exit_primal_residual(eng, name, rows, R, path):
    exit_case(eng, name, rows, R, path, 'pr')


EXIT_BOTH_SHAPES = [('ridge', 255, 9, WG), ('ridge', 271, 13, MFMA), ('ridge', 300, 33, ROWS), ('GL smoothness', 300, 6, COLPROX),
                    ('quadratic nonsym', 300, 6, COLPROX)]


@pytest.mark.parametrize('name,rows,R,path', [pytest.param(*c, id=_cid('exit-both', *c[:3])) for c in EXIT_BOTH_SHAPES])
def test_early_exit_both_criteria(eng, name, rows, R, path):
    """Both tolerances finite, the two criteria first met at different iterations: the loop stops at the later one."""
    _, loop, _ = reference(name, rows, R)
    pr, du = loop.history(EXIT_INNER)
    pp, pd = pick_exit(pr), pick_exit(du)
    pairs = [(a, b) for a in pp for b in pd if a[0] != b[0]]
    assert pairs, 'no pair of exit iterations that differ: pick another input'
    (kp, tol_pr), (kd, tol_du) = pairs[len(pairs) // 2]
    first = [min(k for k in range(1, EXIT_INNER + 1) if s[k - 1] <= t) for s, t in ((pr, tol_pr), (du, tol_du))]
    assert first == [kp, kd] and kp != kd
    # the loop ends at the first iteration where both hold
    kstar = min(k for k in range(1, EXIT_INNER + 1) if pr[k - 1] <= tol_pr and du[k - 1] <= tol_du)
    assert kstar >= max(kp, kd)
    assert_margin(pr, du, kstar, tol_pr, tol_du)
    check_case(eng, name, rows, R, EXIT_INNER, path, tol_pr, tol_du, expect_iters=kstar)


# ---------------------------------------------------------------------------------------------------------------------
# degenerate inputs
# ---------------------------------------------------------------------------------------------------------------------
DEGENERATE_SHAPES = [(37, 5, WG), (271, 13, MFMA), (300, 33, ROWS), (300, 6, COLPROX)]


@pytest.mark.parametrize('rows,R,path', [pytest.param(*c, id='zero-%dx%d' % c[:2]) for c in DEGENERATE_SHAPES])
def test_zero_input_stops_where_the_reference_stops(eng, rows, R, path):
    """A = 0, Z = mu = 0: fac = 0, the primal residual is 0/0 = NaN, the dual residual 0; `NaN > tol` is false, so the
    reference leaves the loop after one iteration whatever the tolerances."""
    name = 'l2-ball' if path == COLPROX else 'non-negativity'
    out = check_case(eng, name, rows, R, 5, path, kind='zero', expect_iters=1)
    assert np.isnan(out['pr']) and out['du'] == 0.0
    assert not out['fac'].any() and not out['Z'].any() and not out['mu'].any()


@pytest.mark.parametrize('rows,R,path', [pytest.param(*c, id='ident-%dx%d' % c[:2]) for c in DEGENERATE_SHAPES[:3]])
def test_zero_dual_variable_takes_the_unscaled_dual_residual(eng, rows, R, path):
    """mu = 0 and a box wider than the data: Z = fac, mu stays exactly 0, so ||mu|| = 0 and the dual residual is the
    unscaled ||Z - Zold|| (eval_res_ADMM_constr :1087-1092); the primal residual is exactly 0."""
    out = check_case(eng, 'wide box', rows, R, 5, path, kind='ident', expect_iters=5)
    assert not out['mu'].any() and out['pr'] == 0.0 and out['du'] > 0.0


def test_fast_host_prox_is_the_oracle_prox():
    """The restated host prox of the long cases (host_prox) against oracle.prox: bitwise for the row simplex (the same
    operations in the same order per row), 1e-13 for the banded solve."""
    x = np.random.default_rng(3).standard_normal((1001, 4))
    c = CONSTRAINTS['GL smoothness']
    dense = OP.constraints_to_prox([1], [c], [1001])[0][0](x, 133.0)
    assert rel_fro(_gl_banded(x, 133.0, c[1]), dense) < 1e-13
    for R in (1, 3, 7):
        y = np.random.default_rng(R).standard_normal((500, R))
        assert np.array_equal(_simplex_rows(y, 133.0, 1.0), OP.project_simplex(y, 1.0, 2))
