"""GPU: the fold-in of new slabs into a fitted PARAFAC2 block (Engine.par2_fold_in) against the
numpy restatement of tests/par2_foldin_ref.py.

Exact: integer data make Y = X'A, ||X||^2 and S exact in fp64 whatever the order of summation, so the Y pass (every
rank class, chunked or not), the norm and the shared system are compared with array_equal.
Rows: the bar rule of tests/test_gpu_admm.py and tests/test_gpu_foldin.py: the device against the longdouble restatement
within max(1e-11, 10 x floor), floor = the distance of the fp64 restatement from the longdouble one.  The rule holds on
well-conditioned inputs only, so the numpy side first asserts sigma_min(W) / sigma_max(W) >= 1e-3 at every iteration and
cond(S + ridge I) <= 1e6."""
import copy
import ctypes as C
import importlib
import itertools
import threading

import numpy as np
import pytest

import par2_foldin_ref as PR
from helpers import options, script4_model
from oracle import aoadmm as OA

pytestmark = pytest.mark.gpu
capi = importlib.import_module('matlab-code_amd._capi')
LD = PR.LD
CHUNK = 4096                                                  # rows of I per chunk of the Y pass (par2_foldin.h)
LDS_DOUBLES = 48 * 1024 // 8                                  # the budget of the alternation's LDS class
_keys = itertools.count(7000)


def path_rule(I, R, Jmax):
    """(Y class, alternation class) as include/aoadmm_hip.h documents them."""
    T = (R + 15) // 16
    return 2 * (T - 1) + (1 if I > CHUNK else 0), 0 if R * R + 2 * Jmax * R <= LDS_DOUBLES else 1


def par2_Z(I, R, Jk, slabs=None):
    K = len(Jk)
    X = slabs if slabs is not None else [np.zeros((I, j)) for j in Jk]
    return dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=[I, list(Jk), K],
                coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
                constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[X], _ranks=[R] * 3)


def state_block(pkg, eng, A, DB, Z=None, miss=None):
    """A PARAFAC2 block that holds state only: A and DeltaB are what the call reads; B_k, P_k, C and the data are zeros
    unless a Z with data is given."""
    I, R = A.shape
    if Z is None:
        Z = par2_Z(I, R, [R, R + 1])
    if miss is not None:
        Z = dict(Z, miss=[miss])
    Jk = Z['size'][1]
    pkg.build_model(eng, Z)
    cells = [np.zeros((j, R)) for j in Jk]
    pkg.upload_state(eng, Z, {'fac': [A, cells, np.ones((len(Jk), R))], 'DeltaB': {0: DB}, 'P': {0: cells}, 'mu_DeltaB': {0: cells}})
    return Z


def same_out(a, b, keys=('C', 'res', 'xnorm', 'iters', 'info')):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ('B', 'P', 'Y'):
        if a.get(k) is not None and b.get(k) is not None:
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[k], b[k])), k


# ---- 1. exact -------------------------------------------------------------------------------------------------------
RS = [1, 3, 4, 5, 16, 17, 20, 32, 33, 48, 49, 64]
IS = [1, 3, 4, 5, 63, 64, 65, 257, CHUNK, CHUNK + 1]
NKS = [1, 2, 7, 40]


def _exact_combos():
    out = [(RS[i % 12], IS[(7 * i + 3) % 10], NKS[(3 * i + 1) % 4], i) for i in range(36)]
    # both sides of the chunking threshold at every tile count
    out += [(R, I, nk, 100 + n) for n, (R, I, nk) in enumerate(
        [(5, CHUNK, 2), (5, CHUNK + 1, 2), (20, CHUNK, 1), (20, CHUNK + 1, 2), (33, CHUNK, 1), (33, CHUNK + 1, 1), (64, CHUNK, 1),
         (64, CHUNK + 1, 1)])]
    return out


def _exact_cols(R, nk, seed):
    cand = [j for j in (R, R + 1, 15, 16, 17, 33, 64, 65, 130) if j >= R]
    return [cand[(seed + 2 * q) % len(cand)] if q else cand[seed % len(cand)] for q in range(nk)]


EXACT = _exact_combos()


def test_exact_combinations_touch_every_value_and_class():
    assert {c[0] for c in EXACT} == set(RS) and {c[1] for c in EXACT} == set(IS) and {c[2] for c in EXACT} == set(NKS)
    cols = set()
    classes = set()
    for R, I, nk, seed in EXACT:
        J = _exact_cols(R, nk, seed)
        cols |= {('R' if j == R else 'R+1' if j == R + 1 else j) for j in J}
        classes.add(path_rule(I, R, max(J)))
    assert cols >= {'R', 'R+1', 15, 16, 17, 33, 64, 65, 130}, cols
    assert {c[0] for c in classes} == set(range(8)) and {c[1] for c in classes} == {0, 1}, classes


@pytest.mark.parametrize('R,I,nk,seed', EXACT, ids=['R%d-I%d-nk%d-%d' % c for c in EXACT])
def test_exact_y_norm_and_system(pkg, eng, R, I, nk, seed):
    rng = np.random.default_rng(50000 + seed)
    A = rng.integers(-3, 4, (I, R)).astype(np.float64)
    DB = rng.integers(-2, 3, (R, R)).astype(np.float64)
    J = _exact_cols(R, nk, seed)
    slabs = [rng.integers(-5, 6, (I, j)).astype(np.float64) for j in J]
    state_block(pkg, eng, A, DB)
    # ridge 1: S is an exact positive semidefinite integer matrix (singular when I < R), S + I has a factor
    out = eng.par2_fold_in(0, slabs, max_iter=1, ridge=1.0, return_y=True, return_sys=True)
    assert out['path'] == path_rule(I, R, max(J))
    for q, X in enumerate(slabs):
        assert np.array_equal(out['Y'][q], X.T @ A), q
    assert np.array_equal(out['xnorm'], np.array([np.sum(X * X) for X in slabs]))
    assert np.array_equal(out['sys'], (A.T @ A) * (DB.T @ DB))
    assert np.all(out['iters'] == 1)


# ---- 2. rows, real values -------------------------------------------------------------------------------------------
SHAPES = [(1, 5, 1), (3, 40, 61), (4, 17, 4), (5, 33, 9), (8, 40, 120), (16, 70, 40), (17, 70, 17), (20, 90, 65), (33, 140, 70),
          (64, 260, 64)]
# one J on each side of the LDS / workspace switch: R^2 + 2 J R <= 6144
SWITCH = {4: (766, 767), 20: (143, 144)}
VARIANTS = [('ls', False, 5), ('nn1', True, 1), ('nn5', True, 5)]
_models, _refs = {}, {}


def row_model(R):
    if R not in _models:
        I = [s for s in SHAPES if s[0] == R][0][1]
        Js = [s[2] for s in SHAPES if s[0] == R] + list(SWITCH.get(R, ()))
        rngA = np.random.default_rng(1000 * R)
        A, DB = PR.make_model(rngA, R, I)
        slabs = [PR.make_slab(np.random.default_rng(1000 * R + J), A, DB, J)[0] for J in Js]
        assert np.linalg.cond(PR.system(A, DB)) <= 1e6
        _models[R] = (A, DB, slabs)
    return _models[R]


def row_refs(R, max_iter, nonneg, max_inner):
    key = (R, max_iter, nonneg, max_inner)
    if key not in _refs:
        A, DB, slabs = row_model(R)
        kw = dict(max_iter=max_iter, tol=0.0, nonneg=nonneg, max_inner=max_inner)
        f64 = [PR.fold_in_slab(A, DB, X, trace=True, **kw) for X in slabs]
        ld = [PR.fold_in_slab(A, DB, X, dtype=LD, **kw) for X in slabs]
        for o in f64:
            assert min(o['conds']) >= 1e-3, o['conds']
        _refs[key] = (f64, ld)
    return _refs[key]


def distances(got, ld):
    """(c, B, P, res) distances of one slab's outputs from the longdouble ones, in the measures of the bar rule."""
    c, B, P = (np.asarray(got[k], dtype=LD) for k in ('c', 'B', 'P'))
    return (float(np.max(np.abs(c - ld['c'])) / np.max(np.abs(ld['c']))), float(np.max(np.abs(B - ld['B'])) / np.max(np.abs(ld['B']))),
            float(np.max(np.abs(P - ld['P']))), float(abs(LD(got['res']) - ld['res']) / ld['xnorm']))


@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('long', [False, True], ids=['it1', 'itN'])
@pytest.mark.parametrize('R', [s[0] for s in SHAPES])
def test_rows_against_longdouble(pkg, eng, R, long, variant):
    _, nonneg, max_inner = variant
    max_iter = 1 if not long else (2 if R >= 48 else 5)
    A, DB, slabs = row_model(R)
    f64, ld = row_refs(R, max_iter, nonneg, max_inner)
    state_block(pkg, eng, A, DB)
    calls = [slabs] if R not in SWITCH else [slabs[:-1], slabs]   # without and with the slab beyond the LDS budget
    worst = np.zeros(4)
    for call in calls:
        out = eng.par2_fold_in(0, call, max_iter=max_iter, tol=0.0, nonneg=nonneg, max_inner=max_inner, return_P=True)
        assert out['path'] == path_rule(A.shape[0], R, max(X.shape[1] for X in call))
        assert np.all(out['info'] == 0)
        for q in range(len(call)):
            # tol = 0 runs max_iter iterations unless c repeats to the bit: at R = 1 it does (P = sign(W), c is a fixed
            # point after the first iteration), in the restatement as on the device
            assert out['iters'][q] == f64[q]['iters'] and (R == 1 or out['iters'][q] == max_iter), (q, out['iters'][q])
            got = dict(c=out['C'][q], B=out['B'][q], P=out['P'][q], res=out['res'][q])
            dev, floor = distances(got, ld[q]), distances(f64[q], ld[q])
            worst = np.maximum(worst, dev)
            for name, d, f in zip(('c', 'B', 'P', 'res'), dev, floor):
                assert d <= max(1e-11, 10 * f), (R, q, name, d, f)
            assert abs(out['xnorm'][q] - float(ld[q]['xnorm'])) <= 1e-13 * out['xnorm'][q]
    if R in SWITCH:                                               # the two alternation classes give the same bits
        a = eng.par2_fold_in(0, slabs[:-1], max_iter=max_iter, tol=0.0, nonneg=nonneg, max_inner=max_inner, return_P=True)
        b = eng.par2_fold_in(0, slabs, max_iter=max_iter, tol=0.0, nonneg=nonneg, max_inner=max_inner, return_P=True)
        assert a['path'][1] == 0 and b['path'][1] == 1
        same_out(a, {k: (v[:-1] if isinstance(v, (list, np.ndarray)) else v) for k, v in b.items()})
    print('par2_fold_in R=%d max_iter=%d %s: worst device error c %.2e B %.2e P %.2e res %.2e' % ((R, max_iter, variant[0]) + tuple(worst)))


# ---- 3. early exit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nonneg', [False, True], ids=['ls', 'nonneg'])
@pytest.mark.parametrize('R', [3, 8, 20])
def test_early_exit(pkg, eng, R, nonneg):
    A, DB, slabs = row_model(R)
    state_block(pkg, eng, A, DB)
    out = eng.par2_fold_in(0, slabs, max_iter=50, tol=1e-6, nonneg=nonneg)
    for q, X in enumerate(slabs):
        ref = PR.fold_in_slab(A, DB, X, max_iter=50, tol=1e-6, nonneg=nonneg, trace=True)
        assert 1 < ref['iters'] < 50
        assert abs(int(out['iters'][q]) - ref['iters']) <= 1, (q, out['iters'][q], ref['iters'])
        last_move = np.linalg.norm(ref['cs'][-1] - ref['cs'][-2])
        assert np.linalg.norm(out['C'][q] - ref['c']) <= last_move, q


# ---- 4. known answer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,J', [(3, 61), (20, 65)])
def test_known_answer_on_the_device(pkg, eng, R, J):
    I = 40 if R == 3 else 90
    rng = np.random.default_rng(1000 * R + J)
    A, DB = PR.make_model(rng, R, I)
    X, c, P = PR.make_slab(rng, A, DB, J, noise=0.0)
    state_block(pkg, eng, A, DB)
    for nonneg in (False, True):
        out = eng.par2_fold_in(0, [X], max_iter=300, tol=1e-14, nonneg=nonneg, max_inner=500 if nonneg else 5, return_P=True)
        assert np.max(np.abs(out['C'][0] - c)) <= 1e-9, (nonneg, out['iters'])
        assert out['fit'][0] >= 1 - 1e-10


# ---- 5. end to end --------------------------------------------------------------------------------------------------
def test_end_to_end_fit_then_fold_in(pkg):
    """A script-4-shaped block (I = 40, R = 3, J_k from 61..120) fitted on K - 3 noise-free slabs of a common truth, then the
    other three folded in under non-negativity.  First the restatement on the ORACLE's factors: it explains the held-out
    slabs (fit >= 0.999; measured on the CPU: the oracle's objective after 150 outer iterations is 1.1e-6 of the data and the
    three held-out fits are 0.999974 .. 0.999999).  Then the engine's fit against the restatement on the
    engine's own A and DeltaB under the bar rule."""
    rng = np.random.default_rng(4)
    K, R = 12, 3
    Zall, io = script4_model(rng, K=K, noise=0.0)
    Xall, Jall = Zall['object'][0], Zall['size'][1]
    Z = dict(Zall, size=[40, Jall[:K - 3], K - 3], object=[Xall[:K - 3]])
    new = Xall[K - 3:]
    opt = options(MaxOuterIters=150)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(5))
    _, Fo, _, _ = OA.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G))
    kw = dict(max_iter=50, tol=1e-10, nonneg=True, max_inner=50)
    for X in new:
        o = PR.fold_in_slab(Fo['fac'][0], Fo['DeltaB'][0], X, **kw)
        assert 1 - float(o['res'] / o['xnorm']) >= 0.999
    with pkg.Engine(0) as eng:
        _, Fg, _, _ = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=eng)
        out = eng.par2_fold_in(0, new, **kw)
    for q, X in enumerate(new):
        f64 = PR.fold_in_slab(Fg['fac'][0], Fg['DeltaB'][0], X, **kw)
        ld = PR.fold_in_slab(Fg['fac'][0], Fg['DeltaB'][0], X, dtype=LD, **kw)
        fit_ld = 1 - ld['res'] / ld['xnorm']
        floor = abs(float((1 - f64['res'] / f64['xnorm']) - fit_ld))
        assert abs(float(LD(out['fit'][q]) - fit_ld)) <= max(1e-11, 10 * floor), (q, out['fit'][q], float(fit_ld), floor)
        assert np.all(out['C'][q] >= 0)


# ---- 6. bits --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bits_case():
    rng = np.random.default_rng(99)
    R, I = 5, 33
    A, DB = PR.make_model(rng, R, I)
    Js = [5 + (7 * q) % 60 for q in range(40)]
    slabs = [PR.make_slab(rng, A, DB, J)[0] for J in Js]
    return A, DB, slabs


def test_bits(pkg, eng, bits_case):
    A, DB, slabs = bits_case
    state_block(pkg, eng, A, DB)
    kw = dict(max_iter=4, tol=1e-9, nonneg=True, return_P=True)
    full = eng.par2_fold_in(0, slabs, **kw)
    same_out(full, eng.par2_fold_in(0, slabs, **kw))                       # twice
    for q in (0, 17, 39):                                                  # alone against the call of 40
        one = eng.par2_fold_in(0, [slabs[q]], **kw)
        same_out(one, {k: (v[q:q + 1] if isinstance(v, (list, np.ndarray)) else v) for k, v in full.items()})
    perm = np.random.default_rng(1).permutation(40)
    pm = eng.par2_fold_in(0, [slabs[i] for i in perm], **kw)
    same_out(pm, {k: ([v[i] for i in perm] if isinstance(v, list) else v[perm] if isinstance(v, np.ndarray) else v) for k, v in full.items()})
    bare = eng.par2_fold_in(0, slabs, max_iter=4, tol=1e-9, nonneg=True, return_B=False)
    assert bare['B'] is None and bare['P'] is None
    same_out(bare, full)
    rich = eng.par2_fold_in(0, slabs, return_y=True, return_sys=True, **kw)
    same_out(rich, full)


def test_nan_and_zero_slabs(pkg, eng, bits_case):
    A, DB, slabs = bits_case
    state_block(pkg, eng, A, DB)
    kw = dict(max_iter=4, tol=1e-9, return_P=True)
    full = eng.par2_fold_in(0, slabs[:8], **kw)
    bad = [X.copy() for X in slabs[:8]]
    bad[3][2, 1] = np.nan
    bad[5][:] = 0.0
    out = eng.par2_fold_in(0, bad, **kw)
    keep = [0, 1, 2, 4, 6, 7]
    same_out({k: ([v[i] for i in keep] if isinstance(v, list) else v[keep] if isinstance(v, np.ndarray) else v) for k, v in out.items()},
             {k: ([v[i] for i in keep] if isinstance(v, list) else v[keep] if isinstance(v, np.ndarray) else v) for k, v in full.items()})
    assert np.all(np.isnan(out['C'][3])) and out['iters'][3] == 4
    assert out['info'][5] == 1 and np.all(out['C'][5] == 0) and out['res'][5] == 0 and out['xnorm'][5] == 0


def test_after_a_solve_against_the_uploaded_state(pkg, eng, bits_case):
    rng = np.random.default_rng(3)
    Z, io = script4_model(rng, K=5)
    new = [rng.standard_normal((40, j)) for j in (61, 3, 130)]
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=rng)
    _, Fg, _, _ = pkg.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=4), init=copy.deepcopy(G), engine=eng)
    a = eng.par2_fold_in(0, new, nonneg=True, return_P=True)
    state_block(pkg, eng, Fg['fac'][0], Fg['DeltaB'][0])
    same_out(a, eng.par2_fold_in(0, new, nonneg=True, return_P=True))


# ---- 7. kinds of block ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['dense', 'sparse', 'masked'])
def test_kinds_of_block_answer_alike(pkg, eng, kind):
    rng = np.random.default_rng(8)
    Z, _ = script4_model(rng, K=4)
    Z = dict(Z, _ranks=[3, 3, 3])
    A, DB = PR.make_model(rng, 3, 40)
    new = [PR.make_slab(rng, A, DB, J)[0] for J in (61, 7, 120)]
    state_block(pkg, eng, A, DB)
    want = eng.par2_fold_in(0, new, nonneg=True, return_P=True)
    miss = None
    if kind == 'sparse':
        Z['object'] = [[pkg.sptensor(np.argwhere(np.abs(Xk) > 0.01), Xk[np.abs(Xk) > 0.01], Xk.shape) for Xk in Z['object'][0]]]
    if kind == 'masked':
        miss = [(rng.random(Xk.shape) < 0.8).astype(np.float64) for Xk in Z['object'][0]]
    state_block(pkg, eng, A, DB, Z=Z, miss=miss)
    same_out(want, eng.par2_fold_in(0, new, nonneg=True, return_P=True))


def test_slab_sharded_block_ranks_ask_different_slabs(pkg, eng):
    rng = np.random.default_rng(10)
    Z, io = script4_model(rng, K=7)
    opt = dict(options(MaxOuterIters=4), hip=dict(par2_slab_sharding=1))
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=rng)
    new = [[rng.standard_normal((40, j)) for j in (61, 9)], [rng.standard_normal((40, j)) for j in (130,)]]
    key, world = next(_keys), 2
    res, err = [None] * world, [None] * world

    def rank_main(r):
        try:
            with pkg.Engine(0) as e:
                e.comm_init_local(key, r, world)
                _, Fg, _, _ = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=e)
                res[r] = (Fg, e.par2_fold_in(0, new[r], nonneg=True, return_P=True))
        except BaseException as ex:   # noqa: BLE001 -- reported by the main thread
            err[r] = ex

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r, ex in enumerate(err):
        assert ex is None, 'rank %d: %r' % (r, ex)
    Fg = res[0][0]
    state_block(pkg, eng, Fg['fac'][0], Fg['DeltaB'][0])
    for r in range(world):
        same_out(res[r][1], eng.par2_fold_in(0, new[r], nonneg=True, return_P=True))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(pkg, eng):
    rng = np.random.default_rng(0)
    R, I = 3, 10
    A, DB = PR.make_model(rng, R, I)
    state_block(pkg, eng, A, DB)
    cols = np.array([4, 5], dtype=np.int64)
    X = rng.standard_normal(I * 9)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_int64)

    def call(p=0, nk=2, cols=cols, X=X, opt=None, null=()):
        bufs = dict(C=np.full(2 * R, 7.0), B=np.full(9 * R, 7.0), P=np.full(9 * R, 7.0), res=np.full(2, 7.0), xnorm=np.full(2, 7.0),
                    Y=np.full(9 * R, 7.0), sys=np.full(R * R, 7.0))
        iters, info, path = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32), (C.c_int * 2)(7, 7)
        o = capi.Par2FoldinOptions(*(opt or (50, 1e-8, 0.0, 0, 5, 0.0, 0.0)))
        g = lambda k: None if k in null else capi.dptr(bufs[k])
        rc = eng.lib.aoadmm_resident_par2_fold_in(
            eng.h, p, nk, None if 'cols' in null else cols.ctypes.data_as(lp), None if 'X' in null else capi.dptr(X), None, C.byref(o),
            g('C'), g('B'), g('P'), g('res'), g('xnorm'), None if 'iters' in null else iters.ctypes.data_as(ip),
            None if 'info' in null else info.ctypes.data_as(ip), g('Y'), g('sys'), path)
        untouched = all(np.all(v == 7.0) for v in bufs.values()) and np.all(iters == 7) and np.all(info == 7) and path[0] == 7
        return rc, untouched

    INVALID, NOT_PD, UNSUPPORTED = capi.ERR_INVALID, capi.ERR_NOT_PD, capi.ERR_UNSUPPORTED
    big = np.array([2 ** 31, 5], dtype=np.int64)
    half = np.array([2 ** 30, 2 ** 30], dtype=np.int64)
    third = np.array([4 * 10 ** 8, 4 * 10 ** 8], dtype=np.int64)      # sum J_q fits an int, R sum J_q does not
    cases = [dict(p=-1), dict(p=1), dict(nk=-1), dict(cols=np.array([4, 2], dtype=np.int64)), dict(cols=big), dict(cols=half),
             dict(cols=third),
             dict(opt=(0, 1e-8, 0.0, 0, 5, 0.0, 0.0)), dict(opt=(5, -1.0, 0.0, 0, 5, 0.0, 0.0)), dict(opt=(5, np.nan, 0.0, 0, 5, 0.0, 0.0)),
             dict(opt=(5, np.inf, 0.0, 0, 5, 0.0, 0.0)), dict(opt=(5, 0.0, -1.0, 0, 5, 0.0, 0.0)), dict(opt=(5, 0.0, np.inf, 0, 5, 0.0, 0.0)),
             dict(opt=(5, 0.0, 0.0, 2, 5, 0.0, 0.0)), dict(opt=(5, 0.0, 0.0, 1, 0, 0.0, 0.0)), dict(opt=(5, 0.0, 0.0, 1, 5, -1.0, 0.0)),
             dict(opt=(5, 0.0, 0.0, 1, 5, 0.0, -1.0))]
    cases += [dict(null=(k,)) for k in ('cols', 'X', 'C', 'res', 'iters', 'info')]
    for kw in cases:
        rc, untouched = call(**kw)
        assert rc == INVALID and untouched, kw
    assert call()[0] == 0 and not call()[1]
    assert call(null=('B', 'P', 'xnorm', 'Y', 'sys'))[0] == 0
    assert call(nk=0) == (0, True)
    # state missing: a block whose DeltaB was never set
    Z = par2_Z(I, R, [R, R + 1])
    pkg.build_model(eng, Z)
    assert call() == (INVALID, True)
    # rank-deficient A: a zero column makes a pivot of S exactly zero
    A0 = A.copy()
    A0[:, 1] = 0.0
    state_block(pkg, eng, A0, DB)
    assert call() == (NOT_PD, True)
    assert call(opt=(5, 0.0, 0.5, 0, 5, 0.0, 0.0))[0] == 0           # the ridge repairs it
    eng.kernel_stats(17, reset=True)
    with pytest.raises(pkg.NotPositiveDefinite):
        eng.par2_fold_in(0, [X[:I * 4].reshape(I, 4, order='F')])
    assert eng.kernel_stats(17)[1:] == (0, 0.0, 0.0)                  # a call that fails counts nothing


def test_wrong_row_count_is_refused_before_the_call(pkg, eng):
    """The C entry takes the rows of a slab from the model, so Engine.par2_fold_in refuses slabs whose row count is not the
    block's I (transposed slabs, a slab of another block) before the library reads them."""
    rng = np.random.default_rng(5)
    R, I = 3, 10
    A, DB = PR.make_model(rng, R, I)
    state_block(pkg, eng, A, DB)
    assert eng.par2_rows(0) == I
    good = rng.standard_normal((I, 7))
    for bad in ([good.T], [good, good[:I - 1]], [np.vstack([good, good])], [good[:0]]):
        with pytest.raises(ValueError):
            eng.par2_fold_in(0, bad)
    assert eng.par2_fold_in(0, [good])['info'][0] == 0
    rows = C.c_int64(-7)
    assert eng.lib.aoadmm_par2_rows(eng.h, 1, C.byref(rows)) == capi.ERR_INVALID and rows.value == -7
    assert eng.lib.aoadmm_par2_rows(eng.h, 0, None) == capi.ERR_INVALID


def test_cp_block_and_multi_device_context(pkg, eng):
    from helpers import cp_model
    rng = np.random.default_rng(1)
    Z, _, _ = cp_model((6, 5, 4), 2, rng, [None, None, None])
    Z = dict(Z, _ranks=[2, 2, 2])
    pkg.build_model(eng, Z)
    pkg.upload_state(eng, Z, {'fac': [rng.standard_normal((n, 2)) for n in (6, 5, 4)]})
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.par2_fold_in(0, [rng.standard_normal((6, 3))])
    assert ei.value.code == capi.ERR_INVALID
    rows = C.c_int64(0)
    assert eng.lib.aoadmm_par2_rows(eng.h, 0, C.byref(rows)) == capi.ERR_INVALID
    with pkg.Engine([0, 0]) as multi:
        pkg.build_model(multi, par2_Z(10, 3, [3, 4]))
        with pytest.raises(pkg.UnsupportedOnDevice):
            multi.par2_fold_in(0, [rng.standard_normal((10, 4))])


def test_kernel_stats_class_17(pkg, eng):
    rng = np.random.default_rng(2)
    A, DB = PR.make_model(rng, 3, 40)
    state_block(pkg, eng, A, DB)
    eng.kernel_stats(17, reset=True)
    slabs = [rng.standard_normal((40, j)) for j in (61, 70)]
    out = eng.par2_fold_in(0, slabs, max_iter=3, tol=0.0)
    eng.par2_fold_in(0, slabs, max_iter=3, tol=0.0)
    ms, launches, nbytes, flops = eng.kernel_stats(17)
    Jtot, I, R, nk = 131, 40, 3, 2
    assert launches == 2 and ms > 0
    assert nbytes == 2 * (8 * (I * Jtot + I * R + 3 * Jtot * R + nk * R + 2 * nk) + 8 * nk)
    assert flops == 2 * (2 * I * Jtot * R + 9 * R * R * float(np.sum(out['iters'] * np.array([61, 70]))))
    with pytest.raises(pkg.AoadmmError):
        eng.kernel_stats(15)
    with pytest.raises(pkg.AoadmmError):
        eng.kernel_stats(18)
