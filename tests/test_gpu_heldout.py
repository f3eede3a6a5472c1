"""GPU: held-out scoring (include/aoadmm_hip.h "held-out entries"): the model of a CP or PARAFAC2
block at a list of subscripts (aoadmm_resident_model_at), the three sums of an attached list
(aoadmm_resident_heldout_stats), the trace a solve keeps (aoadmm_heldout_trace) and early stopping on it
(aoadmm_options.heldout_patience).  The reference is numpy in fp64 on the same factors; no array of the tensor's size
is needed on either side."""
import copy
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from helpers import cp_cp_exact_model, cp_model, options, script4_model
from test_gpu_sparse_sharded import on_ranks

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')

OP_SHAPES = {2: (300, 40), 3: (40, 30, 20), 4: (12, 10, 9, 8)}
RANKS = [1, 3, 4, 5, 8, 9, 16, 17, 20, 32, 33, 64]       # both ends of every lane-team class (4, 8, 16, 32, 64)
LENGTHS = [1, 255, 256, 257, 1500]                       # one entry, both sides of a chunk of 256, chunks + a ragged tail
NN = ('non-negativity',)
OBSERVED = {'sparse_observed_only': 1}
HELDOUT_CLASS = 12                                       # aoadmm_kernel_stats: the held-out passes


def cp_Z(shape, R, obj):
    n = len(shape)
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(shape),
                coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
                constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[obj], _ranks=[R] * n)


def some_entries(pkg, rng, shape, n=50):
    subs = np.stack([rng.integers(0, s, n) for s in shape], axis=1)
    return pkg.sptensor(subs, rng.standard_normal(n), shape)


def make_list(rng, shape, n):
    """n subscripts: the first row of every mode, the last row of every mode (n = 1: only that one), repeated subscripts
    at the end, the rest uniform."""
    subs = np.stack([rng.integers(0, s, n) for s in shape], axis=1).astype(np.int64)
    subs[0] = [s - 1 for s in shape]
    if n > 1:
        subs[1] = 0
    if n >= 8:
        subs[-3:] = subs[2:5]                                 # repeats: each is scored
    return subs


def ref_values(U, subs):
    """(m, bound) in fp64: m = sum_r prod_n U_n(s_n, r), bound = sum_r prod_n |U_n(s_n, r)|"""
    P = np.ones((subs.shape[0], U[0].shape[1]))
    for n, F in enumerate(U):
        P = P * F[subs[:, n]]
    return P.sum(axis=1), np.abs(P).sum(axis=1)


def ref_sums(m, y):
    return float(np.sum((y - m) ** 2)), float(np.sum(y * y)), float(np.sum(m * m))


def cp_block(pkg, eng, rng, shape, R, row_major):
    """One CP block with signed factors on `eng`; row_major: a solve of 0 iterations leaves the Gram kernel's row-major
    copies of the same factors current.  Returns the factors."""
    Z = cp_Z(shape, R, some_entries(pkg, rng, shape))
    U = [rng.random((s, R)) - 0.3 for s in shape]
    pkg.build_model(eng, Z)
    pkg.upload_state(eng, Z, {'fac': U})
    if row_major:
        pkg.run_solver(eng, options(MaxOuterIters=0), len(shape))
    return U


def layouts(N):
    return [False, True] if N == 3 else [False]


# ---- 1. values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('N', [2, 3, 4])
def test_model_at_values(pkg, eng, N, R):
    """|m_dev - m_ref| <= 1e-12 sum_r prod_n |F_n(s_n, r)| per entry: the derived bound is (R + N) 2^-53 = 7.6e-15 of that
    sum at R = 64; 1e-12 is this project's fp64 bar for a change of summation order."""
    shape = OP_SHAPES[N]
    for row_major in layouts(N):
        rng = np.random.default_rng(1000 * N + R)
        U = cp_block(pkg, eng, rng, shape, R, row_major)
        for n in LENGTHS:
            subs = make_list(rng, shape, n)
            m_ref, bound = ref_values(U, subs)
            eng.kernel_stats(HELDOUT_CLASS, reset=True)
            m = eng.model_at(0, subs)
            assert m.shape == (n,)
            worst = float(np.max(np.abs(m - m_ref) / bound))
            assert worst <= 1e-12, (N, R, n, row_major, worst)
            assert eng.heldout_info(0)['row_major'] == int(row_major)
            _, launches, by, fl = eng.kernel_stats(HELDOUT_CLASS)
            assert launches == 1 and by == n * (4 * N + 8 + 8 * N * R) and fl == n * R * N
        if n > 1:
            for mode, s in enumerate(shape):                  # the first and the last row of every mode were asked for
                assert subs[:, mode].min() == 0 and subs[:, mode].max() == s - 1


@pytest.mark.parametrize('R', [3, 20, 64])
def test_order_taken_at_run_time(pkg, eng, R):
    """Orders 2-4 are compiled in; a 5-way block takes the kernel that reads the order at run time."""
    shape, N = (6, 5, 4, 3, 4), 5
    rng = np.random.default_rng(500 + R)
    U = cp_block(pkg, eng, rng, shape, R, False)
    for n in (1, 257, 1500):
        subs = make_list(rng, shape, n)
        m_ref, bound = ref_values(U, subs)
        m = eng.model_at(0, subs)
        assert float(np.max(np.abs(m - m_ref) / bound)) <= 1e-12
        y = rng.standard_normal(n)
        eng.set_heldout(0, subs, y)
        st = eng.heldout_stats(0)
        assert st[3] == n
        for got, want in zip(st[:3], ref_sums(m_ref, y)):
            assert abs(got - want) <= 1e-11 * want, (R, n, got, want)


def par2_block(pkg, eng, rng, sparse):
    Z, _ = script4_model(rng, K=4)
    Z = dict(Z, _ranks=[3, 3, 3])
    if sparse:
        Z['object'] = [[pkg.sptensor(np.argwhere(np.abs(Xk) > 0.01), Xk[np.abs(Xk) > 0.01], Xk.shape) for Xk in Z['object'][0]]]
    I, Jk, K = Z['size']
    A, B, Cm = rng.random((I, 3)) - 0.3, [rng.random((j, 3)) - 0.3 for j in Jk], rng.random((K, 3)) - 0.3
    pkg.build_model(eng, Z)
    pkg.upload_state(eng, Z, {'fac': [A, B, Cm]})
    return Z, A, B, Cm


def par2_list(rng, I, Jk, n):
    k = rng.integers(0, len(Jk), n)
    subs = np.stack([rng.integers(0, I, n), rng.integers(0, np.asarray(Jk)[k]), k], axis=1).astype(np.int64)
    for q, j in enumerate(Jk):                                # first and last row of every slab, of A and of C
        subs[2 * q] = [0, 0, q]
        subs[2 * q + 1] = [I - 1, j - 1, q]
    subs[-3:] = subs[8:11]
    return subs


def par2_ref(A, B, Cm, subs):
    Mk = [A @ np.diag(Cm[k]) @ B[k].T for k in range(len(B))]                  # I x J_k
    m = np.array([Mk[k][i, j] for i, j, k in subs])
    bound = np.array([np.sum(np.abs(A[i] * B[k][j] * Cm[k])) for i, j, k in subs])
    return m, bound


@pytest.mark.parametrize('sparse', [False, True], ids=['dense-slabs', 'sparse-slabs'])
def test_model_at_parafac2(pkg, eng, sparse):
    """Ragged J_k = 61, 68, 75, 82: m = sum_r A(i,r) B_k(j,r) C(k,r) against A diag(C[k]) B_k', and the sums of a list."""
    rng = np.random.default_rng(77)
    Z, A, B, Cm = par2_block(pkg, eng, rng, sparse)
    I, Jk, K = Z['size']
    for n in (257, 1500):
        subs = par2_list(rng, I, Jk, n)
        m_ref, bound = par2_ref(A, B, Cm, subs)
        m = eng.model_at(0, subs)
        assert float(np.max(np.abs(m - m_ref) / bound)) <= 1e-12
        y = rng.standard_normal(n)
        eng.set_heldout(0, subs, y)
        st = eng.heldout_stats(0)
        assert st[3] == n and np.allclose(st[:3], ref_sums(m_ref, y), rtol=1e-11, atol=0)
    with pytest.raises(pkg.AoadmmError) as ei:                # j inside the longest slab but outside its own
        eng.model_at(0, np.array([[0, Jk[0], 0]]))
    assert ei.value.code == capi.ERR_INVALID


# ---- 2. statistics ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('N', [2, 3, 4])
def test_heldout_sums(pkg, eng, N, R):
    """sum (y - m)^2, sum y^2, sum m^2 against numpy at a relative 1e-11: the terms are non-negative, so this bounds the
    chunked order; y is standard normal and independent of the model, so sum (y - m)^2 is not a cancellation."""
    shape = OP_SHAPES[N]
    for row_major in layouts(N):
        rng = np.random.default_rng(2000 * N + R)
        U = cp_block(pkg, eng, rng, shape, R, row_major)
        for n in LENGTHS:
            subs = make_list(rng, shape, n)
            y = rng.standard_normal(n)
            m_ref, _ = ref_values(U, subs)
            eng.set_heldout(0, subs, y)
            st = eng.heldout_stats(0)
            ref = ref_sums(m_ref, y)
            assert st[3] == n
            for got, want in zip(st[:3], ref):
                assert abs(got - want) <= 1e-11 * want, (N, R, n, row_major, got, want)
            assert eng.heldout_info(0)['row_major'] == int(row_major)


@pytest.mark.parametrize('R', [5, 33])
@pytest.mark.parametrize('n', [257, 1500])
def test_heldout_sums_exact(pkg, eng, n, R):
    """Small integers: every product and every sum is exact in fp64, so the device equals numpy bit for bit."""
    shape = OP_SHAPES[3]
    rng = np.random.default_rng(n + R)
    Z = cp_Z(shape, R, some_entries(pkg, rng, shape))
    U = [rng.integers(-2, 3, (s, R)).astype(np.float64) for s in shape]
    pkg.build_model(eng, Z)
    pkg.upload_state(eng, Z, {'fac': U})
    subs = make_list(rng, shape, n)
    y = rng.integers(-3, 4, n).astype(np.float64)
    m_ref, _ = ref_values(U, subs)
    assert np.array_equal(eng.model_at(0, subs), m_ref)
    eng.set_heldout(0, subs, y)
    assert eng.heldout_stats(0) == ref_sums(m_ref, y) + (n,)


# ---- 3. determinism and ranks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('sharded', [False, True], ids=['replicated', 'sharded'])
@pytest.mark.parametrize('world', [2, 3])
def test_ranks_are_bit_identical(pkg, eng, world, sharded):
    """The pass reads only the replicated factors: every rank of a communicator returns the single engine's bits, with the
    block's nonzeros replicated or sharded over the ranks; a second call returns the same bits."""
    shape, R, n = OP_SHAPES[3], 5, 1500
    rng = np.random.default_rng(31)
    S = some_entries(pkg, rng, shape, 700)
    U = [rng.random((s, R)) - 0.3 for s in shape]
    subs, y = make_list(rng, shape, n), rng.standard_normal(n)

    def score(e, r=0, sharding=False):
        Z = cp_Z(shape, R, S)
        pkg.build_model(e, Z, sparse_sharding=sharding)
        pkg.upload_state(e, Z, {'fac': U})
        e.set_heldout(0, subs, y)
        first = (e.model_at(0, subs), e.heldout_stats(0))
        second = (e.model_at(0, subs), e.heldout_stats(0))
        assert np.array_equal(first[0], second[0]) and first[1] == second[1]
        return first

    m1, st1 = score(eng)
    for m2, st2 in on_ranks(pkg, world, lambda e, r: score(e, r, sharded)):
        assert np.array_equal(m1, m2) and st1 == st2


# ---- 4. / 5. the solve is not disturbed, and the trace is right ------------------------------------------------------------
def _pick(rng, where, n):
    cells = np.argwhere(where)
    return cells[rng.choice(len(cells), n, replace=False)].astype(np.int64)


def solve_case(pkg, name):
    """(Z, io, alg_options, {1-based block: (subs, vals)}, precision, block model values from Fac)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    prec = 'f64'
    if name in ('sparse', 'observed', 'rank20-long-mode'):
        shape, R, iters = ((300, 40, 30), 20, 5) if name == 'rank20-long-mode' else ((40, 30, 20), 3, 12)
        Z, io, _ = cp_model(shape, R, rng, [NN] * 3)
        X = np.asarray(Z['object'][0])
        keep = rng.random(shape) < (0.05 if name == 'rank20-long-mode' else 0.2)
        Z = dict(Z, object=[pkg.sptensor(np.argwhere(keep), X[keep], shape)])
        subs = _pick(rng, ~keep, 700)
        held = {1: (subs, X[tuple(subs.T)])}
        hip = {} if name == 'sparse' else dict(OBSERVED)
    elif name in ('dense', 'dense-miss', 'f16'):
        shape, R, iters = (40, 30, 20), 3, 10
        Z, io, _ = cp_model(shape, R, rng, [NN, None, NN])
        X = np.asarray(Z['object'][0])
        hip = {}
        if name == 'dense-miss':
            keep = rng.random(shape) < 0.7
            Z = dict(Z, object=[np.where(keep, X, 0.0)], miss=[keep])
            subs = _pick(rng, ~keep, 700)                     # a subset of the missing entries
        else:
            subs = _pick(rng, np.ones(shape, dtype=bool), 700)
        held = {1: (subs, X[tuple(subs.T)] + 0.01 * rng.standard_normal(700))}
        prec = 'f16' if name == 'f16' else 'f64'
    elif name == 'coupled':
        Z, io = cp_cp_exact_model(rng)
        X = np.asarray(Z['object'][0])
        subs = _pick(rng, np.ones(X.shape, dtype=bool), 600)
        held, hip, iters = {1: (subs, X[tuple(subs.T)] + 0.01 * rng.standard_normal(600))}, {}, 8
    elif name == 'par2':
        Z, io = script4_model(rng, K=4)
        I, Jk, K = Z['size']
        subs = par2_list(rng, I, Jk, 600)
        vals = np.array([Z['object'][0][k][i, j] for i, j, k in subs]) + 0.01 * rng.standard_normal(600)
        held, hip, iters = {1: (subs, vals)}, {}, 6
    else:
        raise KeyError(name)
    return Z, io, options(MaxOuterIters=iters), held, hip, prec


def block_values(Z, Fac, p, subs):
    md = [m - 1 for m in Z['modes'][p]]
    if Z['model'][p] == 'PAR2':
        return par2_ref(Fac['fac'][md[0]], Fac['fac'][md[1]], Fac['fac'][md[2]], subs)[0]
    return ref_values([Fac['fac'][m] for m in md], subs)[0]


def same(a, b):
    """bitwise equality over the nested lists / dicts of a Fac or out struct"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None or isinstance(a, str):
        return a is b or a == b
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


SOLVE_CASES = ['sparse', 'observed', 'dense', 'dense-miss', 'f16', 'coupled', 'par2', 'rank20-long-mode']
_solved = {}


def solved(pkg, eng, name):
    """One set of runs per case, shared by the tests below: without a list, with it, and the prefixes of 0 and 1 iterations."""
    if name not in _solved:
        Z, io, opt, held, hip, prec = solve_case(pkg, name)
        G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))

        def run(iters, with_list):
            alg = {**opt, 'MaxOuterIters': iters, 'hip': {**hip, **({'heldout': held} if with_list else {})}}
            _, F, _, out = pkg.cmtf_AOADMM(Z, alg_options=alg, init=copy.deepcopy(G), engine=eng, precision=prec)
            return F, out

        last = opt['MaxOuterIters']
        _solved[name] = dict(Z=Z, held=held, last=last, plain=run(last, False), scored=run(last, True),
                             prefix={0: run(0, False), 1: run(1, False)})
    return _solved[name]


@pytest.mark.parametrize('name', SOLVE_CASES)
def test_solve_is_not_disturbed(pkg, eng, name):
    """Every factor, dual, innerIters and objective trace is bit for bit that of the solve without a list."""
    s = solved(pkg, eng, name)
    (Fp, op), (Fs, os_) = s['plain'], s['scored']
    assert same(Fp, Fs)
    for k in op:
        if k != 'time_at_it':
            assert same(op[k], os_[k]), k
    assert set(os_) - set(op) == {'func_heldout', 'heldout_sumsq', 'heldout_count', 'heldout_best_iter'}
    assert os_['OuterIterations'] == s['last'] and os_['exit_flag'] == 'maxIterations'


@pytest.mark.parametrize('name', SOLVE_CASES)
def test_trace_is_the_sum_over_the_list(pkg, eng, name):
    """func_heldout[i] for i = 0, 1 and the last iteration against numpy on the factors a solve of i iterations returns
    (tolerances 0: that solve is the prefix of the longer one), at a relative 1e-11."""
    s = solved(pkg, eng, name)
    out = s['scored'][1]
    for q, (subs, y) in s['held'].items():
        T = out['func_heldout'][q]
        assert T.shape == (out['OuterIterations'] + 1,) and np.all(np.isfinite(T))
        assert out['heldout_count'][q] == len(y) and out['heldout_sumsq'][q] == float(np.sum(y * y))
        for i, F in [(0, s['prefix'][0][0]), (1, s['prefix'][1][0]), (s['last'], s['plain'][0])]:
            want = float(np.sum((y - block_values(s['Z'], F, q - 1, subs)) ** 2))
            print('%s block %d iteration %d: device %.17g numpy %.17g' % (name, q, i, T[i], want))
            assert abs(T[i] - want) <= 1e-11 * want, (name, i, T[i], want)
        assert out['heldout_best_iter'] == int(np.argmin(T))      # one block with a list: H_i = w T_i


# ---- 6. early stopping --------------------------------------------------------------------------------------------------
def patience_rule(T, k):
    """the iteration after which the rule stops: T has not been strictly below its best so far for k iterations in a row"""
    best, bad = T[0], 0
    for i in range(1, len(T)):
        if T[i] < best:
            best, bad = T[i], 0
        else:
            bad += 1
        if bad >= k:
            return i
    return len(T) - 1


def test_early_stopping_on_an_overfitting_case(pkg, eng):
    """A rank-4 fit of 702 noisy entries of a rank-2 tensor, 754 more held out.  The oracle (CPU, on the densified block
    with Z.miss): the held-out sum falls to its minimum 0.038351 at iteration 29 and rises monotonically afterwards
    (0.039522 = 1.031 x the minimum at iteration 60; the device gives the same figures); the smallest relative step between consecutive iterations is 4.6e-5, four
    orders above the device-oracle distance, so the rule cannot flip on rounding; patience 5 stops at 34."""
    rng = np.random.default_rng(33)
    shape = (30, 25, 20)
    Z, io, _ = cp_model(shape, 2, rng, [None] * 3, noise=1.0)
    io['lambdas_init'] = [[1] * 4]
    X = np.asarray(Z['object'][0])
    u = rng.random(shape)
    train, hold = u < 0.05, (u >= 0.05) & (u < 0.10)
    assert train.sum() == 702 and hold.sum() == 754
    Zs = dict(Z, object=[pkg.sptensor(np.argwhere(train), X[train], shape)])
    held = {1: (np.argwhere(hold), X[hold])}
    G = OA.init_coupled_AOADMM_CMTF({**Zs, 'prox_operators': None}, io, rng=np.random.default_rng(7))

    def run(**hip):
        alg = {**options(MaxOuterIters=60, MaxInnerIters=5), 'hip': {'heldout': held, **hip}}
        return pkg.cmtf_AOADMM(Zs, alg_options=alg, init=copy.deepcopy(G), engine=eng)[3]

    free = run(**OBSERVED)
    T = free['func_heldout'][1]
    best = int(np.argmin(T))
    print('un-stopped: minimum %.6f at iteration %d, %.4f x the minimum at 60' % (T[best], best, T[60] / T[best]))
    assert free['OuterIterations'] == 60 and free['exit_flag'] == 'maxIterations' and free['heldout_best_iter'] == best
    assert 1 < best < 55                                      # the case cannot pass by running out of iterations
    for k in (5, 1, 3):
        out = run(heldout_patience=k, **OBSERVED)
        Tk = out['func_heldout'][1]
        print('patience %d: stopped after iteration %d, best %d' % (k, out['OuterIterations'], out['heldout_best_iter']))
        assert out['OuterIterations'] == patience_rule(T, k) < 60
        assert out['exit_flag'] == 'heldoutPatience'
        assert out['heldout_best_iter'] == int(np.argmin(Tk)) == best
        assert np.array_equal(Tk, T[:len(Tk)])
    # without the mark the unstored entries are fitted as zeros: the held-out entries are never predicted as well
    plain = run()
    print('zeros as data: minimum %.6f' % plain['func_heldout'][1].min())
    assert plain['func_heldout'][1].min() > T[best]


# ---- 7. hygiene -----------------------------------------------------------------------------------------------------------
def test_list_lifetime_and_refusals(pkg, eng):
    rng = np.random.default_rng(51)
    shape, R, N = (12, 10, 8), 3, 3
    S = some_entries(pkg, rng, shape, 200)
    Z = cp_Z(shape, R, S)
    U = [rng.random((s, R)) for s in shape]
    pkg.build_model(eng, Z)
    pkg.upload_state(eng, Z, {'fac': U})
    storage = eng.tensor_storage_info(0)
    assert eng.heldout_info(0) == dict(n=0, resident_bytes=0, row_major=-1)
    with pytest.raises(pkg.AoadmmError) as ei:                # no list yet
        eng.heldout_stats(0)
    assert ei.value.code == capi.ERR_INVALID
    subs, y = make_list(rng, shape, 300), rng.standard_normal(300)
    eng.set_heldout(0, subs, y)
    info = eng.heldout_info(0)
    assert info['n'] == 300 and info['resident_bytes'] == 300 * (4 * N + 8)
    assert eng.tensor_storage_info(0) == storage              # the block's own bytes do not move
    first = eng.heldout_stats(0)
    # a bad list is refused and the old one is still scored
    for bad_subs, bad_y in [(np.array([[0, 0, shape[2]]]), [1.0]), (np.array([[-1, 0, 0]]), [1.0]),
                            (subs[:2], [1.0, np.nan]), (subs[:2], [np.inf, 1.0])]:
        with pytest.raises(pkg.AoadmmError) as ei:
            eng.set_heldout(0, bad_subs, bad_y)
        assert ei.value.code == capi.ERR_INVALID
        assert eng.heldout_info(0)['n'] == 300 and eng.heldout_stats(0) == first
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.model_at(0, np.array([[shape[0], 0, 0]]))
    assert ei.value.code == capi.ERR_INVALID
    # a re-upload of the block's data keeps the list
    eng.upload_coo(0, S.subs, S.vals)
    assert eng.heldout_info(0)['n'] == 300 and eng.heldout_stats(0) == first
    # n = 0 removes it
    eng.set_heldout(0, np.zeros((0, N), dtype=np.int64), [])
    assert eng.heldout_info(0)['n'] == 0
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.heldout_stats(0)
    assert ei.value.code == capi.ERR_INVALID
    # patience without a list: refused by the library before any work
    drv = importlib.import_module('matlab-code_amd.driver')
    o = drv._make_options({**options(MaxOuterIters=3), 'hip': {'heldout_patience': 2}})
    import ctypes as C
    res = capi.Result()
    assert eng.lib.aoadmm_solve(eng.h, C.byref(o), C.byref(res)) == capi.ERR_INVALID
    # aoadmm_model_begin drops the list
    eng.set_heldout(0, subs, y)
    pkg.build_model(eng, Z)
    assert eng.heldout_info(0)['n'] == 0
    # a model without factors cannot be evaluated
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.model_at(0, subs)
    assert ei.value.code == capi.ERR_INVALID


def test_second_solve_repeats_the_trace(pkg, eng):
    rng = np.random.default_rng(52)
    shape, R = (40, 30, 20), 4
    Z, io, _ = cp_model(shape, R, rng, [NN] * 3)
    X = np.asarray(Z['object'][0])
    keep = rng.random(shape) < 0.25
    Zs = dict(Z, object=[pkg.sptensor(np.argwhere(keep), X[keep], shape)], _ranks=[R] * 3)
    subs = _pick(rng, ~keep, 500)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    alg = {**options(MaxOuterIters=6), 'hip': dict(OBSERVED)}
    pkg.build_model(eng, Zs, observed_only=1)
    eng.set_heldout(0, subs, X[tuple(subs.T)])
    traces = []
    for _ in range(2):
        pkg.upload_state(eng, Zs, copy.deepcopy(G))
        out = pkg.run_solver(eng, alg, 3, has_missing=True)
        traces.append(eng.heldout_trace(0))
        assert len(traces[-1][0]) == out['OuterIterations'] + 1 == 7
    assert np.array_equal(traces[0][0], traces[1][0]) and traces[0][1] == traces[1][1]
    assert eng.heldout_info(0)['row_major'] == 1              # inside a solve the row-major copies are current


def test_multi_device_context_is_refused(pkg):
    rng = np.random.default_rng(53)
    shape, R = (12, 10, 8), 3
    Z = cp_Z(shape, R, some_entries(pkg, rng, shape, 100))
    subs, y = make_list(rng, shape, 20), rng.standard_normal(20)
    with pkg.Engine([0, 0]) as e:
        pkg.build_model(e, Z)
        pkg.upload_state(e, Z, {'fac': [rng.random((s, R)) for s in shape]})
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.set_heldout(0, subs, y)
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.model_at(0, subs)
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.heldout_stats(0)
