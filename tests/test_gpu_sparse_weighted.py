"""GPU: weighted sparse CP blocks (aoadmm_tensor_set_entry_weights; csrc/sparse_em.hip).
Every stored entry has a weight w_e in [0, 1], every unstored entry the one weight alpha: the solve must equal the
weighted EM  Xhat <- W o X + (1 - W) o M  run around the oracle one outer iteration at a time (tests/weighted_ref.py,
pinned to the oracle's own EM by tests/test_sparse_weighted_host.py).  Kernel level: the MTTKRP of the imputed tensor
and the EM statistics against dense numpy, an exact case; solver level: the stepped oracle, the limits of the weight
range, a known answer that needs the weights; plumbing and refusals."""
import copy
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from oracle.tensor_ops import full_ktensor
from oracle.tensor_ops import mttkrp as dense_mttkrp
from helpers import cp_cp_exact_model, cp_model, options, rel_fro, script4_model
from test_gpu_solver import _compare_em, compare
from test_gpu_sparse import assert_close, assert_same_solve
from test_gpu_sparse_observed import OP_SHAPES, RANKS, cp_Z, fms, put_factors, raw_block, signed, stored_entries
from test_gpu_sparse_sharded import on_ranks
from weighted_ref import dense_weights, stepped_em

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')

NN = ('non-negativity',)
SHAPE5 = (7, 6, 5, 4, 3)                                     # the run-time-order instantiation of the passes


def draw_weights(rng, n):
    """half of the weights from {0, 0.25, 0.5, 1}, half uniform in [0, 1)"""
    w = rng.random(n)
    pick = rng.random(n) < 0.5
    w[pick] = rng.choice([0.0, 0.25, 0.5, 1.0], int(pick.sum()))
    return w


def weight_list(rng, stored, wfun=draw_weights):
    """The coalesced stored set in shuffled order with a weight each: (subs, wts)"""
    subs = np.argwhere(stored)
    subs = subs[rng.permutation(len(subs))]
    return subs, wfun(rng, len(subs))


# ---- kernel level ----------------------------------------------------------------------------------------------------
def _mttkrp_case(pkg, eng, shape, R, seed):
    rng = np.random.default_rng(seed)
    N = len(shape)
    subs, vals, X, stored = stored_entries(rng, shape)
    raw_block(pkg, eng, shape, R, subs, vals)
    wsubs, wts = weight_list(rng, stored)
    Fo, F = signed(rng, shape, R), signed(rng, shape, R)
    absF = [np.abs(u) for u in F]
    for alpha in (0.0, 0.25, 1.0):
        W = dense_weights(shape, wsubs, wts, alpha)
        eng.set_entry_weights(0, wsubs, wts, alpha)
        put_factors(pkg, eng, shape, F)
        for n in range(N):                                   # before any step: the MTTKRP of W o X
            assert_close(eng.resident_mttkrp(0, n, shape[n], R), dense_mttkrp(W * X, F, n),
                         scale=dense_mttkrp(np.abs(W * X), absF, n))
        put_factors(pkg, eng, shape, Fo)
        eng.em_step(0)
        put_factors(pkg, eng, shape, F)
        Ximp = W * X + (1.0 - W) * full_ktensor(Fo)
        for n in range(N):
            assert_close(eng.resident_mttkrp(0, n, shape[n], R), dense_mttkrp(Ximp, F, n),
                         scale=dense_mttkrp(np.abs(Ximp), absF, n))


@pytest.mark.parametrize('N', [2, 3, 4])
@pytest.mark.parametrize('R', RANKS)
def test_imputed_mttkrp(pkg, eng, N, R):
    """alpha in {0, 0.25, 1}: the weighted block before any step against numpy's MTTKRP of W o X, and after em_step with
    Fo against numpy's dense MTTKRP of W o X + (1 - W) o M(Fo): 1e-12 of the MTTKRP of absolute values."""
    _mttkrp_case(pkg, eng, OP_SHAPES[N], R, 3000 * N + R)


@pytest.mark.parametrize('R', [3, 20])
def test_imputed_mttkrp_five_way(pkg, eng, R):
    _mttkrp_case(pkg, eng, SHAPE5, R, 3500 + R)


def _dyadic(a, what):
    """every value a multiple of 2^-6 below 2^53: sums and products of such values are exact in fp64"""
    s = np.asarray(a, dtype=np.float64) * 64.0
    assert np.all(s == np.round(s)) and np.all(np.abs(s) < 2.0 ** 53), what
    return a


@pytest.mark.parametrize('R', [4, 20, 33])
@pytest.mark.parametrize('alpha', [0.25, 0.5])
def test_exact_case(pkg, eng, R, alpha):
    """Integer factors in [-2, 2], integer values in [-5, 5], weights in {0, 0.25, 0.5, 0.75, 1}: every intermediate
    of the imputed MTTKRP is a multiple of 2^-6 far below 2^53, so the device must return numpy's numbers exactly."""
    rng = np.random.default_rng(4000 + R)
    shape = OP_SHAPES[3]
    N = len(shape)
    subs, vals, X, stored = stored_entries(rng, shape)
    vals = rng.integers(-5, 6, len(vals)).astype(np.float64)
    X = np.zeros(shape)
    np.add.at(X, tuple(subs.T), vals)
    raw_block(pkg, eng, shape, R, subs, vals)
    wsubs, wts = weight_list(rng, stored, lambda g, n: g.integers(0, 5, n) / 4.0)
    W = dense_weights(shape, wsubs, wts, alpha)
    Fo = [rng.integers(-2, 3, (s, R)).astype(np.float64) for s in shape]
    F = [rng.integers(-2, 3, (s, R)).astype(np.float64) for s in shape]
    eng.set_entry_weights(0, wsubs, wts, alpha)
    put_factors(pkg, eng, shape, Fo)
    eng.em_step(0)
    put_factors(pkg, eng, shape, F)
    Mo = _dyadic(full_ktensor(Fo), 'model')
    _dyadic(np.abs(W * X) + np.abs((1.0 - W) * Mo), 'imputed terms')
    Ximp = _dyadic(W * X + (1.0 - W) * Mo, 'imputed')
    absF = [np.abs(u) for u in F]
    for n in range(N):
        _dyadic(dense_mttkrp(np.abs(W * X) + np.abs(1.0 - W) * full_ktensor([np.abs(u) for u in Fo]), absF, n), 'mttkrp bound')
        want = _dyadic(dense_mttkrp(Ximp, F, n), 'mttkrp')
        assert np.array_equal(eng.resident_mttkrp(0, n, shape[n], R), want), n


def _telescoped(F1, F2):
    """M(F2) - M(F1) = sum_a [[F1_1 .. F1_{a-1}, F2_a - F1_a, F2_{a+1} .. F2_N]]: no difference of two models"""
    out = 0.0
    for a in range(len(F1)):
        out = out + full_ktensor([F1[n] if n < a else F2[n] - F1[n] if n == a else F2[n] for n in range(len(F1))])
    return out


def _stats_numpy(W, X, stored, alpha, F1, F2):
    """(wobj1, num1, wobj2, num2, den2) twice: summed over the dense array, and from the split sums the device forms
    (stored entries and the whole model apart) with the telescoped difference"""
    M1, M2 = full_ktensor(F1), full_ktensor(F2)
    C2 = (1.0 - W) ** 2
    dense = (np.sum(W * (X - M1) ** 2), np.sum(C2 * M1 ** 2), np.sum(W * (X - M2) ** 2), np.sum(C2 * (M2 - M1) ** 2),
             np.sum(C2 * M1 ** 2))
    D = _telescoped(F1, F2)
    w, c2 = W[stored], C2[stored]

    def obj(M):
        return np.sum(w * (X - M)[stored] ** 2) + alpha * (np.sum(M ** 2) - np.sum(M[stored] ** 2))

    def imp(M):
        return (1.0 - alpha) ** 2 * (np.sum(M ** 2) - np.sum(M[stored] ** 2)) + np.sum(c2 * M[stored] ** 2)

    split = (obj(M1), imp(M1), obj(M2), imp(D), imp(M1))
    return dense, split


STAT_STEPS = ((1e-1, 1e-10), (1e-4, 1e-10), (1e-7, 1e-7))


@pytest.mark.parametrize('N,R', [(2, 3), (3, 20), (3, 64), (4, 33)])
@pytest.mark.parametrize('alpha', [0.0, 0.25])
def test_em_step_statistics(pkg, eng, N, R, alpha):
    """Two consecutive steps whose factors differ by a relative 1e-1, 1e-4 and 1e-7 against the dense numpy values of
    sum W o (X - M)^2, ||(1 - W) o (M_new - M_old)||^2 and ||(1 - W) o M_old||^2: rtol 1e-10, and 1e-7 for num at the
    1e-7 step (the bars of test_gpu_sparse_observed.test_em_step_statistics).  The floor under them is the distance of
    two fp64 numpy formulations on the same inputs (the dense sums, and the split sums with the telescoped difference),
    measured on the CPU over all eight cases: at most 2.3e-16 for every quantity but num of the second step, for which
    the dense form subtracts two models: 2.3e-16 at 1e-1, 7.8e-14 at 1e-4 and 4.2e-11 at 1e-7.  Every bar is more than
    10 times its floor (asserted).  First step: den == 0 exactly.  Two runs return the same bits."""
    rng = np.random.default_rng(5000 * N + R)
    shape = OP_SHAPES[N]
    subs, vals, X, stored = stored_entries(rng, shape)
    raw_block(pkg, eng, shape, R, subs, vals)
    wsubs, wts = weight_list(rng, stored)
    W = dense_weights(shape, wsubs, wts, alpha)
    F1 = [rng.random((s, R)) + 0.1 for s in shape]
    for step, rtol in STAT_STEPS:
        F2 = [u * (1.0 + step * rng.standard_normal(u.shape)) for u in F1]
        dense, split = _stats_numpy(W, X, stored, alpha, F1, F2)
        floor = [abs(a / b - 1.0) for a, b in zip(dense, split)]
        runs = []
        for _ in range(2):
            eng.set_entry_weights(0, wsubs, wts, alpha)      # sets again: no snapshot
            put_factors(pkg, eng, shape, F1)
            s1 = eng.em_step(0)
            put_factors(pkg, eng, shape, F2)
            s2 = eng.em_step(0)
            runs.append((s1, s2))
        assert runs[0] == runs[1]
        (res1, num1, den1), (res2, num2, den2) = runs[0]
        got = (res1, num1, res2, num2, den2)
        print('step %g alpha %g: device vs split %s; dense vs split %s' % (
            step, alpha, ' '.join('%.1e' % (g / s - 1.0) for g, s in zip(got, split)), ' '.join('%.1e' % f for f in floor)))
        assert den1 == 0.0
        bars = (1e-10, 1e-10, 1e-10, rtol, 1e-10)
        for f, bar in zip(floor, bars):
            assert bar >= 10.0 * f, (f, bar)
        # the dense sums are the reference; for num the telescoped form is the accurate one of the two
        want = (dense[0], dense[1], dense[2], split[3], dense[4])
        for g, w_, bar in zip(got, want, bars):
            assert g == pytest.approx(w_, rel=bar)


# ---- solves ----------------------------------------------------------------------------------------------------------
def weighted_models(pkg, Z, p, mask, rng, alpha, wfun=draw_weights):
    """(Z with block p as where(mask, X, 0) for the reference, the same with block p as an sptensor, the weights
    aligned with the sptensor's entries, the dense W)"""
    X = np.where(mask, np.asarray(Z['object'][p]), 0.0)
    S = pkg.sptensor(np.argwhere(mask), X[mask], X.shape)
    w = wfun(rng, len(S.vals))
    Zr = dict(Z, object=list(Z['object']))
    Zr['object'][p] = X
    Zs = dict(Z, object=list(Z['object']))
    Zs['object'][p] = S
    return Zr, Zs, w, dense_weights(X.shape, S.subs, w, alpha)


def weighted_alg(opt, P, p, w, alpha, **hip):
    ew = [None] * P
    ew[p] = w
    return {**opt, 'hip': {'sparse_entry_weights': ew, 'sparse_unstored_weight': alpha, **hip}}


def solve_both(pkg, eng, Zr, Zs, io, opt, p, w, W, alpha, iters, seed=7):
    G = OA.init_coupled_AOADMM_CMTF({**Zr, 'prox_operators': None}, io, rng=np.random.default_rng(seed))
    Fo, oo = stepped_em(Zr, {p: W}, copy.deepcopy(G), opt, iters)
    _, Fs, _, os_ = pkg.cmtf_AOADMM(Zs, alg_options=weighted_alg(opt, len(Zs['object']), p, w, alpha),
                                    init=copy.deepcopy(G), engine=eng)
    return Fo, oo, Fs, os_


CASES = {
    'cp-30pct': ((40, 30, 20), 3, 0.30, [NN, NN, NN], 12, 0.1),
    'cp-30pct-tv': ((40, 30, 20), 3, 0.30, [NN, NN, ('TV regularization', 1e-3)], 12, 0.0),
    'matrix': ((30, 25), 4, 0.30, [NN, NN], 12, 0.5),
    'four-way': ((12, 10, 9, 8), 3, 0.30, [NN, None, NN, NN], 8, 0.05),
    'rank20-long-mode': ((300, 40, 30), 20, 0.05, [NN, NN, NN], 5, 0.02),
}


@pytest.mark.parametrize('case', list(CASES))
def test_solve_matches_the_stepped_oracle(pkg, eng, case):
    """compare() of test_gpu_solver.py (factors and duals 1e-8, innerIters equal, traces rtol 1e-7) and _compare_em()
    (func_rel_missing rtol 1e-7 / atol 1e-12, NaN at 0) against the stepped oracle."""
    shape, R, keep, constraints, iters, alpha = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)) + 1)
    Z, io, _ = cp_model(shape, R, rng, constraints)
    Zr, Zs, w, W = weighted_models(pkg, Z, 0, rng.random(shape) < keep, rng, alpha)
    Fo, oo, Fs, os_ = solve_both(pkg, eng, Zr, Zs, io, options(MaxOuterIters=iters), 0, w, W, alpha, iters)
    compare(Fo, oo, Fs, os_)
    _compare_em(oo, os_)


def test_solve_weighted_block_coupled_to_a_dense_block(pkg, eng):
    rng = np.random.default_rng(51)
    Z, io = cp_cp_exact_model(rng)
    Zr, Zs, w, W = weighted_models(pkg, Z, 0, rng.random(np.asarray(Z['object'][0]).shape) < 0.3, rng, 0.1)
    Fo, oo, Fs, os_ = solve_both(pkg, eng, Zr, Zs, io, options(MaxOuterIters=10), 0, w, W, 0.1, 10)
    compare(Fo, oo, Fs, os_)
    _compare_em(oo, os_)


# ---- the limits of the weight range ----------------------------------------------------------------------------------
def _limit_setup(pkg, seed):
    rng = np.random.default_rng(seed)
    shape = (40, 30, 20)
    Z, io, _ = cp_model(shape, 3, rng, [NN] * 3)
    mask = rng.random(shape) < 0.3
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    return rng, Z, mask, G, options(MaxOuterIters=10)


def _solve(pkg, eng, Zs, alg, G):
    _, F, _, out = pkg.cmtf_AOADMM(Zs, alg_options=alg, init=copy.deepcopy(G), engine=eng)
    return F, out


def test_unit_weights_and_alpha_zero_are_the_observed_only_block(pkg, eng):
    rng, Z, mask, G, opt = _limit_setup(pkg, 61)
    _, Zs, w, _ = weighted_models(pkg, Z, 0, mask, rng, 0.0, lambda g, n: np.ones(n))
    Fw, ow = _solve(pkg, eng, Zs, weighted_alg(opt, 1, 0, w, 0.0), G)
    Fb, ob = _solve(pkg, eng, Zs, {**opt, 'hip': {'sparse_observed_only': 1}}, G)
    assert_same_solve(Fb, ob, Fw, ow)
    assert np.allclose(ow['func_rel_missing'][1:], ob['func_rel_missing'][1:], rtol=1e-10, atol=1e-14)


def test_unit_weights_and_alpha_one_are_the_plain_block(pkg, eng):
    rng, Z, mask, G, opt = _limit_setup(pkg, 62)
    _, Zs, w, _ = weighted_models(pkg, Z, 0, mask, rng, 1.0, lambda g, n: np.ones(n))
    Fw, _ = _solve(pkg, eng, Zs, weighted_alg(opt, 1, 0, w, 1.0), G)
    Fp, _ = _solve(pkg, eng, Zs, opt, G)
    for a, b in zip(Fp['fac'], Fw['fac']):
        assert rel_fro(b, a) < 1e-8


def test_zero_weights_make_stored_entries_missing(pkg, eng):
    rng, Z, mask, G, opt = _limit_setup(pkg, 63)
    _, Zs, w, _ = weighted_models(pkg, Z, 0, mask, rng, 0.0, lambda g, n: (g.random(n) >= 0.2).astype(np.float64))
    S = Zs['object'][0]
    assert 0.1 < np.mean(w == 0.0) < 0.3
    Fw, ow = _solve(pkg, eng, Zs, weighted_alg(opt, 1, 0, w, 0.0), G)
    Zk = dict(Zs, object=[pkg.sptensor(S.subs[w > 0], S.vals[w > 0], S.shape)])
    Fb, ob = _solve(pkg, eng, Zk, {**opt, 'hip': {'sparse_observed_only': 1}}, G)
    assert_same_solve(Fb, ob, Fw, ow)
    assert np.allclose(ow['func_rel_missing'][1:], ob['func_rel_missing'][1:], rtol=1e-10, atol=1e-14)


def known_answer_model(pkg):
    """30 x 25 x 20, R = 3, noise-free, non-negative, 30 % kept, a tenth of the kept entries hit by
    + 5 max|X| U(0, 1).  Returns Z (dense, for the reference), Zs, the outlier flags aligned with the sptensor, the
    true factors, the mask and the initial state."""
    rng = np.random.default_rng(11)
    Z, io, A = cp_model((30, 25, 20), 3, rng, [NN] * 3, noise=0.0)
    X = Z['object'][0]
    mask = rng.random(X.shape) < 0.3
    hit = mask & (rng.random(X.shape) < 0.1)
    Xc = np.where(hit, X + 5.0 * np.abs(X).max() * rng.random(X.shape), X)
    Zr = dict(Z, object=[np.where(mask, Xc, 0.0)])
    S = pkg.sptensor(np.argwhere(mask), Xc[mask], X.shape)
    Zs = dict(Z, object=[S])
    G = OA.init_coupled_AOADMM_CMTF({**Zr, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    return Zr, Zs, hit[tuple(S.subs.T)], A, X, mask, G


def test_known_answer_needs_the_weights(pkg, eng):
    """150 iterations.  With weight 0.01 on the outliers the factors are recovered, with unit weights they are not.
    The stepped oracle on these inputs: FMS 0.999608 and relative error 0.0160 on the unstored entries with the weights,
    FMS 0.3964 (error 1.76) without."""
    Zr, Zs, out_flag, A, X, mask, G = known_answer_model(pkg)
    opt = options(MaxOuterIters=150)

    def fit(w):
        F, _ = _solve(pkg, eng, Zs, weighted_alg(opt, 1, 0, w, 0.0), G)
        M = full_ktensor(F['fac'])
        return fms(F['fac'], A), np.linalg.norm((M - X)[~mask]) / np.linalg.norm(X[~mask])

    score, err = fit(np.where(out_flag, 0.01, 1.0))
    score1, err1 = fit(np.ones(len(out_flag)))
    print('weights 0.01 on the outliers: FMS %.6f unstored %.4f; unit weights: FMS %.4f unstored %.3f' % (score, err, score1, err1))
    assert score >= 0.999 and err <= 0.03
    assert score1 < 0.9


# ---- plumbing --------------------------------------------------------------------------------------------------------
def _by_hand(pkg, eng, Zs, G, alg, wsubs, w, alpha, held=None):
    Zs = dict(Zs, _ranks=[int(G['fac'][m].shape[1]) for m in range(len(Zs['size']))])
    pkg.build_model(eng, Zs)
    eng.set_entry_weights(0, wsubs, w, alpha)
    if held is not None:
        eng.set_heldout(0, *held)
    pkg.upload_state(eng, Zs, copy.deepcopy(G))
    out = pkg.run_solver(eng, alg, len(Zs['size']), has_missing=True)
    return pkg.download_state(eng, Zs, copy.deepcopy(G)), out


def _same_bits(Fa, oa, Fb, ob):
    for key in ('fac', 'constraint_fac', 'constraint_dual_fac'):
        for a, b in zip(Fa[key], Fb[key]):
            assert np.array_equal(a, b), key
    for k in ('func_val_conv', 'func_constr_conv', 'func_rel_missing', 'innerIters'):
        assert np.array_equal(oa[k], ob[k], equal_nan=True), k


def test_option_path_by_hand_heldout_and_second_solve(pkg, eng):
    """The options of cmtf_AOADMM equal set_entry_weights by hand with the list in another order; a held-out list on
    the weighted block leaves the solve's bits alone; a second solve on the same engine repeats the first."""
    rng, Z, mask, G, opt = _limit_setup(pkg, 64)
    opt = options(MaxOuterIters=6)
    _, Zs, w, _ = weighted_models(pkg, Z, 0, mask, rng, 0.25)
    S = Zs['object'][0]
    F1, o1 = _solve(pkg, eng, Zs, weighted_alg(opt, 1, 0, w, 0.25), G)
    order = rng.permutation(len(w))
    F2, o2 = _by_hand(pkg, eng, Zs, G, opt, S.subs[order], w[order], 0.25)
    _same_bits(F1, o1, F2, o2)
    pkg.upload_state(eng, Zs, copy.deepcopy(G))              # the same engine again: no snapshot is left over
    o3 = pkg.run_solver(eng, opt, 3, has_missing=True)
    _same_bits(F1, o1, pkg.download_state(eng, Zs, copy.deepcopy(G)), o3)
    hs = np.argwhere(~mask)[:200]
    F4, o4 = _solve(pkg, eng, Zs, weighted_alg(opt, 1, 0, w, 0.25, heldout={1: (hs, np.asarray(Z['object'][0])[tuple(hs.T)])}), G)
    _same_bits(F1, o1, F4, o4)
    assert 1 in o4['func_heldout']


def test_bytes_and_unmarking(pkg, eng):
    """A weight list adds 8 N nnz bytes to the marked block (alpha alone adds none); unmarking drops the weights: the
    plain MTTKRP's bits come back; marking again keeps the weights of a weighted block."""
    rng = np.random.default_rng(65)
    shape, R = OP_SHAPES[3], 5
    N = len(shape)
    subs, vals, X, stored = stored_entries(rng, shape)
    raw_block(pkg, eng, shape, R, subs, vals)
    nnz = int(stored.sum())
    F = signed(rng, shape, R)
    put_factors(pkg, eng, shape, F)
    plain = [eng.resident_mttkrp(0, n, shape[n], R) for n in range(N)]
    eng.set_observed_only(0)
    marked = eng.tensor_storage_info(0)[2]
    wsubs, wts = weight_list(rng, stored)
    eng.set_entry_weights(0, wsubs, wts, 0.25)
    assert eng.tensor_storage_info(0)[2] == marked + 8 * N * nnz
    weighted = [eng.resident_mttkrp(0, n, shape[n], R) for n in range(N)]
    assert not np.array_equal(weighted[0], plain[0])
    eng.set_observed_only(0)                                 # marked again: the weights stay
    assert eng.tensor_storage_info(0)[2] == marked + 8 * N * nnz
    for n in range(N):
        assert np.array_equal(eng.resident_mttkrp(0, n, shape[n], R), weighted[n])
    eng.set_entry_weights(0, None, None, 0.25)               # alpha alone: stored weights 1, no weight arrays
    assert eng.tensor_storage_info(0)[2] == marked
    for n in range(N):
        assert np.array_equal(eng.resident_mttkrp(0, n, shape[n], R), plain[n])
    eng.set_entry_weights(0, wsubs, wts, 0.25)
    eng.set_observed_only(0, False)
    assert eng.tensor_storage_info(0)[2] == N * (4 * N + 8) * nnz
    for n in range(N):
        assert np.array_equal(eng.resident_mttkrp(0, n, shape[n], R), plain[n])
    with pytest.raises(pkg.UnsupportedOnDevice):
        eng.em_step(0)
    # kernel statistics: every pass streams 8 more bytes per entry
    eng.set_entry_weights(0, wsubs, wts, 0.25)
    for which in [3] + [4 + n for n in range(N)]:
        eng.kernel_stats(which, reset=True)
    eng.em_step(0)
    assert eng.kernel_stats(3)[2] == N * nnz * (4 * N + 24 + 8 * N * R)
    assert [eng.kernel_stats(4 + n)[2] for n in range(N)] == [nnz * (4 * N + 24 + 8 * N * R)] * N


def test_two_ranks_replicated_block(pkg, eng):
    rng, Z, mask, G, opt = _limit_setup(pkg, 66)
    opt = options(MaxOuterIters=6)
    _, Zs, w, _ = weighted_models(pkg, Z, 0, mask, rng, 0.1)
    alg = weighted_alg(opt, 1, 0, w, 0.1)
    F1, o1 = _solve(pkg, eng, Zs, alg, G)
    for F2, o2 in on_ranks(pkg, 2, lambda e, r: _solve(pkg, e, Zs, alg, G)):
        _same_bits(F1, o1, F2, o2)


def test_refusals_leave_the_block_as_it_was(pkg, eng):
    rng = np.random.default_rng(67)
    shape, R = OP_SHAPES[3], 4
    N = len(shape)
    subs, vals, X, stored = stored_entries(rng, shape)
    raw_block(pkg, eng, shape, R, subs, vals)
    wsubs, wts = weight_list(rng, stored)
    eng.set_entry_weights(0, wsubs, wts, 0.25)
    F = signed(rng, shape, R)
    put_factors(pkg, eng, shape, F)
    eng.em_step(0)
    before = [eng.resident_mttkrp(0, n, shape[n], R) for n in range(N)]
    bytes_before = eng.tensor_storage_info(0)[2]

    def change(i, v):
        w = wts.copy()
        w[i] = v
        return w

    unstored = wsubs.copy()
    unstored[5] = np.argwhere(~stored)[7]                    # same count, one entry the block does not store
    dup = wsubs.copy()
    dup[9] = dup[10]                                         # a duplicate, so another entry is left out
    bad = [(wsubs, change(3, 1.5), 0.25), (wsubs, change(3, -0.25), 0.25), (wsubs, change(3, np.nan), 0.25),
           (wsubs, change(3, np.inf), 0.25), (wsubs, wts, 1.5), (wsubs, wts, -0.1), (wsubs, wts, np.nan),
           (unstored, wts, 0.25), (dup, wts, 0.25), (wsubs[:-1], wts[:-1], 0.25),
           (np.vstack([wsubs, wsubs[:1]]), np.append(wts, 0.5), 0.25), (None, None, 2.0)]
    oob = wsubs.copy()
    oob[0, 1] = shape[1]
    bad.append((oob, wts, 0.25))
    for s, w, a in bad:
        with pytest.raises(pkg.AoadmmError) as ei:
            eng.set_entry_weights(0, s, w, a)
        assert ei.value.code == capi.ERR_INVALID, (w is None, a)
        assert eng.tensor_storage_info(0)[2] == bytes_before
        for n in range(N):
            assert np.array_equal(eng.resident_mttkrp(0, n, shape[n], R), before[n])
    # blocks the call is not for
    pkg.build_model(eng, cp_Z(shape, 3, rng.random(shape)))
    with pytest.raises(pkg.UnsupportedOnDevice, match='dense'):
        eng.set_entry_weights(0, None, None, 0.5)
    Zp, _ = script4_model(rng, K=4)
    Zp = dict(Zp, _ranks=[3, 3, 3])
    Zp['object'] = [[pkg.sptensor(np.argwhere(np.abs(Xk) > 0.01), Xk[np.abs(Xk) > 0.01], Xk.shape) for Xk in Zp['object'][0]]]
    pkg.build_model(eng, Zp)
    with pytest.raises(pkg.UnsupportedOnDevice, match='PARAFAC2'):
        eng.set_entry_weights(0, None, None, 0.5)
    S = pkg.sptensor(np.argwhere(stored), X[stored], shape)

    def rank_fn(e, r):
        pkg.build_model(e, cp_Z(shape, 3, S), sparse_sharding=True)
        with pytest.raises(pkg.UnsupportedOnDevice, match='sharded'):
            e.set_entry_weights(0, None, None, 0.5)
        return True

    assert on_ranks(pkg, 2, rank_fn) == [True, True]
    with pkg.Engine([0, 0]) as e2:
        pkg.build_model(e2, cp_Z(shape, 3, S))
        with pytest.raises(pkg.UnsupportedOnDevice, match='multi-device'):
            e2.set_entry_weights(0, None, None, 0.5)
    # the driver refuses the options together with sharding before anything reaches the device
    G = {'fac': [rng.random((s, 3)) for s in shape], 'coupling_fac': []}
    with pytest.raises(pkg.UnsupportedOnDevice, match='sparse_sharding'):
        pkg.cmtf_AOADMM(cp_Z(shape, 3, S), alg_options={**options(), 'hip': {'sparse_sharding': 1, 'sparse_unstored_weight': [0.5]}},
                        init=G, engine=eng)
