"""GPU: masked dense CP blocks imputed from the list of their missing entries (`Engine.set_missing_list`, csrc/em_list.hip,
DESIGN.md section 4.5.2).

1. The list: built on the device from the resident bit mask, it must equal np.nonzero(~mask) in column-major order
   exactly, at every edge of its construction (word, workgroup, team and padding boundaries, empty and full columns).
2. The list pass at kernel level (`Engine.resident_em_list_pass`, the solver's own enqueue) against the longdouble
   reference and the bounds of tests/em_ref.py.  The pass forms m in fp64 and rounds once, which lies inside beta; its sums
   run over four fp64 accumulators of at most 64 entries each per team, two adds, a strided sum of the teams' partials
   (at most 2 per thread at these sizes) and an 8-level tree: inside em_ref's 80 u.
3. Solves: marked blocks against the oracle at the bars of tests/test_gpu_solver.py, and against the same solve unmarked.
   The objective of a marked block is combined from cancelled terms, so later values are compared at the bar
   tests/test_gpu_objective.py uses for those, 1e-12 x scale, with scale taken as w * ||miss .* X||^2 <= w * (||Xhat||^2 +
   2 |dot| + ||M||^2): a smaller scale than the bar allows, never a larger one.  Noisy models only (section 4.5.2).
4. Plumbing: the option, the kernel-statistics class, the storage figure, every refusal, and what drops the mark.

Observed on an MI355X (largest over all cases of this file; every case prints its own): imputed value 0.44 of beta, num
0.019 and den 0.039 of their bounds (fp64 storage; fp32 storage below 1e-10 of them); marked against unmarked solves:
factors 5.4e-15, objective differences 5.1e-16 against a bar of 8e-13."""
import copy
import functools
import importlib
import os
import threading

import numpy as np
import pytest

import em_ref
from helpers import cp_model, options, rel_fro, script3_model
from oracle import aoadmm as OA
from test_gpu_solver import _compare_em, _with_mask, compare, run_both

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')
KSTAT_EM_PASS, KSTAT_EM_LIST = 4, 16
PRECS = ['f64', 'f32']


def _cdiv(a, b):
    return -(-a // b)


def _pad(prec, n):
    q = 2 if prec == 'f64' else 4
    return _cdiv(n, q) * q


def _block(dims, R, X, obs=None):
    n = len(dims)
    Z = dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(dims),
             coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
             constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[X], _ranks=[R] * n)
    if obs is not None:
        Z['miss'] = [obs.astype(np.uint8)]
    return Z


def _expected_subs(obs):
    flat = np.flatnonzero(~obs.ravel(order='F'))
    return np.stack(np.unravel_index(flat, obs.shape, order='F'), axis=1).astype(np.int64).reshape(-1, obs.ndim)


def _list_bytes(nd, n):
    return 4 * nd * n + 16 * _cdiv(n, 256) if n else 0


# ---- 1. the list --------------------------------------------------------------------------------------------------------
def _check_list(pkg, eng, obs, prec):
    dims = obs.shape
    X = np.asfortranarray(np.arange(1, obs.size + 1, dtype=np.float64).reshape(dims, order='F'))
    pkg.build_model(eng, _block(dims, 2, X, obs), prec)
    eng.set_missing_list(0)
    want = _expected_subs(obs)
    assert eng.missing_list(0) == want.shape[0]
    got = eng.missing_list(0, len(dims))
    assert got.shape == want.shape and np.array_equal(got, want)


def _storage_offsets_mask(dims, prec, offsets):
    """Missing exactly at the given storage offsets of the padded layout (those that fall on a padding row are left
    out) and at the last entry of the array."""
    obs = np.ones(dims, dtype=bool)
    Ipad, cols = _pad(prec, dims[0]), int(np.prod(dims[1:]))
    o2 = obs.reshape(dims[0], cols, order='F')
    for off in offsets:
        i, c = off % Ipad, off // Ipad
        if i < dims[0] and c < cols:
            o2[i, c] = False
    o2[-1, -1] = False
    return np.asfortranarray(o2.reshape(dims, order='F'))


SHAPES = [(5, 3), (37, 22, 19), (33, 4, 3, 2), (7, 3, 2, 2, 3)]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('dims', SHAPES)
def test_list_equals_the_mask_random_and_edge_offsets(pkg, eng, dims, prec):
    rng = np.random.default_rng(sum(dims))
    _check_list(pkg, eng, np.asfortranarray(rng.random(dims) >= 0.3), prec)
    _check_list(pkg, eng, _storage_offsets_mask(dims, prec, (0, 7, 8, 63, 64)), prec)
    col = np.ones(dims, dtype=bool)
    col[:, 1] = False                                            # an all-missing column (every trailing index)
    _check_list(pkg, eng, np.asfortranarray(col), prec)
    _check_list(pkg, eng, np.ones(dims, dtype=bool), prec)       # n = 0
    _check_list(pkg, eng, np.zeros(dims, dtype=bool), prec)      # everything missing: no cap on the share


@pytest.mark.parametrize('count', [1, 255, 256, 257, 2047, 2048, 2049])
def test_list_counts_at_team_and_workgroup_edges(pkg, eng, count):
    dims = (37, 22, 19)
    obs = np.ones(dims, dtype=bool)
    obs.flat[np.random.default_rng(count).choice(obs.size, count, replace=False)] = False
    _check_list(pkg, eng, np.asfortranarray(obs), 'f32')


def test_list_longer_than_the_finishers_stride(pkg, eng):
    dims = (64, 48, 32)
    obs = np.asfortranarray(np.random.default_rng(9).random(dims) >= 0.7)
    assert (~obs).sum() > 65536
    _check_list(pkg, eng, obs, 'f32')


# ---- 2. the pass ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _data(dims, R):
    X, U = em_ref.make_data(dims, R, np.random.default_rng(1000 * sum(dims) + 7 * len(dims) + R))
    M = em_ref.model(U)
    for a in [X, M] + U:
        a.setflags(write=False)
    return X, U, M


@functools.lru_cache(maxsize=2)
def _ref(dims, R, frac):
    X, U, M = _data(dims, R)
    obs = np.random.default_rng(int(frac * 1e6) + sum(dims)).random(dims) >= frac
    return em_ref.EmRef(X, np.asfortranarray(obs), U, M=M)


def _marked(pkg, eng, ref, dims, R, prec):
    Z = _block(dims, R, np.asfortranarray(ref.X), ref.obs)
    pkg.build_model(eng, Z, prec)
    eng.set_missing_list(0)
    pkg.upload_state(eng, Z, dict(fac=list(ref.U)))


def _run_pass(pkg, eng, dims, R, prec, frac=0.2):
    ref = _ref(dims, R, frac)
    X, obs = ref.X, ref.obs
    _marked(pkg, eng, ref, dims, R, prec)
    still = eng.resident_em_list_pass(0, dims, update=0)
    assert np.array_equal(still['data'], X)                      # update = 0 leaves the data alone
    out = eng.resident_em_list_pass(0, dims, update=1)
    assert np.array_equal(still['stats'], out['stats'])          # and returns the sums the update returns
    stats4 = np.array([out['stats'][0], out['stats'][1], ref.stats[2], ref.stats[3]])
    rs = ref.stat_ratios(stats4, prec)
    re = ref.entry_ratio(out['data'], prec)
    print('list pass %s R=%d %s: entry %.3g of beta, num %.3g den %.3g of their bounds' % (dims, R, prec, re, rs[0], rs[1]))
    assert np.array_equal(out['data'][obs], X[obs])              # bitwise: X holds fp32 values
    assert re <= 1.0, re
    assert ref.stats[1] > 0 and out['stats'][1] > 0              # the non-zero values under the mask enter den
    assert rs[0] <= 1.0 and rs[1] <= 1.0, rs
    if len(dims) == 2:
        assert np.array_equal(out['data_t'], out['data'].T)
    _marked(pkg, eng, ref, dims, R, prec)                        # a second call on a fresh upload: the same bits
    again = eng.resident_em_list_pass(0, dims, update=1)
    assert np.array_equal(again['stats'], out['stats']) and np.array_equal(again['data'], out['data'])
    return out


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R', [1, 4, 5, 8, 9, 16, 17, 20, 32, 33, 64])
def test_pass_both_ends_of_every_team_width(pkg, eng, R, prec):
    _run_pass(pkg, eng, (37, 22, 19), R, prec)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('dims,R', [((30, 26), 3), ((30, 26), 33), ((12, 9, 8, 7), 5), ((12, 9, 8, 7), 20),
                                    ((7, 5, 4, 3, 6), 2), ((7, 5, 4, 3, 6), 9)])
def test_pass_orders_two_four_and_five(pkg, eng, dims, R, prec):
    _run_pass(pkg, eng, dims, R, prec)


@pytest.mark.parametrize('prec', PRECS)
def test_pass_with_an_empty_list_is_exactly_zero(pkg, eng, prec):
    dims, R = (37, 22, 19), 5
    X, U, M = _data(dims, R)
    ref = em_ref.EmRef(X, np.ones(dims, dtype=bool), U, M=M)
    _marked(pkg, eng, ref, dims, R, prec)
    eng.kernel_stats(KSTAT_EM_LIST, reset=True)
    out = eng.resident_em_list_pass(0, dims, update=1)
    assert out['stats'][0] == 0.0 and out['stats'][1] == 0.0
    assert np.array_equal(out['data'], X)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('dims', [(9, 7), (9, 7, 5)])
def test_pass_exact_case(pkg, eng, dims, prec):
    """Small-integer factors and data: every product, sum and square is exact in either precision."""
    rng = np.random.default_rng(3)
    R = 3
    U = [rng.integers(-2, 3, (n, R)).astype(np.float64) for n in dims]
    X = np.asfortranarray(rng.integers(-5, 6, dims).astype(np.float64))
    obs = np.asfortranarray(rng.random(dims) >= 0.3)
    ref = em_ref.EmRef(X, obs, U)
    _marked(pkg, eng, ref, dims, R, prec)
    out = eng.resident_em_list_pass(0, dims, update=1)
    assert np.array_equal(out['data'], ref.X_new)
    assert out['stats'][0] == ref.stats[0] and out['stats'][1] == ref.stats[1]
    if len(dims) == 2:
        assert np.array_equal(out['data_t'], ref.X_new.T)


# ---- 3. solves -------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=['one-launch', 'tensor-pass'])
def mttkrp_path(request):
    if request.param == 'tensor-pass':
        os.environ['AOADMM_NO_SMALL_MTTKRP'] = '1'
    yield request.param
    os.environ.pop('AOADMM_NO_SMALL_MTTKRP', None)


def _three_runs(pkg, eng, Z, io, opt, marked=1, precision='f64'):
    """(oracle, unmarked, marked) solves from one starting point."""
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, Fo, _, oo = OA.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G))
    _, Fu, _, ou = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=eng, precision=precision)
    _, Fm, _, om = pkg.cmtf_AOADMM(Z, alg_options={**opt, 'hip': {'missing_list': marked}}, init=copy.deepcopy(G), engine=eng,
                                   precision=precision)
    return (Fo, oo), (Fu, ou), (Fm, om)


def _scale(Z):
    """sum_p w_p ||miss_p .* X_p||^2: a lower bound of the cancelled terms' magnitude (module docstring)."""
    return sum(float(w) * float((np.asarray(X)[np.asarray(m, dtype=bool)] ** 2).sum())
               for w, X, m in zip(Z['weights'], Z['object'], Z['miss']))


def _check_marked(Z, runs, tol=1e-8):
    (Fo, oo), (Fu, ou), (Fm, om) = runs
    compare(Fo, oo, Fm, om, tol)
    _compare_em(oo, om)
    worst = max(rel_fro(b, a) for a, b in zip(Fu['fac'], Fm['fac']))
    dv = np.abs(np.asarray(om['func_val_conv']) - np.asarray(ou['func_val_conv']))
    print('marked against unmarked: factors %.3g, objective differences up to %.3g (bar %.3g)' % (worst, dv[1:].max(), 1e-12 * _scale(Z)))
    assert worst < 1e-10, worst
    assert om['func_val_conv'][0] == ou['func_val_conv'][0]      # the dense statistics pass: the same bits
    assert np.all(dv[1:] <= 1e-12 * _scale(Z)), dv


@pytest.mark.parametrize('frac', [0.2, 0.01])
def test_solve_cp_tv_nonneg(pkg, eng, mttkrp_path, frac):
    rng = np.random.default_rng(31)
    Z, io, _ = cp_model((37, 22, 19), 3, rng, [('non-negativity',), ('non-negativity',), ('TV regularization', 1e-3)])
    Z = _with_mask(Z, rng, frac)
    _check_marked(Z, _three_runs(pkg, eng, Z, io, options(MaxOuterIters=12)))


def test_solve_matrix(pkg, eng, mttkrp_path):
    rng = np.random.default_rng(32)
    Z, io, _ = cp_model((30, 26), 3, rng, [('non-negativity',), None])
    Z = _with_mask(Z, rng, 0.1)
    _check_marked(Z, _three_runs(pkg, eng, Z, io, options(MaxOuterIters=12)))


def test_solve_four_way(pkg, eng, mttkrp_path):
    rng = np.random.default_rng(91)
    Z, io, _ = cp_model((12, 9, 8, 7), 3, rng, [('non-negativity',), None, ('l2-ball', 1.0), ('non-negativity',)])
    Z = _with_mask(Z, rng)
    _check_marked(Z, _three_runs(pkg, eng, Z, io, options(MaxOuterIters=10)))


def test_solve_marked_block_coupled_with_an_unmarked_masked_one(pkg, eng, mttkrp_path):
    rng = np.random.default_rng(37)
    Z, io = script3_model(rng)[:2]
    Z = _with_mask(Z, rng)
    _check_marked(Z, _three_runs(pkg, eng, Z, io, options(MaxOuterIters=10), marked=[1]))


def test_solve_fp32_storage(pkg, eng, mttkrp_path):
    """The bars test_em_fused_contraction_of_the_second_mode uses for fp32."""
    rng = np.random.default_rng(36)
    Z, io, _ = cp_model((45, 150, 21), 6, rng, [('non-negativity',)] * 3)
    Z = _with_mask(Z, rng)
    (Fo, oo), _, (Fm, om) = _three_runs(pkg, eng, Z, io, options(MaxOuterIters=5), precision='f32')
    for a, b in zip(Fo['fac'], Fm['fac']):
        assert rel_fro(b, a) < 1e-4
    assert np.allclose(om['func_rel_missing'][1:], oo['func_rel_missing'][1:], rtol=1e-3)


def test_solve_stops_on_the_rel_missing_rule_at_the_oracles_iteration(pkg, eng, mttkrp_path):
    """f_rel_missing < OuterRelTol (:457-459) is the last rule to hold: the objective's own rule holds earlier."""
    rng = np.random.default_rng(33)
    Z, io, _ = cp_model((30, 26), 3, rng, [None, None])
    Z = _with_mask(Z, rng, 0.3)                    # (the oracle stops after 31 iterations; the precondition below says why)
    tol = 1e-3
    (Fo, oo), _, (Fm, om) = _three_runs(pkg, eng, Z, io, options(MaxOuterIters=400, OuterRelTol=tol))
    it = oo['OuterIterations']
    f = np.asarray(oo['func_val_conv'])
    assert 1 < it < 400 and om['OuterIterations'] == it
    assert abs(f[it - 2] - f[it - 1]) / f[it - 2] < tol <= oo['func_rel_missing'][it - 1], 'precondition: the rule under test decided'
    for a, b in zip(Fo['fac'], Fm['fac']):
        assert rel_fro(b, a) < 1e-8
    _compare_em(oo, om)


def test_solve_with_an_empty_list_equals_the_unmasked_solve(pkg, eng, mttkrp_path):
    rng = np.random.default_rng(41)
    Z, io, _ = cp_model((37, 22, 19), 3, rng, [('non-negativity',)] * 3)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    opt = options(MaxOuterIters=8)
    _, Fp, _, op = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=eng)
    Zm = dict(Z, miss=[np.ones((37, 22, 19), dtype=bool)])
    _, Fm, _, om = pkg.cmtf_AOADMM(Zm, alg_options={**opt, 'hip': {'missing_list': 1}}, init=copy.deepcopy(G), engine=eng)
    assert eng.missing_list(0) == 0
    for a, b in zip(Fp['fac'], Fm['fac']):
        assert rel_fro(b, a) < 1e-10
    assert np.allclose(om['func_val_conv'], op['func_val_conv'], rtol=0, atol=1e-12 * _scale(Zm))


def test_keep_best_restore_on_a_marked_block(pkg, eng, mttkrp_path):
    """The restore re-imputes the block from the restored factors: through the list, with the unmarked run's result."""
    rng = np.random.default_rng(43)
    dims, R = (37, 22, 19), 3
    Z, io, _ = cp_model(dims, R, rng, [('non-negativity',)] * 3)
    Z = _with_mask(Z, rng)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    subs = _expected_subs(np.asarray(Z['miss'][0], dtype=bool))[::7]
    pkg.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=3), init=copy.deepcopy(G), engine=eng)
    y = eng.model_at(0, subs)                                    # the held-out sum is smallest (zero) at iteration 3
    res = []
    for hip in ({}, {'missing_list': 1}):
        hip = dict(hip, heldout={1: (subs, y)}, heldout_keep_best=1)
        _, F, _, out = pkg.cmtf_AOADMM(Z, alg_options={**options(MaxOuterIters=8), 'hip': hip}, init=copy.deepcopy(G), engine=eng)
        assert out['heldout_restored_iter'] == 3
        res.append((F, eng.resident_em_pass(0, dims, R, update=0)['data']))
    for a, b in zip(res[0][0]['fac'], res[1][0]['fac']):
        assert rel_fro(b, a) < 1e-10
    assert rel_fro(res[1][1], res[0][1]) < 1e-10


# ---- 4. plumbing -----------------------------------------------------------------------------------------------------------
def _small_masked(rng, dims=(13, 9, 7), R=3):
    Z, io, _ = cp_model(dims, R, rng, [('non-negativity',)] * len(dims))
    Z = _with_mask(Z, rng)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    return dict(Z, _ranks=[R] * len(dims)), G


def test_option_equals_the_call_by_hand(pkg, eng):
    Z, G = _small_masked(np.random.default_rng(51))
    opt = options(MaxOuterIters=4)
    _, Fa, _, oa = pkg.cmtf_AOADMM(Z, alg_options={**opt, 'hip': {'missing_list': [1]}}, init=copy.deepcopy(G), engine=eng)
    want = _expected_subs(np.asarray(Z['miss'][0], dtype=bool))
    assert np.array_equal(eng.missing_list(0, 3), want)
    pkg.build_model(eng, Z, 'f64')
    eng.set_missing_list(0, True)
    pkg.upload_state(eng, Z, copy.deepcopy(G))
    ob = pkg.run_solver(eng, opt, len(Z['size']), has_missing=True)
    Fb = pkg.download_state(eng, Z, G)
    for a, b in zip(Fa['fac'], Fb['fac']):
        assert np.array_equal(a, b)
    assert np.array_equal(oa['func_val_conv'], ob['func_val_conv'])
    pkg.build_model(eng, Z, 'f64', missing_list=1)               # build_model's own argument
    assert eng.missing_list(0) == want.shape[0]
    pkg.build_model(eng, Z, 'f64')                               # and without it the block is not marked
    with pytest.raises(capi.AoadmmError):
        eng.missing_list(0)


def test_kernel_stats_class_and_storage_info(pkg, eng):
    dims, R = (37, 22, 19), 5
    ref = _ref(dims, R, 0.2)
    n = int((~ref.obs).sum())
    Z = _block(dims, R, np.asfortranarray(ref.X), ref.obs)
    pkg.build_model(eng, Z, 'f32')
    before = eng.tensor_storage_info(0)[2]
    eng.set_missing_list(0)
    assert eng.tensor_storage_info(0)[2] == before + _list_bytes(3, n)
    pkg.upload_state(eng, Z, dict(fac=list(ref.U)))
    eng.kernel_stats(KSTAT_EM_LIST, reset=True)
    eng.kernel_stats(KSTAT_EM_PASS, reset=True)
    eng.resident_em_list_pass(0, dims, update=1, with_data=False)
    eng.resident_em_list_pass(0, dims, update=0, with_data=False)
    ms, launches, nbytes, flops = eng.kernel_stats(KSTAT_EM_LIST)
    assert launches == 2 and ms > 0
    per = n * (4 * 3 + 8 * 3 * R + 4)                            # subscripts, factor rows, the value read (fp32)
    assert nbytes == 2 * per + 4 * n and flops == 2 * (n * R * 3 + 8 * n)
    assert eng.kernel_stats(KSTAT_EM_PASS)[1] == 0               # no dense pass ran
    with pytest.raises(capi.UnsupportedOnDevice):                # the dense imputing pass is not a marked block's
        eng.resident_em_pass(0, dims, R, update=1)
    eng.set_missing_list(0, False)
    assert eng.tensor_storage_info(0)[2] == before
    with pytest.raises(capi.AoadmmError) as ei:
        eng.resident_em_list_pass(0, dims)
    assert ei.value.code == capi.ERR_INVALID


def _code(fn):
    with pytest.raises(capi.AoadmmError) as ei:
        fn()
    return ei.value.code


def test_refusals(pkg, eng):
    rng = np.random.default_rng(52)
    Z, G = _small_masked(rng)
    plain = {k: v for k, v in Z.items() if k != 'miss'}
    pkg.build_model(eng, plain, 'f64')
    assert _code(lambda: eng.set_missing_list(0)) == capi.ERR_INVALID            # no mask
    W = rng.random((13, 9, 7))
    pkg.build_model(eng, Z, 'f64', dense_entry_weights=[W])
    assert _code(lambda: eng.set_missing_list(0)) == capi.ERR_UNSUPPORTED        # weighted
    X = np.where(rng.random((13, 9, 7)) < 0.2, 1.0, 0.0)
    pkg.build_model(eng, dict(plain, object=[pkg.sptensor(np.argwhere(X != 0), X[X != 0], X.shape)]), 'f64')
    assert _code(lambda: eng.set_missing_list(0)) == capi.ERR_UNSUPPORTED        # sparse
    from helpers import script1_model
    Zp = script1_model(np.random.default_rng(53))[0]
    p2 = Zp['model'].index('PAR2')
    ranks = [3] * len(Zp['size'])
    pkg.build_model(eng, dict(Zp, _ranks=ranks), 'f64')
    assert _code(lambda: eng.set_missing_list(p2)) == capi.ERR_UNSUPPORTED       # PARAFAC2
    # the driver refuses before anything is uploaded
    opt = {**options(MaxOuterIters=1), 'hip': {'missing_list': [1], 'entry_weights': [W]}}
    with pytest.raises(capi.UnsupportedOnDevice):
        pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=eng)
    with pytest.raises(ValueError):
        pkg.cmtf_AOADMM(plain, alg_options={**options(MaxOuterIters=1), 'hip': {'missing_list': [1]}}, init=copy.deepcopy(G), engine=eng)


def test_refused_under_a_communicator_and_on_a_multi_device_context(pkg):
    Z, G = _small_masked(np.random.default_rng(54))
    world, key = 2, 7100 + os.getpid() % 1000
    codes, err = [None] * world, [None] * world

    def rank_main(r):
        try:
            with pkg.Engine(0) as e:
                e.comm_init_local(key, r, world)
                pkg.build_model(e, Z, 'f64')
                codes[r] = _code(lambda: e.set_missing_list(0))
                with pytest.raises(capi.UnsupportedOnDevice):    # and the driver, before it uploads anything
                    pkg.build_model(e, Z, 'f64', missing_list=1)
        except BaseException as ex:   # noqa: BLE001 -- reported by the main thread
            err[r] = ex

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert err == [None] * world, err
    assert codes == [capi.ERR_UNSUPPORTED] * world
    with pkg.Engine([0, 0]) as e:
        pkg.build_model(e, Z, 'f64')
        assert _code(lambda: e.set_missing_list(0)) == capi.ERR_UNSUPPORTED


def test_uploads_drop_the_mark(pkg, eng):
    rng = np.random.default_rng(55)
    Z, G = _small_masked(rng)
    X, mk = capi.as_f(Z['object'][0]), np.asfortranarray(np.asarray(Z['miss'][0]) != 0, dtype=np.uint8)
    import ctypes as C

    def marked():
        pkg.build_model(eng, Z, 'f64')
        eng.set_missing_list(0)
        assert eng.missing_list(0) == int((mk == 0).sum())

    marked()
    capi.check(eng.lib.aoadmm_tensor_mask_upload(eng.h, 0, mk.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert _code(lambda: eng.missing_list(0)) == capi.ERR_INVALID
    marked()
    capi.check(eng.lib.aoadmm_tensor_upload(eng.h, 0, capi.dptr(X), capi.precision_id('f64')))
    assert _code(lambda: eng.missing_list(0)) == capi.ERR_INVALID
    marked()
    eng.tensor_weights_upload(0, rng.random(X.shape))
    assert _code(lambda: eng.missing_list(0)) == capi.ERR_INVALID
