"""GPU: weighted least squares on dense CP blocks (`alg_options['hip']['entry_weights']` -> aoadmm_tensor_weights_upload,
DESIGN.md section 4.5.1) against the oracle stepped one outer iteration at a time (tests/weighted_ref.py::stepped_em).
Bars: the project's whole-solve bars (test_gpu_solver.compare / _compare_em): factors and duals 1e-8, innerIters equal,
traces rtol 1e-7."""
import copy
import itertools
import threading

import numpy as np
import pytest

from oracle import aoadmm as OA
from oracle.tensor_ops import full_ktensor
from helpers import cp_cp_exact_model, cp_model, options, rel_fro
from test_gpu_solver import _compare_em, _with_mask, compare
from test_gpu_sparse_observed import fms
from weighted_ref import stepped_em

pytestmark = pytest.mark.gpu

NN = ('non-negativity',)
_keys = itertools.count(7000)


def weights_for(shape, rng):
    """Uniform on the multiples of 1/256, a tenth of the entries at 0."""
    W = rng.integers(0, 257, size=shape).astype(np.float64) / 256.0
    W[rng.random(shape) < 0.1] = 0.0
    return W


def _init(Z, io, seed=7):
    return OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(seed))


def _hip(Z, W):
    return dict(entry_weights=[W.get(p) for p in range(len(Z['object']))])


def run_both(pkg, eng, Z, io, W, iters, precision='f64'):
    """W: {0-based block: weights}.  (Fo, oo) from stepped_em, (Fg, og) from the device."""
    G = _init(Z, io)
    opt = options(MaxOuterIters=iters)
    Fo, oo = stepped_em(Z, W, copy.deepcopy(G), opt, iters)
    _, Fg, _, og = pkg.cmtf_AOADMM(Z, alg_options=dict(opt, hip=_hip(Z, W)), init=copy.deepcopy(G), engine=eng,
                                   precision=precision)
    return Fo, oo, Fg, og


CASES = {
    '3-way': ((40, 30, 20), 3, [NN, NN, NN], 12),
    '3-way-tv': ((40, 30, 20), 3, [None, None, ('TV regularization', 1e-3)], 12),
    'matrix': ((30, 25), 4, [NN, NN], 12),
    '4-way': ((12, 10, 9, 8), 3, [None] * 4, 8),
    'long-mode': ((300, 40, 30), 20, [None] * 3, 5),
}


@pytest.mark.parametrize('case', list(CASES))
def test_weighted_solve_is_the_stepped_oracle(pkg, eng, case):
    shape, R, constraints, iters = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    Z, io, _ = cp_model(shape, R, rng, constraints)
    W = {0: weights_for(shape, rng)}
    Fo, oo, Fg, og = run_both(pkg, eng, Z, io, W, iters)
    compare(Fo, oo, Fg, og)
    _compare_em(oo, og)


def test_weighted_block_coupled_to_a_plain_one(pkg, eng):
    rng = np.random.default_rng(41)
    Z, io = cp_cp_exact_model(rng)
    W = {0: weights_for(np.shape(Z['object'][0]), rng)}
    Fo, oo, Fg, og = run_both(pkg, eng, Z, io, W, 8)
    compare(Fo, oo, Fg, og)
    _compare_em(oo, og)


def test_fp32_storage(pkg, eng):
    """The bars test_em_fused_contraction_of_the_second_mode holds the masked fp32 path to."""
    rng = np.random.default_rng(36)
    shape = (45, 150, 21)
    Z, io, _ = cp_model(shape, 6, rng, [NN] * 3)
    Fo, oo, Fg, og = run_both(pkg, eng, Z, io, {0: weights_for(shape, rng)}, 5, precision='f32')
    for a, b in zip(Fo['fac'], Fg['fac']):
        assert rel_fro(b, a) < 1e-4, rel_fro(b, a)
    assert np.allclose(og['func_rel_missing'][1:], oo['func_rel_missing'][1:], rtol=1e-3)


def _solve(pkg, eng, Z, G, iters, hip=None, **kw):
    opt = options(MaxOuterIters=iters)
    if hip is not None:
        opt = dict(opt, hip=hip)
    _, F, _, out = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=eng, **kw)
    return F, out


def test_unit_weights_are_the_plain_solve(pkg, eng):
    rng = np.random.default_rng(51)
    shape = (40, 30, 20)
    Z, io, _ = cp_model(shape, 3, rng, [NN] * 3)
    G = _init(Z, io)
    Fp, op = _solve(pkg, eng, Z, G, 10)
    Fw, ow = _solve(pkg, eng, Z, G, 10, hip=dict(entry_weights=[np.ones(shape)]))
    for a, b in zip(Fp['fac'], Fw['fac']):
        assert rel_fro(b, a) < 1e-8, rel_fro(b, a)
    assert np.allclose(ow['func_val_conv'], op['func_val_conv'], rtol=1e-7, atol=1e-10)
    assert np.all(ow['func_rel_missing'][1:] == 0)


def test_boolean_weights_are_the_masked_solve(pkg, eng):
    """The two differ by the fused contraction of the masked path, so 1e-8 and not bitwise."""
    rng = np.random.default_rng(52)
    Z, io, _ = cp_model((40, 30, 20), 3, rng, [NN] * 3)
    Zm = _with_mask(Z, rng)
    G = _init(Zm, io)
    Fm, om = _solve(pkg, eng, Zm, G, 10)
    Fw, ow = _solve(pkg, eng, dict(Zm, miss=None), G, 10, hip=dict(entry_weights=[Zm['miss'][0].astype(np.float64)]))
    for a, b in zip(Fm['fac'], Fw['fac']):
        assert rel_fro(b, a) < 1e-8, rel_fro(b, a)
    assert np.allclose(ow['func_val_conv'], om['func_val_conv'], rtol=1e-7, atol=1e-10)
    assert np.allclose(ow['func_rel_missing'][1:], om['func_rel_missing'][1:], rtol=1e-7, atol=1e-12)


def test_mask_and_weights_together_are_their_product(pkg, eng):
    rng = np.random.default_rng(53)
    shape = (40, 30, 20)
    Z, io, _ = cp_model(shape, 3, rng, [NN] * 3)
    W = weights_for(shape, rng)
    mask = rng.random(shape) < 0.8
    G = _init(Z, io)
    Fa, oa = _solve(pkg, eng, dict(Z, miss=[mask]), G, 6, hip=dict(entry_weights=[W]))
    Fb, ob = _solve(pkg, eng, Z, G, 6, hip=dict(entry_weights=[W * mask]))
    for a, b in zip(Fa['fac'], Fb['fac']):
        assert np.array_equal(a, b)
    assert np.array_equal(oa['func_val_conv'], ob['func_val_conv'])
    assert np.array_equal(oa['func_rel_missing'][1:], ob['func_rel_missing'][1:])


def test_two_solves_in_a_row_return_the_same_bits(pkg, eng):
    """No upload between the two: the second solve must start from Xhat = W o X again, not from the first one's Xhat."""
    rng = np.random.default_rng(54)
    shape = (40, 30, 20)
    Z, io, _ = cp_model(shape, 3, rng, [NN] * 3)
    Z['_ranks'] = [3] * 3
    W = weights_for(shape, rng)
    G = _init(Z, io)
    opt = options(MaxOuterIters=6)
    pkg.build_model(eng, Z, 'f64', dense_entry_weights=[W])
    runs = []
    for _ in range(2):
        pkg.upload_state(eng, Z, G)
        out = pkg.run_solver(eng, opt, 3, has_missing=True)
        runs.append((pkg.download_state(eng, Z, G), out))
    (F1, o1), (F2, o2) = runs
    for a, b in zip(F1['fac'], F2['fac']):
        assert np.array_equal(a, b)
    assert np.array_equal(o1['func_val_conv'], o2['func_val_conv'])
    assert np.array_equal(o1['func_rel_missing'][1:], o2['func_rel_missing'][1:])
    assert o1['func_rel_missing'][2] > 0


def test_world_2_as_threads(pkg):
    """Row shards in the manner of test_sharded_em_missing: every rank passes the full W and keeps its rows; the EM
    statistics are all-reduced.  Ranks bit-identical, 1e-8 against the stepped oracle."""
    rng = np.random.default_rng(31)
    shape = (37, 22, 19)
    Z, io, _ = cp_model(shape, 3, rng, [NN, NN, ('TV regularization', 1e-3)])
    W = {0: weights_for(shape, rng)}
    G = _init(Z, io)
    opt = options(MaxOuterIters=8)
    Fo, oo = stepped_em(Z, W, copy.deepcopy(G), opt, 8)
    key, world = next(_keys), 2
    res, err = [None] * world, [None] * world

    def rank_main(r):
        try:
            with pkg.Engine(0) as e:
                e.comm_init_local(key, r, world)
                _, Fg, _, og = pkg.cmtf_AOADMM(Z, alg_options=dict(opt, hip=_hip(Z, W)), init=copy.deepcopy(G), engine=e)
                res[r] = (Fg, og)
        except BaseException as ex:   # noqa: BLE001 -- reported by the main thread
            err[r] = ex

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r, ex in enumerate(err):
        assert ex is None, 'rank %d: %r' % (r, ex)
    (F0, o0), (F1, o1) = res
    for key_ in ('fac', 'constraint_fac', 'constraint_dual_fac'):
        for a, b in zip(F0[key_], F1[key_]):
            if a is not None:
                assert np.array_equal(a, b), key_
    assert np.array_equal(o0['func_val_conv'], o1['func_val_conv'])
    assert np.array_equal(o0['func_rel_missing'][1:], o1['func_rel_missing'][1:])
    compare(Fo, oo, F0, o0)
    _compare_em(oo, o0)


def test_world_2_bad_weight_in_the_other_ranks_rows_is_refused_by_every_rank(pkg):
    """Every rank holds the whole W and checks all of it: a bad value in rank 1's rows is refused by rank 0 as well, so
    the ranks keep agreeing on which blocks are weighted, and a solve with good weights runs afterwards."""
    capi = __import__('importlib').import_module('matlab-code_amd._capi')
    rng = np.random.default_rng(32)
    shape = (37, 22, 19)
    Z, io, _ = cp_model(shape, 3, rng, [NN] * 3)
    Z['_ranks'] = [3] * 3
    W = weights_for(shape, rng)
    bad = W.copy()
    bad[36, 21, 18] = 1.5                                              # the last row: rank 1's
    G = _init(Z, io)
    opt = options(MaxOuterIters=3)
    key, world = next(_keys), 2
    codes, res, err = [None] * world, [None] * world, [None] * world

    def rank_main(r):
        try:
            with pkg.Engine(0) as e:
                e.comm_init_local(key, r, world)
                pkg.build_model(e, Z, 'f64')
                try:
                    e.tensor_weights_upload(0, bad)
                    codes[r] = 0
                except pkg.AoadmmError as ex:
                    codes[r] = ex.code
                _, Fg, _, og = pkg.cmtf_AOADMM(Z, alg_options=dict(opt, hip=_hip(Z, {0: W})), init=copy.deepcopy(G), engine=e)
                res[r] = og['func_val_conv']
        except BaseException as ex:   # noqa: BLE001 -- reported by the main thread
            err[r] = ex

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r, ex in enumerate(err):
        assert ex is None, 'rank %d: %r' % (r, ex)
    assert codes == [capi.ERR_INVALID] * world, codes
    assert np.array_equal(res[0], res[1])


def test_known_answer_needs_the_weights(pkg, eng):
    """30 x 25 x 20, R = 3, noise-free, non-negative; a tenth of the entries hit by outliers of up to 5 max|X|; 150
    iterations.  With weight 0.01 on the hit entries the factors are recovered (stepped_em on the CPU: FMS 0.99994,
    relative error against the clean tensor 0.011); with unit weights they are not (FMS 0.515, error 1.11)."""
    rng = np.random.default_rng(11)
    Z, io, A = cp_model((30, 25, 20), 3, rng, [NN] * 3, noise=0.0)
    X = Z['object'][0]
    hit = rng.random(X.shape) < 0.1
    Zc = dict(Z, object=[X + hit * (5 * np.abs(X).max() * rng.random(X.shape))])
    G = _init(Zc, io)

    def fit(W):
        F, _ = _solve(pkg, eng, Zc, G, 150, hip=dict(entry_weights=[W]))
        return fms(F['fac'], A), rel_fro(full_ktensor(F['fac']), X)

    fw, ew = fit(np.where(hit, 0.01, 1.0))
    fu, eu = fit(np.ones(X.shape))
    print('known answer: weighted FMS %.6f error %.4g | unit weights FMS %.4f error %.4g' % (fw, ew, fu, eu))
    assert fw >= 0.999 and ew <= 0.03, (fw, ew)
    assert fu < 0.9, fu


def test_driver_refusals(pkg, eng):
    capi = __import__('importlib').import_module('matlab-code_amd._capi')
    rng = np.random.default_rng(55)
    shape = (9, 8, 7)
    Z, io, _ = cp_model(shape, 2, rng, [None] * 3)
    G = _init(Z, io)
    W = np.full(shape, 0.5)
    with pytest.raises(ValueError):
        _solve(pkg, eng, Z, G, 2, hip=dict(entry_weights=[W[:-1]]))
    Wb = W.copy()
    Wb[0, 0, 0] = 1.5
    with pytest.raises(ValueError):
        _solve(pkg, eng, Z, G, 2, hip=dict(entry_weights=[Wb]))
    subs = np.argwhere(np.abs(Z['object'][0]) > 0.05)
    Zs = dict(Z, object=[pkg.sptensor(subs, Z['object'][0][tuple(subs.T)], shape)])
    with pytest.raises(capi.UnsupportedOnDevice) as ei:
        _solve(pkg, eng, Zs, G, 2, hip=dict(entry_weights=[W]))
    assert 'sparse_entry_weights' in str(ei.value)
    with pytest.raises(capi.UnsupportedOnDevice) as ei:
        _solve(pkg, eng, Z, G, 2, hip=dict(sparse_entry_weights=[W.ravel()]))
    assert 'entry_weights' in str(ei.value)
    F, out = _solve(pkg, eng, Z, G, 2, hip=dict(entry_weights=[W]))     # the engine works on
    assert 'func_rel_missing' in out and np.isfinite(out['f_rel_missing'])
