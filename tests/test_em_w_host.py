"""CPU: the bounds of tests/em_w_ref.py against an emulation of the weighted strip kernel's fp32 arithmetic, the
emulation against em_ref's masked one under a boolean W, tests/weighted_ref.py::stepped_em with a boolean dense W against
the oracle's own masked run on a fully stored block, and the driver's checks of `alg_options['hip']['entry_weights']`."""
import copy
import functools
import importlib

import numpy as np
import pytest

import em_ref
import em_w_ref
from oracle import aoadmm as OA
from helpers import cp_model, options
from weighted_ref import stepped_em

capi = importlib.import_module('matlab-code_amd._capi')

SHAPES = [(37, 70, 9), (131, 67, 70)]
RANKS = [1, 5, 20, 32]
KINDS = ['uniform', 'boolean', 'ones', 'zeros']


@functools.lru_cache(maxsize=2)
def _data(dims, R):
    X, U = em_ref.make_data(dims, R, np.random.default_rng(1000 * sum(dims) + R))
    return X, U, em_ref.model(U)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('dims', SHAPES, ids=str)
def test_emulation_stays_inside_the_bounds(dims, R, kind):
    """Two passes: from the reset (q = 0) and, with other factors, from the Xhat the first pass left (q != 0)."""
    X, U, M = _data(dims, R)
    W = em_w_ref.make_weights(dims, np.random.default_rng(sum(dims) + R), kind)
    xh = em_w_ref.reset(X, W, 'f32')
    U2 = em_ref.random_factors(dims, R, np.random.default_rng(5 + R))
    for fac, model in ((U, M), (U2, None)):
        ref = em_w_ref.EmWRef(X, W, xh, fac, M=model)
        xn, stats = em_w_ref.emulate_f32_pass(X, W, xh, fac)
        re, rs = ref.entry_ratio(xn, 'f32'), ref.stat_ratios(stats, 'f32')
        print('emulated weighted pass %s R=%d W=%s: entry %.3g of its bound, sums %s of theirs'
              % (dims, R, kind, re, ' '.join('%.3g' % v for v in rs)))
        assert re <= 1.0, re
        for k, name in enumerate(em_w_ref.STAT_NAMES):
            if ref.stats[k] == 0:
                assert stats[k] == 0, (name, stats[k])
            assert rs[k] <= 1.0, (name, rs[k], stats[k], ref.stats[k])
        if kind == 'ones':
            assert np.array_equal(xn.astype(np.float64), X) and stats[0] == 0 and stats[1] == 0
        xh = np.asfortranarray(xn.astype(np.float64))


@pytest.mark.parametrize('R', RANKS)
@pytest.mark.parametrize('dims', SHAPES, ids=str)
def test_boolean_weights_emulate_to_the_masked_pass_bit_for_bit(dims, R):
    X, U, _ = _data(dims, R)
    obs = np.random.default_rng(3 * sum(dims) + R).random(dims) >= 0.3
    Xz = np.where(obs, X, 0.0)                                       # zeros under the mask
    m, st_masked = em_ref.emulate_f32_pass(Xz, obs, U)
    xn, st = em_w_ref.emulate_f32_pass(Xz, obs.astype(np.float64), Xz, U)
    assert st.tobytes() == st_masked.tobytes()
    assert np.array_equal(xn, np.where(obs, Xz.astype(np.float32), m))
    # and a second pass over the imputed block, where the masked pass reads its own data for `x`
    U2 = em_ref.random_factors(dims, R, np.random.default_rng(11 + R))
    cur = xn.astype(np.float64)
    m2, st2_masked = em_ref.emulate_f32_pass(cur, obs, U2)
    xn2, st2 = em_w_ref.emulate_f32_pass(Xz, obs.astype(np.float64), cur, U2)
    assert st2.tobytes() == st2_masked.tobytes()
    assert np.array_equal(xn2, np.where(obs, Xz.astype(np.float32), m2))


NN = ('non-negativity',)


@pytest.mark.parametrize('shape,R,constraints', [((11, 9, 8), 3, [NN, NN, ('TV regularization', 1e-3)]),
                                                 ((13, 11), 4, [NN, NN])], ids=['3-way', 'matrix'])
def test_stepped_em_with_a_boolean_dense_w_is_the_oracles_masked_run(shape, R, constraints):
    """Z.object fully stored (the values under the mask are whatever the data holds; the oracle zeroes them itself)."""
    rng = np.random.default_rng(sum(shape) + R)
    Z, io, _ = cp_model(shape, R, rng, constraints)
    mask = rng.random(shape) < 0.6
    Zm = dict(Z, object=[np.where(mask, Z['object'][0], 0.0)], miss=[mask])
    G = OA.init_coupled_AOADMM_CMTF({**Zm, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    opt = options(MaxOuterIters=5)
    _, Fo, _, oo = OA.cmtf_AOADMM(Zm, alg_options=opt, init=copy.deepcopy(G))
    Fs, os_ = stepped_em(Z, {0: mask.astype(np.float64)}, copy.deepcopy(G), opt, 5)
    for key in ('fac', 'constraint_fac', 'constraint_dual_fac'):
        for a, b in zip(Fo[key], Fs[key]):
            if a is not None:
                assert np.array_equal(np.asarray(a), np.asarray(b)), key
    assert np.array_equal(oo['innerIters'], os_['innerIters'])
    # summed in another order: a few ulp (tests/test_sparse_weighted_host.py)
    assert np.allclose(os_['func_val_conv'], oo['func_val_conv'], rtol=1e-13, atol=1e-15)
    assert np.allclose(os_['func_rel_missing'][1:], oo['func_rel_missing'][1:], rtol=1e-14, atol=0.0)


# ---- the driver's checks -------------------------------------------------------------------------------------------
def _w(Z, p=0):
    return np.full(np.shape(Z['object'][p]), 0.5)


def test_dense_weight_blocks_accepts_and_folds_the_mask(pkg):
    drv = importlib.import_module('matlab-code_amd.driver')
    rng = np.random.default_rng(1)
    Z, _, _ = cp_model((5, 4, 3), 2, rng, [None] * 3)
    assert drv.dense_weight_blocks(Z, None) == {} and drv.dense_weight_blocks(Z, [None]) == {}
    W = rng.random((5, 4, 3))
    out = drv.dense_weight_blocks(Z, [W])
    assert list(out) == [0] and np.array_equal(out[0], W) and out[0].flags.f_contiguous
    mk = rng.random((5, 4, 3)) < 0.5
    out = drv.dense_weight_blocks(dict(Z, miss=[mk]), [W])
    assert np.array_equal(out[0], W * mk)


@pytest.mark.parametrize('case,exc,word', [
    ('length', ValueError, 'list over'),
    ('shape', ValueError, 'size'),
    ('above', ValueError, 'outside [0, 1]'),
    ('negative', ValueError, 'outside [0, 1]'),
    ('nan', ValueError, 'outside [0, 1]'),
    ('sparse', capi.UnsupportedOnDevice, 'sparse_entry_weights'),
    ('par2', capi.UnsupportedOnDevice, 'sparse_entry_weights'),
])
def test_dense_weight_blocks_refusals(pkg, case, exc, word):
    drv = importlib.import_module('matlab-code_amd.driver')
    rng = np.random.default_rng(2)
    Z, _, _ = cp_model((5, 4, 3), 2, rng, [None] * 3)
    W = _w(Z)
    if case == 'length':
        arg = [W, W]
    elif case == 'shape':
        arg = [W[:-1]]
    elif case in ('above', 'negative', 'nan'):
        W[1, 2, 0] = {'above': 1.0 + 1e-12, 'negative': -1e-12, 'nan': float('nan')}[case]
        arg = [W]
    elif case == 'sparse':
        Z = dict(Z, object=[pkg.sptensor(np.array([[0, 0, 0], [1, 2, 1]]), np.array([1.0, 2.0]), (5, 4, 3))])
        arg = [W]
    else:
        Z = dict(Z, model=['PAR2'])
        arg = [W]
    with pytest.raises(exc) as ei:
        drv.dense_weight_blocks(Z, arg)
    assert word in str(ei.value), str(ei.value)


def test_symbol_and_engine_method_exist(pkg):
    assert 'aoadmm_tensor_weights_upload' in pkg.SYMBOLS
    assert hasattr(pkg.load_library(), 'aoadmm_tensor_weights_upload') and hasattr(pkg.Engine, 'tensor_weights_upload')
