"""Host side of weighted sparse CP blocks (alg_options.hip.sparse_entry_weights / sparse_unstored_weight,
aoadmm_tensor_set_entry_weights): the stepped-oracle reference of tests/weighted_ref.py is pinned to the oracle's own EM
run for every model family the GPU tests use, and the driver's option handling is checked against a stand-in engine.
No GPU."""
import copy
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from helpers import cp_cp_exact_model, cp_model, options
from test_sparse_observed_host import _Eng, _model
from weighted_ref import dense_weights, stepped_em

capi = importlib.import_module('matlab-code_amd._capi')

NN = ('non-negativity',)
FAMILIES = {
    'cp-unconstrained': ((9, 8, 7), 3, [None, None, None]),
    'cp-nonneg-tv': ((9, 8, 7), 3, [NN, NN, ('TV regularization', 1e-3)]),
    'matrix': ((12, 10), 4, [NN, NN]),
    'four-way': ((6, 5, 4, 3), 3, [NN, None, NN, NN]),
}


def _same_run(Fo, oo, Fs, os_):
    for key in ('fac', 'constraint_fac', 'constraint_dual_fac', 'coupling_fac', 'coupling_dual_fac'):
        for a, b in zip(Fo[key], Fs[key]):
            if a is not None:
                assert np.array_equal(np.asarray(a), np.asarray(b)), key
    assert np.array_equal(oo['innerIters'], os_['innerIters'])
    for k in ('func_coupl_conv', 'func_constr_conv'):
        assert np.array_equal(oo[k], os_[k]), k
    # the objective is summed in another order (W o (X - M)^2 over the whole array), f_rel_missing likewise: a few ulp
    # of a sum of at most 2^13 terms
    assert np.allclose(os_['func_val_conv'], oo['func_val_conv'], rtol=1e-13, atol=1e-15)
    assert np.allclose(os_['func_rel_missing'][1:], oo['func_rel_missing'][1:], rtol=1e-14, atol=0.0)
    assert np.isnan(os_['func_rel_missing'][0])


@pytest.mark.parametrize('family', list(FAMILIES))
def test_stepped_loop_with_a_boolean_w_is_the_oracles_em(family):
    shape, R, constraints = FAMILIES[family]
    rng = np.random.default_rng(sum(map(ord, family)))
    Z, io, _ = cp_model(shape, R, rng, constraints)
    mask = rng.random(shape) < 0.4
    Zm = dict(Z, object=[np.where(mask, Z['object'][0], 0.0)], miss=[mask])
    G = OA.init_coupled_AOADMM_CMTF({**Zm, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    opt = options(MaxOuterIters=6)
    _, Fo, _, oo = OA.cmtf_AOADMM(Zm, alg_options=opt, init=copy.deepcopy(G))
    Fs, os_ = stepped_em(Z, {0: mask.astype(np.float64)}, copy.deepcopy(G), opt, 6)
    _same_run(Fo, oo, Fs, os_)


def test_stepped_loop_on_the_exact_coupling():
    rng = np.random.default_rng(41)
    Z, io = cp_cp_exact_model(rng)
    mask = rng.random(np.asarray(Z['object'][0]).shape) < 0.4
    Zm = dict(Z, object=[np.where(mask, Z['object'][0], 0.0), Z['object'][1]], miss=[mask, None])
    G = OA.init_coupled_AOADMM_CMTF({**Zm, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    opt = options(MaxOuterIters=6)
    _, Fo, _, oo = OA.cmtf_AOADMM(Zm, alg_options=opt, init=copy.deepcopy(G))
    Fs, os_ = stepped_em(Z, {0: mask.astype(np.float64)}, copy.deepcopy(G), opt, 6)
    _same_run(Fo, oo, Fs, os_)


def test_weighted_objective_is_non_increasing():
    """Fractional W (stored weights 0.3 .. 1, alpha = 0.1), unconstrained: every exact block update lowers the
    majoriser, which touches the weighted objective at the current iterate."""
    rng = np.random.default_rng(5)
    shape = (9, 8, 7)
    Z, io, _ = cp_model(shape, 3, rng, [None] * 3)
    subs = np.argwhere(rng.random(shape) < 0.4)
    W = dense_weights(shape, subs, 0.3 + 0.7 * rng.random(len(subs)), 0.1)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, out = stepped_em(Z, {0: W}, G, options(), 40)
    obj = np.array(out['wobj'][0])
    assert len(obj) == 41 and np.all(np.diff(obj) <= 1e-15 * obj[0]), np.diff(obj).max()


# ---- the driver against the stand-in engine ----------------------------------------------------------------------
class _WEng(_Eng):
    def __init__(self):
        super().__init__()
        self.weights = []

    def set_entry_weights(self, p, subs, wts, unstored_weight=0.0):
        self.weights.append((p, None if wts is None else (np.asarray(subs).shape, np.asarray(wts).copy()), unstored_weight))


def _wts(Z, p, rng):
    return rng.random(len(Z['object'][p].vals))


def test_build_model_marks_and_weights_exactly_the_named_blocks(pkg):
    Z = _model(pkg)
    rng = np.random.default_rng(1)
    w0 = _wts(Z, 0, rng)
    e = _WEng()
    pkg.build_model(e, Z, entry_weights=[w0, None, None, None], unstored_weight=[0.25, None, 0.5, None])
    assert e.marked == [(0, True), (2, True)] and [p for p, _ in e.coo] == [0, 2]
    (p0, l0, a0), (p2, l2, a2) = e.weights
    assert (p0, a0, p2, l2, a2) == (0, 0.25, 2, None, 0.5)
    assert l0[0] == Z['object'][0].subs.shape and np.array_equal(l0[1], w0)
    # one number: every named block, those of observed_only included; a block named nowhere stays plain
    e = _WEng()
    pkg.build_model(e, Z, observed_only=[3], entry_weights=[w0, None, None, None], unstored_weight=0.125)
    assert e.marked == [(0, True), (2, True)]
    assert [(p, a) for p, _, a in e.weights] == [(0, 0.125), (2, 0.125)] and e.weights[1][1] is None
    # weights alone: alpha defaults to 0
    e = _WEng()
    pkg.build_model(e, Z, entry_weights=[w0, None, None, None])
    assert e.marked == [(0, True)] and [(p, a) for p, _, a in e.weights] == [(0, 0.0)]
    # neither option: nothing is weighted
    e = _WEng()
    pkg.build_model(e, Z, observed_only=1)
    assert e.weights == [] and e.marked == [(0, True), (2, True)]


@pytest.mark.parametrize('kw,exc,word', [
    (dict(entry_weights=[None, np.ones(42), None, None]), capi.UnsupportedOnDevice, 'dense'),
    (dict(unstored_weight=[None, 0.5, None, None]), capi.UnsupportedOnDevice, 'dense'),
    (dict(unstored_weight=[None, None, None, 0.5]), capi.UnsupportedOnDevice, 'PARAFAC2'),
    (dict(unstored_weight=[0.5, None, None, None], sparse_sharding=True), capi.UnsupportedOnDevice, 'sparse_sharding'),
    (dict(entry_weights=[np.ones(3), None, None, None]), ValueError, 'stored entries'),
    (dict(entry_weights=[None, None, None]), ValueError, 'list over'),
    (dict(unstored_weight=[0.5, None]), ValueError, 'list over'),
    (dict(unstored_weight=[1.5, None, None, None]), ValueError, r'outside \[0, 1\]'),
    (dict(unstored_weight=[float('nan'), None, None, None]), ValueError, r'outside \[0, 1\]'),
    (dict(observed_only=[1], unstored_weight=-0.1), ValueError, r'outside \[0, 1\]'),
])
def test_refusals_come_before_any_upload(pkg, kw, exc, word):
    e = _WEng()
    with pytest.raises(exc, match=word):
        pkg.build_model(e, _model(pkg), **kw)
    assert e.coo == [] and e.marked == [] and e.weights == []


@pytest.mark.parametrize('bad', [1.0 + 1e-12, -1e-12, float('inf'), float('nan')])
def test_a_weight_outside_the_range_is_refused(pkg, bad):
    Z = _model(pkg)
    w = np.full(len(Z['object'][0].vals), 0.5)
    w[3] = bad
    e = _WEng()
    with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
        pkg.build_model(e, Z, entry_weights=[w, None, None, None])
    assert e.coo == [] and e.weights == []


def test_symbol_and_engine_method_exist(pkg):
    assert 'aoadmm_tensor_set_entry_weights' in capi.SYMBOLS
    assert callable(pkg.Engine.set_entry_weights)
