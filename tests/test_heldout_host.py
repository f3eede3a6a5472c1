"""CPU: the host layer of held-out scoring.  `sptensor.split` cuts a coalesced tensor into a training and a held-out
part; `heldout_lists` (alg_options['hip']['heldout'] / ['heldout_patience']) validates before the engine is touched, which
`cmtf_AOADMM` is run against a stand-in engine to show; the header declares the five entries and the binding lists them."""
import importlib
import os
import re

import numpy as np
import pytest

capi = importlib.import_module('matlab-code_amd._capi')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['aoadmm_resident_model_at', 'aoadmm_tensor_set_heldout', 'aoadmm_resident_heldout_stats', 'aoadmm_heldout_info',
           'aoadmm_heldout_trace']


def _sp(pkg, shape, rng, dup=0):
    subs = np.argwhere(rng.random(shape) < 0.4)
    vals = rng.standard_normal(len(subs))
    if dup:
        pick = rng.choice(len(subs), dup, replace=False)
        subs, vals = np.vstack([subs, subs[pick]]), np.concatenate([vals, rng.standard_normal(dup)])
    return pkg.sptensor(subs, vals, shape)


def _cells(X):
    return {tuple(s): v for s, v in zip(X.subs.tolist(), X.vals.tolist())}


# ---- sptensor.split ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,frac', [((7, 6, 5), 0.1), ((7, 6, 5), 0.5), ((9, 8), 0.33), ((4, 3, 3, 2), 0.25)])
def test_split_parts_are_disjoint_and_their_union_is_the_tensor(pkg, shape, frac):
    X = _sp(pkg, shape, np.random.default_rng(1), dup=5)       # duplicates are summed first: the cut is after coalescing
    train, held = X.split(frac, np.random.default_rng(2))
    assert train.shape == held.shape == X.shape
    assert held.nnz == int(round(frac * X.nnz)) and train.nnz == X.nnz - held.nnz
    a, b = _cells(train), _cells(held)
    assert not set(a) & set(b)
    assert {**a, **b} == _cells(X)


def test_split_is_deterministic_for_a_given_rng(pkg):
    X = _sp(pkg, (7, 6, 5), np.random.default_rng(1))
    t1, h1 = X.split(0.3, np.random.default_rng(5))
    t2, h2 = X.split(0.3, np.random.default_rng(5))
    t3, h3 = X.split(0.3, 5)                                    # a seed is the generator made from it
    assert np.array_equal(h1.subs, h2.subs) and np.array_equal(h1.vals, h2.vals) and np.array_equal(t1.subs, t2.subs)
    assert np.array_equal(h1.subs, h3.subs) and np.array_equal(t1.vals, t3.vals)
    _, h4 = X.split(0.3, np.random.default_rng(6))
    assert not np.array_equal(h1.subs, h4.subs)


def test_split_frac_0_and_1_give_an_empty_part(pkg):
    X = _sp(pkg, (7, 6, 5), np.random.default_rng(1))
    train, held = X.split(0.0, 1)
    assert held.nnz == 0 and _cells(train) == _cells(X)
    train, held = X.split(1.0, 1)
    assert train.nnz == 0 and _cells(held) == _cells(X)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            X.split(bad, 1)


# ---- driver validation ------------------------------------------------------------------------------------------------
class _Touched(Exception):
    pass


class _Eng:
    """Stand-in for an Engine that must not be reached: any use raises."""
    def __getattr__(self, name):
        raise _Touched(name)


def _model(pkg):
    """Z.object = {sptensor 6x5x4, dense 6x7, PARAFAC2 4 x [3, 5] x 2}"""
    rng = np.random.default_rng(3)
    Z = dict(loss_function=['Frobenius'] * 3, model=['CP', 'CP', 'PAR2'], modes=[[1, 2, 3], [4, 5], [6, 7, 8]],
             size=[6, 5, 4, 6, 7, 4, [3, 5], 2],
             coupling=dict(lin_coupled_modes=[0] * 8, coupling_type=[], coupl_trafo_matrices=[None] * 8),
             constrained_modes=[0] * 8, constraints=[None] * 8, weights=[1.0] * 3,
             object=[_sp(pkg, (6, 5, 4), rng), rng.random((6, 7)), [rng.random((4, 3)), rng.random((4, 5))]])
    G = {'fac': [rng.random((6, 2)), rng.random((5, 2)), rng.random((4, 2)), rng.random((6, 2)), rng.random((7, 2)),
                 rng.random((4, 2)), [rng.random((3, 2)), rng.random((5, 2))], rng.random((2, 2))]}
    return Z, G


def _opt(**hip):
    return dict(MaxOuterIters=3, MaxInnerIters=2, AbsFuncTol=0.0, OuterRelTol=0.0, innerRelPrTol_coupl=0.0,
                innerRelPrTol_constr=0.0, innerRelDualTol_coupl=0.0, innerRelDualTol_constr=0.0, bsum=0, hip=hip)


GOOD = (np.array([[0, 0, 0], [5, 4, 3], [5, 4, 3]]), np.array([1.0, 2.0, 3.0]))
BAD = {
    'block 0': dict(heldout={0: GOOD}),
    'block beyond the model': dict(heldout={4: GOOD}),
    'block not an integer': dict(heldout={'1': GOOD}),
    'wrong width': dict(heldout={1: (np.array([[0, 0], [1, 1]]), np.array([1.0, 2.0]))}),
    'wrong width for the matrix': dict(heldout={2: GOOD}),
    'subs not 2-d': dict(heldout={1: (np.array([0, 0, 0]), np.array([1.0]))}),
    'subscript too large': dict(heldout={1: (np.array([[0, 0, 0], [6, 0, 0]]), np.array([1.0, 2.0]))}),
    'subscript too large in the last mode': dict(heldout={1: (np.array([[0, 0, 4]]), np.array([1.0]))}),
    'negative subscript': dict(heldout={1: (np.array([[0, -1, 0]]), np.array([1.0]))}),
    'non-integer subscript': dict(heldout={1: (np.array([[0, 1.5, 0]]), np.array([1.0]))}),
    'length mismatch': dict(heldout={1: (GOOD[0], np.array([1.0, 2.0]))}),
    'value not finite': dict(heldout={1: (GOOD[0], np.array([1.0, np.nan, 3.0]))}),
    'PAR2 subscript outside its slab': dict(heldout={3: (np.array([[0, 3, 0]]), np.array([1.0]))}),
    'sptensor of another size': dict(heldout={1: 'SP_OTHER'}),
    'not a dict': dict(heldout=[GOOD]),
    'patience without a list': dict(heldout_patience=3),
    'patience with an empty dict': dict(heldout={}, heldout_patience=1),
    'negative patience': dict(heldout={1: GOOD}, heldout_patience=-1),
    'patience not an integer': dict(heldout={1: GOOD}, heldout_patience=1.5),
}


@pytest.mark.parametrize('case', list(BAD))
def test_bad_lists_raise_before_the_engine_is_touched(pkg, case):
    Z, G = _model(pkg)
    hip = dict(BAD[case])
    if isinstance(hip.get('heldout'), dict):
        hip['heldout'] = {k: (_sp(pkg, (6, 5, 3), np.random.default_rng(4)) if isinstance(v, str) else v)
                          for k, v in hip['heldout'].items()}
    with pytest.raises(ValueError):
        pkg.cmtf_AOADMM(Z, alg_options=_opt(**hip), init=G, engine=_Eng())


def test_good_lists_pass_and_reach_the_engine(pkg):
    Z, G = _model(pkg)
    S = _sp(pkg, (6, 5, 4), np.random.default_rng(4))
    held = {1: S, 2: (np.array([[0.0, 6.0]]), [2.5]), 3: (np.array([[3, 4, 1], [0, 2, 0]]), [1.0, -1.0])}
    lists = pkg.heldout_lists(Z, held, 2)
    assert sorted(lists) == [0, 1, 2]
    assert np.array_equal(lists[0][0], S.subs) and np.array_equal(lists[0][1], S.vals)
    assert lists[1][0].dtype == np.int64 and lists[1][0].tolist() == [[0, 6]] and lists[1][1].tolist() == [2.5]
    assert lists[2][0].tolist() == [[3, 4, 1], [0, 2, 0]]
    assert pkg.heldout_lists(Z, None, 0) == {} and pkg.heldout_lists(Z, {}, 0) == {}
    assert pkg.heldout_lists(Z, {1: (np.zeros((0, 3), dtype=np.int64), [])}, 0) == {}     # an empty list is no list
    with pytest.raises(_Touched):                      # valid input goes on to the engine
        pkg.cmtf_AOADMM(Z, alg_options=_opt(heldout=held, heldout_patience=2), init=G, engine=_Eng())


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_binding_lists_them(pkg):
    text = open(os.path.join(ROOT, 'include', 'aoadmm_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\bint\s+(aoadmm_[a-z0-9_]+)\s*\(', text))
    for name in ENTRIES:
        assert name in declared and name in pkg.SYMBOLS and name in capi.SYMBOLS, name
    for method in ('model_at', 'set_heldout', 'heldout_stats', 'heldout_info', 'heldout_trace'):
        assert callable(getattr(pkg.Engine, method))
    assert re.search(r'int32_t\s+heldout_patience\s*;', text) and re.search(r'int32_t\s+reserved\[4\]\s*;', text)
    # the option took one of the reserved ints: no offset moved
    assert capi.Options.heldout_patience.offset == capi.Options.par2_slab_sharding.offset + 4
    assert capi.Options.reserved.offset == capi.Options.heldout_patience.offset + 4 and capi.Options.reserved.size == 16


def test_library_exports_the_entries(pkg):
    lib = pkg.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.aoadmm_abi_version() == 3
