"""CPU: the host layer of `alg_options['hip']['heldout_keep_best']`.  The option is validated
before the engine is touched, which `cmtf_AOADMM` is run against a stand-in engine to show; `aoadmm_options` did not move;
the header declares the three entries and the binding lists them."""
import importlib
import os
import re

import numpy as np
import pytest

from test_heldout_host import GOOD, _Eng, _Touched, _model, _opt

capi = importlib.import_module('matlab-code_amd._capi')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['aoadmm_heldout_keep_best', 'aoadmm_heldout_restore_best', 'aoadmm_heldout_best_info']

BAD = {
    'not an integer': dict(heldout={1: GOOD}, heldout_keep_best=0.5),
    'a string': dict(heldout={1: GOOD}, heldout_keep_best='1'),
    'an array': dict(heldout={1: GOOD}, heldout_keep_best=[0, 1]),
    'None': dict(heldout={1: GOOD}, heldout_keep_best=None),
    'neither 0 nor 1': dict(heldout={1: GOOD}, heldout_keep_best=2),
    'negative': dict(heldout={1: GOOD}, heldout_keep_best=-1),
    'on without a list': dict(heldout_keep_best=1),
    'on with an empty dict': dict(heldout={}, heldout_keep_best=1),
    'on with an empty list': dict(heldout={1: (np.zeros((0, 3), dtype=np.int64), [])}, heldout_keep_best=1),
}


@pytest.mark.parametrize('case', list(BAD))
def test_bad_values_raise_before_the_engine_is_touched(pkg, case):
    Z, G = _model(pkg)
    with pytest.raises(ValueError):
        pkg.cmtf_AOADMM(Z, alg_options=_opt(**BAD[case]), init=G, engine=_Eng())


def test_good_values_pass_and_reach_the_engine(pkg):
    Z, G = _model(pkg)
    lists = pkg.heldout_lists(Z, {1: GOOD}, 0)
    assert pkg.heldout_keep_best_option(0, {}) == 0 and pkg.heldout_keep_best_option(False, lists) == 0
    assert pkg.heldout_keep_best_option(1, lists) == 1 and pkg.heldout_keep_best_option(True, lists) == 1
    assert pkg.heldout_keep_best_option(np.int64(1), lists) == 1
    for on in (0, 1):
        with pytest.raises(_Touched):                  # valid input goes on to the engine
            pkg.cmtf_AOADMM(Z, alg_options=_opt(heldout={1: GOOD}, heldout_keep_best=on), init=G, engine=_Eng())


def test_options_struct_did_not_move(pkg):
    """The switch is an entry point, not an option: size and every offset of aoadmm_options are those of ABI version 3."""
    want = [('MaxOuterIters', 0, 4), ('MaxInnerIters', 4, 4), ('AbsFuncTol', 8, 8), ('OuterRelTol', 16, 8),
            ('innerRelPrTol_coupl', 24, 8), ('innerRelPrTol_constr', 32, 8), ('innerRelDualTol_coupl', 40, 8),
            ('innerRelDualTol_constr', 48, 8), ('bsum', 56, 4), ('bsum_weight', 64, 8),
            ('iter_start_PAR2Bkconstraint', 72, 4), ('has_increase_factor_rhoBk', 76, 4), ('increase_factor_rhoBk', 80, 8),
            ('use_dimtree', 88, 4), ('no_permuted_copy', 92, 4), ('par2_slab_sharding', 96, 4), ('heldout_patience', 100, 4),
            ('reserved', 104, 16)]
    got = [(n, getattr(capi.Options, n).offset, getattr(capi.Options, n).size) for n, _ in capi.Options._fields_]
    assert got == want
    import ctypes as C
    assert C.sizeof(capi.Options) == 120
    text = open(os.path.join(ROOT, 'include', 'aoadmm_hip.h')).read()
    assert re.search(r'int32_t\s+reserved\[4\]\s*;', text) and 'heldout_keep_best;' not in text


def test_header_declares_the_entries_and_the_binding_lists_them(pkg):
    text = open(os.path.join(ROOT, 'include', 'aoadmm_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\bint\s+(aoadmm_[a-z0-9_]+)\s*\(', text))
    for name in ENTRIES:
        assert name in declared and name in pkg.SYMBOLS and name in capi.SYMBOLS, name
    for method in ('heldout_keep_best', 'heldout_restore_best', 'heldout_best_info'):
        assert callable(getattr(pkg.Engine, method))


def test_library_exports_the_entries(pkg):
    lib = pkg.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.aoadmm_abi_version() == 3
