"""CPU: the host layer of the Tucker projection and of core consistency.  The header declares
`aoadmm_resident_project` and `aoadmm_resident_core_consistency`, the binding lists them and the library exports them;
the engine wraps them and the driver knows the option; the numpy references of the GPU tests against a brute-force loop,
an exact model and the planted case."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

from core_ref import (CC_BAD_BELOW, CC_OK_ABOVE, PLANTED_DIMS, pinv_floor, pinv_t, planted_data, planted_oracle_cc, ref_bound,
                      ref_cc, ref_core)

capi = importlib.import_module('matlab-code_amd._capi')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    'aoadmm_resident_project': 'aoadmm_ctx* ctx, int p, const double* const* M, const int64_t* ld, const int* r, double* core',
    'aoadmm_resident_core_consistency': 'aoadmm_ctx* ctx, int p, double* cc, double* core_or_null, int* rank_deficient_or_null',
}


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_entries_are_declared_bound_and_exported(pkg, entry):
    with open(os.path.join(ROOT, 'include', 'aoadmm_hip.h')) as f:
        text = f.read()
    decl = re.search(r'^int %s\(([^;]*)\);' % entry, text, flags=re.M | re.S)
    assert decl, 'the header does not declare %s' % entry
    assert ' '.join(decl.group(1).split()) == ENTRIES[entry]
    assert entry in pkg.SYMBOLS and entry in capi.SYMBOLS
    lib = pkg.load_library()
    assert hasattr(lib, entry) and len(getattr(lib, entry).argtypes) == ENTRIES[entry].count(',') + 1
    assert lib.aoadmm_abi_version() == 3               # functions were added, nothing moved: the version stays


def test_engine_package_and_driver_have_the_wrappers(pkg):
    assert callable(getattr(pkg.Engine, 'project', None)) and callable(getattr(pkg.Engine, 'core_consistency', None))
    assert list(inspect.signature(pkg.Engine.project).parameters) == ['self', 'p', 'mats']
    sig = inspect.signature(pkg.Engine.core_consistency)
    assert list(sig.parameters)[:3] == ['self', 'p', 'return_core'] and sig.parameters['return_core'].default is False
    assert callable(getattr(pkg, 'core_consistency', None)) and 'core_consistency' in pkg.__all__
    drv = importlib.import_module('matlab-code_amd.driver')
    assert "hip.get('core_consistency'" in inspect.getsource(drv.cmtf_AOADMM)


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    assert lib.aoadmm_resident_project(None, 0, None, None, None, None) != capi.OK
    assert lib.aoadmm_resident_core_consistency(None, 0, None, None, None) != capi.OK


def test_ref_core_against_a_triple_loop():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((4, 3, 2))
    M = [rng.standard_normal((4, 3)), rng.standard_normal((3, 2)), rng.standard_normal((2, 4))]
    want = np.zeros((3, 2, 4))
    for p in range(3):
        for q in range(2):
            for r in range(4):
                for i in range(4):
                    for j in range(3):
                        for k in range(2):
                            want[p, q, r] += X[i, j, k] * M[0][i, p] * M[1][j, q] * M[2][k, r]
    assert np.allclose(ref_core(X, M), want, rtol=1e-13, atol=1e-14)
    assert np.all(ref_bound(X, M) >= np.abs(want) - 1e-14)


def test_pinv_t_two_ways_agree():
    rng = np.random.default_rng(1)
    F = rng.standard_normal((9, 4))
    a, b = pinv_t(F), pinv_t(F, 'longdouble')
    assert np.allclose(a, b, rtol=1e-12, atol=1e-13)
    assert np.allclose(a.T @ F, np.eye(4), atol=1e-12)


def test_package_core_consistency_is_ref_cc(pkg):
    rng = np.random.default_rng(2)
    G = rng.standard_normal((5, 5, 5))
    assert pkg.core_consistency(G) == pytest.approx(ref_cc(G), rel=1e-14)
    for bad in (np.zeros((2, 3, 2)), np.zeros((3, 3))):
        with pytest.raises(ValueError):
            pkg.core_consistency(bad)


def test_cc_is_100_on_an_exact_model_with_its_own_factors():
    rng = np.random.default_rng(3)
    A = [rng.standard_normal((n, 3)) for n in (7, 6, 5)]
    X = np.einsum('ir,jr,kr->ijk', *A)
    core = ref_core(X, [pinv_t(a) for a in A])
    assert ref_cc(core) == pytest.approx(100.0, abs=1e-9)
    assert pinv_floor(X, A) < 1e-13


def test_planted_case_drops_from_rank_3_to_rank_4():
    """12 x 10 x 8, rank 3, uniform factors + 0.1, noise 5 % of the mean magnitude (core_ref.PLANTED_SEED).  The oracle's
    fit, 500 outer iterations: cc = 97.31 at R = 3 (100 - cc = 2.69) and cc = -21.72 at R = 4 (100 - cc = 121.7).  The
    thresholds of the GPU test, CC_OK_ABOVE = 90 and CC_BAD_BELOW = 50, leave a factor 3.7 and 2.4 in 100 - cc."""
    assert planted_data().shape == PLANTED_DIMS
    c3, c4 = planted_oracle_cc(3), planted_oracle_cc(4)
    print('oracle core consistency: R = 3: %.4f, R = 4: %.4f' % (c3, c4))
    assert c3 == pytest.approx(97.31, abs=0.05) and c4 == pytest.approx(-21.72, abs=0.5)
    assert 2.0 * (100.0 - c3) <= 100.0 - CC_OK_ABOVE
    assert 100.0 - c4 >= 2.0 * (100.0 - CC_BAD_BELOW)
