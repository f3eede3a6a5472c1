"""CPU: the fold-in entry points are declared, bound and exported; sptensor.take_rows; and the numpy restatement of the
fold-in (tests/foldin_ref.py), which the GPU tests compare against, is pinned to scipy's NNLS and numpy's lstsq."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import foldin_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'aoadmm_hip.h')
capi = importlib.import_module('matlab-code_amd._capi')

CASES = [(3, 5), (3, 20), (2, 33), (4, 64)]                   # (N, R)


def declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(aoadmm_[a-z0-9_]+)\s*\(', text))


def test_entries_are_declared_bound_and_exported(pkg):
    lib = pkg.load_library()
    for name in ('aoadmm_resident_fold_in', 'aoadmm_resident_topk_w', 'aoadmm_tensor_rank'):
        assert name in declared() and name in pkg.SYMBOLS and hasattr(lib, name)
    assert hasattr(pkg.Engine, 'fold_in') and hasattr(pkg.Engine, 'topk_w') and hasattr(pkg.Engine, 'block_rank') and hasattr(pkg.sptensor, 'take_rows')
    assert lib.aoadmm_abi_version() == 3
    # aoadmm_foldin_options: double, int, int, double, double
    assert 'aoadmm_foldin_options' in open(HEADER).read()
    assert C.sizeof(capi.FoldinOptions) == 32
    assert [capi.FoldinOptions.constraint.offset, capi.FoldinOptions.max_inner.offset, capi.FoldinOptions.tol_primal.offset] == [8, 12, 16]


def test_take_rows_against_a_mask(pkg):
    rng = np.random.default_rng(0)
    shape = (9, 7, 5)
    keep = rng.random(shape) < 0.4
    X = rng.standard_normal(shape)
    S = pkg.sptensor(np.argwhere(keep), X[keep], shape)
    for mode, rows in [(0, [7, 2, 3]), (1, [0]), (2, [4, 1, 0, 2]), (0, [])]:
        subs, vals = S.take_rows(mode, rows)
        m = np.isin(S.subs[:, mode], rows)
        assert subs.shape == (int(m.sum()), 3) and subs.dtype == np.int64
        assert np.array_equal(vals, S.vals[m])
        back = subs.copy()
        back[:, mode] = np.asarray(rows, dtype=np.int64)[subs[:, mode]]
        assert np.array_equal(back, S.subs[m])
        for pos, r in enumerate(rows):
            assert int((subs[:, mode] == pos).sum()) == int(keep.take(r, axis=mode).sum())
    with pytest.raises(ValueError):
        S.take_rows(3, [0])
    with pytest.raises(ValueError):
        S.take_rows(0, [9])
    with pytest.raises(ValueError):
        S.take_rows(0, [1, 1])


def problem(N, R, seed=0, nq=3):
    rng = np.random.default_rng(seed)
    shape = [4 * R + 3, 4 * R + 1, 4 * R + 2, 4 * R][:N]
    shape[0] = 50
    U = [rng.standard_normal((s, R)) for s in shape]
    subs, vals = FR.make_list(rng, shape, 0, [4 * R + 8] * nq)
    return U, subs, vals


@pytest.mark.parametrize('N,R', CASES)
def test_the_restated_admm_loop_converges_to_nnls(N, R):
    """max_inner = 500, tolerances 0, ridge 0.1 against scipy.optimize.nnls on [Z; sqrt(ridge) I]: 1e-10 of max |u|
    (measured on the CPU: <= 2.6e-15)."""
    from scipy.optimize import nnls
    U, subs, vals = problem(N, R)
    ridge = 0.1
    G, b = FR.normal(U, 0, subs, vals, 3)
    z = FR.zrows(U, 0, subs)
    worst = 0.0
    for q in range(3):
        sel = np.flatnonzero(subs[:, 0] == q)
        A = np.vstack([z[sel], np.sqrt(ridge) * np.eye(R)])
        want, _ = nnls(A, np.concatenate([vals[sel], np.zeros(R)]), maxiter=100 * R)
        got, info, iters = FR.admm_row(G[q], b[q], ridge, 500)
        assert info == 0 and iters == 500 and (got >= 0).all()
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        worst = max(worst, err)
        assert err <= 1e-10, (q, err)
    print('worst distance to nnls: %.3g' % worst)


@pytest.mark.parametrize('N,R', CASES)
def test_the_restated_solve_is_lstsq(N, R):
    U, subs, vals = problem(N, R, seed=1)
    rows, info, iters = FR.fold_in(U, 0, subs, vals, 3)
    rows_ld, _, _ = FR.fold_in(U, 0, subs, vals, 3, dtype=FR.LD)
    z = FR.zrows(U, 0, subs)
    for q in range(3):
        sel = np.flatnonzero(subs[:, 0] == q)
        want = np.linalg.lstsq(z[sel], vals[sel], rcond=None)[0]
        assert info[q] == 0 and iters[q] == 0
        assert np.max(np.abs(rows[q] - want)) <= 1e-10 * np.max(np.abs(want))
        assert np.max(np.abs(rows_ld[q].astype(np.float64) - want)) <= 1e-10 * np.max(np.abs(want))


def test_the_restatement_reports_a_system_that_is_not_positive_definite():
    R = 4
    u, info = FR.solve_row(np.zeros((R, R)), np.zeros(R), 0.0)
    assert info == 1 and np.isnan(u).all()
    u, info = FR.solve_row(np.zeros((R, R)), np.zeros(R), 1.0)
    assert info == 0 and not u.any()
    z, info, it = FR.admm_row(np.zeros((R, R)), np.zeros(R), 1.0, 5)
    assert info == 0 and it == 1 and not z.any()


def test_no_cpu_fallback(pkg):
    """Without a GPU the call fails loudly: no engine can be made, and the entry itself refuses a null context with its
    outputs untouched."""
    lib = pkg.load_library()
    n = C.c_int(-1)
    assert lib.aoadmm_device_count(C.byref(n)) == 0
    if n.value == 0:
        with pytest.raises(pkg.AoadmmError) as ei:
            pkg.Engine(0)
        assert 'no CPU fallback' in str(ei.value)
    rows = np.full((2, 3), 0.5, order='F')
    info = np.full(2, 7, dtype=np.int32)
    subs = np.zeros((1, 3), dtype=np.int64, order='F')
    vals = np.ones(1)
    st = lib.aoadmm_resident_fold_in(None, 0, 0, 2, 1, subs.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(vals), None,
                                     capi.dptr(rows), info.ctypes.data_as(C.POINTER(C.c_int)), None, None, None)
    assert st != capi.OK and (rows == 0.5).all() and (info == 7).all()
    W = np.ones((2, 3), order='F')
    idx = np.full((2, 1), 77, dtype=np.int64)
    val = np.full((2, 1), 0.5)
    st = lib.aoadmm_resident_topk_w(None, 0, 0, 2, capi.dptr(W), 1, None, None, idx.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(val))
    assert st != capi.OK and (idx == 77).all() and (val == 0.5).all()
