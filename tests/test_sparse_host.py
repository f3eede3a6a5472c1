"""CPU: the sptensor class, build_model's checks for sparse CP blocks (cmtf_AOADMM.m:77-79) and the host Gram matrix of
a sparse unfolding (cmtf_nvecs.m:41-42).  No GPU: build_model runs against a stand-in engine whose C calls succeed."""
import importlib

import numpy as np
import pytest

sp_mod = importlib.import_module('matlab-code_amd.sptensor')


def _dense_unfold(X, n):
    return np.moveaxis(X, n, 0).reshape(X.shape[n], -1, order='F')


def test_sptensor_sums_duplicates_and_orders_column_major(pkg):
    X = pkg.sptensor([[1, 0, 2], [0, 1, 0], [1, 0, 2], [0, 0, 0]], [1.0, 2.0, 3.5, -1.0], (2, 2, 3))
    assert X.nnz == 3
    assert X.subs.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 2]]       # column-major linear order
    assert X.vals.tolist() == [-1.0, 2.0, 4.5]
    F = X.full()
    assert F[1, 0, 2] == 4.5 and F[0, 1, 0] == 2.0 and F[0, 0, 0] == -1.0 and F.sum() == 5.5


@pytest.mark.parametrize('subs', [[[0, 2]], [[-1, 0]], [[0, 0, 0]]])
def test_sptensor_rejects_bad_subscripts(pkg, subs):
    with pytest.raises(ValueError):
        pkg.sptensor(subs, [1.0], (3, 2))


def test_sptensor_full_round_trip(pkg):
    rng = np.random.default_rng(0)
    X = rng.random((5, 4, 3, 2))
    X[X < 0.6] = 0.0
    S = pkg.sptensor(np.argwhere(X), X[X != 0], X.shape)
    assert np.array_equal(S.full(), X)
    assert S.nnz == np.count_nonzero(X)
    E = pkg.sptensor(np.zeros((0, 3), dtype=np.int64), [], (3, 4, 5))
    assert E.nnz == 0 and not E.full().any()


def test_coo_of_scipy_matrix(pkg):
    sps = pytest.importorskip('scipy.sparse')
    M = sps.random(7, 5, density=0.4, random_state=1, format='csc')
    subs, vals, shape = sp_mod.coo_of(M)
    S = pkg.sptensor(subs, vals, shape)
    assert np.allclose(S.full(), M.toarray(), rtol=0, atol=0)


class _Lib:
    def __getattr__(self, name):
        return lambda *a: 0


class _Eng:
    """Stand-in for an Engine: every C call succeeds, uploads are recorded."""
    lib = _Lib()
    h = None

    def __init__(self):
        self.coo = []

    def upload_coo(self, p, subs, vals):
        self.coo.append((p, subs, vals))


def _sparse_model(pkg, shape=(6, 5, 4), miss=None):
    rng = np.random.default_rng(3)
    X = rng.random(shape)
    X[X < 0.5] = 0
    S = pkg.sptensor(np.argwhere(X), X[X != 0], shape)
    n = len(shape)
    Z = dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(shape),
             coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
             constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[S], _ranks=[2] * n)
    if miss is not None:
        Z['miss'] = [miss]
    return Z, S, X


def test_build_model_uploads_sparse_block(pkg):
    Z, S, _ = _sparse_model(pkg)
    e = _Eng()
    pkg.build_model(e, Z)
    assert len(e.coo) == 1 and e.coo[0][0] == 0
    assert np.array_equal(e.coo[0][1], S.subs) and np.array_equal(e.coo[0][2], S.vals)


def test_build_model_rejects_miss_on_sparse_block(pkg):
    Z, _, X = _sparse_model(pkg, miss=np.ones((6, 5, 4)))
    with pytest.raises(ValueError, match=r'Missing data \(Z.miss\) not supported for sptensor objects. Convert to tensor first.'):
        pkg.build_model(_Eng(), Z)


def test_build_model_rejects_shape_mismatch(pkg):
    Z, _, _ = _sparse_model(pkg)
    Z['size'] = [6, 5, 5]
    with pytest.raises(ValueError, match='has size'):
        pkg.build_model(_Eng(), Z)


@pytest.mark.parametrize('shape', [(9, 7), (6, 5, 4), (4, 3, 5, 2)])
def test_sparse_unfold_gram_matches_dense(shape):
    pytest.importorskip('scipy.sparse')
    rng = np.random.default_rng(5)
    X = rng.standard_normal(shape)
    X[rng.random(shape) < 0.7] = 0.0
    subs = np.argwhere(X)
    vals = X[X != 0]
    for n in range(len(shape)):
        A = _dense_unfold(X, n)
        Y = sp_mod.unfold_gram(subs, vals, shape, n)
        ref = A @ A.T
        assert np.allclose(Y, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


def test_cmtf_nvecs_of_sparse_block_needs_no_device(pkg):
    pytest.importorskip('scipy.sparse')
    Z, S, X = _sparse_model(pkg, shape=(8, 6, 5))
    for n in range(3):
        U = pkg.cmtf_nvecs(Z, n, 2)                   # no engine: the sparse path is host-only
        A = _dense_unfold(X, n)
        w, V = np.linalg.eigh(A @ A.T)
        ref = V[:, np.argsort(-np.abs(w))[:2]]
        for r in range(2):
            assert min(np.abs(U[:, r] - ref[:, r]).max(), np.abs(U[:, r] + ref[:, r]).max()) < 1e-10
