"""Host side of PARAFAC2 blocks with sparse slabs (no GPU): packing ragged sparse slabs into (i, j, k) subscripts from
`sptensor` and scipy inputs, duplicates and explicit zeros, the refusals of build_model, and the Gram matrices that
init_options.nvecs = 1 takes on the host without densifying a slab."""
import importlib

import numpy as np
import pytest

from test_sparse_host import _Eng

JK = [5, 3, 7, 4]
I = 6


class _Eng2(_Eng):
    def __init__(self):
        super().__init__()
        self.par2 = []
        self.dense = []

    def upload_par2_coo(self, p, subs, vals):
        self.par2.append((p, np.array(subs), np.array(vals)))


def _slabs(rng, keep=0.4):
    X = []
    for j in JK:
        Xk = rng.standard_normal((I, j))
        Xk[rng.random(Xk.shape) > keep] = 0.0
        X.append(Xk)
    X[1][:] = 0.0                                     # a slab without nonzeros
    return X


def _model(objects, miss=None, size=None):
    Z = dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=size or [I, list(JK), len(JK)],
             coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
             constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[objects], _ranks=[2, 2, 2])
    if miss is not None:
        Z['miss'] = [miss]
    return Z


def _densify(subs, vals):
    out = [np.zeros((I, j)) for j in JK]
    for (i, j, k), v in zip(subs, vals):
        out[k][i, j] += v
    return out


def _sp(pkg, Xk):
    return pkg.sptensor(np.argwhere(Xk), Xk[Xk != 0], Xk.shape)


def test_pack_sptensor_slabs(pkg):
    X = _slabs(np.random.default_rng(0))
    subs, vals = pkg.pack_par2_slabs([_sp(pkg, x) for x in X], I, JK)
    assert subs.dtype == np.int64 and subs.shape == (sum(np.count_nonzero(x) for x in X), 3)
    assert not np.any(subs[:, 2] == 1)                # the empty slab contributes nothing
    for k, j in enumerate(JK):                        # j is local to its slab
        assert np.all(subs[subs[:, 2] == k, 1] < j)
    for a, b in zip(_densify(subs, vals), X):
        assert np.array_equal(a, b)


def test_pack_scipy_slabs_keeps_duplicates_and_explicit_zeros(pkg):
    sps = pytest.importorskip('scipy.sparse')
    X = _slabs(np.random.default_rng(1))
    slabs = [sps.csc_matrix(x) for x in X]
    # slab 2 as COO with a duplicated subscript and an explicit zero: both reach the device untouched
    slabs[2] = sps.coo_matrix((np.array([1.5, 2.5, 0.0]), (np.array([3, 3, 0]), np.array([6, 6, 2]))), shape=(I, JK[2]))
    subs, vals = pkg.pack_par2_slabs(slabs, I, JK)
    s2 = subs[:, 2] == 2
    assert s2.sum() == 3 and sorted(vals[s2].tolist()) == [0.0, 1.5, 2.5]
    want = list(X)
    want[2] = np.zeros((I, JK[2]))
    want[2][3, 6] = 4.0
    for a, b in zip(_densify(subs, vals), want):
        assert np.array_equal(a, b)


def test_sptensor_slab_sums_duplicates_on_construction(pkg):
    S = pkg.sptensor([[1, 2], [1, 2], [0, 0]], [1.0, 2.0, 0.0], (I, JK[0]))
    subs, vals = pkg.pack_par2_slabs([S], I, JK[:1])
    assert subs.tolist() == [[0, 0, 0], [1, 2, 0]] and vals.tolist() == [0.0, 3.0]


def test_build_model_uploads_sparse_slabs(pkg):
    X = _slabs(np.random.default_rng(2))
    e = _Eng2()
    pkg.build_model(e, _model([_sp(pkg, x) for x in X]))
    assert len(e.par2) == 1 and e.par2[0][0] == 0 and not e.coo
    for a, b in zip(_densify(e.par2[0][1], e.par2[0][2]), X):
        assert np.array_equal(a, b)


def test_build_model_rejects_mixed_slabs(pkg):
    X = _slabs(np.random.default_rng(3))
    objs = [_sp(pkg, x) for x in X]
    objs[2] = X[2]
    with pytest.raises(ValueError, match='all sparse or all dense'):
        pkg.build_model(_Eng2(), _model(objs))


def test_build_model_rejects_wrong_slab_shape(pkg):
    X = _slabs(np.random.default_rng(4))
    objs = [_sp(pkg, x) for x in X]
    size = [I, [5, 3, 8, 4], len(JK)]
    with pytest.raises(ValueError, match=r'Z.object\{1\}\{3\} has size \(6, 7\), Z.size says \[6, 8\]'):
        pkg.build_model(_Eng2(), _model(objs, size=size))


def test_build_model_rejects_miss_on_sparse_slabs(pkg):
    X = _slabs(np.random.default_rng(5))
    miss = [np.ones_like(x) for x in X]
    with pytest.raises(ValueError, match=r'Missing data \(Z.miss\) not supported for sparse PARAFAC2 slabs'):
        pkg.build_model(_Eng2(), _model([_sp(pkg, x) for x in X], miss=miss))


def test_host_gram_of_sparse_slabs_equals_dense(pkg):
    pytest.importorskip('scipy.sparse')
    spm = importlib.import_module('matlab-code_amd.sptensor')
    X = _slabs(np.random.default_rng(6), keep=0.6)
    S = [_sp(pkg, x) for x in X]
    YA = sum(spm.slab_gram(s, 0) for s in S)
    want = sum(x @ x.T for x in X)
    assert np.max(np.abs(YA - want)) <= 1e-12 * np.max(np.abs(want))
    for s, x in zip(S, X):
        Yk = spm.slab_gram(s, 1)
        assert Yk.shape == (x.shape[1], x.shape[1])
        assert np.max(np.abs(Yk - x.T @ x)) <= 1e-12 * max(np.max(np.abs(x.T @ x)), 1.0)


def test_nvecs_init_of_sparse_slabs_needs_no_device(pkg):
    """init_options.nvecs = 1: the A mode and every B_k come from host Gram matrices of the sparse slabs and span the
    same subspaces as those of the densified slabs."""
    pytest.importorskip('scipy.sparse')
    rng = np.random.default_rng(7)
    X = _slabs(rng, keep=0.8)
    X[1] = rng.standard_normal((I, JK[1]))
    R = 2
    io = dict(lambdas_init=[[1] * R], nvecs=1, distr=[lambda a, b: rng.random((a, b))] * 3, normalize=1)

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError('the device was asked for ' + name)

    G = pkg.init_coupled_AOADMM_CMTF(_model([_sp(pkg, x) for x in X]), io, rng=np.random.default_rng(1), engine=NoDevice())

    def lead(Y):
        w, V = np.linalg.eigh(Y)
        return V[:, np.argsort(-np.abs(w))[:R]]

    UA = lead(sum(x @ x.T for x in X))
    assert np.allclose(G['fac'][0] @ G['fac'][0].T, UA @ UA.T, atol=1e-10)
    for k, x in enumerate(X):
        Uk = lead(x.T @ x)
        assert np.allclose(G['fac'][1][k] @ G['fac'][1][k].T, Uk @ Uk.T, atol=1e-10)
