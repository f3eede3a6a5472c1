"""GPU: PARAFAC2 blocks whose slabs are sparse (Z.object{p}{k} as 2-way sptensors or scipy.sparse matrices;
cmtf_fun_AOADMM.m:163, :193, :221 only ever multiply a slab by a factor).  Operator parity of the three right-hand
sides against numpy on the densified slabs, solver equivalence with the dense HIP path and with the oracle, bitwise
reproducibility, a block no dense path could hold, the pass count, the multi-device context, and the refusals.

The solver tests run on noisy and sparsified data on purpose: the sparse path evaluates the data term as
||X||^2 - 2 <X, M> + ||M||^2, which loses digits against the oracle's direct residual only where the model fits the
data almost exactly (a noise-free, fully fitted model).  Here the data term ends between 0.40 and 0.68 of ||X||^2 (each
solver test prints the ratio per outer iteration)."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from helpers import options, par2_C_coupled_model, rel_fro, script1_model, script4_model
from test_gpu_solver import compare_par2
from test_gpu_sparse import assert_close, solve_three, sparsify, to_sptensor

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')


# ---- right-hand sides ------------------------------------------------------------------------------------------------
def par2_Z(objects, I, Jk, R):
    return dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=[I, list(Jk), len(Jk)],
                coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
                constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[objects], _ranks=[R] * 3)


def rhs_case(rng, R, I=300, nnz=20001, dup=500, zeros=40):
    """Ragged slabs (J_k = R among them), slab 2 without nonzeros, slab 4 holding half of all nonzeros, the first and
    last rows and the middle column of every slab empty, `dup` repeated subscripts, `zeros` explicit zeros; nnz + dup is
    no multiple of the kernels' chunk of 256."""
    Jk = [R + 5, R, R + 17, R + 2, R + 40, R + 9, R + 1]
    K = len(Jk)
    k = rng.choice([0, 1, 3, 5, 6], nnz)
    k[: nnz // 2] = 4
    j = np.array([rng.integers(0, Jk[kk]) for kk in k])
    mid = np.array([Jk[kk] // 2 for kk in k])
    j = np.where(j == mid, (mid + 1) % np.array([Jk[kk] for kk in k]), j)
    i = rng.integers(1, I - 1, nnz)
    subs = np.stack([i, j, k], axis=1)
    vals = rng.standard_normal(nnz)
    vals[rng.choice(nnz, zeros, replace=False)] = 0.0
    pick = rng.choice(nnz, dup)
    subs = np.vstack([subs, subs[pick]])
    vals = np.concatenate([vals, rng.standard_normal(dup)])
    assert (nnz + dup) % 256 != 0
    return I, Jk, K, subs, vals


def densify(subs, vals, I, Jk):
    X = [np.zeros((I, j)) for j in Jk]
    for k in range(len(Jk)):
        m = subs[:, 2] == k
        np.add.at(X[k], (subs[m, 0], subs[m, 1]), vals[m])
    return X


def ref_rhs(X, A, B, Cf):
    """numpy on dense slabs: sum_k X_k B_k D_k (I x R), X_k' A D_k per slab, diag(A' X_k B_k) (K x R)."""
    K = len(X)
    m0 = sum(X[k] @ B[k] * Cf[k][None, :] for k in range(K))
    m1 = [X[k].T @ A * Cf[k][None, :] for k in range(K)]
    m2 = np.stack([np.sum(A * (X[k] @ B[k]), axis=0) for k in range(K)])
    return m0, m1, m2


@pytest.mark.parametrize('R', [1, 3, 8, 20, 33, 64])
def test_rhs_parity(pkg, eng, R):
    rng = np.random.default_rng(100 + R)
    I, Jk, K, subs, vals = rhs_case(rng, R)
    slabs = [pkg.sptensor(subs[subs[:, 2] == k][:, :2], vals[subs[:, 2] == k], (I, Jk[k])) for k in range(K)]
    Z = par2_Z(slabs, I, Jk, R)
    pkg.build_model(eng, Z)
    A, Cf = rng.standard_normal((I, R)), rng.standard_normal((K, R))
    B = [rng.standard_normal((j, R)) for j in Jk]
    pkg.upload_state(eng, Z, {'fac': [A, B, Cf]})
    X = densify(subs, vals, I, Jk)
    want = ref_rhs(X, A, B, Cf)
    scale = ref_rhs([np.abs(x) for x in X], np.abs(A), [np.abs(b) for b in B], np.abs(Cf))
    Jtot = sum(Jk)
    pack = lambda cells: np.concatenate([c.ravel(order='F') for c in cells])
    got0 = eng.resident_par2_rhs(0, 0, I, R)
    got1 = eng.resident_par2_rhs(0, 1, Jtot, R)
    got2 = eng.resident_par2_rhs(0, 2, K, R)
    assert_close(got0, want[0], scale=scale[0])
    assert_close(got1, pack(want[1]), scale=pack(scale[1]))
    assert_close(got2, want[2], scale=scale[2])
    # rows, columns and slabs without nonzeros are exact zeros
    assert np.all(got0[0] == 0) and np.all(got0[-1] == 0)
    assert np.all(got2[2] == 0)
    o = np.concatenate([[0], np.cumsum(Jk)])
    for k in range(K):
        Gk = got1[o[k] * R:o[k + 1] * R].reshape((Jk[k], R), order='F')
        assert np.all(Gk[Jk[k] // 2] == 0) or Jk[k] < 2
    assert np.all(got1[o[2] * R:o[3] * R] == 0)
    normsq = C.c_double(0)
    capi.check(eng.lib.aoadmm_tensor_normsq(eng.h, 0, C.byref(normsq)))
    assert normsq.value == pytest.approx(sum(float(np.sum(x * x)) for x in X), rel=1e-12)
    # every call runs its pass again, with the same bits
    assert np.array_equal(eng.resident_par2_rhs(0, 0, I, R), got0)
    assert np.array_equal(eng.resident_par2_rhs(0, 1, Jtot, R), got1)


def test_rhs_no_nonzeros_and_scipy_slabs(pkg, eng):
    sps = pytest.importorskip('scipy.sparse')
    rng = np.random.default_rng(7)
    I, Jk, R = 9, [4, 6, 5], 3
    A, Cf = rng.random((I, R)), rng.random((3, R))
    B = [rng.random((j, R)) for j in Jk]
    Z = par2_Z([sps.csr_matrix((I, j)) for j in Jk], I, Jk, R)
    pkg.build_model(eng, Z)
    pkg.upload_state(eng, Z, {'fac': [A, B, Cf]})
    for mode, rows in ((0, I), (1, sum(Jk)), (2, 3)):
        assert np.all(eng.resident_par2_rhs(0, mode, rows, R) == 0)
    X = [sparsify(rng.random((I, j)), rng) for j in Jk]
    Z = par2_Z([sps.csc_matrix(x) for x in X], I, Jk, R)
    pkg.build_model(eng, Z)
    pkg.upload_state(eng, Z, {'fac': [A, B, Cf]})
    assert_close(eng.resident_par2_rhs(0, 0, I, R), ref_rhs(X, A, B, Cf)[0])


# ---- solver equivalence ----------------------------------------------------------------------------------------------
def sparse_pair(pkg, Z, p, rng, keep):
    """(Z with block p's slabs sparsified and dense, the same with the slabs as 2-way sptensors)."""
    Zd = dict(Z)
    Zd['object'] = list(Z['object'])
    Zd['object'][p] = [sparsify(Xk, rng, keep) for Xk in Z['object'][p]]
    Zs = dict(Zd)
    Zs['object'] = list(Zd['object'])
    Zs['object'][p] = [to_sptensor(pkg, Xk) for Xk in Zd['object'][p]]
    return Zd, Zs


def assert_same_par2_solve(Fd, od, Fs, os_, tol=1e-10):
    def each(a, b, key):
        if a is None:
            return
        if isinstance(a, (list, tuple)):
            for x, y in zip(a, b):
                each(x, y, key)
        elif isinstance(a, dict):
            for k in a:
                each(a[k], b[k], key)
        else:
            assert rel_fro(b, a) < tol, (key, rel_fro(b, a))
    for key in ('fac', 'constraint_fac', 'constraint_dual_fac', 'coupling_fac', 'coupling_dual_fac', 'DeltaB', 'P', 'mu_DeltaB'):
        each(Fd[key], Fs[key], key)
    assert os_['OuterIterations'] == od['OuterIterations']
    assert np.array_equal(os_['innerIters'], od['innerIters'])
    for k in ('func_val_conv', 'func_coupl_conv', 'func_constr_conv', 'func_PAR2_coupl'):
        print(k, np.max(np.abs(os_[k] - od[k]) / np.maximum(np.abs(od[k]), 1e-300)))
        assert np.allclose(os_[k], od[k], rtol=tol, atol=1e-14), (k, os_[k], od[k])


def run_par2_case(pkg, eng, Z, io, opt, p, keep, seed=7):
    Zd, Zs = sparse_pair(pkg, Z, p, np.random.default_rng(seed + 1), keep)
    (Fo, oo), (Fd, od), (Fs, os_) = solve_three(pkg, eng, Zd, Zs, io, opt, seed)
    nrm = sum(float(np.sum(x * x)) for x in Zd['object'][p])
    print('f_tensors / (w ||X||^2):', oo['func_val_conv'] / (Z['weights'][p] * nrm))
    assert np.all(np.isfinite(oo['func_val_conv']))
    assert_same_par2_solve(Fd, od, Fs, os_)
    compare_par2(Fo, oo, Fs, os_)


def test_solve_script4(pkg, eng):
    rng = np.random.default_rng(21)
    Z, io = script4_model(rng, K=12)
    run_par2_case(pkg, eng, Z, io, options(MaxOuterIters=10), 0, 0.4)


def test_solve_forty_slabs_rank5_empty_columns(pkg, eng):
    rng = np.random.default_rng(22)
    Z, io = script4_model(rng, K=40, R=5)
    Zd, _ = sparse_pair(pkg, Z, 0, np.random.default_rng(8), 0.15)
    assert any(np.any(np.all(x == 0, axis=0)) for x in Zd['object'][0])      # 15 % kept leaves empty columns
    run_par2_case(pkg, eng, Z, io, options(MaxOuterIters=8), 0, 0.15)


def test_solve_script1_cp_coupled_to_sparse_parafac2(pkg, eng):
    rng = np.random.default_rng(23)
    Z, io = script1_model(rng)
    run_par2_case(pkg, eng, Z, io, options(MaxOuterIters=10), 1, 0.4)


def test_solve_constrained_Bk(pkg, eng):
    rng = np.random.default_rng(24)
    Z, io = script4_model(rng, constraints_B=('non-negativity',))
    run_par2_case(pkg, eng, Z, io, options(MaxOuterIters=8), 0, 0.4)


def test_solve_coupled_C_mode(pkg, eng):
    rng = np.random.default_rng(25)
    Z, io = par2_C_coupled_model(rng, 0)
    run_par2_case(pkg, eng, Z, io, options(MaxOuterIters=8), 1, 0.4)


def test_solve_rank9_four_launch_Bk_loop(pkg, eng):
    rng = np.random.default_rng(26)
    Z, io = script4_model(rng, K=5, R=9)
    run_par2_case(pkg, eng, Z, io, options(MaxOuterIters=6), 0, 0.4)


def _one_sparse_model(pkg, seed=27):
    rng = np.random.default_rng(seed)
    Z, io = script4_model(rng, K=12)
    Zd, Zs = sparse_pair(pkg, Z, 0, rng, 0.4)
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=rng)
    return Zs, G


def test_solve_bitwise_reproducible(pkg, eng):
    Zs, G = _one_sparse_model(pkg)
    outs = [pkg.cmtf_AOADMM(Zs, alg_options=options(MaxOuterIters=8), init=copy.deepcopy(G), engine=eng) for _ in range(2)]
    F0, F1 = outs[0][1], outs[1][1]
    assert np.array_equal(F0['fac'][0], F1['fac'][0]) and np.array_equal(F0['fac'][2], F1['fac'][2])
    for a, b in zip(F0['fac'][1] + F0['P'][0] + F0['mu_DeltaB'][0], F1['fac'][1] + F1['P'][0] + F1['mu_DeltaB'][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(F0['DeltaB'][0], F1['DeltaB'][0])
    for k in ('func_val_conv', 'func_PAR2_coupl', 'func_constr_conv'):
        assert np.array_equal(outs[0][3][k], outs[1][3][k])


def test_two_passes_per_outer_iteration(pkg, eng):
    """Uncoupled block: one pass over the row-sorted copy (mode A) and one over the column-sorted copy (Y = X' A, shared
    by the B_k update, the C update and the objective) per outer iteration, plus the first objective and the A pass
    prepared ahead of an iteration that the stopping test may cancel."""
    Zs, G = _one_sparse_model(pkg, seed=28)
    eng.kernel_stats(3, reset=True)
    _, _, _, out = pkg.cmtf_AOADMM(Zs, alg_options=options(MaxOuterIters=7), init=copy.deepcopy(G), engine=eng)
    ms, launches, by, fl = eng.kernel_stats(3)
    print('passes', launches, 'outer iterations', out['OuterIterations'])
    assert 0 < launches <= 2 * out['OuterIterations'] + 2
    nz = sum(s.nnz for s in Zs['object'][0])
    assert fl == pytest.approx(launches * nz * 3 * 2) and by > 0 and ms > 0


# ---- beyond dense reach ----------------------------------------------------------------------------------------------
def device_mem_free():
    try:
        hip = C.CDLL('libamdhip64.so')
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    except OSError:
        import torch
        return torch.cuda.mem_get_info()[0]


def test_beyond_dense_reach(pkg, eng):
    """I = 30 000, K = 3 000 ragged slabs (J_k in 20..80), 3e6 nonzeros, R = 5: the dense path would hold 36 GB of slabs
    and a 3.6 GB X_k B_k intermediate.  Random data has no low rank: f_tensors stays near ||X||^2, the expansion of
    the data term cancels nothing."""
    rng = np.random.default_rng(29)
    I, K, R, nnz = 30_000, 3_000, 5, 3_000_000
    Jk = rng.integers(20, 81, K)
    off = np.concatenate([[0], np.cumsum(Jk)])
    Jtot = int(off[-1])
    g = rng.integers(0, Jtot, nnz)
    i = rng.integers(0, I, nnz)
    order = np.argsort(g, kind='stable')
    g, i = g[order], i[order]
    vals = rng.random(nnz)
    kk = np.searchsorted(off, g, side='right') - 1
    cut = np.searchsorted(g, off)
    slabs = [pkg.sptensor(np.stack([i[cut[k]:cut[k + 1]], g[cut[k]:cut[k + 1]] - off[k]], axis=1), vals[cut[k]:cut[k + 1]],
                          (I, int(Jk[k]))) for k in range(K)]
    Z = dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=[I, [int(j) for j in Jk], K],
             coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
             constrained_modes=[0, 0, 1], constraints=[None, None, ('non-negativity',)], weights=[1.0], object=[slabs])
    distr = [lambda a, b: rng.standard_normal((a, b)), lambda a, b: rng.standard_normal((a, b)), lambda a, b: rng.random((a, b)) + 0.1]
    io = dict(lambdas_init=[[1] * R], nvecs=0, distr=distr, normalize=1)
    G = pkg.init_coupled_AOADMM_CMTF(Z, io, rng=rng, engine=eng)
    eng.synchronize()
    free0 = device_mem_free()
    _, F, _, out = pkg.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=3, MaxInnerIters=5), init=G, engine=eng)
    eng.synchronize()
    grown = free0 - device_mem_free()
    print('device memory in use grew by %.1f MB; T1 of the dense path alone: %.1f MB' % (grown / 1e6, K * I * R * 8 / 1e6))
    assert grown < K * I * R * 8
    f = out['func_val_conv']
    assert out['OuterIterations'] == 3 and np.all(np.isfinite(f))
    A, Bl, Cf = F['fac']
    assert all(np.all(np.isfinite(x)) for x in [A, Cf] + list(Bl))
    # the same expansion in numpy from the returned factors and the coalesced COO data
    sub = np.vstack([np.column_stack([s.subs, np.full(s.nnz, k)]) for k, s in enumerate(slabs)])
    v = np.concatenate([s.vals for s in slabs])
    Bcat = np.vstack(Bl)
    gg = off[sub[:, 2]] + sub[:, 1]
    cross = float(np.sum(v * np.sum(A[sub[:, 0]] * Bcat[gg] * Cf[sub[:, 2]], axis=1)))
    GA = A.T @ A
    model = sum(float(np.sum(GA * np.outer(Cf[k], Cf[k]) * (Bl[k].T @ Bl[k]))) for k in range(K))
    want = float(np.sum(v * v)) - 2.0 * cross + model
    print('f_tensors', out['f_tensors'], 'numpy', want, '||X||^2', float(np.sum(v * v)))
    assert out['f_tensors'] == pytest.approx(want, rel=1e-9)


# ---- multi-device context --------------------------------------------------------------------------------------------
def test_multi_device_sparse_parafac2_with_row_sharded_dense_tensor(pkg, eng):
    """Engine([0, 0]): the sparse PARAFAC2 block is replicated on both engines, the CP tensor coupled to its A mode is
    row-sharded."""
    rng = np.random.default_rng(30)
    Z, io = script1_model(rng, noise=0.1)
    Zd, Zs = sparse_pair(pkg, Z, 1, rng, 0.4)
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=rng)
    opt = options(MaxOuterIters=8)
    _, F1, _, o1 = pkg.cmtf_AOADMM(Zs, alg_options=opt, init=copy.deepcopy(G), engine=eng)
    with pkg.Engine([0, 0]) as e2:
        _, F2, _, o2 = pkg.cmtf_AOADMM(Zs, alg_options=opt, init=copy.deepcopy(G), engine=e2)
    for key in ('fac', 'coupling_fac'):
        for a, b in zip(F1[key], F2[key]):
            if a is None:
                continue
            for x, y in zip(a, b) if isinstance(a, list) else [(a, b)]:
                assert rel_fro(y, x) < 1e-12, (key, rel_fro(y, x))
    assert np.allclose(o2['func_val_conv'], o1['func_val_conv'], rtol=1e-12, atol=0)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals(pkg, eng):
    rng = np.random.default_rng(31)
    I, Jk, R = 10, [4, 6, 5], 3
    K = len(Jk)
    X = [sparsify(rng.random((I, j)), rng) for j in Jk]
    Z = par2_Z([to_sptensor(pkg, x) for x in X], I, Jk, R)
    pkg.build_model(eng, Z)
    A, Cf = rng.random((I, R)), rng.random((K, R))
    B = [rng.random((j, R)) for j in Jk]
    pkg.upload_state(eng, Z, {'fac': [A, B, Cf]})
    subs, vals = pkg.pack_par2_slabs(Z['object'][0], I, Jk)

    def invalid(call):
        with pytest.raises(pkg.AoadmmError) as ei:
            call()
        assert ei.value.code == capi.ERR_INVALID, str(ei.value)

    mask = np.ones((I, Jk[1]), dtype=np.uint8, order='F')
    invalid(lambda: capi.check(eng.lib.aoadmm_par2_slab_mask_upload(eng.h, 0, 1, mask.ctypes.data_as(C.POINTER(C.c_uint8)))))
    invalid(lambda: capi.check(eng.lib.aoadmm_par2_slab_upload(eng.h, 0, 1, capi.dptr(np.asfortranarray(X[1])))))
    with pytest.raises(pkg.UnsupportedOnDevice):
        eng.resident_unfold_gram(0, 0, I)
    for col, lim in ((0, I), (1, Jk[2]), (2, K)):           # j = J_k of its own slab is out of range too
        bad = subs.copy()
        row = int(np.flatnonzero(subs[:, 2] == 2)[0])
        bad[row, col] = lim
        invalid(lambda: eng.upload_par2_coo(0, bad, vals))
        bad[row, col] = -1
        invalid(lambda: eng.upload_par2_coo(0, bad, vals))
    invalid(lambda: capi.check(eng.lib.aoadmm_par2_slab_upload_coo(eng.h, 0, -1, None, None)))
    # the block still holds the sparse slabs after the refused calls
    want = ref_rhs(X, A, B, Cf)
    assert_close(eng.resident_par2_rhs(0, 0, I, R), want[0])
    assert_close(eng.resident_par2_rhs(0, 2, K, R), want[2])
    # the right-hand-side entry is for sparse slabs; a dense upload of all slabs replaces them and solves as before
    Xall = np.concatenate([x.ravel(order='F') for x in X])
    capi.check(eng.lib.aoadmm_par2_slab_upload(eng.h, 0, capi.ALL_SLABS, capi.dptr(Xall)))
    invalid(lambda: eng.resident_par2_rhs(0, 0, I, R))
    assert np.allclose(eng.resident_unfold_gram(0, 0, I), sum(x @ x.T for x in X), rtol=1e-12, atol=1e-14)
    rng = np.random.default_rng(32)
    Zm, io = script4_model(rng, K=6)
    Zd, Zs = sparse_pair(pkg, Zm, 0, rng, 0.4)
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=rng)
    opt = options(MaxOuterIters=5)
    _, Fo, _, oo = OA.cmtf_AOADMM(Zd, alg_options=opt, init=copy.deepcopy(G))
    pkg.cmtf_AOADMM(Zs, alg_options=opt, init=copy.deepcopy(G), engine=eng)
    # same model, same engine: the dense slabs go up over the sparse ones
    Zd['_ranks'] = [3, 3, 3]
    Xall = np.concatenate([np.asarray(x).ravel(order='F') for x in Zd['object'][0]])
    capi.check(eng.lib.aoadmm_par2_slab_upload(eng.h, 0, capi.ALL_SLABS, capi.dptr(Xall)))
    pkg.upload_state(eng, Zd, G)
    og = pkg.run_solver(eng, opt, 3)
    Fg = pkg.download_state(eng, Zd, G)
    compare_par2(Fo, oo, Fg, og)


def test_f32_precision_leaves_sparse_slabs_fp64(pkg, eng):
    Zs, G = _one_sparse_model(pkg, seed=33)
    opt = options(MaxOuterIters=4)
    _, F64, _, o64 = pkg.cmtf_AOADMM(Zs, alg_options=opt, init=copy.deepcopy(G), engine=eng)
    _, F32, _, o32 = pkg.cmtf_AOADMM(Zs, alg_options=opt, init=copy.deepcopy(G), engine=eng, precision='f32')
    assert np.array_equal(F64['fac'][0], F32['fac'][0]) and np.array_equal(o64['func_val_conv'], o32['func_val_conv'])
