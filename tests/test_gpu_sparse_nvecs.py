"""GPU: nvecs initialisation of sparse blocks by subspace iteration on the device (`aoadmm_resident_nvecs`,
DESIGN.md section 9.2).  The reference everywhere is numpy.linalg.eigh of the dense A @ A.T of the densified unfolding.

Bars (lam the exact spectrum, gap = (lam[r-1] - lam[r]) / lam[0]; Davis-Kahan bounds the subspace error of Ritz vectors
with residual rho by rho / gap):
    ||U - Uref Uref' U||_2 <= 2 * info.residual / gap + 1e-12,   max |U'U - I| <= 1e-12,
    |eigvals / lam[:r] - 1| <= 1e-10,   info.converged == 1,
and where every (lam[j] - lam[j+1]) / lam[0] >= 1e-2 for j < r: each column equals the reference column up to sign within
10 * rho / min-separation, its entry of largest magnitude positive."""
import copy
import importlib
import warnings

import numpy as np
import pytest

from helpers import options, script3_model

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')


# ---- inputs --------------------------------------------------------------------------------------------------------
def full_cp(factors, weights):
    X = np.zeros([f.shape[0] for f in factors])
    for j, w in enumerate(weights):
        t = np.asarray(w, dtype=np.float64)
        for f in factors:
            t = np.multiply.outer(t, f[:, j])
        X += t
    return X


def generator_a(rng, shape, dens, r0):
    """Spectral gap at r0: standard-normal factors, weights 2^-j, max |x| = 1, noise 0.02 N(0,1), density `dens`."""
    X = full_cp([rng.standard_normal((s, r0)) for s in shape], 2.0 ** -np.arange(r0))
    X /= np.abs(X).max()
    X += 0.02 * rng.standard_normal(shape)
    X[rng.random(shape) >= dens] = 0.0
    return X


def generator_b(rng, shape=(200, 64, 64), dens=0.1):
    """Decaying spectrum: orthonormalised random factors with 64 components, weights 0.85^j, max |x| = 1, no noise."""
    fac = [np.linalg.qr(rng.standard_normal((s, 64)))[0] for s in shape]
    X = full_cp(fac, 0.85 ** np.arange(64))
    X /= np.abs(X).max()
    X[rng.random(shape) >= dens] = 0.0
    return X


def unfold(X, n):
    return np.moveaxis(X, n, 0).reshape(X.shape[n], -1, order='F')


def spectrum(A):
    """Eigenvalues (descending) and eigenvectors of A @ A.T."""
    w, V = np.linalg.eigh(A @ A.T)
    return w[::-1].copy(), V[:, ::-1].copy()


def cp_Z(obj, shape, R):
    n = len(shape)
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(shape),
                coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
                constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[obj], _ranks=[R] * n)


def upload(pkg, eng, X, R):
    S = pkg.sptensor(np.argwhere(X), X[X != 0], X.shape)
    pkg.build_model(eng, cp_Z(S, X.shape, R))
    return S


def check_bars(U, ev, info, A, r, what=''):
    """Every bar of the module docstring against the dense unfolding A; prints each figure before it asserts."""
    lam, Vr = spectrum(A)
    rho = info['residual']
    gap = (lam[r - 1] - (lam[r] if r < len(lam) else 0.0)) / lam[0]
    Ur = Vr[:, :r]
    sub = np.linalg.norm(U - Ur @ (Ur.T @ U), 2)
    orth = np.abs(U.T @ U - np.eye(r)).max()
    eerr = np.abs(ev / lam[:r] - 1).max()
    seps = np.array([(lam[j] - (lam[j + 1] if j + 1 < len(lam) else 0.0)) / lam[0] for j in range(r)])
    print('%s r=%d b=%d F=%d it=%d conv=%d rho=%.3e gap=%.3e sub=%.3e bound=%.3e orth=%.3e eig=%.3e minsep=%.3e'
          % (what, r, info['block'], info['fibers'], info['iterations'], info['converged'], rho, gap, sub,
             2 * rho / gap + 1e-12, orth, eerr, seps.min()))
    assert info['converged'] == 1
    assert np.isfinite(U).all()
    assert sub <= 2 * rho / gap + 1e-12
    assert orth <= 1e-12
    assert eerr <= 1e-10
    assert np.all(np.diff(ev) <= 0)
    if seps.min() >= 1e-2:
        for c in range(r):
            d = min(np.abs(U[:, c] - Ur[:, c]).max(), np.abs(U[:, c] + Ur[:, c]).max())
            assert d <= 10 * rho / seps.min() + 1e-12, (c, d)
            assert U[np.argmax(np.abs(U[:, c])), c] > 0


# ---- 1. generator A: 2-way, 3-way, 4-way, short modes (G = 4 / 8), one carry level -----------------------------------------
A_CASES = [((40, 30, 20), 0.15, 3), ((300, 40, 30), 0.05, 4), ((33, 17, 9, 5), 0.2, 2), ((70, 45), 0.3, 3)]


@pytest.mark.parametrize('shape,dens,r0', A_CASES)
def test_generator_a_every_mode(pkg, eng, shape, dens, r0):
    X = generator_a(np.random.default_rng(0), shape, dens, r0)
    upload(pkg, eng, X, r0)
    for n in range(len(shape)):
        U, ev, info = eng.resident_nvecs(0, n, shape[n], r0)
        assert info['block'] == min(shape[n], r0 + 8)
        if len(shape) == 2:
            assert info['fibers'] == shape[1 - n]                       # no compaction for matrices
        else:
            assert info['fibers'] == len({tuple(np.delete(s, n)) for s in np.argwhere(X)})
        check_bars(U, ev, info, unfold(X, n), r0, 'A%s mode %d' % (shape, n))


# ---- 2. generator B: G = 16 / 32 / 64, b = 64, two carry levels ---------------------------------------------------------
@pytest.fixture(scope='module')
def gen_b():
    X = generator_b(np.random.default_rng(0))
    assert np.count_nonzero(X) > 256 * 128                               # two carry levels (82 090 nonzeros)
    return X


@pytest.mark.parametrize('r', [1, 3, 8, 9, 20, 24, 25, 40, 56])
@pytest.mark.parametrize('n', [0, 1])
def test_generator_b_rank_classes(pkg, eng, gen_b, n, r):
    upload(pkg, eng, gen_b, r)
    U, ev, info = eng.resident_nvecs(0, n, gen_b.shape[n], r, tol=1e-9)
    assert info['block'] == min(64, r + 8)
    check_bars(U, ev, info, unfold(gen_b, n), r, 'B mode %d' % n)


# ---- 3. skew: a full fiber of five chunks, a full row of eight (a row of this shape has 2000 cells) ------------------
def test_skewed_fiber_and_row(pkg, eng):
    """Hot fiber and hot row.  A row of mode 0 has 50 x 40 cells, so it cannot hold half of the 49 000 nonzeros: it is
    filled completely (2000 nonzeros, eight chunks)."""
    rng = np.random.default_rng(1)
    shape = (1200, 50, 40)
    X = generator_a(rng, shape, 0.02, 5)
    assert np.count_nonzero(X) == 48008
    X[:, 7, 11] = rng.standard_normal(1200)                              # one full fiber: 1200 nonzeros
    row = X[3]                                                           # one row of mode 0 without an empty cell
    empty = row == 0
    row[empty] = 0.05 * rng.standard_normal(int(empty.sum()))
    upload(pkg, eng, X, 5)
    for n in range(3):
        U, ev, info = eng.resident_nvecs(0, n, shape[n], 5)
        check_bars(U, ev, info, unfold(X, n), 5, 'skew mode %d' % n)


# ---- 4. duplicates, 5. seeds -----------------------------------------------------------------------------------------------
def test_duplicated_subscripts_same_bits(pkg, eng):
    X = generator_a(np.random.default_rng(2), (40, 30, 20), 0.15, 3)
    upload(pkg, eng, X, 3)
    want = [eng.resident_nvecs(0, n, X.shape[n], 3)[0] for n in range(3)]
    subs, vals = np.argwhere(X), X[X != 0]
    # every value split into two exactly representable halves at the same subscript, in a shuffled order
    perm = np.random.default_rng(3).permutation(2 * len(vals))
    subs2, vals2 = np.vstack([subs, subs])[perm], np.concatenate([vals / 2, vals / 2])[perm]
    eng.upload_coo(0, subs2, vals2)                                       # replaces the block's data; summed on the device
    for n in range(3):
        assert np.array_equal(eng.resident_nvecs(0, n, X.shape[n], 3)[0], want[n])


def test_same_seed_same_bits_other_seed_within_bar(pkg, eng):
    X = generator_a(np.random.default_rng(4), (300, 40, 30), 0.05, 4)
    upload(pkg, eng, X, 4)
    U1, e1, i1 = eng.resident_nvecs(0, 0, 300, 4, seed=5)
    U2, e2, i2 = eng.resident_nvecs(0, 0, 300, 4, seed=5)
    assert np.array_equal(U1, U2) and np.array_equal(e1, e2) and i1 == i2
    U3, e3, i3 = eng.resident_nvecs(0, 0, 300, 4, seed=6)
    assert not np.array_equal(U1, U3)
    check_bars(U1, e1, i1, unfold(X, 0), 4, 'seed 5')
    check_bars(U3, e3, i3, unfold(X, 0), 4, 'seed 6')


# ---- 6. rank deficiency --------------------------------------------------------------------------------------------------
def test_rank_deficient_unfolding(pkg, eng):
    rng = np.random.default_rng(6)
    X = np.zeros((60, 20, 10))
    X[:, 3, 2] = rng.standard_normal(60)
    X[:, 11, 7] = rng.standard_normal(60)
    upload(pkg, eng, X, 3)
    U, ev, info = eng.resident_nvecs(0, 0, 60, 3)
    print(info, ev)
    assert info['fibers'] == 2 and info['block'] == 3
    assert np.isfinite(U).all() and np.isfinite(ev).all()
    assert np.abs(U.T @ U - np.eye(3)).max() <= 1e-12
    Q = np.linalg.qr(unfold(X, 0)[:, [3 + 20 * 2, 11 + 20 * 7]])[0]       # the two-dimensional range
    assert np.linalg.norm(U[:, :2] - Q @ (Q.T @ U[:, :2]), 2) <= 1e-10
    lam, _ = spectrum(unfold(X, 0))
    assert np.abs(ev[:2] / lam[:2] - 1).max() <= 1e-10


# ---- 7. PARAFAC2 block with sparse slabs -----------------------------------------------------------------------------------
def test_parafac2_sparse_slabs_first_mode(pkg, eng):
    rng = np.random.default_rng(7)
    I, K, R = 50, 12, 3
    Jk = [int(j) for j in rng.integers(5, 16, K)]
    A = rng.standard_normal((I, R)) * 2.0 ** -np.arange(R)
    slabs = []
    for k in range(K):
        Xk = A @ rng.standard_normal((Jk[k], R)).T + 0.02 * rng.standard_normal((I, Jk[k]))
        Xk[rng.random(Xk.shape) >= 0.3] = 0.0
        slabs.append(Xk)
    objs = [pkg.sptensor(np.argwhere(Xk), Xk[Xk != 0], Xk.shape) for Xk in slabs]
    Z = dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=[I, Jk, K],
             coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
             constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[objs], _ranks=[R] * 3)
    pkg.build_model(eng, Z)
    U, ev, info = eng.resident_nvecs(0, 0, I, R)
    assert info['fibers'] == sum(Jk)
    check_bars(U, ev, info, np.hstack(slabs), R, 'PARAFAC2')              # Xcat Xcat' = sum_k X_k X_k'
    for pos, rows in ((1, Jk[0]), (2, K)):
        with pytest.raises(capi.UnsupportedOnDevice):
            eng.resident_nvecs(0, pos, rows, 2)


# ---- 8. errors ------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, eng):
    rng = np.random.default_rng(8)
    pkg.build_model(eng, cp_Z(rng.random((6, 5, 4)), (6, 5, 4), 2))
    with pytest.raises(capi.UnsupportedOnDevice):
        eng.resident_nvecs(0, 0, 6, 2)
    X = generator_a(rng, (12, 9, 7), 0.3, 2)
    upload(pkg, eng, X, 2)
    for r in (0, 13):
        with pytest.raises(capi.AoadmmError) as ei:
            eng.resident_nvecs(0, 0, 12, r)
        assert ei.value.code == capi.ERR_INVALID
    U = np.zeros((12, 2), order='F')
    st = eng.lib.aoadmm_resident_nvecs(eng.h, 0, 0, 2, None, capi.dptr(U), 11, None, None)      # ldU < I_n
    assert st == capi.ERR_INVALID
    st = eng.lib.aoadmm_resident_nvecs(eng.h, 0, 0, 2, None, capi.dptr(U), 12, None, None)      # null options / outputs
    assert st == capi.OK and np.abs(U.T @ U - np.eye(2)).max() <= 1e-12
    pkg.build_model(eng, cp_Z(pkg.sptensor(np.zeros((0, 3), dtype=np.int64), [], (12, 9, 7)), (12, 9, 7), 2))
    with pytest.raises(capi.AoadmmError) as ei:
        eng.resident_nvecs(0, 0, 12, 2)
    assert ei.value.code == capi.ERR_INVALID


# ---- 9. driver ------------------------------------------------------------------------------------------------------------
def test_driver_iterative_init_matches_gram(pkg, eng):
    """A sparse 3-way block coupled with a sparse matrix (the model of example script 3, generator-A data).  The two
    inits agree up to the sign of each column; for the solve the 'gram' init takes the device path's sign rule (LAPACK's
    signs are arbitrary and a non-negativity constraint is not invariant to them)."""
    rng = np.random.default_rng(9)
    Z, io = script3_model(rng)
    X1 = generator_a(rng, (50, 30, 40), 0.15, 4)
    X2 = generator_a(rng, (50, 70), 0.3, 3)
    Z['object'] = [pkg.sptensor(np.argwhere(X), X[X != 0], X.shape) for X in (X1, X2)]
    uploads = []
    orig = eng.upload_coo
    eng.upload_coo = lambda p, subs, vals: (uploads.append(p), orig(p, subs, vals))[1]
    try:
        G = {}
        for method in ('gram', 'iterative'):
            eng.kernel_stats(3, reset=True)
            uploads.clear()
            draw = np.random.default_rng(11)                     # the same draws for both inits
            io['distr'] = [lambda a, b: draw.random((a, b))] * 5
            with warnings.catch_warnings():
                warnings.simplefilter('error', RuntimeWarning)                 # converged: rho <= 1e-10
                G[method] = pkg.init_coupled_AOADMM_CMTF(Z, {**io, 'nvecs': 1, 'nvecs_method': method},
                                                         rng=np.random.default_rng(10), engine=eng)
            launches = eng.kernel_stats(3)[1]
            if method == 'gram':
                assert uploads == [] and launches == 0
            else:
                assert uploads == [0, 0], uploads             # two blocks, each one went up once as scratch tensor 0
                assert launches > 0 and launches % 2 == 0     # two passes per iteration
                assert eng._resident_model is None
    finally:
        del eng.upload_coo
    owner = {0: (X1, 0), 1: (X1, 1), 2: (X1, 2), 3: (X2, 0), 4: (X2, 1)}
    for m, (X, pos) in owner.items():
        Ug, Ui = G['gram']['fac'][m], G['iterative']['fac'][m]
        r = Ui.shape[1]
        lam, _ = spectrum(unfold(X, pos))
        gap = (lam[r - 1] - lam[r]) / lam[0]
        sub = np.linalg.norm(Ui - Ug @ (Ug.T @ Ui), 2)
        print('mode %d: gap %.3e subspace %.3e' % (m + 1, gap, sub))
        assert sub <= 2 * 1e-10 / gap + 1e-12
        seps = np.array([(lam[j] - lam[j + 1]) / lam[0] for j in range(r)])
        for c in range(r):
            s = 1.0 if Ug[np.argmax(np.abs(Ug[:, c])), c] > 0 else -1.0
            Ug[:, c] *= s
            if seps.min() >= 1e-2:
                assert np.abs(Ui[:, c] - Ug[:, c]).max() <= 10 * 1e-10 / seps.min() + 1e-12
    for key in ('constraint_fac', 'constraint_dual_fac', 'coupling_fac', 'coupling_dual_fac'):
        for a, b in zip(G['gram'][key], G['iterative'][key]):
            assert (a is None and b is None) or np.array_equal(a, b)            # the same draws
    opt = options(MaxOuterIters=3)
    outs = {k: pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G[k]), engine=eng)[3] for k in G}
    print(outs['gram']['func_val_conv'], outs['iterative']['func_val_conv'])
    assert np.allclose(outs['iterative']['func_val_conv'], outs['gram']['func_val_conv'], rtol=1e-8, atol=0)
