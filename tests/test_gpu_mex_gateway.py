"""The MEX gateway (matlab-code_amd/mex/aoadmm_mex.cpp) against the real library: compiled with the mock of the C Matrix
API (tests/mxmock/mxmock.cpp), linked to libaoadmm_hip.so and run in this process beside `pkg.cmtf_AOADMM`.

driver.py is the ctypes twin of the gateway: both describe the same Z, G and options to the same deterministic library
through the same C ABI.  So the reference needs no tolerance: every field of `Fac` and every field of `out` except
`time_at_it` must be equal bit for bit (NaN equal to NaN).  A difference means one side marshals differently.  The
driver path itself is pinned to the oracle by the rest of the suite; cases 1 and 3 close the chain gateway -> oracle
directly with `compare` / `compare_par2` of tests/test_gpu_solver.py as they are."""
import copy
import importlib

import numpy as np
import pytest
import scipy.sparse as sps

import mex_harness as MH
from mex_harness import MexError
from helpers import (cp_model, options, par2_C_coupled_model, script1_model, script3_model, script4_model,
                     transformed_coupling_model)
from oracle import aoadmm as OA
from test_gpu_solver import compare, compare_par2

pytestmark = pytest.mark.gpu

RANK_FIELDS = ['iters', 'n', 'n_auc', 'hit', 'ndcg', 'mrr', 'auc', 'hits', 'ndcg_sum', 'mrr_sum', 'auc_sum']
NN = ('non-negativity',)


@pytest.fixture(scope='module')
def gw(tmp_path_factory, pkg):
    """The gateway + mock, linked against the library `pkg` loads; the gateway keeps its own persistent context."""
    h = MH.Harness(MH.build(tmp_path_factory.mktemp('mexgw_real'), fake=False), fake=False)
    yield h
    h.lib.mxmock_run_at_exit()


def init(Z, io, seed=7, Delta=None):
    return OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, Delta=Delta, rng=np.random.default_rng(seed))


def eq(a, b, where):
    if a is None or b is None:
        assert a is None and (b is None or (isinstance(b, (list, tuple)) and len(b) == 0)), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and set(a) <= set(b), (where, sorted(a), sorted(b))
        for k in a:
            eq(a[k], b[k], where + (k,))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            eq(x, y, where + (i,))
    elif isinstance(a, str):
        assert a == b, where
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape or a.size == b.size == 1, (where, a.shape, b.shape)
        assert np.array_equal(a.reshape(-1), b.reshape(-1), equal_nan=True), (where, float(np.max(np.abs(a.reshape(-1) - b.reshape(-1)))))


def same(Fg, og, Fd, od):
    """Gateway against driver: the same fields, the same bits (time_at_it: the same length)."""
    assert list(Fg) == list(Fd)
    for k in Fg:
        eq(Fg[k], Fd[k], ('Fac', k))
    assert set(og) == set(od) - {'heldout_sumsq', 'heldout_count'}, (sorted(og), sorted(od))
    for k in og:
        if k == 'time_at_it':
            assert len(og[k]) == len(od[k]) == og['OuterIterations'] + 1
        else:
            eq(og[k], od[k], ('out', k))
    if 'rank_trace' in og:
        assert all(list(t) == RANK_FIELDS for t in og['rank_trace'].values())


def both(gw, pkg, eng, Z, G, opt, precision='f64'):
    Fg, og, _ = gw.gateway(Z, copy.deepcopy(G), opt, precision=None if precision == 'f64' else precision)
    _, Fd, _, od = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=eng, precision=precision)
    same(Fg, og, Fd, od)
    return Fg, og, Fd, od


# ------------------------------------------------------------------------------------------------------------ cases 1 - 5
@pytest.fixture(scope='module')
def case1(pkg, eng):
    Z, io, _ = cp_model((20, 30, 40), 3, np.random.default_rng(1), [NN] * 3)
    G = init(Z, io)
    opt = options(MaxOuterIters=20)
    _, Fd, _, od = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=eng)
    return Z, G, opt, Fd, od


def run_case1(gw, case1):
    Z, G, opt, Fd, od = case1
    Fg, og, _ = gw.gateway(Z, copy.deepcopy(G), opt)
    same(Fg, og, Fd, od)
    return Fg, og


def test_cp_nonneg(gw, case1):
    """Case 1, and the chain gateway -> oracle closed directly."""
    Z, G, opt = case1[:3]
    Fg, og = run_case1(gw, case1)
    _, Fo, _, oo = OA.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G))
    compare(Fo, oo, Fg, og)
    assert og['exit_flag'] == 'maxIterations' and og['OuterIterations'] == 20 and og['innerIters'].shape == (3, 20)


def test_script3_partial_coupling(gw, pkg, eng):
    Z, io = script3_model(np.random.default_rng(3))
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=10))


def test_script4_ragged_parafac2(gw, pkg, eng):
    """Case 3 (cell-valued state), and the chain gateway -> oracle for the PARAFAC2 family."""
    Z, io = script4_model(np.random.default_rng(10), K=12)
    G = init(Z, io)
    opt = options(MaxOuterIters=12)
    Fg, og, _, _ = both(gw, pkg, eng, Z, G, opt)
    _, Fo, _, oo = OA.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G))
    compare_par2(Fo, oo, Fg, og)


def test_script1_cp_coupled_to_parafac2(gw, pkg, eng):
    Z, io = script1_model(np.random.default_rng(4), dims=(12, 10, 8), K=6, Jk=9)
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=10))


@pytest.mark.parametrize('ctype', [1, 2, 3, 5])
def test_transformed_couplings(gw, pkg, eng, ctype):
    Z, io = transformed_coupling_model(np.random.default_rng(20 + ctype), ctype)
    G = init(Z, io, Delta=[np.zeros((25, 4))] if ctype == 5 else None)
    both(gw, pkg, eng, Z, G, options(MaxOuterIters=8))


def test_parafac2_C_mode_coupled(gw, pkg, eng):
    Z, io = par2_C_coupled_model(np.random.default_rng(30), 1)
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=8))


# ------------------------------------------------------------------------------------------------------------ case 6
def _quad_L(sym):
    rng = np.random.default_rng(52)
    L = np.triu(rng.random((13, 13)), 1) * 0.6 + np.diag(1.0 + rng.random(13)) - 0.2 * np.tril(rng.random((13, 13)), -1)
    return L + L.T if sym else L


SWEEP = {
    'box': ([('box', 0.0, 0.5), NN, None], {}, {}),
    'unimodality': ([('unimodality', 1), ('unimodality', 0), NN], {}, {}),
    'tv': ([('TV regularization', 0.01), NN, NN], {}, {}),
    'quadratic-symmetric': ([('quadratic regularization', 0.05, _quad_L(True)), NN, None], {}, {}),
    'quadratic-nonsymmetric': ([('quadratic regularization', 0.05, _quad_L(False)), NN, None], {}, {}),
    'ridge': ([NN, None, NN], dict(ridge=[0.01, 0.02, 0.03]), {}),
    'bsum': ([NN, NN, NN], {}, dict(bsum=1, bsum_weight=0.5)),
}


@pytest.mark.parametrize('name', sorted(SWEEP))
def test_constraints_sweep(gw, pkg, eng, name):
    cons, zextra, oextra = SWEEP[name]
    Z, io, _ = cp_model((13, 11, 9), 3, np.random.default_rng(40), cons)
    Z.update(zextra)
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=8, **oextra))


def test_parafac2_Bk_constraint_schedule(gw, pkg, eng):
    Z, io = script4_model(np.random.default_rng(41), K=4, constraints_B=NN)
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=8, iter_start_PAR2Bkconstraint=2, increase_factor_rhoBk=1.1))


# ------------------------------------------------------------------------------------------------------------ cases 7, 8
def test_missing_entries_cp_and_parafac2(gw, pkg, eng):
    rng = np.random.default_rng(50)
    Z, io, _ = cp_model((13, 11, 9), 3, rng, [NN] * 3)
    Z['miss'] = [(rng.random((13, 11, 9)) < 0.8).astype(float)]
    _, og, _, _ = both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=8))
    assert len(og['func_rel_missing']) == 9 and np.isfinite(og['f_rel_missing']) and np.isnan(og['func_rel_missing'][0])
    Z, io = script4_model(rng, K=4)
    Z['miss'] = [[(rng.random(np.shape(Xk)) < 0.8).astype(float) for Xk in Z['object'][0]]]
    _, og, _, _ = both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=6))
    assert len(og['func_rel_missing']) == 7 and np.isfinite(og['f_rel_missing'])


def test_precisions(gw, pkg, eng, case1):
    Z, G, opt = case1[:3]
    Fg32 = both(gw, pkg, eng, Z, G, opt, precision='f32')[0]
    Fg16 = both(gw, pkg, eng, Z, G, opt, precision='f16')[0]
    assert not np.array_equal(Fg32['fac'][0], case1[3]['fac'][0]) and not np.array_equal(Fg16['fac'][0], Fg32['fac'][0])
    Z, io = script3_model(np.random.default_rng(3))                 # the 3-way block fp16, the coupled matrix fp32
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=8), precision='f16')


# ------------------------------------------------------------------------------------------------------------ case 9
def sparse_cp(pkg, seed=60, dims=(12, 10, 8), keep=0.3):
    rng = np.random.default_rng(seed)
    Z, io, _ = cp_model(dims, 3, rng, [NN] * 3)
    X = Z['object'][0]
    subs = np.argwhere(rng.random(dims) < keep)
    Z['object'] = [pkg.sptensor(subs, X[tuple(subs.T)], dims)]
    return Z, io, rng


def test_sparse_blocks(gw, pkg, eng):
    Z, io, rng = sparse_cp(pkg)
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=8))
    # a sparse matrix coupled to a dense tensor; compressed columns on both sides, so the same entry order
    Z, io = script3_model(rng, rows=20)
    X2 = Z['object'][1]
    Z['object'][1] = sps.csc_matrix(np.where(rng.random(X2.shape) < 0.3, X2, 0.0))
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=8))
    # PARAFAC2 with sparse slabs
    Z, io = script4_model(rng, K=4)
    Z['object'] = [[sps.csc_matrix(np.where(rng.random(Xk.shape) < 0.4, Xk, 0.0)) for Xk in Z['object'][0]]]
    both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=6))


@pytest.mark.parametrize('name', ['observed-1', 'observed-list', 'weights', 'weights-alpha', 'alpha-cell', 'observed-alpha'])
def test_sparse_observed_only_and_weights(gw, pkg, eng, name):
    Z, io, rng = sparse_cp(pkg)
    w = np.round(rng.random(Z['object'][0].nnz), 2)
    hip = {'observed-1': dict(sparse_observed_only=1), 'observed-list': dict(sparse_observed_only=[1]),
           'weights': dict(sparse_entry_weights=[w]), 'weights-alpha': dict(sparse_entry_weights=[w], sparse_unstored_weight=0.25),
           'alpha-cell': dict(sparse_unstored_weight=[0.5]), 'observed-alpha': dict(sparse_observed_only=1, sparse_unstored_weight=0.25)}[name]
    _, og, _, _ = both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=6, hip=hip))
    assert 'func_rel_missing' in og


# ------------------------------------------------------------------------------------------------------------ case 10
def held_list(rng, dims, n, X=None):
    subs = np.stack([rng.integers(0, d, n) for d in dims], axis=1)
    return subs, (X[tuple(subs.T)] if X is not None else rng.standard_normal(n))


def test_heldout_cp_and_parafac2(gw, pkg, eng):
    rng = np.random.default_rng(70)
    Z, io, _ = cp_model((13, 11, 9), 3, rng, [NN] * 3)
    hip = dict(heldout={1: held_list(rng, (13, 11, 9), 40, Z['object'][0])})
    _, og, _, od = both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=8, hip=hip))
    assert len(og['func_heldout'][1]) == 9 and og['heldout_best_iter'] == od['heldout_best_iter']
    Z, io = script4_model(rng, K=4)
    Jk = Z['size'][1]
    k = rng.integers(0, 4, 30)
    subs = np.stack([rng.integers(0, 40, 30), np.array([rng.integers(0, Jk[kk]) for kk in k]), k], axis=1)
    hip = dict(heldout={1: (subs, rng.standard_normal(30) * 0.01)})
    _, og, _, _ = both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=6, hip=hip))
    assert len(og['func_heldout'][1]) == 7


def test_heldout_patience_and_keep_best(gw, pkg, eng):
    """Held-out values that contradict the data: the held-out sum rises while the fit improves, so patience ends the run
    and the best iterate is an early one."""
    rng = np.random.default_rng(71)
    Z, io, _ = cp_model((13, 11, 9), 3, rng, [NN] * 3)
    subs, vals = held_list(rng, (13, 11, 9), 40, Z['object'][0])
    hip = dict(heldout={1: (subs, -5.0 * vals)}, heldout_patience=2, heldout_keep_best=1)
    _, og, _, od = both(gw, pkg, eng, Z, init(Z, io), options(MaxOuterIters=30, hip=hip))
    assert og['exit_flag'] == 'heldoutPatience' and og['OuterIterations'] < 30
    assert og['heldout_restored_iter'] == og['heldout_best_iter'] == od['heldout_restored_iter'] < og['OuterIterations']


def test_rank_lists_patience_and_criterion(gw, pkg, eng):
    Z, io, rng = sparse_cp(pkg, seed=72)
    X = Z['object'][0]
    train, held = X.split(0.2, rng)
    Z['object'] = [train]
    q = held.subs[:25]
    lists = {1: dict(mode=1, subs=q, exclude=train.fiber_lists(0, q))}
    G = init(Z, io)
    _, og, _, _ = both(gw, pkg, eng, Z, G, options(MaxOuterIters=8, hip=dict(rank_lists=lists, rank_metric='hit@5', rank_every=2)))
    assert list(og['rank_trace'][1]['iters']) == [0, 2, 4, 6, 8]
    hip = dict(rank_lists=lists, rank_metric='ndcg@5', rank_criterion=1, rank_patience=2, heldout_keep_best=1)
    _, og, _, od = both(gw, pkg, eng, Z, G, options(MaxOuterIters=40, hip=hip))
    assert og['rank_best_iter'] == od['rank_best_iter'] == og['heldout_restored_iter']
    assert og['exit_flag'] in ('rankPatience', 'maxIterations') and og['exit_flag'] == od['exit_flag']


# ------------------------------------------------------------------------------------------------------------ case 11
@pytest.mark.parametrize('tol', [dict(AbsFuncTol=5e-2), dict(OuterRelTol=5e-2)])
def test_early_stop_exit_flag_struct(gw, pkg, eng, case1, tol):
    Z, G = case1[:2]
    _, og, _, _ = both(gw, pkg, eng, Z, G, options(MaxOuterIters=50, **tol))
    assert og['OuterIterations'] < 50 and isinstance(og['exit_flag'], dict)
    assert list(og['exit_flag']) == ['f_tensors', 'f_couplings', 'f_constraints', 'f_PAR2_couplings']
    assert set(og['exit_flag'].values()) <= {'AbsFuncTol', 'RelFuncTol'}
    assert ('AbsFuncTol' in og['exit_flag'].values()) == ('AbsFuncTol' in tol)


# ------------------------------------------------------------------------------------------------------------ cases 12, 13
def display_rows(gw, pkg, engine, Z, G, opt, capsys):
    capsys.readouterr()
    _, Fd, _, od = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=engine)
    lines = capsys.readouterr().out.splitlines()
    driver_rows = lines[2:-1]                                         # without the header and the final row
    Fg, og, printed = gw.gateway(Z, copy.deepcopy(G), opt)
    same(Fg, og, Fd, od)
    assert printed.splitlines() == driver_rows and printed.endswith('\n')
    assert len(driver_rows) == od['OuterIterations'] // opt['DisplayIters'] + 1
    assert gw.evals == ['drawnow;'] * len(driver_rows)                # one flush per row
    assert set(gw.print_threads) == {gw.call_thread}                  # every mexPrintf from the calling thread


def test_display_iter_rows(gw, pkg, eng, capsys):
    rng = np.random.default_rng(80)
    Z, io, _ = cp_model((13, 11, 9), 3, rng, [NN] * 3)
    G = init(Z, io)
    opt = options(MaxOuterIters=7, Display='iter', DisplayIters=2)
    display_rows(gw, pkg, eng, Z, G, opt, capsys)
    Z['miss'] = [(rng.random((13, 11, 9)) < 0.8).astype(float)]
    display_rows(gw, pkg, eng, Z, G, opt, capsys)


def test_multi_device_context(gw, pkg, case1, capsys):
    Z, G = case1[:2]
    opt = options(MaxOuterIters=6, Display='iter', DisplayIters=2, hip=dict(devices=[0, 0]))
    with pkg.Engine([0, 0]) as e2:
        display_rows(gw, pkg, e2, Z, G, opt, capsys)
    # the context now drives two engines: it answers 'f16' with unsupported ...
    with pytest.raises(MexError) as e:
        gw.gateway(Z, copy.deepcopy(G), options(MaxOuterIters=2, hip=dict(devices=[0, 0])), precision='f16')
    assert e.value.id == 'cmtf:hip:unsupported'
    # ... and a following call with device = 0 recreates it: one engine, which stores fp16
    gw.gateway(Z, copy.deepcopy(G), options(MaxOuterIters=2, hip=dict(device=0)), precision='f16')
    run_case1(gw, case1)


# ------------------------------------------------------------------------------------------------------------ case 14
def test_unfold_gram_operation(gw):
    rng = np.random.default_rng(90)
    for dims in ((23, 17), (13, 11, 9)):
        X = rng.standard_normal(dims)
        for n in range(len(dims)):
            A = np.moveaxis(X, n, 0).reshape(dims[n], -1)
            Y, = gw.call(['unfold_gram', X, float(n + 1)])
            assert Y.shape == (dims[n], dims[n])
            assert np.linalg.norm(Y - A @ A.T) / np.linalg.norm(A @ A.T) < 1e-12
    with pytest.raises(MexError) as e:
        gw.call(['unfold_gram', rng.standard_normal((3, 4, 5, 2)), 1.0])
    assert e.value.id == 'cmtf:hip:unsupported'


def test_nvecs_operation(gw, pkg, eng):
    drv = importlib.import_module('matlab-code_amd.driver')
    Z, io, rng = sparse_cp(pkg, seed=91)
    for n in range(3):
        U, = gw.call(['nvecs', Z['object'][0], float(n + 1), 3.0])
        assert np.array_equal(U, drv.cmtf_nvecs(Z, n, 3, eng, method='iterative'))
    Zm, io = script3_model(rng, rows=20)
    M = sps.csc_matrix(np.where(rng.random(Zm['object'][1].shape) < 0.3, Zm['object'][1], 0.0))
    Z2 = dict(loss_function=['Frobenius'], model=['CP'], modes=[[1, 2]], size=list(M.shape), weights=[1.0], object=[M],
              coupling=dict(lin_coupled_modes=[0, 0], coupling_type=[], coupl_trafo_matrices=[None, None]),
              constrained_modes=[0, 0], constraints=[None, None])
    for n in range(2):
        U, = gw.call(['nvecs', M, float(n + 1), 2.0])
        assert U.shape == (M.shape[n], 2) and np.array_equal(U, drv.cmtf_nvecs(Z2, n, 2, eng, method='iterative'))
    assert gw.warns == []


# ------------------------------------------------------------------------------------------------------------ case 15
def test_real_library_errors_leave_the_gateway_usable(gw, pkg, eng, case1):
    Z, G, opt = case1[:3]
    with pytest.raises(MexError) as e:
        gw.gateway(dict(Z, constraints=[('custom', 1.0), NN, NN]), copy.deepcopy(G), opt)
    assert e.value.id == 'cmtf:hip:unsupported'
    run_case1(gw, case1)
    with pytest.raises(MexError) as e:
        gw.gateway(dict(Z, loss_function=['KL']), copy.deepcopy(G), opt)
    assert e.value.id == 'cmtf:hip:unsupported'
    run_case1(gw, case1)
    # all-zero factors: every mode's system matrix is the zero matrix, which has no Cholesky factor
    G0 = copy.deepcopy(G)
    G0['fac'] = [np.zeros_like(Fm) for Fm in G0['fac']]
    with pytest.raises(pkg.NotPositiveDefinite):
        pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G0), engine=eng)
    with pytest.raises(MexError) as e:
        gw.gateway(Z, G0, opt)
    assert e.value.id == 'cmtf:hip:notPositiveDefinite' and 'positive definite' in e.value.msg
    run_case1(gw, case1)
    # a size the model does not have never reaches the library
    with pytest.raises(MexError) as e:
        gw.gateway(dict(Z, object=[Z['object'][0][:, :, :39]]), copy.deepcopy(G), opt)
    assert e.value.id == 'cmtf:hip:invalid'
    run_case1(gw, case1)
