"""The MEX gateway (matlab-code_amd/mex/aoadmm_mex.cpp) executed on the CPU: compiled with the mock of the C Matrix API
(tests/mxmock/mxmock.cpp) and the recording fake of the C ABI (tests/mxmock/fake_aoadmm.cpp).  The fake logs every
call with copies of its arguments, so what the gateway marshals -- shifts from 1-based to 0-based, layouts, packing,
lengths, the fields of `Fac` and `out`, every error id -- is asserted exactly.  No GPU, no library, no MATLAB."""
import importlib
import itertools
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

import mex_harness as MH
from mex_harness import MexError, MockMisuse, Raw, TensorObject
from helpers import cp_model, options, script3_model, transformed_coupling_model
from oracle import aoadmm as OA

sptensor = importlib.import_module('matlab-code_amd.sptensor').sptensor

F_FAC, F_CFAC, F_CDUAL, F_COUPFAC, F_COUPDUAL, F_DELTAB, F_P, F_MU = range(8)
ALL_SLABS = -1
BASE_OUT = {'f_tensors', 'f_couplings', 'f_constraints', 'f_PAR2_couplings', 'f_rel_missing', 'exit_flag', 'OuterIterations',
            'func_val_conv', 'func_coupl_conv', 'func_constr_conv', 'func_PAR2_coupl', 'time_at_it', 'innerIters'}
RANK_FIELDS = ['iters', 'n', 'n_auc', 'hit', 'ndcg', 'mrr', 'auc', 'hits', 'ndcg_sum', 'mrr_sum', 'auc_sum']


@pytest.fixture(scope='module')
def so(tmp_path_factory):
    return MH.build(tmp_path_factory.mktemp('mexgw_fake'), fake=True)


@pytest.fixture(scope='module')
def h(so):
    return MH.Harness(so, fake=True)


@pytest.fixture
def fresh(so, tmp_path):
    """A second copy of the shared object: its own statics, so the gateway's persistent context starts from nothing."""
    return MH.Harness(shutil.copy(so, str(tmp_path / 'mexgw_fresh.so')), fake=True)


def init(Z, io, seed=3, Delta=None):
    return OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, Delta=Delta, rng=np.random.default_rng(seed))


def cp3(cons=(('non-negativity',), ('box', 0.0, 2.0), None), seed=0):
    """One CP block 4 x 3 x 2, R = 2."""
    Z, io, _ = cp_model((4, 3, 2), 2, np.random.default_rng(seed), list(cons))
    return Z, init(Z, io)


def mat2(obj=None):
    """One CP block 5 x 4, R = 2 (a matrix), `obj` in place of the dense data."""
    Z, io, _ = cp_model((5, 4), 2, np.random.default_rng(1), [None, ('non-negativity',)])
    if obj is not None:
        Z['object'] = [obj]
    return Z, init(Z, io)


def par2(slabs=None, cons_B=None):
    """One PARAFAC2 block: I = 3, J_k = (2, 3), K = 2, R = 2."""
    rng = np.random.default_rng(2)
    X = [rng.standard_normal((3, 2)), rng.standard_normal((3, 3))] if slabs is None else slabs
    Z = dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=[3, [2, 3], 2],
             coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
             constrained_modes=[0, 1 if cons_B else 0, 1], constraints=[None, cons_B, ('non-negativity',)], weights=[0.75], object=[X])
    io = dict(lambdas_init=[[1, 1]], nvecs=0, distr=[lambda a, b: rng.standard_normal((a, b))] * 2 + [lambda a, b: rng.random((a, b))],
              normalize=1)
    return Z, init(Z, io)


def sp3():
    """The CP block of cp3 as an sptensor with 5 stored entries, given out of order."""
    Z, G = cp3()
    subs = np.array([[3, 2, 1], [0, 0, 0], [2, 1, 0], [1, 2, 1], [0, 1, 1]])
    X = sptensor(subs, np.array([1.5, -2.0, 3.0, 0.25, 4.0]), (4, 3, 2))
    Z['object'] = [X]
    return Z, G, X


def F(a):
    return list(np.asarray(a, dtype=np.float64).ravel(order='F'))


def one(h, fn, log):
    c = h.calls(fn, log)
    assert len(c) == 1, (fn, len(c))
    return c[0]


def run(h, Z, G, opt=None, **kw):
    h.log()
    Fac, out, printed = h.gateway(Z, G, options(**(opt or {})), **kw)
    return Fac, out, printed, h.log()


# ---------------------------------------------------------------------------------------------------------------- marshalling
def test_sptensor_subs_arrive_zero_based_int64_column_major(h):
    Z, G, X = sp3()
    log = run(h, Z, G)[3]
    c = one(h, 'aoadmm_tensor_upload_coo', log)
    assert c['p'] == 0 and c['nnz'] == 5
    assert c['subs'] == [int(v) for v in X.subs.ravel(order='F')]       # nnz x N, column-major, 0-based
    assert c['subs'] == [0, 2, 0, 1, 3, 0, 1, 1, 2, 2, 0, 0, 1, 1, 1]
    assert c['vals'] == list(X.vals) == [-2.0, 3.0, 4.0, 0.25, 1.5]
    assert not h.calls('aoadmm_tensor_upload', log) and not h.calls('aoadmm_tensor_set_observed_only', log)


def test_csc_matrix_with_empty_columns_and_without_entries(h):
    M = np.zeros((5, 4))
    M[3, 0], M[1, 0], M[4, 2] = 1.5, -2.0, 3.0
    Z, G = mat2(sps.csc_matrix(M))
    c = one(h, 'aoadmm_tensor_upload_coo', run(h, Z, G)[3])
    assert (c['nnz'], c['subs'], c['vals']) == (3, [1, 3, 4, 0, 0, 2], [-2.0, 1.5, 3.0])
    Z, G = mat2(sps.csc_matrix((5, 4)))
    c = one(h, 'aoadmm_tensor_upload_coo', run(h, Z, G)[3])
    assert c['nnz'] == 0 and not c['subs'] and not c['vals']          # nothing to read: the library takes null for nnz = 0


def test_sparse_par2_slabs_arrive_as_ijk_in_slab_order(h):
    X0 = sps.csc_matrix(([1.0, 2.0], ([2, 0], [0, 1])), shape=(3, 2))
    X1 = sps.csc_matrix(([3.0, 4.0], ([1, 1], [2, 0])), shape=(3, 3))
    Z, G = par2([X0, X1])
    log = run(h, Z, G)[3]
    c = one(h, 'aoadmm_par2_slab_upload_coo', log)
    assert (c['p'], c['nnz']) == (0, 4)
    assert c['subs'] == [2, 0, 1, 1, 0, 1, 0, 2, 0, 0, 1, 1]
    assert c['vals'] == [1.0, 2.0, 4.0, 3.0]
    assert not h.calls('aoadmm_par2_slab_upload', log)


def test_dense_slabs_and_cell_state_arrive_back_to_back(h):
    Z, G = par2(cons_B=('non-negativity',))
    log = run(h, Z, G)[3]
    assert one(h, 'aoadmm_model_set_mode_slabs', log) == dict(fn='aoadmm_model_set_mode_slabs', mode=1, K=2, rows_k=[2, 3], rank=2)
    assert one(h, 'aoadmm_model_add_par2', log) == dict(fn='aoadmm_model_add_par2', p=0, modes=[0, 1, 2], weight=0.75)
    c = one(h, 'aoadmm_par2_slab_upload', log)
    assert c['k'] == ALL_SLABS and c['data'] == F(Z['object'][0][0]) + F(Z['object'][0][1])
    sets = {(c['field'], c['index']): c for c in h.calls('aoadmm_state_set', log)}
    for field, index, cells in ((F_FAC, 1, G['fac'][1]), (F_CFAC, 1, G['constraint_fac'][1]), (F_CDUAL, 1, G['constraint_dual_fac'][1]),
                                (F_P, 0, G['P'][0]), (F_MU, 0, G['mu_DeltaB'][0])):
        c = sets[(field, index)]
        assert (c['slab'], c['rows'], c['cols']) == (ALL_SLABS, 5, 2)         # the summed row count
        assert c['host'] == F(cells[0]) + F(cells[1])
    c = sets[(F_DELTAB, 0)]
    assert (c['slab'], c['rows'], c['cols'], c['host']) == (0, 2, 2, F(G['DeltaB'][0]))
    assert sets[(F_FAC, 0)]['host'] == F(G['fac'][0]) and sets[(F_FAC, 0)]['slab'] == 0


def test_modes_and_couplings_arrive_shifted_by_one(h):
    Z, io = script3_model(np.random.default_rng(4), rows=5, R=3)
    G = init(Z, io)
    log = run(h, Z, G)[3]
    assert one(h, 'aoadmm_model_begin', log)['n_couplings'] == 1
    assert [c['modes'] for c in h.calls('aoadmm_model_add_cp', log)] == [[0, 1, 2], [3, 4]]
    assert [c['weight'] for c in h.calls('aoadmm_model_add_cp', log)] == [0.5, 0.5]
    cs = h.calls('aoadmm_model_set_coupling', log)
    assert [c['mode'] for c in cs] == [0, 1, 2, 3, 4]
    assert [c['coupling'] for c in cs] == [0, -1, -1, 0, -1]
    H = Z['coupling']['coupl_trafo_matrices']
    assert (cs[0]['H'], cs[0]['hr'], cs[0]['hc']) == (F(H[0]), 3, 3)
    assert (cs[3]['H'], cs[3]['hr'], cs[3]['hc']) == (F(H[3]), 3, 2)              # not square: rows and columns in order
    assert all(c['H'] is None and c['hr'] == 0 for c in (cs[1], cs[2], cs[4]))
    assert all(c['H2'] is None and c['h2r'] == 0 and c['h2c'] == 0 for c in cs)   # coupl_trafo_matrices2 absent
    assert one(h, 'aoadmm_model_set_coupling_type', log) == dict(fn='aoadmm_model_set_coupling_type', coupling=0, type=4)
    c = [c for c in h.calls('aoadmm_state_set', log) if c['field'] == F_COUPFAC]
    assert len(c) == 1 and c[0]['index'] == 0 and c[0]['host'] == F(G['coupling_fac'][0])
    assert sorted(c['index'] for c in h.calls('aoadmm_state_set', log) if c['field'] == F_COUPDUAL) == [0, 3]


def test_second_trafo_matrices_arrive_when_present(h):
    Z, io = transformed_coupling_model(np.random.default_rng(5), 5)
    log = run(h, Z, init(Z, io, Delta=[np.zeros((25, 4))]))[3]
    cs = h.calls('aoadmm_model_set_coupling', log)
    H2 = Z['coupling']['coupl_trafo_matrices2']
    assert (cs[0]['H2'], cs[0]['h2r'], cs[0]['h2c']) == (F(H2[0]), 4, 4)
    assert (cs[3]['H2'], cs[3]['h2r'], cs[3]['h2c']) == (F(H2[3]), 4, 3)
    assert cs[1]['H2'] is None and cs[3]['H'] == F(Z['coupling']['coupl_trafo_matrices'][3]) and (cs[3]['hr'], cs[3]['hc']) == (25, 50)


def test_constraint_parameters_in_order_and_L_as_Lmat(h):
    L = np.arange(16.0).reshape(4, 4) + np.eye(4)
    Z, G = cp3(cons=(('quadratic regularization', 0.05, L), ('box', -1.0, 2.5), ('unimodality', 1)))
    Z['ridge'] = [0.1, 0.2, 0.3]
    log = run(h, Z, G)[3]
    cs = h.calls('aoadmm_model_set_constraint', log)
    assert [(c['mode'], c['constraint'], c['params'], c['n_params']) for c in cs] == [(0, 17, [0.05], 1), (1, 2, [-1.0, 2.5], 2), (2, 7, [1.0], 1)]
    assert cs[0]['Lmat'] == F(L) and cs[1]['Lmat'] is None and cs[2]['Lmat'] is None
    assert one(h, 'aoadmm_model_set_ridge', log)['ridge'] == [0.1, 0.2, 0.3]


def test_heldout_and_rank_lists_arrive_shifted_offsets_do_not(h):
    Z, G = cp3()
    hs = np.array([[3, 2, 1], [0, 0, 0], [1, 1, 0]])
    rs = np.array([[0, 2, 1], [3, 0, 0]])
    hip = dict(heldout={1: (hs, [0.5, -1.0, 2.0])}, heldout_patience=2,
               rank_lists={1: dict(mode=2, subs=rs, exclude=([0, 2, 3], [1, 0, 2]))}, rank_metric='hit@5', rank_every=3)
    log = run(h, Z, G, dict(hip=hip))[3]
    c = one(h, 'aoadmm_tensor_set_heldout', log)
    assert (c['p'], c['n'], c['subs'], c['vals']) == (0, 3, [int(v) for v in hs.ravel(order='F')], [0.5, -1.0, 2.0])
    c = one(h, 'aoadmm_tensor_set_ranklist', log)
    assert (c['p'], c['mode'], c['nq'], c['subs']) == (0, 1, 2, [int(v) for v in rs.ravel(order='F')])
    assert c['excl_off'] == [0, 2, 3] and c['excl_idx'] == [1, 0, 2]
    assert one(h, 'aoadmm_rank_track', log) == dict(fn='aoadmm_rank_track', metric=0, k=5, every=3, patience=0, criterion=0)
    assert one(h, 'aoadmm_solve', log)['heldout_patience'] == 2
    # the order the library needs: lists after the data, the state after the lists
    names = [c['fn'] for c in log]
    assert names.index('aoadmm_tensor_upload') < names.index('aoadmm_tensor_set_heldout') < names.index('aoadmm_tensor_set_ranklist') \
        < names.index('aoadmm_rank_track') < names.index('aoadmm_state_set') < names.index('aoadmm_solve')


def test_empty_exclusion_list_still_gets_an_address(h):
    Z, G = cp3()
    hip = dict(rank_lists={1: dict(mode=1, subs=np.array([[0, 2, 1], [3, 0, 0]]), exclude=([0, 0, 0], []))})
    c = one(h, 'aoadmm_tensor_set_ranklist', run(h, Z, G, dict(hip=hip))[3])
    assert c['excl_off'] == [0, 0, 0] and c['excl_idx'] == [] and c['excl_idx_set'] == 1
    hip = dict(rank_lists={1: dict(mode=1, subs=np.array([[0, 2, 1]]))})             # no exclusion lists at all: null
    c = one(h, 'aoadmm_tensor_set_ranklist', run(h, Z, G, dict(hip=hip))[3])
    assert c['excl_off'] is None and c['excl_idx'] is None and c['excl_idx_set'] == 0 and c['mode'] == 0


@pytest.mark.parametrize('spec,metric,k', [('ndcg@10', 1, 10), ('hit@5', 0, 5), ('mrr', 2, 10), ('auc', 3, 10), ('ndcg', 1, 10),
                                           ('hit@2147483647', 0, 2147483647)])
def test_rank_metric_parses(h, spec, metric, k):
    Z, G = cp3()
    c = one(h, 'aoadmm_rank_track', run(h, Z, G, dict(hip=dict(rank_metric=spec, rank_patience=0, rank_criterion=0)))[3])
    assert (c['metric'], c['k'], c['every'], c['patience'], c['criterion']) == (metric, k, 1, 0, 0)


@pytest.mark.parametrize('spec', ['mrr@3', 'hit@0', 'foo', 'auc@1', 'hit@', 'ndcg@1.5', 'hit@2147483648', 'hit@-1'])
def test_rank_metric_refused(h, spec):
    Z, G = cp3()
    with pytest.raises(MexError) as e:
        run(h, Z, G, dict(hip=dict(rank_metric=spec)))
    assert e.value.id == 'cmtf:hip:invalid' and ("'%s'" % spec) in e.value.msg


def test_f16_rule(h):
    Z, G = cp3()
    upload = lambda Z, G, prec: one(h, 'aoadmm_tensor_upload', run(h, Z, G, precision=prec)[3])['precision']
    assert upload(Z, G, None) == 0 and upload(Z, G, 'f64') == 0 and upload(Z, G, 'f32') == 1
    assert upload(Z, G, 'f16') == 2                                             # 3-way, no mask
    Zm = dict(Z, miss=[np.ones((4, 3, 2))])
    assert upload(Zm, G, 'f16') == 1                                            # a mask: fp32
    assert upload(dict(Z, miss=[None]), G, 'f16') == 2                          # an empty Z.miss cell is no mask
    Z2, G2 = mat2()
    assert upload(Z2, G2, 'f16') == 1 and upload(Z2, G2, 'f32') == 1            # a matrix: fp32
    Z3, io = script3_model(np.random.default_rng(4), rows=5, R=3)
    log = run(h, Z3, init(Z3, io), precision='f16')[3]
    assert [c['precision'] for c in h.calls('aoadmm_tensor_upload', log)] == [2, 1]


def test_masks_arrive_as_bytes_one_is_observed(h):
    Z, G = cp3()
    mk = (np.random.default_rng(6).random((4, 3, 2)) > 0.3)
    out, log = run(h, dict(Z, miss=[mk.astype(float)]), G)[1::2]
    assert one(h, 'aoadmm_tensor_mask_upload', log)['mask'] == [int(v) for v in mk.ravel(order='F')]
    assert set(out) == BASE_OUT | {'func_rel_missing'} and out['f_rel_missing'] == 0.125
    Z, G = par2()
    mks = [np.array([[1, 0], [0, 1], [1, 1]]), np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1]])]
    log = run(h, dict(Z, miss=[mks]), G)[3]
    cs = h.calls('aoadmm_par2_slab_mask_upload', log)
    assert [(c['p'], c['k'], c['mask']) for c in cs] == [(0, 0, [1, 0, 1, 0, 1, 1]), (0, 1, [1, 0, 1, 1, 1, 0, 0, 1, 1])]


def test_tensor_object_data_goes_up(h):
    Z, G = cp3()
    X = Z['object'][0]
    Zt = dict(Z, object=[TensorObject(X)])
    assert one(h, 'aoadmm_tensor_upload', run(h, Zt, G)[3])['data'] == F(X)


def test_entry_weights_unstored_weight_and_observed_only(h):
    Z, G, X = sp3()
    subs = [int(v) for v in X.subs.ravel(order='F')]
    w = [0.5, 1.0, 0.25, 0.0, 0.75]
    calls = lambda hip: [(c['fn'], c) for c in run(h, Z, G, dict(hip=hip))[3]
                         if c['fn'] in ('aoadmm_tensor_set_entry_weights', 'aoadmm_tensor_set_observed_only')]
    # weights with the scalar alpha
    (f1, c1), (f2, c2) = calls(dict(sparse_entry_weights=[w], sparse_unstored_weight=0.125))
    assert f1 == 'aoadmm_tensor_set_entry_weights' and (c1['p'], c1['nnz'], c1['subs'], c1['wts'], c1['unstored_weight']) == (0, 5, subs, w, 0.125)
    assert f2 == 'aoadmm_tensor_set_observed_only' and (c2['p'], c2['on']) == (0, 1)
    # weights alone: alpha 0
    (f1, c1), _ = calls(dict(sparse_entry_weights=[w]))
    assert c1['unstored_weight'] == 0.0 and c1['wts'] == w
    # the cell form of alpha, no weights: alpha alone, no subscripts
    (f1, c1), _ = calls(dict(sparse_unstored_weight=[0.5]))
    assert (c1['nnz'], c1['subs'], c1['wts'], c1['unstored_weight']) == (0, None, None, 0.5)
    # a scalar alpha names no block by itself ...
    assert calls(dict(sparse_unstored_weight=0.5)) == []
    # ... but is the alpha of a block sparse_observed_only marks
    (f1, c1), (f2, c2) = calls(dict(sparse_unstored_weight=0.5, sparse_observed_only=1))
    assert (c1['nnz'], c1['wts'], c1['unstored_weight']) == (0, None, 0.5) and c2['on'] == 1
    # observed-only as 0, as 1 and as a list of 1-based block numbers
    assert calls(dict(sparse_observed_only=0)) == []
    for v in (1, [1]):
        got = calls(dict(sparse_observed_only=v))
        assert [(f, c['p'], c['on']) for f, c in got] == [('aoadmm_tensor_set_observed_only', 0, 1)]
    out = run(h, Z, G, dict(hip=dict(sparse_observed_only=1)))[1]
    assert 'func_rel_missing' in out                                           # the block has missing entries
    # sharded upload
    log = run(h, Z, G, dict(hip=dict(sparse_sharding=1)))[3]
    assert one(h, 'aoadmm_tensor_upload_coo_sharded', log)['subs'] == subs and not h.calls('aoadmm_tensor_upload_coo', log)


def test_options_arrive(h):
    Z, G = par2()
    opt = dict(MaxOuterIters=7, MaxInnerIters=9, AbsFuncTol=1e-3, OuterRelTol=2e-4, innerRelPrTol_coupl=1e-2, innerRelPrTol_constr=2e-2,
               innerRelDualTol_coupl=3e-2, innerRelDualTol_constr=4e-2, bsum=1, bsum_weight=0.5, iter_start_PAR2Bkconstraint=3,
               increase_factor_rhoBk=1.5, hip=dict(no_permuted_copy=1, par2_slab_sharding=-1))
    c = one(h, 'aoadmm_solve', run(h, Z, G, opt)[3])
    want = dict(opt, has_increase_factor_rhoBk=1, use_dimtree=1, no_permuted_copy=1, par2_slab_sharding=-1, heldout_patience=0,
                reserved=[0, 0, 0, 0], fn='aoadmm_solve')
    del want['hip']
    assert c == want
    c = one(h, 'aoadmm_solve', run(h, Z, G)[3])
    assert (c['has_increase_factor_rhoBk'], c['increase_factor_rhoBk'], c['bsum'], c['bsum_weight']) == (0, 0.0, 0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- outputs
def pattern(field, index, shape, offset=0):
    n = shape[0] * shape[1]
    return (1e6 * field + 1e3 * index + offset + np.arange(n, dtype=np.float64)).reshape(shape, order='F')


def test_Fac_has_the_fields_of_G_filled_from_the_state(h):
    Z, G = par2(cons_B=('non-negativity',))
    Fac, out, _, log = run(h, Z, G)
    assert list(Fac) == list(G)
    assert np.array_equal(Fac['fac'][0], pattern(F_FAC, 0, (3, 2))) and np.array_equal(Fac['fac'][2], pattern(F_FAC, 2, (2, 2)))
    for key, field, index in (('fac', F_FAC, 1), ('constraint_fac', F_CFAC, 1), ('constraint_dual_fac', F_CDUAL, 1)):
        cells = Fac[key][1]
        assert [c.shape for c in cells] == [(2, 2), (3, 2)]
        assert np.array_equal(cells[0], pattern(field, index, (2, 2))) and np.array_equal(cells[1], pattern(field, index, (3, 2), 4))
    for key, field in (('P', F_P), ('mu_DeltaB', F_MU)):
        cells = Fac[key][0]
        assert np.array_equal(cells[0], pattern(field, 0, (2, 2))) and np.array_equal(cells[1], pattern(field, 0, (3, 2), 4))
    assert np.array_equal(Fac['DeltaB'][0], pattern(F_DELTAB, 0, (2, 2)))
    assert Fac['constraint_fac'][0] is None and Fac['coupling_dual_fac'] == [None] * 3 and Fac['coupling_fac'] == []
    gets = [(c['field'], c['index'], c['slab'], c['rows'], c['cols']) for c in h.calls('aoadmm_state_get', log)]
    assert (F_FAC, 1, ALL_SLABS, 5, 2) in gets and (F_P, 0, ALL_SLABS, 5, 2) in gets and (F_FAC, 0, 0, 3, 2) in gets
    # a coupled model: coupling_fac and the coupling duals
    Z, io = script3_model(np.random.default_rng(4), rows=5, R=3)
    G = init(Z, io)
    Fac = run(h, Z, G)[0]
    assert list(Fac) == list(G)
    assert np.array_equal(Fac['coupling_fac'][0], pattern(F_COUPFAC, 0, G['coupling_fac'][0].shape))
    assert np.array_equal(Fac['coupling_dual_fac'][3], pattern(F_COUPDUAL, 3, G['coupling_dual_fac'][3].shape))
    assert Fac['coupling_dual_fac'][1] is None and Fac['fac'][4].shape == (70, 2)


def test_out_traces_inner_iterations_and_field_sets(h):
    Z, G = cp3()
    out = run(h, Z, G, dict(MaxOuterIters=5))[1]
    assert set(out) == BASE_OUT
    assert out['OuterIterations'] == 3 and out['exit_flag'] == 'maxIterations' and np.isnan(out['f_rel_missing'])
    assert (out['f_tensors'], out['f_couplings'], out['f_constraints'], out['f_PAR2_couplings']) == (1.5, 2.5, 3.5, 4.5)
    for t, k in enumerate(('func_val_conv', 'func_coupl_conv', 'func_constr_conv', 'func_PAR2_coupl', 'time_at_it')):
        assert list(out[k]) == [100.0 * (t + 1) + i for i in range(4)]                # OuterIterations + 1 entries
    assert out['innerIters'].shape == (3, 3)
    assert np.array_equal(out['innerIters'], [[10.0 * m + i + 1 for i in range(3)] for m in range(3)])
    out = run(h, Z, G, dict(MaxOuterIters=2))[1]
    assert out['OuterIterations'] == 2 and out['innerIters'].shape == (3, 2) and len(out['func_val_conv']) == 3
    out = run(h, Z, G, dict(MaxOuterIters=0))[1]                                      # MaxOuterIters = 0 works
    assert out['OuterIterations'] == 0 and out['innerIters'].shape == (3, 1) and list(out['func_val_conv']) == [100.0]
    assert np.array_equal(out['innerIters'], [[1.0], [11.0], [21.0]])
    assert run(h, Z, G, nlhs=1)[1] is None and run(h, Z, G, nlhs=0)[0] is not None


def test_out_fields_with_heldout_keep_best_and_rank(h):
    Z, G = cp3()
    held = {1: (np.array([[3, 2, 1], [0, 0, 0]]), [0.5, -1.0])}
    ranks = {1: dict(mode=1, subs=np.array([[0, 2, 1]]))}
    out = run(h, Z, G, dict(hip=dict(heldout=held)))[1]
    assert set(out) == BASE_OUT | {'func_heldout', 'heldout_best_iter'}
    assert list(out['func_heldout'][1]) == [700.0, 701.0, 702.0, 703.0] and out['heldout_best_iter'] == 1
    out, log = run(h, Z, G, dict(hip=dict(heldout=held, heldout_keep_best=1)))[1::2]
    assert set(out) == BASE_OUT | {'func_heldout', 'heldout_best_iter', 'heldout_restored_iter'} and out['heldout_restored_iter'] == 1
    names = [c['fn'] for c in log]
    assert one(h, 'aoadmm_heldout_keep_best', log)['on'] == 1
    assert names.index('aoadmm_heldout_keep_best') < names.index('aoadmm_solve') < names.index('aoadmm_heldout_restore_best') \
        < names.index('aoadmm_state_get')                                             # Fac is read after the best iterate is back
    out = run(h, Z, G, dict(hip=dict(heldout=held, heldout_keep_best=0)))[1]
    assert 'heldout_restored_iter' not in out
    out = run(h, Z, G, dict(hip=dict(rank_lists=ranks)))[1]
    assert set(out) == BASE_OUT | {'rank_trace', 'rank_best_iter'} and out['rank_best_iter'] == 2
    tr = out['rank_trace'][1]
    assert list(tr) == RANK_FIELDS
    e = np.arange(4.0)
    assert list(tr['iters']) == [0, 2, 4, 6] and list(tr['n']) == list(100 + e) and list(tr['n_auc']) == [0.0, 201.0, 202.0, 203.0]
    for name, what in (('hits', 2), ('ndcg_sum', 3), ('mrr_sum', 4), ('auc_sum', 5)):
        assert list(tr[name]) == list(100.0 * (what + 1) + e)
    for name, what in (('hit', 2), ('ndcg', 3), ('mrr', 4)):
        assert np.array_equal(tr[name], (100.0 * (what + 1) + e) / (100 + e))
    assert np.isnan(tr['auc'][0]) and np.array_equal(tr['auc'][1:], (600 + e[1:]) / (200 + e[1:]))   # a mean over nothing is NaN
    # rank_criterion = 1 with keep-best: the ranking list serves, no held-out list needed
    out = run(h, Z, G, dict(hip=dict(rank_lists=ranks, rank_criterion=1, rank_patience=2, heldout_keep_best=1, rank_metric='mrr')))[1]
    assert set(out) == BASE_OUT | {'rank_trace', 'rank_best_iter', 'heldout_restored_iter'}
    out = run(h, dict(Z, miss=[np.ones((4, 3, 2))]), G, dict(hip=dict(heldout=held, rank_lists=ranks)))[1]
    assert set(out) == BASE_OUT | {'func_rel_missing', 'func_heldout', 'heldout_best_iter', 'rank_trace', 'rank_best_iter'}
    assert np.isnan(out['func_rel_missing'][0]) and list(out['func_rel_missing'][1:]) == [601.0, 602.0, 603.0]


@pytest.mark.parametrize('missing,heldout,keep,rank', [c for c in itertools.product((0, 1), repeat=4) if c[1] or not c[2]])
def test_out_field_set_in_every_combination(h, missing, heldout, keep, rank):
    Z, G = cp3()
    if missing:
        Z['miss'] = [np.ones((4, 3, 2))]
    hip = {}
    if heldout:
        hip['heldout'] = {1: (np.array([[3, 2, 1], [0, 0, 0]]), [0.5, -1.0])}
    if keep:
        hip['heldout_keep_best'] = 1
    if rank:
        hip['rank_lists'] = {1: dict(mode=3, subs=np.array([[0, 2, 1]]))}
    out = run(h, Z, G, dict(hip=hip))[1]
    want = set(BASE_OUT)
    want |= {'func_rel_missing'} if missing else set()
    want |= {'func_heldout', 'heldout_best_iter'} if heldout else set()
    want |= {'heldout_restored_iter'} if keep else set()
    want |= {'rank_trace', 'rank_best_iter'} if rank else set()
    assert set(out) == want
    assert np.isnan(out['f_rel_missing']) == (not missing)


def test_exit_flag(h):
    Z, G = cp3()
    try:
        for code, want in ((0, 'maxIterations'), (2, 'heldoutPatience'), (3, 'rankPatience')):
            h.lib.fake_script_solve(code, None, 3)
            assert run(h, Z, G)[1]['exit_flag'] == want
        h.lib.fake_script_solve(1, (MH.C.c_int * 4)(1, 0, 0, 1), 3)
        assert run(h, Z, G)[1]['exit_flag'] == dict(f_tensors='AbsFuncTol', f_couplings='RelFuncTol', f_constraints='RelFuncTol',
                                                    f_PAR2_couplings='AbsFuncTol')
    finally:
        h.lib.fake_script_solve(0, None, 3)


def test_display_rows(h):
    Z, G = cp3()
    _, _, printed, log = run(h, Z, G, dict(Display='iter', DisplayIters=2, MaxOuterIters=5))
    sets = h.calls('aoadmm_set_progress', log)
    assert [(c['set'], c['every']) for c in sets] == [(1, 2), (0, 0)]
    assert printed == '     0     1.875000     1.000000     0.250000          0.500000     0.125000\n' \
                      '     2     3.875000     3.000000     0.250000          0.500000     0.125000\n'
    assert h.evals == ['drawnow;'] * 2 and set(h.print_threads) == {h.call_thread}
    _, _, printed, _ = run(h, dict(Z, miss=[np.ones((4, 3, 2))]), G, dict(Display='iter', DisplayIters=3))
    assert printed.splitlines()[1] == '     3     4.875000     4.000000     0.250000          0.500000     0.125000     0.187500'
    _, _, printed, log = run(h, Z, G, dict(Display='final'))
    assert printed == '' and not h.calls('aoadmm_set_progress', log)
    # a solve that fails still takes the callback back before the error leaves
    h.lib.fake_fail(b'aoadmm_solve', 3)
    with pytest.raises(MexError) as e:
        run(h, Z, G, dict(Display='iter'))
    assert e.value.id == 'cmtf:hip:notPositiveDefinite'
    assert [(c['set'], c['every']) for c in h.calls('aoadmm_set_progress', h.log())] == [(1, 10), (0, 0)]


def test_unfold_gram_and_nvecs_operations(h):
    h.log()
    X = np.arange(24.0).reshape((4, 3, 2), order='F')
    for n in (1, 2, 3):
        Y, = h.call(['unfold_gram', X, float(n)])
        c = one(h, 'aoadmm_op_unfold_gram', h.log())
        assert (c['X'], c['ndims'], c['dims'], c['n'], c['precision']) == (F(X), 3, [4, 3, 2], n - 1, 0)
        assert Y.shape == (X.shape[n - 1],) * 2 and Y[1, 0] == 5e6 + 1
    Y, = h.call(['unfold_gram', X[:, :, 0], 2.0])
    assert one(h, 'aoadmm_op_unfold_gram', h.log())['dims'] == [4, 3] and Y.shape == (3, 3)
    _, _, Xs = sp3()
    U, = h.call(['nvecs', Xs, 2.0, 2.0])
    log = h.log()
    assert [c['fn'] for c in log] == ['aoadmm_model_begin'] + ['aoadmm_model_set_mode'] * 3 + ['aoadmm_model_add_cp'] + \
        ['aoadmm_model_set_coupling'] * 3 + ['aoadmm_model_end', 'aoadmm_tensor_upload_coo', 'aoadmm_resident_nvecs']
    assert [(c['rows'], c['rank']) for c in h.calls('aoadmm_model_set_mode', log)] == [(4, 2), (3, 2), (2, 2)]
    assert one(h, 'aoadmm_tensor_upload_coo', log)['subs'] == [int(v) for v in Xs.subs.ravel(order='F')]
    c = one(h, 'aoadmm_resident_nvecs', log)
    assert (c['p'], c['tensor_mode'], c['r'], c['ldU'], c['opt_set']) == (0, 1, 2, 3, 0)
    assert U.shape == (3, 2) and U[2, 1] == 6e6 + 5 and h.warns == []
    M = sps.csc_matrix(([1.0, 2.0], ([4, 0], [0, 3])), shape=(5, 4))
    U, = h.call(['nvecs', M, 1.0, 1.0])
    log = h.log()
    assert one(h, 'aoadmm_tensor_upload_coo', log)['subs'] == [4, 0, 0, 3] and U.shape == (5, 1)
    h.lib.fake_script_nvecs(0)
    try:
        h.call(['nvecs', M, 2.0, 1.0])
    finally:
        h.lib.fake_script_nvecs(1)
    assert h.warns == [('cmtf:hip:nvecs', 'nvecs of mode 2: subspace iteration stopped after 7 iterations with residual 5.000e-01')]
    h.log()


# ---------------------------------------------------------------------------------------------------------------- errors
def _sp_obj(**props):
    """An sptensor object with the given properties replaced (a value None: the property is left out)."""
    def make(hh):
        base = dict(subs=Raw(lambda q: q.double(np.array([[1.0, 1, 1], [2, 2, 2]]), (2, 3))), vals=Raw(lambda q: q.double([1.0, 2.0], (2, 1))),
                    size=np.array([4.0, 3, 2]))
        base.update(props)
        return hh.obj('sptensor', {k: v for k, v in base.items() if v is not None})
    return Raw(make)


DROP = object()


def _with(base, **kw):
    """(Z, G, opt) of `base()` with Z fields (z_*), option fields (o_*) and options.hip fields (h_*) replaced."""
    def make():
        Z, G = base()[:2]
        opt = {}
        for k, v in kw.items():
            if k.startswith('z_') and v is DROP:
                del Z[k[2:]]
            elif k.startswith('z_'):
                Z[k[2:]] = v
            elif k.startswith('o_'):
                opt[k[2:]] = v
            elif k.startswith('h_'):
                opt.setdefault('hip', {})[k[2:]] = v
        return Z, G, opt
    return make


_X0 = sps.csc_matrix(([1.0], ([2], [0])), shape=(3, 2))
_X1 = sps.csc_matrix(([3.0], ([1], [2])), shape=(3, 3))
_RL = dict(mode=1, subs=np.array([[0, 2, 1], [3, 0, 0]]))
_HELD = {1: (np.array([[3, 2, 1]]), [0.5])}
sp3m = lambda: sp3()[:2]
par2_sparse = lambda: par2([_X0, _X1])

# name -> (inputs, id, the whole message or None where the text is the library's)
ERRORS = {
    'missing-field-Z': (_with(cp3, z_size=DROP), 'cmtf:hip:missingField', None),
    'no-constraint': (_with(cp3, z_constraints=[None, ('box', 0.0, 1.0), None]), 'cmtf:hip:invalid', 'No constraint provided for mode 1.'),
    'custom-constraint': (_with(cp3, z_constraints=[('custom', 1.0), ('box', 0.0, 1.0), None]), 'cmtf:hip:unsupported',
                          "'custom' prox handles cannot cross to the device (constraints_to_prox.m:86-90)"),
    'unknown-constraint': (_with(cp3, z_constraints=[('nonneg',), ('box', 0.0, 1.0), None]), 'cmtf:hip:invalid', "unknown constraint 'nonneg'"),
    'loss': (_with(cp3, z_loss_function=['KL']), 'cmtf:hip:unsupported', 'non-Frobenius losses need the L-BFGS-B path of the MATLAB code'),
    'single-data': (_with(cp3, z_object=[Raw(lambda hh: hh.single(np.zeros((4, 6))))]), 'cmtf:hip:unsupported', None),
    'dense-size': (_with(cp3, z_object=[np.zeros((4, 3))]), 'cmtf:hip:invalid', 'Z.object{1}: size does not match Z.size of its modes'),
    'dense-size-transposed': (_with(cp3, z_object=[np.zeros((3, 4, 2))]), 'cmtf:hip:invalid', 'Z.object{1}: size does not match Z.size of its modes'),
    'sptensor-no-subs': (_with(cp3, z_object=[_sp_obj(subs=None)]), 'cmtf:hip:invalid', 'Z.object{1}: sptensor without double subs / size'),
    'sptensor-single-vals': (_with(cp3, z_object=[_sp_obj(vals=np.zeros((2, 1), dtype=np.float32))]), 'cmtf:hip:unsupported',
                             'Z.object{1}: sptensor values are not real doubles: it stays on the MATLAB path'),
    'sptensor-subs-shape': (_with(cp3, z_object=[_sp_obj(subs=np.ones((3, 2)))]), 'cmtf:hip:invalid', 'Z.object{1}: sptensor subs is not nnz x 3'),
    'sptensor-size': (_with(cp3, z_object=[_sp_obj(size=np.array([4.0, 3, 3]))]), 'cmtf:hip:invalid', 'Z.object{1}: size does not match Z.size of its modes'),
    'weights-length': (_with(sp3m, h_sparse_entry_weights=[[0.5, 0.5]]), 'cmtf:hip:invalid',
                       'options.hip.sparse_entry_weights{1} must hold one real double per stored entry of Z.object{1} (5)'),
    'weights-not-cell': (_with(sp3m, h_sparse_entry_weights=Raw(lambda hh: hh.double(np.ones(5)))), 'cmtf:hip:invalid', 'options.hip.sparse_entry_weights must be a cell over the blocks of Z.object'),
    'alpha-vector': (_with(sp3m, h_sparse_unstored_weight=Raw(lambda hh: hh.double(np.ones(2)))), 'cmtf:hip:invalid', 'options.hip.sparse_unstored_weight must be one number or a cell over the blocks of Z.object'),
    'weights-sharding': (_with(sp3m, h_sparse_entry_weights=[None], h_sparse_sharding=1), 'cmtf:hip:unsupported',
                         'options.hip.sparse_entry_weights is not available together with options.hip.sparse_sharding'),
    'observed-sharding': (_with(sp3m, h_sparse_observed_only=1, h_sparse_sharding=1), 'cmtf:hip:unsupported',
                          'options.hip.sparse_observed_only is not available together with options.hip.sparse_sharding'),
    'observed-cell': (_with(sp3m, h_sparse_observed_only=Raw(lambda hh: hh.cell([1.0]))), 'cmtf:hip:invalid', 'options.hip.sparse_observed_only must be 0, 1 or a list of block numbers'),
    'observed-uint8-list': (_with(sp3m, h_sparse_observed_only=Raw(lambda hh: hh.uint8([1, 1]))), 'cmtf:hip:invalid', 'options.hip.sparse_observed_only: a list of block numbers must be double'),
    'observed-dense': (_with(cp3, h_sparse_observed_only=[1, 1]), 'cmtf:hip:unsupported', 'options.hip.sparse_observed_only: Z.object{1} is dense (use Z.miss)'),
    'observed-par2': (_with(par2, h_sparse_observed_only=[1, 1]), 'cmtf:hip:unsupported', 'options.hip.sparse_observed_only: Z.object{1} is a PARAFAC2 block'),
    'precision': (_with(cp3, h_precision='f8'), 'aoadmm:precision', "options.hip.precision must be 'f64', 'f32' or 'f16', got 'f8'"),
    'state-empty-cell': (lambda: (lambda Z, G: (Z, dict(G, fac=[G['fac'][0], [G['fac'][1][0], None], G['fac'][2]]), {}))(*par2()),
                         'cmtf:hip:state', 'empty cell 2 in a cell-valued state field'),
    'mixed-slabs': (_with(par2, z_object=[[_X0, np.zeros((3, 3))]]), 'aoadmm:mixedSlabs', 'Z.object{1}: the slabs of a PARAFAC2 block must be all sparse or all full.'),
    'sparse-slab-count': (_with(par2, z_object=[[_X0, _X1, _X1]]), 'aoadmm:slabCount', 'Z.object{1} has 3 slabs, Z.size says 2.'),
    'sparse-slab-type': (_with(par2, z_object=[[_X0, Raw(lambda hh: hh.sparse(_X1, is_complex=True))]]), 'aoadmm:sparseSlabType', 'Z.object{1}{2} must be a real sparse double matrix.'),
    'sparse-slab-size': (_with(par2, z_object=[[_X0, _X0]]), 'aoadmm:slabSize', 'Z.object{1}{2} has size [3 2], Z.size says [3 3].'),
    'dense-slab-count': (_with(par2, z_object=[[np.zeros((3, 2))]]), 'aoadmm:slabCount', 'Z.object{1} has 1 slabs, Z.size says 2.'),
    'dense-slab-size': (_with(par2, z_object=[[np.zeros((3, 2)), np.zeros((3, 2))]]), 'aoadmm:slabSize', 'Z.object{1}{2} has size [3 2], Z.size says [3 3].'),
    'dense-slab-rows': (_with(par2, z_object=[[np.zeros((2, 2)), np.zeros((3, 3))]]), 'aoadmm:slabSize', 'Z.object{1}{1} has size [2 2], Z.size says [3 2].'),
    'dense-slab-type': (_with(par2, z_object=[[np.zeros((3, 2)), Raw(lambda hh: hh.single(np.zeros((3, 3))))]]), 'cmtf:hip:unsupported',
                        'Z.object{1}{2} is not a real double matrix: it stays on the MATLAB path'),
    'miss-sptensor': (_with(sp3m, z_miss=[np.ones((4, 3, 2))]), 'cmtf:missingData:sptensor', 'Missing data (Z.miss) not supported for sptensor objects. Convert to tensor first.'),
    'miss-sparse-slabs': (_with(par2_sparse, z_miss=[[np.ones((3, 2)), np.ones((3, 3))]]), 'cmtf:missingData:sparseSlabs',
                          'Missing data (Z.miss) not supported for sparse PARAFAC2 slabs. Convert to full slabs first.'),
    'miss-par2-not-cell': (_with(par2, z_miss=[np.ones((3, 5))]), 'cmtf:missingData:PAR2maskNotCell', 'Z.miss{1} must be a cell array of length 2 for PAR2.'),
    'miss-par2-slice-size': (_with(par2, z_miss=[[np.ones((3, 2)), np.ones((3, 2))]]), 'cmtf:missingData:PAR2maskSliceSizeMismatch', 'Z.miss{1}{2} size does not match Z.object{1}{2}.'),
    'miss-size': (_with(cp3, z_miss=[np.ones((4, 3))]), 'cmtf:missingData:maskSizeMismatch', 'Z.miss{1} size does not match Z.object{1}.'),
    'miss-not-uint8': (_with(cp3, z_miss=[Raw(lambda hh: hh.double(np.ones((4, 3, 2))))]), 'cmtf:missingData:maskSizeMismatch', 'Z.miss{1} size does not match Z.object{1}.'),
    'heldout-not-cell': (_with(cp3, h_heldout=Raw(lambda hh: hh.double([1.0]))), 'cmtf:hip:invalid', 'options.hip.heldout must be a cell with at most one entry per block of Z.object'),
    'heldout-not-struct': (_with(cp3, h_heldout=Raw(lambda hh: hh.cell([np.ones((1, 3))]))), 'cmtf:hip:invalid', 'options.hip.heldout{1} must be a struct with subs and vals'),
    'heldout-no-vals': (_with(cp3, h_heldout=Raw(lambda hh: hh.cell([dict(subs=np.ones((1, 3)))]))), 'cmtf:hip:missingField', "Reference to non-existent field 'vals'."),
    'heldout-shape': (_with(cp3, h_heldout={1: (np.array([[1, 1]]), [0.5])}), 'cmtf:hip:invalid', 'options.hip.heldout{1}: subs must be a double n x 3 array and vals n real doubles'),
    'heldout-fraction': (_with(cp3, h_heldout={1: (np.array([[1, 0.5, 1]]), [0.5])}), 'cmtf:hip:invalid', 'options.hip.heldout{1}: subscripts must be integers'),
    'ranklists-not-cell': (_with(cp3, h_rank_lists=Raw(lambda hh: hh.double([1.0]))), 'cmtf:hip:invalid', 'options.hip.rank_lists must be a cell with at most one entry per block of Z.object'),
    'ranklists-not-struct': (_with(cp3, h_rank_lists=Raw(lambda hh: hh.cell([np.ones((1, 3))]))), 'cmtf:hip:invalid', 'options.hip.rank_lists{1} must be a struct with mode and subs'),
    'ranklists-shape': (_with(cp3, h_rank_lists={1: dict(mode=1, subs=np.array([[1, 1]]))}), 'cmtf:hip:invalid', 'options.hip.rank_lists{1}: subs must be a double nq x 3 array'),
    'ranklists-fraction': (_with(cp3, h_rank_lists={1: dict(mode=1, subs=np.array([[1, 0.5, 1]]))}), 'cmtf:hip:invalid', 'options.hip.rank_lists{1}: subs must hold integers'),
    'ranklists-offsets': (_with(cp3, h_rank_lists={1: dict(_RL, exclude=([0, 1], [0]))}), 'cmtf:hip:invalid', 'options.hip.rank_lists{1}: excl_off must hold nq + 1 offsets and excl_idx doubles'),
    'ranklists-offsets-end': (_with(cp3, h_rank_lists={1: dict(_RL, exclude=([0, 1, 3], [0, 1]))}), 'cmtf:hip:invalid', 'options.hip.rank_lists{1}: excl_off ends at 3, excl_idx holds 2 rows'),
    'rank-metric-not-char': (_with(cp3, h_rank_metric=3.0), 'cmtf:hip:invalid', "options.hip.rank_metric must be a string such as 'ndcg@10', 'hit@5', 'mrr' or 'auc'"),
    'rank-metric-name': (_with(cp3, h_rank_metric='foo'), 'cmtf:hip:invalid', "options.hip.rank_metric 'foo': the metric must be hit, ndcg, mrr or auc"),
    'rank-metric-cut': (_with(cp3, h_rank_metric='mrr@3'), 'cmtf:hip:invalid', "options.hip.rank_metric 'mrr@3': the cut-off must be an integer in [1, 2^31) after hit or ndcg"),
    'keep-best-value': (_with(cp3, h_heldout=_HELD, h_heldout_keep_best=2.0), 'cmtf:hip:invalid', 'options.hip.heldout_keep_best must be 0 or 1'),
    'keep-best-string': (_with(cp3, h_heldout=_HELD, h_heldout_keep_best='1'), 'cmtf:hip:invalid', 'options.hip.heldout_keep_best must be 0 or 1'),
    'keep-best-no-list': (_with(cp3, h_heldout_keep_best=1.0), 'cmtf:hip:invalid', 'options.hip.heldout_keep_best = 1 needs a held-out list (options.hip.heldout)'),
    'keep-best-rank-criterion-no-ranklist': (_with(cp3, h_heldout=_HELD, h_heldout_keep_best=1.0, h_rank_criterion=1), 'cmtf:hip:invalid',
                                             'options.hip.heldout_keep_best = 1 needs a held-out list (options.hip.heldout)'),
}
# errors of the calls that are not [Fac, out] = aoadmm_mex(Z, G, options): the argument list, nlhs
USAGE = {
    'usage-two-args': (lambda: ([1.0, 2.0], 1), 'cmtf:hip:usage', 'usage: [Fac,out] = aoadmm_mex(Z, G, options)'),
    'usage-three-outputs': (lambda: ([1.0, 2.0, 3.0], 3), 'cmtf:hip:usage', 'usage: [Fac,out] = aoadmm_mex(Z, G, options)'),
    'op3-unknown': (lambda: (['unfold', np.ones((2, 2)), 1.0], 1), 'cmtf:hip:usage', "unknown operation 'unfold'"),
    'op4-unknown': (lambda: (['nvec', np.ones((2, 2)), 1.0, 1.0], 1), 'cmtf:hip:usage', "unknown operation 'nvec'"),
    'unfold-gram-4-way': (lambda: (['unfold_gram', np.ones((2, 2, 2, 2)), 1.0], 1), 'cmtf:hip:unsupported', 'unfold_gram handles matrices and 3-way tensors'),
    'unfold-gram-mode': (lambda: (['unfold_gram', np.ones((2, 2, 2)), 4.0], 1), 'cmtf:hip:unsupported', 'unfold_gram handles matrices and 3-way tensors'),
    'nvecs-dense': (lambda: (['nvecs', np.ones((2, 2)), 1.0, 1.0], 1), 'cmtf:hip:unsupported', "nvecs handles sptensors and sparse double matrices (dense data: 'unfold_gram')"),
    'nvecs-mode': (lambda: (['nvecs', sps.csc_matrix((3, 2)), 3.0, 1.0], 1), 'cmtf:hip:invalid', 'nvecs: mode 3 of an order-2 object'),
}


def _good_log(h):
    Z, G = cp3()
    return [c for c in run(h, Z, G)[3] if c['fn'] != 'aoadmm_create']


@pytest.fixture(scope='module')
def good_log(h):
    return _good_log(h)


@pytest.mark.parametrize('name', sorted(ERRORS))
def test_gateway_error(h, good_log, name):
    make, eid, text = ERRORS[name]
    Z, G, opt = make()
    with pytest.raises(MexError) as e:
        run(h, Z, G, opt)
    assert e.value.id == eid
    if text is not None:
        assert e.value.msg == text
    assert _good_log(h) == good_log                    # the next good call is what it would have been


@pytest.mark.parametrize('name', sorted(USAGE))
def test_usage_error(h, good_log, name):
    make, eid, text = USAGE[name]
    args, nlhs = make()
    with pytest.raises(MexError) as e:
        h.call(args, nlhs)
    assert (e.value.id, e.value.msg) == (eid, text)
    assert _good_log(h) == good_log


STATUS_IDS = {1: 'cmtf:hip:invalid', 2: 'cmtf:hip:device', 3: 'cmtf:hip:notPositiveDefinite', 4: 'cmtf:hip:rccl', 5: 'cmtf:hip:unsupported',
              6: 'cmtf:hip:outOfMemory', 7: 'cmtf:hip:invalid', -1: 'cmtf:hip:invalid'}


@pytest.mark.parametrize('status', sorted(STATUS_IDS))
def test_every_library_status_maps_to_its_id(h, good_log, status):
    Z, G = cp3()
    h.lib.fake_fail(b'aoadmm_solve', status)
    with pytest.raises(MexError) as e:
        run(h, Z, G)
    assert (e.value.id, e.value.msg) == (STATUS_IDS[status], 'fake: aoadmm_solve was told to fail')
    assert _good_log(h) == good_log


@pytest.mark.parametrize('fn', ['aoadmm_model_begin', 'aoadmm_model_set_mode', 'aoadmm_model_add_cp', 'aoadmm_model_set_constraint',
                                'aoadmm_model_set_coupling', 'aoadmm_model_end', 'aoadmm_tensor_upload', 'aoadmm_state_set', 'aoadmm_state_get'])
def test_an_error_at_any_stage_leaves_the_next_call_intact(h, good_log, fn):
    """Also between aoadmm_model_begin and aoadmm_model_end, which leaves the persistent context in the middle of a model:
    the next call begins a model again, on the same context."""
    Z, G = cp3()
    h.lib.fake_fail(fn.encode(), 1)
    with pytest.raises(MexError) as e:
        run(h, Z, G)
    assert e.value.id == 'cmtf:hip:invalid'
    log = h.log()
    assert log[-1]['fn'] == fn and not h.calls('aoadmm_create', log)
    assert _good_log(h) == good_log


def test_every_error_site_of_the_gateway_is_reached():
    """Each mexErrMsgIdAndTxt of the source is matched -- by its id and the literal start of its message -- by a case above."""
    src = open(MH.gateway_source()).read()
    sites = re.findall(r'mexErrMsgIdAndTxt\(\s*"([^"]+)",\s*"([^"]*)"', src)
    assert len(sites) == src.count('mexErrMsgIdAndTxt(') and len(sites) > 60
    cases = [(eid, text) for _, eid, text in list(ERRORS.values()) + list(USAGE.values())]
    cases += [(eid, 'fake: ') for eid in STATUS_IDS.values()]
    cases += [('cmtf:hip:missingField', "Reference to non-existent field 'size'."), ('cmtf:hip:unsupported', 'Z.object is not a double array, a dense tensor, a real double sptensor or a real sparse double matrix')]
    cases += [('cmtf:hip:invalid', "options.hip.rank_metric 'hit@0': the cut-off")]
    missed = []
    for eid, fmt in sites:
        # the first string literal of the format as a pattern: conversions match anything
        pat = '.*'.join(re.escape(piece) for piece in re.split(r'%[-0-9.]*(?:lld|d|s|e|f)', fmt))
        if fmt == '%s':
            ok = any(c[0] == eid and c[1] == 'fake: ' for c in cases)
        else:
            ok = any(c[0] == eid and c[1] is not None and re.match(pat, c[1]) for c in cases)
        if not ok:
            missed.append((eid, fmt))
    assert not missed, missed


def test_texts_of_the_two_errors_whose_table_entry_has_none(h):
    Z, G, opt = ERRORS['missing-field-Z'][0]()
    with pytest.raises(MexError) as e:
        run(h, Z, G, opt)
    assert e.value.msg == "Reference to non-existent field 'size'."
    Z, G, opt = ERRORS['single-data'][0]()
    with pytest.raises(MexError) as e:
        run(h, Z, G, opt)
    assert e.value.msg.startswith('Z.object is not a double array, a dense tensor, a real double sptensor or a real sparse double matrix')


def test_the_mock_refuses_what_matlab_leaves_undefined(h, good_log):
    Z, G = cp3()
    with pytest.raises(MockMisuse, match='mxGetScalar: the array is empty'):
        h.gateway(Z, G, dict(options(), MaxOuterIters=None))
    with pytest.raises(MockMisuse, match='mxGetDoubles: the array is not double'):
        h.gateway(dict(Z, weights=Raw(lambda hh: hh.uint8([1]))), G, options())
    with pytest.raises(MockMisuse, match='mxGetCell: the array is not a cell'):
        h.gateway(dict(Z, size=Raw(lambda hh: hh.double([4.0, 3, 2]))), G, options())
    with pytest.raises(MockMisuse, match='mxGetCell: index out of range'):
        h.gateway(dict(Z, constraints=[('non-negativity',)]), G, options())
    assert _good_log(h) == good_log


# ---------------------------------------------------------------------------------------------------------------- lifecycle
def test_context_lifecycle(fresh):
    h = fresh
    Z, G = cp3()
    created = lambda log: [(c['fn'], c.get('device', c.get('devices'))) for c in log if c['fn'] in ('aoadmm_create', 'aoadmm_create_multi', 'aoadmm_destroy')]
    log = run(h, Z, G)[3]
    assert log[0] == dict(fn='aoadmm_create', device=0) and log[1]['fn'] == 'aoadmm_model_begin' and log[1]['ctx'] == 1
    assert created(run(h, Z, G)[3]) == []                                             # reused
    assert created(run(h, Z, G, dict(hip=dict(device=0)))[3]) == []
    assert created(run(h, Z, G, dict(hip=dict(device=1)))[3]) == [('aoadmm_destroy', None), ('aoadmm_create', 1)]
    assert created(run(h, Z, G, dict(hip=dict(device=1)))[3]) == []
    log = run(h, Z, G, dict(hip=dict(devices=[0, 0])))[3]
    assert created(log) == [('aoadmm_destroy', None), ('aoadmm_create_multi', [0, 0])] and one(h, 'aoadmm_model_begin', log)['ctx'] == 3
    assert created(run(h, Z, G, dict(hip=dict(devices=[0, 0])))[3]) == []
    assert created(run(h, Z, G)[3]) == [('aoadmm_destroy', None), ('aoadmm_create', 0)]      # no options.hip: device 0
    h.call(['unfold_gram', np.ones((2, 2)), 1.0])
    assert created(h.log()) == []                                                     # the operations share the context
    # a context that cannot be created is not kept
    h.lib.fake_fail(b'aoadmm_create', 2)
    with pytest.raises(MexError) as e:
        run(h, Z, G, dict(hip=dict(device=2)))
    assert e.value.id == 'cmtf:hip:device'
    assert created(run(h, Z, G, dict(hip=dict(device=2)))[3]) == [('aoadmm_create', 2)]
    assert h.lib.mxmock_at_exit_registered() == 1
    assert (h.lib.fake_contexts_created(), h.lib.fake_contexts_destroyed()) == (5, 4)
    assert h.lib.mxmock_run_at_exit() == 1 and created(h.log()) == [('aoadmm_destroy', None)]
    assert h.lib.mxmock_run_at_exit() == 1 and h.log() == []                          # destroyed exactly once
    assert (h.lib.fake_contexts_created(), h.lib.fake_contexts_destroyed()) == (5, 5)


def test_operations_create_the_context_and_register_the_hook_once(fresh):
    h = fresh
    h.call(['unfold_gram', np.ones((2, 2)), 1.0])
    assert [c['fn'] for c in h.log()] == ['aoadmm_create', 'aoadmm_op_unfold_gram']
    Z, G = cp3()
    assert not h.calls('aoadmm_create', run(h, Z, G)[3])
    assert h.lib.mxmock_at_exit_registered() == 1
    assert h.lib.mxmock_run_at_exit() == 1 and [c['fn'] for c in h.log()] == ['aoadmm_destroy']


def test_nothing_the_gateway_created_outlives_the_call(fresh):
    """Arrays made during a call and not returned are released at its end (MATLAB's rule), the returned ones by the
    harness: between calls the mock holds nothing."""
    h = fresh
    for Z, G in (sp3()[:2], par2(cons_B=('non-negativity',)), (lambda Z, G: (dict(Z, object=[TensorObject(Z['object'][0])]), G))(*cp3())):
        h.gateway(Z, G, options(hip=dict(heldout=_HELD)))
        assert h.nodes_read > 20 and h.live_after - h.live_before == h.nodes_read
    # mxSetCell does not free the element it replaces: the gateway destroys what it displaces in the copy of G
    assert h.lib.mxmock_orphans() == 0


# ---------------------------------------------------------------------------------------------------------------- host_check
def test_host_check_program_runs(tmp_path):
    """tests/mxmock/host_check.cpp: a stand-alone program that hand-builds four inputs with the mock's constructors and
    calls mexFunction against the fake (the Makefile's `host_check_asan` target builds the same program under
    AddressSanitizer and UBSan; here it is built without)."""
    exe = MH.build_host_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'RESULT ok' in out.stdout, out.stdout
