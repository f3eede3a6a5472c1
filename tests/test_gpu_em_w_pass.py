"""GPU: ONE weighted dense EM pass (csrc/em.hip em_cp_vec_k / em_cp_k under EmWeighted) as a solve runs it -- `Engine.resident_em_pass`
on a block with `Engine.tensor_weights_upload` -- against the longdouble reference and the derived bounds of
tests/em_w_ref.py, in both precisions: every rank class of the strip kernel, the kernel for R > 32, rows, walk lengths,
several tiles per piece, matrix and 4-way blocks, the statistics-only pass, a second pass with other factors (q != 0), the
limits W = 1, W = 0, a single weight below 1 at every lane / slot position (the line ballot) and a boolean W against the
masked pass bit for bit, and the refusals of aoadmm_tensor_weights_upload.

Every update case checks: entries of weight 1 bitwise the data; every entry within its bound of w x0 + (1 - w) M; the four
statistics within their bounds (exactly 0 where the reference terms are); a second run on re-uploaded data returns the
same bits; `info` is the unfused masked launch's (test_gpu_em_pass._expected_info).

Observed error-to-bound ratios on an MI355X (largest over all cases of this file; every case prints its own).  The new
value comes close to its bound where w is just below 1: the bound is then the rounding of the final multiply-add alone.
             new value    num      den      obs_res   obs_x2
    fp64     0.989        0.036    0.017    0.019     0.037
    fp32     0.989        0.014    0.100    0.0059    0.0074
"""
import functools
import importlib

import numpy as np
import pytest

import em_ref
import em_w_ref
from helpers import cp_model, options
from test_gpu_em_pass import _block as _masked_block, _expected_info

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')
PRECS = ['f64', 'f32']


def _block(dims, R, X):
    n = len(dims)
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(dims),
                coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
                constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[X], _ranks=[R] * n)


@functools.lru_cache(maxsize=4)
def _data(dims, R):
    X, U = em_ref.make_data(dims, R, np.random.default_rng(1000 * sum(dims) + 7 * len(dims) + R))
    M = em_ref.model(U)
    for a in [X, M] + U:
        a.setflags(write=False)
    return X, U, M


def _weights(dims, kind):
    if isinstance(kind, tuple):                                          # ('single', index, value): one weight below 1
        W = np.ones(dims, order='F')
        W[tuple(kind[1])] = kind[2]
        return W
    return em_w_ref.make_weights(dims, np.random.default_rng(sum(dims) + len(kind)), kind)


def _check(ref, out, prec, W, X, update, what):
    rs = ref.stat_ratios(out['stats'], prec)
    re = ref.entry_ratio(out['data'], prec) if update else 0.0
    print('weighted em pass %s %s update=%d: entry %.3g of its bound, sums %s of theirs'
          % (what, prec, update, re, ' '.join('%.3g' % v for v in rs)))
    if update:
        assert np.array_equal(out['data'][W == 1], X[W == 1])            # bitwise: X holds fp32 values
        assert re <= 1.0, re
    else:
        assert np.array_equal(out['data'], ref.Xh)
    for q, name in enumerate(em_w_ref.STAT_NAMES):
        if ref.stats[q] == 0:
            assert out['stats'][q] == 0, (name, out['stats'][q])
        assert rs[q] <= 1.0, (name, rs[q], out['stats'][q], ref.stats[q])
    assert out['mttkrp'] is None and out['mttkrp_mode'] == -1 and out['info']['fused'] == -1


def _run(pkg, eng, dims, R, prec, kind='uniform', update=1, fuse=0):
    """One case: the pass twice on freshly uploaded data and weights, every check of the module docstring.  Returns the
    first call's result."""
    X, U, M = _data(dims, R)
    W = _weights(dims, kind)
    Z = _block(dims, R, np.asfortranarray(X))

    def once():
        pkg.build_model(eng, Z, prec, dense_entry_weights=[W])
        pkg.upload_state(eng, Z, dict(fac=list(U)))
        return eng.resident_em_pass(0, dims, R, update=update, fuse=fuse)

    out = once()
    assert out['info'] == _expected_info(dims, R, prec, -1), (out['info'], _expected_info(dims, R, prec, -1))
    ref = em_w_ref.EmWRef(X, W, em_w_ref.reset(X, W, prec), U, M=M)
    _check(ref, out, prec, W, X, update, '%s R=%d W=%s' % (dims, R, kind))
    again = once()
    assert again['stats'].tobytes() == out['stats'].tobytes()            # fixed summation order
    assert np.array_equal(again['data'], out['data'])
    return out


# ---- rank classes -----------------------------------------------------------------------------------------------------
RANK_SHAPES = [(37, 70, 9), (131, 67, 70)]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R', [1, 4, 5, 20, 21, 32, 33, 64])
@pytest.mark.parametrize('dims', RANK_SHAPES, ids=str)
def test_rank_classes(pkg, eng, dims, R, prec):
    """Both ends of rank classes of the strip kernel and the one-row kernel em_cp_k; fuse = 1 is ignored."""
    out = _run(pkg, eng, dims, R, prec, fuse=1)
    want = (1, 64) if R > 32 else (2 if prec == 'f64' else 4, (R + 3) // 4 * 4)
    assert (out['info']['vec'], out['info']['rmax']) == want


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('I', [1, 3, 13, 513, 525, 1025, 1029])
def test_rows(pkg, eng, I, prec):
    """Far below one wave, odd in both paddings, one row past a strip in fp64 (513, 525) and in fp32 (1025, 1029)."""
    _run(pkg, eng, (I, 9, 5), 5, prec)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('L', [1, 3, 64, 65, 130])
def test_walk_lengths(pkg, eng, L, prec):
    """1 and 3: fewer columns than the look-ahead ring holds; the tile edges."""
    _run(pkg, eng, (37, L, 9), 6, prec)


@pytest.mark.parametrize('prec', PRECS)
def test_pieces_of_several_tiles(pkg, eng, prec):
    """(8, 130, 3100): 2 pieces of the 130 columns: two whole tiles, then a ragged piece of 2 columns."""
    out = _run(pkg, eng, (8, 130, 3100), 5, prec)
    assert (out['info']['jchunks'], out['info']['jlen']) == (2, 128)


@pytest.mark.parametrize('prec', PRECS)
def test_matrix_block(pkg, eng, prec):
    """(30, 26): the natural array and the transposed copy are both imputed, from the transposed X0 and W; the two
    agree bitwise (the same rounded factors in the same order, the operands of each multiply-add swapped)."""
    dims, R = (30, 26), 4
    out = _run(pkg, eng, dims, R, prec)
    assert out['data_t'].shape == (26, 30)
    assert np.array_equal(out['data_t'].T, out['data'])
    stat = _run(pkg, eng, dims, R, prec, update=0)
    X, _, _ = _data(dims, R)
    assert np.array_equal(stat['data_t'].T, em_w_ref.reset(X, _weights(dims, 'uniform'), prec))


@pytest.mark.parametrize('prec', PRECS)
def test_four_way_block(pkg, eng, prec):
    """(12, 10, 9, 8): modes 3 and 4 merged, their factor the Khatri-Rao product built on the device."""
    out = _run(pkg, eng, (12, 10, 9, 8), 3, prec)
    assert out['info']['rmax'] == 4


@pytest.mark.parametrize('prec', PRECS)
def test_statistics_only_pass_leaves_xhat_alone(pkg, eng, prec):
    _run(pkg, eng, (37, 70, 9), 5, prec, update=0)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R', [5, 40])
def test_second_pass_with_other_factors(pkg, eng, R, prec):
    """q != 0: the second pass starts from the Xhat the first one left; num and den against the reference."""
    dims = (37, 70, 9)
    X, U, M = _data(dims, R)
    W = _weights(dims, 'uniform')
    U2 = em_ref.random_factors(dims, R, np.random.default_rng(99 + R))
    Z = _block(dims, R, np.asfortranarray(X))
    pkg.build_model(eng, Z, prec, dense_entry_weights=[W])
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    first = eng.resident_em_pass(0, dims, R)
    assert first['stats'][1] == 0                                        # den: q = 0 exactly after the reset
    pkg.upload_state(eng, Z, dict(fac=list(U2)))
    second = eng.resident_em_pass(0, dims, R)
    ref = em_w_ref.EmWRef(X, W, first['data'], U2)
    assert ref.stats[0] > 0 and ref.stats[1] > 0
    _check(ref, second, prec, W, X, 1, '%s R=%d second pass' % (dims, R))


# ---- the limits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R', [5, 40])
def test_unit_weights_change_nothing(pkg, eng, R, prec):
    dims = (37, 70, 9)
    out = _run(pkg, eng, dims, R, prec, kind='ones')
    assert np.array_equal(out['data'], _data(dims, R)[0])
    assert out['stats'][0] == 0 and out['stats'][1] == 0


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R', [5, 40])
def test_zero_weights_give_the_model(pkg, eng, R, prec):
    dims = (37, 70, 9)
    out = _run(pkg, eng, dims, R, prec, kind='zeros')
    _, U, M = _data(dims, R)
    err = np.abs(out['data'].astype(np.longdouble) - M).astype(np.float64)
    # at w = 0 the combine is exact (w x0 = 0, (1 - 0) m = m, fma(0, x0, m) = m): the model value's own bound
    assert np.all(err <= em_ref.beta(U, prec)), float((err / em_ref.beta(U, prec)).max())
    assert out['stats'][2] == 0 and out['stats'][3] == 0


def test_unit_weight_entries_survive_a_model_that_overflows(pkg, eng):
    """fp32, factors whose model overflows to inf: lines with a weight below 1 are written, and the entries of weight 1
    inside them must still be the data, not 1 * x0 + 0 * inf."""
    dims, R = (37, 9, 5), 3
    X = _data(dims, R)[0]
    W = _weights(dims, 'uniform')
    assert (W == 1).any() and (W < 1).any()
    U = [np.full((n, R), 1e15) for n in dims]                            # finite in fp64; the product is 1e45 > FLT_MAX
    Z = _block(dims, R, np.asfortranarray(X))
    pkg.build_model(eng, Z, 'f32', dense_entry_weights=[W])
    pkg.upload_state(eng, Z, dict(fac=U))
    out = eng.resident_em_pass(0, dims, R)
    assert np.array_equal(out['data'][W == 1], X[W == 1])
    assert not np.isfinite(out['data'][(W > 0) & (W < 1)]).any()


# One weight below 1 in a block of unit weights: one 128-byte line goes back and exactly one entry changes.  I = 260 (fp32:
# 65 vectors of 16 bytes per column) / 130 (fp64: the same): lane 0 of the strip sits at 16-byte slot w mod 8 of its line
# in column w (tests/test_gpu_em_pass.py), and lanes 0, 7, 8, 63, 64 are rows 0, 7, 8, 63, 64 times the vector.
SINGLE_I = {'f64': 130, 'f32': 260}


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('lane', [0, 7, 8, 63, 64])
def test_single_weight_at_every_slot(pkg, eng, lane, prec):
    I, vec = SINGLE_I[prec], (2 if prec == 'f64' else 4)
    dims = (I, 8, 2)
    X = _data(dims, 5)[0]
    for w in range(8):
        for v in (0, vec - 1):                                           # first and last entry of the lane's vector
            idx = (lane * vec + v, w, 1)
            out = _run(pkg, eng, dims, 5, prec, kind=('single', idx, 0.25))
            changed = np.argwhere(out['data'] != X)
            assert changed.tolist() == [list(idx)], changed
            assert out['stats'][0] > 0 and out['stats'][1] == 0


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('where', ['first', 'last'])
def test_single_weight_at_the_ends_of_the_block(pkg, eng, where, prec):
    dims = (37, 70, 9)
    idx = (0, 0, 0) if where == 'first' else (36, 69, 8)
    out = _run(pkg, eng, dims, 5, prec, kind=('single', idx, 0.0))
    assert np.argwhere(out['data'] != _data(dims, 5)[0]).tolist() == [list(idx)]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('dims,R', [((37, 70, 9), 5), ((131, 67, 70), 20), ((37, 70, 9), 40), ((30, 26), 4)], ids=str)
def test_boolean_weights_are_the_masked_pass_bit_for_bit(pkg, eng, dims, R, prec):
    """Two passes each (the second with other factors, over the imputed block): data and all four statistics of the
    weighted block are those of the masked block that holds zeros at its missing entries, fuse = 0."""
    X, U, _ = _data(dims, R)
    obs = np.random.default_rng(5 * sum(dims) + R).random(dims) >= 0.3
    Xz = np.asfortranarray(np.where(obs, X, 0.0))
    U2 = em_ref.random_factors(dims, R, np.random.default_rng(3 + R))

    def two_passes(Z, **kw):
        pkg.build_model(eng, Z, prec, **kw)
        outs = []
        for fac in (U, U2):
            pkg.upload_state(eng, Z, dict(fac=list(fac)))
            outs.append(eng.resident_em_pass(0, dims, R, update=1, fuse=0))
        return outs

    masked = two_passes(_masked_block(dims, R, Xz, obs))
    weighted = two_passes(_block(dims, R, Xz), dense_entry_weights=[obs.astype(np.float64)])
    for a, b in zip(masked, weighted):
        assert a['info'] == b['info']
        assert a['stats'].tobytes() == b['stats'].tobytes(), (a['stats'], b['stats'])
        assert a['data'].tobytes() == b['data'].tobytes()
        if len(dims) == 2:
            assert a['data_t'].tobytes() == b['data_t'].tobytes()


# ---- aoadmm_tensor_weights_upload -------------------------------------------------------------------------------------
def _weighted_block(pkg, eng, dims=(9, 7, 3), R=2, prec='f64'):
    X, U, _ = _data(dims, R)
    W = _weights(dims, 'uniform')
    Z = _block(dims, R, np.asfortranarray(X))
    pkg.build_model(eng, Z, prec, dense_entry_weights=[W])
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    return Z, X, W, U


def _normsq(eng):
    import ctypes as C
    v = C.c_double(0)
    capi.check(eng.lib.aoadmm_tensor_normsq(eng.h, 0, C.byref(v)))
    return v.value


def _raises(pkg, code, fn, word=None):
    with pytest.raises(pkg.AoadmmError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    if word:
        assert word in str(ei.value), str(ei.value)


@pytest.mark.parametrize('bad', [1.0 + 1e-12, -1e-12, float('inf'), float('nan')])
def test_a_weight_outside_the_range_leaves_the_block_as_it_was(pkg, eng, bad):
    dims, R = (9, 7, 3), 2
    Z, X, W, U = _weighted_block(pkg, eng)
    before = eng.resident_em_pass(0, dims, R, update=0)
    Wb = W.copy()
    Wb[8, 6, 2] = bad
    _raises(pkg, capi.ERR_INVALID, lambda: eng.tensor_weights_upload(0, Wb), '[0, 1]')
    after = eng.resident_em_pass(0, dims, R, update=0)
    assert after['stats'].tobytes() == before['stats'].tobytes() and np.array_equal(after['data'], before['data'])


def test_refusals(pkg, eng, monkeypatch):
    dims, R = (9, 7, 3), 2
    X, U, _ = _data(dims, R)
    W = _weights(dims, 'uniform')
    lib = eng.lib
    # no data yet
    Z = _block(dims, R, np.asfortranarray(X))
    import ctypes as C
    capi.check(lib.aoadmm_model_begin(eng.h, 3, 1, 0))
    for m, n in enumerate(dims):
        capi.check(lib.aoadmm_model_set_mode(eng.h, m, n, R))
    capi.check(lib.aoadmm_model_add_cp(eng.h, 0, 3, (C.c_int * 3)(0, 1, 2), 1.0))
    capi.check(lib.aoadmm_model_end(eng.h))
    _raises(pkg, capi.ERR_INVALID, lambda: eng.tensor_weights_upload(0, W), 'no data')
    # a sparse block: the message names the sparse call
    subs = np.argwhere(np.abs(X) > 1.0)
    eng.upload_coo(0, subs, X[tuple(subs.T)])
    _raises(pkg, capi.ERR_INVALID, lambda: eng.tensor_weights_upload(0, W), 'aoadmm_tensor_set_entry_weights')
    # an fp16 block
    pkg.build_model(eng, Z, 'f16')
    _raises(pkg, capi.ERR_INVALID, lambda: eng.tensor_weights_upload(0, W), 'fp16')
    # a PARAFAC2 block
    rng = np.random.default_rng(4)
    Zp = dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=[6, [4, 5], 2],
              coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
              constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0],
              object=[[rng.standard_normal((6, 4)), rng.standard_normal((6, 5))]], _ranks=[2] * 3)
    pkg.build_model(eng, Zp, 'f64')
    _raises(pkg, capi.ERR_UNSUPPORTED, lambda: eng.tensor_weights_upload(0, np.ones((6, 9))), 'PARAFAC2')
    # a one-process multi-device context
    with pkg.Engine([0, 0]) as e2:
        pkg.build_model(e2, Z, 'f64')
        _raises(pkg, capi.ERR_UNSUPPORTED, lambda: e2.tensor_weights_upload(0, W), 'multi-device')
    # the engine works on afterwards
    _run(pkg, eng, dims, R, 'f64')


def test_a_released_natural_array_is_refused(pkg, monkeypatch):
    import copy
    from oracle import aoadmm as OA
    rng = np.random.default_rng(77)
    dims = (120, 90, 80)                               # beyond the one-launch MTTKRP of tiny blocks (test_gpu_solver.py)
    Z, io, _ = cp_model(dims, 4, rng, [None] * 3)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(5))
    monkeypatch.setenv('AOADMM_RELEASE_NATURAL', '1')
    with pkg.Engine(0) as e:
        pkg.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=4), init=copy.deepcopy(G), engine=e)
        _raises(pkg, capi.ERR_INVALID, lambda: e.tensor_weights_upload(0, np.ones(dims)), 'released')


def test_mask_after_weights_and_weights_after_mask(pkg, eng):
    """The later call wins: a mask drops the weights (Xhat <- X0 first), weights drop the mask; NULL makes the block
    plain again."""
    dims, R = (9, 7, 3), 2
    Z, X, W, U = _weighted_block(pkg, eng)
    eng.resident_em_pass(0, dims, R)                                     # Xhat now holds imputed values
    obs = np.random.default_rng(8).random(dims) >= 0.3
    mk = np.asfortranarray(obs, dtype=np.uint8)
    import ctypes as C
    capi.check(eng.lib.aoadmm_tensor_mask_upload(eng.h, 0, mk.ctypes.data_as(C.POINTER(C.c_uint8))))
    got = eng.resident_em_pass(0, dims, R, update=0)
    ref = em_ref.EmRef(X, obs, U)
    assert np.array_equal(got['data'], X)                                # the data as uploaded
    assert np.all(ref.stat_ratios(got['stats'], 'f64') <= 1.0)
    # weights after the mask
    eng.tensor_weights_upload(0, W)
    got = eng.resident_em_pass(0, dims, R, update=0)
    wref = em_w_ref.EmWRef(X, W, em_w_ref.reset(X, W, 'f64'), U)
    assert np.all(wref.stat_ratios(got['stats'], 'f64') <= 1.0)
    assert np.array_equal(got['data'], wref.Xh)
    # NULL: plain again, holding the data
    eng.tensor_weights_upload(0, None)
    _raises(pkg, capi.ERR_INVALID, lambda: eng.resident_em_pass(0, dims, R), 'neither masked nor weighted')
    assert _normsq(eng) == pytest.approx(float(np.sum(X * X)), rel=1e-13)


def test_weights_on_an_imputed_masked_block_are_refused(pkg, eng):
    """After a masked update pass the block holds model values at its missing entries: they must not become data."""
    dims, R = (9, 7, 3), 2
    X, U, _ = _data(dims, R)
    obs = np.random.default_rng(9).random(dims) >= 0.3
    Z = _masked_block(dims, R, np.asfortranarray(X), obs)
    pkg.build_model(eng, Z, 'f64')
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    eng.resident_em_pass(0, dims, R, update=0)
    eng.tensor_weights_upload(0, _weights(dims, 'uniform'))              # nothing imputed yet: the weights win
    pkg.build_model(eng, Z, 'f64')
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    before = eng.resident_em_pass(0, dims, R, update=1)
    _raises(pkg, capi.ERR_INVALID, lambda: eng.tensor_weights_upload(0, _weights(dims, 'uniform')), 'upload the data again')
    after = eng.resident_em_pass(0, dims, R, update=0)                   # still the masked block
    assert np.array_equal(after['data'], before['data']) and after['stats'][3] == before['stats'][3]


def test_normsq_and_storage_of_a_weighted_block(pkg, eng):
    dims, R = (9, 7, 3), 2
    X = _data(dims, R)[0]
    Z = _block(dims, R, np.asfortranarray(X))
    pkg.build_model(eng, Z, 'f64')
    plain = eng.tensor_storage_info(0)[2]
    Z, X, W, U = _weighted_block(pkg, eng)
    assert _normsq(eng) == pytest.approx(float(np.sum(W * X * X)), rel=1e-13)
    pad = 10 * 7 * 3 * 8                                                 # one array of the padded block
    assert plain >= pad and eng.tensor_storage_info(0)[2] == 3 * pad     # Xhat, X0, W and no pass copy
