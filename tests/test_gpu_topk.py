"""GPU: top-k completions of a CP block along one mode (aoadmm_resident_topk; csrc/topk.hip).
The models hold no data (an empty sptensor) unless a test is about the kind of block; the reference is numpy: fp64
scores, then lexsort((arange(I), -score)) over the rows that are not excluded and whose score is not NaN."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from helpers import cp_model, options
from test_gpu_heldout import par2_block
from test_gpu_sparse_observed import NN, OBSERVED, observed_models
from test_gpu_sparse_sharded import cp_Z, empty, on_ranks

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')
TOPK_CLASS = 13
TOL = 1e-12            # times sum_r prod_n |F_n|: model_at's bar of DESIGN.md section 9.4 ((R + N) 2^-53 derived)


def dataless(pkg, e, U):
    shape = tuple(u.shape[0] for u in U)
    Z = cp_Z(shape, U[0].shape[1], empty(pkg, shape))
    pkg.build_model(e, Z)
    pkg.upload_state(e, Z, {'fac': U})
    return Z


def int_factors(rng, shape, R):
    return [rng.integers(-3, 4, (s, R)).astype(np.float64) for s in shape]


def queries(rng, shape, nq):
    return np.stack([rng.integers(0, s, nq) for s in shape], axis=1).astype(np.int64)


def weights(U, mode, subs):
    W = np.ones((subs.shape[0], U[0].shape[1]))
    for m in range(len(U)):
        if m != mode:
            W = W * U[m][subs[:, m]]
    return W


def ref_topk(U, mode, subs, k, exclude=None, with_scores=False):
    """(idx nq x k, val nq x k[, scores I x nq, bound I x nq]) by the rule of the header, in numpy."""
    W = weights(U, mode, subs)
    S = U[mode] @ W.T
    I, nq = S.shape
    idx = np.full((nq, k), -1, dtype=np.int64)
    val = np.full((nq, k), -np.inf)
    for q in range(nq):
        s = S[:, q]
        ok = ~np.isnan(s)
        if exclude is not None:
            ok[np.asarray(exclude[1][exclude[0][q]:exclude[0][q + 1]], dtype=np.int64)] = False
        rows = np.flatnonzero(ok)
        if len(rows) > k:                                      # only rows that reach the k-th largest score can be among
            rows = rows[s[rows] >= np.partition(s[rows], -k)[-k]]   # the first k: the order below is that of all rows
        order = rows[np.lexsort((rows, -s[rows]))][:k]
        idx[q, :len(order)] = order
        val[q, :len(order)] = s[order]
    if with_scores:
        return idx, val, S, np.abs(U[mode]) @ np.abs(W).T
    return idx, val


def check_close(U, mode, subs, k, got, exclude=None):
    """The rule of the real-valued tests: on the numpy side every gap between consecutive scores among the first k + 1
    candidates exceeds twice the tolerance (no position can be skipped); then idx is numpy's at every position and val
    lies within TOL sum_r prod_n |F_n| of numpy's per entry.  Returns the smallest gap in units of twice the tolerance."""
    idx, val = got
    ridx, rval, S, B = ref_topk(U, mode, subs, k + 1, exclude, with_scores=True)
    worst = np.inf
    for q in range(subs.shape[0]):
        have = int(np.sum(ridx[q] >= 0))
        tol = TOL * B[ridx[q, :have], q]
        gaps = rval[q, :have - 1] - rval[q, 1:have]
        need = 2.0 * np.maximum(tol[:-1], tol[1:])
        assert np.all(gaps > need), (q, float(np.min(gaps / need)))
        if have > 1:
            worst = min(worst, float(np.min(gaps / need)))
        n = min(have, k)
        assert np.array_equal(idx[q], ridx[q, :k]), (q, idx[q], ridx[q, :k])
        assert np.all(np.abs(val[q, :n] - rval[q, :n]) <= tol[:n]), q
        assert np.all(np.isneginf(val[q, n:]))
    return worst


# ---- 1. exact --------------------------------------------------------------------------------------------------------
PAIRS = [(N, mode) for N in (2, 3, 4) for mode in range(N)]                       # 9: the free mode in every position
RS = [1, 3, 4, 5, 16, 17, 20, 33, 64]
IS = [1, 15, 16, 17, 255, 256, 257, 1000, 5003]
NQS = [1, 15, 16, 17, 40]
KS = [1, 2, 10, 64]
# 40 combinations; the strides are coprime to the lengths of the lists, so every value of every list occurs, and the
# shift per round of nine pairs every rank with several lengths
EXACT = [(PAIRS[t % 9] + (RS[(2 * t + t // 9) % 9], IS[(4 * t + 1 + 2 * (t // 9)) % 9], NQS[t % 5], KS[(3 * t) % 4])) for t in range(40)]


def test_the_exact_cases_touch_every_value():
    assert len(set(EXACT)) == 40
    for pos, values in [(slice(0, 2), PAIRS), (2, RS), (3, IS), (4, NQS), (5, KS)]:
        assert {c[pos] for c in EXACT} == set(values)


@pytest.mark.parametrize('N,mode,R,I,nq,k', EXACT)
def test_exact(pkg, eng, N, mode, R, I, nq, k):
    """Integer factors in [-3, 3]: every score is exact in any order and ties abound; idx and val equal numpy's."""
    rng = np.random.default_rng(hash((N, mode, R, I, nq, k)) % (2 ** 32))
    shape = [6, 5, 4, 3][:N]
    shape[mode] = I
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    subs = queries(rng, shape, nq)
    subs[:, mode] = -5                                         # ignored and not range-checked
    idx, val = eng.topk(0, mode, subs, k)
    ridx, rval = ref_topk(U, mode, subs, k)
    assert idx.shape == (nq, k) and idx.dtype == np.int64 and val.shape == (nq, k)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)


@pytest.mark.parametrize('KS', range(1, 17))
def test_exact_at_every_chain_length(pkg, eng, KS):
    """Every compiled-in chain length ceil(R / 4) = 1 .. 16 at R = 4 KS - 1: the last step carries a zeroed column and a
    clamped column address.  I = 273 and nq = 17 are the smallest that take every branch of the stream: two tiles per
    workgroup, the second ragged, and two slabs of 144 and 129 rows, which is more than two turns of the ring of four
    steps and a last step that holds one live row."""
    from rank_of_ref import count_plan
    mode, R, I, nq, k = 1, 4 * KS - 1, 273, 17, 2              # N = 3
    qt, qtiles, slabs, slab_rows = count_plan(I, nq)           # top-k's plan at k <= 32
    assert (qt, qtiles, slabs, slab_rows, I - slab_rows) == (2, 1, 2, 144, 129)
    rng = np.random.default_rng(1000 + KS)
    shape = [6, I, 4]
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    subs = queries(rng, shape, nq)
    subs[:, mode] = -5                                         # ignored and not range-checked
    idx, val = eng.topk(0, mode, subs, k)
    ridx, rval = ref_topk(U, mode, subs, k)
    assert idx.shape == (nq, k) and idx.dtype == np.int64 and val.shape == (nq, k)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)


def test_nan_scores_are_no_candidates(pkg, eng):
    rng = np.random.default_rng(3)
    U = int_factors(rng, (300, 5), 4)
    U[0][7, 1] = np.nan                                        # row 7's score is NaN wherever w(1) is used
    U[0][9, 0] = np.inf
    U[0][11, 0] = -np.inf
    U[1][:, :2] = np.abs(U[1][:, :2]) + 1.0                   # w(0), w(1) > 0: +inf first, -inf last, NaN nowhere
    dataless(pkg, eng, U)
    subs = queries(rng, (300, 5), 17)
    idx, val = eng.topk(0, 0, subs, 64)
    with np.errstate(invalid='ignore'):
        ridx, rval = ref_topk(U, 0, subs, 64)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)
    assert not (idx == 7).any() and (idx[:, 0] == 9).all()
    idx, val = eng.topk(0, 0, subs, 64, exclude=(np.arange(18) * 0, []))
    assert np.array_equal(idx, ridx)


# ---- 2. padding --------------------------------------------------------------------------------------------------------
def test_padding(pkg, eng):
    rng = np.random.default_rng(4)
    shape = (5, 6, 4)
    U = int_factors(rng, shape, 3)
    dataless(pkg, eng, U)
    subs = queries(rng, shape, 4)
    idx, val = eng.topk(0, 0, subs, 10)                        # k > I
    ridx, rval = ref_topk(U, 0, subs, 10)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)
    assert (idx[:, 5:] == -1).all() and np.isneginf(val[:, 5:]).all() and (idx[:, :5] >= 0).all()
    # k larger than the rows left after exclusion; every row excluded
    ex = (np.array([0, 4, 4, 10, 16]), np.array([0, 1, 2, 3, 4, 4, 4, 3, 2, 2, 5, 4, 3, 2, 1, 0]))
    idx, val = eng.topk(0, 1, subs, 4, exclude=ex)
    ridx, rval = ref_topk(U, 1, subs, 4, ex)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)
    assert (idx[0, 2:] == -1).all() and (idx[0, :2] >= 4).all()
    assert (idx[2] >= 0).sum() == 3 and (idx[3] == -1).all() and np.isneginf(val[3]).all()


# ---- 3. exclusions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('I,R,k', [(1000, 5, 10), (5003, 20, 64), (257, 3, 2)])
def test_exclusions(pkg, eng, I, R, k):
    rng = np.random.default_rng(I + R)
    shape = (6, I, 5)
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    nq = 40
    subs = queries(rng, shape, nq)
    best, _ = ref_topk(U, 1, subs, 1)
    lists = []
    for q in range(nq):
        if q % 4 == 3:
            lists.append(np.zeros(0, dtype=np.int64))         # no exclusions for this query
            continue
        rows = rng.integers(0, I, int(rng.integers(1, 3 * k + 2)))
        rows = np.concatenate([rows, rows[:3], best[q]])       # duplicates, and the best row itself
        lists.append(rows[rng.permutation(len(rows))])         # unsorted
    off = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    ex = (off, np.concatenate(lists))
    idx, val = eng.topk(0, 1, subs, k, exclude=ex)
    ridx, rval = ref_topk(U, 1, subs, k, ex)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)
    for q in range(nq):
        assert not np.isin(idx[q], lists[q]).any()
        assert (best[q, 0] in idx[q]) == (q % 4 == 3)
    for bad in (I, -1):                                        # an excluded row out of range
        rows = ex[1].copy()
        rows[len(rows) // 2] = bad
        with pytest.raises(pkg.AoadmmError) as ei:
            eng.topk(0, 1, subs, k, exclude=(off, rows))
        assert ei.value.code == capi.ERR_INVALID
    for bad_off in (off + 1, np.concatenate([off[:5], [off[4] - 1], off[6:]])):   # not from 0; decreasing
        with pytest.raises(pkg.AoadmmError) as ei:
            eng.topk(0, 1, subs, k, exclude=(bad_off, np.concatenate([ex[1], [0]])[:bad_off[-1]]))
        assert ei.value.code == capi.ERR_INVALID


# ---- 4. several slabs and buffer compaction --------------------------------------------------------------------------------
def test_several_slabs_and_compaction(pkg, eng):
    rng = np.random.default_rng(5)
    I, R, nq, k = 70001, 20, 3, 64
    shape = (4, I, 3)
    U = int_factors(rng, shape, R)
    subs = queries(rng, shape, nq)
    dataless(pkg, eng, U)
    idx, val = eng.topk(0, 1, subs, k)
    ridx, rval = ref_topk(U, 1, subs, k)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)
    # scores that ascend along every slab: every row beats the threshold and the buffers are compacted all the way
    e0 = np.zeros(R)
    e0[0] = 1.0
    U[0][:] = e0
    U[2][:] = e0
    for column in (np.arange(I, dtype=np.float64), np.arange(I, dtype=np.float64)[::-1].copy()):
        U[1][:, 0] = column
        dataless(pkg, eng, U)
        idx, val = eng.topk(0, 1, subs, k)
        ridx, rval = ref_topk(U, 1, subs, k)
        assert np.array_equal(val, rval) and np.array_equal(idx, ridx)
        assert np.array_equal(val[0], np.arange(I - 1, I - 1 - k, -1.0))
        ex = (np.array([0, 2, 2, 5]), np.array([idx[0, 0], idx[0, 5], idx[2, 63], idx[2, 0], idx[2, 1]]))
        idx, val = eng.topk(0, 1, subs, k, exclude=ex)
        ridx, rval = ref_topk(U, 1, subs, k, ex)
        assert np.array_equal(val, rval) and np.array_equal(idx, ridx)


# ---- 5. real-valued ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('I,R,N,nq,k', [(5003, 20, 3, 40, 64), (257, 64, 4, 17, 64), (1000, 5, 2, 16, 10)])
def test_real_valued(pkg, eng, I, R, N, nq, k):
    """val within 1e-12 sum_r prod_n |F_n| of numpy per entry, idx numpy's at every position; the numpy side first shows
    that no position can be skipped (check_close)."""
    rng = np.random.default_rng(0)
    shape = [7, 6, 5, 4][:N]
    shape[N - 1] = I
    U = [rng.standard_normal((s, R)) for s in shape]
    dataless(pkg, eng, U)
    subs = queries(rng, shape, nq)
    worst = check_close(U, N - 1, subs, k, eng.topk(0, N - 1, subs, k))
    print('smallest gap: %.3g times twice the tolerance' % worst)


# ---- 6. no score array ---------------------------------------------------------------------------------------------------
def test_no_score_array(pkg, eng):
    """2-way, I = 2 000 000, R = 4, nq = 20 000, k = 10: an I x nq fp64 array would be 320 GB."""
    rng = np.random.default_rng(0)
    I, J, R, nq, k = 2_000_000, 5000, 4, 20_000, 10
    U = [rng.standard_normal((I, R)), rng.standard_normal((J, R))]
    dataless(pkg, eng, U)
    subs = queries(rng, (I, J), nq)
    idx, val = eng.topk(0, 0, subs, k)
    assert idx.shape == (nq, k) and (idx >= 0).all()
    pick = rng.choice(nq, 50, replace=False)
    worst = check_close(U, 0, subs[pick], k, (idx[pick], val[pick]))
    print('smallest gap: %.3g times twice the tolerance' % worst)


# ---- 7. the bits depend on the inputs only -------------------------------------------------------------------------------
def test_bits_depend_on_the_inputs_only(pkg, eng):
    rng = np.random.default_rng(7)
    shape, R, k = (5003, 30, 20), 20, 64
    U = [rng.standard_normal((s, R)) for s in shape]
    dataless(pkg, eng, U)
    subs = queries(rng, shape, 40)
    first = eng.topk(0, 0, subs, k)
    second = eng.topk(0, 0, subs, k)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    for q in (0, 17, 39):                                      # asked alone: another tile shape, another slab cut
        alone = eng.topk(0, 0, subs[q:q + 1], k)
        assert np.array_equal(alone[0][0], first[0][q]) and np.array_equal(alone[1][0], first[1][q])
    part = eng.topk(0, 0, subs[3:20], k)
    assert np.array_equal(part[0], first[0][3:20]) and np.array_equal(part[1], first[1][3:20])


def test_bits_after_a_solve_and_after_an_upload(pkg, eng):
    """After a solve the row-major factor copies are current and are gathered from; the same factors uploaded are
    gathered column-major.  Same bits."""
    rng = np.random.default_rng(8)
    shape, R, k = (300, 40, 30), 4, 10
    Z, io, _ = cp_model(shape, R, rng, [NN] * 3)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, Fac, _, _ = pkg.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=3), init=copy.deepcopy(G), engine=eng)
    subs = queries(rng, shape, 33)
    for mode in range(3):
        pkg.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=3), init=copy.deepcopy(G), engine=eng)
        after_solve = eng.topk(0, mode, subs, k)
        eng.model_at(0, subs)                                  # the held-out pass reports which layout the factors offer
        assert eng.heldout_info(0)['row_major'] == 1
        pkg.upload_state(eng, Z, {'fac': Fac['fac']})
        after_upload = eng.topk(0, mode, subs, k)
        eng.model_at(0, subs)
        assert eng.heldout_info(0)['row_major'] == 0
        assert np.array_equal(after_solve[0], after_upload[0]) and np.array_equal(after_solve[1], after_upload[1])
        check_close([np.asarray(f) for f in Fac['fac']], mode, subs, k, after_upload)


# ---- 8. every kind of block ----------------------------------------------------------------------------------------------
def test_every_kind_of_block(pkg, eng):
    rng = np.random.default_rng(9)
    shape, R, k = (300, 12, 10), 5, 10
    U = [rng.standard_normal((s, R)) for s in shape]
    subs = queries(rng, shape, 40)
    dataless(pkg, eng, U)
    want = [eng.topk(0, mode, subs, k) for mode in range(3)]
    keep = rng.random(shape) < 0.2
    X = rng.standard_normal(shape)
    S = pkg.sptensor(np.argwhere(keep), X[keep], shape)

    def same(e, mode, rows=slice(None)):
        got = e.topk(0, mode, subs[rows], k)
        assert np.array_equal(got[0], want[mode][0][rows]) and np.array_equal(got[1], want[mode][1][rows])

    for obj, kw in [(X, {}), (X, dict(precision='f16')), (S, {}), (S, dict(observed_only=1))]:
        Z = cp_Z(shape, R, obj)
        pkg.build_model(eng, Z, **kw)
        pkg.upload_state(eng, Z, {'fac': U})
        for mode in range(3):
            same(eng, mode)

    def rank_fn(e, r):                                         # sharded sparse, every rank asks its own queries
        Z = cp_Z(shape, R, S)
        pkg.build_model(e, Z, sparse_sharding=True)
        pkg.upload_state(e, Z, {'fac': U})
        for mode in range(3):
            same(e, mode, slice(0, 23) if r == 0 else slice(23, 40))
        return True

    assert on_ranks(pkg, 2, rank_fn) == [True, True]


# ---- 9. end to end -------------------------------------------------------------------------------------------------------
def test_end_to_end_on_the_observed_only_model(pkg, eng):
    rng = np.random.default_rng(11)
    Z, io, A = cp_model((30, 25, 20), 3, rng, [NN] * 3, noise=0.0)
    mask = rng.random((30, 25, 20)) < 0.3
    Zm, Zs = observed_models(pkg, Z, 0, mask)
    G = OA.init_coupled_AOADMM_CMTF({**Zm, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, Fac, _, _ = pkg.cmtf_AOADMM(Zs, alg_options={**options(MaxOuterIters=20), **OBSERVED}, init=copy.deepcopy(G), engine=eng)
    S = Zs['object'][0]
    k = 5
    subs = np.stack([rng.integers(0, 30, 10), np.zeros(10, dtype=np.int64), rng.integers(0, 20, 10)], axis=1)
    ex = S.fiber_lists(1, subs)
    got = eng.topk(0, 1, subs, k, exclude=ex)
    check_close([np.asarray(f) for f in Fac['fac']], 1, subs, k, got, ex)
    stored = {tuple(s) for s in S.subs.tolist()}
    for q in range(10):
        assert len(ex[1][ex[0][q]:ex[0][q + 1]]) == int(mask[subs[q, 0], :, subs[q, 2]].sum())
        for j in got[0][q]:
            assert j >= 0 and (int(subs[q, 0]), int(j), int(subs[q, 2])) not in stored


# ---- 10. refusals and accounting -----------------------------------------------------------------------------------------
def raw_topk(e, p, mode, subs, k, cols):
    """The C entry itself with pre-filled outputs: (status, idx, val)."""
    subs = np.asfortranarray(np.asarray(subs, dtype=np.int64))
    idx = np.full((subs.shape[0], cols), 77, dtype=np.int64)
    val = np.full((subs.shape[0], cols), 0.5)
    i64p = C.POINTER(C.c_int64)
    st = e.lib.aoadmm_resident_topk(e.h, p, mode, subs.shape[0], subs.ctypes.data_as(i64p), k, None, None,
                                    idx.ctypes.data_as(i64p), capi.dptr(val))
    return st, idx, val


def test_refusals_and_accounting(pkg, eng):
    rng = np.random.default_rng(12)
    shape, R = (40, 1000, 6), 5
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    subs = queries(rng, shape, 17)
    for mode, k, s in [(1, 0, subs), (1, 65, subs), (3, 4, subs), (-1, 4, subs),
                       (1, 4, np.where(np.arange(17)[:, None] == 9, [40, 0, 0], subs)),
                       (1, 4, np.where(np.arange(17)[:, None] == 2, [0, 0, -1], subs))]:
        st, idx, val = raw_topk(eng, 0, mode, s, k, 65)
        assert st == capi.ERR_INVALID, (mode, k)
        assert (idx == 77).all() and (val == 0.5).all()       # untouched
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.topk(0, 1, subs, 0)
    assert ei.value.code == capi.ERR_INVALID
    # nq = 0 is a no-op
    idx, val = eng.topk(0, 1, np.zeros((0, 3), dtype=np.int64), 4)
    assert idx.shape == (0, 4) and val.shape == (0, 4)
    assert eng.lib.aoadmm_resident_topk(eng.h, 0, 1, 0, None, 4, None, None, None, None) == capi.OK
    assert eng.lib.aoadmm_resident_topk(eng.h, 0, 1, -1, None, 4, None, None, None, None) == capi.ERR_INVALID
    # accounting
    eng.kernel_stats(TOPK_CLASS, reset=True)
    for calls, (mode, nq) in enumerate([(1, 17), (0, 5), (2, 17)], start=1):
        eng.topk(0, mode, subs[:nq], 4)
        _, launches, by, fl = eng.kernel_stats(TOPK_CLASS)
        assert launches == calls
    assert fl == 2.0 * R * (1000 * 17 + 40 * 5 + 6 * 17) and by > 0
    # a model without factors cannot be asked
    Z = cp_Z(shape, R, empty(pkg, shape))
    pkg.build_model(eng, Z)
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.topk(0, 1, subs, 4)
    assert ei.value.code == capi.ERR_INVALID


@pytest.mark.parametrize('sparse', [False, True])
def test_parafac2_block_is_refused(pkg, eng, sparse):
    rng = np.random.default_rng(13)
    Z, A, B, Cm = par2_block(pkg, eng, rng, sparse)
    with pytest.raises(pkg.UnsupportedOnDevice) as ei:
        eng.topk(0, 0, np.zeros((3, 3), dtype=np.int64), 4)
    assert ei.value.code == capi.ERR_UNSUPPORTED and 'PARAFAC2' in str(ei.value)


def test_multi_device_context_is_refused(pkg):
    rng = np.random.default_rng(14)
    shape, R = (12, 10, 8), 3
    Z = cp_Z(shape, R, empty(pkg, shape))
    with pkg.Engine([0, 0]) as e:
        pkg.build_model(e, Z)
        pkg.upload_state(e, Z, {'fac': [rng.random((s, R)) for s in shape]})
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.topk(0, 0, queries(rng, shape, 5), 3)
