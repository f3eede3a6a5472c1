"""GPU: the place of held-out entries along one mode (aoadmm_resident_rank_of / _w; csrc/rank_of.hip, DESIGN.md section
9.7).  The models hold no data (an empty sptensor) unless a test is about the kind of block; the reference is numpy
(tests/rank_of_ref.py): fp64 scores, then the number of candidates before the target in lexsort((row, -score))."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from helpers import cp_model, options
from rank_of_ref import count_plan, ref_rank, weights, well_separated
from test_gpu_heldout import par2_block
from test_gpu_sparse_observed import NN
from test_gpu_sparse_sharded import cp_Z, empty, on_ranks
from test_gpu_sparse_weighted import weighted_alg
from test_gpu_topk import dataless, int_factors, queries
from test_rank_of_host import REAL, real_case

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')
RANK_CLASS = 13        # counted with the top-k completions
CHUNK = 1024           # listed rows per workgroup of the exclusion pass (kRankExclChunk)


def same(got, want):
    return all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)) and len(got) == len(want) == 3


def random_lists(rng, I, nq, longest, targets=None):
    """Unsorted lists with repeats; every fourth query has none; with targets, every other list holds its target."""
    lists = []
    for q in range(nq):
        if q % 4 == 3:
            lists.append(np.zeros(0, dtype=np.int64))
            continue
        rows = rng.integers(0, I, int(rng.integers(1, longest + 1)))
        rows = np.concatenate([rows, rows[:3]])
        if targets is not None and q % 2 == 0:
            rows = np.concatenate([rows, [targets[q], targets[q]]])
        lists.append(rows[rng.permutation(len(rows))].astype(np.int64))
    off = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    return (off, np.concatenate(lists)), lists


# ---- 1. exact --------------------------------------------------------------------------------------------------------
PAIRS = [(N, mode) for N in (2, 3, 4) for mode in range(N)]                       # 9: the free mode in every position
RS = [1, 3, 4, 5, 16, 17, 20, 33, 64]
IS = [1, 15, 16, 17, 255, 256, 257, 1000, 5003]
NQS = [1, 15, 16, 17, 40]
# 40 combinations; the strides are coprime to the lengths of the lists, so every value of every list occurs, and the
# shift per round of nine pairs every rank with several lengths
EXACT = [(PAIRS[t % 9] + (RS[(2 * t + t // 9) % 9], IS[(4 * t + 1 + 2 * (t // 9)) % 9], NQS[t % 5])) for t in range(40)]


def test_the_exact_cases_touch_every_value():
    assert len(set(EXACT)) == 40
    for pos, values in [(slice(0, 2), PAIRS), (2, RS), (3, IS), (4, NQS)]:
        assert {c[pos] for c in EXACT} == set(values)


@pytest.mark.parametrize('N,mode,R,I,nq', EXACT)
def test_exact(pkg, eng, N, mode, R, I, nq):
    """Integer factors in [-3, 3]: every score is exact in any order and ties abound; rank, score and ncand equal
    numpy's.  The first queries' targets are row 0, row I - 1 and the first row of the last group of 16 rows."""
    rng = np.random.default_rng(hash((N, mode, R, I, nq)) % (2 ** 32))
    shape = [6, 5, 4, 3][:N]
    shape[mode] = I
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    subs = queries(rng, shape, nq)
    forced = [0, I - 1, (I - 1) - (I - 1) % 16]
    for q in range(min(nq, 3)):
        subs[q, mode] = forced[(q + R + I) % 3]
    got = eng.rank_of(0, mode, subs)
    assert got[0].shape == (nq,) and got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[2].dtype == np.int64
    assert same(got, ref_rank(U, mode, subs))
    assert (got[2] == I).all() and (got[0] >= 0).all()


@pytest.mark.parametrize('KS', range(1, 17))
def test_exact_at_every_chain_length(pkg, eng, KS):
    """Every compiled-in chain length ceil(R / 4) = 1 .. 16 at R = 4 KS - 1: the last step carries a zeroed column and a
    clamped column address.  I = 273 and nq = 17 are the smallest that take every branch of the stream: two tiles per
    workgroup, the second ragged, and two slabs of 144 and 129 rows, which is more than two turns of the ring of four
    steps and a last step that holds one live row.  The first targets as in test_exact."""
    mode, R, I, nq = 1, 4 * KS - 1, 273, 17                    # N = 3
    qt, qtiles, slabs, slab_rows = count_plan(I, nq)
    assert (qt, qtiles, slabs, slab_rows, I - slab_rows) == (2, 1, 2, 144, 129)
    rng = np.random.default_rng(2000 + KS)
    shape = [6, I, 4]
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    subs = queries(rng, shape, nq)
    subs[:3, mode] = [0, I - 1, (I - 1) - (I - 1) % 16]
    got = eng.rank_of(0, mode, subs)
    assert same(got, ref_rank(U, mode, subs))
    assert (got[2] == I).all() and (got[0] >= 0).all()


# ---- 2. slabs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nq', [3, 40])
def test_targets_on_the_slab_cuts(pkg, eng, nq):
    """I = 70 001: scores that ascend, then descend, along the rows; the rank is I - 1 - t, then t.  Targets on the first
    and the last row of a slab of the counting pass, of the first and of the last slab."""
    rng = np.random.default_rng(5)
    I, R = 70001, 20
    shape = (4, I, 3)
    qt, qtiles, slabs, slab_rows = count_plan(I, nq)
    assert slabs > 1 and (slabs - 1) * slab_rows < I
    U = int_factors(rng, shape, R)
    e0 = np.zeros(R)
    e0[0] = 1.0
    U[0][:] = e0
    U[2][:] = e0
    U[1][:] = 0.0
    subs = queries(rng, shape, nq)
    cuts = [0, slab_rows - 1, slab_rows, 2 * slab_rows - 1, (slabs - 1) * slab_rows - 1, (slabs - 1) * slab_rows, I - 1,
            (slabs // 2) * slab_rows, (slabs // 2) * slab_rows - 1]
    if nq == 3:
        subs[:, 1] = [slab_rows - 1, slab_rows, (slabs - 1) * slab_rows]
    else:
        subs[:2 * len(cuts), 1] = cuts + cuts                  # both tiles of a workgroup; the other targets are random
    t = subs[:, 1]
    for column, want in ((np.arange(I, dtype=np.float64), I - 1 - t), (np.arange(I, dtype=np.float64)[::-1].copy(), t)):
        U[1][:, 0] = column
        dataless(pkg, eng, U)
        rank, score, ncand = eng.rank_of(0, 1, subs)
        assert np.array_equal(rank, want) and np.array_equal(score, column[t]) and (ncand == I).all()
        # every row but the target and its two neighbours excluded: one list longer than a chunk of the exclusion pass
        q = nq - 1
        keep = np.array([max(t[q] - 1, 0), t[q], min(t[q] + 1, I - 1)])
        rows = np.setdiff1d(np.arange(I), keep)
        off = np.zeros(nq + 1, dtype=np.int64)
        off[q + 1:] = len(rows)
        assert len(rows) > CHUNK
        got = eng.rank_of(0, 1, subs, exclude=(off, rows))
        assert same(got, ref_rank(U, 1, subs, (off, rows)))
        assert got[2][q] == len(np.unique(keep)) and got[0][q] <= 1


# ---- 3. NaN and infinities ----------------------------------------------------------------------------------------------
def test_nan_infinities_and_ties(pkg, eng):
    rng = np.random.default_rng(3)
    U = int_factors(rng, (300, 5), 4)
    U[0][7, 1] = np.nan                                        # row 7's score is NaN wherever w(1) is used
    U[0][9, 0] = np.inf
    U[0][11, 0] = -np.inf
    U[0][20] = U[0][150]                                       # the target's score on both sides of row 150
    U[0][280] = U[0][150]
    U[1][:, :2] = np.abs(U[1][:, :2]) + 1.0                   # w(0), w(1) > 0: +inf first, -inf last, NaN nowhere else
    dataless(pkg, eng, U)
    subs = queries(rng, (300, 5), 17)
    subs[:6, 0] = [7, 9, 11, 150, 20, 280]
    got = eng.rank_of(0, 0, subs)
    rank, score, ncand = got
    assert same(got, ref_rank(U, 0, subs))
    assert rank[0] == -1 and np.isnan(score[0]) and (ncand == 299).all()   # the NaN target: no rank, ncand still right
    assert rank[1] == 0 and score[1] == np.inf and rank[2] == 298 and score[2] == -np.inf
    # the three rows under one query's weights: consecutive places in row order
    three = np.repeat(subs[3:4], 3, axis=0)
    three[:, 0] = [20, 150, 280]
    r3, s3, _ = eng.rank_of(0, 0, three)
    assert s3[0] == s3[1] == s3[2] and r3[0] < r3[1] < r3[2]
    # the NaN row listed: it was no candidate, nothing is subtracted; the NaN target listed: still -1
    ex = (np.arange(18, dtype=np.int64), np.full(17, 7, dtype=np.int64))
    assert same(eng.rank_of(0, 0, subs, exclude=ex), got)


# ---- 4. exclusions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('I,R', [(1000, 5), (5003, 20), (257, 3)])
def test_exclusions(pkg, eng, I, R):
    rng = np.random.default_rng(I + R)
    shape = (6, I, 5)
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    nq = 40
    subs = queries(rng, shape, nq)
    t = subs[:, 1]
    ex, lists = random_lists(rng, I, nq, 200, targets=t)
    plain = eng.rank_of(0, 1, subs)
    got = eng.rank_of(0, 1, subs, exclude=ex)
    assert same(got, ref_rank(U, 1, subs, ex))
    for q in range(nq):
        others = np.setdiff1d(lists[q], [t[q]])
        assert got[2][q] == I - len(others) and got[1][q] == plain[1][q] and got[0][q] <= plain[0][q]
    above = [q for q in range(nq) if (lists[q] < t[q]).any()]
    below = [q for q in range(nq) if (lists[q] > t[q]).any()]
    assert above and below
    # a list longer than one chunk of the exclusion pass (with repeats), and every other row excluded
    long_rows = rng.integers(0, I, 3 * CHUNK + 7)
    everything = rng.permutation(I)
    off = np.zeros(nq + 1, dtype=np.int64)
    off[2:] = len(long_rows)
    off[6:] += I
    got = eng.rank_of(0, 1, subs, exclude=(off, np.concatenate([long_rows, everything])))
    assert same(got, ref_rank(U, 1, subs, (off, np.concatenate([long_rows, everything]))))
    assert got[0][5] == 0 and got[2][5] == 1                   # the target alone is left
    if I > CHUNK:
        assert len(np.unique(long_rows)) > CHUNK
    # refusals: an excluded row out of range, offsets that do not start at 0 or that decrease
    for bad in (I, -1):
        rows = ex[1].copy()
        rows[len(rows) // 2] = bad
        with pytest.raises(pkg.AoadmmError) as ei:
            eng.rank_of(0, 1, subs, exclude=(ex[0], rows))
        assert ei.value.code == capi.ERR_INVALID
    o = ex[0]
    for bad_off in (o + 1, np.concatenate([o[:5], [o[4] - 1], o[6:]])):
        with pytest.raises(pkg.AoadmmError) as ei:
            eng.rank_of(0, 1, subs, exclude=(bad_off, np.concatenate([ex[1], [0]])[:bad_off[-1]]))
        assert ei.value.code == capi.ERR_INVALID


# ---- 5. agreement with top-k: the same bits ----------------------------------------------------------------------------------
@pytest.mark.parametrize('I,R,N,nq,excluded', [c + (False,) for c in REAL] + [REAL[0] + (True,)])
def test_agreement_with_topk(pkg, eng, I, R, N, nq, excluded):
    """Real-valued factors.  For every query whose target stands among the first 64 and is not excluded, top-k's answer
    holds the target at position `rank` with the bits of `score`."""
    U, mode, subs, ex = real_case(I, R, N, nq, excluded)
    dataless(pkg, eng, U)
    rank, score, ncand = eng.rank_of(0, mode, subs, exclude=ex)
    idx, val = eng.topk(0, mode, subs, 64, exclude=ex)
    checked = 0
    for q in range(nq):
        t = subs[q, mode]
        if ex is not None and t in ex[1][ex[0][q]:ex[0][q + 1]]:
            continue
        if 0 <= rank[q] < 64:
            assert idx[q, rank[q]] == t and val[q, rank[q]].tobytes() == score[q].tobytes(), q
            checked += 1
        else:
            assert t not in idx[q]
    assert 2 * checked >= nq, checked


# ---- 6. real-valued against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('I,R,N,nq,excluded', [c + (False,) for c in REAL] + [REAL[0] + (True,)])
def test_real_valued(pkg, eng, I, R, N, nq, excluded):
    """No row's score lies within twice the tolerance 1e-12 sum_r prod_n |F_n| of a target's (asserted on the numpy side;
    tests/test_rank_of_host.py holds it for these seeds without a device): rank and ncand equal numpy's, score within
    the tolerance."""
    U, mode, subs, ex = real_case(I, R, N, nq, excluded)
    worst, tol = well_separated(U, mode, subs, ex)
    assert worst > 1.0, worst
    dataless(pkg, eng, U)
    rank, score, ncand = eng.rank_of(0, mode, subs, exclude=ex)
    rrank, rscore, rncand = ref_rank(U, mode, subs, ex)
    print('smallest gap: %.3g times twice the tolerance; worst score error %.3g of the tolerance'
          % (worst, float(np.max(np.abs(score - rscore) / tol))))
    assert np.array_equal(rank, rrank) and np.array_equal(ncand, rncand)
    assert np.all(np.abs(score - rscore) <= tol)


# ---- 7. the bits depend on the inputs only -------------------------------------------------------------------------------
def test_bits_depend_on_the_inputs_only(pkg, eng):
    rng = np.random.default_rng(7)
    shape, R = (5003, 30, 20), 20
    U = [rng.standard_normal((s, R)) for s in shape]
    dataless(pkg, eng, U)
    subs = queries(rng, shape, 40)
    ex, _ = random_lists(rng, shape[0], 40, 50)
    for exclude in (None, ex):
        first = eng.rank_of(0, 0, subs, exclude=exclude)
        assert same(eng.rank_of(0, 0, subs, exclude=exclude), first)
        for q in (0, 17, 39):                                  # asked alone: another tile shape, another slab cut
            one = None if exclude is None else (exclude[0][q:q + 2] - exclude[0][q], exclude[1][exclude[0][q]:exclude[0][q + 1]])
            assert same(eng.rank_of(0, 0, subs[q:q + 1], exclude=one), [x[q:q + 1] for x in first])
        part = None if exclude is None else (exclude[0][3:21] - exclude[0][3], exclude[1][exclude[0][3]:exclude[0][20]])
        assert same(eng.rank_of(0, 0, subs[3:20], exclude=part), [x[3:20] for x in first])


def test_bits_after_a_solve_and_after_an_upload(pkg, eng):
    """After a solve the row-major factor copies are current and are gathered from; the same factors uploaded are
    gathered column-major.  Same bits."""
    rng = np.random.default_rng(8)
    shape, R = (300, 40, 30), 4
    Z, io, _ = cp_model(shape, R, rng, [NN] * 3)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    subs = queries(rng, shape, 33)
    for mode in range(3):
        _, Fac, _, _ = pkg.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=3), init=copy.deepcopy(G), engine=eng)
        after_solve = eng.rank_of(0, mode, subs)
        eng.model_at(0, subs)                                  # the held-out pass reports which layout the factors offer
        assert eng.heldout_info(0)['row_major'] == 1
        pkg.upload_state(eng, Z, {'fac': Fac['fac']})
        after_upload = eng.rank_of(0, mode, subs)
        eng.model_at(0, subs)
        assert eng.heldout_info(0)['row_major'] == 0
        assert same(after_solve, after_upload)
        assert (after_upload[0] >= 0).all() and (after_upload[2] == shape[mode]).all()


def test_every_kind_of_block(pkg, eng):
    rng = np.random.default_rng(9)
    shape, R = (300, 12, 10), 5
    U = [rng.standard_normal((s, R)) for s in shape]
    subs = queries(rng, shape, 40)
    dataless(pkg, eng, U)
    want = [eng.rank_of(0, mode, subs) for mode in range(3)]
    keep = rng.random(shape) < 0.2
    X = rng.standard_normal(shape)
    S = pkg.sptensor(np.argwhere(keep), X[keep], shape)

    def check(e, mode, rows=slice(None)):
        assert same(e.rank_of(0, mode, subs[rows]), [x[rows] for x in want[mode]])

    for obj, kw in [(X, {}), (S, {})]:
        Z = cp_Z(shape, R, obj)
        pkg.build_model(eng, Z, **kw)
        pkg.upload_state(eng, Z, {'fac': U})
        for mode in range(3):
            check(eng, mode)

    def rank_fn(e, r):                                         # sharded sparse, every rank asks its own queries
        Z = cp_Z(shape, R, S)
        pkg.build_model(e, Z, sparse_sharding=True)
        pkg.upload_state(e, Z, {'fac': U})
        for mode in range(3):
            check(e, mode, slice(0, 23) if r == 0 else slice(23, 40))
        return True

    assert on_ranks(pkg, 2, rank_fn) == [True, True]


# ---- 8. the weights given ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('I,R,N,nq', [(5003, 20, 3, 40), (257, 33, 4, 17), (1000, 5, 2, 1)])
def test_rank_of_w_is_rank_of(pkg, eng, I, R, N, nq):
    """W formed in numpy in mode order (IEEE products: the bits of topk_weights_k): the triple equals rank_of's."""
    rng = np.random.default_rng(I)
    shape = [7, 6, 5, 4][:N]
    shape[N - 1] = I
    U = [rng.standard_normal((s, R)) for s in shape]
    dataless(pkg, eng, U)
    subs = queries(rng, shape, nq)
    W = weights(U, N - 1, subs)
    ex, _ = random_lists(rng, I, nq, 40, targets=subs[:, N - 1])
    for exclude in (None, ex):
        assert same(eng.rank_of_w(0, N - 1, W, subs[:, N - 1], exclude=exclude), eng.rank_of(0, N - 1, subs, exclude=exclude))
    for bad in (I, -1):                                        # a target out of range
        t = subs[:, N - 1].copy()
        t[nq // 2] = bad
        with pytest.raises(pkg.AoadmmError) as ei:
            eng.rank_of_w(0, N - 1, W, t)
        assert ei.value.code == capi.ERR_INVALID
    with pytest.raises(ValueError):
        eng.rank_of_w(0, N - 1, W[:, :R - 1] if R > 1 else np.ones((nq, 2)), subs[:, N - 1])


# ---- 9. end to end -------------------------------------------------------------------------------------------------------
def planted_feedback(pkg, rng):
    """60 users x 40 items in four groups of 15 x 10: a user stores an item of its own group with probability 0.7, any
    other with probability 0.03; every stored value is 1.  One stored entry per user is held out."""
    group_u, group_i = np.arange(60) // 15, np.arange(40) // 10
    p = np.where(group_u[:, None] == group_i[None, :], 0.7, 0.03)
    X = (rng.random((60, 40)) < p).astype(np.float64)
    X[np.arange(60), group_u * 10] = 1.0                       # nobody without a stored item
    X[np.arange(60), group_u * 10 + 1] = 1.0                   # ... or with a single one
    train_subs, held_subs = [], []
    for u in range(60):
        items = np.flatnonzero(X[u])
        row = pkg.sptensor(np.stack([np.full(len(items), u), items], axis=1), np.ones(len(items)), (60, 40))
        tr, ho = row.split(1.0 / len(items), rng)              # round(frac nnz) = 1 entry
        assert ho.nnz == 1 and tr.nnz == len(items) - 1
        train_subs.append(tr.subs)
        held_subs.append(ho.subs)
    train_subs = np.concatenate(train_subs)
    return pkg.sptensor(train_subs, np.ones(len(train_subs)), (60, 40)), np.concatenate(held_subs).astype(np.int64)


def test_end_to_end_on_implicit_feedback(pkg, eng):
    """Fitted with entry weights 1 and the unstored-entry weight 0.1; the held-out items are ranked among the items the
    training part does not store.  The device's metrics equal numpy's on the returned factors, and hit@10 lies above
    chance, mean(min(10, ncand) / ncand)."""
    rng = np.random.default_rng(21)
    train, held = planted_feedback(pkg, rng)
    R = 4
    Z, io, _ = cp_model((60, 40), R, rng, [NN, NN], noise=0.0)
    dense = np.zeros((60, 40))
    dense[tuple(train.subs.T)] = train.vals
    G = OA.init_coupled_AOADMM_CMTF({**dict(Z, object=[dense]), 'prox_operators': None}, io, rng=np.random.default_rng(7))
    Zs = dict(Z, object=[train])
    alg = weighted_alg(options(MaxOuterIters=40), 1, 0, np.ones(train.nnz), 0.1)
    _, Fac, _, _ = pkg.cmtf_AOADMM(Zs, alg_options=alg, init=copy.deepcopy(G), engine=eng)
    F = [np.asarray(f) for f in Fac['fac']]
    ex = train.fiber_lists(1, held)
    rank, score, ncand = eng.rank_of(0, 1, held, exclude=ex)
    rrank, rscore, rncand = ref_rank(F, 1, held, ex)
    got, want = pkg.ranking_metrics(rank, ncand), pkg.ranking_metrics(rrank, rncand)
    assert got == want and got['n'] == 60
    assert np.array_equal(ncand, 40 - np.diff(ex[0])) and np.array_equal(ncand, rncand)
    chance = float(np.mean(np.minimum(10, ncand) / ncand))
    print('hit@10 %.4f (chance %.4f), ndcg@10 %.4f, mrr %.4f, auc %.4f' % (got['hit@10'], chance, got['ndcg@10'], got['mrr'], got['auc']))
    assert got['hit@10'] > chance
    # the whole tensor's stored rows as the lists: the held-out target is listed and still ranked
    whole = pkg.sptensor(np.concatenate([train.subs, held]), np.ones(train.nnz + 60), (60, 40))
    assert same(eng.rank_of(0, 1, held, exclude=whole.fiber_lists(1, held)), (rank, score, ncand))


# ---- 10. refusals and accounting -----------------------------------------------------------------------------------------
def raw_rank(e, p, mode, subs, off=None, ex=None, null=()):
    """The C entry itself with pre-filled outputs: (status, rank, score, ncand)."""
    subs = np.asfortranarray(np.asarray(subs, dtype=np.int64))
    nq = subs.shape[0]
    rank = np.full(nq, 77, dtype=np.int64)
    score = np.full(nq, 0.5)
    ncand = np.full(nq, 55, dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(i64p)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.int64) for a in (off, ex)]
    st = e.lib.aoadmm_resident_rank_of(e.h, p, mode, nq, subs.ctypes.data_as(i64p),
                                       None if keep[0] is None else keep[0].ctypes.data_as(i64p),
                                       None if keep[1] is None else keep[1].ctypes.data_as(i64p),
                                       None if 'rank' in null else rank.ctypes.data_as(i64p),
                                       None if 'score' in null else capi.dptr(score),
                                       None if 'ncand' in null else ncand.ctypes.data_as(i64p))
    return st, rank, score, ncand


def test_refusals_and_accounting(pkg, eng):
    rng = np.random.default_rng(12)
    shape, R = (40, 1000, 6), 5
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    subs = queries(rng, shape, 17)
    row = np.arange(17)[:, None]
    off = np.arange(18, dtype=np.int64)
    rows = rng.integers(0, 1000, 17)
    bad_rows = rows.copy()
    bad_rows[4] = 1000
    cases = [dict(p=1), dict(p=-1), dict(mode=3), dict(mode=-1),
             dict(subs=np.where(row == 9, [40, 0, 0], subs)), dict(subs=np.where(row == 2, [0, 0, -1], subs)),
             dict(subs=np.where(row == 5, [0, 1000, 0], subs)), dict(subs=np.where(row == 16, [0, -1, 0], subs)),   # the targets
             dict(off=off, ex=bad_rows), dict(off=off + 1, ex=np.concatenate([rows, [0]])),
             dict(off=np.concatenate([off[:5], [3], off[6:]]), ex=rows), dict(null=('rank',)), dict(null=('score',))]
    for kw in cases:
        args = dict(p=0, mode=1, subs=subs)
        args.update(kw)
        st, rank, score, ncand = raw_rank(eng, **args)
        assert st == capi.ERR_INVALID, kw
        assert (rank == 77).all() and (score == 0.5).all() and (ncand == 55).all(), kw   # untouched
    st, rank, score, ncand = raw_rank(eng, 0, 1, subs, null=('ncand',))       # ncand may be left out
    assert st == capi.OK and np.array_equal(rank, ref_rank(U, 1, subs)[0]) and (ncand == 55).all()
    # nq = 0 is a no-op, nq < 0 is refused
    got = eng.rank_of(0, 1, np.zeros((0, 3), dtype=np.int64))
    assert all(x.shape == (0,) for x in got)
    got = eng.rank_of_w(0, 1, np.zeros((0, R)), np.zeros(0, dtype=np.int64))
    assert all(x.shape == (0,) for x in got)
    assert eng.lib.aoadmm_resident_rank_of(eng.h, 0, 1, 0, None, None, None, None, None, None) == capi.OK
    assert eng.lib.aoadmm_resident_rank_of(eng.h, 0, 1, -1, None, None, None, None, None, None) == capi.ERR_INVALID
    assert eng.lib.aoadmm_resident_rank_of_w(eng.h, 0, 1, 2 ** 31, None, None, None, None, None, None, None) == capi.ERR_INVALID
    # accounting: class 13, one launch per call
    eng.kernel_stats(RANK_CLASS, reset=True)
    ex = (np.array([0, 3, 3, 8, 8, 8, 9], dtype=np.int64), np.array([5, 5, 7, 1, 2, 3, 2, 1, 999]))   # 2 + 3 + 1 distinct rows
    want = 0.0
    for calls, (mode, nq, exclude) in enumerate([(1, 17, None), (0, 5, None), (2, 17, None), (1, 6, ex)], start=1):
        if calls == 3:
            eng.rank_of_w(0, mode, weights(U, mode, subs[:nq]), subs[:nq, mode])
        else:
            eng.rank_of(0, mode, subs[:nq], exclude=exclude)
        _, launches, by, fl = eng.kernel_stats(RANK_CLASS)
        assert launches == calls
        want += 2.0 * shape[mode] * nq * R + 2.0 * R * ((6 if exclude is not None else 0) + nq)
        assert fl == want and by > 0
    # a model without factors cannot be asked
    Z = cp_Z(shape, R, empty(pkg, shape))
    pkg.build_model(eng, Z)
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.rank_of(0, 1, subs)
    assert ei.value.code == capi.ERR_INVALID


@pytest.mark.parametrize('sparse', [False, True])
def test_parafac2_block_is_refused(pkg, eng, sparse):
    rng = np.random.default_rng(13)
    par2_block(pkg, eng, rng, sparse)
    with pytest.raises(pkg.UnsupportedOnDevice) as ei:
        eng.rank_of(0, 0, np.zeros((3, 3), dtype=np.int64))
    assert ei.value.code == capi.ERR_UNSUPPORTED and 'PARAFAC2' in str(ei.value)
    with pytest.raises(pkg.UnsupportedOnDevice):
        eng.rank_of_w(0, 0, np.ones((3, 3)), np.zeros(3, dtype=np.int64))


def test_multi_device_context_is_refused(pkg):
    rng = np.random.default_rng(14)
    shape, R = (12, 10, 8), 3
    Z = cp_Z(shape, R, empty(pkg, shape))
    with pkg.Engine([0, 0]) as e:
        pkg.build_model(e, Z)
        pkg.upload_state(e, Z, {'fac': [rng.random((s, R)) for s in shape]})
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.rank_of(0, 0, queries(rng, shape, 5))
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.rank_of_w(0, 0, np.ones((5, R)), np.zeros(5, dtype=np.int64))
