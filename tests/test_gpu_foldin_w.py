"""GPU: new rows of a CP block under entry weights and a weight for the unlisted cells (aoadmm_resident_fold_in_w;
csrc/foldin_dev.h, csrc/foldin_w.hip).  The models hold no data (an empty sptensor) unless a test
is about the kind of block; the reference is tests/foldin_w_ref.py, in fp64 and in longdouble.

Worst device error of test_rows (max |u_dev - u_longdouble| / max |u|) is printed per case; DESIGN.md section 9.6 quotes it.

A weight that is not finite is refused with the whole call (test_refusals_and_accounting), so what reaches its own query
only is shown with a NaN value under weights (test_bits_depend_on_the_query_alone)."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import foldin_ref as FR
import foldin_w_ref as FW
from oracle import aoadmm as OA
from helpers import cp_model, options
from test_gpu_foldin import CHUNK, FOLDIN_CLASS, same_bits
from test_gpu_heldout import par2_block
from test_gpu_sparse_observed import NN
from test_gpu_sparse_sharded import cp_Z, empty, on_ranks
from test_gpu_sparse_weighted import known_answer_model, weighted_alg
from test_gpu_topk import dataless, int_factors

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')


def raw_w(e, p, mode, nq, subs, vals, wts, alpha, opt, R, fill=False):
    """The C entry itself.  fill=False: (rows, info, iters, gram, rhs) of a call that must succeed; fill=True: (status,
    every pre-filled output untouched)."""
    subs = np.asfortranarray(np.asarray(subs, dtype=np.int64))
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    w = None if wts is None else np.ascontiguousarray(wts, dtype=np.float64)
    n = int(nq) if 0 < int(nq) <= 1000 else 1
    rows, rhs = np.full((n, R), 0.5, order='F'), np.full((n, R), 0.5, order='F')
    gram = np.full((n, R, R), 0.5)
    info, iters = np.full(n, 77, dtype=np.int32), np.full(n, 77, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    st = e.lib.aoadmm_resident_fold_in_w(
        e.h, p, mode, nq, vals.shape[0], subs.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(vals), capi.dptr(w), float(alpha),
        None if opt is None else C.byref(opt), capi.dptr(rows), info.ctypes.data_as(ip), iters.ctypes.data_as(ip), capi.dptr(gram),
        capi.dptr(rhs))
    if fill:
        untouched = (rows == 0.5).all() and (rhs == 0.5).all() and (gram == 0.5).all() and (info == 77).all() and (iters == 77).all()
        return st, untouched
    assert st == capi.OK
    return rows, info, iters, gram, rhs


def distinct_list(rng, shape, mode, counts, shuffle=True):
    """counts[q] observations of query q at distinct cells of the other modes (a cell listed twice would be taken off
    alpha H twice); standard normal values."""
    other = [m for m in range(len(shape)) if m != mode]
    dims = [shape[m] for m in other]
    parts = []
    for q, n in enumerate(counts):
        lin = rng.choice(int(np.prod(dims)), int(n), replace=False)
        s = np.zeros((int(n), len(shape)), dtype=np.int64)
        for m, col in zip(other, np.unravel_index(lin, dims)):
            s[:, m] = col
        s[:, mode] = q
        parts.append(s)
    subs = np.concatenate(parts)
    vals = rng.standard_normal(len(subs))
    if shuffle:
        perm = rng.permutation(len(subs))
        subs, vals = subs[perm], vals[perm]
    return np.ascontiguousarray(subs), vals


# ---- 5. exact normal equations -------------------------------------------------------------------------------------------
PAIRS = [(N, mode) for N in (2, 3, 4) for mode in range(N)]                       # 9: the new mode in every position
RS = [1, 3, 16, 17, 32, 33, 48, 49, 64]                                           # both ends of every rank class
COUNTS = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 2500]        # 2500: ten partials, more than the eight in flight
ALPHAS = [0.0, 0.125, 0.5, 1.0]
WEIGHTS = np.arange(9) / 8.0
NQS = [1, 2, 17, 40]
# 36 combinations: nine cases per alpha, in which every rank and every pair occurs once (the rank shifted by one against
# the pair from one alpha to the next); the count of query i of case t is COUNTS[(3 t + 7 i) % 10]: mixed inside one call
EXACT = [(PAIRS[t % 9] + (RS[(t + t // 9) % 9], NQS[t % 4], ALPHAS[t // 9], t)) for t in range(36)]


def exact_counts(nq, t):
    return [COUNTS[(3 * t + 7 * i) % 10] for i in range(nq)]


def exact_list(N, mode, nq, t):
    rng = np.random.default_rng(2000 + t)
    shape = [6, 5, 4, 3][:N]
    shape[mode] = 2                                            # the fitted rows of the new mode are not read
    subs, vals = FR.make_list(rng, shape, mode, exact_counts(nq, t), values='int')
    wts = rng.choice(WEIGHTS, len(vals))
    return rng, shape, subs, vals, wts


def test_the_exact_cases_touch_every_value():
    assert len({c[:5] for c in EXACT}) == 36
    for pos, values in [(slice(0, 2), PAIRS), (2, RS), (3, NQS), (4, ALPHAS)]:
        assert {c[pos] for c in EXACT} == set(values)
    assert {(c[2], c[4]) for c in EXACT} == {(R, a) for R in RS for a in ALPHAS}
    assert {n for _, _, _, nq, _, t in EXACT for n in exact_counts(nq, t)} == set(COUNTS)
    seen_w, seen_v = set(), set()
    for N, mode, R, nq, alpha, t in EXACT:
        _, _, _, vals, wts = exact_list(N, mode, nq, t)
        seen_w |= set(wts.tolist())
        seen_v |= set(vals.tolist())
    assert seen_w == set(WEIGHTS.tolist()) and seen_v == set(float(v) for v in range(-5, 6))


@pytest.mark.parametrize('N,mode,R,nq,alpha,t', EXACT)
def test_exact_normal_equations(pkg, eng, N, mode, R, nq, alpha, t):
    """Integer factors in [-3, 3], integer values in [-5, 5], weights k / 8 and alpha a multiple of 1 / 8: every product
    and every sum is exact in fp64 in any order; gram (alpha H included) and rhs equal numpy's, gram is symmetric."""
    rng, shape, subs, vals, wts = exact_list(N, mode, nq, t)
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    rows, info, iters, gram, rhs = eng.fold_in(0, mode, subs, vals, nq=nq, return_normal=True, weights=wts, unstored_weight=alpha)
    G, b = FW.normal(U, mode, subs, vals, wts, alpha, nq)
    assert gram.shape == (nq, R, R) and rhs.shape == (nq, R) and rows.shape == (nq, R)
    assert np.array_equal(gram, G) and np.array_equal(rhs, b)
    assert np.array_equal(gram, gram.transpose(0, 2, 1))
    assert not iters.any()


# ---- 9. empty queries ----------------------------------------------------------------------------------------------------
def test_empty_queries(pkg, eng):
    rng = np.random.default_rng(2)
    shape, R = (2, 30, 25), 5
    U = [rng.standard_normal((s, R)) for s in shape]
    dataless(pkg, eng, U)
    counts = [0, 3 * R, 0, CHUNK + 1, 0]
    subs, vals = distinct_list(rng, shape, 0, counts)
    wts = rng.random(len(vals))
    for nonneg in (False, True):
        rows, info, iters = eng.fold_in(0, 0, subs, vals, nq=5, ridge=0.0, nonneg=nonneg, weights=wts, unstored_weight=0.25)
        assert not info.any() and not rows[[0, 2, 4]].any() and np.isfinite(rows).all()     # G = alpha H, b = 0
        rows, info, iters = eng.fold_in(0, 0, subs, vals, nq=5, ridge=0.0, nonneg=nonneg, weights=wts, unstored_weight=0.0)
        assert list(info) == [1, 0, 1, 0, 1] and np.isnan(rows[[0, 2, 4]]).all()           # as without weights
    none = np.zeros((0, 3), dtype=np.int64)
    rows, info, iters, gram, rhs = eng.fold_in(0, 0, none, [], nq=3, unstored_weight=1.0, return_normal=True)
    assert not rows.any() and not info.any() and not rhs.any()
    H = FW.hadamard_gram(U, 0)
    assert np.allclose(gram, H[None], rtol=0, atol=1e-13 * np.abs(H).max())
    rows, info, iters = eng.fold_in(0, 0, none, [], nq=3, weights=[])
    assert np.isnan(rows).all() and info.all()


# ---- 6. rows, real values ------------------------------------------------------------------------------------------------
NQ_ROWS = 5
ROW_ALPHAS = [0.0, 0.05, 1.0]


def real_case(R, N, kind, alpha):
    rng = np.random.default_rng(97 * R + N + int(1000 * alpha))
    shape = [2] + [4 * R + 11, 4 * R + 9, 4 * R + 10][:N - 1]   # at least 4 R rows, and 4 R + 8 distinct cells at N = 2
    U = [rng.standard_normal((s, R)) for s in shape]
    n = 4 * R + 8 if kind == 'full' else max(1, R // 2)
    ridge = 0.0 if kind == 'full' else 0.1
    subs, vals = distinct_list(rng, shape, 0, [n] * NQ_ROWS)
    return U, subs, vals, rng.random(len(vals)), ridge


def check_rows(got, ld, f64, what=''):
    """The bar rule of tests/test_gpu_foldin.py: per query, max |u_dev - u_longdouble| / max |u| <= max(1e-11, 10 floor_q)
    with floor_q the same distance for the fp64 numpy restatement."""
    worst = 0.0
    for q in range(got.shape[0]):
        scale = float(np.max(np.abs(ld[q])))
        if scale == 0.0:                                       # a row the constraint put at zero: zero it is
            assert not got[q].any()
            continue
        floor = float(np.max(np.abs(f64[q].astype(FR.LD) - ld[q]))) / scale
        err = float(np.max(np.abs(got[q].astype(FR.LD) - ld[q]))) / scale
        worst = max(worst, err)
        assert err <= max(1e-11, 10.0 * floor), (what, q, err, floor)
    return worst


@pytest.mark.parametrize('alpha', ROW_ALPHAS)
@pytest.mark.parametrize('kind', ['full', 'short'])
@pytest.mark.parametrize('R,N', [(R, 3) for R in RS] + [(33, 2), (64, 2), (5, 4), (64, 4)])
def test_rows(pkg, eng, R, N, kind, alpha):
    U, subs, vals, wts, ridge = real_case(R, N, kind, alpha)
    G, _ = FW.normal(U, 0, subs, vals, wts, alpha, NQ_ROWS)
    conds = [float(np.linalg.cond(G[q] + ridge * np.eye(R))) for q in range(NQ_ROWS)]
    assert max(conds) <= 1e6, conds
    dataless(pkg, eng, U)
    report = []
    for name, kw in [('plain', {}), ('nonneg/1', dict(nonneg=True, max_inner=1)), ('nonneg/5', dict(nonneg=True, max_inner=5))]:
        rows, info, iters = eng.fold_in(0, 0, subs, vals, ridge=ridge, weights=wts, unstored_weight=alpha, **kw)
        ld, info_ld, _ = FW.fold_in(U, 0, subs, vals, wts, alpha, NQ_ROWS, ridge=ridge, dtype=FR.LD, **kw)
        f64, _, _ = FW.fold_in(U, 0, subs, vals, wts, alpha, NQ_ROWS, ridge=ridge, **kw)
        assert not info.any() and not info_ld.any()
        assert (iters == kw.get('max_inner', 0)).all() and (not kw or (rows >= 0).all())
        report.append('%s %.3g' % (name, check_rows(rows, ld, f64, name)))
    print('R = %d, N = %d, %s, alpha = %g: cond <= %.3g; worst device error: %s' % (R, N, kind, alpha, max(conds), ', '.join(report)))


# ---- 7. reductions to what exists ----------------------------------------------------------------------------------------
def mixed_counts(R, nq):
    return [[4 * R + 8, CHUNK + 5, 3 * R, 2 * CHUNK + 3, R + 1][q % 5] for q in range(nq)]   # fused and split queries


@pytest.mark.parametrize('values', ['int', 'normal'])
def test_without_weights_the_new_entry_is_the_old_one(pkg, eng, values):
    rng = np.random.default_rng(21)
    shape, R, nq = (2, 40, 35), 20, 12
    U = int_factors(rng, shape, R) if values == 'int' else [rng.standard_normal((s, R)) for s in shape]
    dataless(pkg, eng, U)
    subs, vals = FR.make_list(rng, shape, 0, mixed_counts(R, nq), values=values)
    for kw, opt in [(dict(ridge=0.5), capi.FoldinOptions(0.5, 0, 5, 0.0, 0.0)),
                    (dict(ridge=0.5, nonneg=True, max_inner=7, tol=(1e-4, 1e-4)), capi.FoldinOptions(0.5, 1, 7, 1e-4, 1e-4))]:
        old = eng.fold_in(0, 0, subs, vals, nq=nq, return_normal=True, **kw)
        assert same_bits(old, raw_w(eng, 0, 0, nq, subs, vals, None, 0.0, opt, R))              # wts = NULL, alpha = 0
        assert same_bits(old, raw_w(eng, 0, 0, nq, subs, vals, np.ones(len(vals)), 0.0, opt, R))
        assert same_bits(old, eng.fold_in(0, 0, subs, vals, nq=nq, return_normal=True, weights=np.ones(len(vals)), **kw))


def test_zero_weights_drop_their_observations(pkg, eng):
    """Integer data only: a weight of zero leaves a zero operand in the chain where the sub-list has no step at all, so
    the order of summation inside a chunk differs."""
    rng = np.random.default_rng(22)
    shape, R, nq = (2, 40, 35), 20, 12
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    subs, vals = FR.make_list(rng, shape, 0, mixed_counts(R, nq), values='int')
    w = (rng.random(len(vals)) < 0.7).astype(np.float64)
    got = eng.fold_in(0, 0, subs, vals, nq=nq, ridge=0.5, return_normal=True, weights=w, unstored_weight=0.0)
    want = eng.fold_in(0, 0, subs[w == 1], vals[w == 1], nq=nq, ridge=0.5, return_normal=True)
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    assert same_bits(got, want)


# ---- 8. bits -------------------------------------------------------------------------------------------------------------
def test_bits_depend_on_the_query_alone(pkg, eng):
    rng = np.random.default_rng(7)
    shape, R, nq = (2, 90, 85), 20, 40
    U = [rng.standard_normal((s, R)) for s in shape]
    dataless(pkg, eng, U)
    subs, vals = distinct_list(rng, shape, 0, mixed_counts(R, nq))
    wts = rng.random(len(vals))
    kw = dict(ridge=0.01, nonneg=True, max_inner=7, tol=(1e-4, 1e-4), unstored_weight=0.05)
    first = eng.fold_in(0, 0, subs, vals, weights=wts, return_normal=True, **kw)
    assert same_bits(first, eng.fold_in(0, 0, subs, vals, weights=wts, return_normal=True, **kw))
    assert same_bits(first[:3], eng.fold_in(0, 0, subs, vals, weights=wts, **kw))   # fused: nothing of it written to HBM
    for q in (0, 1, 3, 17, 39):                                # asked alone: another launch shape
        sel = subs[:, 0] == q
        s1 = subs[sel].copy()
        s1[:, 0] = 0
        alone = eng.fold_in(0, 0, s1, vals[sel], weights=wts[sel], return_normal=True, **kw)
        assert same_bits([x[q] for x in first], [x[0] for x in alone]), q
    # the queries renumbered and the list reordered by query, each query's own order kept
    perm = rng.permutation(nq)                                 # old query q becomes perm[q]
    order = np.argsort(perm[subs[:, 0]] * 3 % nq, kind='stable')
    s2 = subs[order].copy()
    s2[:, 0] = perm[s2[:, 0]]
    moved = eng.fold_in(0, 0, s2, vals[order], weights=wts[order], return_normal=True, **kw)
    assert same_bits(first, [x[perm] for x in moved])
    # a NaN value reaches its own query only (a NaN weight is refused with the call)
    v3 = vals.copy()
    v3[np.flatnonzero(subs[:, 0] == 3)[5]] = np.nan
    v3[np.flatnonzero(subs[:, 0] == 4)[0]] = np.nan
    hurt = eng.fold_in(0, 0, subs, v3, weights=wts, return_normal=True, **kw)
    others = np.setdiff1d(np.arange(nq), [3, 4])
    assert same_bits([x[others] for x in first], [x[others] for x in hurt])
    assert np.isnan(hurt[4][3]).any() and np.isnan(hurt[4][4]).any()
    assert np.array_equal(first[3], hurt[3])                   # gram holds no value
    w3 = wts.copy()
    w3[7] = np.nan
    with pytest.raises(pkg.AoadmmError):
        eng.fold_in(0, 0, subs, vals, weights=w3, **kw)


def test_bits_after_a_solve_and_after_an_upload(pkg, eng):
    """After a solve the row-major factor copies are gathered from and H is summed from them; the same factors uploaded
    are read column-major.  H never comes from a Gram matrix the solve left."""
    rng = np.random.default_rng(8)
    shape, R = (300, 40, 30), 4
    Z, io, _ = cp_model(shape, R, rng, [NN] * 3)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    for mode in range(3):
        counts = [4 * R + 8, CHUNK + 9, 3, 2 * CHUNK + 1]
        subs, vals = distinct_list(rng, shape, mode, counts)
        wts = rng.random(len(vals))
        kw = dict(ridge=1e-3, return_normal=True, weights=wts, unstored_weight=0.05)
        _, Fac, _, _ = pkg.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=3), init=copy.deepcopy(G), engine=eng)
        after_solve = eng.fold_in(0, mode, subs, vals, **kw)
        eng.model_at(0, np.zeros((1, 3), dtype=np.int64))
        assert eng.heldout_info(0)['row_major'] == 1
        pkg.upload_state(eng, Z, {'fac': Fac['fac']})
        after_upload = eng.fold_in(0, mode, subs, vals, **kw)
        eng.model_at(0, np.zeros((1, 3), dtype=np.int64))
        assert eng.heldout_info(0)['row_major'] == 0
        assert same_bits(after_solve, after_upload)
        Gn, bn = FW.normal([np.asarray(f) for f in Fac['fac']], mode, subs, vals, wts, 0.05, 4)
        assert np.allclose(after_upload[3], Gn, rtol=0, atol=1e-12 * np.abs(Gn).max())
        assert np.allclose(after_upload[4], bn, rtol=0, atol=1e-12 * np.abs(bn).max())


def test_every_kind_of_block(pkg, eng):
    rng = np.random.default_rng(9)
    shape, R = (300, 12, 10), 5
    U = [rng.standard_normal((s, R)) for s in shape]
    lists = []
    for mode in range(3):
        other = int(np.prod([s for m, s in enumerate(shape) if m != mode]))
        long = min(CHUNK + 3, other)
        subs, vals = distinct_list(rng, shape, mode, [4 * R + 8, long] * 4)
        lists.append((subs, vals, rng.random(len(vals))))
    dataless(pkg, eng, U)
    kw = dict(ridge=0.05, nonneg=True, return_normal=True, unstored_weight=0.1)
    want = [eng.fold_in(0, mode, lists[mode][0], lists[mode][1], weights=lists[mode][2], **kw) for mode in range(3)]
    keep = rng.random(shape) < 0.2
    X = rng.standard_normal(shape)
    S = pkg.sptensor(np.argwhere(keep), X[keep], shape)

    def same(e, mode, qs=None):
        subs, vals, wts = lists[mode]
        if qs is None:
            assert same_bits(e.fold_in(0, mode, subs, vals, weights=wts, **kw), want[mode])
            return
        sel = np.isin(subs[:, mode], qs)
        s1 = subs[sel].copy()
        s1[:, mode] -= qs[0]
        got = e.fold_in(0, mode, s1, vals[sel], nq=len(qs), weights=wts[sel], **kw)
        assert same_bits(got, [x[qs] for x in want[mode]])

    kinds = [(X, {}), (X, dict(precision='f16')), (S, {}), (S, dict(observed_only=1)),
             (S, dict(entry_weights=[rng.random(len(S.vals))], unstored_weight=0.3))]
    for obj, okw in kinds:
        Z = cp_Z(shape, R, obj)
        pkg.build_model(eng, Z, **okw)
        pkg.upload_state(eng, Z, {'fac': U})
        for mode in range(3):
            same(eng, mode)

    def rank_fn(e, r):                                         # sharded sparse, every rank asks its own queries
        Z = cp_Z(shape, R, S)
        pkg.build_model(e, Z, sparse_sharding=True)
        pkg.upload_state(e, Z, {'fac': U})
        for mode in range(3):
            same(e, mode, np.arange(0, 5) if r == 0 else np.arange(5, 8))
        return True

    assert on_ranks(pkg, 2, rank_fn) == [True, True]


# ---- 10. refusals and accounting -----------------------------------------------------------------------------------------
def test_refusals_and_accounting(pkg, eng):
    rng = np.random.default_rng(12)
    shape, R, nq = (40, 50, 6), 5, 17
    U = int_factors(rng, shape, R)
    dataless(pkg, eng, U)
    subs, vals = FR.make_list(rng, shape, 1, [3 * R] * nq)
    wts = rng.choice(WEIGHTS, len(vals))
    good = capi.FoldinOptions(0.5, 1, 5, 0.0, 0.0)
    st, untouched = raw_w(eng, 0, 1, nq, subs, vals, wts, 0.25, good, R, fill=True)
    assert st == capi.OK and not untouched
    for bad in (-0.1, 1.5, np.nan, np.inf):
        w = wts.copy()
        w[11] = bad
        st, untouched = raw_w(eng, 0, 1, nq, subs, vals, w, 0.25, good, R, fill=True)
        assert st == capi.ERR_INVALID and untouched, bad
        st, untouched = raw_w(eng, 0, 1, nq, subs, vals, wts, bad, good, R, fill=True)
        assert st == capi.ERR_INVALID and untouched, bad
        st, untouched = raw_w(eng, 0, 1, nq, subs, vals, None, bad, None, R, fill=True)
        assert st == capi.ERR_INVALID and untouched, bad
    # what the unweighted entry refuses, with the same code
    row = np.arange(len(vals))[:, None]
    for p, mode, n, s, o in [(0, 3, nq, subs, good), (1, 1, nq, subs, good), (0, 1, -1, subs, good), (0, 1, nq - 1, subs, good),
                             (0, 1, nq, np.where(row == 9, [40, 0, 0], subs), good), (0, 1, nq, subs, capi.FoldinOptions(-0.5, 0, 5, 0, 0)),
                             (0, 1, nq, subs, capi.FoldinOptions(0.5, 2, 5, 0, 0)), (0, 1, nq, subs, capi.FoldinOptions(0.5, 1, 0, 0, 0))]:
        st, untouched = raw_w(eng, p, mode, n, s, vals, wts, 0.25, o, R, fill=True)
        assert st == capi.ERR_INVALID and untouched, (p, mode, n)
    assert eng.lib.aoadmm_resident_fold_in_w(eng.h, 0, 1, 0, 0, None, None, None, 0.5, None, None, None, None, None, None) == capi.OK
    with pytest.raises(ValueError):
        eng.fold_in(0, 1, subs, vals, weights=wts[:-1])
    # accounting: one launch per call; a weight list adds 8 bytes per observation, alpha > 0 the rows read for H
    def stats(**kw):
        eng.kernel_stats(FOLDIN_CLASS, reset=True)
        eng.fold_in(0, 1, subs, vals, nq=nq, ridge=0.5, **kw)
        ms, launches, by, fl = eng.kernel_stats(FOLDIN_CLASS)
        assert launches == 1 and ms >= 0.0
        return by, fl

    nobs, other = len(vals), shape[0] + shape[2]
    by0, fl0 = stats()
    assert stats(weights=wts) == (by0 + 8 * nobs, fl0)
    assert stats(unstored_weight=0.5) == (by0 + 8 * R * other, fl0 + R * R * other)
    assert stats(weights=wts, unstored_weight=0.5) == (by0 + 8 * nobs + 8 * R * other, fl0 + R * R * other)


@pytest.mark.parametrize('sparse', [False, True])
def test_parafac2_block_is_refused(pkg, eng, sparse):
    rng = np.random.default_rng(13)
    par2_block(pkg, eng, rng, sparse)
    with pytest.raises(pkg.UnsupportedOnDevice) as ei:
        eng.fold_in(0, 0, np.zeros((3, 3), dtype=np.int64), np.ones(3), ridge=1.0, weights=np.ones(3), unstored_weight=0.5)
    assert ei.value.code == capi.ERR_UNSUPPORTED and 'PARAFAC2' in str(ei.value)


def test_multi_device_context_is_refused(pkg):
    rng = np.random.default_rng(14)
    shape, R = (12, 10, 8), 3
    Z = cp_Z(shape, R, empty(pkg, shape))
    with pkg.Engine([0, 0]) as e:
        pkg.build_model(e, Z)
        pkg.upload_state(e, Z, {'fac': [rng.random((s, R)) for s in shape]})
        subs, vals = FR.make_list(rng, shape, 0, [5, 5])
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.fold_in(0, 0, subs, vals, ridge=1.0, unstored_weight=0.5)


# ---- 11. known answer: outliers -------------------------------------------------------------------------------------------
# The numpy restatement (FW.fold_in, fp64) on the draw below: relative error of the five rows against the generating
# rows, worst with weight 0.01 on the outliers and best with unit weights.  The bars are these with a factor 2 of slack.
OUTLIER_NUMPY_WORST_WEIGHTED = 0.00358
OUTLIER_NUMPY_BEST_UNWEIGHTED = 0.0542


def outlier_case():
    rng = np.random.default_rng(31)
    shape, R, nq = (5, 25, 20), 3, 5
    U = [rng.standard_normal((s, R)) for s in shape]
    subs, _ = FW.make_cells(rng, shape, 0, nq, 0.3)
    x = np.einsum('er,er->e', U[0][subs[:, 0]], FR.zrows(U, 0, subs)) + 0.01 * rng.standard_normal(len(subs))
    out = rng.random(len(subs)) < 0.1
    x = x + np.where(out, 5.0 * rng.standard_normal(len(subs)), 0.0)
    return U, subs, x, out


def row_errors(rows, U):
    return np.linalg.norm(rows - U[0], axis=1) / np.linalg.norm(U[0], axis=1)


def test_known_answer_outliers(pkg, eng):
    """Five new rows of a 5 x 25 x 20 model at R = 3 (the true factors are the state), 30 % of the cells listed, noise
    0.01, a tenth of the listed entries hit by N(0, 5^2).  With weight 0.01 on those the rows come back; with unit
    weights they do not."""
    U, subs, x, out = outlier_case()
    dataless(pkg, eng, U)
    w = np.where(out, 0.01, 1.0)
    rows_w, info, _ = eng.fold_in(0, 0, subs, x, nq=5, weights=w)
    rows_1, info1, _ = eng.fold_in(0, 0, subs, x, nq=5, weights=np.ones(len(x)))
    assert not info.any() and not info1.any()
    ew, e1 = row_errors(rows_w, U), row_errors(rows_1, U)
    print('weighted rows: worst %.4g; unit weights: best %.4g' % (ew.max(), e1.min()))
    assert ew.max() <= 2.0 * OUTLIER_NUMPY_WORST_WEIGHTED
    assert e1.min() >= OUTLIER_NUMPY_BEST_UNWEIGHTED / 2.0
    assert ew.max() < e1.min()


# ---- 12. known answer: alpha = 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('other,R', [((25, 20), 3), ((9, 8), 20), ((6, 5, 4), 17), ((20, 16), 64)])
def test_known_answer_alpha_one(pkg, eng, other, R):
    """A row whose unlisted cells are true zeros, w = 1, alpha = 1: the dense least-squares row over all cells, within
    the bar of test_rows against the longdouble solve of the dense normal equations."""
    rng = np.random.default_rng(41 + R)
    shape = (3,) + tuple(other)
    U = [rng.standard_normal((s, R)) for s in shape]
    subs, vals = FW.make_cells(rng, shape, 0, 3, 0.3)
    dataless(pkg, eng, U)
    rows, info, _ = eng.fold_in(0, 0, subs, vals, nq=3, weights=np.ones(len(vals)), unstored_weight=1.0)
    f64, _, _ = FW.fold_in(U, 0, subs, vals, None, 1.0, 3)
    assert not info.any()
    ld = np.zeros((3, R), dtype=FR.LD)
    for q in range(3):
        sel = subs[:, 0] == q
        Z, W, x = FW.dense_problem(U, 0, subs[sel], vals[sel], None, 1.0)
        assert (W == 1.0).all()
        Zl, xl = Z.astype(FR.LD), x.astype(FR.LD)
        assert np.linalg.cond(Z.T @ Z) <= 1e6
        ld[q], bad = FR.solve_row(Zl.T @ Zl, Zl.T @ xl, 0.0)
        assert bad == 0
        want = np.linalg.lstsq(Z, x, rcond=None)[0]
        assert np.max(np.abs(ld[q].astype(np.float64) - want)) <= 1e-10 * np.max(np.abs(want))
    print('other = %s, R = %d: worst device error %.3g' % (other, R, check_rows(rows, ld, f64)))


# ---- 13. end to end ------------------------------------------------------------------------------------------------------
def test_end_to_end_on_the_weighted_model(pkg, eng):
    """The 30 x 25 x 20 weighted model of tests/test_gpu_sparse_weighted.py (weight 0.01 on the outliers, alpha = 0.05):
    take_rows(return_index=True) cuts the weights beside the values, fold_in under them (non-negative), topk_w with the
    stored fibres excluded returns no stored entry."""
    Zr, Zs, out_flag, A, X, mask, G = known_answer_model(pkg)
    S = Zs['object'][0]
    w, alpha = np.where(out_flag, 0.01, 1.0), 0.05
    _, Fac, _, _ = pkg.cmtf_AOADMM(Zs, alg_options=weighted_alg(options(MaxOuterIters=20), 1, 0, w, alpha), init=copy.deepcopy(G), engine=eng)
    F = [np.asarray(f) for f in Fac['fac']]
    new = np.array([4, 11, 12, 20, 29])
    subs, vals, index = S.take_rows(0, new, return_index=True)
    assert np.array_equal(S.vals[index], vals)
    kw = dict(nq=len(new), nonneg=True, max_inner=50, ridge=1e-8)
    rows, info, iters = eng.fold_in(0, 0, subs, vals, weights=w[index], unstored_weight=alpha, **kw)
    assert not info.any() and (rows >= 0).all()
    want, _, _ = FW.fold_in(F, 0, subs, vals, w[index], alpha, len(new), ridge=1e-8, nonneg=True, max_inner=50)
    assert np.max(np.abs(rows - want)) <= 1e-9 * np.max(np.abs(want))
    plain, _, _ = eng.fold_in(0, 0, subs, vals, **kw)
    assert np.max(np.abs(rows - plain)) > 1e-3 * np.max(np.abs(rows))         # another objective, another row
    rng = np.random.default_rng(5)
    k = 5
    ctx = rng.integers(0, S.shape[2], len(new))
    q3 = np.stack([new, np.zeros(len(new), dtype=np.int64), ctx], axis=1)
    ex = S.fiber_lists(1, q3)
    W = rows * F[2][ctx]
    idx, val = eng.topk_w(0, 1, W, k, exclude=ex)
    stored = {tuple(s) for s in S.subs.tolist()}
    scores = W @ F[1].T
    for q in range(len(new)):
        free = np.setdiff1d(np.arange(S.shape[1]), ex[1][ex[0][q]:ex[0][q + 1]])
        best = free[np.lexsort((free, -scores[q, free]))][:k]
        assert np.allclose(val[q][:len(best)], scores[q, best], rtol=1e-12, atol=1e-300)
        for j in idx[q]:
            assert j == -1 or (int(new[q]), int(j), int(ctx[q])) not in stored
        assert (idx[q] >= 0).sum() == min(k, len(free))
