"""CPU: the host layer of the ranks of held-out entries.  The header declares
`aoadmm_resident_rank_of` and `aoadmm_resident_rank_of_w`, the binding lists them and the library exports them; the
engine wraps them; `ranking_metrics` against a brute-force loop; the numpy reference of the GPU tests against
`ref_topk`."""
import importlib
import math
import os
import re

import numpy as np
import pytest

from rank_of_ref import count_plan, ref_rank, ref_rank_w, weights, well_separated
from test_gpu_topk import int_factors, queries, ref_topk

capi = importlib.import_module('matlab-code_amd._capi')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ('const int64_t* excl_off, const int64_t* excl_idx, int64_t* rank, double* score, int64_t* ncand_or_null')
ENTRIES = {
    'aoadmm_resident_rank_of': 'aoadmm_ctx* ctx, int p, int mode, int64_t nq, const int64_t* subs, ' + TAIL,
    'aoadmm_resident_rank_of_w': 'aoadmm_ctx* ctx, int p, int mode, int64_t nq, const double* W, const int64_t* targets, ' + TAIL,
}


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_entries_are_declared_bound_and_exported(pkg, entry):
    with open(os.path.join(ROOT, 'include', 'aoadmm_hip.h')) as f:
        text = f.read()
    decl = re.search(r'^int %s\(([^;]*)\);' % entry, text, flags=re.M | re.S)
    assert decl, 'the header does not declare %s' % entry
    assert ' '.join(decl.group(1).split()) == ENTRIES[entry]
    assert entry in pkg.SYMBOLS and entry in capi.SYMBOLS
    lib = pkg.load_library()
    assert hasattr(lib, entry) and len(getattr(lib, entry).argtypes) == ENTRIES[entry].count(',') + 1
    assert lib.aoadmm_abi_version() == 3               # functions were added, nothing moved: the version stays


def test_engine_and_package_have_the_wrappers(pkg):
    assert callable(getattr(pkg.Engine, 'rank_of', None)) and callable(getattr(pkg.Engine, 'rank_of_w', None))
    assert callable(getattr(pkg, 'ranking_metrics', None)) and 'ranking_metrics' in pkg.__all__


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    assert lib.aoadmm_resident_rank_of(None, 0, 0, 0, None, None, None, None, None, None) != capi.OK
    assert lib.aoadmm_resident_rank_of_w(None, 0, 0, 0, None, None, None, None, None, None, None) != capi.OK


def brute_metrics(rank, ncand, ks):
    out = {}
    used = [int(r) for r in rank if r >= 0]
    out['n'] = len(used)
    for k in ks:
        out['hit@%d' % k] = sum(1.0 for r in used if r < k) / len(used)
        out['ndcg@%d' % k] = sum(1.0 / math.log2(r + 2) for r in used if r < k) / len(used)
    out['mrr'] = sum(1.0 / (r + 1) for r in used) / len(used)
    if ncand is not None:
        terms = [1.0 - r / (n - 1.0) for r, n in zip(rank, ncand) if r >= 0 and n >= 2]
        out['auc'] = sum(terms) / len(terms)
        out['n_auc'] = len(terms)
    return out


@pytest.mark.parametrize('seed', range(4))
def test_ranking_metrics_against_a_brute_force_loop(pkg, seed):
    rng = np.random.default_rng(seed)
    n = 200
    ncand = rng.integers(0, 60, n)
    ncand[:30] = rng.integers(0, 3, 30)                        # 0, 1 and 2 candidates
    rank = np.array([rng.integers(0, c) if c > 0 else -1 for c in ncand], dtype=np.int64)
    rank[rng.random(n) < 0.1] = -1                             # NaN targets, whatever their ncand
    assert {0, 1, 2} <= set(ncand.tolist()) and (rank == -1).any() and ((rank >= 0) & (ncand == 1)).any()
    ks = (1, 5, 10, 37)
    got = pkg.ranking_metrics(rank, ncand, ks=ks)
    want = brute_metrics(rank, ncand, ks)
    assert set(got) == set(want)
    for key in want:
        assert got[key] == pytest.approx(want[key], rel=1e-13, abs=0), key
    assert got['n'] == int((rank >= 0).sum()) and isinstance(got['n'], int)
    short = pkg.ranking_metrics(rank)                          # without ncand: no auc; the default ks
    assert set(short) == {'n', 'mrr', 'hit@1', 'hit@5', 'hit@10', 'ndcg@1', 'ndcg@5', 'ndcg@10'}
    assert short['mrr'] == got['mrr'] and short['hit@5'] == got['hit@5']


def test_ranking_metrics_edges(pkg):
    m = pkg.ranking_metrics([0, 0, 0], [5, 1, 2])
    assert m['hit@1'] == 1.0 and m['ndcg@1'] == 1.0 and m['mrr'] == 1.0 and m['auc'] == 1.0 and m['n_auc'] == 2 and m['n'] == 3
    m = pkg.ranking_metrics([4], [5])
    assert m['hit@1'] == 0.0 and m['hit@5'] == 1.0 and m['auc'] == 0.0 and m['ndcg@5'] == 1.0 / math.log2(6.0)
    m = pkg.ranking_metrics([-1, -1], [3, 0])
    assert m['n'] == 0 and math.isnan(m['mrr']) and math.isnan(m['auc']) and m['n_auc'] == 0
    with pytest.raises(ValueError):
        pkg.ranking_metrics([0, 1], [3])


@pytest.mark.parametrize('N,mode,I,R', [(2, 0, 257, 3), (3, 1, 100, 5), (4, 3, 40, 4)])
def test_reference_against_ref_topk(N, mode, I, R):
    """Integer factors: every score exact, ties everywhere.  The reference's rank is the target's position in ref_topk's
    answer over all rows, its score the value there, ncand the length of the answer without padding."""
    rng = np.random.default_rng(N + I)
    shape = [6, 5, 4, 3][:N]
    shape[mode] = I
    U = int_factors(rng, shape, R)
    U[mode][5, :] = np.nan                                     # one row that is never a candidate
    nq = 23
    subs = queries(rng, shape, nq)
    subs[0, mode] = 5                                          # a NaN target
    lists = [rng.integers(0, I, int(rng.integers(0, 9))) for _ in range(nq)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    ex = (off, np.concatenate(lists).astype(np.int64))
    for exclude in (None, ex):
        with np.errstate(invalid='ignore'):
            rank, score, ncand = ref_rank(U, mode, subs, exclude)
            idx, val = ref_topk(U, mode, subs, I, exclude)
        assert rank[0] == -1 and np.isnan(score[0])
        for q in range(nq):
            t = subs[q, mode]
            listed = exclude is not None and t in lists[q]
            have = int((idx[q] >= 0).sum())
            assert ncand[q] == have + (1 if listed and q != 0 else 0)
            if q == 0:
                continue
            if not listed:
                assert idx[q, rank[q]] == t and val[q, rank[q]] == score[q]
            else:                                              # the listed target: the place it would take in the answer
                before = sum(1 for j in range(have) if val[q, j] > score[q] or (val[q, j] == score[q] and idx[q, j] < t))
                assert rank[q] == before
    # the form with weights is the same function
    W = weights(U, mode, subs)
    with np.errstate(invalid='ignore'):
        a = ref_rank(U, mode, subs, ex)
        b = ref_rank_w(U[mode], W, subs[:, mode], ex)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


REAL = [(5003, 20, 3, 40), (257, 64, 4, 17), (1000, 5, 2, 16)]


def real_case(I, R, N, nq, excluded=False):
    """The real-valued cases of the GPU tests: factors, queries whose targets come from the reference's best 64 for
    every second query and from all rows for the rest, and exclusion lists when asked for."""
    rng = np.random.default_rng(1)
    shape = [7, 6, 5, 4][:N]
    mode = N - 1
    shape[mode] = I
    U = [rng.standard_normal((s, R)) for s in shape]
    subs = queries(rng, shape, nq)
    ex = None
    lists = None
    if excluded:
        lists = [rng.integers(0, I, int(rng.integers(0, 30))) for _ in range(nq)]
        off = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
        ex = (off, np.concatenate(lists).astype(np.int64))
    best, _ = ref_topk(U, mode, subs, 64, ex)
    for q in range(nq):
        if q % 4 != 3:                                         # three of four targets stand among the first 64
            subs[q, mode] = best[q, int(rng.integers(0, 64))]
    return U, mode, subs, ex


@pytest.mark.parametrize('I,R,N,nq', REAL)
@pytest.mark.parametrize('excluded', [False, True])
def test_the_real_valued_cases_are_well_separated(I, R, N, nq, excluded):
    """The seeds of the GPU tests: no row's score lies within twice the tolerance of a target's, so the device's ranks
    must equal numpy's."""
    U, mode, subs, ex = real_case(I, R, N, nq, excluded)
    worst, tol = well_separated(U, mode, subs, ex)
    assert worst > 1.0, worst
    rank, _, _ = ref_rank(U, mode, subs, ex)
    assert (rank < 64).sum() * 2 >= nq and (rank >= 0).all()


def test_count_plan():
    assert count_plan(70001, 40) == (2, 2, 274, 256)
    assert count_plan(70001, 3) == (1, 1, 274, 256)
    assert count_plan(1, 1) == (1, 1, 1, 16)
    assert count_plan(1_000_000, 16384) == (2, 512, 4, 250000)
