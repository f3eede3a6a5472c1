"""GPU: ranking metrics tracked inside a solve (aoadmm_tensor_set_ranklist, aoadmm_rank_track, aoadmm_rank_trace,
aoadmm_ranklist_last, aoadmm_op_rank_metrics; csrc/rank_metrics.hip).  The reference is
`ranking_metrics` and numpy sums with its formulas applied to what `Engine.rank_of` returns on an engine brought to the
iteration in question by a prefix solve (solves are bit-reproducible), never the code under test."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from helpers import cp_model, options
from test_gpu_heldout import NN, cp_Z, par2_block, same, solve_case, some_entries
from test_gpu_heldout_best import assert_state
from test_gpu_rank_of import planted_feedback
from test_gpu_sparse_sharded import empty, on_ranks
from test_gpu_sparse_weighted import draw_weights, weighted_alg
from test_gpu_topk import queries
from test_rank_of_host import REAL

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')
RANK_CLASS = 13        # counted with the top-k completions and the rank_of calls
N_CLASSES = 15
FLOAT_SUMS = ('ndcg_sum', 'mrr_sum', 'auc_sum')


def bound(n):
    """Relative bound of a float sum over n non-negative terms: numpy's summation order against the device's, each within
    (n - 1) 2^-53 of the exact sum of its terms, and a few ulp per term for log2 and the divisions."""
    return (n + 8) * 2.0 ** -52


def ref_sums(rank, ncand, k):
    """The sums behind `ranking_metrics`, with its formulas word for word and np.sum in the place of np.mean."""
    rank = np.asarray(rank, dtype=np.int64).reshape(-1)
    ncand = np.asarray(ncand, dtype=np.int64).reshape(-1)
    use = rank >= 0
    r = rank[use].astype(np.float64)
    hit = r < k
    sel = use & (ncand >= 2)
    return dict(n=int(use.sum()), n_auc=int(sel.sum()), hits=int(hit.sum()),
                ndcg_sum=float(np.sum(np.where(hit, 1.0 / np.log2(r + 2.0), 0.0))), mrr_sum=float(np.sum(1.0 / (r + 1.0))),
                auc_sum=float(np.sum(1.0 - rank[sel] / (ncand[sel] - 1.0))))


def close(got, want, n):
    """|got - want| <= bound(n) |want|; returns the ratio to the bound (0 for an exact zero)"""
    if want == 0.0:
        assert got == 0.0
        return 0.0
    ratio = abs(got - want) / (bound(n) * abs(want))
    assert ratio <= 1.0, (got, want, n, ratio)
    return ratio


# ---- 1. the reduction alone ----------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 255, 256, 257, 4097, 70001]     # one lane, one wave, both sides of a team, many teams, the finisher's stride
KS = [1, 10, 2 ** 31 - 1]


def draw(rng, n, k):
    """Ranks from {-1, 0, k - 1, k, 2^31 - 2} mixed with uniform ones; ncand from {1, 2, rank + 1, 2^31 - 1}, raised to
    rank + 1 where the draw fell below it: rank_of never returns fewer candidates than the target's place needs, and
    with rank <= ncand - 1 every term of every sum is non-negative, which the bound rests on."""
    special = np.array([-1, 0, k - 1, k, 2 ** 31 - 2], dtype=np.int64)
    rank = np.where(rng.random(n) < 0.5, special[rng.integers(0, 5, n)], rng.integers(0, 3000, n)).astype(np.int64)
    pick = rng.integers(0, 4, n)
    ncand = np.choose(pick, [np.ones(n, dtype=np.int64), np.full(n, 2, dtype=np.int64), rank + 1, np.full(n, 2 ** 31 - 1, dtype=np.int64)])
    return rank, np.maximum(ncand, rank + 1).astype(np.int64)


def check_op(eng, rank, ncand, k):
    out = eng.op_rank_metrics(rank, ncand, k)
    want = ref_sums(rank, ncand, k)
    assert np.array_equal(out[[capi.RANKSUM_N, capi.RANKSUM_N_AUC, capi.RANKSUM_HITS]], [want['n'], want['n_auc'], want['hits']])
    assert out[6] == 0.0 and out[7] == 0.0
    n = len(rank)
    ratios = [close(out[capi.RANKSUM_NDCG], want['ndcg_sum'], n), close(out[capi.RANKSUM_MRR], want['mrr_sum'], n),
              close(out[capi.RANKSUM_AUC], want['auc_sum'], n)]
    assert np.array_equal(eng.op_rank_metrics(rank, ncand, k), out)          # two calls: the same bits
    return out, want, max(ratios)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', SIZES)
def test_reduction_against_numpy(pkg, eng, n, k):
    rng = np.random.default_rng(n + k % 1000)
    rank, ncand = draw(rng, n, k)
    out, want, worst = check_op(eng, rank, ncand, k)
    print('n = %d, k = %d: largest |device - numpy| / bound = %.3f' % (n, k, worst))
    # the means of ranking_metrics follow from the same sums
    m = pkg.ranking_metrics(rank, ncand, ks=(k,))
    if want['n']:
        assert m['n'] == want['n'] and m['hit@%d' % k] == want['hits'] / want['n']
        assert abs(m['mrr'] - out[capi.RANKSUM_MRR] / want['n']) <= (bound(n) + 2.0 ** -51) * m['mrr']


@pytest.mark.parametrize('n', [1, 257, 4097])
def test_reduction_edges(pkg, eng, n):
    # every rank -1: counts 0, sums 0, every mean NaN
    out = eng.op_rank_metrics(np.full(n, -1), np.full(n, 5), 10)
    assert np.array_equal(out, np.zeros(8))
    d = pkg.Engine._rank_trace_dict(np.zeros(1, dtype=np.int64), out[:capi.RANKSUM_COUNT, None], 0)
    assert all(np.isnan(d[key][0]) for key in ('hit', 'ndcg', 'mrr', 'auc')) and d['n'][0] == 0 and d['n_auc'][0] == 0
    # a single ncand = 1: left out of AUC only
    rng = np.random.default_rng(n)
    rank = rng.integers(0, 50, n)
    ncand = rank + 1 + rng.integers(1, 50, n)
    rank[n // 2], ncand[n // 2] = 0, 1
    out, want, _ = check_op(eng, rank, ncand, 10)
    assert want['n'] == n and want['n_auc'] == n - 1 and out[capi.RANKSUM_N_AUC] == n - 1
    # exact cases: every rank 0 among two candidates -> every sum is n
    out = eng.op_rank_metrics(np.zeros(n), np.full(n, 2), 1)
    assert np.array_equal(out, [n, n, n, n, n, n, 0, 0])


def test_reduction_refusals(pkg, eng):
    i64p = C.POINTER(C.c_int64)
    r = np.zeros(4, dtype=np.int64)
    out = np.zeros(8)
    for n, k in ((0, 1), (-1, 1), (4, 0)):
        assert eng.lib.aoadmm_op_rank_metrics(eng.h, n, r.ctypes.data_as(i64p), r.ctypes.data_as(i64p), k, capi.dptr(out)) == capi.ERR_INVALID
    assert eng.lib.aoadmm_op_rank_metrics(eng.h, 4, None, r.ctypes.data_as(i64p), 1, capi.dptr(out)) == capi.ERR_INVALID


# ---- 2. inside solves --------------------------------------------------------------------------------------------------------
class Fit:
    """A model and its starting point, run through the engine step by step (block 1 carries the lists)."""

    def __init__(self, Z, io, opt, hip=None, prec='f64'):
        self.G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
        ranks = [int((F[0] if isinstance(F, (list, tuple)) else F).shape[1]) for F in self.G['fac']]
        self.Z = dict(Z, _ranks=ranks)
        self.opt, self.hip, self.prec = opt, dict(hip or {}), prec
        self.has_missing = bool(self.hip.get('sparse_observed_only')) or self.hip.get('sparse_entry_weights') is not None

    def start(self, pkg, e, rank=None, track=None, held=None, keep=False, sharding=False):
        pkg.build_model(e, self.Z, self.prec, sparse_sharding=sharding, observed_only=self.hip.get('sparse_observed_only', 0),
                        entry_weights=self.hip.get('sparse_entry_weights'), unstored_weight=self.hip.get('sparse_unstored_weight'))
        if held is not None:
            e.set_heldout(0, *held)
        if rank is not None:
            e.set_ranklist(0, rank[0], rank[1], exclude=rank[2])
        if track is not None:
            e.rank_track(**track)
        if keep:
            e.heldout_keep_best(True)
        pkg.upload_state(e, self.Z, copy.deepcopy(self.G))

    def solve(self, pkg, e, iters, **hip):
        out = pkg.run_solver(e, {**self.opt, 'MaxOuterIters': iters, 'hip': {**self.hip, **hip}}, len(self.Z['size']),
                             has_missing=self.has_missing)
        del out['time_at_it']
        return out

    def state(self, pkg, e):
        return pkg.download_state(e, self.Z, self.G)


def sparse_fit(pkg, I, R, N, nq):
    """rank_of's shapes as sparse blocks of 3000 nonzeros, every mode non-negative; the list's exclusions are the stored
    rows of every query's fibre plus, for query 1, 3000 random rows with repeats (more than one chunk of 1024 where the
    mode is long enough)."""
    rng = np.random.default_rng(I + R)
    shape = [7, 6, 5, 4][:N]
    mode = N - 1
    shape[mode] = I
    S = some_entries(pkg, rng, shape, 3000)
    Z = cp_Z(shape, R, S)
    Z.update(constrained_modes=[1] * N, constraints=[NN] * N)
    del Z['_ranks']
    io = dict(lambdas_init=[[1] * R], nvecs=0, distr=[(lambda a, b: rng.random((a, b)))] * N, normalize=1)
    subs = queries(rng, shape, nq)
    off, idx = S.fiber_lists(mode, subs)
    lists = [idx[off[q]:off[q + 1]] for q in range(nq)]
    lists[1] = np.concatenate([lists[1], rng.integers(0, I, 3000)])
    off = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    return Fit(Z, io, options(MaxInnerIters=5)), (mode, subs, (off, np.concatenate(lists).astype(np.int64)))


def check_trace_entry(pkg, tr, e, got_rank, k):
    """entry e of a trace dict against rank_of's output on the same state"""
    rank, _, ncand = got_rank
    want = ref_sums(rank, ncand, k)
    assert (tr['n'][e], tr['n_auc'][e], tr['hits'][e]) == (want['n'], want['n_auc'], want['hits'])
    worst = max(close(tr[key][e], want[key], len(rank)) for key in FLOAT_SUMS)
    m = pkg.ranking_metrics(rank, ncand, ks=(k,))
    for name, key in (('hit', 'hit@%d' % k), ('ndcg', 'ndcg@%d' % k), ('mrr', 'mrr'), ('auc', 'auc')):
        assert abs(tr[name][e] - m[key]) <= (bound(len(rank)) + 2.0 ** -51) * abs(m[key]), name
    return worst


@pytest.mark.parametrize('I,R,N,nq', REAL)
def test_trace_equals_rank_of(pkg, eng, I, R, N, nq):
    fit, rl = sparse_fit(pkg, I, R, N, nq)
    mode, subs, ex = rl
    k = I // 3                                                  # deep enough that hit and NDCG see a share of the targets
    fit.start(pkg, eng, rank=rl, track=dict(metric='ndcg', k=k))
    info = eng.ranklist_info(0)
    assert info['nq'] == nq and info['mode'] == mode and 0 < info['listed'] < len(ex[1]) and info['resident_bytes'] > 0
    if I > 3000:
        assert info['listed'] > 2 * 1024                        # an exclusion pass of several chunks
    fit.solve(pkg, eng, 4)
    tr = eng.rank_trace(0)
    assert tr['iters'].tolist() == [0, 1, 2, 3, 4]
    last = eng.ranklist_last(0)
    after = eng.rank_of(0, mode, subs, exclude=ex)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(last, after))
    worst = check_trace_entry(pkg, tr, 4, after, k)
    for i in (0, 1):
        fit.start(pkg, eng)
        fit.solve(pkg, eng, i)
        worst = max(worst, check_trace_entry(pkg, tr, i, eng.rank_of(0, mode, subs, exclude=ex), k))
    print('I = %d R = %d: ndcg@(I/3) %s, largest |trace - numpy| / bound = %.3f' % (I, R, np.round(tr['ndcg'], 4), worst))


def launches(eng, reset=False):
    return [eng.kernel_stats(c, reset=reset)[1] for c in range(N_CLASSES)]


MOVE_CASES = ['sparse', 'weighted', 'dense', 'f16', 'coupled']


@pytest.mark.parametrize('name', MOVE_CASES)
def test_nothing_else_moves(pkg, eng, name):
    """With a held-out list attached, a solve with and without a ranking list: factors, duals, innerIters, every trace
    and every kernel-statistics class but 13 are the same bits; class 13 grows by one launch per list and evaluation."""
    Z, io, opt, held, hip, prec = solve_case(pkg, 'sparse' if name == 'weighted' else name)
    rng = np.random.default_rng(len(name))
    if name == 'weighted':
        opt = weighted_alg(opt, 1, 0, draw_weights(rng, Z['object'][0].nnz), 0.1)
        hip = opt.pop('hip')
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    md = [m - 1 for m in Z['modes'][0]]
    shape = [int(Z['size'][m]) for m in md]
    subs = queries(rng, shape, 30)
    S = Z['object'][0]
    ex = S.fiber_lists(2, subs) if hasattr(S, 'fiber_lists') else None
    rl = {1: dict(mode=3, subs=subs, exclude=ex)}

    def run(with_list):
        alg = {**opt, 'hip': {**hip, 'heldout': held, **({'rank_lists': rl, 'rank_metric': 'hit@5'} if with_list else {})}}
        launches(eng, reset=True)
        _, F, _, out = pkg.cmtf_AOADMM(Z, alg_options=alg, init=copy.deepcopy(G), engine=eng, precision=prec)
        return F, out, launches(eng)

    (Fp, op, lp), (Fr, orr, lr) = run(False), run(True)
    assert same(Fp, Fr)
    for key in op:
        if key != 'time_at_it':
            assert same(op[key], orr[key]), key
    assert set(orr) - set(op) == {'rank_trace', 'rank_best_iter'}
    iters = op['OuterIterations']
    assert iters == opt['MaxOuterIters'] and orr['rank_trace'][1]['iters'].tolist() == list(range(iters + 1))
    for c in range(N_CLASSES):
        assert lr[c] - lp[c] == (iters + 1 if c == RANK_CLASS else 0), c
    assert orr['rank_trace'][1]['n'].tolist() == [30] * (iters + 1)


def test_every_third_iteration(pkg, eng):
    fit, rl = sparse_fit(pkg, *REAL[2])
    fit.start(pkg, eng, rank=rl, track=dict(metric='mrr', every=1))
    out1 = fit.solve(pkg, eng, 7)
    t1 = eng.rank_trace(0)
    fit.start(pkg, eng, rank=rl, track=dict(metric='mrr', every=3))
    launches(eng, reset=True)
    out3 = fit.solve(pkg, eng, 7)
    t3 = eng.rank_trace(0)
    assert t3['iters'].tolist() == [0, 3, 6] and t1['iters'].tolist() == list(range(8))
    for key in ('n', 'n_auc', 'hits') + FLOAT_SUMS:
        assert np.array_equal(t3[key], t1[key][[0, 3, 6]]), key
    assert launches(eng)[RANK_CLASS] == 3 and same(out1, out3)
    last = eng.ranklist_last(0)                                  # the evaluation of iteration 6, not of the last iteration
    fit.start(pkg, eng)
    fit.solve(pkg, eng, 6)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(last, eng.rank_of(0, rl[0], rl[1], exclude=rl[2])))


# ---- 3. the maximum is placed ------------------------------------------------------------------------------------------------
B, LAST, NQ = 3, 12, 200
_placed = {}


def placed(pkg, eng):
    """A noisy rank-4 fit; the targets are each query's best non-excluded row of the B-iteration solve (top-k with k = 1),
    so hit@1 = 1 at iteration B and nothing later can be strictly larger.  Computed once, left unchanged: the fit, the
    list, the state of the B-iteration solve and of two more iterations, and the un-stopped long solve."""
    if not _placed:
        rng = np.random.default_rng(12)
        shape = (30, 20, 300)
        Z, io, _ = cp_model(shape, 4, rng, [NN] * 3, noise=0.5)
        fit = Fit(Z, io, options(MaxInnerIters=5))
        subs = queries(rng, shape, NQ)
        lists = [rng.integers(0, 300, int(rng.integers(0, 40))) for _ in range(NQ)]
        off = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
        ex = (off, np.concatenate(lists).astype(np.int64))
        fit.start(pkg, eng)
        fit.solve(pkg, eng, B)
        best, _ = eng.topk(0, 2, subs, 1, exclude=ex)
        subs[:, 2] = best[:, 0]
        state_b = fit.state(pkg, eng)
        more_out = fit.solve(pkg, eng, 2)
        more_state = fit.state(pkg, eng)
        rl = (2, subs, ex)
        track = dict(metric='hit', k=1)
        fit.start(pkg, eng, rank=rl, track=track)
        out = fit.solve(pkg, eng, LAST)
        tr = eng.rank_trace(0)
        S = pkg.pooled_score([tr], 'hit')
        print('hit@1 over the un-stopped solve:', np.round(S, 3))
        assert tr['best_iter'] == B and S[B] == 1.0 and (S[:B] < 1.0).all(), 'precondition: iteration %d is the first with S = 1' % B
        _placed.update(fit=fit, rl=rl, track=track, state_b=state_b, more_out=more_out, more_state=more_state, out=out, tr=tr, S=S,
                       state=fit.state(pkg, eng))
    return _placed


@pytest.mark.parametrize('patience', [1, 2, 4])
def test_patience_stops_where_the_host_rule_says(pkg, eng, patience):
    p = placed(pkg, eng)
    fit = p['fit']
    fit.start(pkg, eng, rank=p['rl'], track=dict(p['track'], patience=patience, criterion=1))
    out = fit.solve(pkg, eng, LAST)
    tr = eng.rank_trace(0)
    stop = B + patience
    assert pkg.rank_rule(p['S'], patience) == (B, stop)           # the host rule on the un-stopped trace
    assert out['OuterIterations'] == stop and out['exit_flag'] == 'rankPatience' and tr['best_iter'] == B
    assert tr['iters'].tolist() == list(range(stop + 1))
    for key in ('n', 'n_auc', 'hits') + FLOAT_SUMS:
        assert np.array_equal(tr[key], p['tr'][key][:stop + 1]), key
    assert np.array_equal(out['func_val_conv'], p['out']['func_val_conv'][:stop + 1])


@pytest.mark.parametrize('patience', [1, 2])
def test_patience_counts_evaluations(pkg, eng, patience):
    """every = 3: the evaluations are at 0, 3, 6, 9, 12 and the second of them has S = 1; patience n stops n evaluations,
    that is 3 n iterations, later."""
    p = placed(pkg, eng)
    fit = p['fit']
    fit.start(pkg, eng, rank=p['rl'], track=dict(p['track'], every=3, patience=patience, criterion=1))
    out = fit.solve(pkg, eng, LAST)
    tr = eng.rank_trace(0)
    assert pkg.rank_rule(p['S'][::3], patience) == (1, 1 + patience)
    assert out['OuterIterations'] == B + 3 * patience and out['exit_flag'] == 'rankPatience' and tr['best_iter'] == B
    assert tr['iters'].tolist() == list(range(0, B + 3 * patience + 1, 3))
    assert np.array_equal(tr['hits'], p['tr']['hits'][:B + 3 * patience + 1:3])


def test_last_permitted_iteration_reports_max_iterations(pkg, eng):
    p = placed(pkg, eng)
    fit = p['fit']
    fit.start(pkg, eng, rank=p['rl'], track=dict(p['track'], patience=2, criterion=1))
    out = fit.solve(pkg, eng, B + 2)                              # the rule fires in the last permitted iteration: code 0
    assert out['OuterIterations'] == B + 2 and out['exit_flag'] == 'maxIterations'


def test_keep_best_by_the_ranking_score(pkg, eng):
    p = placed(pkg, eng)
    fit = p['fit']
    fit.start(pkg, eng, rank=p['rl'], track=dict(p['track'], criterion=1), keep=True)
    out = fit.solve(pkg, eng, LAST)
    assert same(out, p['out'])                                    # the solve returns what it returned without the switch
    assert_state(fit.state(pkg, eng), p['state'], 'the solve with the switch on')
    info = eng.heldout_best_info()
    assert info['have'] and info['iter'] == B
    assert eng.heldout_restore_best() == B
    assert_state(fit.state(pkg, eng), p['state_b'], 'restored')
    more_out = fit.solve(pkg, eng, 2)
    assert same({k: v for k, v in more_out.items()}, p['more_out'])
    assert_state(fit.state(pkg, eng), p['more_state'], 'two iterations after the restore')


@pytest.mark.parametrize('criterion', [0, 1])
def test_keep_best_follows_the_criterion(pkg, eng, criterion):
    """A held-out list whose values are the model's own at iteration 5 (H is minimal there) beside the ranking list whose
    score is maximal at iteration 3: criterion 0 restores 5, criterion 1 restores 3."""
    p = placed(pkg, eng)
    fit = p['fit']
    rng = np.random.default_rng(5)
    hsubs = queries(rng, (30, 20, 300), 400)
    fit.start(pkg, eng)
    fit.solve(pkg, eng, 5)
    y = eng.model_at(0, hsubs)
    fit.start(pkg, eng, rank=p['rl'], track=dict(p['track'], criterion=criterion), held=(hsubs, y), keep=True)
    out = fit.solve(pkg, eng, LAST)
    H, hbest = eng.heldout_trace(0)
    tr = eng.rank_trace(0)
    assert hbest == 5 and tr['best_iter'] == B, 'precondition: H is smallest at 5 (%d), S largest at %d (%d)' % (hbest, B, tr['best_iter'])
    assert out['exit_flag'] == 'maxIterations' and np.array_equal(tr['hits'], p['tr']['hits'])
    assert eng.heldout_restore_best() == (B if criterion == 1 else 5)
    if criterion == 1:
        assert_state(fit.state(pkg, eng), p['state_b'], 'restored by S')


# ---- 4. ranks of a communicator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sharded', [False, True], ids=['replicated', 'sharded'])
def test_two_ranks_take_the_same_decision(pkg, eng, sharded):
    fit, rl = sparse_fit(pkg, *REAL[2])
    track = dict(metric='ndcg', k=10, patience=1, criterion=1)

    def run(e, r=0, sharding=False):
        fit.start(pkg, e, rank=rl, track=track, sharding=sharding)
        out = fit.solve(pkg, e, 10)
        tr = e.rank_trace(0)
        return out['OuterIterations'], out['exit_flag'], tr, e.ranklist_last(0)

    it1, flag1, tr1, last1 = run(eng)
    print('one engine: stops at %d (%s), best %d' % (it1, flag1, tr1['best_iter']))
    res = on_ranks(pkg, 2, lambda e, r: run(e, r, sharded))
    for it2, flag2, tr2, last2 in res:
        assert (it2, flag2) == (it1, flag1) and same(tr2, tr1)
        # per query: the ranks agree with each other to the bit; with the one engine in rank and ncand, and in the score
        # too where the nonzeros are replicated (a sharded block's MTTKRPs are summed over the ranks in another order)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(res[0][3], last2))
        assert np.array_equal(last1[0], last2[0]) and np.array_equal(last1[2], last2[2])
        assert sharded or np.array_equal(last1[1], last2[1], equal_nan=True)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def test_end_to_end_on_implicit_feedback(pkg, eng):
    """DESIGN.md section 9.7's planted 60 x 40 fit (R = 4, non-negativity, alpha = 0.1, 40 iterations, one stored entry
    per user held out) with the list tracked inside the solve: the last entry of out['rank_trace'] is what rank_of gives
    on the returned factors, and hit@10 exceeds 0.9 (section 9.7 measured 0.950 against a chance of 0.308)."""
    rng = np.random.default_rng(21)
    train, held = planted_feedback(pkg, rng)
    Z, io, _ = cp_model((60, 40), 4, rng, [NN, NN], noise=0.0)
    dense = np.zeros((60, 40))
    dense[tuple(train.subs.T)] = train.vals
    G = OA.init_coupled_AOADMM_CMTF({**dict(Z, object=[dense]), 'prox_operators': None}, io, rng=np.random.default_rng(7))
    ex = train.fiber_lists(1, held)
    alg = weighted_alg(options(MaxOuterIters=40), 1, 0, np.ones(train.nnz), 0.1,
                       rank_lists={1: dict(mode=2, subs=held, exclude=ex)}, rank_metric='hit@10')
    _, Fac, _, out = pkg.cmtf_AOADMM(dict(Z, object=[train]), alg_options=alg, init=copy.deepcopy(G), engine=eng)
    tr = out['rank_trace'][1]
    assert tr['iters'].tolist() == list(range(41)) and out['exit_flag'] == 'maxIterations'
    after = eng.rank_of(0, 1, held, exclude=ex)
    check_trace_entry(pkg, tr, 40, after, 10)
    m = pkg.ranking_metrics(after[0], after[2], ks=(10,))
    assert tr['hit'][40] == m['hit@10'] and tr['n'][40] == 60
    print('hit@10 %.4f at iteration 40, best pooled score at iteration %d' % (tr['hit'][40], out['rank_best_iter']))
    assert tr['hit'][40] > 0.9
    assert out['rank_best_iter'] == int(tr['iters'][pkg.rank_rule(tr['hit'])[0]])


# ---- 6. lifetime and refusals ------------------------------------------------------------------------------------------------
def invalid(pkg, fn):
    with pytest.raises(pkg.AoadmmError) as ei:
        fn()
    assert ei.value.code == capi.ERR_INVALID
    return str(ei.value)


def test_list_lifetime_and_refusals(pkg, eng):
    fit, rl = sparse_fit(pkg, *REAL[2])
    mode, subs, ex = rl
    S = fit.Z['object'][0]
    fit.start(pkg, eng, rank=rl)
    info = eng.ranklist_info(0)
    assert info['nq'] == len(subs)
    invalid(pkg, lambda: eng.ranklist_last(0))                    # no evaluation yet
    # a bad argument leaves the old list in place
    bad = subs.copy()
    bad[3, 0] = 7
    invalid(pkg, lambda: eng.set_ranklist(0, mode, bad, exclude=ex))
    invalid(pkg, lambda: eng.set_ranklist(0, 2, subs, exclude=ex))
    invalid(pkg, lambda: eng.set_ranklist(1, mode, subs, exclude=ex))
    rows = ex[1].copy()
    rows[5] = 1000
    invalid(pkg, lambda: eng.set_ranklist(0, mode, subs, exclude=(ex[0], rows)))
    invalid(pkg, lambda: eng.set_ranklist(0, mode, subs, exclude=(ex[0] + 1, np.concatenate([ex[1], [0]]))))
    assert eng.ranklist_info(0) == info
    # a new upload of the data keeps the list and the settings; the solve evaluates it
    eng.rank_track(metric='auc', every=2)
    eng.upload_coo(0, S.subs, S.vals)
    assert eng.ranklist_info(0) == info
    fit.solve(pkg, eng, 3)
    assert eng.rank_trace(0)['iters'].tolist() == [0, 2] and len(eng.ranklist_last(0)[0]) == len(subs)
    # the settings aoadmm_rank_track refuses; the old ones stay (every = 2 is still what a solve does)
    for args in ((9, 10, 1, 0, 0), (-1, 10, 1, 0, 0), (1, 0, 1, 0, 0), (1, -5, 1, 0, 0), (1, 10, 0, 0, 0), (1, 10, 1, -1, 0), (1, 10, 1, 0, 2),
                 (1, 10, 1, 0, -1), (1, 10, 1, 2, 0)):
        assert eng.lib.aoadmm_rank_track(eng.h, *args) == capi.ERR_INVALID, args
    with pytest.raises(ValueError):
        eng.rank_track(metric='precision')
    with pytest.raises(ValueError):
        eng.rank_track(k=2 ** 31)
    fit.solve(pkg, eng, 2)
    assert eng.rank_trace(0)['iters'].tolist() == [0, 2]
    # criterion 1 together with heldout_patience, and with no list at all
    eng.rank_track(criterion=1, patience=2)
    eng.set_heldout(0, subs, np.ones(len(subs)))
    assert 'heldout_patience' in invalid(pkg, lambda: fit.solve(pkg, eng, 2, heldout_patience=1))
    eng.set_heldout(0, subs[:0], np.zeros(0))
    eng.set_ranklist(0, mode, subs[:0])                           # nq = 0 removes the list
    assert eng.ranklist_info(0) == dict(nq=0, mode=-1, listed=0, resident_bytes=0)
    assert 'ranking list' in invalid(pkg, lambda: fit.solve(pkg, eng, 2))
    # keep-best with neither kind of list is still refused, whatever the criterion
    eng.heldout_keep_best(True)
    invalid(pkg, lambda: fit.solve(pkg, eng, 2))
    eng.rank_track(criterion=0)
    invalid(pkg, lambda: fit.solve(pkg, eng, 2))
    eng.set_ranklist(0, mode, subs, exclude=ex)                   # criterion 0: a ranking list does not serve keep-best
    invalid(pkg, lambda: fit.solve(pkg, eng, 2))
    eng.heldout_keep_best(False)
    # aoadmm_model_begin drops the list and the settings: criterion = 1 would refuse the solve without a list
    eng.rank_track(criterion=1)
    fit.start(pkg, eng)
    assert eng.ranklist_info(0)['nq'] == 0
    out = fit.solve(pkg, eng, 2)
    assert out['OuterIterations'] == 2 and eng.rank_trace(0)['iters'].tolist() == [] and eng.rank_trace(0)['best_iter'] == -1


@pytest.mark.parametrize('sparse', [False, True])
def test_parafac2_block_is_refused(pkg, eng, sparse):
    par2_block(pkg, eng, np.random.default_rng(13), sparse)
    with pytest.raises(pkg.UnsupportedOnDevice) as ei:
        eng.set_ranklist(0, 0, np.zeros((3, 3), dtype=np.int64))
    assert ei.value.code == capi.ERR_UNSUPPORTED and 'PARAFAC2' in str(ei.value)
    assert eng.ranklist_info(0)['nq'] == 0


def test_multi_device_context_is_refused(pkg):
    rng = np.random.default_rng(14)
    shape, R = (12, 10, 8), 3
    Z = cp_Z(shape, R, empty(pkg, shape))
    with pkg.Engine([0, 0]) as e:
        pkg.build_model(e, Z)
        pkg.upload_state(e, Z, {'fac': [rng.random((s, R)) for s in shape]})
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.set_ranklist(0, 0, queries(rng, shape, 5))
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.rank_track()
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.ranklist_last(0)
