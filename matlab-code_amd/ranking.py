"""Ranking metrics from the ranks `Engine.rank_of` returns, and the host statement of the rule a
solve applies to the ranking metric it tracks (section 9.8).  Host code: a few sums over nq integers."""
import math

import numpy as np


def ranking_metrics(rank, ncand=None, ks=(1, 5, 10)):
    """Hit-rate, NDCG, MRR and AUC of held-out entries from their 0-based ranks (one relevant row per query).

    rank[q] is the number of candidates that come before query q's target (`Engine.rank_of`); queries with rank = -1
    (a target whose score is NaN) are left out of everything.  Returns a dict with
      'n'       the number of queries used,
      'hit@k'   the mean of rank < k,
      'ndcg@k'  the mean of 1 / log2(rank + 2) where rank < k, else 0 (the ideal DCG of one relevant row is 1),
      'mrr'     the mean of 1 / (rank + 1),
    for every k of `ks`, and with `ncand` (the number of candidates per query) also
      'auc'     the mean of 1 - rank / (ncand - 1) over the queries with ncand >= 2: the share of the other candidates
                the target comes before,
      'n_auc'   the number of queries that mean is over.
    A mean over no query is NaN."""
    rank = np.asarray(rank, dtype=np.int64).reshape(-1)
    use = rank >= 0
    r = rank[use].astype(np.float64)
    n = int(r.shape[0])

    def mean(x):
        return float(np.mean(x)) if x.shape[0] else float('nan')

    out = {'n': n}
    for k in ks:
        k = int(k)
        hit = r < k
        out['hit@%d' % k] = mean(hit.astype(np.float64))
        out['ndcg@%d' % k] = mean(np.where(hit, 1.0 / np.log2(r + 2.0), 0.0))
    out['mrr'] = mean(1.0 / (r + 1.0))
    if ncand is not None:
        ncand = np.asarray(ncand, dtype=np.int64).reshape(-1)
        if ncand.shape[0] != rank.shape[0]:
            raise ValueError('ranking_metrics: %d ranks but %d candidate counts' % (rank.shape[0], ncand.shape[0]))
        sel = use & (ncand >= 2)
        out['auc'] = mean(1.0 - rank[sel] / (ncand[sel] - 1.0))
        out['n_auc'] = int(sel.sum())
    return out


def parse_rank_metric(spec):
    """'ndcg@10' -> ('ndcg', 10), 'hit@5' -> ('hit', 5), 'mrr' -> ('mrr', 10), 'auc' -> ('auc', 10): the metric a solve
    tracks and the cut-off k of hit and ndcg (default 10; mrr and auc take none).  ValueError for anything else."""
    if not isinstance(spec, str):
        raise ValueError("rank_metric must be a string such as 'ndcg@10', 'hit@5', 'mrr' or 'auc', got %r" % (spec,))
    name, at, ktxt = spec.strip().lower().partition('@')
    if name not in ('hit', 'ndcg', 'mrr', 'auc'):
        raise ValueError("rank_metric %r: the metric must be one of 'hit', 'ndcg', 'mrr', 'auc'" % (spec,))
    if not at:
        return name, 10
    if name in ('mrr', 'auc'):
        raise ValueError('rank_metric %r: %s takes no cut-off' % (spec, name))
    if not ktxt.isdigit():
        raise ValueError('rank_metric %r: the cut-off must be a positive integer' % (spec,))
    k = int(ktxt)
    if not 1 <= k < 2 ** 31:
        raise ValueError('rank_metric %r: k = %d outside [1, 2^31)' % (spec, k))
    return name, k


def pooled_score(traces, metric):
    """S per evaluation from the `Engine.rank_trace` dicts of all blocks with a list: the sum of the blocks' sums of
    `metric` ('hit', 'ndcg', 'mrr', 'auc') over the sum of their n (n_auc for auc); 0 / 0 is NaN.  Block weights do
    not enter."""
    key = {'hit': 'hits', 'ndcg': 'ndcg_sum', 'mrr': 'mrr_sum', 'auc': 'auc_sum'}[metric]
    num = sum(np.asarray(t[key], dtype=np.float64) for t in traces)
    den = sum(np.asarray(t['n_auc' if metric == 'auc' else 'n'], dtype=np.float64) for t in traces)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(den > 0, num / den, np.nan)


def rank_rule(scores, patience=0):
    """The best / patience rule of a solve on the scores S of its evaluations, in order (larger is better).  The first
    evaluation is the first best; a later one becomes the best only if its S is strictly larger, or if the best so far
    is NaN and it is not: a NaN never becomes the best, and a tie keeps the earlier evaluation.  With patience = n > 0
    the solve stops after the first evaluation at which S has not improved for n consecutive evaluations.  Returns
    (best, stop): the index of the best evaluation among those the solve reaches (-1 for no evaluation) and the index
    of the evaluation it stops after (None: the rule never fires)."""
    best, best_s, bad = -1, float('nan'), 0
    for e, s in enumerate(scores):
        s = float(s)
        if e == 0 or s > best_s or (math.isnan(best_s) and not math.isnan(s)):
            best, best_s, bad = e, s, 0
        else:
            bad += 1
        if e > 0 and patience > 0 and bad >= patience:
            return best, e
    return best, None
