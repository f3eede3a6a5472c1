"""Ranking metrics from the ranks `Engine.rank_of` returns.  Host code: a few sums over nq
integers."""
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
