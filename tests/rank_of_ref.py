"""The numpy reference of `Engine.rank_of`: fp64 scores, then the number of candidates that come
before the target in lexsort((row, -score)).  Also the slab cut of the counting pass (topk_plan's rule, csrc/topk.hip)
so that a test can put targets on the first and last row of a slab."""
import numpy as np

TOL = 1e-12            # times sum_r prod_n |F_n|: the bar of test_gpu_topk ((R + N) 2^-53 derived)


def weights(U, mode, subs):
    W = np.ones((subs.shape[0], U[0].shape[1]))
    for m in range(len(U)):
        if m != mode:
            W = W * U[m][subs[:, m]]
    return W


def ref_rank_w(F, W, targets, exclude=None, with_scores=False):
    """(rank, score, ncand[, S I x nq]) for the weights W (nq x R) against the rows of F (I x R)."""
    with np.errstate(invalid='ignore'):
        S = F @ W.T
    I, nq = S.shape
    rank = np.full(nq, -1, dtype=np.int64)
    score = np.full(nq, np.nan)
    ncand = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        s = S[:, q]
        t = int(targets[q])
        ok = ~np.isnan(s)
        if exclude is not None:
            ok[np.asarray(exclude[1][exclude[0][q]:exclude[0][q + 1]], dtype=np.int64)] = False
        ok[t] = not np.isnan(s[t])                              # the target is a candidate, listed or not
        rows = np.flatnonzero(ok)
        ncand[q] = len(rows)
        score[q] = s[t]
        if ok[t]:
            order = rows[np.lexsort((rows, -s[rows]))]
            rank[q] = int(np.flatnonzero(order == t)[0])
    if with_scores:
        return rank, score, ncand, S
    return rank, score, ncand


def ref_rank(U, mode, subs, exclude=None, with_scores=False):
    return ref_rank_w(U[mode], weights(U, mode, subs), subs[:, mode], exclude, with_scores)


def well_separated(U, mode, subs, exclude=None):
    """The smallest |score(row) - score(target)| over the candidates other than the target, in units of twice the
    tolerance TOL sum_r prod_n |F_n| of the larger bound of the two; above 1 no rounding of the device's scores can move
    a rank.  Also returns the per-query tolerance of the target's score."""
    W = weights(U, mode, subs)
    S = U[mode] @ W.T
    B = np.abs(U[mode]) @ np.abs(W).T
    worst = np.inf
    tol_t = np.zeros(subs.shape[0])
    for q in range(subs.shape[0]):
        t = int(subs[q, mode])
        ok = np.ones(S.shape[0], dtype=bool)
        if exclude is not None:
            ok[np.asarray(exclude[1][exclude[0][q]:exclude[0][q + 1]], dtype=np.int64)] = False
        ok[t] = False
        tol_t[q] = TOL * B[t, q]
        if ok.any():
            need = 2.0 * TOL * np.maximum(B[ok, q], B[t, q])
            worst = min(worst, float(np.min(np.abs(S[ok, q] - S[t, q]) / need)))
    return worst, tol_t


def count_plan(I, nq):
    """(qt, qtiles, slabs, slab_rows) of the counting pass: topk_plan at its smallest k."""
    cdiv = lambda a, b: -(-a // b)
    qt = 2 if nq > 16 else 1
    qtiles = cdiv(nq, 16 * qt)
    slabs = max(1, cdiv(2048, qtiles))
    slabs = min(slabs, max(1, cdiv(I, 256)), 65535)
    slab_rows = cdiv(cdiv(I, slabs), 16) * 16
    return qt, qtiles, cdiv(I, slab_rows), slab_rows
