"""Reference for weighted sparse CP blocks (aoadmm_tensor_set_entry_weights): the oracle
stepped one outer iteration at a time.  The oracle's own mask is boolean, so the weighted EM

    Xhat <- W o X + (1 - W) o M(F)          (cmtf_fun_AOADMM.m:408-441 with the majoriser of Srebro and Jaakkola)

is run around it: Xhat is held as a dense array, every outer iteration is one call of the oracle on Z with Xhat as the
object and no Z.miss, started from the state the call before returned.  With a boolean W the loop is the oracle's own EM
run (tests/test_sparse_weighted_host.py pins that bit for bit)."""
import copy

import numpy as np

from oracle import aoadmm as OA
from oracle.tensor_ops import full_ktensor


def dense_weights(shape, subs, wts, alpha):
    """W: wts on the stored entries subs (n x N, distinct), alpha everywhere else"""
    W = np.full(shape, float(alpha))
    W[tuple(np.asarray(subs).T)] = wts
    return W


def block_model(Z, F, p):
    return full_ktensor([F['fac'][m - 1] for m in Z['modes'][p]])


def stepped_em(Z, W, G, opt, iters):
    """Z: the model with every Z.object dense (the weighted blocks hold X); W: {0-based block: dense weights in [0, 1]};
    G: the initial state; opt: the options of the solve (MaxOuterIters is ignored: `iters` iterations are taken, so the
    tolerances of opt must be 0).  Returns (F, out) with out as the oracle's EM run would return it: func_val_conv is
    f_tensors with sum W o (X - M)^2 as the weighted blocks' term, func_rel_missing comes from
    num = ||(1 - W) o (M_new - M_old)||^2 and den = ||(1 - W) o M_old||^2 summed over the weighted blocks (M_old = 0
    before the first iteration), and 'wobj' / 'num' / 'den' hold the per-iteration values {block: list}."""
    X = {p: np.asarray(Z['object'][p], dtype=np.float64) for p in W}
    Xhat = {p: W[p] * X[p] for p in W}
    wt = [float(w) for w in Z['weights']]
    F = copy.deepcopy(G)
    one = dict(opt, MaxOuterIters=1)
    fv, fcoupl, fconstr, frm, inner = [], [], [], [float('nan')], []
    wobj = {p: [] for p in W}
    nums, dens = {p: [] for p in W}, {p: [] for p in W}

    def tensors_term(f_oracle, F_at):
        # the oracle's f_tensors holds w_p ||Xhat_p - M_p||^2 for a weighted block: swap it for w_p sum W o (X - M)^2
        f = f_oracle
        for p in W:
            M = block_model(Z, F_at, p)
            obj = float(np.sum(W[p] * (X[p] - M) ** 2))
            f += wt[p] * (obj - float(np.sum((Xhat[p] - M) ** 2)))
            wobj[p].append(obj)
        return f

    for it in range(iters):
        Zs = dict(Z, object=list(Z['object']), miss=None)
        for p in W:
            Zs['object'][p] = Xhat[p].copy()
        _, Fn, _, out = OA.cmtf_AOADMM(Zs, alg_options=one, init=copy.deepcopy(F))
        if it == 0:
            fv.append(tensors_term(out['func_val_conv'][0], F))
            fcoupl.append(out['func_coupl_conv'][0]); fconstr.append(out['func_constr_conv'][0])
        fv.append(tensors_term(out['func_val_conv'][-1], Fn))       # Xhat is still the one this iteration fitted
        fcoupl.append(out['func_coupl_conv'][-1]); fconstr.append(out['func_constr_conv'][-1])
        inner.append(out['innerIters'][:, :1])
        num = den = 0.0
        for p in W:
            old = Xhat[p] - W[p] * X[p]                              # (1 - W) o M_old, 0 before the first iteration
            new = (1.0 - W[p]) * block_model(Z, Fn, p)
            nums[p].append(float(np.sum((new - old) ** 2))); dens[p].append(float(np.sum(old ** 2)))
            num += nums[p][-1]; den += dens[p][-1]
            Xhat[p] = W[p] * X[p] + new
        frm.append(float(np.sqrt(num / den)) if den > 0 else float(np.sqrt(num)))
        F = Fn
    res = dict(OuterIterations=iters, func_val_conv=np.array(fv), func_coupl_conv=np.array(fcoupl),
               func_constr_conv=np.array(fconstr), func_rel_missing=np.array(frm), f_rel_missing=frm[-1],
               innerIters=np.hstack(inner) if inner else np.zeros((len(Z['size']), 1)), wobj=wobj, num=nums, den=dens)
    return F, res
