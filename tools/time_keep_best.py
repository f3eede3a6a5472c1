"""Wall time of aoadmm_heldout_keep_best on a small coupled CP + PARAFAC2 model (the shapes of example_script1: CP
20 x 30 x 40, PARAFAC2 I = 20, K = 20, J_k = 30, R = 3, first modes coupled exactly, 22 state arrays).

    python3 tools/time_keep_best.py [--iters 40] [--reps 7] [--out profiles/heldout_keep_best_time.jsonl]

A list of held-out entries of the CP block is attached; solves of --iters iterations from the same starting point run with
the switch on and off, alternating.  Reported: the wall time per outer iteration of both (median, min, max over --reps),
the snapshot launches aoadmm_heldout_best_info counted (one per iteration at which the held-out sum improved, iteration 0
included), the state's bytes, and the added time per snapshot = (t_on - t_off) / launches of the medians.  The solves with
the switch on and off must return the same state bit for bit; one restore is timed at the end.
The one-launch snapshot against a chain of hipMemcpyAsync over the same arrays: tools/micro/snapshot_vs_memcpy.
"""
from __future__ import annotations

import argparse
import copy
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('matlab-code_amd')
from oracle import aoadmm as OA                      # noqa: E402  (the initialisation of the reference, on the host)
from oracle.tensor_ops import full_ktensor           # noqa: E402


def script1_model(rng, dims=(20, 30, 40), K=20, Jk=30, R=3, noise=0.1):
    I = dims[0]
    A = rng.random((I, R))
    X1 = full_ktensor([A, rng.random((dims[1], R)), rng.random((dims[2], R))])
    N = rng.standard_normal(X1.shape)
    X1 = X1 + noise * np.linalg.norm(X1) / np.linalg.norm(N) * N
    X1 /= np.linalg.norm(X1)
    Cm = rng.random((K, R)) + 0.1
    DB = rng.standard_normal((R, R))
    Xk = []
    for k in range(K):
        Q, _ = np.linalg.qr(rng.standard_normal((Jk, R)))
        Xk.append(A @ np.diag(Cm[k]) @ (Q @ DB).T)
    nrm = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in Xk))
    Xk = [x / nrm for x in Xk]
    NN = ('non-negativity',)
    Z = dict(loss_function=['Frobenius'] * 2, model=['CP', 'PAR2'], modes=[[1, 2, 3], [4, 5, 6]],
             size=[dims[0], dims[1], dims[2], I, [Jk] * K, K],
             coupling=dict(lin_coupled_modes=[1, 0, 0, 1, 0, 0], coupling_type=[0], coupl_trafo_matrices=[None] * 6),
             constrained_modes=[1, 1, 1, 1, 0, 1], constraints=[NN] * 4 + [None, NN], weights=[0.5, 0.5], object=[X1, Xk])
    distr = [lambda a, b: rng.random((a, b))] * 4 + [lambda a, b: rng.standard_normal((a, b)), lambda a, b: rng.random((a, b))]
    io = dict(lambdas_init=[[1] * R, [1] * R], nvecs=0, distr=distr, normalize=1)
    return Z, io


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'heldout_keep_best_time.jsonl'))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    Z, io = script1_model(rng)
    X1 = Z['object'][0]
    hold = rng.random(X1.shape) < 0.1
    subs, y = np.argwhere(hold), X1[hold]
    Z['object'][0] = np.where(hold, 0.0, X1)
    Z['miss'] = [~hold, None]                         # the held-out entries are kept out of the fit
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    Z['_ranks'] = [int((F[0] if isinstance(F, (list, tuple)) else F).shape[1]) for F in G['fac']]
    opt = dict(Display='no', MaxOuterIters=a.iters, MaxInnerIters=5, AbsFuncTol=0.0, OuterRelTol=0.0, innerRelPrTol_coupl=0.0,
               innerRelPrTol_constr=0.0, innerRelDualTol_coupl=0.0, innerRelDualTol_constr=0.0, bsum=0)

    def mmm(v):
        return [round(float(np.median(v)), 5), round(min(v), 5), round(max(v), 5)]

    with pkg.Engine(0) as eng:
        def solve(on):
            pkg.build_model(eng, Z)
            eng.set_heldout(0, subs, y)
            eng.heldout_keep_best(on)
            pkg.upload_state(eng, Z, copy.deepcopy(G))
            eng.synchronize()
            t0 = time.time()
            out = pkg.run_solver(eng, opt, len(Z['size']), has_missing=True)
            eng.synchronize()
            ms = (time.time() - t0) * 1e3
            return ms / out['OuterIterations'], eng.heldout_best_info(), pkg.download_state(eng, Z, G)

        solve(True), solve(False)                     # warm-up
        on, off = [], []
        for _ in range(a.reps):                       # alternating
            t, info, F_on = solve(True)
            on.append(t)
            t, _, F_off = solve(False)
            off.append(t)
            assert all(np.array_equal(x, z) for x, z in zip(F_on['fac'][:4], F_off['fac'][:4]))
        solve(True)
        t_restore = []
        for _ in range(a.reps):
            eng.synchronize()
            t0 = time.time()
            best = eng.heldout_restore_best()
            t_restore.append((time.time() - t0) * 1e3)
        state_bytes = info['bytes'] // (2 * info['launches'])
        added = (float(np.median(on)) - float(np.median(off))) * a.iters / info['launches']
        line = json.dumps({'what': 'keep_best_small_model', 'model': 'script1 shapes, CP block with Z.miss', 'iters': a.iters,
                           'reps': a.reps, 'state_bytes': state_bytes, 'snapshot_bytes_moved': 2 * state_bytes,
                           'snapshots': info['launches'], 'best_iter': best, 'iter_ms_wall_switch_on': mmm(on),
                           'iter_ms_wall_switch_off': mmm(off), 'added_us_per_snapshot': round(added * 1e3, 3),
                           'restore_ms_wall': mmm(t_restore)})
    print(line, flush=True)
    with open(a.out, 'a') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
