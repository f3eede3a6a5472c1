"""Time of the fold-in of new PARAFAC2 slabs (csrc/par2_foldin.hip, aoadmm_resident_par2_fold_in) on one GPU, next to a
torch restatement on the same device, in one process.

    python3 tools/time_par2_foldin.py [--shape a|b] [--reps 7] [--max-iter 5] [--skip torch,solve]
                                      [--out profiles/par2_foldin_time.jsonl]
    python3 tools/time_par2_foldin.py --kernel-csv <rocprofv3 kernel_stats.csv> --shape a|b

Shapes: (a) I = 40, J_q cycled over 61..120, R = 3, nk = 4096 (BASELINE config 4's slabs); (b) I = J = 2000, R = 20, nk = 64.
One line per run:
  `call_dev_ms`   the kernels of one call: HIP events of aoadmm_kernel_stats(17), median (min, max) of --reps after one
                  warm-up call, at max_iter = --max-iter and tol = 0 (every slab takes every iteration);
  `call_ms`       wall time of Engine.par2_fold_in: packing, the upload of the slabs, the kernels, the outputs back;
  `torch_ms`      Y = X'A by bmm, then per iteration W, batched torch.linalg.svd, P = U V', B, b and a Cholesky solve of the
                  shared system, the slabs batched by J (torch events); `torch_max_rel` the largest row difference;
  `stream_ms`     the slab bytes at the 7.1 TB/s plain-read figure of DESIGN.md section 6.
Unless skipped, one outer iteration of a solve of a block made of the same slabs follows, so that a run under
`rocprofv3 --kernel-trace --stats` holds par2_xta_k (the solver's kernel for the same product X_k'A) beside par2_fold_y_k;
--kernel-csv turns that table into a `kernels` line (average ns per launch of the kernels named here).
"""
from __future__ import annotations

import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASS = 17
PLAIN_READ_TBS = 7.1
KERNELS = ('par2_fold_y_k', 'par2_fold_alt_k', 'par2_fold_system_k', 'par2_fold_ysum_k', 'par2_xta_k')


def med(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def shape_of(name):
    if name == 'a':
        return 40, 3, [61 + q % 60 for q in range(4096)]
    return 2000, 20, [2000] * 64


def make(rng, I, R, Js):
    A = rng.standard_normal((I, R))
    Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    DB = Q + 0.1 * rng.standard_normal((R, R))
    slabs = []
    for J in Js:
        P, _ = np.linalg.qr(rng.standard_normal((J, R)))
        X = (A * (0.75 + 0.5 * rng.random(R))) @ (P @ DB).T
        N = rng.standard_normal(X.shape)
        slabs.append(X + 0.05 * np.linalg.norm(X) / np.linalg.norm(N) * N)
    return A, DB, slabs


def par2_Z(I, R, Jk, slabs):
    return dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=[I, list(Jk), len(Jk)],
                coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
                constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[slabs], _ranks=[R] * 3)


def torch_fold_in(torch, A, DB, groups, max_iter):
    S = (A.T @ A) * (DB.T @ DB)
    L = torch.linalg.cholesky(S)
    rows = {}
    for J, (idx, X) in groups.items():
        Y = torch.matmul(X.transpose(1, 2), A)                       # n x J x R
        c = torch.ones((X.shape[0], A.shape[1]), dtype=torch.float64, device=A.device)
        for _ in range(max_iter):
            W = torch.matmul(Y * c[:, None, :], DB.T)
            U, _, Vh = torch.linalg.svd(W, full_matrices=False)
            B = torch.matmul(torch.matmul(U, Vh), DB)
            b = (Y * B).sum(dim=1)
            c = torch.cholesky_solve(b.T, L).T
        rows[J] = (idx, c)
    return rows


def kernel_lines(path, shape):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Name', '')
            for k in KERNELS:
                if k in name:
                    e = rows.setdefault(k, dict(calls=0, total_ns=0.0))
                    e['calls'] += int(r['Calls'])
                    e['total_ns'] += float(r['TotalDurationNs'])
    for e in rows.values():
        e['avg_ns'] = round(e['total_ns'] / max(e['calls'], 1), 1)
    return dict(what='kernels', shape=shape, kernels=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='a', choices=['a', 'b'])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-iter', type=int, default=5)
    ap.add_argument('--skip', default='')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--kernel-csv', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'par2_foldin_time.jsonl'))
    a = ap.parse_args()
    skip = set(a.skip.split(',')) if a.skip else set()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, 'a')

    def emit(line):
        print(json.dumps(line), flush=True)
        out.write(json.dumps(line) + '\n')
        out.flush()

    if a.kernel_csv:
        emit(kernel_lines(a.kernel_csv, a.shape))
        return
    # torch (and the HIP runtime it ships) first, as bench.py does
    import torch
    torch.cuda.init()
    pkg = importlib.import_module('matlab-code_amd')
    I, R, Js = shape_of(a.shape)
    rng = np.random.default_rng(a.seed)
    A, DB, slabs = make(rng, I, R, Js)
    nk, Jtot = len(Js), int(sum(Js))
    dev = torch.device('cuda', 0)
    with pkg.Engine(0) as eng:
        Zs = par2_Z(I, R, [R, R + 1], [np.zeros((I, R)), np.zeros((I, R + 1))])
        pkg.build_model(eng, Zs)
        cells = [np.zeros((R, R)), np.zeros((R + 1, R))]
        pkg.upload_state(eng, Zs, {'fac': [A, cells, np.ones((2, R))], 'DeltaB': {0: DB}, 'P': {0: cells}, 'mu_DeltaB': {0: cells}})
        t_dev, t_call, res = [], [], None
        for rep in range(a.reps + 1):                              # the first repetition warms up and is dropped
            eng.kernel_stats(CLASS, reset=True)
            t0 = time.perf_counter()
            res = eng.par2_fold_in(0, slabs, max_iter=a.max_iter, tol=0.0, return_B=False)
            t1 = time.perf_counter()
            ms, launches, by, fl = eng.kernel_stats(CLASS)
            assert launches == 1 and not res['info'].any() and np.all(res['iters'] == a.max_iter)
            if rep:
                t_dev.append(ms)
                t_call.append(1e3 * (t1 - t0))
        m_dev = med(t_dev)
        slab_bytes = 8.0 * I * Jtot
        line = dict(what='par2_foldin', shape=a.shape, I=I, R=R, nk=nk, Jtot=Jtot, max_iter=a.max_iter, reps=a.reps, path=list(res['path']),
                    call_dev_ms=m_dev, call_ms=med(t_call), algorithmic_bytes=by, flops=fl, slab_bytes=slab_bytes,
                    stream_ms=round(slab_bytes / (PLAIN_READ_TBS * 1e12) * 1e3, 5), mean_fit=float(np.mean(res['fit'])))
        if 'torch' not in skip:
            At, DBt = torch.from_numpy(A).to(dev), torch.from_numpy(DB).to(dev)
            groups = {}
            for J in sorted(set(Js)):
                idx = [q for q in range(nk) if Js[q] == J]
                groups[J] = (idx, torch.from_numpy(np.stack([slabs[q] for q in idx])).to(dev))
            t_torch, got = [], None
            for rep in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                got = torch_fold_in(torch, At, DBt, groups, a.max_iter)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    t_torch.append(e0.elapsed_time(e1))
            Ct = np.zeros((nk, R))
            for J, (idx, c) in got.items():
                Ct[idx] = c.cpu().numpy()
            rel = np.abs(Ct - res['C']).max(axis=1) / np.abs(res['C']).max(axis=1)
            line.update(torch_ms=med(t_torch), torch_over_call=round(med(t_torch)['median'] / m_dev['median'], 2), torch_max_rel=float(rel.max()))
            del groups, got
            torch.cuda.empty_cache()
        emit(line)
        if 'solve' not in skip:
            # one outer iteration of a solve over the same slabs: par2_xta_k forms X_k'A D_k there
            from oracle import aoadmm as OA
            Z = par2_Z(I, R, Js, slabs)
            io = dict(lambdas_init=[[1] * R], nvecs=0, distr=[lambda r, c: rng.standard_normal((r, c))] * 3, normalize=1)
            G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=rng)
            opt = dict(Display='no', DisplayIters=10, MaxOuterIters=1, MaxInnerIters=5, AbsFuncTol=0.0, OuterRelTol=0.0,
                       innerRelPrTol_coupl=0.0, innerRelPrTol_constr=0.0, innerRelDualTol_coupl=0.0, innerRelDualTol_constr=0.0,
                       bsum=0, eps_log=1e-10)
            pkg.cmtf_AOADMM(Z, alg_options=opt, init=G, engine=eng)
            emit(dict(what='solve_iteration', shape=a.shape, note='one outer iteration over the same slabs (par2_xta_k in the kernel table)'))
    out.close()


if __name__ == '__main__':
    main()
