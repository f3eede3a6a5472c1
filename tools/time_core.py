#!/usr/bin/env python3
"""Time of the Tucker projection of a resident block (csrc/core.hip, aoadmm_resident_project) on one GPU, next to two
baselines measured in the same process: the unchanged tensor pass of the same block and torch doing the same three
contractions on the same device.

    python3 tools/time_core.py [--size 2000] [--R 20] [--reps 5] [--nnz 10000000] [--sparse-shape 100000,10000,1000]
                               [--skip dense-f32,dense-f16,sparse] [--out profiles/core_time.jsonl]

Dense (one CP block size^3, synthetic data generated in HBM, stored fp32 and then fp16), per repetition:
  `call_ms`     wall time of Engine.project: the upload of the three matrices, the pass, the fold, the download;
  `pass_ms`     the tensor pass inside the call (aoadmm_kernel_stats(0) or (1), every pass bracketed by events);
  `fold_ms`     the core fold over T inside the call (aoadmm_kernel_stats(2));
  `mttkrp_pass_ms`  the pass of aoadmm_resident_mttkrp on the same block at the same rank: the unchanged pass;
  `torch_ms`    torch events around three matmuls on a torch tensor of the block's shape and precision (random data:
                a time, not a check), X_(3)' M2, then mode 2, then mode 1; fp16 operands for the fp16 block.
Sparse (10^7 nonzeros, uniform subscripts):
  `call_ms`, `mttkrp_ms` (the R MTTKRPs of the call, aoadmm_kernel_stats(3)), `one_mttkrp_ms` (aoadmm_resident_mttkrp of
  the same mode), `torch_ms` (chunks of 10^6 nonzeros: (x o M0[i])' (M1[j] kr M2[k]), a 20 x 400 GEMM per chunk).
The first repetition warms up and is dropped; medians (min, max) over the rest.  One JSON line per case to stdout and
appended to --out."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('AOADMM_PASS_EVENT_EVERY', '1')


def med(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def cp_block(shape, R, obj):
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[[1, 2, 3]], size=list(shape),
                coupling=dict(lin_coupled_modes=[0] * 3, coupling_type=[], coupl_trafo_matrices=[None] * 3),
                constrained_modes=[0] * 3, constraints=[None] * 3, weights=[1.0], object=[obj], _ranks=[R] * 3)


def pass_ms(eng):
    """(ms, launches) of the tensor passes since the last reset, either kernel"""
    a, b = eng.kernel_stats(0), eng.kernel_stats(1)
    return a[0] + b[0], a[1] + b[1]


def dense(pkg, torch, a, prec, emit):
    N, R = a.size, a.R
    shape = (N, N, N)
    rng = np.random.default_rng(0)
    M = [rng.standard_normal((n, R)) for n in shape]
    dev = torch.device('cuda', 0)
    tdt = torch.float16 if prec == 'f16' else torch.float32
    with pkg.Engine(0) as eng:
        Z = cp_block(shape, R, dict(synthetic=True, rank=R, seed=0, noise=0.05))
        pkg.build_model(eng, Z, prec)
        pkg.upload_state(eng, Z, {'fac': M})
        eng.kernel_stats(2)                                       # from here on the reductions over T are timed
        Xt = torch.empty(shape, dtype=tdt, device=dev).normal_()
        Mt = [torch.from_numpy(m).to(dev).to(tdt) for m in M]
        t_call, t_pass, t_fold, t_mt, t_torch = [], [], [], [], []
        for rep in range(a.reps + 1):
            for w in (0, 1, 2):
                eng.kernel_stats(w, reset=True)
            t0 = time.perf_counter()
            eng.project(0, M)
            t1 = time.perf_counter()
            p_ms, p_n = pass_ms(eng)
            f_ms, f_n = eng.kernel_stats(2)[:2]
            assert (p_n, f_n) == (1, 1), (p_n, f_n)
            for w in (0, 1):
                eng.kernel_stats(w, reset=True)
            eng.resident_mttkrp(0, 0, N, R)
            m_ms, m_n = pass_ms(eng)
            assert m_n == 1, m_n
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            T = (Xt.reshape(N * N, N) @ Mt[2]).reshape(N, N, R)              # (i, j, r)
            V = torch.einsum('ijr,jq->iqr', T, Mt[1])
            G = torch.einsum('iqr,ip->pqr', V, Mt[0]).float()
            e1.record()
            torch.cuda.synchronize()
            del T, V, G
            if rep:
                t_call.append(1e3 * (t1 - t0)); t_pass.append(p_ms); t_fold.append(f_ms); t_mt.append(m_ms)
                t_torch.append(e0.elapsed_time(e1))
        dev_ms = med([p + f for p, f in zip(t_pass, t_fold)])
        emit(what='project', block='dense', precision=prec, size=N, R=R, reps=a.reps, call_ms=med(t_call), pass_ms=med(t_pass),
             fold_ms=med(t_fold), device_ms=dev_ms, mttkrp_pass_ms=med(t_mt), torch_ms=med(t_torch),
             fold_over_pass=round(med(t_fold)['median'] / med(t_pass)['median'], 3),
             device_over_mttkrp_pass=round(dev_ms['median'] / med(t_mt)['median'], 3),
             torch_over_device=round(med(t_torch)['median'] / dev_ms['median'], 3),
             t_bytes=float(N) * N * R * 4, fold_flops=2.0 * N * N * R * R + 2.0 * N * R ** 3)
        del Xt
        torch.cuda.empty_cache()


def sparse(pkg, torch, a, emit):
    shape = tuple(int(v) for v in a.sparse_shape.split(','))
    R, nnz = a.R, int(a.nnz)
    rng = np.random.default_rng(1)
    subs = np.stack([rng.integers(0, s, nnz) for s in shape], axis=1).astype(np.int64)
    vals = rng.standard_normal(nnz)
    M = [rng.standard_normal((n, R)) for n in shape]
    dev = torch.device('cuda', 0)
    with pkg.Engine(0) as eng:
        Z = cp_block(shape, R, pkg.sptensor(subs, vals, shape))
        pkg.build_model(eng, Z)
        pkg.upload_state(eng, Z, {'fac': M})
        st = [torch.from_numpy(np.ascontiguousarray(subs[:, n])).to(dev) for n in range(3)]
        vt = torch.from_numpy(vals).to(dev)
        Mt = [torch.from_numpy(m).to(dev) for m in M]
        t_call, t_mt, t_one, t_torch = [], [], [], []
        for rep in range(a.reps + 1):
            eng.kernel_stats(3, reset=True)
            t0 = time.perf_counter()
            eng.project(0, M)
            t1 = time.perf_counter()
            ms, n = eng.kernel_stats(3)[:2]
            assert n == R, n
            eng.kernel_stats(3, reset=True)
            eng.resident_mttkrp(0, 0, shape[0], R)
            one = eng.kernel_stats(3)[0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            G = torch.zeros((R, R * R), dtype=torch.float64, device=dev)
            for c0 in range(0, nnz, 1_000_000):
                s = slice(c0, c0 + 1_000_000)
                A = vt[s, None] * Mt[0][st[0][s]]
                B = (Mt[1][st[1][s]][:, :, None] * Mt[2][st[2][s]][:, None, :]).reshape(-1, R * R)
                G += A.T @ B
            e1.record()
            torch.cuda.synchronize()
            if rep:
                t_call.append(1e3 * (t1 - t0)); t_mt.append(ms); t_one.append(one); t_torch.append(e0.elapsed_time(e1))
        emit(what='project', block='sparse', shape=list(shape), nnz=nnz, R=R, reps=a.reps, call_ms=med(t_call), mttkrp_ms=med(t_mt),
             one_mttkrp_ms=med(t_one), torch_ms=med(t_torch),
             call_over_R_mttkrps=round(med(t_call)['median'] / (R * med(t_one)['median']), 3),
             torch_over_call=round(med(t_torch)['median'] / med(t_call)['median'], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=2000)
    ap.add_argument('--R', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--nnz', type=float, default=1e7)
    ap.add_argument('--sparse-shape', default='100000,10000,1000')
    ap.add_argument('--skip', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'core_time.jsonl'))
    a = ap.parse_args()
    import torch                                                  # torch (and the HIP runtime it ships) first, as bench.py does
    torch.cuda.init()
    pkg = importlib.import_module('matlab-code_amd')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        with open(a.out, 'a') as f:
            f.write(json.dumps(kw) + '\n')

    skip = set(a.skip.split(',')) if a.skip else set()
    if 'dense-f32' not in skip:
        dense(pkg, torch, a, 'f32', emit)
    if 'dense-f16' not in skip:
        dense(pkg, torch, a, 'f16', emit)
    if 'sparse' not in skip:
        sparse(pkg, torch, a, emit)


if __name__ == '__main__':
    main()
