"""Time of the fold-in of new rows (csrc/foldin.hip, aoadmm_resident_fold_in) on one GPU, next to a residual pass of an
observed-only block over the same number of entries and to a torch baseline on the same device, in one process.

    python3 tools/time_foldin.py [--dims 1000000,100000,10000] [--R 20] [--nq 100000] [--nobs 10000000] [--reps 7]
                                 [--ridge 0.1] [--skip residual,torch,paths] [--out profiles/foldin_time.jsonl]
                                 [--weights] [--alpha 0.05]

A data-less block of --dims at rank R; --nq new rows of mode 0 are folded in from --nobs observations, once with the same
count for every query ('uniform') and once with counts that follow 1 / rank ('powerlaw': a few queries hold more than
10^5 observations and go through the split path, most hold a handful).  The list is given shuffled.  One line per case:
  `foldin_ms`  the kernels of one call: HIP events of aoadmm_kernel_stats(14), median (min, max) of --reps after one
               warm-up call; `ns_per_entry` and `gbytes_per_s` (the call's algorithmic bytes) follow from its median;
  `call_ms`    wall time of Engine.fold_in: the host's validation and counting sort, the uploads, the kernels, the rows back;
  `torch_ms`   chunked gather of the factor rows, einsum outer products, index_add_ into nq x R x R, torch.linalg.cholesky
               and cholesky_solve (torch events); `torch_max_rel` the largest row difference against the library;
  `residual_ns_per_entry`  the pass of an EM step of an observed-only block with --nobs stored entries over one sorted
               copy (class 4 + n, n >= 1: the residuals x - m alone), which gathers N rows per entry where the fold-in
               gathers N - 1.
'paths' times 256 and 257 observations per query (the largest fused query and the smallest split one) at the same total.
--weights and/or --alpha > 0 add, per case, one `foldin_weighted` line: the unweighted call, the call under uniform random
weights at alpha = 0 and (with --alpha) the call under the same weights at --alpha, on the same list, alternating call by
call in this process, --reps of each after one warm-up round; `h_ms` is the call with --alpha on one query without
observations, that is the launches that form H and one wave.
"""
from __future__ import annotations

import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FOLDIN_CLASS = 14


def med(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def make_list(rng, dims, counts):
    nobs = int(np.sum(counts))
    subs = np.stack([rng.integers(0, s, nobs) for s in dims], axis=1).astype(np.int64)
    subs[:, 0] = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    perm = rng.permutation(nobs)
    return np.asfortranarray(subs[perm]), rng.standard_normal(nobs)


def powerlaw_counts(nq, nobs):
    w = 1.0 / np.arange(1, nq + 1)
    c = np.floor(w / w.sum() * nobs).astype(np.int64)
    c[0] += nobs - c.sum()
    return c


def torch_fold_in(torch, Ft, subs_t, vals_t, nq, R, ridge, chunk):
    G = torch.zeros((nq, R, R), dtype=torch.float64, device=vals_t.device)
    b = torch.zeros((nq, R), dtype=torch.float64, device=vals_t.device)
    for c0 in range(0, vals_t.shape[0], chunk):
        s = subs_t[c0:c0 + chunk]
        z = Ft[0][s[:, 1]]
        for m in range(1, len(Ft)):
            z = z * Ft[m][s[:, m + 1]]
        G.index_add_(0, s[:, 0], torch.einsum('er,es->ers', z, z))
        b.index_add_(0, s[:, 0], z * vals_t[c0:c0 + chunk, None])
    G += ridge * torch.eye(R, dtype=torch.float64, device=vals_t.device)
    L = torch.linalg.cholesky(G)
    return torch.cholesky_solve(b[:, :, None], L)[:, :, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', default='1000000,100000,10000')
    ap.add_argument('--R', type=int, default=20)
    ap.add_argument('--nq', type=float, default=1e5)
    ap.add_argument('--nobs', type=float, default=1e7)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--ridge', type=float, default=0.1)
    ap.add_argument('--torch-chunk', type=float, default=1e6)
    ap.add_argument('--skip', default='')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--weights', action='store_true', help='time calls under entry weights against unweighted ones')
    ap.add_argument('--alpha', type=float, default=0.0, help='unstored weight of the weighted calls')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'foldin_time.jsonl'))
    a = ap.parse_args()
    skip = set(a.skip.split(',')) if a.skip else set()
    # torch (and the HIP runtime it ships) first, as bench.py does
    import torch
    torch.cuda.init()
    pkg = importlib.import_module('matlab-code_amd')
    capi = importlib.import_module('matlab-code_amd._capi')
    dims = tuple(int(v) for v in a.dims.split(','))
    N, R, nq, nobs = len(dims), a.R, int(a.nq), int(a.nobs)
    rng = np.random.default_rng(a.seed)
    U = [rng.standard_normal((s, R)) for s in dims]
    Z = dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, N + 1))], size=list(dims),
             coupling=dict(lin_coupled_modes=[0] * N, coupling_type=[], coupl_trafo_matrices=[None] * N),
             constrained_modes=[0] * N, constraints=[None] * N, weights=[1.0],
             object=[pkg.sptensor(np.zeros((0, N), dtype=np.int64), np.zeros(0), dims)], _ranks=[R] * N)
    dev = torch.device('cuda', 0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, 'a')

    def emit(line):
        print(json.dumps(line), flush=True)
        out.write(json.dumps(line) + '\n')
        out.flush()

    def time_fold(eng, subs, vals, n, **kw):
        t_dev, t_call, rows, by = [], [], None, 0.0
        for rep in range(a.reps + 1):                          # the first repetition warms up and is dropped
            eng.kernel_stats(FOLDIN_CLASS, reset=True)
            t0 = time.perf_counter()
            rows, info, _ = eng.fold_in(0, 0, subs, vals, nq=n, ridge=a.ridge, **kw)
            t1 = time.perf_counter()
            ms, launches, by, _ = eng.kernel_stats(FOLDIN_CLASS)
            assert launches == 1 and not info.any()
            if rep:
                t_dev.append(ms)
                t_call.append(1e3 * (t1 - t0))
        return med(t_dev), med(t_call), by, rows

    def time_alternating(eng, subs, vals, n, variants):
        """{name: median (min, max) of the kernels' ms} for calls that differ in their keywords, taken turn by turn."""
        t = {name: [] for name, _ in variants}
        for rep in range(a.reps + 1):                          # the first round warms up and is dropped
            for name, kw in variants:
                eng.kernel_stats(FOLDIN_CLASS, reset=True)
                rows, info, _ = eng.fold_in(0, 0, subs, vals, nq=n, ridge=a.ridge, **kw)
                ms, launches, by, _ = eng.kernel_stats(FOLDIN_CLASS)
                assert launches == 1 and not info.any()
                if rep:
                    t[name].append(ms)
        return {name: med(v) for name, v in t.items()}

    residual_ns = None
    if 'residual' not in skip:
        # an observed-only block of nobs stored entries of the same shape: the pass of an EM step over one copy
        with pkg.Engine(0) as obs:
            lib, h = obs.lib, obs.h
            capi.check(lib.aoadmm_model_begin(h, N, 1, 0))
            for m, s in enumerate(dims):
                capi.check(lib.aoadmm_model_set_mode(h, m, s, R))
            capi.check(lib.aoadmm_model_add_cp(h, 0, N, (C.c_int * N)(*range(N)), 1.0))
            for m in range(N):
                capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
            capi.check(lib.aoadmm_model_end(h))
            subs = np.stack([rng.integers(0, s, nobs) for s in dims], axis=1).astype(np.int64)
            obs.upload_coo(0, subs, rng.standard_normal(nobs))
            obs.set_observed_only(0)
            for m in range(N):
                Um = np.asfortranarray(rng.random((dims[m], R)))
                capi.check(lib.aoadmm_state_set(h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], R))
            o, res = capi.Options(), capi.Result()
            o.MaxOuterIters, o.MaxInnerIters, o.use_dimtree = 1, 1, 1
            capi.check(lib.aoadmm_solve(h, C.byref(o), C.byref(res)))   # row-major copies; the block takes its snapshot
            per = [[] for _ in range(N)]
            for rep in range(a.reps + 1):
                for c in [3] + [4 + n for n in range(N)]:
                    obs.kernel_stats(c, reset=True)
                obs.em_step(0)
                for n in range(N):
                    if rep:
                        per[n].append(obs.kernel_stats(4 + n)[0])
            stored = nobs                                      # random subscripts among prod(dims) positions: no duplicates to speak of
            residual_ns = med([1e6 * t / stored for t in per[1]])
            emit(dict(what='residual_pass', dims=list(dims), R=R, stored=int(stored), reps=a.reps,
                      pass_ms=[med(p) for p in per], ns_per_entry_mode2=residual_ns))
            del subs

    with pkg.Engine(0) as eng:
        pkg.build_model(eng, Z)
        pkg.upload_state(eng, Z, {'fac': U})
        Ft = [torch.from_numpy(U[m]).to(dev) for m in range(1, N)]
        cases = [('uniform', np.full(nq, nobs // nq, dtype=np.int64)), ('powerlaw', powerlaw_counts(nq, nobs))]
        for name, counts in cases:
            subs, vals = make_list(rng, dims, counts)
            m_dev, m_call, by, rows = time_fold(eng, subs, vals, nq)
            n = int(counts.sum())
            line = dict(what='foldin', case=name, dims=list(dims), R=R, N=N, nq=nq, nobs=n, ridge=a.ridge, reps=a.reps,
                        max_count=int(counts.max()), split_queries=int((counts > 256).sum()), foldin_ms=m_dev, call_ms=m_call,
                        ns_per_entry=round(1e6 * m_dev['median'] / n, 4), algorithmic_bytes=by,
                        gbytes_per_s=round(by / (m_dev['median'] * 1e-3) / 1e9, 1),
                        residual_ns_per_entry=residual_ns['median'] if residual_ns else None,
                        over_residual=round(1e6 * m_dev['median'] / n / residual_ns['median'], 3) if residual_ns else None)
            if 'torch' not in skip:
                subs_t, vals_t = torch.from_numpy(np.ascontiguousarray(subs)).to(dev), torch.from_numpy(vals).to(dev)
                t_torch, got = [], None
                for rep in range(a.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    got = torch_fold_in(torch, Ft, subs_t, vals_t, nq, R, a.ridge, int(a.torch_chunk))
                    e1.record()
                    torch.cuda.synchronize()
                    if rep:
                        t_torch.append(e0.elapsed_time(e1))
                diff = np.abs(got.cpu().numpy() - rows).max(axis=1) / np.maximum(np.abs(rows).max(axis=1), 1e-300)
                line.update(torch_ms=med(t_torch), torch_chunk=int(a.torch_chunk), torch_over_foldin=round(med(t_torch)['median'] / m_dev['median'], 2),
                            torch_max_rel=float(diff.max()))
                del subs_t, vals_t, got
                torch.cuda.empty_cache()
            emit(line)
            if a.weights or a.alpha > 0:
                w = rng.random(n)
                variants = [('unweighted', {}), ('weighted', dict(weights=w))]
                if a.alpha > 0:
                    variants.append(('weighted_alpha', dict(weights=w, unstored_weight=a.alpha)))
                t = time_alternating(eng, subs, vals, nq, variants)
                wline = dict(what='foldin_weighted', case=name, dims=list(dims), R=R, N=N, nq=nq, nobs=n, ridge=a.ridge, reps=a.reps,
                             alpha=a.alpha, foldin_ms=t, weighted_over_unweighted=round(t['weighted']['median'] / t['unweighted']['median'], 4),
                             expected_bytes_ratio=round((4.0 * (N - 1) + 16.0 + 8.0 * R * (N - 1)) / (4.0 * (N - 1) + 8.0 + 8.0 * R * (N - 1)), 4))
                if a.alpha > 0:
                    wline['alpha_over_unweighted'] = round(t['weighted_alpha']['median'] / t['unweighted']['median'], 4)
                    none = np.zeros((0, N), dtype=np.int64, order='F')
                    wline['h_ms'] = time_alternating(eng, none, np.zeros(0), 1, [('h', dict(unstored_weight=a.alpha))])['h']
                    wline['h_bytes'] = 8 * R * int(sum(dims[1:]))
                emit(wline)
        if 'paths' not in skip:
            for per_query in (256, 257):
                n = max(1, nobs // 4 // per_query)
                subs, vals = make_list(rng, dims, np.full(n, per_query, dtype=np.int64))
                m_dev, m_call, by, _ = time_fold(eng, subs, vals, n)
                emit(dict(what='foldin_paths', path='fused' if per_query <= 256 else 'split', per_query=per_query, nq=n, nobs=n * per_query,
                          R=R, N=N, reps=a.reps, foldin_ms=m_dev, call_ms=m_call, ns_per_entry=round(1e6 * m_dev['median'] / (n * per_query), 4)))
    out.close()


if __name__ == '__main__':
    main()
