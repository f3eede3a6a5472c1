"""Time of the ranks of held-out entries along one mode (csrc/rank_of.hip, aoadmm_resident_rank_of) on one GPU, next to
`aoadmm_resident_topk` at k = 10 and a torch baseline, in the same process on the same GPU.

    python3 tools/time_rank_of.py [--rows 1000000] [--R 20] [--nq 1,16,1024,16384] [--excl 0,100] [--reps 7]
                                  [--peak-tflops 0] [--out profiles/rank_of_time.jsonl]

The block is 3-way, rows x 1000 x 1000, and holds no data: the calls read factors only.  Factors are standard normal,
the free mode is the first one, targets are uniform over the rows.  Per (nq, excluded rows per query): the median
(min, max) over --reps of
  `rank_ms`   the launches of one rank_of call (weights, targets' scores, counting pass, exclusion pass, finisher): HIP
              events of aoadmm_kernel_stats(13) around them on the library's stream;
  `call_ms`   the wall time of the whole call: host-side checks and sorting of the lists, uploads, device allocations,
              the launches, the download of the answer;
  `topk_ms`   the same events around one topk call at k = --k with the same queries and lists;
  `torch_ms`  S = W_c @ F.T, (S > S[q, t_q]).sum(1) over chunks c of at most --chunk queries (the c x rows fp64 score
              array of a chunk must fit), torch events around the loop.  W is given to torch ready-made and nothing is
              excluded: the baseline does less than the call.
The three alternate inside a repetition.  `tflops` = 2 rows nq R / rank_ms, `topk_tflops` likewise; with --peak-tflops P
(the fp64 rate tools/micro/mfma_rate.hip measured on the same machine) `of_peak` = tflops / P.  `equal_rank` says
whether torch's counts agree with the library's ranks (only asked without exclusions; standard normal scores have no
ties).  Prints one JSON line per (nq, excl); every line also goes to --out.
"""
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

STATS_CLASS = 13


def med(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=float, default=1e6)
    ap.add_argument('--R', type=int, default=20)
    ap.add_argument('--nq', default='1,16,1024,16384')
    ap.add_argument('--excl', default='0,100')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=1024)
    ap.add_argument('--peak-tflops', type=float, default=0.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank_of_time.jsonl'))
    a = ap.parse_args()
    # torch (and the HIP runtime it ships) first, as bench.py does
    import torch
    torch.cuda.init()
    pkg = importlib.import_module('matlab-code_amd')
    I, R = int(a.rows), a.R
    shape = (I, 1000, 1000)
    rng = np.random.default_rng(a.seed)
    U = [rng.standard_normal((s, R)) for s in shape]
    Z = dict(loss_function=['Frobenius'], model=['CP'], modes=[[1, 2, 3]], size=list(shape),
             coupling=dict(lin_coupled_modes=[0] * 3, coupling_type=[], coupl_trafo_matrices=[None] * 3),
             constrained_modes=[0] * 3, constraints=[None] * 3, weights=[1.0],
             object=[pkg.sptensor(np.zeros((0, 3), dtype=np.int64), np.zeros(0), shape)], _ranks=[R] * 3)
    dev = torch.device('cuda', 0)
    Ft = torch.from_numpy(U[0]).to(dev)
    lines = []
    with pkg.Engine(0) as eng:
        pkg.build_model(eng, Z)
        pkg.upload_state(eng, Z, {'fac': U})
        for nq in [int(v) for v in a.nq.split(',')]:
            subs = np.stack([rng.integers(0, s, nq) for s in shape], axis=1).astype(np.int64)
            Wt = torch.from_numpy(U[1][subs[:, 1]] * U[2][subs[:, 2]]).to(dev)
            tt = torch.from_numpy(subs[:, 0]).to(dev)
            for ne in [int(v) for v in a.excl.split(',')]:
                ex = None
                if ne:
                    ex = (np.arange(nq + 1, dtype=np.int64) * ne, rng.integers(0, I, nq * ne).astype(np.int64))
                t_dev, t_call, t_topk, t_torch = [], [], [], []
                rank = trank = None
                for rep in range(a.reps + 1):                  # the first repetition warms all three up and is dropped
                    eng.kernel_stats(STATS_CLASS, reset=True)
                    t0 = time.perf_counter()
                    rank, score, ncand = eng.rank_of(0, 0, subs, exclude=ex)
                    t1 = time.perf_counter()
                    ms, launches, by, fl = eng.kernel_stats(STATS_CLASS, reset=True)
                    eng.topk(0, 0, subs, a.k, exclude=ex)
                    ms_topk = eng.kernel_stats(STATS_CLASS)[0]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    parts = []
                    for c0 in range(0, nq, a.chunk):
                        S = Wt[c0:c0 + a.chunk] @ Ft.T
                        s = S.gather(1, tt[c0:c0 + a.chunk, None])
                        parts.append((S > s).sum(1))
                    e1.record()
                    torch.cuda.synchronize()
                    trank = torch.cat(parts).cpu().numpy()
                    del parts, S
                    if rep:
                        t_dev.append(ms)
                        t_call.append(1e3 * (t1 - t0))
                        t_topk.append(ms_topk)
                        t_torch.append(e0.elapsed_time(e1))
                m, mt = med(t_dev), med(t_topk)
                tfl = 2.0 * I * nq * R / (m['median'] * 1e-3) / 1e12
                line = dict(what='rank_of', rows=I, R=R, N=3, nq=nq, excl_per_query=ne, reps=a.reps, rank_ms=m, call_ms=med(t_call),
                            topk_k=a.k, topk_ms=mt, torch_ms=med(t_torch), torch_chunk=min(a.chunk, nq),
                            topk_over_rank=round(mt['median'] / m['median'], 3), torch_over_rank=round(med(t_torch)['median'] / m['median'], 3),
                            tflops=round(tfl, 3), topk_tflops=round(2.0 * I * nq * R / (mt['median'] * 1e-3) / 1e12, 3),
                            of_peak=round(tfl / a.peak_tflops, 4) if a.peak_tflops > 0 else None, peak_tflops=a.peak_tflops or None,
                            algorithmic_bytes=by, flops=fl, equal_rank=bool(np.array_equal(rank, trank)) if not ne else None)
                print(json.dumps(line), flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
