#!/usr/bin/env python3
"""fp16 against fp32 tensor storage on the headline workload (bench.py: one CP block N^3, rank 20, synthetic data
generated in HBM with 5 % noise, TV on mode 1, non-negativity on modes 2 and 3, MaxInnerIters 5), measured in ONE
process with the two modes alternating.

Two engines on the same device hold the same synthetic tensor (same seed), one stored fp32 (AOADMM_PREC_F32) and one
fp16 (AOADMM_PREC_F16), and start from the same factors.  Per mode:
  upload_s           aoadmm_tensor_synth including the pass copies (host clock around a call that ends synchronised)
  resident_bytes     aoadmm_tensor_storage_info
  factor gap         after --gap-iters outer iterations from the common start: two different data sets (the fp16 block
                     is the fp32 block quantised to 11 bits, 2e-4 relative), not an error of either mode
and per round of --steps outer iterations (host clock around a solve that ends with the read-back of the objective):
  iter_ms            time per outer iteration
  pass_ms, pass_TBs  mean tensor-pass time and algorithmic bytes over it, from aoadmm_kernel_stats(0) with every pass
                     bracketed by events (AOADMM_PASS_EVENT_EVERY=1)
--as-rank R --of N measures ONE RANK'S SHARE of an N-GPU job instead (bench.py's option of the same name): both engines
join a one-rank communicator through aoadmm_comm_init_rank_share before the model is built, hold rank R's rows and its
mode-3 slab, and run every collective without peers.  Such a run is a measurement, not a solve: its sums are partial.
After the timed rounds one more round per mode runs with the reductions over T timed as well (aoadmm_kernel_stats(2)),
so that a share whose iteration falls short of the pass ratio shows where the rest of the time goes.
Raw lines go to --out (JSON lines), a summary to stdout."""
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
os.environ.setdefault('AOADMM_PASS_EVENT_EVERY', '1')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=2000)
    ap.add_argument('--rank', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10, help='outer iterations per timed round')
    ap.add_argument('--rounds', type=int, default=5, help='timed rounds per mode, alternating')
    ap.add_argument('--gap-iters', type=int, default=25)
    ap.add_argument('--as-rank', type=int, default=-1, help="measure rank R's share of an N-GPU job (needs --of)")
    ap.add_argument('--of', type=int, default=0, help='number of ranks of the job whose share is measured')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'f16_time_%s.jsonl' % time.strftime('%Y%m%d_%H%M%S')))
    args = ap.parse_args()
    share = args.as_rank >= 0
    if share and not (args.of > 1 and args.as_rank < args.of):
        raise SystemExit('time_f16.py: --as-rank R needs --of N with 0 <= R < N, N > 1')
    pkg = importlib.import_module('matlab-code_amd')
    N, R = args.size, args.rank
    Z = dict(loss_function=['Frobenius'], model=['CP'], modes=[[1, 2, 3]], size=[N, N, N],
             coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
             constrained_modes=[1, 1, 1],
             constraints=[('TV regularization', 0.001), ('non-negativity',), ('non-negativity',)],
             weights=[1.0], object=[dict(synthetic=True, rank=R, seed=0, noise=0.05)], _ranks=[R] * 3)
    rng = np.random.default_rng(1)
    io = dict(lambdas_init=[[1] * R], nvecs=0, distr=[lambda a, b: rng.random((a, b))] * 3, normalize=1)
    G0 = pkg.init_coupled_AOADMM_CMTF(Z, io, rng=rng)

    def opts(n):
        return dict(MaxOuterIters=n, MaxInnerIters=5, AbsFuncTol=0.0, OuterRelTol=0.0, innerRelPrTol_coupl=0.0,
                    innerRelPrTol_constr=0.0, innerRelDualTol_coupl=0.0, innerRelDualTol_constr=0.0, bsum=0)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, 'w')

    def emit(**kw):
        log.write(json.dumps(kw) + '\n')
        log.flush()
        print(json.dumps(kw), flush=True)

    modes = ('f32', 'f16')
    eng, fac = {}, {}
    for m in modes:
        eng[m] = pkg.Engine(0)
        if share:
            eng[m].comm_init_rank_share(eng[m].comm_unique_id(), args.as_rank, args.of)
        t0 = time.perf_counter()
        pkg.build_model(eng[m], Z, m)
        eng[m].synchronize()
        up = time.perf_counter() - t0
        prec, scale, nbytes = eng[m].tensor_storage_info(0)
        emit(kind='storage', mode=m, size=N, rank=R, as_rank=args.as_rank, of=args.of, upload_s=up, precision=prec,
             scale=scale, resident_bytes=nbytes,
             bytes_per_entry=nbytes / float(N) ** 3)
        pkg.upload_state(eng[m], Z, copy.deepcopy(G0))
    # the factor gap, which is also the warm-up of every kernel the timed rounds use
    for m in modes:
        out = pkg.run_solver(eng[m], opts(args.gap_iters), 3)
        fac[m] = pkg.download_state(eng[m], Z, G0)['fac']
        emit(kind='after_gap_iters', mode=m, iters=int(out['OuterIterations']), f_tensors=float(out['f_tensors']))
    gap = [float(np.linalg.norm(a - b) / np.linalg.norm(b)) for a, b in zip(fac['f16'], fac['f32'])]
    emit(kind='factor_gap', iters=args.gap_iters, rel_fro_per_mode=gap,
         note='two different data sets: the fp16 block is the fp32 block quantised (2e-4 relative)')
    rows = {m: [] for m in modes}
    for rnd in range(args.rounds):
        for m in modes:
            e = eng[m]
            e.kernel_stats(0, reset=True)
            e.kernel_stats(1, reset=True)
            e.synchronize()
            t0 = time.perf_counter()
            out = pkg.run_solver(e, opts(args.steps), 3)
            e.synchronize()
            dt = time.perf_counter() - t0
            ms, launches, nbytes, flops = e.kernel_stats(0)
            assert out['OuterIterations'] == args.steps and e.kernel_stats(1)[1] == 0
            row = dict(kind='round', round=rnd, mode=m, steps=args.steps, iter_ms=dt / args.steps * 1e3, passes=launches,
                       pass_ms=ms / launches, pass_bytes=nbytes / launches, pass_TBs=nbytes / ms * 1e-9,
                       pass_TFs=flops / ms * 1e-9)
            rows[m].append(row)
            emit(**row)
    med = {m: {k: float(np.median([r[k] for r in rows[m]])) for k in ('iter_ms', 'pass_ms', 'pass_TBs', 'pass_bytes')}
           for m in modes}
    # where an iteration's time goes: passes (class 0) and reductions over T (class 2), every launch timed
    for m in modes:
        e = eng[m]
        e.kernel_stats(2, reset=True)                     # switches the reductions' events on
        e.kernel_stats(0, reset=True)
        e.synchronize()
        t0 = time.perf_counter()
        pkg.run_solver(e, opts(args.steps), 3)
        e.synchronize()
        dt = time.perf_counter() - t0
        p_ms, p_n = e.kernel_stats(0)[:2]
        r_ms, r_n = e.kernel_stats(2)[:2]
        emit(kind='kernel_stats', mode=m, steps=args.steps, iter_ms=dt / args.steps * 1e3, pass_ms_per_iter=p_ms / args.steps,
             passes=p_n, reduction_ms_per_iter=r_ms / args.steps, reductions=r_n)
    emit(kind='summary', size=N, rank=R, as_rank=args.as_rank, of=args.of, median=med,
         pass_ratio_f16_over_f32=med['f16']['pass_ms'] / med['f32']['pass_ms'],
         iter_ratio_f16_over_f32=med['f16']['iter_ms'] / med['f32']['iter_ms'])
    for m in modes:
        eng[m].close()


if __name__ == '__main__':
    main()
