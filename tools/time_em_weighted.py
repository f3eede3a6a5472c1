#!/usr/bin/env python3
"""Development timing of per-entry weights on a dense block at 1000^3, R = 20, fp32 tensor, in one process: the outer
iteration with W uniform in (0, 1), with Z.miss at 20 % missing and without a mask, and the weighted pass alone against
the unfused masked pass (`aoadmm_resident_em_pass`, statistics only read back): by the HIP events the call records
around the pass (`kernel_stats(4)`), and by a host clock around the call, which ends in a stream synchronise.  Medians of 7
with min-max; raw lines go to profiles/em_weighted_time.jsonl.
usage: time_em_weighted.py [n, default 1000]"""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('matlab-code_amd')
capi = importlib.import_module('matlab-code_amd._capi')
import bench  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
R, frac, REPS = 20, 0.2, 7
OPTS = dict(MaxInnerIters=5, AbsFuncTol=0.0, OuterRelTol=0.0, innerRelPrTol_coupl=0.0, innerRelPrTol_constr=0.0,
            innerRelDualTol_coupl=0.0, innerRelDualTol_constr=0.0, bsum=0)
out_path = os.path.join(ROOT, 'profiles', 'em_weighted_time.jsonl')
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []


def note(**kw):
    kw.update(n=n, R=R, precision='f32')
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


eng = pkg.Engine(0)
rng = np.random.default_rng(1)
for kind in ('plain', 'masked', 'weighted'):
    Z = bench.build_Z(n, n, n, R, seed=0, noise=0.05)
    Z['_ranks'] = [R] * 3
    io = dict(lambdas_init=[[1] * R], nvecs=0, distr=[lambda a, b: rng.random((a, b))] * 3, normalize=1)
    pkg.build_model(eng, Z, 'f32')
    if kind == 'masked':
        mk = (np.random.default_rng(2).random(n * n * n, dtype=np.float32) > frac).astype(np.uint8)
        capi.check(eng.lib.aoadmm_tensor_mask_upload(eng.h, 0, mk.ctypes.data_as(C.POINTER(C.c_uint8))))
        del mk
    elif kind == 'weighted':
        W = np.random.default_rng(2).random(n * n * n, dtype=np.float32).astype(np.float64)
        capi.check(eng.lib.aoadmm_tensor_weights_upload(eng.h, 0, capi.dptr(W)))
        del W
    G = pkg.init_coupled_AOADMM_CMTF(Z, io, rng=rng, engine=eng)
    per_iter = []
    for rep in range(REPS + 1):                        # the first repetition warms up
        t = {}
        for k in (3, 23):
            pkg.upload_state(eng, Z, G)
            eng.synchronize()
            t0 = time.perf_counter()
            pkg.run_solver(eng, dict(OPTS, MaxOuterIters=k), 3, has_missing=kind != 'plain')
            t[k] = time.perf_counter() - t0
        if rep:
            per_iter.append((t[23] - t[3]) / 20 * 1e3)
    note(what='outer_iteration_ms', block=kind, **spread(per_iter))
    if kind != 'plain':
        pkg.upload_state(eng, Z, G)
        ms, ev = [], []
        for rep in range(REPS + 2):
            eng.synchronize()
            eng.kernel_stats(4, reset=True)
            t0 = time.perf_counter()
            eng.resident_em_pass(0, (n, n, n), R, update=1, fuse=0, with_data=False)
            wall = (time.perf_counter() - t0) * 1e3
            ev_ms, launches = eng.kernel_stats(4)[:2]
            assert launches == 1, launches
            if rep >= 2:
                ms.append(wall)
                ev.append(ev_ms)
        note(what='unfused_update_pass_event_ms', block=kind, **spread(ev))
        note(what='unfused_update_pass_wall_ms', block=kind, **spread(ms))
eng.close()
with open(out_path, 'a') as f:
    for ln in lines:
        f.write(json.dumps(ln) + '\n')
