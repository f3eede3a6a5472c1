#!/usr/bin/env python3
"""Development timing of the EM (Z.miss) path at 1000^3, R = 20, fp32 tensor.

usage: time_em.py [missing fraction, default 0.2]
           outer iteration with and without a mask
       time_em.py --missing-list [--unmarked-only] [--out FILE]
           the block marked with Engine.set_missing_list beside the unmarked one at missing
           shares 20 %, 5 %, 1 % and 0.1 %, one process: the outer iteration, the list pass by its HIP events (class 16)
           and the dense update pass (class 4), medians of 7 with min and max; one JSON line per measurement to stdout
           and to FILE.  --unmarked-only measures the unmarked block alone (what a build without the feature can run)."""
import argparse, importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('matlab-code_amd')
capi = importlib.import_module('matlab-code_amd._capi')
import ctypes as C
import bench
n, R = 1000, 20
REPS = 7


def solver_options(k, hip=None):
    o = dict(MaxOuterIters=k, MaxInnerIters=5, AbsFuncTol=0.0, OuterRelTol=0.0, innerRelPrTol_coupl=0.0, innerRelPrTol_constr=0.0,
             innerRelDualTol_coupl=0.0, innerRelDualTol_constr=0.0, bsum=0)
    if hip:
        o['hip'] = hip
    return o


def model(eng, rng, mask=None):
    Z = bench.build_Z(n, n, n, R, seed=0, noise=0.05); Z['_ranks'] = [R] * 3
    io = dict(lambdas_init=[[1] * R], nvecs=0, distr=[lambda a, b: rng.random((a, b))] * 3, normalize=1)
    pkg.build_model(eng, Z, 'f32')
    if mask is not None:
        capi.check(eng.lib.aoadmm_tensor_mask_upload(eng.h, 0, mask.ctypes.data_as(C.POINTER(C.c_uint8))))
    return Z, io


def iteration_ms(eng, Z, G, masked, hip=None):
    """(t[23 iterations] - t[3 iterations]) / 20 from the same state"""
    t = {}
    for k in (3, 23):
        pkg.upload_state(eng, Z, G)
        eng.synchronize()
        t0 = time.perf_counter()
        pkg.run_solver(eng, solver_options(k, hip), 3, has_missing=masked)
        t[k] = time.perf_counter() - t0
    return (t[23] - t[3]) / 20 * 1e3


def one_fraction(frac):
    eng = pkg.Engine(0)
    rng = np.random.default_rng(1)
    for masked in (False, True):
        mk = (np.random.default_rng(2).random(n * n * n, dtype=np.float32) > frac).astype(np.uint8) if masked else None
        Z, io = model(eng, rng, mk)
        G = pkg.init_coupled_AOADMM_CMTF(Z, io, rng=rng, engine=eng)
        iteration_ms(eng, Z, G, masked)
        print('1000^3 R=20 fp32, mask=%s (%.1f %% missing): %.3f ms per outer iteration'
              % (masked, 100 * frac if masked else 0.0, iteration_ms(eng, Z, G, masked)), flush=True)
    eng.close()


def spread(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def missing_list(unmarked_only, out_path):
    eng = pkg.Engine(0)
    rng = np.random.default_rng(1)
    out = open(out_path, 'a') if out_path else None

    def emit(**rec):
        line = json.dumps(dict(shape=[n, n, n], R=R, precision='f32', reps=REPS, **rec))
        print(line, flush=True)
        if out:
            out.write(line + '\n'); out.flush()

    def event_ms(which, call):
        v = []
        for _ in range(REPS):
            eng.kernel_stats(which, reset=True)
            call()
            v.append(eng.kernel_stats(which)[0])
        return spread(v)

    Z, io = model(eng, rng)
    G = pkg.init_coupled_AOADMM_CMTF(Z, io, rng=rng, engine=eng)
    iteration_ms(eng, Z, G, False)
    emit(what='outer_iteration_ms', missing=0.0, marked=False, **spread([iteration_ms(eng, Z, G, False) for _ in range(REPS)]))
    emit(what='outer_iteration_ms', missing=0.0, marked=False, no_permuted_copy=1,
         **spread([iteration_ms(eng, Z, G, False, dict(no_permuted_copy=1)) for _ in range(REPS)]))
    for frac in (0.2, 0.05, 0.01, 0.001):
        mk = (np.random.default_rng(2).random(n * n * n, dtype=np.float32) > frac).astype(np.uint8)
        for marked in ((False,) if unmarked_only else (False, True)):
            Z, io = model(eng, rng, mk)
            if marked:
                eng.synchronize()
                t0 = time.perf_counter()
                eng.set_missing_list(0)
                emit(what='list_build_ms', missing=frac, marked=True, entries=eng.missing_list(0), ms=(time.perf_counter() - t0) * 1e3,
                     resident_bytes=eng.tensor_storage_info(0)[2])
            iteration_ms(eng, Z, G, True)
            emit(what='outer_iteration_ms', missing=frac, marked=marked, **spread([iteration_ms(eng, Z, G, True) for _ in range(REPS)]))
            if marked:
                emit(what='list_pass_ms', missing=frac, marked=True,
                     **event_ms(16, lambda: eng.resident_em_list_pass(0, (n, n, n), update=1, with_data=False)))
            else:
                for fuse in (0, 1):
                    emit(what='dense_update_pass_ms', missing=frac, marked=False, fuse=fuse,
                         **event_ms(4, lambda: eng.resident_em_pass(0, (n, n, n), R, update=1, fuse=fuse, with_data=False)))
        del mk
    eng.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('fraction', nargs='?', type=float, default=0.2)
    ap.add_argument('--missing-list', action='store_true')
    ap.add_argument('--unmarked-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.missing_list:
        missing_list(a.unmarked_only, a.out)
    else:
        one_fraction(a.fraction)
