"""Time of a PARAFAC2 block with sparse slabs (csrc/par2_sparse.hip) on one GPU: the three right-hand sides and one
outer iteration, optionally next to the dense path on the densified slabs.

    python3 tools/time_sparse_par2.py [--I 2000] [--K 2000] [--J 50] [--density 0.01 | --nnz 1e8] [--R 5] [--skew]
                                      [--reps 5] [--iters 6] [--dense] [--label TEXT] [--out profiles/sparse_par2_time_x.jsonl]

Slabs are ragged: J_k uniform in [max(R, 0.4 J), 1.6 J].  Prints (and appends to --out) one JSON line per measurement.
'rhs' lines: HIP events on the library's stream around the whole right-hand side (`ms_events_*`, from
aoadmm_resident_par2_rhs) and around the pass over the nonzeros alone (`pass_ms`, aoadmm_kernel_stats(3)), with the
pass's algorithmic bytes (nonzeros streamed + factor rows gathered + output written) as TB/s.  Layout 'colmajor' is
the state before any solve (Y = X'A gathers the column-major A), 'rowmajor' after one outer iteration.  'outer' lines:
host clock between the objective read-backs of consecutive outer iterations (every iteration ends with the host
waiting for that read-back), first iteration dropped.  --dense runs the same model with the slabs densified through
aoadmm_par2_slab_upload instead.  To time the dense path of another commit, copy this file into a checkout of that
commit (built there) and run it with --dense: that half uses only entries every build has.  --label goes into the
'setup' line to say which build a file of results belongs to.
--skew draws rows and global columns as floor(size * u^4): the first slab and the first row then own a large share.
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
pkg = importlib.import_module('matlab-code_amd')
capi = importlib.import_module('matlab-code_amd._capi')


def emit(a, row):
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--I', type=float, default=2000)
    ap.add_argument('--K', type=float, default=2000)
    ap.add_argument('--J', type=int, default=50)
    ap.add_argument('--density', type=float, default=0.01)
    ap.add_argument('--nnz', type=float, default=0)
    ap.add_argument('--R', type=int, default=5)
    ap.add_argument('--skew', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=6)
    ap.add_argument('--dense', action='store_true')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--label', default='this build')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    I, K, R = int(a.I), int(a.K), a.R
    rng = np.random.default_rng(a.seed)
    Jk = rng.integers(max(R, int(0.4 * a.J)), int(1.6 * a.J) + 1, K)
    off = np.concatenate([[0], np.cumsum(Jk)]).astype(np.int64)
    Jtot = int(off[-1])
    nnz = int(a.nnz) if a.nnz else int(a.density * I * Jtot)
    t0 = time.time()
    if a.skew:
        i = np.minimum((I * rng.random(nnz) ** 4).astype(np.int64), I - 1)
        g = np.minimum((Jtot * rng.random(nnz) ** 4).astype(np.int64), Jtot - 1)
    else:
        i = rng.integers(0, I, nnz)
        g = rng.integers(0, Jtot, nnz)
    k = np.searchsorted(off, g, side='right') - 1
    subs = np.empty((nnz, 3), dtype=np.int64, order='F')
    subs[:, 0], subs[:, 1], subs[:, 2] = i, g - off[k], k
    vals = rng.random(nnz)
    share_row = float(np.bincount(i, minlength=1).max()) / nnz
    share_slab = float(np.bincount(k, minlength=1).max()) / nnz
    del i, g, k
    t_gen = time.time() - t0
    eng = pkg.Engine(0)
    try:
        run(a, eng, I, K, R, Jk, off, Jtot, subs, vals, t_gen, share_row, share_slab)
    finally:
        eng.close()


def run(a, eng, I, K, R, Jk, off, Jtot, subs, vals, t_gen, share_row, share_slab):
    rng = np.random.default_rng(a.seed + 1)
    lib, h = eng.lib, eng.h
    capi.check(lib.aoadmm_model_begin(h, 3, 1, 0))
    capi.check(lib.aoadmm_model_set_mode(h, 0, I, R))
    rows = (C.c_int64 * K)(*[int(v) for v in Jk])
    capi.check(lib.aoadmm_model_set_mode_slabs(h, 1, K, rows, R))
    capi.check(lib.aoadmm_model_set_mode(h, 2, K, R))
    capi.check(lib.aoadmm_model_add_par2(h, 0, (C.c_int * 3)(0, 1, 2), 1.0))
    for m in range(3):
        capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
    capi.check(lib.aoadmm_model_end(h))
    t0 = time.time()
    if a.dense:
        X = np.zeros(I * Jtot)                         # slabs back to back, each I x J_k column-major
        np.add.at(X, subs[:, 0] + I * (off[subs[:, 2]] + subs[:, 1]), vals)
        capi.check(lib.aoadmm_par2_slab_upload(h, 0, capi.ALL_SLABS, capi.dptr(X)))
        del X
    else:
        eng.upload_par2_coo(0, subs, vals)
    eng.synchronize()
    t_up = time.time() - t0
    normsq = C.c_double(0)
    capi.check(lib.aoadmm_tensor_normsq(h, 0, C.byref(normsq)))

    def put(field, index, slab, M):
        M = np.asfortranarray(M)
        capi.check(lib.aoadmm_state_set(h, field, index, slab, capi.dptr(M), M.shape[0], M.shape[1]))

    def put_cells(field, index, cells):
        packed = np.concatenate([c.ravel(order='F') for c in cells])
        capi.check(lib.aoadmm_state_set(h, field, index, capi.ALL_SLABS, capi.dptr(packed), Jtot, R))

    def set_state():
        r2 = np.random.default_rng(a.seed + 2)
        put(capi.F_FAC, 0, 0, r2.standard_normal((I, R)) / np.sqrt(I))
        put_cells(capi.F_FAC, 1, [r2.standard_normal((int(j), R)) / np.sqrt(j) for j in Jk])
        put(capi.F_FAC, 2, 0, r2.random((K, R)) + 0.1)
        put(capi.F_DELTAB, 0, 0, r2.random((R, R)))
        put_cells(capi.F_P, 0, [np.eye(int(j), R) for j in Jk])
        put_cells(capi.F_MU_DELTAB, 0, [r2.random((int(j), R)) for j in Jk])

    set_state()
    emit(a, {'what': 'setup', 'path': 'dense' if a.dense else 'sparse', 'I': I, 'K': K, 'Jtot': Jtot, 'R': R,
             'nnz_given': int(vals.shape[0]), 'density_given': vals.shape[0] / (I * Jtot), 'skew': a.skew,
             'largest_row_share': round(share_row, 4), 'largest_slab_share': round(share_slab, 4),
             'gen_s': round(t_gen, 2), 'upload_s': round(t_up, 2), 'normsq': normsq.value,
             'build': a.label})

    def time_rhs(layout):
        for mode in range(3):
            ms = C.c_float(0)
            capi.check(lib.aoadmm_resident_par2_rhs(h, 0, mode, None, C.byref(ms)))      # warm-up
            eng.kernel_stats(3, reset=True)
            ev = []
            for _ in range(a.reps):
                capi.check(lib.aoadmm_resident_par2_rhs(h, 0, mode, None, C.byref(ms)))
                ev.append(ms.value)
            kms, launches, by, fl = eng.kernel_stats(3, reset=True)
            per, bpl = kms / launches, by / launches
            emit(a, {'what': 'rhs', 'layout': layout, 'mode': mode, 'ms_events_min': round(min(ev), 4),
                     'ms_events_median': round(float(np.median(ev)), 4), 'pass_ms': round(per, 4),
                     'pass_GB': round(bpl / 1e9, 3), 'pass_TBps': round(bpl / per / 1e9, 3),
                     'nnz_coalesced': int(round(fl / launches / (2 * R)))})

    if not a.dense:
        time_rhs('colmajor')
    o = capi.Options()
    o.MaxOuterIters, o.MaxInnerIters, o.use_dimtree = a.iters, 5, 1
    tt = np.zeros(a.iters + 1)
    fv = np.zeros(a.iters + 1)
    res = capi.Result()
    res.time_at_it = capi.dptr(tt)
    res.func_val_conv = capi.dptr(fv)
    eng.kernel_stats(3, reset=True)
    capi.check(lib.aoadmm_solve(h, C.byref(o), C.byref(res)))
    kms, launches, by, fl = eng.kernel_stats(3, reset=True)
    per_it = np.diff(tt)[1:] * 1e3
    emit(a, {'what': 'outer', 'path': 'dense' if a.dense else 'sparse', 'iters': int(res.OuterIterations),
             'ms_per_outer_median': round(float(np.median(per_it)), 4), 'ms_per_outer_min': round(float(per_it.min()), 4),
             'ms_per_outer_all': [round(float(v), 3) for v in np.diff(tt) * 1e3], 'passes': int(launches),
             'pass_ms_sum': round(kms, 4), 'f_first': fv[0], 'f_last': fv[int(res.OuterIterations)]})
    if not a.dense:
        time_rhs('rowmajor')


if __name__ == '__main__':
    main()
