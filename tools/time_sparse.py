"""Per-mode time of the sparse (COO) MTTKRP (csrc/sparse.hip) on one GPU, next to a torch index_add_ MTTKRP of the same
data on the same GPU.

    python3 tools/time_sparse.py [--dims 1000000,100000,10000] [--nnz 100000000] [--R 20] [--skew] [--reps 5]
    python3 tools/time_sparse.py --nvecs [--nvecs-iters 20] [--host-gram] ...
    python3 tools/time_sparse.py --as-rank 0 --of 8 [--skew] ...
    python3 tools/time_sparse.py --observed-only [--out profiles/sparse_observed_time.jsonl] ...
    python3 tools/time_sparse.py --observed-only --weights [ALPHA] [--reps 7] [--out profiles/sparse_weighted_time.jsonl] ...
    python3 tools/time_sparse.py --heldout [FRAC] [--skew] [--reps 7] [--out profiles/sparse_heldout_time.jsonl] ...
    python3 tools/time_sparse.py --heldout [FRAC] --keep-best [--out profiles/heldout_keep_best_time.jsonl] ...
    python3 tools/time_sparse.py --ranklist NQ [--rank-every M] [--reps 7] [--out profiles/rank_track_time.jsonl] ...

Prints one JSON line per (layout, mode) and a summary line.  Layouts: 'colmajor' gathers from the column-major factors
(what aoadmm_resident_mttkrp sees before any solve), 'rowmajor' after one outer iteration, when the Gram kernel has left
the row-major copies the solver's own MTTKRPs gather from.  Bytes are algorithmic (nonzeros streamed + factor rows
gathered + output written, aoadmm_kernel_stats(3)); the HBM peak taken for the share is 8 TB/s.
--skew draws every subscript as floor(size * u^4), u uniform: a power law, row 0 of the first mode then owns ~3 %
of all nonzeros.  Subscripts go up unsorted and uncoalesced: the device sorts and sums duplicates.
--nvecs times the nvecs start of every mode instead (aoadmm_resident_nvecs, r = R, block b = R + 8): the model takes
rank b, so that the block's own MTTKRP of the mode at rank b stands next to it.  Per mode: F, the mean time of one
pass over the nonzeros (HIP events, aoadmm_kernel_stats(3); an iteration runs two), the wall time of an iteration with
its dense part (difference of a run of --nvecs-iters iterations and a run of one) and of the list build (what is left
of the one-iteration run), the iterations run and whether the tolerance was reached within --nvecs-iters.
--host-gram adds the wall time of the host path (sptensor.unfold_gram + eigh) for modes of at most 16384 rows.
--as-rank R --of N times one rank's share of a block sharded over N ranks (aoadmm_tensor_upload_coo_sharded) next to the
replicated block, in one process: the replicated upload and its per-mode MTTKRP first (row-major gathers, after one outer
iteration) on one engine, and on a second engine aoadmm_comm_init_rank_share(R, N), the sharded upload of the same list and
the same factors; the MTTKRPs of the two engines alternate.  Per mode: the median (and min, max) over --reps of both kernel
times (HIP events around the MTTKRP kernels, aoadmm_kernel_stats(3)), the ratio of the medians next to 1/N, the share's
nonzeros and row span.  --of takes a list (2,4,8); R is taken modulo each N, so --as-rank -1 is the last rank.  The
communicator has ONE rank: `allreduce_1rank_ms` is what is left of aoadmm_resident_mttkrp's own events after the
kernels, i.e. a one-rank ncclAllReduce of I_n x R doubles on one GPU.  It says nothing about the all-reduce between
GPUs, which this tool cannot time.
--observed-only times the block marked observed-only (aoadmm_tensor_set_observed_only, csrc/sparse_em.hip) next to the
plain block of the same data in the same process, one engine each, after one outer iteration of both (row-major gathers,
and the observed block holds a snapshot).  Per mode: the median (min, max) over --reps of the plain MTTKRP, of the
imputed MTTKRP (residual values + dense correction) and of the EM step's pass over that mode's copy (HIP events,
aoadmm_kernel_stats(3) and (4 + n); the pass over the first copy carries the statistics with the snapshot's gathers),
and their ratio next to N / (N - 1).  Then the statistics-only pass (first step after a new mark: no snapshot, residuals
written), the whole EM step, and the wall time of one outer iteration of both engines (difference of solves of 3 and of
1 iterations, unconstrained modes).  Every line also goes to --out.
--observed-only --weights ALPHA (default 0.1) times the passes of a weighted block (aoadmm_tensor_set_entry_weights:
uniform weights on the coalesced entries, ALPHA on the unstored ones) against those of the observed-only block of the
same data in the same process, one engine each, after one outer iteration of both; the EM steps of the two engines
alternate.  Per mode: the median (min, max) over --reps (at least 7) of both passes (HIP events, aoadmm_kernel_stats
(4 + n); the pass over the first copy is the statistics pass with the snapshot's gathers), the ratio of the medians and
the ratio of the algorithmic bytes, which is what 8 more streamed bytes per entry predict.  Then the statistics pass of
a first step (no snapshot) of both.  The duplicates of the drawn list are dropped on the host first: the weight list
must name the stored entries once each.
--heldout FRAC (default 0.1) holds FRAC of the drawn list out (its first rows: the draw is i.i.d.) and times the
held-out pass (csrc/heldout.hip, aoadmm_resident_heldout_stats, HIP events of aoadmm_kernel_stats(12)) in one process
with the residual passes of an observed-only block of the training entries (classes 4 + n) and with one outer iteration
(wall, solves of 3 and of 1 iterations) of the plain and of the observed-only block, each with the list attached and
without it, alternating.  Medians of --reps (at least 7).  `per_entry_ratio` is the pass's time per held-out entry over
the time per nonzero of a residual pass over modes 2 and 3 (both do N gathers per entry; the held-out pass writes
nothing).  The list is scored in the caller's order and again sorted by its first subscript on the host, which is what
a sort at attach time would give the pass.
--ranklist NQ times a ranking list of NQ queries along the first mode tracked inside a solve,
without exclusions and with 100 excluded rows per query: the wall time of an outer iteration with the list attached and
removed, alternating in one process (every --rank-every-th iteration is evaluated; the added time is per evaluated
iteration), the HIP-event time of the evaluation's launches inside the solve (aoadmm_kernel_stats(13): the rank pass and
the two launches of the metric reduction), and next to it the launches of a stand-alone `Engine.rank_of` of the same
list.  `rank_metrics` lines time `Engine.op_rank_metrics` (wall, uploads included) at 16 384 and 10^7 queries.

--heldout FRAC --keep-best times solves of 4 iterations (wall) of the plain block with the list attached and
aoadmm_heldout_keep_best on and off, alternating, and one aoadmm_heldout_restore_best.  The held-out values are the
model's own after those 4 iterations (the solve is bit-reproducible), so that the held-out sum falls from iteration to
iteration: `snapshots_per_solve` is what aoadmm_heldout_best_info counted, 5 = the starting point and every iteration, the
worst case.  `added_ms_per_snapshot` is the difference of the medians over that count.
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

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', default='1000000,100000,10000')
    ap.add_argument('--nnz', type=float, default=1e8)
    ap.add_argument('--R', type=int, default=20)
    ap.add_argument('--skew', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--nvecs', action='store_true')
    ap.add_argument('--nvecs-iters', type=int, default=20)
    ap.add_argument('--host-gram', action='store_true')
    ap.add_argument('--as-rank', type=int, default=None)
    ap.add_argument('--of', default=None)
    ap.add_argument('--observed-only', action='store_true')
    ap.add_argument('--weights', type=float, nargs='?', const=0.1, default=None, metavar='ALPHA')
    ap.add_argument('--heldout', type=float, nargs='?', const=0.1, default=None, metavar='FRAC')
    ap.add_argument('--keep-best', action='store_true')
    ap.add_argument('--ranklist', type=int, default=None, metavar='NQ')
    ap.add_argument('--rank-every', type=int, default=1, metavar='M')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.keep_best and a.heldout is None:
        ap.error('--keep-best goes with --heldout')
    if a.weights is not None:
        if not a.observed_only:
            ap.error('--weights goes with --observed-only')
        if not 0.0 <= a.weights <= 1.0:
            ap.error('--weights ALPHA must lie inside [0, 1]')
        a.reps = max(a.reps, 7)
    if a.ranklist is not None:
        if a.ranklist < 1 or a.rank_every < 1:
            ap.error('--ranklist NQ and --rank-every M must be positive')
        a.reps = max(a.reps, 7)
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'rank_track_time.jsonl' if a.ranklist is not None else
                             'sparse_weighted_time.jsonl' if a.weights is not None else
                             'heldout_keep_best_time.jsonl' if a.keep_best else
                             'sparse_heldout_time.jsonl' if a.heldout is not None else 'sparse_observed_time.jsonl')
    if a.heldout is not None:
        if not 0.0 < a.heldout < 1.0:
            ap.error('--heldout FRAC must lie inside (0, 1)')
        a.reps = max(a.reps, 7)
    if not a.no_torch:
        # torch (and the HIP runtime it ships) first, as bench.py does: loaded after the library, the process aborted in
        # its exit-time destructors
        import torch
        torch.cuda.init()
    dims = [int(float(v)) for v in a.dims.split(',')]
    N, R, nnz = len(dims), a.R, int(a.nnz)
    if (a.as_rank is None) != (a.of is None):
        ap.error('--as-rank and --of go together')
    if a.nvecs or a.of is not None or a.observed_only or a.heldout is not None or a.ranklist is not None:
        a.no_torch = True
    rng = np.random.default_rng(a.seed)
    t0 = time.time()
    subs = np.empty((nnz, N), dtype=np.int64, order='F')
    for m, s in enumerate(dims):
        if a.skew:
            subs[:, m] = np.minimum((s * rng.random(nnz) ** 4).astype(np.int64), s - 1)
        else:
            subs[:, m] = rng.integers(0, s, nnz)
    vals = rng.random(nnz)
    t_gen = time.time() - t0
    eng = pkg.Engine(0)
    try:
        (run_ranklist if a.ranklist is not None else run_nvecs if a.nvecs else run_share if a.of is not None else run_weighted if a.weights is not None else
         run_observed if a.observed_only else
         run_heldout if a.heldout is not None else run)(a, eng, dims, N, R, nnz, subs, vals, t_gen)
    finally:
        eng.close()


def run_nvecs(a, eng, dims, N, R, nnz, subs, vals, t_gen):
    rng = np.random.default_rng(a.seed + 1)
    lib, h = eng.lib, eng.h
    b = min(64, R + 8)
    capi.check(lib.aoadmm_model_begin(h, N, 1, 0))
    for m, s in enumerate(dims):
        capi.check(lib.aoadmm_model_set_mode(h, m, s, b))
    capi.check(lib.aoadmm_model_add_cp(h, 0, N, (C.c_int * N)(*range(N)), 1.0))
    for m in range(N):
        capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
    capi.check(lib.aoadmm_model_end(h))
    t0 = time.time()
    eng.upload_coo(0, subs, vals)
    eng.synchronize()
    print(json.dumps({'what': 'setup', 'dims': dims, 'nnz_given': nnz, 'r': R, 'b': b, 'skew': a.skew,
                      'gen_s': round(t_gen, 2), 'upload_s': round(time.time() - t0, 2)}), flush=True)
    for m in range(N):
        Um = np.asfortranarray(rng.random((dims[m], b)))
        capi.check(lib.aoadmm_state_set(h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], b))
    for n in range(N):
        rmax = min(R, dims[n])
        ms = C.c_float(0)
        capi.check(lib.aoadmm_resident_mttkrp(h, 0, n, None, C.byref(ms)))              # warm-up
        ev = []
        for _ in range(a.reps):
            capi.check(lib.aoadmm_resident_mttkrp(h, 0, n, None, C.byref(ms)))
            ev.append(ms.value)
        eng.resident_nvecs(0, n, dims[n], rmax, max_iters=1)                             # warm-up
        t0 = time.time()
        _, _, i1 = eng.resident_nvecs(0, n, dims[n], rmax, max_iters=1)
        w1 = (time.time() - t0) * 1e3
        eng.kernel_stats(3, reset=True)
        t0 = time.time()
        _, _, ik = eng.resident_nvecs(0, n, dims[n], rmax, max_iters=a.nvecs_iters)
        wk = (time.time() - t0) * 1e3
        kms, launches, by, _ = eng.kernel_stats(3, reset=True)
        it_ms = (wk - w1) / (ik['iterations'] - 1) if ik['iterations'] > 1 else float('nan')
        r = {'what': 'nvecs', 'mode': n + 1, 'rows': dims[n], 'r': rmax, 'b': ik['block'], 'F': ik['fibers'],
             'pass_ms': round(kms / launches, 4), 'pass_TBps': round(by / launches / (kms / launches) / 1e9, 3),
             'iter_ms_wall': round(it_ms, 3), 'build_ms_wall': round(w1 - it_ms, 3) if it_ms == it_ms else None,
             'iterations': ik['iterations'], 'converged': ik['converged'], 'residual': ik['residual'],
             'mttkrp_rank_b_ms': round(float(np.median(ev)), 4),
             'passes_over_two_mttkrps': round(2 * kms / launches / (2 * float(np.median(ev))), 3)}
        if a.host_gram and dims[n] <= 16384:
            sp = importlib.import_module('matlab-code_amd.sptensor')
            t0 = time.time()
            w, V = np.linalg.eigh(sp.unfold_gram(subs, vals, dims, n))
            r['host_gram_ms'] = round((time.time() - t0) * 1e3, 1)
        print(json.dumps(r), flush=True)


def run_share(a, eng, dims, N, R, nnz, subs, vals, t_gen):
    lib = eng.lib
    worlds = [int(v) for v in a.of.split(',')]
    o = capi.Options()
    o.MaxOuterIters, o.MaxInnerIters, o.use_dimtree = 1, 1, 1

    def prepare(e):
        """The replicated block, the same factors on every engine, and one outer iteration (unconstrained, no
        couplings; deterministic) so that the Gram kernels leave the row-major factor copies behind."""
        rng = np.random.default_rng(a.seed + 1)
        h = e.h
        capi.check(lib.aoadmm_model_begin(h, N, 1, 0))
        for m, s in enumerate(dims):
            capi.check(lib.aoadmm_model_set_mode(h, m, s, R))
        capi.check(lib.aoadmm_model_add_cp(h, 0, N, (C.c_int * N)(*range(N)), 1.0))
        for m in range(N):
            capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
        capi.check(lib.aoadmm_model_end(h))
        t0 = time.time()
        e.upload_coo(0, subs, vals)
        e.synchronize()
        t_up = time.time() - t0
        for m in range(N):
            Um = np.asfortranarray(rng.random((dims[m], R)))
            capi.check(lib.aoadmm_state_set(h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], R))
        res = capi.Result()
        capi.check(lib.aoadmm_solve(h, C.byref(o), C.byref(res)))
        return t_up

    def once(e, n):
        """(kernel ms, ms of aoadmm_resident_mttkrp's own events, algorithmic bytes) of one MTTKRP of mode n"""
        ms = C.c_float(0)
        e.kernel_stats(3, reset=True)
        capi.check(lib.aoadmm_resident_mttkrp(e.h, 0, n, None, C.byref(ms)))
        kms, launches, by, _ = e.kernel_stats(3, reset=True)
        assert launches == 1
        return kms, ms.value, by

    share_eng = pkg.Engine(0)                 # the replicated block stays on `eng`, the share goes here: same process
    try:
        t_up = prepare(eng)
        prepare(share_eng)
        full_bytes = eng.tensor_storage_info(0)[2]
        nnz_c = full_bytes // (N * (4 * N + 8))
        print(json.dumps({'what': 'setup', 'dims': dims, 'nnz_given': nnz, 'nnz_coalesced': int(nnz_c), 'R': R,
                          'skew': a.skew, 'reps': a.reps, 'gen_s': round(t_gen, 2), 'upload_s': round(t_up, 2),
                          'resident_bytes': int(full_bytes)}), flush=True)
        for world in worlds:
            rank = a.as_rank % world
            capi.check(lib.aoadmm_comm_init_rank_share(share_eng.h, share_eng.comm_unique_id(), rank, world))
            t0 = time.time()
            share_eng.upload_coo(0, subs, vals, sharded=True)
            share_eng.synchronize()
            t_cut = time.time() - t0
            share_bytes = share_eng.tensor_storage_info(0)[2]
            lo, hi = capi.coo_share(nnz_c, rank, world)
            assert share_bytes == N * (4 * N + 8) * (hi - lo), (share_bytes, lo, hi)
            for n in range(N):
                once(eng, n), once(share_eng, n)                             # warm-up
                rep, sh = [], []
                for _ in range(a.reps):                                      # alternating, same process, same factors
                    rep.append(once(eng, n))
                    sh.append(once(share_eng, n))
                rk, sk = [v[0] for v in rep], [v[0] for v in sh]
                # output rows of the span: what is left of the algorithmic bytes after the nonzeros and the gathers
                span_rows = (sh[0][2] - (hi - lo) * (4 * N + 8 + (N - 1) * R * 8)) / (R * 8)
                print(json.dumps({
                    'what': 'share', 'as_rank': rank, 'of': world, 'skew': a.skew, 'mode': n + 1, 'reps': a.reps,
                    'share_nnz': int(hi - lo), 'span_rows': int(round(span_rows)), 'rows': dims[n],
                    'share_ms': round(float(np.median(sk)), 4), 'share_ms_min_max': [round(min(sk), 4), round(max(sk), 4)],
                    'replicated_ms': round(float(np.median(rk)), 4),
                    'replicated_ms_min_max': [round(min(rk), 4), round(max(rk), 4)],
                    'ratio': round(float(np.median(sk)) / float(np.median(rk)), 4), 'one_over_N': round(1.0 / world, 4),
                    'allreduce_1rank_ms': round(float(np.median([v[1] - v[0] for v in sh])), 4),
                    'allreduce_MB': round(dims[n] * R * 8 / 1e6, 2), 'upload_s': round(t_cut, 2),
                    'resident_bytes': int(share_bytes)}), flush=True)
    finally:
        share_eng.close()


def run_observed(a, eng, dims, N, R, nnz, subs, vals, t_gen):
    lib = eng.lib
    out = open(a.out, 'a')

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def solve(e, iters):
        o = capi.Options()
        o.MaxOuterIters, o.MaxInnerIters, o.use_dimtree = iters, 1, 1
        res = capi.Result()
        e.synchronize()
        t0 = time.time()
        capi.check(lib.aoadmm_solve(e.h, C.byref(o), C.byref(res)))
        e.synchronize()
        return (time.time() - t0) * 1e3

    def set_factors(e):
        rng = np.random.default_rng(a.seed + 1)
        for m in range(N):
            Um = np.asfortranarray(rng.random((dims[m], R)))
            capi.check(lib.aoadmm_state_set(e.h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], R))

    def prepare(e, observed):
        h = e.h
        capi.check(lib.aoadmm_model_begin(h, N, 1, 0))
        for m, s in enumerate(dims):
            capi.check(lib.aoadmm_model_set_mode(h, m, s, R))
        capi.check(lib.aoadmm_model_add_cp(h, 0, N, (C.c_int * N)(*range(N)), 1.0))
        for m in range(N):
            capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
        capi.check(lib.aoadmm_model_end(h))
        t0 = time.time()
        e.upload_coo(0, subs, vals)
        if observed:
            e.set_observed_only(0)
        e.synchronize()
        t_up = time.time() - t0
        set_factors(e)
        solve(e, 1)                                   # row-major factor copies; the observed block takes its snapshot
        return t_up

    def mttkrp_once(e, n):
        ms = C.c_float(0)
        e.kernel_stats(3, reset=True)
        capi.check(lib.aoadmm_resident_mttkrp(e.h, 0, n, None, C.byref(ms)))
        kms, launches, by, _ = e.kernel_stats(3, reset=True)
        assert launches == 1
        return kms, by

    def step_once(e):
        """(ms of the whole EM step, [ms of the pass over every copy], [their algorithmic bytes])"""
        for c in [3] + [4 + n for n in range(N)]:
            e.kernel_stats(c, reset=True)
        e.em_step(0)
        whole = e.kernel_stats(3, reset=True)[0]
        per = [e.kernel_stats(4 + n, reset=True) for n in range(N)]
        return whole, [p[0] for p in per], [p[2] for p in per]

    def mmm(v):
        return [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]

    obs = pkg.Engine(0)
    try:
        t_up = prepare(eng, False)
        t_up_obs = prepare(obs, True)
        plain_bytes, obs_bytes = eng.tensor_storage_info(0)[2], obs.tensor_storage_info(0)[2]
        emit({'what': 'setup', 'dims': dims, 'nnz_given': nnz, 'nnz_coalesced': int(plain_bytes // (N * (4 * N + 8))),
              'R': R, 'skew': a.skew, 'reps': a.reps, 'gen_s': round(t_gen, 2), 'upload_s': round(t_up, 2),
              'upload_observed_s': round(t_up_obs, 2), 'resident_bytes': int(plain_bytes),
              'resident_bytes_observed': int(obs_bytes)})
        for n in range(N):
            mttkrp_once(eng, n), mttkrp_once(obs, n)
        step_once(obs)                                # warm-up
        plain, imputed, steps = [[] for _ in range(N)], [[] for _ in range(N)], []
        for _ in range(a.reps):                       # alternating, same process, same data
            for n in range(N):
                plain[n].append(mttkrp_once(eng, n))
                imputed[n].append(mttkrp_once(obs, n))
            steps.append(step_once(obs))
        for n in range(N):
            pk, ik = [v[0] for v in plain[n]], [v[0] for v in imputed[n]]
            ps = [s[1][n] for s in steps]
            emit({'what': 'observed_mode', 'mode': n + 1, 'rows': dims[n], 'carries_statistics': n == 0,
                  'plain_mttkrp_ms': mmm(pk), 'imputed_mttkrp_ms': mmm(ik), 'em_pass_ms': mmm(ps),
                  'em_pass_GB': round(steps[0][2][n] / 1e9, 3),
                  'em_pass_TBps': round(steps[0][2][n] / float(np.median(ps)) / 1e9, 3),
                  'em_pass_over_plain_mttkrp': round(float(np.median(ps)) / float(np.median(pk)), 3),
                  'imputed_over_plain_mttkrp': round(float(np.median(ik)) / float(np.median(pk)), 3),
                  'N_over_N_minus_1': round(N / (N - 1.0), 3)})
        emit({'what': 'observed_step', 'em_step_ms': mmm([s[0] for s in steps]),
              'passes_ms_sum': round(float(np.median([sum(s[1]) for s in steps])), 4)})
        # the pass of a first step: statistics without a snapshot
        first = []
        for _ in range(a.reps):
            obs.set_observed_only(0)
            first.append(step_once(obs)[1][0])
        emit({'what': 'observed_first_pass', 'statistics_pass_no_snapshot_ms': mmm(first)})
        # one outer iteration, wall: solves of 3 and of 1 iterations from the same factors
        it = {}
        for name, e in (('plain', eng), ('observed', obs)):
            w = []
            for _ in range(a.reps):
                set_factors(e)
                t1 = solve(e, 1)
                set_factors(e)
                t3 = solve(e, 3)
                w.append((t3 - t1) / 2)
            it[name] = w
        emit({'what': 'observed_iteration', 'plain_iter_ms_wall': mmm(it['plain']), 'observed_iter_ms_wall': mmm(it['observed']),
              'ratio': round(float(np.median(it['observed'])) / float(np.median(it['plain'])), 3)})
    finally:
        obs.close()
        out.close()


def run_weighted(a, eng, dims, N, R, nnz, subs, vals, t_gen):
    lib = eng.lib
    out = open(a.out, 'a')

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def mmm(v):
        return [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]

    # the stored entries once each (column-major linear index; the sizes' product must fit in 63 bits)
    t0 = time.time()
    assert float(np.prod([float(s) for s in dims])) < 2.0 ** 63, 'linear index of --dims does not fit in int64'
    lin = np.zeros(nnz, dtype=np.int64)
    stride = 1
    for m, s in enumerate(dims):
        lin += subs[:, m] * stride
        stride *= s
    _, first = np.unique(lin, return_index=True)
    del lin
    if len(first) < nnz:
        first.sort()
        subs, vals = np.asfortranarray(subs[first]), vals[first]
    nnz_c = len(vals)
    wts = np.random.default_rng(a.seed + 2).random(nnz_c)
    t_unique = time.time() - t0

    def set_factors(e):
        rng = np.random.default_rng(a.seed + 1)
        for m in range(N):
            Um = np.asfortranarray(rng.random((dims[m], R)))
            capi.check(lib.aoadmm_state_set(e.h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], R))

    def mark(e, weighted):
        if weighted:
            e.set_entry_weights(0, subs, wts, a.weights)
        else:
            e.set_observed_only(0)

    def prepare(e, weighted):
        h = e.h
        capi.check(lib.aoadmm_model_begin(h, N, 1, 0))
        for m, s in enumerate(dims):
            capi.check(lib.aoadmm_model_set_mode(h, m, s, R))
        capi.check(lib.aoadmm_model_add_cp(h, 0, N, (C.c_int * N)(*range(N)), 1.0))
        for m in range(N):
            capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
        capi.check(lib.aoadmm_model_end(h))
        e.upload_coo(0, subs, vals)
        e.synchronize()
        t0 = time.time()
        mark(e, weighted)
        e.synchronize()
        t_mark = time.time() - t0
        set_factors(e)
        o = capi.Options()
        o.MaxOuterIters, o.MaxInnerIters, o.use_dimtree = 1, 1, 1
        res = capi.Result()
        capi.check(lib.aoadmm_solve(e.h, C.byref(o), C.byref(res)))   # row-major factor copies and a snapshot
        return t_mark

    def step_once(e):
        """([ms of the pass over every copy], [their algorithmic bytes]) of one EM step"""
        for c in [3] + [4 + n for n in range(N)]:
            e.kernel_stats(c, reset=True)
        e.em_step(0)
        per = [e.kernel_stats(4 + n, reset=True) for n in range(N)]
        return [p[0] for p in per], [p[2] for p in per]

    wtd = pkg.Engine(0)
    try:
        t_mark_obs = prepare(eng, False)
        t_mark_wtd = prepare(wtd, True)
        emit({'what': 'setup', 'dims': dims, 'nnz_given': nnz, 'nnz_coalesced': int(nnz_c), 'R': R, 'skew': a.skew,
              'reps': a.reps, 'alpha': a.weights, 'gen_s': round(t_gen, 2), 'unique_s': round(t_unique, 2),
              'mark_s': round(t_mark_obs, 2), 'set_entry_weights_s': round(t_mark_wtd, 2),
              'resident_bytes_observed': int(eng.tensor_storage_info(0)[2]),
              'resident_bytes_weighted': int(wtd.tensor_storage_info(0)[2])})
        step_once(eng), step_once(wtd)                # warm-up
        so, sw = [], []
        for _ in range(a.reps):                       # alternating, same process, same data
            so.append(step_once(eng))
            sw.append(step_once(wtd))
        for n in range(N):
            po, pw = [s[0][n] for s in so], [s[0][n] for s in sw]
            emit({'what': 'weighted_mode', 'mode': n + 1, 'rows': dims[n], 'statistics_pass': n == 0,
                  'observed_pass_ms': mmm(po), 'weighted_pass_ms': mmm(pw),
                  'observed_pass_GB': round(so[0][1][n] / 1e9, 3), 'weighted_pass_GB': round(sw[0][1][n] / 1e9, 3),
                  'weighted_pass_TBps': round(sw[0][1][n] / float(np.median(pw)) / 1e9, 3),
                  'time_ratio': round(float(np.median(pw)) / float(np.median(po)), 4),
                  'bytes_ratio': round(sw[0][1][n] / so[0][1][n], 4)})
        fo, fw = [], []
        for _ in range(a.reps):                       # a first step: statistics without a snapshot
            mark(eng, False)
            fo.append(step_once(eng)[0][0])
            wtd.set_observed_only(0)                  # marked again: the weights stay, the snapshot goes
            fw.append(step_once(wtd)[0][0])
        emit({'what': 'weighted_first_pass', 'observed_statistics_pass_no_snapshot_ms': mmm(fo),
              'weighted_statistics_pass_no_snapshot_ms': mmm(fw),
              'time_ratio': round(float(np.median(fw)) / float(np.median(fo)), 4)})
    finally:
        wtd.close()
        out.close()


def run_heldout(a, eng, dims, N, R, nnz, subs, vals, t_gen):
    lib = eng.lib
    out = open(a.out, 'a')

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def mmm(v):
        return [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]

    def solve(e, iters):
        o = capi.Options()
        o.MaxOuterIters, o.MaxInnerIters, o.use_dimtree = iters, 1, 1
        res = capi.Result()
        e.synchronize()
        t0 = time.time()
        capi.check(lib.aoadmm_solve(e.h, C.byref(o), C.byref(res)))
        e.synchronize()
        return (time.time() - t0) * 1e3

    def set_factors(e):
        rng = np.random.default_rng(a.seed + 1)
        for m in range(N):
            Um = np.asfortranarray(rng.random((dims[m], R)))
            capi.check(lib.aoadmm_state_set(e.h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], R))

    k = int(round(a.heldout * nnz))
    hs, hv = np.ascontiguousarray(subs[:k]), np.ascontiguousarray(vals[:k])
    ts, tv = subs[k:], vals[k:]
    order = np.argsort(hs[:, 0], kind='stable')
    hs_sorted, hv_sorted = np.ascontiguousarray(hs[order]), np.ascontiguousarray(hv[order])

    def prepare(e, observed):
        h = e.h
        capi.check(lib.aoadmm_model_begin(h, N, 1, 0))
        for m, s in enumerate(dims):
            capi.check(lib.aoadmm_model_set_mode(h, m, s, R))
        capi.check(lib.aoadmm_model_add_cp(h, 0, N, (C.c_int * N)(*range(N)), 1.0))
        for m in range(N):
            capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
        capi.check(lib.aoadmm_model_end(h))
        e.upload_coo(0, ts, tv)
        if observed:
            e.set_observed_only(0)
        set_factors(e)
        solve(e, 1)                                   # row-major factor copies; the observed block takes its snapshot

    def pass_once(e):
        e.kernel_stats(12, reset=True)
        e.heldout_stats(0)
        ms, launches, by, _ = e.kernel_stats(12, reset=True)
        assert launches == 1
        return ms, by

    def residual_once(e):
        for c in [3] + [4 + n for n in range(N)]:
            e.kernel_stats(c, reset=True)
        e.em_step(0)
        return [e.kernel_stats(4 + n, reset=True)[0] for n in range(N)]

    def iteration(e):
        set_factors(e)
        t1 = solve(e, 1)
        set_factors(e)
        t3 = solve(e, 3)
        return (t3 - t1) / 2

    if a.keep_best:
        # The snapshot is taken when the held-out sum improves.  The solve is bit-reproducible, so the list is given the
        # model's own values after `iters` iterations: H_i = |m_i - m_iters|^2 then falls as the iterates approach their
        # last one, and every iteration of the timed solves takes a snapshot (the worst case; the count is reported).
        iters = 4
        try:
            prepare(eng, False)
            set_factors(eng)
            solve(eng, iters)
            eng.set_heldout(0, hs, eng.model_at(0, hs))
            state_bytes = 8 * R * sum(dims)

            def solve_kept(on):
                eng.heldout_keep_best(on)
                set_factors(eng)
                return solve(eng, iters), eng.heldout_best_info()

            solve_kept(True), solve_kept(False)           # warm-up
            w_on, w_off, shots = [], [], []
            for _ in range(a.reps):                       # alternating: switch on, switch off
                t, info = solve_kept(True)
                w_on.append(t)
                shots.append(info['launches'])
                assert info['bytes'] == info['launches'] * 2 * state_bytes
                w_off.append(solve_kept(False)[0])
            solve_kept(True)
            t_restore = []
            for _ in range(a.reps):
                eng.synchronize()
                t0 = time.time()
                eng.heldout_restore_best()
                t_restore.append((time.time() - t0) * 1e3)
            emit({'what': 'keep_best_solve', 'block': 'plain', 'dims': dims, 'nnz_given': nnz, 'heldout_n': k, 'R': R,
                  'skew': a.skew, 'reps': a.reps, 'iters': iters, 'state_bytes': state_bytes,
                  'snapshot_bytes_moved': 2 * state_bytes, 'solve_ms_wall_switch_on': mmm(w_on),
                  'solve_ms_wall_switch_off': mmm(w_off), 'snapshots_per_solve': shots,
                  'added_ms_per_snapshot': round((float(np.median(w_on)) - float(np.median(w_off))) / max(shots[0], 1), 4),
                  'restore_ms_wall': mmm(t_restore)})
        finally:
            out.close()
        return
    obs = pkg.Engine(0)
    try:
        prepare(eng, False)
        prepare(obs, True)
        nnz_train = eng.tensor_storage_info(0)[2] // (N * (4 * N + 8))
        t0 = time.time()
        eng.set_heldout(0, hs, hv)
        t_attach = time.time() - t0
        emit({'what': 'setup', 'dims': dims, 'nnz_given': nnz, 'heldout_frac': a.heldout, 'heldout_n': k,
              'train_nnz_coalesced': int(nnz_train), 'R': R, 'skew': a.skew, 'reps': a.reps, 'gen_s': round(t_gen, 2),
              'attach_s': round(t_attach, 2), 'heldout_info': eng.heldout_info(0)})
        pass_once(eng), residual_once(obs)            # warm-up
        caller, res = [], []
        for _ in range(a.reps):                       # alternating, same process
            caller.append(pass_once(eng))
            res.append(residual_once(obs))
        eng.set_heldout(0, hs_sorted, hv_sorted)
        pass_once(eng)
        srt = [pass_once(eng) for _ in range(a.reps)]
        eng.set_heldout(0, hs, hv)
        assert eng.heldout_info(0)['row_major'] == 1
        ho = float(np.median([v[0] for v in caller]))
        r23 = float(np.median([(v[1] + v[2]) / 2 for v in res])) if N >= 3 else float(np.median([v[1] for v in res]))
        emit({'what': 'heldout_pass', 'heldout_pass_ms': mmm([v[0] for v in caller]),
              'heldout_pass_sorted_by_mode1_ms': mmm([v[0] for v in srt]), 'GB': round(caller[0][1] / 1e9, 3),
              'TBps': round(caller[0][1] / ho / 1e9, 3),
              'residual_pass_ms_by_mode': [mmm([v[n] for v in res]) for n in range(N)],
              'ns_per_heldout_entry': round(ho * 1e6 / k, 5), 'ns_per_nonzero_residual_modes_2_3': round(r23 * 1e6 / nnz_train, 5),
              'per_entry_ratio': round((ho / k) / (r23 / nnz_train), 3)})
        it = {}
        for name, e in (('plain', eng), ('observed', obs)):
            w_list, w_none = [], []
            iteration(e)                              # warm-up
            for _ in range(a.reps):                   # alternating: list attached, list removed
                e.set_heldout(0, hs, hv)
                w_list.append(iteration(e))
                e.set_heldout(0, hs[:0], hv[:0])
                w_none.append(iteration(e))
            it[name] = (w_list, w_none)
            emit({'what': 'heldout_iteration', 'block': name, 'iter_ms_wall_with_list': mmm(w_list),
                  'iter_ms_wall_no_list': mmm(w_none),
                  'added_ms': round(float(np.median(w_list)) - float(np.median(w_none)), 4)})
    finally:
        obs.close()
        out.close()


def run_ranklist(a, eng, dims, N, R, nnz, subs, vals, t_gen):
    lib = eng.lib
    out = open(a.out, 'a')

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def mmm(v):
        return [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]

    def solve(e, iters):
        o = capi.Options()
        o.MaxOuterIters, o.MaxInnerIters, o.use_dimtree = iters, 1, 1
        res = capi.Result()
        e.synchronize()
        t0 = time.time()
        capi.check(lib.aoadmm_solve(e.h, C.byref(o), C.byref(res)))
        e.synchronize()
        return (time.time() - t0) * 1e3

    def set_factors(e):
        rng = np.random.default_rng(a.seed + 1)
        for m in range(N):
            Um = np.asfortranarray(rng.random((dims[m], R)))
            capi.check(lib.aoadmm_state_set(e.h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], R))

    M, nq = a.rank_every, a.ranklist
    span = 2 * M                                      # iterations between the two timed solves: two evaluations

    def iteration(e):
        """wall time per outer iteration and, with a list, the event time of one evaluation's launches"""
        set_factors(e)
        t1 = solve(e, M)
        set_factors(e)
        e.kernel_stats(13, reset=True)
        t3 = solve(e, M + span)
        ms, launches, _, _ = e.kernel_stats(13, reset=True)
        return (t3 - t1) / span, (ms / launches if launches else 0.0), launches

    try:
        h = eng.h
        capi.check(lib.aoadmm_model_begin(h, N, 1, 0))
        for m, s in enumerate(dims):
            capi.check(lib.aoadmm_model_set_mode(h, m, s, R))
        capi.check(lib.aoadmm_model_add_cp(h, 0, N, (C.c_int * N)(*range(N)), 1.0))
        for m in range(N):
            capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
        capi.check(lib.aoadmm_model_end(h))
        eng.upload_coo(0, subs, vals)
        set_factors(eng)
        solve(eng, 1)                                 # row-major factor copies
        emit({'what': 'setup', 'dims': dims, 'nnz_given': nnz, 'R': R, 'skew': a.skew, 'reps': a.reps, 'nq': nq, 'rank_every': M,
              'gen_s': round(t_gen, 2)})
        rng = np.random.default_rng(a.seed + 2)
        q = np.stack([rng.integers(0, s, nq) for s in dims], axis=1).astype(np.int64)
        for ne in (0, 100):
            ex = None
            if ne:
                ex = (np.arange(nq + 1, dtype=np.int64) * ne, rng.integers(0, dims[0], nq * ne).astype(np.int64))

            def alone():
                eng.kernel_stats(13, reset=True)
                eng.rank_of(0, 0, q, exclude=ex)
                ms, launches, _, _ = eng.kernel_stats(13, reset=True)
                assert launches == 1
                return ms

            t0 = time.time()
            eng.set_ranklist(0, 0, q, exclude=ex)
            t_attach = (time.time() - t0) * 1e3
            eng.rank_track(metric='ndcg', k=10, every=M)
            info = eng.ranklist_info(0)
            iteration(eng), alone()                   # warm-up
            w_list, w_none, ev, sa = [], [], [], []
            for _ in range(a.reps):                   # alternating: list attached, list removed, the stand-alone call
                eng.set_ranklist(0, 0, q, exclude=ex)
                w, e_ms, launches = iteration(eng)
                assert launches == 4                  # 3 M iterations: evaluations at 0, M, 2 M and 3 M
                w_list.append(w)
                ev.append(e_ms)
                eng.set_ranklist(0, 0, q[:0])
                w_none.append(iteration(eng)[0])
                sa.append(alone())
            added_wall = (float(np.median(w_list)) - float(np.median(w_none))) * M
            emit({'what': 'rank_track_iteration', 'nq': nq, 'excl_per_query': ne, 'rank_every': M, 'attach_ms': round(t_attach, 3),
                  'ranklist_info': info, 'iter_ms_wall_with_list': mmm(w_list), 'iter_ms_wall_no_list': mmm(w_none),
                  'added_ms_wall_per_evaluated_iteration': round(added_wall, 4), 'evaluation_ms_events_in_solve': mmm(ev),
                  'rank_of_alone_ms_events': mmm(sa),
                  'evaluation_minus_alone_ms': round(float(np.median(ev)) - float(np.median(sa)), 4)})
        for n in (16384, 10 ** 7):
            rank = rng.integers(-1, 10 ** 6, n).astype(np.int64)
            ncand = np.full(n, 10 ** 6, dtype=np.int64)
            eng.op_rank_metrics(rank, ncand, 10)
            t = []
            for _ in range(a.reps):
                t0 = time.time()
                eng.op_rank_metrics(rank, ncand, 10)
                t.append((time.time() - t0) * 1e3)
            emit({'what': 'rank_metrics', 'n': n, 'op_ms_wall_with_uploads': mmm(t), 'bytes_read_by_the_kernels': 16 * n})
    finally:
        out.close()


def run(a, eng, dims, N, R, nnz, subs, vals, t_gen):
    rng = np.random.default_rng(a.seed + 1)
    lib, h = eng.lib, eng.h
    capi.check(lib.aoadmm_model_begin(h, N, 1, 0))
    for m, s in enumerate(dims):
        capi.check(lib.aoadmm_model_set_mode(h, m, s, R))
    modes = (C.c_int * N)(*range(N))
    capi.check(lib.aoadmm_model_add_cp(h, 0, N, modes, 1.0))
    for m in range(N):
        capi.check(lib.aoadmm_model_set_coupling(h, m, -1, None, 0, 0, None, 0, 0))
    capi.check(lib.aoadmm_model_end(h))
    t0 = time.time()
    eng.upload_coo(0, subs, vals)
    eng.synchronize()
    t_up = time.time() - t0
    normsq = C.c_double(0)
    capi.check(lib.aoadmm_tensor_normsq(h, 0, C.byref(normsq)))
    U = [rng.random((s, R)) for s in dims]
    for m in range(N):
        Um = np.asfortranarray(U[m])
        capi.check(lib.aoadmm_state_set(h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], R))
    print(json.dumps({'what': 'setup', 'dims': dims, 'nnz_given': nnz, 'R': R, 'skew': a.skew, 'gen_s': round(t_gen, 2),
                      'upload_s': round(t_up, 2), 'normsq': normsq.value}), flush=True)
    rows = []

    def time_modes(layout):
        for n in range(N):
            out = np.zeros((dims[n], R), order='F')
            ms = C.c_float(0)
            capi.check(lib.aoadmm_resident_mttkrp(h, 0, n, None, C.byref(ms)))          # warm-up
            eng.kernel_stats(3, reset=True)
            ev = []
            for _ in range(a.reps):
                capi.check(lib.aoadmm_resident_mttkrp(h, 0, n, None, C.byref(ms)))
                ev.append(ms.value)
            kms, launches, by, fl = eng.kernel_stats(3, reset=True)
            per = kms / launches
            bpl = by / launches
            r = {'what': 'mttkrp_coo', 'layout': layout, 'mode': n + 1, 'ms': round(per, 4),
                 'ms_events_min': round(min(ev), 4), 'GB': round(bpl / 1e9, 3), 'TBps': round(bpl / per / 1e9, 3),
                 'hbm_share': round(bpl / (per * 1e-3) / PEAK, 3), 'GFLOPs': round(fl / launches / per / 1e6, 1)}
            if n == 0:
                capi.check(lib.aoadmm_resident_mttkrp(h, 0, n, capi.dptr(out), C.byref(ms)))
                r['checksum'] = float(out.sum())
            rows.append(r)
            print(json.dumps(r), flush=True)

    time_modes('colmajor')
    # one outer iteration (unconstrained, no couplings): the Gram kernels leave the row-major factor copies behind
    o = capi.Options()
    o.MaxOuterIters, o.MaxInnerIters, o.use_dimtree = 1, 1, 1
    res = capi.Result()
    capi.check(lib.aoadmm_solve(h, C.byref(o), C.byref(res)))
    time_modes('rowmajor')
    if not a.no_torch:
        import torch
        dev = torch.device('cuda:0')
        # the coalesced data the library holds would differ only in a few duplicates; the reference takes the raw COO
        ts = torch.from_numpy(np.ascontiguousarray(subs.T)).to(dev)
        tv = torch.from_numpy(vals).to(dev)
        Uf = []
        for m in range(N):
            Um = np.zeros((dims[m], R), order='F')
            capi.check(lib.aoadmm_state_get(h, capi.F_FAC, m, 0, capi.dptr(Um), dims[m], R))
            Uf.append(torch.from_numpy(np.ascontiguousarray(Um)).to(dev))
        for n in range(N):
            def torch_mttkrp():
                p = tv[:, None].clone()
                for m in range(N):
                    if m != n:
                        p = p * Uf[m].index_select(0, ts[m])
                o_ = torch.zeros(dims[n], R, dtype=torch.float64, device=dev)
                o_.index_add_(0, ts[n], p)
                return o_
            torch_mttkrp()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                torch_mttkrp()
            e1.record()
            torch.cuda.synchronize()
            per = e0.elapsed_time(e1) / a.reps
            ours = [r for r in rows if r.get('layout') == 'rowmajor' and r['mode'] == n + 1][0]
            r = {'what': 'torch_index_add', 'mode': n + 1, 'ms': round(per, 4), 'speedup_of_coo': round(per / ours['ms'], 2)}
            rows.append(r)
            print(json.dumps(r), flush=True)
    rm = [r for r in rows if r.get('layout') == 'rowmajor']
    print(json.dumps({'what': 'summary', 'skew': a.skew, 'rowmajor_ms_sum': round(sum(r['ms'] for r in rm), 3),
                      'rowmajor_TBps_mean': round(float(np.mean([r['TBps'] for r in rm])), 3)}), flush=True)


if __name__ == '__main__':
    main()
