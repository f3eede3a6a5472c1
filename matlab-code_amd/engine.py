"""Thin object wrapper over the C ABI context plus the op-level calls.

Mirrors the L2->L1 calls of the reference solver
(`functions/cmtf_fun_AOADMM.m:97` mttkrp, `:66` Gram, `:142` chol,
`functions/constraints_to_prox.m` prox handles, `:591-623` ADMM inner loop).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi

# constraint names of "List of constraints and regularizations.txt" -> ids of include/aoadmm_hip.h
CONSTRAINT_IDS = {
    'non-negativity': 1, 'box': 2, 'simplex column-wise': 3, 'simplex row-wise': 4, 'non-decreasing': 5,
    'non-increasing': 6, 'unimodality': 7, 'l1-ball': 8, 'l2-ball': 9, 'non-negative l2-ball': 10,
    'non-negative l2-sphere': 11, 'orthonormal': 12, 'l1 regularization': 13, 'l0 regularization': 14,
    'l2 regularization': 15, 'ridge': 16, 'quadratic regularization': 17, 'GL smoothness': 18,
    'TV regularization': 19, 'tPARAFAC2': 20,
}


def constraint_descriptor(c):
    """`Z.constraints{m}` cell -> (id, params, Lmat) (constraints_to_prox.m:13-91)."""
    if c is None or len(c) == 0:
        raise ValueError('No constraint provided')
    name = c[0]
    if name == 'custom':
        raise capi.UnsupportedOnDevice(capi.ERR_UNSUPPORTED,
                                       "'custom' prox handles cannot cross to the device (constraints_to_prox.m:86-90)")
    if name not in CONSTRAINT_IDS:
        raise ValueError('unknown constraint %r' % (name,))
    cid = CONSTRAINT_IDS[name]
    params = []
    Lmat = None
    if name == 'quadratic regularization':
        params = [float(c[1])]
        Lmat = capi.as_f(c[2])
    elif name == 'unimodality':
        params = [1.0 if c[1] else 0.0]
    else:
        params = [float(v) for v in c[1:]]
    return cid, np.asarray(params, dtype=np.float64), Lmat


class Engine:
    """One `aoadmm_ctx`: one GPU (`Engine(0)`), or several GPUs driven from this one process (`Engine([0, 1, 2, 3])`,
    aoadmm_create_multi: one engine + one host thread per device inside the library, RCCL between them).
    Raises when no GPU / library is available."""

    def __init__(self, device=0):
        self.lib = capi.load_library()
        self.h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            devs = (C.c_int * len(device))(*[int(d) for d in device])
            capi.check(self.lib.aoadmm_create_multi(C.byref(self.h), len(device), devs))
        else:
            capi.check(self.lib.aoadmm_create(C.byref(self.h), int(device)))

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.aoadmm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        capi.check(self.lib.aoadmm_synchronize(self.h))

    # ---- communicator ---------------------------------------------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        capi.check(self.lib.aoadmm_comm_unique_id(buf))
        return buf.raw

    def comm_init_rank(self, uid, rank, world):
        """Rank `rank` of a `world`-rank RCCL communicator (`aoadmm_comm_init_rank`).  Afterwards `build_model` shards
        dense CP blocks by rows, and with 'f16' it is a collective whose scale comes from the whole tensor."""
        capi.check(self.lib.aoadmm_comm_init_rank(self.h, uid, int(rank), int(world)))

    def comm_init_rank_share(self, uid, rank, world):
        """Measurement hook: rank `rank` of `world` in every sharding decision, on a ONE-rank RCCL communicator.  Nothing
        is learnt from peers: sums are partial, and an 'f16' block takes its scale from this rank's rows and mode-3 slab."""
        capi.check(self.lib.aoadmm_comm_init_rank_share(self.h, uid, int(rank), int(world)))

    def comm_rank(self):
        """(rank, world) of this engine's communicator; (0, 1) without one."""
        r, w = C.c_int(0), C.c_int(1)
        capi.check(self.lib.aoadmm_comm_rank(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_info(self):
        """{'rccl_version', 'comm_ranks', 'librccl'}: what the collectives of this context run on."""
        v, n = C.c_int(0), C.c_int(0)
        buf = C.create_string_buffer(1024)
        capi.check(self.lib.aoadmm_comm_info(self.h, C.byref(v), C.byref(n), buf, 1024))
        return {'rccl_version': v.value, 'comm_ranks': n.value, 'librccl': buf.value.decode('utf-8', 'replace')}

    def comm_init_local(self, key, rank, world):
        """Bring-up/test transport: engines driven by threads of this process form group `key` (see aoadmm_hip.h).  As on
        RCCL ranks, an 'f16' `build_model` is a collective here: all ranks of the group must make it together."""
        capi.check(self.lib.aoadmm_comm_init_local(self.h, int(key), int(rank), int(world)))

    # ---- data -----------------------------------------------------------------------
    def upload_coo(self, p, subs, vals, sharded=False):
        """Z.object{p} of a CP block as COO nonzeros (`aoadmm_tensor_upload_coo`): subs nnz x N, 0-based; vals nnz.
        Duplicates are summed on the device; the sizes are those of the model.  sharded
        (`aoadmm_tensor_upload_coo_sharded`): every rank of the communicator makes the call with the whole list and keeps
        its share of the coalesced nonzeros (`capi.coo_share`); the block's MTTKRPs are collectives afterwards.  Without
        a communicator it is the plain upload."""
        subs = np.asarray(subs, dtype=np.int64)
        vals = np.ascontiguousarray(np.asarray(vals, dtype=np.float64).reshape(-1))
        if subs.ndim != 2 or subs.shape[0] != vals.shape[0]:
            raise ValueError('upload_coo: subs must be nnz x N with nnz = len(vals)')
        subs = np.asfortranarray(subs)                # column-major nnz x N (the layout of sptensor.subs)
        upload = self.lib.aoadmm_tensor_upload_coo_sharded if sharded else self.lib.aoadmm_tensor_upload_coo
        capi.check(upload(self.h, int(p), int(vals.shape[0]), subs.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(vals)))

    def upload_par2_coo(self, p, subs, vals):
        """The slabs of a PARAFAC2 block as COO nonzeros (`aoadmm_par2_slab_upload_coo`): subs nnz x 3, 0-based
        (i, j within the slab, k), all slabs in one call; vals nnz.  Duplicates are summed on the device."""
        subs = np.asarray(subs, dtype=np.int64)
        vals = np.ascontiguousarray(np.asarray(vals, dtype=np.float64).reshape(-1))
        if subs.size == 0:
            subs = np.zeros((0, 3), dtype=np.int64)
        if subs.ndim != 2 or subs.shape[1] != 3 or subs.shape[0] != vals.shape[0]:
            raise ValueError('upload_par2_coo: subs must be nnz x 3 with nnz = len(vals)')
        subs = np.asfortranarray(subs)
        capi.check(self.lib.aoadmm_par2_slab_upload_coo(self.h, int(p), int(vals.shape[0]),
                                                        subs.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(vals)))

    def resident_par2_rhs(self, p, tensor_mode, rows, R, with_ms=False):
        """Unweighted right-hand side of tensor mode 0 (I x R), 1 (sum J_k x R, slabs back to back, each J_k x R
        column-major) or 2 (K x R) of a PARAFAC2 block with sparse slabs (`aoadmm_resident_par2_rhs`).  Mode 1 comes
        back as the packed vector of the state fields; with_ms: (result, device ms)."""
        out = np.zeros(rows * R) if tensor_mode == 1 else np.zeros((rows, R), order='F')
        ms = C.c_float(0)
        capi.check(self.lib.aoadmm_resident_par2_rhs(self.h, int(p), int(tensor_mode), capi.dptr(out), C.byref(ms)))
        return (out, ms.value) if with_ms else out

    def set_observed_only(self, p, on=True):
        """Marks the sparse CP block p observed-only (`aoadmm_tensor_set_observed_only`): its stored entries are the
        observations and every other entry is missing, fitted by the reference's EM step without a dense array.  For a
        block uploaded with `upload_coo` (not sharded) that holds at least one entry; any later upload clears it."""
        capi.check(self.lib.aoadmm_tensor_set_observed_only(self.h, int(p), int(bool(on))))

    def set_entry_weights(self, p, subs, wts, unstored_weight=0.0):
        """Weights for the sparse CP block p (`aoadmm_tensor_set_entry_weights`): wts[e] in [0, 1] for the stored entry
        subs[e] (subs nnz x N, 0-based, any order, exactly the block's stored entries once each) and `unstored_weight`
        in [0, 1] for every other entry.  subs = wts = None sets `unstored_weight` alone, with stored weights 1.  Marks
        the block observed-only if it is not; weights above 1 are the caller's to normalise (divide by the maximum)."""
        if wts is None:
            if subs is not None:
                raise ValueError('set_entry_weights: subs without wts')
            capi.check(self.lib.aoadmm_tensor_set_entry_weights(self.h, int(p), 0, None, None, float(unstored_weight)))
            return
        subs = np.asarray(subs, dtype=np.int64)
        wts = np.ascontiguousarray(np.asarray(wts, dtype=np.float64).reshape(-1))
        if subs.ndim != 2 or subs.shape[0] != wts.shape[0]:
            raise ValueError('set_entry_weights: subs must be nnz x N with nnz = len(wts)')
        subs = np.asfortranarray(subs)
        capi.check(self.lib.aoadmm_tensor_set_entry_weights(self.h, int(p), int(wts.shape[0]),
                                                            subs.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(wts),
                                                            float(unstored_weight)))

    def tensor_weights_upload(self, p, W):
        """Per-entry weights for the dense CP block p (`aoadmm_tensor_weights_upload`): W has the block's shape (the full
        array under a communicator) with entries in [0, 1]; upload after the data.  None removes the weights.  An fp32
        block keeps W rounded to fp32.  A value outside [0, 1] raises `AoadmmError` (ERR_INVALID) and leaves the block
        as it was."""
        if W is None:
            capi.check(self.lib.aoadmm_tensor_weights_upload(self.h, int(p), None))
            return
        W = np.asfortranarray(np.asarray(W, dtype=np.float64))
        capi.check(self.lib.aoadmm_tensor_weights_upload(self.h, int(p), capi.dptr(W)))

    def em_step(self, p):
        """One EM step of the observed-only block p with the current factors (`aoadmm_resident_em_step`):
        (sum over the stored entries of (x - m)^2, num, den) of `f_rel_missing`; `resident_mttkrp` then returns the
        MTTKRP of the imputed tensor as of this step."""
        st = np.zeros(3)
        capi.check(self.lib.aoadmm_resident_em_step(self.h, int(p), capi.dptr(st)))
        return float(st[0]), float(st[1]), float(st[2])

    def resident_em_pass(self, p, dims, R, update=1, fuse=0, with_data=True):
        """One EM pass over the masked or weighted dense block p with the current factors, as a solve runs it
        (`aoadmm_resident_em_pass`).  dims: the block's sizes (a PARAFAC2 block: (I, [J_k], K)); fuse: 0 none, 1 the
        solver's choice, 2 the second mode.  Returns a dict: stats = (num, den, obs_res, obs_x2) as a float64 array;
        data = the block after the pass as doubles (PARAFAC2: a list of I x J_k slabs), data_t = a matrix block's
        transposed copy (J x I), both None without with_data; mttkrp = the MTTKRP of tensor mode `mttkrp_mode` finished
        from the partial contraction the pass fused (None when it fused none); info = dict(vec, rmax, fused, walk,
        strips, jchunks, jlen)."""
        stats = np.zeros(4)
        info = np.zeros(8, dtype=np.int64)
        par2 = isinstance(dims[1], (list, tuple))
        data = data_t = None
        if with_data:
            if par2:
                data = np.zeros(int(dims[0]) * int(sum(dims[1])))
            else:
                data = np.zeros(tuple(int(d) for d in dims), order='F')
                if len(dims) == 2:
                    data_t = np.zeros((int(dims[1]), int(dims[0])), order='F')
        rows = 0 if par2 else max(int(d) for d in dims)
        mt = np.zeros((max(rows, 1), int(R)), order='F')           # room for any mode; cut to the mode reported
        capi.check(self.lib.aoadmm_resident_em_pass(self.h, int(p), int(update), int(fuse), capi.dptr(stats),
                                                    capi.dptr(data), capi.dptr(data_t), capi.dptr(mt),
                                                    info.ctypes.data_as(C.POINTER(C.c_int64))))
        if par2 and with_data:
            off = np.concatenate([[0], np.cumsum([int(j) for j in dims[1]])]) * int(dims[0])
            data = [data[off[k]:off[k + 1]].reshape((int(dims[0]), int(j)), order='F').copy()
                    for k, j in enumerate(dims[1])]
        mode = int(info[7])
        mttkrp = None
        if mode >= 0:
            n = int(dims[mode])
            mttkrp = np.array(mt.ravel(order='F')[:n * int(R)].reshape((n, int(R)), order='F'), order='F')
        return dict(stats=stats, data=data, data_t=data_t, mttkrp=mttkrp, mttkrp_mode=mode,
                    info=dict(vec=int(info[0]), rmax=int(info[1]), fused=int(info[2]), walk=int(info[3]),
                              strips=int(info[4]), jchunks=int(info[5]), jlen=int(info[6])))

    # ---- the missing entries of a masked dense block as a list -------------------------
    def set_missing_list(self, p, on=True):
        """Marks the masked dense CP block p (`aoadmm_tensor_set_missing_list`): the list of its missing entries is built
        on the device from the resident mask, and every imputing EM pass of the block then evaluates the model at the
        listed entries only instead of passing over the whole array.  Opt-in; on=False releases the list, as does any
        later upload of the block's data, mask or weights.  The iteration-0 objective stays the dense pass's, bit for
        bit.  Later objective values of a marked block are formed from the iteration's last MTTKRP like an unmasked
        block's, (obs_x2 + den) - 2 <Xhat, M> + ||M||^2 - num clamped at 0, and so have that form's absolute floor of
        about u * ||Xhat||^2 (u = 2^-53), where an unmarked block's directly summed residual has none: leave a
        noise-free fit to machine precision unmarked.  Raises `AoadmmError` with ERR_UNSUPPORTED for a PARAFAC2, sparse
        or weighted block, under a communicator of more than one rank and on a multi-device context, ERR_INVALID for a
        block without a mask, ERR_NOMEM (block unchanged) when the list does not fit."""
        capi.check(self.lib.aoadmm_tensor_set_missing_list(self.h, int(p), int(bool(on))))

    def missing_list(self, p, nmodes=None):
        """The list of the marked block p (`aoadmm_tensor_missing_list`): without `nmodes` the number of entries; with
        the block's order N an int64 array n x N of their 0-based subscripts in list order (ascending column-major
        storage offset)."""
        n = C.c_int64(0)
        capi.check(self.lib.aoadmm_tensor_missing_list(self.h, int(p), C.byref(n), None))
        if nmodes is None:
            return int(n.value)
        subs = np.zeros((int(n.value), int(nmodes)), dtype=np.int64, order='F')
        if n.value > 0:
            capi.check(self.lib.aoadmm_tensor_missing_list(self.h, int(p), None, subs.ctypes.data_as(C.POINTER(C.c_int64))))
        return subs

    def resident_em_list_pass(self, p, dims, update=1, with_data=True):
        """One list pass over the marked block p with the current factors, as a solve runs it
        (`aoadmm_resident_em_list_pass`).  Returns a dict: stats = (num, den) as a float64 array; data = the block after
        the pass as doubles, data_t = a matrix block's transposed copy (J x I), both None without with_data.  Timed
        under `kernel_stats(16)`."""
        stats = np.zeros(2)
        data = data_t = None
        if with_data:
            data = np.zeros(tuple(int(d) for d in dims), order='F')
            if len(dims) == 2:
                data_t = np.zeros((int(dims[1]), int(dims[0])), order='F')
        capi.check(self.lib.aoadmm_resident_em_list_pass(self.h, int(p), int(update), capi.dptr(stats), capi.dptr(data),
                                                         capi.dptr(data_t)))
        return dict(stats=stats, data=data, data_t=data_t)

    # ---- held-out scoring ------------------------------------------------------------
    @staticmethod
    def _subs_f(subs, what):
        subs = np.asarray(subs, dtype=np.int64)
        if subs.ndim != 2:
            raise ValueError('%s: subs must be n x N' % what)
        return np.asfortranarray(subs)                # column-major n x N (the layout of sptensor.subs)

    def model_at(self, p, subs):
        """The model of block p for the current factors at the subscripts `subs` (n x N, 0-based; a PARAFAC2 block:
        (i, j within slab k, k)), in the caller's order (`aoadmm_resident_model_at`).  Needs the model and the factor
        state, not the block's data; no array of the tensor's size exists."""
        subs = self._subs_f(subs, 'model_at')
        out = np.zeros(subs.shape[0])
        capi.check(self.lib.aoadmm_resident_model_at(self.h, int(p), int(subs.shape[0]),
                                                     subs.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(out)))
        return out

    def set_heldout(self, p, subs, vals):
        """Attaches the held-out list of block p (`aoadmm_tensor_set_heldout`): subs n x N, 0-based; vals n.  An empty
        list removes it.  Duplicates are scored once each.  The list belongs to the model: `build_model` drops it, a new
        upload of the block's data keeps it.  A solve then scores it with every evaluation of the objective."""
        vals = np.ascontiguousarray(np.asarray(vals, dtype=np.float64).reshape(-1))
        if vals.shape[0] == 0:
            capi.check(self.lib.aoadmm_tensor_set_heldout(self.h, int(p), 0, None, None))
            return
        subs = self._subs_f(subs, 'set_heldout')
        if subs.shape[0] != vals.shape[0]:
            raise ValueError('set_heldout: subs must be n x N with n = len(vals)')
        capi.check(self.lib.aoadmm_tensor_set_heldout(self.h, int(p), int(vals.shape[0]),
                                                      subs.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(vals)))

    def heldout_stats(self, p):
        """(sum (y - m)^2, sum y^2, sum m^2, n) of block p's held-out list for the current factors
        (`aoadmm_resident_heldout_stats`); `AoadmmError` (ERR_INVALID) without a list."""
        st = np.zeros(4)
        capi.check(self.lib.aoadmm_resident_heldout_stats(self.h, int(p), capi.dptr(st)))
        return float(st[0]), float(st[1]), float(st[2]), int(st[3])

    def heldout_info(self, p):
        """dict(n, resident_bytes, row_major) of block p's held-out list (`aoadmm_heldout_info`): n (4 N + 8) bytes;
        row_major: 1 when the block's last held-out pass gathered from the row-major factor copies, 0 from the
        column-major factors, -1 before any pass."""
        n, nb, rm = C.c_int64(0), C.c_int64(0), C.c_int(-1)
        capi.check(self.lib.aoadmm_heldout_info(self.h, int(p), C.byref(n), C.byref(nb), C.byref(rm)))
        return dict(n=n.value, resident_bytes=nb.value, row_major=rm.value)

    def heldout_trace(self, p):
        """(trace, best_iter) of the last solve (`aoadmm_heldout_trace`): sum (y - m)^2 of block p's list at iteration
        0 .. OuterIterations (empty without a list) and the iteration of the smallest weighted sum over the blocks."""
        ln, best = C.c_int(0), C.c_int(-1)
        capi.check(self.lib.aoadmm_heldout_trace(self.h, int(p), None, 0, C.byref(ln), C.byref(best)))
        out = np.zeros(max(ln.value, 1))
        capi.check(self.lib.aoadmm_heldout_trace(self.h, int(p), capi.dptr(out), ln.value, C.byref(ln), C.byref(best)))
        return out[:ln.value].copy(), best.value

    def heldout_keep_best(self, on=True):
        """Switch of the model (`aoadmm_heldout_keep_best`): every later solve keeps on the device a copy of the whole
        solver state of the iteration with the smallest weighted held-out sum (the earliest such; iteration 0 is the
        starting point).  The solve returns what it returned before; `heldout_restore_best` brings the copy back.
        `build_model` clears the switch, `on=False` releases the copy."""
        capi.check(self.lib.aoadmm_heldout_keep_best(self.h, int(on)))

    def heldout_restore_best(self):
        """Copies the kept state back into the engine's state (`aoadmm_heldout_restore_best`) and returns its iteration:
        the engine is then where a solve of that many iterations from the same start would have left it.  A second call
        returns the same; the next solve, any state upload and `build_model` invalidate the copy (`AoadmmError`,
        ERR_INVALID, when nothing is kept).  With a communicator every rank makes the call."""
        it = C.c_int(-1)
        capi.check(self.lib.aoadmm_heldout_restore_best(self.h, C.byref(it)))
        return it.value

    def heldout_best_info(self):
        """dict(have, iter, bytes, launches) (`aoadmm_heldout_best_info`): whether a kept state can be restored, its
        iteration (-1: none), and the snapshot launches of the last solve with the bytes they read and wrote."""
        have, it, nb, nl = C.c_int(0), C.c_int(-1), C.c_int64(0), C.c_int64(0)
        capi.check(self.lib.aoadmm_heldout_best_info(self.h, C.byref(have), C.byref(it), C.byref(nb), C.byref(nl)))
        return dict(have=bool(have.value), iter=it.value, bytes=nb.value, launches=nl.value)

    def topk(self, p, mode, subs, k, exclude=None):
        """The k best entries of CP block p along its mode `mode` (0-based position in the block) for every query
        (`aoadmm_resident_topk`).  subs is nq x N, 0-based; its column `mode` is ignored.  Query q scores every row i of
        the free mode, sum_r F_mode(i, r) prod_{m != mode} F_m(subs[q, m], r), and gets the k rows that come first in
        the order "larger score first, equal scores by smaller row" among those that are not excluded and whose score
        is not NaN.  exclude = (off, idx): off has nq + 1 offsets into idx, the excluded rows per query in any order
        (`sptensor.fiber_lists` gives the stored ones).  Returns (idx int64 nq x k, val float64 nq x k), padded with
        -1 and -inf.  Needs the model and the factor state, not the block's data; no nq x I_mode array exists."""
        subs = self._subs_f(subs, 'topk')
        i64p = C.POINTER(C.c_int64)
        return self._topk_call('topk', self.lib.aoadmm_resident_topk, p, mode, int(subs.shape[0]),
                               subs.ctypes.data_as(i64p), k, exclude, keep=subs)

    def _topk_call(self, what, entry, p, mode, nq, queries, k, exclude, keep=None):
        """The part `topk` and `topk_w` share: the outputs, the exclusion lists, the call.  `queries` is the pointer the
        entry takes as its fifth argument (the subscripts or the weights); `keep` holds its array alive."""
        k = int(k)
        idx = np.full((nq, max(k, 0)), -1, dtype=np.int64)
        val = np.full((nq, max(k, 0)), -np.inf)
        i64p = C.POINTER(C.c_int64)
        off = ex = None
        if exclude is not None:
            off = np.ascontiguousarray(np.asarray(exclude[0], dtype=np.int64).reshape(-1))
            ex = np.ascontiguousarray(np.asarray(exclude[1], dtype=np.int64).reshape(-1))
            if off.shape[0] != nq + 1:
                raise ValueError('%s: exclude[0] must hold nq + 1 = %d offsets, got %d' % (what, nq + 1, off.shape[0]))
            if off[-1] != ex.shape[0]:
                raise ValueError('%s: exclude[0][-1] = %d but exclude[1] holds %d rows' % (what, off[-1], ex.shape[0]))
            if ex.shape[0] == 0:
                ex = np.zeros(1, dtype=np.int64)          # a valid address for an empty list
        capi.check(entry(self.h, int(p), int(mode), nq, queries, k,
                         off.ctypes.data_as(i64p) if off is not None else None, ex.ctypes.data_as(i64p) if ex is not None else None,
                         idx.ctypes.data_as(i64p), capi.dptr(val)))
        return idx, val

    def rank_of(self, p, mode, subs, exclude=None):
        """Where held-out entries stand along mode `mode` of CP block p (`aoadmm_resident_rank_of`).  subs is nq x N,
        0-based; unlike `topk` its column `mode` is read: it holds the target row t_q.  Scores, order and exclusion
        lists are `topk`'s, with one difference: the target is a candidate whenever its score is not NaN, listed or not,
        so `sptensor.fiber_lists` of the whole tensor can be passed.  Returns (rank int64 nq, score float64 nq, ncand
        int64 nq): rank[q] is the number of candidates that come before t_q in `topk`'s order (its 0-based place; -1
        when its score is NaN), score[q] its score, ncand[q] the number of candidates.  `ranking_metrics` turns them
        into hit-rate, NDCG, MRR and AUC.  No nq x I_mode array exists."""
        subs = self._subs_f(subs, 'rank_of')
        i64p = C.POINTER(C.c_int64)
        return self._rank_call('rank_of', self.lib.aoadmm_resident_rank_of, p, mode, int(subs.shape[0]),
                               (subs.ctypes.data_as(i64p),), exclude, keep=subs)

    def rank_of_w(self, p, mode, W, targets, exclude=None):
        """`rank_of` with the weights given (`aoadmm_resident_rank_of_w`): W is nq x R, row q the weights of query q,
        used as they are, and targets[q] the row to place.  Ranks a row that `fold_in` returned (see `topk_w`)."""
        W = capi.as_f(W)
        if W.ndim != 2:
            raise ValueError('rank_of_w: W must be nq x R')
        R = self.block_rank(p)                                  # an unknown block is refused here, as the library refuses it
        if W.shape[1] != R:
            raise ValueError('rank_of_w: W has %d columns, block %d has R = %d' % (W.shape[1], int(p), R))
        targets = np.ascontiguousarray(np.asarray(targets, dtype=np.int64).reshape(-1))
        if targets.shape[0] != W.shape[0]:
            raise ValueError('rank_of_w: %d targets for %d rows of W' % (targets.shape[0], W.shape[0]))
        i64p = C.POINTER(C.c_int64)
        return self._rank_call('rank_of_w', self.lib.aoadmm_resident_rank_of_w, p, mode, int(W.shape[0]),
                               (capi.dptr(W), targets.ctypes.data_as(i64p)), exclude, keep=(W, targets))

    def _rank_call(self, what, entry, p, mode, nq, queries, exclude, keep=None):
        """The part `rank_of` and `rank_of_w` share: the outputs, the exclusion lists, the call.  `queries` holds the
        pointers the entry takes after nq; `keep` holds their arrays alive."""
        rank = np.full(nq, -1, dtype=np.int64)
        score = np.full(nq, np.nan)
        ncand = np.zeros(nq, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        off = ex = None
        if exclude is not None:
            off = np.ascontiguousarray(np.asarray(exclude[0], dtype=np.int64).reshape(-1))
            ex = np.ascontiguousarray(np.asarray(exclude[1], dtype=np.int64).reshape(-1))
            if off.shape[0] != nq + 1:
                raise ValueError('%s: exclude[0] must hold nq + 1 = %d offsets, got %d' % (what, nq + 1, off.shape[0]))
            if off[-1] != ex.shape[0]:
                raise ValueError('%s: exclude[0][-1] = %d but exclude[1] holds %d rows' % (what, off[-1], ex.shape[0]))
            if ex.shape[0] == 0:
                ex = np.zeros(1, dtype=np.int64)          # a valid address for an empty list
        capi.check(entry(self.h, int(p), int(mode), nq, *queries,
                         off.ctypes.data_as(i64p) if off is not None else None, ex.ctypes.data_as(i64p) if ex is not None else None,
                         rank.ctypes.data_as(i64p), capi.dptr(score), ncand.ctypes.data_as(i64p)))
        return rank, score, ncand

    @staticmethod
    def _exclude_arrays(what, nq, exclude):
        """(off, ex) int64 arrays of an `exclude = (off, idx)` argument, checked against nq; (None, None) without one."""
        if exclude is None:
            return None, None
        off = np.ascontiguousarray(np.asarray(exclude[0], dtype=np.int64).reshape(-1))
        ex = np.ascontiguousarray(np.asarray(exclude[1], dtype=np.int64).reshape(-1))
        if off.shape[0] != nq + 1:
            raise ValueError('%s: exclude[0] must hold nq + 1 = %d offsets, got %d' % (what, nq + 1, off.shape[0]))
        if off[-1] != ex.shape[0]:
            raise ValueError('%s: exclude[0][-1] = %d but exclude[1] holds %d rows' % (what, off[-1], ex.shape[0]))
        if ex.shape[0] == 0:
            ex = np.zeros(1, dtype=np.int64)          # a valid address for an empty list
        return off, ex

    def set_ranklist(self, p, mode, subs, exclude=None):
        """Attaches the ranking list of CP block p (`aoadmm_tensor_set_ranklist`): the arguments of `rank_of` (subs nq x N,
        0-based, column `mode` the target row; exclude = (off, idx) in any order, repeats allowed).  An empty subs
        removes the list; an error leaves the previous one.  The list is checked, sorted and uploaded once and belongs
        to the model: `build_model` drops it, a new upload of the block's data keeps it.  A solve then evaluates it at
        iteration 0 and every `every`-th iteration (`rank_track`) beside the objective and keeps the metric sums as a
        trace (`rank_trace`); nothing else the solve computes changes."""
        subs = np.asarray(subs, dtype=np.int64)
        if subs.size == 0:
            capi.check(self.lib.aoadmm_tensor_set_ranklist(self.h, int(p), int(mode), 0, None, None, None))
            return
        subs = self._subs_f(subs, 'set_ranklist')
        nq = int(subs.shape[0])
        off, ex = self._exclude_arrays('set_ranklist', nq, exclude)
        i64p = C.POINTER(C.c_int64)
        capi.check(self.lib.aoadmm_tensor_set_ranklist(self.h, int(p), int(mode), nq, subs.ctypes.data_as(i64p),
                                                       off.ctypes.data_as(i64p) if off is not None else None,
                                                       ex.ctypes.data_as(i64p) if ex is not None else None))

    def ranklist_info(self, p):
        """dict(nq, mode, listed, resident_bytes) of block p's ranking list (`aoadmm_ranklist_info`): listed counts the
        excluded rows kept after the per-query removal of repeats; nq = 0 and mode = -1 without a list."""
        nq, mode, listed, nb = C.c_int64(0), C.c_int(-1), C.c_int64(0), C.c_int64(0)
        capi.check(self.lib.aoadmm_ranklist_info(self.h, int(p), C.byref(nq), C.byref(mode), C.byref(listed), C.byref(nb)))
        return dict(nq=nq.value, mode=mode.value, listed=listed.value, resident_bytes=nb.value)

    def rank_track(self, metric='ndcg', k=10, every=1, patience=0, criterion=0):
        """What a solve does with the ranking lists (`aoadmm_rank_track`).  metric: 'hit', 'ndcg', 'mrr' or 'auc'; k: the
        cut-off of hit and ndcg; the lists are evaluated at iteration 0 and every `every`-th iteration.  At an
        evaluation S is the pooled mean of the metric over the blocks with a list (`rank_rule` states the best /
        patience rule).  criterion = 0: trace only.  criterion = 1: S selects the iterate `heldout_keep_best` keeps, and
        patience = n > 0 stops the solve after n consecutive evaluations without improvement
        (`exit_flag = 'rankPatience'`).  Belongs to the model: `build_model` restores the defaults."""
        try:
            mid = capi.RANK_METRICS[metric]
        except (KeyError, TypeError):
            raise ValueError("rank_track: metric must be one of 'hit', 'ndcg', 'mrr', 'auc', got %r" % (metric,)) from None
        k = int(k)
        if not 1 <= k < 2 ** 31:
            raise ValueError('rank_track: k = %d outside [1, 2^31)' % k)
        capi.check(self.lib.aoadmm_rank_track(self.h, mid, k, int(every), int(patience), int(criterion)))

    def rank_trace(self, p):
        """The ranking trace of block p's list over the last solve (`aoadmm_rank_trace`): a dict of arrays with one
        entry per evaluation: `iters`, the counts `n`, `n_auc`, the means `hit`, `ndcg`, `mrr` (over n) and `auc` (over
        n_auc; a mean over nothing is NaN), the raw sums `hits`, `ndcg_sum`, `mrr_sum`, `auc_sum`, and `best_iter`, the
        iteration of the best pooled score (-1 without a list)."""
        ln, best = C.c_int(0), C.c_int(-1)
        capi.check(self.lib.aoadmm_rank_trace(self.h, int(p), 0, None, 0, C.byref(ln), None, C.byref(best)))
        n = ln.value
        iters = np.zeros(max(n, 1), dtype=np.int32)
        sums = np.zeros((capi.RANKSUM_COUNT, max(n, 1)))
        for what in range(capi.RANKSUM_COUNT):
            capi.check(self.lib.aoadmm_rank_trace(self.h, int(p), what, capi.dptr(sums[what]), n, None,
                                                  iters.ctypes.data_as(C.POINTER(C.c_int)), None))
        return self._rank_trace_dict(iters[:n].astype(np.int64), sums[:, :n], best.value)

    @staticmethod
    def _rank_trace_dict(iters, sums, best_iter):
        cnt, cnt_auc = sums[capi.RANKSUM_N], sums[capi.RANKSUM_N_AUC]
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = lambda x, c: np.where(c > 0, x / c, np.nan)
            return dict(iters=iters, n=cnt.astype(np.int64), n_auc=cnt_auc.astype(np.int64),
                        hit=mean(sums[capi.RANKSUM_HITS], cnt), ndcg=mean(sums[capi.RANKSUM_NDCG], cnt),
                        mrr=mean(sums[capi.RANKSUM_MRR], cnt), auc=mean(sums[capi.RANKSUM_AUC], cnt_auc),
                        hits=sums[capi.RANKSUM_HITS].copy(), ndcg_sum=sums[capi.RANKSUM_NDCG].copy(),
                        mrr_sum=sums[capi.RANKSUM_MRR].copy(), auc_sum=sums[capi.RANKSUM_AUC].copy(), best_iter=int(best_iter))

    def ranklist_last(self, p):
        """(rank, score, ncand) of block p's ranking list as its last evaluation left them (`aoadmm_ranklist_last`): what
        `rank_of` returns for the factors that evaluation used."""
        nq = self.ranklist_info(p)['nq']
        rank = np.full(max(nq, 1), -1, dtype=np.int64)
        score = np.full(max(nq, 1), np.nan)
        ncand = np.zeros(max(nq, 1), dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        capi.check(self.lib.aoadmm_ranklist_last(self.h, int(p), rank.ctypes.data_as(i64p), capi.dptr(score), ncand.ctypes.data_as(i64p)))
        return rank[:nq], score[:nq], ncand[:nq]

    def op_rank_metrics(self, rank, ncand, k):
        """The device reduction from ranks to metric sums on host arrays (`aoadmm_op_rank_metrics`): eight doubles,
        `capi.RANKSUM_*` order (n, n_auc, hits, sum ndcg, sum mrr, sum auc, two spare zeros)."""
        rank = np.ascontiguousarray(np.asarray(rank, dtype=np.int64).reshape(-1))
        ncand = np.ascontiguousarray(np.asarray(ncand, dtype=np.int64).reshape(-1))
        if rank.shape[0] != ncand.shape[0]:
            raise ValueError('op_rank_metrics: %d ranks but %d candidate counts' % (rank.shape[0], ncand.shape[0]))
        out = np.zeros(8)
        i64p = C.POINTER(C.c_int64)
        capi.check(self.lib.aoadmm_op_rank_metrics(self.h, int(rank.shape[0]), rank.ctypes.data_as(i64p), ncand.ctypes.data_as(i64p),
                                                   int(k), capi.dptr(out)))
        return out

    def block_rank(self, p):
        """The number of components R of block p (`aoadmm_tensor_rank`), from the model the engine holds."""
        r = C.c_int(0)
        capi.check(self.lib.aoadmm_tensor_rank(self.h, int(p), C.byref(r)))
        return r.value

    def topk_w(self, p, mode, W, k, exclude=None):
        """`topk` with the weights given (`aoadmm_resident_topk_w`): W is nq x R, row q the weights of query q, used as
        they are.  Ranks a row that `fold_in` returned: for a 2-way block the folded rows are the weights along the
        other mode; for a higher order multiply them by the rows of the remaining modes.  Same order, exclusions and
        padding as `topk`."""
        W = capi.as_f(W)
        if W.ndim != 2:
            raise ValueError('topk_w: W must be nq x R')
        R = self.block_rank(p)                                  # an unknown block is refused here, as the library refuses it
        if W.shape[1] != R:
            raise ValueError('topk_w: W has %d columns, block %d has R = %d' % (W.shape[1], int(p), R))
        return self._topk_call('topk_w', self.lib.aoadmm_resident_topk_w, p, mode, int(W.shape[0]), capi.dptr(W), k, exclude, keep=W)

    def fold_in(self, p, mode, subs, vals, nq=None, ridge=0.0, nonneg=False, max_inner=5, tol=(0.0, 0.0), return_normal=False,
                weights=None, unstored_weight=0.0):
        """The factor rows of new indices along mode `mode` (0-based position in the block) of CP block p from their
        entries, every other factor held fixed (`aoadmm_resident_fold_in`).  subs is nobs x N, 0-based, with the query
        number in column `mode` (`sptensor.take_rows` gives such a list); vals has nobs values; nq=None: max(q) + 1.
        Row q solves (G_q + ridge I) u = b_q over the observations of q, or with nonneg=True runs the row ADMM loop for
        non-negativity (at most max_inner iterations, tol = (primal, dual)) and returns its feasible iterate.  Returns
        (rows nq x R, info int32 nq: 1 where the system was not positive definite and the row is NaN, iters int32 nq),
        and with return_normal=True also (gram nq x R x R, rhs nq x R), the normal equations before the ridge.
        weights (nobs values in [0, 1]) and unstored_weight = alpha in [0, 1] give the row of a model fitted under
        `set_entry_weights` (`aoadmm_resident_fold_in_w`): G_q = sum (w_e - alpha) z z' + alpha H with H the Hadamard
        product of the other factors' Gram matrices, b_q = sum w_e x_e z; every cell the list does not name counts as a
        zero of weight alpha, so with alpha > 0 each cell is listed once.  With both at their defaults the unweighted
        entry is called."""
        vals = np.ascontiguousarray(np.asarray(vals, dtype=np.float64).reshape(-1))
        subs = self._subs_f(subs, 'fold_in')
        nobs = int(vals.shape[0])
        if subs.shape[0] != nobs:
            raise ValueError('fold_in: subs must be nobs x N with nobs = len(vals)')
        mode = int(mode)
        if nq is None:
            if not 0 <= mode < subs.shape[1]:
                raise ValueError('fold_in: mode %d outside [0, %d)' % (mode, subs.shape[1]))
            nq = int(subs[:, mode].max()) + 1 if nobs else 0
        nq = int(nq)
        R = self.block_rank(p)                                  # an unknown block is refused here, as the library refuses it
        n = max(nq, 0)
        rows = np.zeros((n, R), order='F')
        info = np.zeros(n, dtype=np.int32)
        iters = np.zeros(n, dtype=np.int32)
        gram = np.zeros((n, R, R)) if return_normal else None     # block q: R x R, symmetric
        rhs = np.zeros((n, R), order='F') if return_normal else None
        opt = capi.FoldinOptions(float(ridge), 1 if nonneg else 0, int(max_inner), float(tol[0]), float(tol[1]))
        ip = C.POINTER(C.c_int)
        head = (self.h, int(p), mode, nq, nobs, subs.ctypes.data_as(C.POINTER(C.c_int64)) if nobs else None,
                capi.dptr(vals) if nobs else None)
        tail = (C.byref(opt), capi.dptr(rows), info.ctypes.data_as(ip), iters.ctypes.data_as(ip), capi.dptr(gram), capi.dptr(rhs))
        if weights is None and float(unstored_weight) == 0.0:
            capi.check(self.lib.aoadmm_resident_fold_in(*head, *tail))
        else:
            w = None
            if weights is not None:
                w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
                if w.shape[0] != nobs:
                    raise ValueError('fold_in: weights must hold nobs = %d values, got %d' % (nobs, w.shape[0]))
            capi.check(self.lib.aoadmm_resident_fold_in_w(*head, capi.dptr(w) if w is not None and nobs else None, float(unstored_weight), *tail))
        if return_normal:
            return rows, info, iters, gram, rhs
        return rows, info, iters

    def par2_rows(self, p):
        """I of PARAFAC2 block p: the rows of each of its slabs (`aoadmm_par2_rows`)."""
        rows = C.c_int64(0)
        capi.check(self.lib.aoadmm_par2_rows(self.h, int(p), C.byref(rows)))
        return rows.value

    def par2_fold_in(self, p, slabs, c0=None, max_iter=50, tol=1e-8, ridge=0.0, nonneg=False, max_inner=5, inner_tol=(0, 0),
                     return_B=True, return_P=False, return_y=False, return_sys=False):
        """The rows of C of new slabs of PARAFAC2 block p against its fitted A and DeltaB, B_q = P_q DeltaB imposed exactly
        (`aoadmm_resident_par2_fold_in`).  slabs is a list of 2-D arrays, each I x J_q with J_q >= R (a scipy.sparse slab
        is densified, one at a time); c0 (nk x R) starts the alternation (None: ones).  Per slab W = Y diag(c) DeltaB' with
        Y = X_q' A, P = its polar factor, b = diag(Y' P DeltaB), then c = (S + ridge I)^-1 b with S = (A'A) .* (DeltaB'DeltaB),
        or with nonneg=True the row ADMM loop of `fold_in` (at most max_inner iterations, inner_tol = (primal, dual)), at
        most max_iter times and until ||c - c_old|| <= tol ||c||.  Returns a dict: C (nk x R), B and P (lists of J_q x R,
        None unless asked for), res = ||X_q - A diag(c) B_q'||^2, xnorm = ||X_q||^2, fit = 1 - res / xnorm, iters, info (1:
        W lost a column, a zero slab for one), path = (Y class, alternation class), and with return_y / return_sys also
        Y (list) and sys = S."""
        mats = []
        for Xq in slabs:
            if hasattr(Xq, 'toarray'):
                Xq = Xq.toarray()
            Xq = np.asarray(Xq, dtype=np.float64)
            if Xq.ndim != 2:
                raise ValueError('par2_fold_in: every slab must be a 2-D array')
            mats.append(Xq)
        nk = len(mats)
        R = self.block_rank(p)                                  # an unknown block is refused here, as the library refuses it
        I = self.par2_rows(p)                                   # and so is a block that is not PARAFAC2
        for q, m in enumerate(mats):                            # the library reads I x J_q doubles per slab
            if m.shape[0] != I:
                raise ValueError('par2_fold_in: slab %d has %d rows, block %d has I = %d' % (q, m.shape[0], int(p), I))
        cols = np.array([m.shape[1] for m in mats], dtype=np.int64)
        Jtot = int(cols.sum())
        X = np.concatenate([m.ravel(order='F') for m in mats]) if nk else np.zeros(0)
        C0 = None
        if c0 is not None:
            C0 = capi.as_f(c0)
            if C0.shape != (nk, R):
                raise ValueError('par2_fold_in: c0 must be nk x R = %d x %d' % (nk, R))
        Cm = np.zeros((nk, R), order='F')
        res, xnorm = np.zeros(nk), np.zeros(nk)
        iters, info = np.zeros(nk, dtype=np.int32), np.zeros(nk, dtype=np.int32)
        flat = lambda want: np.zeros(Jtot * R) if want else None
        Bf, Pf, Yf = flat(return_B), flat(return_P), flat(return_y)
        sysm = np.zeros((R, R), order='F') if return_sys else None
        path = (C.c_int * 2)(-1, -1)
        opt = capi.Par2FoldinOptions(int(max_iter), float(tol), float(ridge), 1 if nonneg else 0, int(max_inner),
                                     float(inner_tol[0]), float(inner_tol[1]))
        ip = C.POINTER(C.c_int)
        capi.check(self.lib.aoadmm_resident_par2_fold_in(
            self.h, int(p), nk, cols.ctypes.data_as(C.POINTER(C.c_int64)) if nk else None, capi.dptr(X) if nk else None, capi.dptr(C0),
            C.byref(opt), capi.dptr(Cm), capi.dptr(Bf), capi.dptr(Pf), capi.dptr(res), capi.dptr(xnorm), iters.ctypes.data_as(ip),
            info.ctypes.data_as(ip), capi.dptr(Yf), capi.dptr(sysm), path))
        off = np.concatenate([[0], np.cumsum(cols)]) * R

        def cells(flatv):
            if flatv is None:
                return None
            return [flatv[off[q]:off[q + 1]].reshape((int(cols[q]), R), order='F') for q in range(nk)]
        with np.errstate(invalid='ignore', divide='ignore'):
            fit = 1.0 - res / xnorm
        out = dict(C=Cm, B=cells(Bf), P=cells(Pf), res=res, xnorm=xnorm, fit=fit, iters=iters, info=info, path=(path[0], path[1]))
        if return_y:
            out['Y'] = cells(Yf)
        if return_sys:
            out['sys'] = sysm
        return out

    def project(self, p, mats):
        """Tucker projection of the resident 3-way block p (`aoadmm_resident_project`): mats = (M0, M1, M2) with M_n of
        shape dims[n] x r_n; returns the core X x_1 M0' x_2 M1' x_3 M2' as an ndarray of shape (r0, r1, r2).  X is the
        block as it stands on the device: released, half, imputed (Xhat) or sparse with zeros for the unstored entries.
        A block the library cannot project raises `UnsupportedOnDevice`; see include/aoadmm_hip.h for the list."""
        if len(mats) != 3:
            raise ValueError('project: mats must hold three matrices, got %d' % len(mats))
        M = [capi.as_f(m) for m in mats]
        if any(m.ndim != 2 for m in M):
            raise ValueError('project: every matrix must be dims[n] x r_n')
        r = [int(m.shape[1]) for m in M]
        dp = C.POINTER(C.c_double)
        ptrs = (dp * 3)(*[capi.dptr(m) for m in M])
        ld = (C.c_int64 * 3)(*[max(1, int(m.shape[0])) for m in M])
        rr = (C.c_int * 3)(*r)
        core = np.zeros(tuple(max(x, 0) for x in r), order='F')
        capi.check(self.lib.aoadmm_resident_project(self.h, int(p), ptrs, ld, rr, capi.dptr(core)))
        return core

    def core_consistency(self, p, return_core=False, return_info=False):
        """Core consistency (CORCONDIA) of block p's CP model with the factors the engine holds
        (`aoadmm_resident_core_consistency`): 100 (1 - sum (core - superdiagonal ones)^2 / R) with core the projection
        of the block on M_n = F_n (F_n'F_n)^+.  Near 100: trilinear at this R; it has no lower bound.  Returns cc, then
        the R x R x R core with return_core=True, then {'rank_deficient': bool} with return_info=True (a factor whose
        Gram matrix has an eigenvalue below R 2^-52 of its largest)."""
        R = self.block_rank(p)
        cc, flag = C.c_double(0), C.c_int(0)
        core = np.zeros((R, R, R), order='F') if return_core else None
        capi.check(self.lib.aoadmm_resident_core_consistency(self.h, int(p), C.byref(cc), capi.dptr(core), C.byref(flag)))
        out = (cc.value,)
        if return_core:
            out += (core,)
        if return_info:
            out += ({'rank_deficient': bool(flag.value)},)
        return out[0] if len(out) == 1 else out

    def resident_mttkrp(self, p, tensor_mode, rows, R):
        """One MTTKRP of the resident block p against the current factors (`aoadmm_resident_mttkrp`): rows x R."""
        out = np.zeros((rows, R), order='F')
        ms = C.c_float(0)
        capi.check(self.lib.aoadmm_resident_mttkrp(self.h, int(p), int(tensor_mode), capi.dptr(out), C.byref(ms)))
        return out

    def tensor_storage_info(self, p):
        """(precision id capi.PREC_*, scale, resident bytes) of tensor p (`aoadmm_tensor_storage_info`): the precision
        its passes stream, the power-of-two scale of an 'f16' block (1.0 otherwise) and the bytes a CP block holds on
        the device now (a sparse block: N (4 N + 8) per nonzero held).  On a rank of a communicator: the scale common to
        all ranks (that of the whole tensor) and this rank's own bytes."""
        prec, scale, nbytes = C.c_int(0), C.c_double(0), C.c_int64(0)
        capi.check(self.lib.aoadmm_tensor_storage_info(self.h, int(p), C.byref(prec), C.byref(scale), C.byref(nbytes)))
        return prec.value, scale.value, nbytes.value

    def kernel_stats(self, which, reset=False):
        """(ms, launches, bytes, flops) of a kernel class since the last reset (`aoadmm_kernel_stats`); which = 3:
        MTTKRPs of sparse blocks (of a sharded block: this rank's share), passes over the nonzeros of PARAFAC2
        blocks with sparse slabs and EM steps of observed-only blocks; which = 4 + n: the pass of those EM steps over
        the copy of tensor mode n, and for which = 4 the pass of every `resident_em_pass` call over a dense CP block; which = 12: the held-out passes; which = 13: the top-k completions and the ranks of targets (one launch per `topk` or `rank_of` call and per
        evaluation of a ranking list inside a solve);
        which = 14: the fold-in of new rows (one launch per `fold_in` call, weighted or not); which = 16: the list pass
        of every `resident_em_list_pass` call; which = 17: the fold-in of new PARAFAC2 slabs (one launch per `par2_fold_in`
        call)."""
        ms, n, by, fl = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        capi.check(self.lib.aoadmm_kernel_stats(self.h, int(which), int(bool(reset)), C.byref(ms), C.byref(n),
                                                C.byref(by), C.byref(fl)))
        return ms.value, n.value, by.value, fl.value

    # ---- op level -----------------------------------------------------------------
    def mttkrp(self, X, U, n, precision='f64'):
        """`mttkrp(X,U,n)` with 0-based n (cmtf_fun_AOADMM.m:97).  'f16' exists for resident blocks only: the library
        answers it with `UnsupportedOnDevice` here."""
        X = capi.as_f(X)
        dims = (C.c_int64 * X.ndim)(*X.shape)
        Us = [capi.as_f(u) for u in U]
        R = Us[0].shape[1]
        arr = (C.POINTER(C.c_double) * X.ndim)(*[capi.dptr(u) for u in Us])
        out = np.zeros((X.shape[n], R), order='F')
        prec = capi.precision_id(precision)
        capi.check(self.lib.aoadmm_op_mttkrp(self.h, capi.dptr(X), X.ndim, dims, arr, R, int(n), prec, capi.dptr(out)))
        return out

    def unfold_gram(self, X, n, precision='f64'):
        """`Y = A*A'` with A the mode-n unfolding of X (0-based n), cmtf_nvecs.m:40-56."""
        X = capi.as_f(X)
        dims = (C.c_int64 * X.ndim)(*X.shape)
        out = np.zeros((X.shape[n], X.shape[n]), order='F')
        prec = capi.precision_id(precision)
        capi.check(self.lib.aoadmm_op_unfold_gram(self.h, capi.dptr(X), X.ndim, dims, int(n), prec, capi.dptr(out)))
        return out

    def resident_unfold_gram(self, p, tensor_mode, n, slab=0):
        """The same Gram matrix (n x n) from the data of tensor p already on the device (`aoadmm_resident_unfold_gram`)."""
        out = np.zeros((n, n), order='F')
        capi.check(self.lib.aoadmm_resident_unfold_gram(self.h, int(p), int(tensor_mode), int(slab), capi.dptr(out)))
        return out

    def resident_nvecs(self, p, tensor_mode, n, r, oversample=0, max_iters=0, tol=0.0, seed=0):
        """The r leading eigenvectors of X_(n) X_(n)' from the SPARSE data of tensor p already on the device
        (`aoadmm_resident_nvecs`): block subspace iteration on the nonzeros, no n x n Gram matrix.  n = I_n; zeros =
        the library's defaults (oversample 8, max_iters 500, tol 1e-10).  Returns (U n x r, eigvals r, info) with
        info = dict(iterations, converged, block, residual, fibers); not converged is reported, not raised."""
        U = np.zeros((int(n), int(r)), order='F')
        ev = np.zeros(int(r))
        opt = capi.NvecsOptions(int(oversample), int(max_iters), float(tol), int(seed))
        info = capi.NvecsInfo()
        capi.check(self.lib.aoadmm_resident_nvecs(self.h, int(p), int(tensor_mode), int(r), C.byref(opt), capi.dptr(U),
                                                  max(int(n), 1), capi.dptr(ev), C.byref(info)))
        return U, ev, dict(iterations=info.iterations, converged=info.converged, block=info.block,
                           residual=info.residual, fibers=info.fibers)

    def gram(self, F):
        F = capi.as_f(F)
        out = np.zeros((F.shape[1], F.shape[1]), order='F')
        capi.check(self.lib.aoadmm_op_gram(self.h, capi.dptr(F), F.shape[0], F.shape[1], capi.dptr(out)))
        return out

    def chol(self, B):
        B = capi.as_f(B)
        out = np.zeros_like(B, order='F')
        capi.check(self.lib.aoadmm_op_chol(self.h, capi.dptr(B), B.shape[0], capi.dptr(out)))
        return out

    def prox(self, constraint, X, rho):
        """Evaluate the prox handle `constraints_to_prox` builds for `constraint` at (X, rho)."""
        cid, params, Lmat = constraint_descriptor(constraint)
        X = capi.as_f(X)
        out = np.zeros_like(X, order='F')
        capi.check(self.lib.aoadmm_op_prox(self.h, cid, capi.dptr(params) if params.size else None, params.size,
                                           capi.dptr(Lmat) if Lmat is not None else None, capi.dptr(X),
                                           X.shape[0], X.shape[1], float(rho), capi.dptr(out)))
        return out

    def admm_constrained(self, A, Bsys, rho, constraint, fac, Z, mu, max_inner, tol_pr, tol_du):
        """ADMM_constrained_only (cmtf_fun_AOADMM.m:591-623); returns (fac, Z, mu, inner_iters)."""
        cid, params, Lmat = constraint_descriptor(constraint)
        A = capi.as_f(A)
        Bsys = capi.as_f(Bsys)
        fac = capi.as_f(fac).copy(order='F')
        Z = capi.as_f(Z).copy(order='F')
        mu = capi.as_f(mu).copy(order='F')
        it = C.c_int(0)
        capi.check(self.lib.aoadmm_op_admm_constrained(
            self.h, capi.dptr(A), capi.dptr(Bsys), float(rho), cid, capi.dptr(params) if params.size else None,
            params.size, capi.dptr(Lmat) if Lmat is not None else None, A.shape[0], A.shape[1], int(max_inner),
            float(tol_pr), float(tol_du), capi.dptr(fac), capi.dptr(Z), capi.dptr(mu), C.byref(it)))
        return fac, Z, mu, it.value

    def admm_mode(self, A, Cmat, constraint, fac, Z, mu, max_inner, tol_pr, tol_du):
        """The ADMM update of one constrained CP mode as the solver runs it (`aoadmm_op_admm_mode`): system and
        kernels chosen by the library from `Cmat` (Hadamard product of the other modes' Gram matrices) and the shape.
        Returns a dict: fac, Z, mu, inner_iters, pr, du (residuals of the last iteration), gram (fac'*fac), facT (the
        row-major copy of fac as a rows x R C-ordered array) and path (one of capi.PATH_*)."""
        cid, params, Lmat = constraint_descriptor(constraint)
        A = capi.as_f(A)
        Cmat = capi.as_f(Cmat)
        rows, R = A.shape
        fac = capi.as_f(fac).copy(order='F')
        Z = capi.as_f(Z).copy(order='F')
        mu = capi.as_f(mu).copy(order='F')
        it, path = C.c_int(0), C.c_int(-1)
        res = np.zeros(2)
        gram = np.zeros((R, R), order='F')
        facT = np.zeros((rows, R), order='C')
        capi.check(self.lib.aoadmm_op_admm_mode(
            self.h, capi.dptr(A), capi.dptr(Cmat), cid, capi.dptr(params) if params.size else None, params.size,
            capi.dptr(Lmat) if Lmat is not None else None, rows, R, int(max_inner), float(tol_pr), float(tol_du),
            capi.dptr(fac), capi.dptr(Z), capi.dptr(mu), C.byref(it), capi.dptr(res), capi.dptr(gram), capi.dptr(facT),
            C.byref(path)))
        return dict(fac=fac, Z=Z, mu=mu, inner_iters=it.value, pr=float(res[0]), du=float(res[1]), gram=gram,
                    facT=facT, path=path.value)

    def par2_b_loop(self, rows_k, R, Ak, GA, Cmat, weight, rho_scale, constraint, max_inner, tol, P, mu_DeltaB, DeltaB,
                    Z=None, muZ=None):
        """Mode B of a PARAFAC2 block from the right-hand side on, as the solver runs it (`aoadmm_op_par2_b_loop`):
        slab systems, ADMM_B_Parafac2 with the kernels the library picks for (R, max J_k, constrained), Gram matrices.
        Ak, P, mu_DeltaB, Z, muZ: lists of K arrays J_k x R; GA R x R; Cmat K x R; constraint: a `Z.constraints` cell
        or None; tol: (pr_coupl, pr_constr, du_coupl, du_constr).  Returns a dict: B, P, mu, Z, muZ (lists; Z, muZ
        None when unconstrained), DeltaB, rho (K), L and GB (K x R x R, [k] = the slab's matrix), inner_iters,
        res (4, order of tol) and path = (folded, slab class capi.P2SLAB_*, in_lds, dual_fold class)."""
        rows = [int(j) for j in rows_k]
        K, R = len(rows), int(R)
        if constraint is None:
            cid, params = 0, np.zeros(0)
        else:
            cid, params, Lmat = constraint_descriptor(constraint)
            if Lmat is not None:
                raise ValueError('par2_b_loop: quadratic regularization is not available here')

        def pack(xs):
            xs = [np.asarray(x, dtype=np.float64).reshape(j, R) for x, j in zip(xs, rows)]
            if len(xs) != K:
                raise ValueError('par2_b_loop: one array per slab')
            return np.concatenate([x.ravel(order='F') for x in xs])

        def unpack(v):
            off = np.concatenate([[0], np.cumsum(rows)]) * R
            return [v[off[k]:off[k + 1]].reshape(rows[k], R, order='F').copy() for k in range(K)]

        ak, p, mu = pack(Ak), pack(P), pack(mu_DeltaB)
        z = pack(Z) if cid else None
        mz = pack(muZ) if cid else None
        ga, cm = capi.as_f(GA), capi.as_f(Cmat)
        if ga.shape != (R, R) or cm.shape != (K, R):
            raise ValueError('par2_b_loop: GA must be R x R and C K x R')
        db = capi.as_f(DeltaB).copy(order='F')
        n = ak.size
        b = np.zeros(n)
        rho, L, GB = np.zeros(K), np.zeros(K * R * R), np.zeros(K * R * R)
        it = C.c_int(0)
        res = np.zeros(4)
        path = (C.c_int * 4)(-1, -1, -1, -1)
        tolv = np.asarray(tol, dtype=np.float64).reshape(4).copy()
        rk = (C.c_int64 * K)(*rows)
        capi.check(self.lib.aoadmm_op_par2_b_loop(
            self.h, K, rk, R, capi.dptr(ak), capi.dptr(ga), capi.dptr(cm), float(weight), float(rho_scale), cid,
            capi.dptr(params) if params.size else None, params.size, int(max_inner), capi.dptr(tolv), capi.dptr(p),
            capi.dptr(mu), capi.dptr(db), capi.dptr(z), capi.dptr(mz), capi.dptr(b), capi.dptr(rho), capi.dptr(L),
            capi.dptr(GB), C.byref(it), capi.dptr(res), path))
        mats = lambda v: np.stack([v[k * R * R:(k + 1) * R * R].reshape(R, R, order='F') for k in range(K)])
        return dict(B=unpack(b), P=unpack(p), mu=unpack(mu), Z=unpack(z) if cid else None,
                    muZ=unpack(mz) if cid else None, DeltaB=db, rho=rho, L=mats(L), GB=mats(GB), inner_iters=it.value,
                    res=res, path=tuple(path))

    @staticmethod
    def _par2_pack(who, xs, rows, n, slabs=False):
        """Slab layout of csrc/par2.h: X_k (n x J_k) or slab-valued factors (J_k x n), column-major, back to back."""
        if len(xs) != len(rows):
            raise ValueError('%s: one array per slab' % who)
        shape = (lambda j: (n, j)) if slabs else (lambda j: (j, n))
        return np.concatenate([np.asarray(x, dtype=np.float64).reshape(shape(j)).ravel(order='F')
                               for x, j in zip(xs, rows)])

    def par2_mode_a(self, X, B, Cmat):
        """Mode A of a dense PARAFAC2 block as the solver runs it (`aoadmm_op_par2_mode_a`, cmtf_fun_AOADMM.m:160-165).
        X: list of K slabs I x J_k; B: list of K arrays J_k x R; Cmat K x R.  Returns a dict: T1 (K x I x R, X_k B_k),
        GB (K x R x R), Amt (I x R, unweighted), Csys (R x R), Csys_only (the launch of blocks with sparse slabs) and
        path = (tile width of the Amt + Csys launch, of the Csys-only launch)."""
        cm = capi.as_f(Cmat)
        K, R = cm.shape
        I = int(np.asarray(X[0]).shape[0])
        rows = [int(np.asarray(x).shape[1]) for x in X]
        x, b = self._par2_pack('par2_mode_a', X, rows, I, True), self._par2_pack('par2_mode_a', B, rows, R)
        if len(rows) != K:
            raise ValueError('par2_mode_a: C has one row per slab')
        T1, GB = np.zeros(K * I * R), np.zeros(K * R * R)
        Amt, Csys, Cso = np.zeros((I, R), order='F'), np.zeros((R, R), order='F'), np.zeros((R, R), order='F')
        path = (C.c_int * 2)(-1, -1)
        capi.check(self.lib.aoadmm_op_par2_mode_a(
            self.h, K, (C.c_int64 * K)(*rows), I, R, capi.dptr(x), capi.dptr(b), capi.dptr(cm), capi.dptr(T1),
            capi.dptr(GB), capi.dptr(Amt), capi.dptr(Csys), capi.dptr(Cso), path))
        return dict(T1=T1.reshape(K, R, I).transpose(0, 2, 1).copy(), GB=GB.reshape(K, R, R).transpose(0, 2, 1).copy(),
                    Amt=Amt, Csys=Csys, Csys_only=Cso, path=tuple(path))

    def par2_mode_c(self, X, A, B, Cmat, weight=1.0, ridge=0.0, bsum_half=0.0, constraint=None, Z=None, mu=None,
                    max_inner=5, tol=(0.0, 0.0), system=0, sysmat=None):
        """Mode C of a dense PARAFAC2 block as the solver runs it (`aoadmm_op_par2_mode_c`, cmtf_fun_AOADMM.m:219-248 and
        the coupled systems :260-312).  X, B: lists of K slabs I x J_k / J_k x R; A I x R; Cmat, Z, mu K x R;
        constraint: a `Z.constraints` cell or None; tol: (pr_constr, du_constr); system: capi.P2CSYS_* (0: the
        uncoupled update; 1..4: only the builders of a coupled C mode, sysmat = H*H' (R x R) for 2, the diagonal of H'*H
        (K) for 3, H'*H (K x K) for 4).  Returns a dict: a (K x R), rho (K), L (K x R x R), rho_max / rho_mean /
        rho_sum (NaN where the entry does not set them), M ((K R)^2, system 4), C, Z, mu, inner_iters, res (2) and
        path = (capi.P2C_* or -1, rank class of the row solve)."""
        A = capi.as_f(A)
        I, R = A.shape
        rows = [int(np.asarray(x).shape[1]) for x in X]
        K = len(rows)
        if constraint is None:
            cid, params = 0, np.zeros(0)
        else:
            cid, params, Lmat = constraint_descriptor(constraint)
            if Lmat is not None:
                raise ValueError('par2_mode_c: quadratic regularization is not available here')
        x, b = self._par2_pack('par2_mode_c', X, rows, I, True), self._par2_pack('par2_mode_c', B, rows, R)
        cm = capi.as_f(Cmat).copy(order='F')
        if cm.shape != (K, R):
            raise ValueError('par2_mode_c: C must be K x R')
        z = capi.as_f(Z).copy(order='F') if Z is not None else None
        m = capi.as_f(mu).copy(order='F') if mu is not None else None
        sm = capi.as_f(sysmat) if sysmat is not None else None
        a, rho, L = np.zeros((K, R), order='F'), np.zeros(K), np.zeros(K * R * R)
        stats = np.full(3, np.nan)
        M = np.zeros((K * R, K * R), order='F') if system == capi.P2CSYS_DENSE else None
        it = C.c_int(-1)
        res = np.zeros(2)
        path = (C.c_int * 2)(-1, -1)
        tolv = np.asarray(tol, dtype=np.float64).reshape(2).copy()
        capi.check(self.lib.aoadmm_op_par2_mode_c(
            self.h, int(system), K, (C.c_int64 * K)(*rows), I, R, capi.dptr(x), capi.dptr(A), capi.dptr(b),
            float(weight), float(ridge), float(bsum_half), cid, capi.dptr(params) if params.size else None, params.size,
            int(max_inner), capi.dptr(tolv), capi.dptr(sm), capi.dptr(cm), capi.dptr(z), capi.dptr(m), capi.dptr(a),
            capi.dptr(rho), capi.dptr(L), capi.dptr(stats), capi.dptr(M), C.byref(it), capi.dptr(res), path))
        return dict(a=a, rho=rho, L=L.reshape(K, R, R).transpose(0, 2, 1).copy(), rho_max=float(stats[0]),
                    rho_mean=float(stats[1]), rho_sum=float(stats[2]), M=M, C=cm, Z=z, mu=m, inner_iters=it.value,
                    res=res, path=tuple(path))

    def par2_objective(self, X, A, B, Cmat, P, DeltaB, Z=None, reg=None):
        """Objective pieces of a dense PARAFAC2 block as the solver runs them (`aoadmm_op_par2_objective`,
        cmtf_fun_AOADMM.m:1262-1264, :1355, :1337, :1279-1281).  X, B, P, Z: lists of K slabs; reg: a `Z.constraints`
        cell of a regularisation type (its first parameter is eta) or None.  Returns a dict: res (K), q (K x 4),
        regv (K, None without reg)."""
        A = capi.as_f(A)
        I, R = A.shape
        rows = [int(np.asarray(x).shape[1]) for x in X]
        K = len(rows)
        who = 'par2_objective'
        x, b, p = self._par2_pack(who, X, rows, I, True), self._par2_pack(who, B, rows, R), self._par2_pack(who, P, rows, R)
        z = self._par2_pack(who, Z, rows, R) if Z is not None else None
        cm, db = capi.as_f(Cmat), capi.as_f(DeltaB)
        if cm.shape != (K, R) or db.shape != (R, R):
            raise ValueError('par2_objective: C must be K x R and DeltaB R x R')
        rid, eta = 0, 0.0
        if reg is not None:
            rid, params, _ = constraint_descriptor(reg)
            eta = float(params[0]) if params.size else 0.0
        res, q = np.zeros(K), np.zeros((K, 4))
        regv = np.zeros(K) if rid else None
        capi.check(self.lib.aoadmm_op_par2_objective(
            self.h, K, (C.c_int64 * K)(*rows), I, R, capi.dptr(x), capi.dptr(A), capi.dptr(b), capi.dptr(cm), capi.dptr(p),
            capi.dptr(db), capi.dptr(z), rid, eta, capi.dptr(res), capi.dptr(q), capi.dptr(regv)))
        return dict(res=res, q=q, regv=regv)

    def coupled_loop(self, coupling, A, Cmat, max_inner, tol):
        """The inner loop of coupling `coupling` (0-based) of the model this engine holds, as the solver runs it behind
        the MTTKRPs (`aoadmm_op_coupled_loop`): systems, the form of the loop the library picks, Gram matrices.  A, Cmat:
        one array per coupled mode in ascending mode order (rows_j x R_j: the MTTKRP; R_j x R_j: the Hadamard product
        of the other modes' Gram matrices, weight applied); tol: (pr_coupl, pr_constr, du_coupl, du_constr).  The state
        goes in and out through `aoadmm_state_set` / `aoadmm_state_get`.  Returns a dict: inner_iters, res (4, order of
        tol), rho (n), L and gram (lists of R_j x R_j), slots (n x 8 squared norms behind the residuals) and path =
        (capi.CPATH_*, rank class of the row kernels or 0)."""
        A = [capi.as_f(a) for a in A]
        Cmat = [capi.as_f(c) for c in Cmat]
        n = len(A)
        if n == 0 or len(Cmat) != n or any(a.ndim != 2 or c.shape != (a.shape[1],) * 2 for a, c in zip(A, Cmat)):
            raise ValueError('coupled_loop: one rows x R array and one R x R array per coupled mode')
        L = [np.zeros(c.shape, order='F') for c in Cmat]
        gram = [np.zeros(c.shape, order='F') for c in Cmat]
        rho, slots, res = np.zeros(n), np.zeros((n, 8)), np.zeros(4)
        it = C.c_int(0)
        path = (C.c_int * 2)(-1, -1)
        tolv = np.asarray(tol, dtype=np.float64).reshape(4).copy()
        ptrs = lambda xs: (C.POINTER(C.c_double) * n)(*[capi.dptr(x) for x in xs])
        capi.check(self.lib.aoadmm_op_coupled_loop(
            self.h, int(coupling), ptrs(A), ptrs(Cmat), int(max_inner), capi.dptr(tolv), C.byref(it), capi.dptr(res),
            capi.dptr(rho), ptrs(L), ptrs(gram), capi.dptr(slots), path))
        return dict(inner_iters=it.value, res=res, rho=rho, L=L, gram=gram, slots=slots, path=tuple(path))


_default = None


def default_engine():
    """Process-wide engine on the GPU LOCAL_RANK points at (device 0 otherwise)."""
    global _default
    if _default is None:
        import os
        _default = Engine(int(os.environ.get('LOCAL_RANK', '0')))
    return _default
