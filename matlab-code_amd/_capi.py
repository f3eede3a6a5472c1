"""ctypes binding of libaoadmm_hip.so (C ABI: include/aoadmm_hip.h).

This is the same marshalling a MEX gateway does; there is
no CPU fallback: if the library is missing or no GPU is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('AOADMM_LIB_PATH') or os.path.join(_HERE, 'libaoadmm_hip.so')   # the override is for A/B timing of builds

# status codes (include/aoadmm_hip.h)
OK, ERR_INVALID, ERR_HIP, ERR_NOT_PD, ERR_RCCL, ERR_UNSUPPORTED, ERR_NOMEM = range(7)
PREC_F64, PREC_F32, PREC_F16 = 0, 1, 2
PRECISIONS = {'f64': PREC_F64, 'f32': PREC_F32, 'f16': PREC_F16}


def precision_id(precision):
    """'f64' | 'f32' | 'f16' -> AOADMM_PREC_*; anything else is a ValueError."""
    try:
        return PRECISIONS[precision]
    except (KeyError, TypeError):
        raise ValueError("precision must be one of 'f64', 'f32', 'f16', got %r" % (precision,)) from None


def quantize_f16(X):
    """The AOADMM_PREC_F16 storage rule of include/aoadmm_hip.h on the host: (q, s) with q the float16 array the device
    stores and s its power-of-two scale; the block's data is q / s.  A non-finite entry is a ValueError."""
    x = np.asarray(X, dtype=np.float64).astype(np.float32)
    if not np.all(np.isfinite(x)):
        raise ValueError('quantize_f16: the tensor holds an entry that is not finite')
    a = float(np.abs(x).max()) if x.size else 0.0
    s = 1.0
    if a > 0.0:
        _, E = np.frexp(a)
        s = float(np.ldexp(1.0, min(127, max(-126, 15 - int(E)))))
    return (x * np.float32(s)).astype(np.float16), s


def coo_share(nnz, rank, world):
    """(first, end) of rank `rank`'s share of `nnz` coalesced nonzeros under `aoadmm_tensor_upload_coo_sharded`: the
    entries [floor(rank nnz / world), floor((rank + 1) nnz / world)) of every mode's sorted copy."""
    nnz, rank, world = int(nnz), int(rank), int(world)
    if nnz < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError('coo_share: need nnz >= 0 and 0 <= rank < world, got %d, %d, %d' % (nnz, rank, world))
    return rank * nnz // world, (rank + 1) * nnz // world


(F_FAC, F_CONSTRAINT_FAC, F_CONSTRAINT_DUAL, F_COUPLING_FAC, F_COUPLING_DUAL, F_DELTAB, F_P,
 F_MU_DELTAB) = range(8)
ALL_SLABS = -1            # AOADMM_ALL_SLABS
(PATH_WG, PATH_MFMA, PATH_ROWS_FUSED, PATH_ROWS_COLPROX, PATH_ROWS_TV, PATH_ROWL) = range(6)   # AOADMM_PATH_*
(CPATH_REGS, CPATH_WG, CPATH_ROWSTEPS, CPATH_GENERIC) = range(4)   # AOADMM_CPATH_*
(P2SLAB_REGS1, P2SLAB_REGS2, P2SLAB_REGS4, P2SLAB_LDS4, P2SLAB_LDS8, P2SLAB_LDS16, P2SLAB_LDS64) = range(7)   # AOADMM_P2SLAB_*
(P2CSYS_UNCOUPLED, P2CSYS_ROWS, P2CSYS_HHT, P2CSYS_DIAG, P2CSYS_DENSE) = range(5)   # AOADMM_P2CSYS_*
(P2C_SINGLE, P2C_WG, P2C_LAUNCHED) = range(3)   # AOADMM_P2C_*
(P2FOLD_ALT_LDS, P2FOLD_ALT_WS) = range(2)      # AOADMM_P2FOLD_ALT_*; AOADMM_P2FOLD_Y_* is 2 (T - 1) + chunked
(RANK_HIT, RANK_NDCG, RANK_MRR, RANK_AUC) = range(4)   # AOADMM_RANK_*
RANK_METRICS = {'hit': RANK_HIT, 'ndcg': RANK_NDCG, 'mrr': RANK_MRR, 'auc': RANK_AUC}
(RANKSUM_N, RANKSUM_N_AUC, RANKSUM_HITS, RANKSUM_NDCG, RANKSUM_MRR, RANKSUM_AUC, RANKSUM_COUNT) = range(7)   # AOADMM_RANKSUM_*
PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_double)   # aoadmm_progress_fn

# every symbol include/aoadmm_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    'aoadmm_abi_version', 'aoadmm_last_error', 'aoadmm_device_count', 'aoadmm_create', 'aoadmm_create_multi', 'aoadmm_destroy',
    'aoadmm_synchronize', 'aoadmm_set_progress', 'aoadmm_comm_unique_id', 'aoadmm_comm_init_rank', 'aoadmm_comm_init_rank_share', 'aoadmm_comm_init_local', 'aoadmm_comm_rank', 'aoadmm_comm_info',
    'aoadmm_model_begin', 'aoadmm_model_set_mode', 'aoadmm_model_set_mode_slabs', 'aoadmm_model_add_cp',
    'aoadmm_model_add_par2', 'aoadmm_model_set_constraint', 'aoadmm_model_set_coupling',
    'aoadmm_model_set_coupling_type', 'aoadmm_model_set_ridge', 'aoadmm_model_end', 'aoadmm_tensor_upload',
    'aoadmm_tensor_upload_rows', 'aoadmm_tensor_upload_coo', 'aoadmm_tensor_upload_coo_sharded', 'aoadmm_par2_slab_upload', 'aoadmm_par2_slab_upload_coo', 'aoadmm_tensor_mask_upload', 'aoadmm_tensor_weights_upload', 'aoadmm_par2_slab_mask_upload', 'aoadmm_tensor_synth', 'aoadmm_tensor_normsq', 'aoadmm_tensor_storage_info', 'aoadmm_tensor_rank',
    'aoadmm_tensor_set_observed_only', 'aoadmm_tensor_set_entry_weights', 'aoadmm_resident_em_step', 'aoadmm_resident_em_pass',
    'aoadmm_tensor_set_missing_list', 'aoadmm_tensor_missing_list', 'aoadmm_resident_em_list_pass',
    'aoadmm_resident_model_at', 'aoadmm_tensor_set_heldout', 'aoadmm_resident_heldout_stats', 'aoadmm_heldout_info', 'aoadmm_heldout_trace',
    'aoadmm_heldout_keep_best', 'aoadmm_heldout_restore_best', 'aoadmm_heldout_best_info', 'aoadmm_resident_topk',
    'aoadmm_resident_topk_w', 'aoadmm_resident_rank_of', 'aoadmm_resident_rank_of_w', 'aoadmm_resident_project', 'aoadmm_resident_core_consistency', 'aoadmm_resident_fold_in', 'aoadmm_resident_fold_in_w',
    'aoadmm_resident_par2_fold_in', 'aoadmm_par2_rows',
    'aoadmm_tensor_set_ranklist', 'aoadmm_ranklist_info', 'aoadmm_rank_track', 'aoadmm_rank_trace', 'aoadmm_ranklist_last',
    'aoadmm_state_set', 'aoadmm_state_get', 'aoadmm_solve', 'aoadmm_resident_mttkrp', 'aoadmm_resident_par2_rhs', 'aoadmm_kernel_stats',
    'aoadmm_op_mttkrp', 'aoadmm_op_unfold_gram', 'aoadmm_resident_unfold_gram', 'aoadmm_resident_nvecs', 'aoadmm_op_gram', 'aoadmm_op_chol', 'aoadmm_op_prox', 'aoadmm_op_admm_constrained',
    'aoadmm_op_admm_mode', 'aoadmm_op_par2_b_loop', 'aoadmm_op_coupled_loop',
    'aoadmm_op_par2_mode_a', 'aoadmm_op_par2_mode_c', 'aoadmm_op_par2_objective', 'aoadmm_op_rank_metrics',
]


class AoadmmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('[aoadmm status %d] %s' % (code, msg))
        self.code = code


class NotPositiveDefinite(AoadmmError):
    """chol() failure -- MATLAB raises 'Matrix must be positive definite' (cmtf_fun_AOADMM.m:142)."""


class UnsupportedOnDevice(AoadmmError):
    """Model feature that the host layer must route to the original MATLAB path."""


class Options(C.Structure):
    _fields_ = [
        ('MaxOuterIters', C.c_int32), ('MaxInnerIters', C.c_int32),
        ('AbsFuncTol', C.c_double), ('OuterRelTol', C.c_double),
        ('innerRelPrTol_coupl', C.c_double), ('innerRelPrTol_constr', C.c_double),
        ('innerRelDualTol_coupl', C.c_double), ('innerRelDualTol_constr', C.c_double),
        ('bsum', C.c_int32), ('bsum_weight', C.c_double),
        ('iter_start_PAR2Bkconstraint', C.c_int32), ('has_increase_factor_rhoBk', C.c_int32),
        ('increase_factor_rhoBk', C.c_double), ('use_dimtree', C.c_int32), ('no_permuted_copy', C.c_int32),
        ('par2_slab_sharding', C.c_int32), ('heldout_patience', C.c_int32), ('reserved', C.c_int32 * 4),
    ]


class Result(C.Structure):
    _fields_ = [
        ('f_tensors', C.c_double), ('f_couplings', C.c_double), ('f_constraints', C.c_double),
        ('f_PAR2_couplings', C.c_double), ('OuterIterations', C.c_int32), ('exit_code', C.c_int32),
        ('exit_abs', C.c_int32 * 4),
        ('func_val_conv', C.POINTER(C.c_double)), ('func_coupl_conv', C.POINTER(C.c_double)),
        ('func_constr_conv', C.POINTER(C.c_double)), ('func_PAR2_coupl', C.POINTER(C.c_double)),
        ('time_at_it', C.POINTER(C.c_double)), ('innerIters', C.POINTER(C.c_double)),
        ('f_rel_missing', C.c_double), ('func_rel_missing', C.POINTER(C.c_double)),
    ]


class NvecsOptions(C.Structure):                  # aoadmm_nvecs_options (zeros = defaults)
    _fields_ = [('oversample', C.c_int), ('max_iters', C.c_int), ('tol', C.c_double), ('seed', C.c_uint64)]


class FoldinOptions(C.Structure):                 # aoadmm_foldin_options
    _fields_ = [('ridge', C.c_double), ('constraint', C.c_int), ('max_inner', C.c_int), ('tol_primal', C.c_double),
                ('tol_dual', C.c_double)]


class Par2FoldinOptions(C.Structure):             # aoadmm_par2_foldin_options
    _fields_ = [('max_iter', C.c_int), ('tol', C.c_double), ('ridge', C.c_double), ('constraint', C.c_int), ('max_inner', C.c_int),
                ('tol_primal', C.c_double), ('tol_dual', C.c_double)]


class NvecsInfo(C.Structure):                     # aoadmm_nvecs_info
    _fields_ = [('iterations', C.c_int), ('converged', C.c_int), ('block', C.c_int), ('residual', C.c_double),
                ('fibers', C.c_int64)]


_lib = None


def load_library():
    """Load libaoadmm_hip.so; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'libaoadmm_hip.so is missing (%s). Build it with `python -c "import __graft_entry__ as g; g.build()"` '
            'or `make -C matlab-code_amd/csrc`. There is no CPU fallback.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    lib.aoadmm_last_error.restype = C.c_char_p
    dp = C.POINTER(C.c_double)
    i64 = C.c_int64
    vp = C.c_void_p
    lib.aoadmm_create.argtypes = [C.POINTER(vp), C.c_int]
    lib.aoadmm_create_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int)]
    lib.aoadmm_destroy.argtypes = [vp]
    lib.aoadmm_synchronize.argtypes = [vp]
    lib.aoadmm_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.aoadmm_set_progress.argtypes = [vp, PROGRESS_FN, vp, C.c_int]
    lib.aoadmm_comm_unique_id.argtypes = [C.c_char_p]
    lib.aoadmm_comm_init_rank.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    lib.aoadmm_comm_init_rank_share.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    lib.aoadmm_comm_init_local.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.aoadmm_comm_rank.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.aoadmm_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    lib.aoadmm_model_begin.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.aoadmm_model_set_mode.argtypes = [vp, C.c_int, i64, C.c_int]
    lib.aoadmm_model_set_mode_slabs.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i64), C.c_int]
    lib.aoadmm_model_add_cp.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_double]
    lib.aoadmm_model_add_par2.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.c_double]
    lib.aoadmm_model_set_constraint.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int, dp]
    lib.aoadmm_model_set_coupling.argtypes = [vp, C.c_int, C.c_int, dp, i64, i64, dp, i64, i64]
    lib.aoadmm_model_set_coupling_type.argtypes = [vp, C.c_int, C.c_int]
    lib.aoadmm_model_set_ridge.argtypes = [vp, dp]
    lib.aoadmm_model_end.argtypes = [vp]
    lib.aoadmm_tensor_upload.argtypes = [vp, C.c_int, dp, C.c_int]
    lib.aoadmm_tensor_upload_rows.argtypes = [vp, C.c_int, dp, i64, i64, C.c_int]
    lib.aoadmm_tensor_upload_coo.argtypes = [vp, C.c_int, i64, C.POINTER(i64), dp]
    lib.aoadmm_tensor_upload_coo_sharded.argtypes = [vp, C.c_int, i64, C.POINTER(i64), dp]
    lib.aoadmm_par2_slab_upload.argtypes = [vp, C.c_int, C.c_int, dp]
    lib.aoadmm_par2_slab_upload_coo.argtypes = [vp, C.c_int, i64, C.POINTER(i64), dp]
    lib.aoadmm_tensor_mask_upload.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8)]
    lib.aoadmm_par2_slab_mask_upload.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_uint8)]
    lib.aoadmm_tensor_weights_upload.argtypes = [vp, C.c_int, dp]
    lib.aoadmm_tensor_synth.argtypes = [vp, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_int]
    lib.aoadmm_tensor_normsq.argtypes = [vp, C.c_int, dp]
    lib.aoadmm_tensor_storage_info.argtypes = [vp, C.c_int, C.POINTER(C.c_int), dp, C.POINTER(i64)]
    lib.aoadmm_tensor_rank.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    lib.aoadmm_tensor_set_observed_only.argtypes = [vp, C.c_int, C.c_int]
    lib.aoadmm_tensor_set_entry_weights.argtypes = [vp, C.c_int, i64, C.POINTER(i64), dp, C.c_double]
    lib.aoadmm_resident_em_step.argtypes = [vp, C.c_int, dp]
    lib.aoadmm_resident_em_pass.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, C.POINTER(i64)]
    lib.aoadmm_tensor_set_missing_list.argtypes = [vp, C.c_int, C.c_int]
    lib.aoadmm_tensor_missing_list.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    lib.aoadmm_resident_em_list_pass.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp]
    lib.aoadmm_resident_model_at.argtypes = [vp, C.c_int, i64, C.POINTER(i64), dp]
    lib.aoadmm_tensor_set_heldout.argtypes = [vp, C.c_int, i64, C.POINTER(i64), dp]
    lib.aoadmm_resident_heldout_stats.argtypes = [vp, C.c_int, dp]
    lib.aoadmm_heldout_info.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int)]
    lib.aoadmm_heldout_trace.argtypes = [vp, C.c_int, dp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.aoadmm_heldout_keep_best.argtypes = [vp, C.c_int]
    lib.aoadmm_heldout_restore_best.argtypes = [vp, C.POINTER(C.c_int)]
    lib.aoadmm_heldout_best_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(i64)]
    lib.aoadmm_resident_topk.argtypes = [vp, C.c_int, C.c_int, i64, C.POINTER(i64), C.c_int, C.POINTER(i64), C.POINTER(i64),
                                         C.POINTER(i64), dp]
    lib.aoadmm_resident_topk_w.argtypes = [vp, C.c_int, C.c_int, i64, dp, C.c_int, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), dp]
    lib.aoadmm_resident_rank_of.argtypes = [vp, C.c_int, C.c_int, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), dp,
                                            C.POINTER(i64)]
    lib.aoadmm_resident_rank_of_w.argtypes = [vp, C.c_int, C.c_int, i64, dp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
                                              dp, C.POINTER(i64)]
    lib.aoadmm_resident_project.argtypes = [vp, C.c_int, C.POINTER(dp), C.POINTER(i64), C.POINTER(C.c_int), dp]
    lib.aoadmm_resident_core_consistency.argtypes = [vp, C.c_int, dp, dp, C.POINTER(C.c_int)]
    lib.aoadmm_tensor_set_ranklist.argtypes = [vp, C.c_int, C.c_int, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    lib.aoadmm_ranklist_info.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(i64)]
    lib.aoadmm_rank_track.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.aoadmm_rank_trace.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.aoadmm_ranklist_last.argtypes = [vp, C.c_int, C.POINTER(i64), dp, C.POINTER(i64)]
    lib.aoadmm_op_rank_metrics.argtypes = [vp, i64, C.POINTER(i64), C.POINTER(i64), i64, dp]
    lib.aoadmm_resident_fold_in.argtypes = [vp, C.c_int, C.c_int, i64, i64, C.POINTER(i64), dp, C.POINTER(FoldinOptions), dp,
                                            C.POINTER(C.c_int), C.POINTER(C.c_int), dp, dp]
    lib.aoadmm_resident_fold_in_w.argtypes = [vp, C.c_int, C.c_int, i64, i64, C.POINTER(i64), dp, dp, C.c_double, C.POINTER(FoldinOptions),
                                              dp, C.POINTER(C.c_int), C.POINTER(C.c_int), dp, dp]
    lib.aoadmm_par2_rows.argtypes = [vp, C.c_int, C.POINTER(i64)]
    lib.aoadmm_resident_par2_fold_in.argtypes = [vp, C.c_int, i64, C.POINTER(i64), dp, dp, C.POINTER(Par2FoldinOptions), dp, dp, dp, dp, dp,
                                                 C.POINTER(C.c_int), C.POINTER(C.c_int), dp, dp, C.POINTER(C.c_int)]
    lib.aoadmm_state_set.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, i64, i64]
    lib.aoadmm_state_get.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, i64, i64]
    lib.aoadmm_solve.argtypes = [vp, C.POINTER(Options), C.POINTER(Result)]
    lib.aoadmm_resident_mttkrp.argtypes = [vp, C.c_int, C.c_int, dp, C.POINTER(C.c_float)]
    lib.aoadmm_resident_par2_rhs.argtypes = [vp, C.c_int, C.c_int, dp, C.POINTER(C.c_float)]
    lib.aoadmm_kernel_stats.argtypes = [vp, C.c_int, C.c_int, dp, C.POINTER(i64), dp, dp]
    lib.aoadmm_op_mttkrp.argtypes = [vp, dp, C.c_int, C.POINTER(i64), C.POINTER(dp), C.c_int, C.c_int, C.c_int, dp]
    lib.aoadmm_op_unfold_gram.argtypes = [vp, dp, C.c_int, C.POINTER(i64), C.c_int, C.c_int, dp]
    lib.aoadmm_resident_unfold_gram.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    lib.aoadmm_resident_nvecs.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(NvecsOptions), dp, i64, dp,
                                          C.POINTER(NvecsInfo)]
    lib.aoadmm_op_gram.argtypes = [vp, dp, i64, C.c_int, dp]
    lib.aoadmm_op_chol.argtypes = [vp, dp, C.c_int, dp]
    lib.aoadmm_op_prox.argtypes = [vp, C.c_int, dp, C.c_int, dp, dp, i64, C.c_int, C.c_double, dp]
    lib.aoadmm_op_admm_constrained.argtypes = [vp, dp, dp, C.c_double, C.c_int, dp, C.c_int, dp, i64, C.c_int,
                                               C.c_int, C.c_double, C.c_double, dp, dp, dp, C.POINTER(C.c_int)]
    lib.aoadmm_op_admm_mode.argtypes = [vp, dp, dp, C.c_int, dp, C.c_int, dp, i64, C.c_int, C.c_int, C.c_double,
                                        C.c_double, dp, dp, dp, C.POINTER(C.c_int), dp, dp, dp, C.POINTER(C.c_int)]
    ip = C.POINTER(C.c_int)
    lib.aoadmm_op_par2_b_loop.argtypes = [vp, C.c_int, C.POINTER(i64), C.c_int, dp, dp, dp, C.c_double, C.c_double,
                                          C.c_int, dp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, ip, dp, ip]
    dpp = C.POINTER(dp)
    lib.aoadmm_op_coupled_loop.argtypes = [vp, C.c_int, dpp, dpp, C.c_int, dp, ip, dp, dp, dpp, dpp, dp, ip]
    lib.aoadmm_op_par2_mode_a.argtypes = [vp, C.c_int, C.POINTER(i64), C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, ip]
    lib.aoadmm_op_par2_mode_c.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i64), C.c_int, C.c_int, dp, dp, dp, C.c_double,
                                          C.c_double, C.c_double, C.c_int, dp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp,
                                          dp, dp, dp, dp, ip, dp, ip]
    lib.aoadmm_op_par2_objective.argtypes = [vp, C.c_int, C.POINTER(i64), C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp,
                                             C.c_int, C.c_double, dp, dp, dp]
    for name in SYMBOLS:
        fn = getattr(lib, name)
        if name != 'aoadmm_last_error':
            fn.restype = C.c_int
    _lib = lib
    return lib


def check(status):
    if status == OK:
        return
    msg = load_library().aoadmm_last_error().decode('utf-8', 'replace')
    if status == ERR_NOT_PD:
        raise NotPositiveDefinite(status, msg)
    if status == ERR_UNSUPPORTED:
        raise UnsupportedOnDevice(status, msg)
    raise AoadmmError(status, msg)


def as_f(a):
    """Column-major (MATLAB layout) float64 copy/view."""
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
