/*
 * aoadmm_hip.h -- C ABI of the MI355X-native AO-ADMM engine (libaoadmm_hip.so).
 *
 * This is the drop-in boundary for the hot path of
 * AOADMM-DataFusionFramework/Matlab-Code.  Citations are relative to the
 * reference repository root.
 *
 *   solver level : replaces the call
 *       [Fac,out] = cmtf_fun_AOADMM(Z,Znorm_const,G,fh,gh,lscalar,uscalar,options)
 *       at functions/cmtf_AOADMM.m:193 (signature functions/cmtf_fun_AOADMM.m:1).
 *   op level     : the L2->L1 calls inside that function (mttkrp, Gram,
 *       Cholesky system, ADMM inner loops, prox operators, objective), exported
 *       for unit parity against the CPU oracle.
 *
 * Conventions
 *   - every matrix/tensor crossing the boundary is IEEE double, column-major
 *     (MATLAB layout), passed as plain pointer + 64-bit sizes;
 *   - mode numbers, tensor numbers and coupling ids are 0-based here (the MEX /
 *     ctypes host layer subtracts 1 from MATLAB's numbers); "no coupling" is -1;
 *   - every function returns an int status (AOADMM_OK == 0); the message of the
 *     last failure on the calling thread is returned by aoadmm_last_error();
 *   - no C++ exception crosses this boundary; the library owns all device
 *     memory behind the opaque handle and keeps no pointer into caller memory
 *     after a call returns (functions/cmtf_AOADMM.m value semantics).
 *   - there is NO CPU fallback: without a usable gfx950 device every compute
 *     entry point returns AOADMM_ERR_HIP.
 */
#ifndef AOADMM_HIP_H
#define AOADMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AOADMM_ABI_VERSION 3

/* ---- status codes ------------------------------------------------------ */
enum {
  AOADMM_OK = 0,
  AOADMM_ERR_INVALID = 1,     /* bad argument / inconsistent model (check_data_input.m) */
  AOADMM_ERR_HIP = 2,         /* HIP runtime failure or no device */
  AOADMM_ERR_NOT_PD = 3,      /* chol() failed: system matrix not positive definite
                                 (cmtf_fun_AOADMM.m:142,185,273,362 throw in MATLAB) */
  AOADMM_ERR_RCCL = 4,        /* collective failure */
  AOADMM_ERR_UNSUPPORTED = 5, /* feature routed back to the MATLAB path:
                                 non-Frobenius loss, 'custom' prox; also an op the engine has no
                                 answer for on the data it holds (e.g. resident_unfold_gram of a
                                 sparse block) */
  AOADMM_ERR_NOMEM = 6
};

/* ---- constraint catalogue: functions/constraints_to_prox.m:13-91 -------- */
enum {
  AOADMM_C_NONE = 0,
  AOADMM_C_NONNEG = 1,          /* :13  {'non-negativity'} */
  AOADMM_C_BOX = 2,             /* :15  {'box',l,u}                 params: l,u */
  AOADMM_C_SIMPLEX_COL = 3,     /* :19  {'simplex column-wise',eta} params: eta */
  AOADMM_C_SIMPLEX_ROW = 4,     /* :22  {'simplex row-wise',eta} */
  AOADMM_C_NONDECREASING = 5,   /* :25 */
  AOADMM_C_NONINCREASING = 6,   /* :27 */
  AOADMM_C_UNIMODAL = 7,        /* :29  {'unimodality',nn}          params: nn (0/1) */
  AOADMM_C_L1_BALL = 8,         /* :32  params: eta */
  AOADMM_C_L2_BALL = 9,         /* :35  params: eta */
  AOADMM_C_NONNEG_L2_BALL = 10, /* :38  params: eta */
  AOADMM_C_NONNEG_L2_SPHERE = 11, /* :41 params: eta (ignored, as in the reference) */
  AOADMM_C_ORTHONORMAL = 12,    /* :44 */
  AOADMM_C_L1_REG = 13,         /* :46  params: eta */
  AOADMM_C_L0_REG = 14,         /* :50 */
  AOADMM_C_L2_REG = 15,         /* :54 */
  AOADMM_C_RIDGE = 16,          /* :58 */
  AOADMM_C_QUADRATIC = 17,      /* :62  params: eta ; matrix L passed separately */
  AOADMM_C_GL_SMOOTH = 18,      /* :68  params: eta */
  AOADMM_C_TV = 19,             /* :78  params: eta */
  AOADMM_C_TPARAFAC2 = 20       /* :82  params: eta (PARAFAC2 B_k mode only) */
};

/* ---- state fields of the struct G: init_coupled_AOADMM_CMTF.m:41-45 ----- */
enum {
  AOADMM_F_FAC = 0,              /* G.fac{m} (or G.fac{m}{k})            index = mode     */
  AOADMM_F_CONSTRAINT_FAC = 1,   /* G.constraint_fac{m}                  index = mode     */
  AOADMM_F_CONSTRAINT_DUAL = 2,  /* G.constraint_dual_fac{m}             index = mode     */
  AOADMM_F_COUPLING_FAC = 3,     /* G.coupling_fac{c}                    index = coupling */
  AOADMM_F_COUPLING_DUAL = 4,    /* G.coupling_dual_fac{m}               index = mode     */
  AOADMM_F_DELTAB = 5,           /* G.DeltaB{p}                          index = tensor   */
  AOADMM_F_P = 6,                /* G.P{p}{k}                            index = tensor   */
  AOADMM_F_MU_DELTAB = 7         /* G.mu_DeltaB{p}{k}                    index = tensor   */
};

/* storage / arithmetic of the big tensor passes */
enum {
  AOADMM_PREC_F64 = 0, /* tensor stored fp64, v_mfma_f64_16x16x4_f64 (parity mode)        */
  AOADMM_PREC_F32 = 1, /* tensor stored fp32, v_mfma_f32_16x16x4_f32 (+ packed-fp32 VALU for 1-4 leftover columns),
                          fp64 everywhere else */
  AOADMM_PREC_F16 = 2  /* dense 3-way CP blocks only: entries stored fp16 with one power-of-two scale per block,
                          v_mfma_f32_16x16x32_f16 with fp32 accumulation; everything else as AOADMM_PREC_F32.
                          The rule, which a host can reproduce bit for bit:
                            1. round the entries to fp32 (as AOADMM_PREC_F32 does);
                            2. a = max |x| over those fp32 values = m * 2^E with m in [0.5, 1)  (frexp);
                            3. s = 2^(15 - E), the exponent clamped to [-126, 127] so that s is a normal fp32 number:
                               a * s lies in [2^14, 2^15);  an all-zero block has s = 1;
                            4. a non-finite entry makes the upload fail with AOADMM_ERR_INVALID;
                            5. stored: q = fp16(x_fp32 * s), round to nearest even, subnormals kept;
                            6. the block's data IS q / s: aoadmm_tensor_normsq is the fp64 sum of (q / s)^2 and the
                               model is fitted to q / s.
                          Resident: three fp16 pass copies (6 bytes per entry; 10 at the peak of the upload); the
                          natural-layout array is released at once, so aoadmm_tensor_mask_upload on such a block is
                          AOADMM_ERR_INVALID and aoadmm_resident_unfold_gram AOADMM_ERR_UNSUPPORTED, and aoadmm_solve
                          with options.no_permuted_copy = 1 is AOADMM_ERR_INVALID (the copies are the data).
                          On an engine that belongs to a communicator (aoadmm_comm_init_rank, aoadmm_comm_init_local,
                          aoadmm_comm_init_rank_share, also one of a single rank) aoadmm_tensor_upload with the whole
                          array and aoadmm_tensor_synth are COLLECTIVE for this precision: every rank must make the
                          call.  Each rank takes max |x| and "not finite" over everything it holds (its rows of mode 1
                          and, where every rank owns one, its slab of mode 3 for the mode-1 pass), one sum all-reduce
                          of world + 1 doubles carries them round, and steps 2-4 apply to the maximum of the WHOLE
                          tensor: s is the same on every rank, and a non-finite entry anywhere fails the call on
                          EVERY rank (after the exchange, so no rank is left alone in a later collective).
                          aoadmm_tensor_normsq is all-reduced over the ranks' rows before the division by s^2;
                          aoadmm_tensor_storage_info reports the rank's own resident bytes and the common s.
                          AOADMM_ERR_UNSUPPORTED, the block left as it was: a block that is not 3-way,
                          aoadmm_tensor_upload_rows (the scale comes from the whole tensor),
                          aoadmm_op_mttkrp / aoadmm_op_unfold_gram (they run on a natural-layout array), and a
                          multi-device context (aoadmm_create_multi with more than one device: one caller, one array
                          for all engines; one context per rank and a communicator serve the same job).  A copy that
                          cannot be built fails the upload on that rank alone (AOADMM_ERR_NOMEM: no room in device
                          memory; AOADMM_ERR_UNSUPPORTED: a mode too
                          long for the copy kernels) and leaves the block without data. */
};

typedef struct aoadmm_ctx aoadmm_ctx;

/* options struct: example_script1_CP_PAR2_nonneg.m:110-123, cmtf_fun_AOADMM.m:4-9 */
typedef struct aoadmm_options {
  int32_t MaxOuterIters;
  int32_t MaxInnerIters;
  double AbsFuncTol;
  double OuterRelTol;
  double innerRelPrTol_coupl;
  double innerRelPrTol_constr;
  double innerRelDualTol_coupl;
  double innerRelDualTol_constr;
  int32_t bsum;
  double bsum_weight;
  int32_t iter_start_PAR2Bkconstraint;   /* default 0 (cmtf_fun_AOADMM.m:7-9) */
  int32_t has_increase_factor_rhoBk;     /* isfield(options,'increase_factor_rhoBk') */
  double increase_factor_rhoBk;
  int32_t use_dimtree;                   /* engine option (options.hip.*): reuse partial
                                            contractions between modes; 1 = default */
  int32_t no_permuted_copy;              /* engine option: 1 = do not keep the two mode-permuted resident copies of
                                            3-way tensors (saves twice the tensor's size in HBM; mode-1 contractions then
                                            use the LDS-transposed kernel, mode-2 ones run batched); 0 = default */
  int32_t par2_slab_sharding;            /* engine option, with a communicator: 0 = auto (a PARAFAC2 block is repeated
                                            on every rank unless it has >= 1024 slabs per rank), 1 = shard the slabs
                                            over the ranks, -1 = never.  Blocks with Z.miss or the tPARAFAC2 constraint
                                            are always repeated */
  int32_t heldout_patience;              /* engine option: k > 0 stops the solve after iteration i when H_i = sum over the
                                            blocks with a held-out list of w_p * sum (y - m)^2 has not been strictly below
                                            its best value so far for k consecutive iterations (exit_code 2); 0 = off.
                                            k > 0 with no list attached: AOADMM_ERR_INVALID before any work */
  int32_t reserved[4];
} aoadmm_options;

/* `out` struct of cmtf_fun_AOADMM.m:480-494.  Arrays are caller-allocated with
 * MaxOuterIters+1 entries (innerIters: n_modes*MaxOuterIters, column-major
 * n_modes x MaxOuterIters like out.innerIters). */
typedef struct aoadmm_result {
  double f_tensors, f_couplings, f_constraints, f_PAR2_couplings;
  int32_t OuterIterations;
  int32_t exit_code;            /* 0 = 'maxIterations', 1 = stopping rule met (make_exit_flag.m), 2 = stopped by
                                   aoadmm_options.heldout_patience, 3 = stopped by the patience of aoadmm_rank_track
                                   (when the stopping rule fires in the same iteration: 1; a rule that fires in
                                   iteration MaxOuterIters reports 0, as before) */
  int32_t exit_abs[4];          /* per quantity: 1 = 'AbsFuncTol', 0 = 'RelFuncTol' */
  double *func_val_conv, *func_coupl_conv, *func_constr_conv, *func_PAR2_coupl, *time_at_it;
  double *innerIters;
  /* EM missing data (cmtf_fun_AOADMM.m:408-441, :485, :490-492): NaN / untouched without Z.miss */
  double f_rel_missing;
  double *func_rel_missing;     /* MaxOuterIters+1 entries, [0] = NaN; may be NULL */
} aoadmm_result;

/* Progress report of options.Display = 'iter' (cmtf_fun_AOADMM.m:44-59, :462-468): called on the caller's thread
 * from inside aoadmm_solve after the initial evaluation (iter = 0) and after every `every`-th outer iteration with
 * f = {f_tensors, f_couplings, f_constraints, f_PAR2_couplings} and f_rel_missing (NaN without Z.miss).
 * On a multi-device context the rows are produced by rank 0's worker thread and handed to the calling thread,
 * which delivers them while it waits inside aoadmm_solve (a MEX callback may use mexPrintf / drawnow).
 * The callback must not throw and must not call back into the library. */
typedef void (*aoadmm_progress_fn)(void* user, int iter, const double f[4], double f_rel_missing);

/* ---- library / context ------------------------------------------------- */
int aoadmm_abi_version(void);
const char* aoadmm_last_error(void);
int aoadmm_device_count(int* n);
int aoadmm_create(aoadmm_ctx** ctx, int device);
/* One process, several GPUs (a MATLAB session): the context owns one engine and one host thread per
 * listed device, joined by RCCL; every call below is executed by all of them together and returns when the last is
 * done, outputs come from rank 0.  The model is sharded exactly as with one process per GPU.  Listing a device more
 * than once selects the host-staged bring-up transport of aoadmm_comm_init_local (that is how the one-GPU test box
 * runs this path).  aoadmm_comm_init_* are not valid on such a context. */
int aoadmm_create_multi(aoadmm_ctx** ctx, int n_devices, const int* devices);
int aoadmm_destroy(aoadmm_ctx* ctx);
int aoadmm_synchronize(aoadmm_ctx* ctx);
/* fn = NULL or every <= 0 switches the report off (options.DisplayIters is `every`) */
int aoadmm_set_progress(aoadmm_ctx* ctx, aoadmm_progress_fn fn, void* user, int every);

/* Multi-GPU (one process per GPU): rank 0 creates an id, the host layer
 * broadcasts it (torch.distributed / MPI / a file), every rank joins.  The CP
 * tensor is then row-sharded along its first mode; factor matrices
 * are replicated and only MTTKRP partials cross xGMI. */
int aoadmm_comm_unique_id(char id[128]);
int aoadmm_comm_init_rank(aoadmm_ctx* ctx, const char id[128], int rank, int world);
/* Measurement hook (bench.py --as-rank R --of N): the context takes rank `rank` of `world` in every sharding decision
 * (row block of mode 1, mode-3 slab of the mode-1 pass, own-rows buffers) but joins a ONE-rank RCCL communicator, so
 * every collective is issued (ncclAllReduce on the library's stream) without peers.  It times one rank's share of an
 * N-GPU job on a one-GPU box; the sums are that rank's partial sums only, so the factors are NOT those of the N-rank job. */
int aoadmm_comm_init_rank_share(aoadmm_ctx* ctx, const char id[128], int rank, int world);
/* Bring-up/test transport: `world` contexts driven by threads of ONE process (on one device or several) form
 * group `key`; collectives go through host staging in rank order.  It lets the sharded data path run with
 * world > 1 on a single GPU, which RCCL refuses.  Every rank must make the same sequence of library calls. */
int aoadmm_comm_init_local(aoadmm_ctx* ctx, int key, int rank, int world);
int aoadmm_comm_rank(aoadmm_ctx* ctx, int* rank, int* world);
/* What the collectives run on: ncclGetVersion() of the RCCL this process resolved, ncclCommCount() of the context's
 * communicator (0 without one; the group size for the bring-up transport) and the path of the loaded librccl
 * (bench.py reports all three).  Any pointer may be NULL. */
int aoadmm_comm_info(aoadmm_ctx* ctx, int* nccl_version, int* comm_ranks, char* lib_path, int lib_path_cap);

/* ---- model (the struct Z) ---------------------------------------------- */
/* Z.size / Z.modes / Z.model / Z.weights (example_script1_CP_PAR2_nonneg.m:74-89) */
int aoadmm_model_begin(aoadmm_ctx* ctx, int n_modes, int n_tensors, int n_couplings);
int aoadmm_model_set_mode(aoadmm_ctx* ctx, int mode, int64_t rows, int rank);
int aoadmm_model_set_mode_slabs(aoadmm_ctx* ctx, int mode, int K, const int64_t* rows_k, int rank);
int aoadmm_model_add_cp(aoadmm_ctx* ctx, int p, int n_tensor_modes, const int* modes, double weight);
int aoadmm_model_add_par2(aoadmm_ctx* ctx, int p, const int* modes3, double weight);
/* Z.constrained_modes / Z.constraints{m}; Lmat only for AOADMM_C_QUADRATIC (rows x rows) */
int aoadmm_model_set_constraint(aoadmm_ctx* ctx, int mode, int constraint, const double* params,
                                int n_params, const double* Lmat);
/* Z.coupling.lin_coupled_modes(mode)=coupling ; coupl_trafo_matrices{mode} (H, hr x hc) ;
 * coupl_trafo_matrices2{mode} (H2).  Pass NULL/0 when absent. */
int aoadmm_model_set_coupling(aoadmm_ctx* ctx, int mode, int coupling, const double* H, int64_t hr,
                              int64_t hc, const double* H2, int64_t h2r, int64_t h2c);
int aoadmm_model_set_coupling_type(aoadmm_ctx* ctx, int coupling, int type);
int aoadmm_model_set_ridge(aoadmm_ctx* ctx, const double* ridge_per_mode); /* Z.ridge */
int aoadmm_model_end(aoadmm_ctx* ctx);

/* ---- data (Z.object{p}) ------------------------------------------------- */
/* dense CP block: host column-major doubles, dims as given to model_set_mode.
 * With a communicator, every rank passes the FULL array and keeps its row block,
 * or passes only its block with local_rows/row_offset != full. */
int aoadmm_tensor_upload(aoadmm_ctx* ctx, int p, const double* data, int precision);
/* one-process-per-GPU contexts only (a multi-device context takes the full array and shards it itself) */
int aoadmm_tensor_upload_rows(aoadmm_ctx* ctx, int p, const double* block, int64_t row_offset,
                              int64_t local_rows, int precision);
/* PARAFAC2 slab k (I x J_k).  k = AOADMM_ALL_SLABS: the K slabs back to back (I x sum J_k) in one transfer;
 * the same convention holds for aoadmm_par2_slab_mask_upload and for the cell-valued state fields below. */
#define AOADMM_ALL_SLABS (-1)
int aoadmm_par2_slab_upload(aoadmm_ctx* ctx, int p, int k, const double* Xk);
/* Z.miss{p} (cmtf_AOADMM.m:68-121): one byte per entry, 1 = observed, 0 = missing, same shape and
 * column-major order as Z.object{p} (the FULL array also when row-sharded) / as slab k.  Upload after the
 * data.  A block with a mask is handled by EM imputation inside aoadmm_solve (cmtf_fun_AOADMM.m:408-441):
 * the resident copy of the data is overwritten at the missing positions every outer iteration. */
int aoadmm_tensor_mask_upload(aoadmm_ctx* ctx, int p, const uint8_t* mask);
int aoadmm_par2_slab_mask_upload(aoadmm_ctx* ctx, int p, int k, const uint8_t* mask_k);
/* PER-ENTRY WEIGHTS on a dense CP block: W in [0, 1], same shape and column-major order as
 * Z.object{p} (the FULL array also when row-sharded, like the mask).  Upload after the data.  aoadmm_solve then minimises
 * Z.weights(p) * sum W o (X - M)^2 with the rest of the model by the reference's EM (cmtf_fun_AOADMM.m:408-441) with the
 * imputation Xhat = W o X + (1 - W) o M(F) after every outer iteration, from Xhat = W o X in every solve:
 *   func_val_conv      carries Z.weights(p) * sum W o (X - M)^2 for the block
 *   func_rel_missing   num = ||(1 - W) o (M_new - M_old)||^2, den = ||(1 - W) o M_old||^2, M_old = 0 before the first
 *                      iteration (den = 0 gives sqrt(num), as with a mask)
 *   aoadmm_tensor_normsq   sum W o X^2
 * A boolean W is Z.miss, W = 1 everywhere the plain block, w = 0 makes an entry missing.  The weights live in the
 * block's precision: an fp32 block rounds W to fp32 here, and the objective uses the rounded weights.  The block keeps
 * the data as uploaded and the weights beside Xhat: three arrays of the tensor's size (a matrix: six with the transposed
 * copies; aoadmm_tensor_storage_info counts them), and no pass copies.  W = NULL removes the weights: the block is plain
 * again and holds the data as uploaded.  A later upload of the data clears the weights; of aoadmm_tensor_mask_upload and
 * this call the later one wins (a mask drops the weights, weights drop the mask).  Weights above 1 are the caller's to
 * normalise: divide W by its maximum and fold that maximum into Z.weights(p).
 * On a masked block the call takes what the block holds as the data, so it is refused once an EM pass or a solve has
 * written model values over the missing entries: upload the data again first.  With a communicator every rank checks the
 * whole W, so all ranks reach the same verdict.
 * AOADMM_ERR_INVALID, block as it was: a value outside [0, 1] or not finite; no data yet; a masked block that has been
 * imputed; a sparse block (its weights go
 * through aoadmm_tensor_set_entry_weights); an fp16 block; a block whose natural array was released.
 * AOADMM_ERR_UNSUPPORTED: a PARAFAC2 block, a multi-device context.  Two runs return the same bits. */
int aoadmm_tensor_weights_upload(aoadmm_ctx* ctx, int p, const double* W);
/* device-side synthetic CP tensor: X = [[A1,..,AN]] + noise, ||X|| = 1;
 * never crosses PCIe.  normsq_out receives ||X||^2 after normalisation. */
int aoadmm_tensor_synth(aoadmm_ctx* ctx, int p, int rank, uint64_t seed, double noise, int precision);
/* Z.object{p} as a Tensor Toolbox sptensor (cmtf_AOADMM.m:77-79, :132) or a MATLAB sparse matrix:
 * nnz nonzeros, subs column-major nnz x n_tensor_modes (the layout of sptensor.subs), 0-based; vals nnz doubles.
 * Duplicate subscripts are summed (sptensor's constructor rule).  Values stay fp64.
 * Sizes come from aoadmm_model_set_mode (each below 2^31); a subscript out of range or nnz < 0 is
 * AOADMM_ERR_INVALID, nnz = 0 is valid.  A later aoadmm_tensor_upload replaces the sparse form and this call
 * replaces a dense one.  On a sparse block aoadmm_tensor_mask_upload, aoadmm_tensor_upload_rows and
 * aoadmm_tensor_synth return AOADMM_ERR_INVALID and aoadmm_resident_unfold_gram AOADMM_ERR_UNSUPPORTED
 * (aoadmm_resident_nvecs gives the leading eigenvectors instead);
 * aoadmm_tensor_normsq, aoadmm_resident_mttkrp and aoadmm_solve work as for dense data.  With a communicator
 * every rank holds all nonzeros and computes the complete MTTKRP (no collective for the block): N (4 N + 8) bytes
 * per coalesced nonzero on every rank, and no rank's MTTKRP gets shorter with more ranks.
 * aoadmm_tensor_upload_coo_sharded is the form that divides both. */
int aoadmm_tensor_upload_coo(aoadmm_ctx* ctx, int p, int64_t nnz, const int64_t* subs, const double* vals);
/* The same block with its nonzeros SHARDED over the ranks of the communicator.  Arguments and validation are those of
 * aoadmm_tensor_upload_coo; every rank passes the WHOLE list and all ranks make the call together.  The list is
 * coalesced as a whole first (duplicates summed before anything is cut: the same model), then with nnz coalesced
 * nonzeros rank g of `world` keeps the entries [floor(g nnz / world), floor((g + 1) nnz / world)) of EVERY mode's
 * sorted copy: the same numeric cut applied to each mode's own order.  A copy is sorted by its mode's row, so a rank's
 * share of mode n is a contiguous row span that overlaps its neighbours in at most the boundary rows, and a row with
 * many nonzeros is spread over as many ranks as its length asks for (the balance does not depend on skew).  A share
 * may be empty (nnz < world).  Resident afterwards: N (4 N + 8) bytes per KEPT nonzero; the peak during the call is
 * that of aoadmm_tensor_upload_coo (the full copies are built, cut and freed; an upload that hands each rank only a
 * part of the list does not exist).  Without a communicator, or with world = 1, the call IS
 * aoadmm_tensor_upload_coo, bit for bit.  A multi-device context shards over its engines.
 *   On a sharded block: aoadmm_tensor_normsq is the all-reduced sum of squares of the mode-0 shares;
 *   aoadmm_resident_mttkrp and every MTTKRP inside aoadmm_solve are COLLECTIVES (each rank writes its partial sums into
 *   its row span of a zeroed send buffer of I_n x R doubles, one all-reduce returns the complete result on every rank;
 *   every rank takes part, with an empty share too; no float atomics, two runs return the same bits);
 *   aoadmm_resident_nvecs returns AOADMM_ERR_UNSUPPORTED (its fiber lists need all nonzeros); the refusals of a sparse
 *   block above stay.  A block whose share was cut for another (rank, world) than the context has now answers
 *   AOADMM_ERR_INVALID ("upload again") to these calls.  The next upload of either kind replaces the block. */
int aoadmm_tensor_upload_coo_sharded(aoadmm_ctx* ctx, int p, int64_t nnz, const int64_t* subs, const double* vals);
/* Marks (on != 0) or unmarks a sparse CP block as OBSERVED-ONLY: its stored entries (after coalescing; explicit zeros
 * are kept) are the observations, every other entry is MISSING instead of an observed zero.  aoadmm_solve then runs the
 * reference's EM imputation (cmtf_fun_AOADMM.m:408-441) on the block as it would on the densified tensor with the mask
 * "is stored" -- same factors, duals, innerIters, func_val_conv, func_rel_missing and stopping rule (:457-459) -- without
 * an array of the tensor's size: the missing entries start at 0 in every solve, the MTTKRP is the sparse MTTKRP of the
 * residuals on the stored entries plus a rank-R correction from the factor snapshot of the last EM step, and the
 * statistics are sums over the stored entries and R x R products (no float atomics: two runs return the same bits).
 * Resident afterwards: N (4 N + 16) bytes per nonzero plus two copies of every factor (aoadmm_tensor_storage_info).
 * Valid on a block uploaded with aoadmm_tensor_upload_coo that holds at least one entry (none: AOADMM_ERR_INVALID);
 * AOADMM_ERR_UNSUPPORTED for a dense block, a PARAFAC2 block and a block uploaded with
 * aoadmm_tensor_upload_coo_sharded.  Any later upload of the block clears the mark.  aoadmm_tensor_mask_upload on
 * sparse data stays refused.  With a communicator the block is replicated: every rank does the same work, no
 * collective. */
int aoadmm_tensor_set_observed_only(aoadmm_ctx* ctx, int p, int on);
/* WEIGHTS for an observed-only block: stored entry e gets w_e = wts[e] in [0, 1], every unstored entry the one weight
 * unstored_weight (alpha) in [0, 1]; W is the dense array those define.  aoadmm_solve then minimises
 * Z.weights(p) * sum W o (X - M)^2 with the rest of the model by the same EM (cmtf_fun_AOADMM.m:408-441) with the
 * imputation Xhat = W o X + (1 - W) o M_old (the majoriser of Srebro and Jaakkola), from Xhat = W o X in every solve.
 * w = 1 everywhere with alpha = 0 is the observed-only block, with alpha = 1 the plain block; w_e = 0 makes a stored
 * entry missing.  The model never exists as an array:
 *   residual array of a copy   r_e = w_e x_e - (w_e - alpha) m_old,e              (w_e x_e before the first step)
 *   MTTKRP of mode n           weight * [sparse MTTKRP of r + (1 - alpha) Fo_n had_{j != n}(Fo_j' F_j)]
 *   objective                  sum_Omega w_e (x_e - m_e)^2 + alpha (sum(had_n F_n' F_n) - sum_Omega m_e^2)
 *   num of f_rel_missing       (1 - alpha)^2 (||M_new - M_old||^2 - sum_Omega dm^2) + sum_Omega (1 - w_e)^2 dm_e^2
 *   den                        (1 - alpha)^2 (||M_old||^2 - sum_Omega m_old^2) + sum_Omega (1 - w_e)^2 m_old,e^2
 * (the stopping rule :457-459 is unchanged, num = den = 0 gives 0), and aoadmm_tensor_normsq returns sum_Omega w x^2.
 * subs is column-major nnz x N, 0-based, in any order, as aoadmm_tensor_upload_coo takes it, and must name exactly the
 * block's stored entries (after coalescing), once each; wts[e] belongs to subs[e].  nnz = 0 with wts = NULL sets
 * alpha alone, with stored weights 1 (and no weight array: the footprint stays that of the mark).  The call marks the
 * block observed-only if it is not; aoadmm_tensor_set_observed_only(p, 0) and any upload drop the weights,
 * aoadmm_tensor_set_observed_only(p, 1) on a weighted block keeps them.  Resident with a weight list: N (4 N + 24) bytes
 * per nonzero plus the snapshots.  aoadmm_resident_em_step returns its three numbers under these definitions.
 * Weights above 1 are the caller's to normalise: divide W by its maximum, which scales the block's objective by that
 * maximum (fold it into Z.weights(p)).  Small alpha and small w slow EM down: its rate follows the share of the
 * information that is imputed.
 * AOADMM_ERR_INVALID, block untouched: a weight or alpha outside [0, 1] or not finite; a duplicate, an unstored or an
 * out-of-range subscript, a stored entry the list leaves out; nnz other than the block's count of stored entries.
 * AOADMM_ERR_UNSUPPORTED: a dense block, a PARAFAC2 block, a block uploaded with aoadmm_tensor_upload_coo_sharded and a
 * multi-device context.  No float atomics: two runs return the same bits. */
int aoadmm_tensor_set_entry_weights(aoadmm_ctx* ctx, int p, int64_t nnz, const int64_t* subs, const double* wts,
                                    double unstored_weight);
/* One EM step of an observed-only block with the current factors: the residuals x - m of the stored entries, then the
 * snapshot of the factors.  stats = {sum over the stored entries of (x - m)^2, num, den} with num / den the squared
 * norms of the change of the missing entries and of their old values (:436-440); the first step after the mark or a
 * solve has den = 0 and num = the squared norm of the model outside the stored entries.  Afterwards
 * aoadmm_resident_mttkrp on the block returns the MTTKRP of the imputed tensor as of this step (before any step: the
 * plain sparse MTTKRP, bit for bit). */
int aoadmm_resident_em_step(aoadmm_ctx* ctx, int p, double stats[3]);
/* One EM pass over the dense block p that holds a mask (aoadmm_tensor_mask_upload / aoadmm_par2_slab_mask_upload) or
 * weights (aoadmm_tensor_weights_upload; see the end of this comment) with
 * the current AOADMM_F_FAC state, exactly as aoadmm_solve runs it (cmtf_fun_AOADMM.m:408-441, :1224-1226): update = 0
 * leaves the data alone (the pass behind the start objective and Znorm_const), update = 1 also overwrites the missing
 * entries with the model.  fuse selects the partial contraction an update pass over a 3-way CP block leaves for the
 * next outer iteration: 0 none (a solve's last iteration), 1 the solver's own choice, 2 the second mode whenever
 * allowed; the library fuses only where a solve would (rank <= 24, not a block its one-launch MTTKRP serves).
 * stats = {num, den, obs_res, obs_x2}: the squared change of the missing entries, the squared norm of their old
 * values, and the squared residual and squared norm of the observed entries.  Returned when not NULL: data = the block
 * after the pass, unpadded, column-major, as doubles (a PARAFAC2 block: its slabs back to back); data_t = the
 * transposed copy a matrix block keeps (J x I); mttkrp = when the pass fused a contraction, the unweighted MTTKRP of
 * the first mode the model updates (I_n x R), finished from the partial contraction the pass left, with no further
 * tensor pass; info[0..7] = {rows per thread 4 / 2 / 1, rank class of the kernel, contracted tensor mode of the fused
 * pass (0-based: 1 or 2) or -1, mode the strips walk (1: second, 2: third), strips, pieces of the walk, walk positions
 * per piece, tensor mode of `mttkrp` or -1}; all zero but info[2] = info[7] = -1 for a PARAFAC2 block.  Two calls on
 * the same data return the same bits.  AOADMM_ERR_INVALID for a sparse or fp16 block and for one that is neither masked nor
 * weighted; AOADMM_ERR_UNSUPPORTED on a context that belongs to a communicator or drives several devices.
 *   A weighted block: stats = {||(1 - W) o M - Q||^2, ||Q||^2, sum W o (X - M)^2, sum W o X^2} with Q = Xhat - W o X
 * before the pass (0 after the upload and at the start of a solve), data = Xhat after the pass (data_t for a matrix), fuse
 * is ignored (a weighted pass fuses no contraction), info[2] = info[7] = -1 and the other fields describe the unfused
 * launch. */
int aoadmm_resident_em_pass(aoadmm_ctx* ctx, int p, int update, int fuse, double stats[4], double* data, double* data_t,
                            double* mttkrp, int64_t info[8]);
/* Marks (on != 0) the masked dense CP block p: the library builds, on the device, the list of its missing entries in
 * ascending storage order (column-major, first mode fastest) from the resident mask, and every imputing EM pass of the
 * block (aoadmm_solve, the re-imputation of aoadmm_heldout_restore_best) then evaluates the model at the listed entries
 * only and scatters it into the array, instead of passing over the whole block with a fused contraction.  Opt-in: an
 * unmarked block launches what it always did.  The statistics-only pass behind the start objective and Znorm_const stays
 * the dense one, so a marked block's iteration-0 objective is bit for bit the unmarked one.  Later objective values of
 * the block are formed as  (obs_x2 + den) - 2 <Xhat, M> + ||M||^2 - num  from the last MTTKRP of the iteration, as an
 * unmasked block's are, clamped at 0: they carry that form's absolute floor of about u * ||Xhat||^2 (u the fp64 unit
 * roundoff), where an unmarked block's directly summed residual has none.  A noise-free fit to machine precision
 * belongs on an unmarked block.  Resident: 4 N bytes per missing entry plus 16 bytes per 256 of them
 * (aoadmm_tensor_storage_info counts them); no cap on the missing share: AOADMM_ERR_NOMEM when the list does not fit,
 * with the block as it was.  on = 0 releases the list and the mark; so does any later upload of the block's data, mask
 * or weights.  AOADMM_ERR_UNSUPPORTED for a PARAFAC2, sparse or weighted block, on a context whose communicator has
 * more than one rank and on a multi-device context; AOADMM_ERR_INVALID for a block without a mask. */
int aoadmm_tensor_set_missing_list(aoadmm_ctx* ctx, int p, int on);
/* The list of the marked block p: *n (may be NULL) = its entries; subs (may be NULL) = their 0-based subscripts,
 * column-major n x N (mode m of entry e at subs[m * n + e]), in list order.  AOADMM_ERR_INVALID for an unmarked block. */
int aoadmm_tensor_missing_list(aoadmm_ctx* ctx, int p, int64_t* n, int64_t* subs_or_null);
/* One list pass over the marked block p with the current AOADMM_F_FAC state, exactly as aoadmm_solve enqueues it:
 * per listed entry m = sum_r prod_n F_n(s_n, r) in fp64, stats2 = {num, den} = {sum (m - x_old)^2, sum x_old^2} over
 * the list, and with update != 0 x <- m rounded once to the block's precision (a matrix block: in its transposed copy
 * too).  Observed entries are never touched.  Returned when not NULL: data = the block after the pass, unpadded,
 * column-major, as doubles; data_t = the transposed copy a matrix block keeps (J x I).  An empty list launches nothing
 * and returns two zeros.  Two calls on the same data return the same bits.  Timed under aoadmm_kernel_stats class 16.
 * AOADMM_ERR_INVALID for an unmarked block; AOADMM_ERR_UNSUPPORTED on a context that belongs to a communicator or
 * drives several devices.  (aoadmm_resident_em_pass with update != 0 on a marked block is AOADMM_ERR_UNSUPPORTED; with
 * update = 0 it is the dense statistics pass, as in a solve.) */
int aoadmm_resident_em_list_pass(aoadmm_ctx* ctx, int p, int update, double stats2[2], double* data, double* data_t);
/* Z.object{p}{k} of a PARAFAC2 block as sparse matrices, all K slabs in one call: nnz nonzeros, subs column-major
 * nnz x 3, 0-based (i, j within the slab, k); vals nnz doubles.  Duplicates are summed, explicit zeros are allowed,
 * nnz = 0 is valid; a subscript out of range (j >= J_k included) or nnz < 0 is AOADMM_ERR_INVALID and leaves the block
 * as it was.  Values stay fp64.  No array of size I x sum(J_k) or K x I x R exists for such a block.  A later
 * aoadmm_par2_slab_upload(..., AOADMM_ALL_SLABS, ...) replaces the sparse form and this call replaces a dense one.
 * On a block with sparse slabs aoadmm_par2_slab_mask_upload and a single-slab aoadmm_par2_slab_upload return
 * AOADMM_ERR_INVALID and aoadmm_resident_unfold_gram AOADMM_ERR_UNSUPPORTED; aoadmm_tensor_normsq and aoadmm_solve
 * work as for dense slabs.  With a communicator every rank holds all nonzeros, the block issues no collective and
 * aoadmm_options.par2_slab_sharding is ignored for it. */
int aoadmm_par2_slab_upload_coo(aoadmm_ctx* ctx, int p, int64_t nnz, const int64_t* subs, const double* vals);
/* Znorm_const{p} (cmtf_AOADMM.m:130-156) */
int aoadmm_tensor_normsq(aoadmm_ctx* ctx, int p, double* out);
/* How tensor p is stored on the device (each output may be NULL): *precision = the AOADMM_PREC_* its passes stream
 * (AOADMM_PREC_F64 for sparse and PARAFAC2 data), *scale = the power-of-two scale s of an AOADMM_PREC_F16 block (1.0
 * otherwise), *resident_bytes = what a CP block holds now: natural-layout array, pass copies, transposed copy and
 * mask of a dense block, and the list of a block marked with aoadmm_tensor_set_missing_list; the per-mode copies of the nonzeros of a sparse block, N (4 N + 8) bytes per nonzero this
 * rank holds (all of them, or its share of a sharded block; a multi-device context reports rank 0's), for an
 * observed-only block N (4 N + 16) per nonzero plus the factor snapshots (2 * 8 * I_n * R bytes per mode); 0 for
 * PARAFAC2 data.  No device work. */
int aoadmm_tensor_storage_info(aoadmm_ctx* ctx, int p, int* precision, double* scale, int64_t* resident_bytes);
/* *rank = the number of components R of block p, the columns of its factors: what a caller sizes the outputs of
 * aoadmm_resident_fold_in and the W of aoadmm_resident_topk_w by.  Needs aoadmm_model_end; no device work. */
int aoadmm_tensor_rank(aoadmm_ctx* ctx, int p, int* rank);

/* ---- held-out entries ---------------------------- */
/* The model of block p for the current AOADMM_F_FAC state at n subscripts: out[e] = sum_r prod_m F_m(s_m, r) for a CP
 * block, sum_r A(i, r) B_k(j, r) C(k, r) for a PARAFAC2 block with subscripts (i, j within slab k, k).  subs is
 * column-major n x n_tensor_modes, 0-based, the layout aoadmm_tensor_upload_coo takes; out is n doubles on the host, in
 * the caller's order.  Needs a finished model (aoadmm_model_end) and the factors of the block's modes
 * (aoadmm_state_set); the block need not hold data.  A subscript out of range (j >= J_k included) or a missing factor
 * is AOADMM_ERR_INVALID; n = 0 does nothing.  Only factors are read, so the answer is the same for dense, sparse,
 * sharded and row-sharded blocks and on every rank of a communicator (no collective).  No array of the tensor's size
 * exists.  Bitwise reproducible. */
int aoadmm_resident_model_at(aoadmm_ctx* ctx, int p, int64_t n, const int64_t* subs, double* out);
/* Attaches (n > 0) or removes (n = 0) the HELD-OUT LIST of block p: n entries (subs as above, vals n doubles) that were
 * kept out of the fit.  Duplicates are allowed and each is scored; whether an entry is also stored in the block's data
 * is the caller's business (documented, not checked).  A subscript out of range or a value that is not finite is
 * AOADMM_ERR_INVALID and the previous list stays.  Resident: 4 N + 8 bytes per entry (int32 subscripts, fp64 value), in
 * the caller's order; aoadmm_tensor_storage_info does not count them (aoadmm_heldout_info does).  The list belongs to
 * the MODEL: aoadmm_model_begin drops it, a new upload of the block's data keeps it.  With a list attached every
 * evaluation of the objective inside aoadmm_solve (the starting point included) also scores the list against the
 * factors that evaluation uses; the sums travel in the solve's one read-back per outer iteration and are kept as a
 * trace (aoadmm_heldout_trace).  Nothing else the solve computes changes: factors, duals, innerIters and the objective
 * traces are bit for bit those of the solve without a list.  With a communicator every rank attaches the same list
 * and does the same work (no collective, bit-identical ranks); a PARAFAC2 block with a list is never slab-sharded
 * (aoadmm_options.par2_slab_sharding is ignored for it). */
int aoadmm_tensor_set_heldout(aoadmm_ctx* ctx, int p, int64_t n, const int64_t* subs, const double* vals);
/* stats = {sum (y - m)^2, sum y^2, sum m^2, n as a double} of block p's list for the current factors, outside a solve
 * (relative error sqrt(stats[0] / stats[1]), RMSE sqrt(stats[0] / stats[3])).  AOADMM_ERR_INVALID without a list. */
int aoadmm_resident_heldout_stats(aoadmm_ctx* ctx, int p, double stats[4]);
/* *n = entries of block p's list (0: none), *resident_bytes = n (4 N + 8), *row_major = what the block's last held-out
 * pass (aoadmm_resident_model_at, aoadmm_resident_heldout_stats or inside a solve) gathered from: 1 the row-major
 * factor copies the Gram kernel leaves (current inside a solve), 0 the column-major factors (after aoadmm_state_set),
 * -1 no pass yet.  Each output may be NULL.  No device work. */
int aoadmm_heldout_info(aoadmm_ctx* ctx, int p, int64_t* n, int64_t* resident_bytes, int* row_major);
/* After aoadmm_solve: out[i] = sum (y - m)^2 of block p's list at iteration i = 0 .. OuterIterations (at most cap
 * entries are written), *len = OuterIterations + 1 (0 when the block had no list), *best_iter = the iteration at which
 * H_i = sum over the blocks with a list of w_p * sum (y - m)^2 was smallest (the first such; -1 without a list).  The
 * factors a solve returns are those of its LAST iteration; aoadmm_heldout_keep_best / aoadmm_heldout_restore_best bring
 * the best iterate back (without them a second solve from the same state with MaxOuterIters = *best_iter returns it: the
 * solve is bit-reproducible).  Each output may be NULL.
 * aoadmm_resident_model_at, aoadmm_tensor_set_heldout and aoadmm_resident_heldout_stats answer AOADMM_ERR_UNSUPPORTED
 * on a multi-device context (aoadmm_create_multi with more than one device). */
int aoadmm_heldout_trace(aoadmm_ctx* ctx, int p, double* out, int cap, int* len, int* best_iter);
/* on = 1: every later aoadmm_solve keeps, on the device, a copy of the complete solver state -- every field
 * aoadmm_state_get can return -- of the iteration at which H_i (aoadmm_heldout_trace) was smallest so far.  Iteration
 * 0 is the starting point and the comparison is strict: the earliest minimum wins, the rule of *best_iter.  The copy is
 * ONE kernel launch over a table of the state arrays whenever H improved (one hipMemcpyAsync per array would cost more
 * than a small model's outer iteration); it follows the read-back the host already waits for, so no synchronisation
 * is added.  The solve itself does not change: its state on return, its traces, exit_code and result scalars are those
 * of the LAST iteration, bit for bit, with the switch on or off.  on = 0 releases the copy; any other value is
 * AOADMM_ERR_INVALID.  The switch belongs to the MODEL, as the lists do: aoadmm_model_begin clears it.  A solve with
 * the switch on and no list attached is AOADMM_ERR_INVALID before any work.  Costs the state's bytes once more in HBM.
 * With aoadmm_rank_track(criterion = 1) the copy follows the best ranking score S instead of the smallest H, and the
 * list the solve needs is a ranking list (aoadmm_tensor_set_ranklist). */
int aoadmm_heldout_keep_best(aoadmm_ctx* ctx, int on);
/* Copies the kept state back into the engine's state and reports its iteration in *iter (may be NULL).  Afterwards the
 * engine is where a solve of *iter iterations from the same start would have left it: what is derived from the factors
 * (Gram matrices, row-major copies, the cached tensor pass, the B_k Gram matrices and the Y cache of sparse slabs) is
 * invalidated as aoadmm_state_set invalidates it, and the imputed entries of a block with Z.miss are brought to the
 * restored factors' model by one imputation pass (*iter = 0 took no EM step: the entries then stay as the last iteration
 * left them; an observed-only block starts every solve from zeros and needs nothing).  The kept copy survives the call:
 * a second call returns the same.  It is invalidated by the next aoadmm_solve, by any aoadmm_state_set and by
 * aoadmm_model_begin; AOADMM_ERR_INVALID when nothing is kept.  With a communicator every rank makes the call (a block
 * with Z.miss all-reduces its statistics; a slab-sharded PARAFAC2 block keeps and restores each rank's own slabs and
 * ends with the gather that ends a solve).  Both entries answer AOADMM_ERR_UNSUPPORTED on a multi-device context
 * (aoadmm_create_multi with more than one device). */
int aoadmm_heldout_restore_best(aoadmm_ctx* ctx, int* iter);
/* *have = 1 when a kept state can be restored, *iter = its iteration (-1: none), *launches = snapshot launches of the
 * last solve (one per iteration at which H improved, iteration 0 included), *bytes = the bytes those launches read and
 * wrote (launches * 2 * the state's bytes).  Each output may be NULL.  No device work. */
int aoadmm_heldout_best_info(aoadmm_ctx* ctx, int* have, int* iter, int64_t* bytes, int64_t* launches);

/* ---- top-k completions --------------------------- */
/* The k best entries of CP block p along its mode `mode` (0-based position in the block) for nq queries, from the
 * current AOADMM_F_FAC state.  Query q names a subscript for every other mode; w_q(r) = prod_{m != mode} F_m(s_{q,m}, r),
 * score_q(i) = sum_r F_mode(i, r) w_q(r) for 0 <= i < I_mode.  The candidates of q are the rows that are not in q's
 * exclusion list and whose score is not NaN; the answer is the k candidates that come first in the total order "larger
 * score first, equal scores by smaller row", idx[q * k + j] and val[q * k + j] for j = 0 .. k - 1, padded with row -1
 * and score -inf when fewer than k candidates exist.  subs is column-major nq x n_tensor_modes, 0-based, as for
 * aoadmm_resident_model_at; its column `mode` is neither read nor range-checked.  excl_off holds nq + 1 offsets into
 * excl_idx, the excluded rows per query in any order, repeats allowed; excl_off = NULL: no exclusions.  nq = 0 does
 * nothing.  AOADMM_ERR_INVALID, with idx and val untouched, for: mode outside the block, k outside [1, 64], nq < 0 or
 * nq >= 2^31, a subscript or an excluded row out of range, offsets that do not start at 0 or decrease.
 * AOADMM_ERR_UNSUPPORTED for a PARAFAC2 block and on a multi-device context (aoadmm_create_multi with more than one
 * device).  Like aoadmm_resident_model_at it reads factors only: the answer is the same for dense, fp16, masked,
 * sparse, observed-only, sharded and row-sharded blocks, and there is no collective, so the ranks of a communicator
 * may ask different queries.  The I_mode x nq score array never exists: device workspace O(nq R + nq k slabs).  The
 * summation order of a score depends on R alone, so the answer's bits are a function of the inputs only. */
int aoadmm_resident_topk(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const int64_t* subs, int k, const int64_t* excl_off,
                         const int64_t* excl_idx, int64_t* idx, double* val);
/* aoadmm_resident_topk with the weights given instead of formed from subscripts: W is nq x R column-major, row q is w_q,
 * uploaded as it is (finite or not; a NaN score is no candidate, by the rule above).  This is how a row that
 * aoadmm_resident_fold_in returned is ranked: for a block of order 2 the folded rows ARE the weights along the other
 * mode; for a higher order multiply them by the remaining modes' rows.  Everything else -- the order, the exclusions,
 * the padding, the refusals, the kernels that score and select -- is that of aoadmm_resident_topk. */
int aoadmm_resident_topk_w(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const double* W, int k, const int64_t* excl_off,
                           const int64_t* excl_idx, int64_t* idx, double* val);

/* ---- ranks of held-out entries -------------------- */
/* Where a known row stands among the candidates of aoadmm_resident_topk: the integer that hit-rate@k, NDCG@k, MRR and
 * AUC follow from.  subs is column-major nq x n_tensor_modes, 0-based, as for aoadmm_resident_topk, except that column
 * `mode` IS read and range-checked: it holds the target row t_q.  w_q and score_q(i) are those of aoadmm_resident_topk
 * bit for bit (the same products, the same chain of MFMAs).  The candidates of q are the rows whose score is not NaN
 * and that are not in q's exclusion list -- and, unlike top-k, the target itself whenever its score is not NaN: listing
 * it is ignored, so the stored rows of the whole tensor can be passed as they are.
 *   score[q] = score_q(t_q)
 *   rank[q]  = the number of candidates c != t_q with score_q(c) > score[q], or score_q(c) == score[q] and c < t_q: the
 *              0-based place of t_q in top-k's total order; -1 when score[q] is NaN
 *   ncand[q] = the number of candidates, also when rank[q] = -1 (ncand may be NULL)
 * excl_off / excl_idx follow top-k's rules (any order, repeats allowed -- a repeated row counts once --, NULL: none).
 * nq = 0 does nothing.  AOADMM_ERR_INVALID, with every output untouched, for: p or mode outside the model, nq < 0 or
 * nq >= 2^31, a subscript or an excluded row out of range, offsets that do not start at 0 or decrease, NULL rank or
 * score.  AOADMM_ERR_UNSUPPORTED for a PARAFAC2 block and on a multi-device context (aoadmm_create_multi with more than
 * one device).  Like aoadmm_resident_topk it reads factors only: the same answer for every kind of block, no
 * collective, the ranks of a communicator may ask different queries.  The I_mode x nq score array never exists: device
 * workspace 8 nq R + 8 nq + 8 nq_pad slabs bytes and 8 bytes per 1024 excluded rows.  Integer counts of scores whose
 * summation order depends on R alone: the answer's bits are a function of the inputs only. */
int aoadmm_resident_rank_of(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off,
                            const int64_t* excl_idx, int64_t* rank, double* score, int64_t* ncand_or_null);
/* aoadmm_resident_rank_of with the weights given: W is nq x R column-major, row q is w_q, uploaded as it is, and
 * targets[q] in [0, I_mode) is t_q (out of range: AOADMM_ERR_INVALID).  This is how a row that aoadmm_resident_fold_in
 * returned is ranked; see aoadmm_resident_topk_w for the weights of a block of higher order. */
int aoadmm_resident_rank_of_w(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const double* W, const int64_t* targets,
                              const int64_t* excl_off, const int64_t* excl_idx, int64_t* rank, double* score,
                              int64_t* ncand_or_null);

/* ---- Tucker projection and core consistency ------- */
/* core (r[0] x r[1] x r[2], column-major) = X x_1 M[0]' x_2 M[1]' x_3 M[2]' of the resident 3-way block p;
 * M[n] is dims[n] x r[n] column-major with leading dimension ld[n], host memory.  X is the block as it stands on the
 * device, whatever is resident of it: the natural array, the pass copies alone after the natural array was released,
 * the half copies of an AOADMM_PREC_F16 block (q / scale), the imputed array Xhat of a block with a mask or per-entry
 * weights (after a solve or an EM pass; a mask whose missing entries were never imputed is AOADMM_ERR_INVALID), or the
 * nonzeros of a plain sparse block (unstored entries are zero).  Dense: one tensor pass with M[c] in place of factor c
 * (c the mode with the largest dims[c] / r[c] the block can contract) and one fold over its result that reads it once;
 * sparse: with a the mode of the largest r[a], max(r[b], r[c]) MTTKRPs of mode a over the nonzeros and a fold of each
 * (workspace: I_a x max(r[b], r[c]) doubles and the fold's partial sums).  No float atomics and fixed summation orders: two calls return the same bits.  Nothing of the solver's state
 * moves: a solve after the call returns the bits of the solve without it.  Kernel statistics: the pass under which = 0 /
 * 1, the fold under which = 2, the sparse MTTKRPs under which = 3.
 * AOADMM_ERR_INVALID, with core untouched, for: p outside the model, a block without data, r[n] outside 1..64, NULL M,
 * M[n], ld, r or core, ld[n] smaller than dims[n].  AOADMM_ERR_UNSUPPORTED, with core and the block untouched, for: a
 * block that is not 3-way, a PARAFAC2 block, a sparse block fitted on its stored entries only or under entry weights (its
 * Xhat has no array), a sharded block (dense or sparse), any engine of a communicator with more than one rank, and a
 * multi-device context (aoadmm_create_multi with more than one device). */
int aoadmm_resident_project(aoadmm_ctx* ctx, int p, const double* const* M, const int64_t* ld, const int* r, double* core);
/* Core consistency of block p's CP model with the current AOADMM_F_FAC state: M[n] = F_n (F_n'F_n)^+ , core as above
 * (R x R x R, may be NULL), *cc = 100 (1 - sum (core - superdiagonal ones)^2 / R) (CORCONDIA, Bro & Kiers 2003: near 100
 * the data are trilinear at this R, far below -- it has no lower bound -- R is too large).  The factors are downloaded and
 * the pseudo-inverses formed on the host from the eigendecomposition of the R x R Gram matrices; eigenvalues below
 * R 2^-52 lambda_max count as zero and set *rank_deficient (may be NULL) to 1, else it is 0.  Refusals and block states
 * are those of aoadmm_resident_project; also AOADMM_ERR_INVALID for NULL cc or a missing factor.  Every output is
 * written last: an error leaves all three untouched. */
int aoadmm_resident_core_consistency(aoadmm_ctx* ctx, int p, double* cc, double* core_or_null, int* rank_deficient_or_null);

/* ---- ranking metrics tracked inside a solve ------- */
/* the metric aoadmm_rank_track follows; also the order of the float sums in aoadmm_rank_trace */
enum {
  AOADMM_RANK_HIT = 0,    /* hit-rate@k: the share of queries with rank < k */
  AOADMM_RANK_NDCG = 1,   /* NDCG@k: the mean of 1 / log2(rank + 2) where rank < k, else 0 */
  AOADMM_RANK_MRR = 2,    /* the mean of 1 / (rank + 1) */
  AOADMM_RANK_AUC = 3     /* the mean of 1 - rank / (ncand - 1) over the queries with ncand >= 2 */
};
/* the quantities of aoadmm_rank_trace and the slots of aoadmm_op_rank_metrics: sums, not means; counts are doubles
 * that hold integers */
enum {
  AOADMM_RANKSUM_N = 0,       /* queries with rank >= 0 */
  AOADMM_RANKSUM_N_AUC = 1,   /* those of them with ncand >= 2 */
  AOADMM_RANKSUM_HITS = 2,    /* #{rank < k} */
  AOADMM_RANKSUM_NDCG = 3,    /* sum over rank < k of 1 / log2(rank + 2) */
  AOADMM_RANKSUM_MRR = 4,     /* sum of 1 / (rank + 1) */
  AOADMM_RANKSUM_AUC = 5,     /* sum over the N_AUC queries of 1 - rank / (ncand - 1) */
  AOADMM_RANKSUM_COUNT = 6    /* slots 6 and 7 of an out[8] are spare and zero */
};
/* Attaches (nq > 0) or removes (nq = 0) the RANKING LIST of CP block p: nq queries with one target row each along mode
 * `mode`, and their exclusion lists.  Arguments and validation are exactly those of aoadmm_resident_rank_of (column
 * `mode` of subs is the target; lists in any order, repeats allowed, NULL: none); an error leaves the previous list
 * untouched.  The call does once what aoadmm_resident_rank_of does per call -- range checks, per-query sort and removal
 * of repeats, the chunk table -- uploads the result and allocates the rank pass's workspace and the three per-query
 * output arrays: an evaluation inside a solve allocates nothing, uploads nothing and touches no host memory.  The list
 * belongs to the MODEL, as a held-out list does: aoadmm_model_begin drops it, a new upload of the block's data keeps it.
 * One list per block.  With a list attached, aoadmm_solve evaluates it at iteration 0 and at every iteration i with
 * i % every == 0 (aoadmm_rank_track) beside the objective: the launches of aoadmm_resident_rank_of against the factors
 * that evaluation uses, then two launches that reduce rank and ncand to the AOADMM_RANKSUM_* sums, which travel in the
 * solve's one read-back per outer iteration.  Nothing else the solve computes changes: factors, duals, innerIters, the
 * objective and held-out traces and every kernel-statistics class but 13 are bit for bit those of the solve without a
 * list; class 13 counts one launch per list and evaluation.  With a communicator every rank attaches the same list and
 * does the same work (no collective, bit-identical ranks, so every rank takes the same decision).
 * AOADMM_ERR_UNSUPPORTED for a PARAFAC2 block and on a multi-device context (aoadmm_create_multi with more than one
 * device). */
int aoadmm_tensor_set_ranklist(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off,
                               const int64_t* excl_idx);
/* *nq = queries of block p's ranking list (0: none), *mode = its target mode (-1: none), *listed_after_dedup = excluded
 * rows kept after the per-query removal of repeats, *resident_bytes = device bytes of the list, the workspace and the
 * outputs.  Each output may be NULL.  No device work. */
int aoadmm_ranklist_info(aoadmm_ctx* ctx, int p, int64_t* nq, int* mode, int64_t* listed_after_dedup, int64_t* resident_bytes);
/* What a solve does with the ranking lists.  metric: AOADMM_RANK_*; k in [1, 2^31): the cut-off of hit-rate and NDCG;
 * every >= 1: the lists are evaluated at iteration 0 and at every iteration i with i % every == 0; patience >= 0;
 * criterion 0 or 1.  At an evaluation S is the pooled mean of the metric over all blocks with a list: the sum of their
 * sums over the sum of their N (N_AUC for AUC); block weights do not enter; 0 / 0 is NaN.  Larger is better: iteration 0
 * is the first best, a later evaluation becomes the best only if S is strictly larger; a NaN never does, and a NaN at
 * iteration 0 is replaced by the first S that is not NaN.  The best evaluation's iteration is reported by
 * aoadmm_rank_trace whatever the criterion.
 *   criterion = 0: trace only.  The held-out sum H, heldout_patience and aoadmm_heldout_keep_best work as without lists.
 *   criterion = 1: S is the solve's model-selection number.  patience = n > 0 stops the solve after the evaluation at
 *     which S has not improved for n consecutive EVALUATIONS (exit_code 3); aoadmm_heldout_keep_best keeps the state
 *     of the best S instead of the smallest H, and aoadmm_heldout_restore_best returns it.  aoadmm_solve answers
 *     AOADMM_ERR_INVALID before any work when no ranking list is attached or aoadmm_options.heldout_patience > 0.
 * patience > 0 with criterion = 0, or any argument out of range, is AOADMM_ERR_INVALID and the settings stay.  The
 * settings belong to the MODEL: aoadmm_model_begin restores the defaults (AOADMM_RANK_NDCG, 10, 1, 0, 0). */
int aoadmm_rank_track(aoadmm_ctx* ctx, int metric, int k, int every, int patience, int criterion);
/* After aoadmm_solve: out[e] = the sum `what` (AOADMM_RANKSUM_*) of block p's list at its e-th evaluation and iters[e]
 * (may be NULL) the iteration of that evaluation; at most cap entries each are written, *len = evaluations (0 when the
 * block had no list), *best_iter = the iteration of the best S (-1 without a list).  len and best_iter may be NULL.
 * No device work. */
int aoadmm_rank_trace(aoadmm_ctx* ctx, int p, int what, double* out, int cap, int* len, int* iters_or_null, int* best_iter);
/* rank, score and ncand (nq entries each; any may be NULL) of block p's list as its last evaluation left them on the
 * device: the outputs of aoadmm_resident_rank_of for the factors that evaluation used.  AOADMM_ERR_INVALID without a
 * list or before its first evaluation; AOADMM_ERR_UNSUPPORTED on a multi-device context. */
int aoadmm_ranklist_last(aoadmm_ctx* ctx, int p, int64_t* rank, double* score, int64_t* ncand);

/* ---- fold-in of new rows -------------------------- */
/* The factor rows of nq NEW indices ("queries": a new user, document, sample) along mode `mode` (0-based position in
 * the block) of CP block p, from their entries, with every other factor of the current AOADMM_F_FAC state held fixed:
 * the row update of the observed-only model.  subs is column-major nobs x n_tensor_modes, 0-based, as for
 * aoadmm_resident_model_at, except that column `mode` holds the query number q in [0, nq); vals holds one value per
 * observation (not checked for finiteness: a NaN reaches its own query's row only).  Any order; duplicates are separate
 * observations.  With z_e(r) = prod_{m != mode} F_m(s_{e,m}, r) (multiplied in mode order from 1) and, over the
 * observations of q in the caller's order, G_q = sum z_e z_e', b_q = sum x_e z_e (the block's weight is not applied; it
 * scales both sides):
 *   constraint = 0:  u_q = (G_q + ridge I)^-1 b_q by Cholesky;
 *   constraint = 1 (non-negativity): ADMM_constrained_only of the reference on the single row, cold-started: rho =
 *     trace(G_q) / R, L = chol(G_q + (ridge + rho / 2) I), z = mu = 0, then u = (b + rho / 2 (z - mu)) / (L L'),
 *     z_old = z, z = max(u + mu, 0), mu += u - z at least once and while iter < max_inner and ||u - z|| / ||u|| >
 *     tol_primal or ||z - z_old|| / ||mu|| > tol_dual (the latter unscaled when mu = 0); the test is per query and the
 *     row returned is z.
 * rows is nq x R column-major; info[q] = 0, or 1 when a pivot of the query's Cholesky was not positive (the row is
 * then NaN; the call still returns AOADMM_OK); iters[q] = ADMM iterations taken (0 without a constraint); gram holds
 * nq blocks of R x R (column-major, both triangles) and rhs nq x R column-major: G_q and b_q before the ridge.  The
 * last three may be NULL.  A query without observations gives the zero row when ridge > 0 and info 1 when ridge = 0.
 * opt = NULL: ridge 0, no constraint.  nq = 0 does nothing.
 * AOADMM_ERR_INVALID, with every output untouched, for: p or mode outside the model, nq < 0 or nq >= 2^31, nobs < 0, a
 * query number outside [0, nq), any other subscript out of range, ridge negative or not finite, constraint outside
 * {0, 1}, max_inner < 1, a negative tolerance, NULL subs / vals (with nobs > 0) / rows / info.  AOADMM_ERR_UNSUPPORTED
 * for a PARAFAC2 block and on a multi-device context (aoadmm_create_multi with more than one device).  Like
 * aoadmm_resident_model_at it reads factors only: the answer is the same for dense, fp16, masked, sparse,
 * observed-only, sharded and row-sharded blocks, and there is no collective, so the ranks of a communicator may ask
 * different things.  A query's outputs are a function of the factors, its own observations in the caller's order and
 * the options: not of nq, the other queries or their order. */
typedef struct {
  double ridge;
  int constraint;    /* 0: none, 1: non-negativity */
  int max_inner;
  double tol_primal;
  double tol_dual;
} aoadmm_foldin_options;
int aoadmm_resident_fold_in(aoadmm_ctx* ctx, int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals,
                            const aoadmm_foldin_options* opt_or_null, double* rows, int* info, int* iters_or_null,
                            double* gram_or_null, double* rhs_or_null);
/* aoadmm_resident_fold_in for a model fitted under entry weights and a weight for the unstored entries
 * (aoadmm_tensor_set_entry_weights): wts[e] in [0, 1] is the weight of observation e in the
 * caller's order (NULL: all ones) and unstored_weight = alpha in [0, 1] the weight of every cell of the new row that the
 * list does not name, where the data is 0.  Row q minimises sum_listed w_e (x_e - z_e'u)^2 + alpha sum_unlisted (z'u)^2 +
 * ridge |u|^2 with every other factor fixed, the fixed point of the weighted EM row by row.  With z_e as above and
 * H = had_{m != mode} F_m'F_m over ALL rows of the other modes' factors (computed inside the call, in a fixed order):
 *   G_q = sum_e (w_e - alpha) z_e z_e' + alpha H,   b_q = sum_e (w_e x_e) z_e
 * and then constraint 0 / 1, rho = trace(G_q) / R with alpha H included, info, iters, the pivot rule, the NaN row and the
 * exit are those of aoadmm_resident_fold_in; gram / rhs return G_q with alpha H included, before the ridge, and b_q.  Entry
 * (i, j) of the stored part with i <= j is the sum of ((w_e - alpha) z_e(i)) z_e(j) and defines (j, i); alpha H is added
 * once, as fma(alpha, H(i, j), .).  subs, vals, opt, the outputs and the role of mode are unchanged.
 * What follows from the form and is not special-cased: every listed observation contributes (w_e - alpha) z z', so a cell
 * listed twice is subtracted twice and with alpha > 0 the caller lists each cell once; a query without observations has
 * G_q = alpha H, b_q = 0 and gives the zero row with info 0 whenever alpha H + ridge I is positive definite; w_e - alpha
 * may be negative: G_q is positive semidefinite mathematically and what cancellation does at ridge 0 is reported through
 * info; a factor entry that is not finite reaches every query through H when alpha > 0, a value that is not finite only
 * its own query.
 * AOADMM_ERR_INVALID, before any output is written, for a weight or alpha outside [0, 1] or not finite (the convention of
 * aoadmm_tensor_set_entry_weights: the caller normalises and scales ridge with it), and for everything
 * aoadmm_resident_fold_in refuses, with the same codes (a PARAFAC2 block and a multi-device context:
 * AOADMM_ERR_UNSUPPORTED).  nq = 0 returns at once.  wts = NULL or all ones with alpha = 0 returns the bits of
 * aoadmm_resident_fold_in; the weighted kernels are instantiations of their own and aoadmm_resident_fold_in launches what
 * it always launched.  The block's own weight list is not read: the call stays data-less. */
int aoadmm_resident_fold_in_w(aoadmm_ctx* ctx, int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals,
                              const double* wts_or_null, double unstored_weight, const aoadmm_foldin_options* opt_or_null,
                              double* rows, int* info, int* iters_or_null, double* gram_or_null, double* rhs_or_null);

/* ---- fold-in of new slabs into a PARAFAC2 block ---- */
/* The rows of C of nk NEW slabs (a new sample, run, patient visit) of PARAFAC2 block p, with the fitted A = AOADMM_F_FAC
 * of the block's first mode (I x R) and DeltaB = AOADMM_F_DELTAB (R x R) held fixed and B_q = P_q DeltaB imposed exactly
 * (direct-fitting PARAFAC2).  X holds the slabs back to back, slab q is I x cols[q] column-major; cols[q] = J_q >= R.
 * With Y = X_q' A (J_q x R, the only pass over the data) and S = (A'A) .* (DeltaB'DeltaB) (once per call, fixed order), per
 * slab, starting from c = c0[q] (c0 is nk x R column-major; NULL: ones), at least once and at most max_iter times:
 *   W = Y diag(c) DeltaB';  P = U V' of svd(W, 'econ') by one-sided Jacobi (cmtf_fun_AOADMM.m:532-534);  B = P DeltaB;
 *   b(r) = sum_j Y(j, r) B(j, r);  c_old = c;
 *   constraint = 0:  c = (S + ridge I)^-1 b by Cholesky, factored once per call;
 *   constraint = 1 (non-negativity): the cold-started row loop of aoadmm_resident_fold_in on (S + ridge I, b): rho =
 *     trace(S) / R, L = chol(S + (ridge + rho / 2) I) once per call, z = mu = 0, u = (b + rho / 2 (z - mu)) / (L L'),
 *     z_old = z, z = max(u + mu, 0), mu += u - z at least once and while iter < max_inner and ||u - z|| / ||u|| > tol_primal
 *     or ||z - z_old|| / ||mu|| > tol_dual (unscaled when mu = 0); c = z;
 *   stop when ||c - c_old|| <= tol ||c||.
 * Then res[q] = ||X_q||^2 - 2 c'b + c'S c and xnorm[q] = ||X_q||^2.  With P'P = I the system of c does not depend on the
 * slab, which is why one factorisation serves the call.
 * Outputs: C nk x R column-major; B and P in the slab layout of the state fields (slab q at (sum_{q' < q} J_q') R, J_q x R
 * column-major); res, xnorm, iters (outer iterations taken), info: one per slab; Y in the slab layout; sys = S (R x R)
 * before the ridge; path[0] = AOADMM_P2FOLD_Y_* of the Y pass and path[1] = AOADMM_P2FOLD_ALT_* of the alternation.
 * B, P, xnorm, Y, sys and path may be NULL; so may c0 and opt (NULL: max_iter 50, tol 1e-8, ridge 0, no constraint).
 * info[q] = 1 when W lost a column in some iteration: its norm after the sweeps was exactly 0 (an all-zero slab is the
 * plainest case); the polar factor then has a zero column there and the row is still returned (a zero slab gives C = 0,
 * res = 0).  A failed pivot of the shared system returns AOADMM_ERR_NOT_PD with every output untouched.
 * AOADMM_ERR_INVALID, with every output untouched, for: p out of range or not a PARAFAC2 block, A or DeltaB never set,
 * nk < 0, J_q < R, J_q, sum J_q or R sum J_q beyond the int range, max_iter < 1, tol or ridge negative or not finite, every option
 * value aoadmm_resident_fold_in refuses, NULL cols / X / C / res / iters / info.  AOADMM_ERR_UNSUPPORTED on a multi-device
 * context (aoadmm_create_multi with more than one device).  nk = 0 returns at once.
 * Values are not checked for finiteness: a NaN reaches its own slab only.  The block's weight, B_k, P_k, C and its data are
 * not read: dense, sparse-slab, masked and slab-sharded blocks answer alike, there is no collective, and the ranks of a
 * communicator may ask different things.  A slab's outputs are a function of A, DeltaB, the slab, c0[q] and the options:
 * not of nk, the other slabs or their order.
 * The call takes the number of rows of every slab from the model: X must hold I sum J_q doubles with I =
 * aoadmm_par2_rows(p), which a caller that receives slabs from elsewhere checks first (Engine.par2_fold_in does).  A call
 * that fails counts nothing in kernel-statistics class 17. */
typedef struct {
  int max_iter;
  double tol;
  double ridge;
  int constraint;    /* 0: none, 1: non-negativity */
  int max_inner;
  double tol_primal;
  double tol_dual;
} aoadmm_par2_foldin_options;
/* path[0]: 2 (T - 1) + chunked, T = ceil(R / 16) factor tiles of 16 columns per wave; chunked: I > 4096 rows, the Y pass
 * cuts I into ceil(I / 4096) chunks (a number that depends on I alone) and adds their partials in chunk order */
enum {
  AOADMM_P2FOLD_Y_T1 = 0, AOADMM_P2FOLD_Y_T1_CHUNKED = 1, AOADMM_P2FOLD_Y_T2 = 2, AOADMM_P2FOLD_Y_T2_CHUNKED = 3,
  AOADMM_P2FOLD_Y_T3 = 4, AOADMM_P2FOLD_Y_T3_CHUNKED = 5, AOADMM_P2FOLD_Y_T4 = 6, AOADMM_P2FOLD_Y_T4_CHUNKED = 7
};
/* path[1]: Y_q and W of every slab in LDS (R^2 + 2 max(J_q) R doubles within 48 KB), or in a workspace */
enum { AOADMM_P2FOLD_ALT_LDS = 0, AOADMM_P2FOLD_ALT_WS = 1 };
/* *rows = I of PARAFAC2 block p, the number of rows of each of its slabs and of its first factor.  AOADMM_ERR_INVALID for
 * p out of range, a CP block or a NULL pointer.  No device work. */
int aoadmm_par2_rows(aoadmm_ctx* ctx, int p, int64_t* rows);
int aoadmm_resident_par2_fold_in(aoadmm_ctx* ctx, int p, int64_t nk, const int64_t* cols, const double* X, const double* c0_or_null,
                                 const aoadmm_par2_foldin_options* opt_or_null, double* C, double* B_or_null, double* P_or_null,
                                 double* res, double* xnorm_or_null, int* iters, int* info, double* Y_or_null, double* sys_or_null,
                                 int* path_or_null);

/* ---- state (the struct G) ---------------------------------------------- */
/* slab = k for cell-valued fields (PARAFAC2 B mode, P, mu_DeltaB), else 0.  slab = AOADMM_ALL_SLABS moves
 * all K cells at once: host holds them back to back, each J_k x R column-major, rows = sum J_k. */
int aoadmm_state_set(aoadmm_ctx* ctx, int field, int index, int slab, const double* host,
                     int64_t rows, int64_t cols);
int aoadmm_state_get(aoadmm_ctx* ctx, int field, int index, int slab, double* host, int64_t rows,
                     int64_t cols);

/* ---- solver level: cmtf_fun_AOADMM.m:1 ---------------------------------- */
int aoadmm_solve(aoadmm_ctx* ctx, const aoadmm_options* opt, aoadmm_result* out);
/* one bare MTTKRP on the resident tensor p against the current factors (bench leg);
 * result stays on the device; elapsed device time of the kernels is returned */
int aoadmm_resident_mttkrp(aoadmm_ctx* ctx, int p, int tensor_mode, double* out_host_or_null,
                           float* elapsed_ms);
/* PARAFAC2 block with sparse slabs: the UNWEIGHTED right-hand side of tensor mode 0 (I x R: sum_k X_k B_k D_k),
 * 1 (sum(J_k) x R, the slabs back to back as in the state fields: X_k' A D_k) or 2 (K x R: diag(A' X_k B_k)) against
 * the current factors, column-major; every call runs its pass over the nonzeros (operator tests, timing). */
int aoadmm_resident_par2_rhs(aoadmm_ctx* ctx, int p, int tensor_mode, double* out_host_or_null, float* elapsed_ms);
/* device time (ms, HIP events on the library's stream around the kernel only), launch count, algorithmic
 * bytes and flops of a tensor-pass kernel since the last reset.  which = 0: register-streaming contraction
 * (contract_f32/f64, trailing modes); which = 1: LDS-transposed leading-mode contraction (contract_lead_f32);
 * which = 2: the reductions over the partial contraction T that finish an MTTKRP (bytes = size of T per reduction;
 * timed only from the first call with which = 2 on, two more events per reduction); which = 3: the MTTKRPs of
 * sparse blocks (launches = MTTKRPs, each the streaming kernel plus its carry passes; bytes = nonzeros streamed +
 * factor rows gathered + output written; flops = nnz * R * N) and the passes over the nonzeros of PARAFAC2 blocks
 * with sparse slabs (one launch per pass, counted as the MTTKRP of the I x sum(J_k) matrix it is); an EM step of an
 * observed-only block counts as one launch with the bytes and flops of its N passes, and its MTTKRPs include the
 * dense correction; which = 4 + n (n = 0 .. 7): the pass of those EM steps over the copy of tensor mode n alone, and under which = 4 also the
 * pass of every aoadmm_resident_em_pass call over a dense CP block, masked or weighted (a solve's own EM passes record no events) (the
 * residuals x - m; n = 0 also carries the statistics, and is the whole of a statistics-only step).  Of a sharded
 * sparse block: this rank's share (its nonzeros, and the rows of its span as the output written); the all-reduce is
 * outside the events; which = 12: the held-out passes (aoadmm_resident_model_at, aoadmm_resident_heldout_stats and the pass
 * of every objective evaluation of a solve with a list attached: one launch each; bytes = subscripts and values streamed
 * + factor rows gathered, flops = n * R * N + 8 n for the sums); which = 13: aoadmm_resident_topk (one launch per call:
 * its weights, scores-and-selection and merge kernels inside one event pair; bytes = F_mode streamed once per query tile
 * + rows gathered + the answer, flops = 2 * I_mode * nq * R) and aoadmm_resident_rank_of / _w (one launch per call: every
 * kernel of the call inside one event pair; bytes = F_mode streamed once per query tile + the rows gathered for the
 * weights, the targets and the excluded rows + the answer, flops = 2 * I_mode * nq * R + 2 * R * (excluded rows after
 * repeats are dropped + nq)); which = 14: aoadmm_resident_fold_in (one launch per call: its
 * kernels inside one event pair; bytes = the list streamed + rows gathered + the outputs, flops = nobs * (R (R + 1) +
 * 2 R (N - 1)) + nq * (R^3 / 3 + 2 R^2) for the solves; aoadmm_resident_fold_in_w counts in the same class: with a weight
 * list 8 nobs bytes more, and with alpha > 0 the factor rows read for H, 8 R sum_{m != mode} I_m bytes, and its
 * R^2 sum_{m != mode} I_m flops); which = 16 (15 is not assigned and stays AOADMM_ERR_INVALID): the list pass of every aoadmm_resident_em_list_pass call (one launch per
 * call, the gather kernel and its finisher inside one event pair; a solve's own list passes record no events; bytes =
 * subscripts streamed + factor rows gathered + the value read and, with update = 1, written in the block's precision,
 * twice for a matrix; flops = n * R * N + 8 n for the sums); which = 17: aoadmm_resident_par2_fold_in (one launch per
 * call: its kernels inside one event pair; bytes = the slabs + A + the outputs Y, P, B, C, res, xnorm, iters, info; flops =
 * 2 I sum(J_q) R for Y + 9 R^2 J_q per slab and iteration taken: W, P, B and one sweep of rotations) */
int aoadmm_kernel_stats(aoadmm_ctx* ctx, int which, int reset, double* contract_ms, int64_t* contract_launches,
                        double* contract_bytes, double* contract_flops);

/* ---- op level (host in / host out) -------------------------------------- */
/* mttkrp(X,U,n): cmtf_fun_AOADMM.m:97, cp_func.m:47.  X dense, dims[ndims]; U[m] is dims[m] x R */
int aoadmm_op_mttkrp(aoadmm_ctx* ctx, const double* X, int ndims, const int64_t* dims,
                     const double* const* U, int R, int n, int precision, double* out);
/* Y = X_(n)*X_(n)' (dims[n] x dims[n]) of a dense matrix / 3-way tensor: the Gram matrix whose leading eigenvectors
 * initialise mode n when init_options.nvecs = 1 (cmtf_nvecs.m:40-58, init_coupled_AOADMM_CMTF.m:50-73; for a
 * PARAFAC2 block pass [X_1 ... X_K] with n = 0, or X_k with n = 1).  The eigenvectors are taken by the caller
 * (MATLAB `eigs`, numpy `eigh`). */
int aoadmm_op_unfold_gram(aoadmm_ctx* ctx, const double* X, int ndims, const int64_t* dims, int n, int precision,
                          double* out);
/* The same Gram matrix from the RESIDENT data of tensor p (uploaded or generated before): no second transfer of the
 * tensor for init_options.nvecs = 1 (cmtf_nvecs.m:31-56 unfolds the data it already holds).  CP blocks: tensor_mode
 * 0..2, slab ignored; PARAFAC2 blocks: tensor_mode 0 (all slabs side by side) or 1 (slab `slab`).  With a communicator
 * the partial sums of the row blocks are all-reduced; the first mode of a row-sharded block has no local answer:
 * AOADMM_ERR_UNSUPPORTED (use aoadmm_op_unfold_gram with the host array). */
int aoadmm_resident_unfold_gram(aoadmm_ctx* ctx, int p, int tensor_mode, int slab, double* out);
/* The r leading eigenvectors of X_(n) X_(n)' for the RESIDENT SPARSE data of tensor p: the start that
 * init_options.nvecs = 1 asks for (cmtf_nvecs.m:54-56) without the I_n x I_n Gram matrix, by block subspace iteration
 * with Rayleigh-Ritz on the nonzeros (two passes over them per iteration).
 *   Accepted: a sparse CP block (aoadmm_tensor_upload_coo), any tensor_mode, order 2..8; a PARAFAC2 block with sparse
 *   slabs (aoadmm_par2_slab_upload_coo), tensor_mode 0 (sum_k X_k X_k').  Dense data and tensor_mode 1, 2 of a
 *   PARAFAC2 block: AOADMM_ERR_UNSUPPORTED (dense data have aoadmm_resident_unfold_gram).  A block without nonzeros,
 *   r outside 1..min(I_n, 64) or ldU < I_n: AOADMM_ERR_INVALID.  Work arrays that do not fit the free device memory:
 *   AOADMM_ERR_NOMEM, before anything is launched.
 *   Options (null or zeros = defaults): oversample (8): the iterated block has b = min(I_n, 64, max(r, min(F, r +
 *   oversample))) columns, F the number of non-empty mode-n fibers, so the oversampling shrinks for r > 64 - oversample;
 *   max_iters (500); tol (1e-10) on the residual ||Y Q_r - V Q_r Theta_r||_F / theta_1 of the first r Ritz pairs;
 *   seed of the counter-based generator of the start block (deterministic, matches no host generator).
 *   U: I_n x r column-major with leading dimension ldU, columns by descending eigenvalue, each with its entry of
 *   largest magnitude positive (the first such entry on a tie); eigvals (optional): the r eigenvalues.  Not converged
 *   within max_iters is not an error: AOADMM_OK with info->converged = 0 and the last iterate.  Bitwise reproducible
 *   for a given seed.  With a communicator the block is replicated: every rank computes the same bits, no collective
 *   (a block uploaded with aoadmm_tensor_upload_coo_sharded: AOADMM_ERR_UNSUPPORTED). */
typedef struct { int oversample; int max_iters; double tol; uint64_t seed; } aoadmm_nvecs_options;
typedef struct { int iterations; int converged; int block; double residual; int64_t fibers; } aoadmm_nvecs_info;
int aoadmm_resident_nvecs(aoadmm_ctx* ctx, int p, int tensor_mode, int r, const aoadmm_nvecs_options* opt_or_null,
                          double* U, int64_t ldU, double* eigvals_or_null, aoadmm_nvecs_info* info_or_null);
/* G'*G : cmtf_fun_AOADMM.m:66,148 */
int aoadmm_op_gram(aoadmm_ctx* ctx, const double* F, int64_t rows, int R, double* out);
/* L = chol(B','lower') : cmtf_fun_AOADMM.m:142 ; AOADMM_ERR_NOT_PD on failure */
int aoadmm_op_chol(aoadmm_ctx* ctx, const double* B, int R, double* L);
/* prox handle built by constraints_to_prox.m, evaluated as prox(X,rho) */
int aoadmm_op_prox(aoadmm_ctx* ctx, int constraint, const double* params, int n_params,
                   const double* Lmat, const double* X, int64_t rows, int R, double rho, double* out);
/* ADMM_constrained_only (cmtf_fun_AOADMM.m:591-623) for one CP mode: A is the
 * MTTKRP (rows x R), Bsys the system matrix *before* +rho/2*I (line :141 is applied
 * inside), fac/Z/mu updated in place, inner iteration count returned. */
int aoadmm_op_admm_constrained(aoadmm_ctx* ctx, const double* A, const double* Bsys, double rho,
                               int constraint, const double* params, int n_params,
                               const double* Lmat, int64_t rows, int R, int max_inner,
                               double tol_pr, double tol_du, double* fac, double* Z, double* mu,
                               int* inner_iters);
/* Kernel family that ran an ADMM_constrained_only loop (reported by aoadmm_op_admm_mode).  The library picks it
 * from the shape, the constraint and max_inner alone. */
enum {
  AOADMM_PATH_WG = 0,             /* whole loop in one workgroup: rows <= 256, R <= 16 */
  AOADMM_PATH_MFMA = 1,           /* element-wise prox, two launches on the matrix cores */
  AOADMM_PATH_ROWS_FUSED = 2,     /* one launch per inner iteration, element-/row-wise prox inside */
  AOADMM_PATH_ROWS_COLPROX = 3,   /* primal kernel, column/matrix prox, dual kernel per inner iteration */
  AOADMM_PATH_ROWS_TV = 4,        /* primal kernel, TV prox with the dual update inside */
  AOADMM_PATH_ROWL = 5            /* triangular solves per row (aoadmm_op_admm_constrained only) */
};
/* The same loop as one constrained CP mode of aoadmm_solve runs it: C is the Hadamard product of the other modes'
 * Gram matrices (R x R); rho = trace(C)/R, L = chol(C + rho/2*I) and inv(L*L') are built on the device
 * (cmtf_fun_AOADMM.m:98-127,141-142 with weight 1), and the kernels are the ones the solver picks for this shape.
 * fac/Z/mu are updated in place.  Also returned (each may be NULL): the inner iteration count, res[0] / res[1] =
 * relative primal / dual residual of the last iteration (:1079-1096), gram = fac'*fac (R x R, :148),
 * fac_rowmajor = the row-major copy of fac the next tensor pass reads (rows x R), path = AOADMM_PATH_*. */
int aoadmm_op_admm_mode(aoadmm_ctx* ctx, const double* A, const double* C, int constraint,
                        const double* params, int n_params, const double* Lmat, int64_t rows, int R,
                        int max_inner, double tol_pr, double tol_du, double* fac, double* Z, double* mu,
                        int* inner_iters, double* res, double* gram, double* fac_rowmajor, int* path);
/* Kernels that run the B_k loop of a PARAFAC2 block (reported by aoadmm_op_par2_b_loop).  The library picks them from
 * R, the longest slab and whether the B_k constraint is active. */
enum {
  AOADMM_P2SLAB_REGS1 = 0,        /* slab in registers, one row per lane: R <= 4, max J_k <= 64 */
  AOADMM_P2SLAB_REGS2 = 1,        /* two rows per lane: max J_k <= 128 */
  AOADMM_P2SLAB_REGS4 = 2,        /* four rows per lane: max J_k <= 256 */
  AOADMM_P2SLAB_LDS4 = 3,         /* slab through LDS / global memory: R <= 4, longer slabs */
  AOADMM_P2SLAB_LDS8 = 4,         /* R in 5..8 */
  AOADMM_P2SLAB_LDS16 = 5,        /* R in 9..16 */
  AOADMM_P2SLAB_LDS64 = 6         /* R in 17..64 */
};
/* Mode B of a PARAFAC2 block as aoadmm_solve runs it from the right-hand side on (cmtf_fun_AOADMM.m:194-218 with
 * ADMM_B_Parafac2 :509-589), on K slabs of rows_k[k] rows: Ak = the slabs' right-hand sides w*X_k'*A*D_k back to back
 * (each rows_k[k] x R, column-major), GA = A'*A (R x R), C (K x R).  rho_k = rho_scale*trace(D_k GA D_k)/R and
 * L_k = chol(weight*D_k GA D_k + rho_k/2*(1 + constrained)*I) are built on the device; AOADMM_ERR_NOT_PD when one fails.
 * constraint = AOADMM_C_NONE: no B_k constraint (Z, muZ ignored, may be NULL).  tol = the four inner tolerances
 * {pr_coupl, pr_constr, du_coupl, du_constr}.  P, mu_DeltaB (slabs back to back), DeltaB (R x R) and, when constrained,
 * Z and muZ are updated in place; B receives the new B_k.  Also returned (each may be NULL): rho (K), L and
 * GB = B_k'*B_k ([K][R*R]), the inner iteration count, res[0..3] = the four residual means of the last iteration in
 * the order of tol, path[0..3] = {two-launch folded loop (1) or four launches (0), AOADMM_P2SLAB_*, slab staged in
 * LDS (1) or rotated in global memory (0), class of the folded dual kernel (16 / 64, 0 when not folded)}. */
int aoadmm_op_par2_b_loop(aoadmm_ctx* ctx, int K, const int64_t* rows_k, int R, const double* Ak, const double* GA,
                          const double* C, double weight, double rho_scale, int constraint, const double* params,
                          int n_params, int max_inner, const double* tol, double* P, double* mu_DeltaB,
                          double* DeltaB, double* Z, double* muZ, double* B, double* rho, double* L, double* GB,
                          int* inner_iters, double* res, int* path);
/* The three entries below run the steps of a dense PARAFAC2 block outside the B_k loop as aoadmm_solve runs them, on
 * host arrays and without a model: K slabs X_k (I x rows_k[k], column-major) back to back in X; B (and P, Z) = the
 * slab-valued factors back to back, slab k rows_k[k] x R column-major; A (I x R); C (K x R).  Each answers
 * AOADMM_ERR_UNSUPPORTED on a context that belongs to a communicator or drives several devices.
 *
 * Mode A (cmtf_fun_AOADMM.m:160-165): GB[k] = B_k'*B_k, T1[k] = X_k*B_k, Amt = sum_k T1[k]*D_k (the unweighted MTTKRP,
 * I x R), Csys = sum_k D_k GB[k] D_k (R x R), and Csys_only = the same Csys from the launch a block with sparse slabs
 * uses.  Every output may be NULL.  T1 is [K][I*R], GB [K][R*R].  path[0] / path[1] = tile width (4, 16 or 64 outputs per
 * workgroup) of the Amt + Csys launch / of the Csys-only launch; the library picks them from I*R + R*R and R*R. */
int aoadmm_op_par2_mode_a(aoadmm_ctx* ctx, int K, const int64_t* rows_k, int I, int R, const double* X, const double* B,
                          const double* C, double* T1, double* GB, double* Amt, double* Csys, double* Csys_only,
                          int* path);
/* What aoadmm_op_par2_mode_c builds (`system`) and the form its uncoupled update took (path[0]). */
enum {
  AOADMM_P2CSYS_UNCOUPLED = 0,    /* the uncoupled update: systems, then the row solve or the ADMM loop (:219-248) */
  AOADMM_P2CSYS_ROWS = 1,         /* coupled, types 0, 3, 4: chol(w*C_k + ... + rho_k/2*(1 + constrained)*I)  (:260-267) */
  AOADMM_P2CSYS_HHT = 2,          /* coupled, type 2: chol(... + rho_k/2*(H*H' + constrained*I))  (:305-312) */
  AOADMM_P2CSYS_DIAG = 3,         /* coupled, types 1, 5, H'*H = diag(d): chol(B_k + mean(rho)/2*(d_k + constrained)*I) */
  AOADMM_P2CSYS_DENSE = 4         /* coupled, types 1, 5: M = blkdiag(B_k) + mean(rho)/2*(kron(H'*H, I) + constrained*I) */
};
enum {
  AOADMM_P2C_SINGLE = 0,          /* unconstrained: one row solve (:236) */
  AOADMM_P2C_WG = 1,              /* whole ADMM loop in one workgroup, a row system per thread: K <= 256, R <= 16 */
  AOADMM_P2C_LAUNCHED = 2         /* row solve, constraint update and loop test launched per inner iteration */
};
/* Mode C (cmtf_fun_AOADMM.m:219-248, coupled systems :260-312).  A'*A, B_k'*B_k and X_k*B_k are formed on the device;
 * a(k,r) = weight*sum_i A(i,r)(X_k B_k)(i,r) + bsum_half*C(k,r), C_k = A'A .* B_k'B_k, rho_k = trace(C_k)/R,
 * B_k = weight*C_k + (ridge + bsum_half)*I.  constraint = AOADMM_C_NONE: unconstrained.
 * system = AOADMM_P2CSYS_UNCOUPLED: L_k = chol(B_k + constrained*rho_k/2*I); unconstrained, C(k,:) = a_k / (L_k L_k');
 * constrained, ADMM_constrained_only on the K row systems (:600-606) with max(rho) in the prox, from C / Z / mu (K x R,
 * updated in place) for at most max_inner iterations under tol = {pr_constr, du_constr}.
 * Other systems: only the builders run (C, Z, mu are not changed; max_inner and tol are ignored); `constrained` is
 * constraint != AOADMM_C_NONE; sysmat = H*H' (R x R), d (K) or H'*H (K x K) for systems 2, 3, 4.
 * Returned (each may be NULL): a (K x R); rho (K); L ([K][R*R]: the factors, the raw B_k for system 4);
 * rho_stats[0..2] = max, mean, sum of rho (the uncoupled update sets [0] only, and nothing when path[0] is
 * AOADMM_P2C_WG: that loop takes the maximum itself); M ((K*R) x (K*R), system 4, unknowns ordered k*R + r); the
 * inner iteration count (0 without a loop); res[0] / res[1] = relative primal / dual constraint residual of the last
 * iteration; path[0] = AOADMM_P2C_* (-1 for the coupled builders), path[1] = rank class of the row solve (4, 8, 16 or
 * 64).  AOADMM_ERR_NOT_PD when a factorisation fails. */
int aoadmm_op_par2_mode_c(aoadmm_ctx* ctx, int system, int K, const int64_t* rows_k, int I, int R, const double* X,
                          const double* A, const double* B, double weight, double ridge, double bsum_half,
                          int constraint, const double* params, int n_params, int max_inner, const double* tol,
                          const double* sysmat, double* C, double* Z, double* mu, double* a, double* rho, double* L,
                          double* rho_stats, double* M, int* inner_iters, double* res, int* path);
/* Objective pieces (cmtf_fun_AOADMM.m:1262-1264, :1355, :1337, :1279-1281): res[k] = ||X_k - A D_k B_k'||_F^2;
 * q[4k..4k+3] = ||B_k - P_k DeltaB||^2, ||B_k||^2, ||B_k - Z_k||^2 (0 when Z is NULL), ||B_k - B_{k-1}||^2 (0 for k = 0
 * and where the two slabs differ in size); regv[k] = reg_func(B_k) of regularisation type reg_type (an AOADMM_C_* with
 * a reg_func value other than the quadratic one; AOADMM_C_NONE: regv untouched, may be NULL) with parameter eta. */
int aoadmm_op_par2_objective(aoadmm_ctx* ctx, int K, const int64_t* rows_k, int I, int R, const double* X,
                             const double* A, const double* B, const double* C, const double* P, const double* DeltaB,
                             const double* Z, int reg_type, double eta, double* res, double* q, double* regv);
/* Form of the coupled ADMM loop (cmtf_fun_AOADMM.m:625-1075; reported by aoadmm_op_coupled_loop).  The library picks
 * it from the coupling type, the number of coupled modes, the rows and columns of Delta, the ranks and the constraints. */
enum {
  AOADMM_CPATH_REGS = 0,          /* types 0/4, whole loop in one workgroup, a row per thread in registers */
  AOADMM_CPATH_WG = 1,            /* types 0/4, whole loop in one workgroup through LDS / global memory */
  AOADMM_CPATH_ROWSTEPS = 2,      /* types 0/4, row kernels launched per step */
  AOADMM_CPATH_GENERIC = 3        /* any type: images, small products and solves launched per step */
};
/* The inner loop of coupling `coupling` of the current model as aoadmm_solve runs it once the MTTKRPs of its modes are
 * there (cmtf_fun_AOADMM.m:253-404 with ADMM_coupled :625-1075).  The model is declared with aoadmm_model_*; no tensor
 * data is needed.  A[j] (rows_j x R_j) is the MTTKRP and C[j] (R_j x R_j) the Hadamard product of the other modes' Gram
 * matrices, block weight applied, of the coupling's j-th mode (modes in ascending order).  Per mode rho = trace(C)/R and
 * the system matrix C [+ Z.ridge] + rho/2*(I, twice if constrained: types 0, 3, 4 | H*H' + I if constrained: type 2)
 * with its Cholesky factor, or its eigenvectors for the Sylvester solve (types 1, 5), are built on the device;
 * AOADMM_ERR_NOT_PD when a factorisation fails.  The state is read from and left in the context (aoadmm_state_set /
 * aoadmm_state_get: FAC, CONSTRAINT_FAC, CONSTRAINT_DUAL, COUPLING_DUAL of the modes, COUPLING_FAC of the coupling).
 * tol = the four inner tolerances {pr_coupl, pr_constr, du_coupl, du_constr}.  Returned (each may be NULL): the inner
 * iteration count; res[0..3] = the four residual means of the last iteration in the order of tol; rho[j]; L[j] and
 * gram[j] = fac'*fac (arrays of pointers, R_j x R_j each); slots[8*j..8*j+7] = the squared norms behind the residuals
 * of mode j {|fac-Z|, |fac|, |mu|, |Z-Zold|, |Tf(C)-Sd(Delta)|, |mu_Delta|, |Sd(dDelta)|, |denominator|}; path[0] =
 * AOADMM_CPATH_*, path[1] = rank class of the row kernels (4, 8 or 16; 0 with AOADMM_CPATH_GENERIC).
 * AOADMM_ERR_UNSUPPORTED for a coupling that holds a mode of a PARAFAC2 block (its systems come from the block's slabs)
 * and on a context that belongs to a communicator or drives several devices. */
int aoadmm_op_coupled_loop(aoadmm_ctx* ctx, int coupling, const double* const* A, const double* const* C, int max_inner,
                           const double* tol, int* inner_iters, double* res, double* rho, double* const* L,
                           double* const* gram, double* slots, int* path);
/* The reduction a solve runs behind the rank pass of a ranking list, on host arrays: out[0..5] =
 * the AOADMM_RANKSUM_* sums of rank[0..n) and ncand[0..n) at cut-off k, out[6] = out[7] = 0.  n >= 1, k >= 1;
 * a query with rank < 0 is left out of everything.  Two launches (team partials in query order, a one-workgroup
 * finisher in a fixed order): the bits are a function of (rank, ncand, k) alone. */
int aoadmm_op_rank_metrics(aoadmm_ctx* ctx, int64_t n, const int64_t* rank, const int64_t* ncand, int64_t k, double out[8]);

#ifdef __cplusplus
}
#endif
#endif /* AOADMM_HIP_H */
