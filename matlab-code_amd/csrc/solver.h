// Host-side engine: model (struct Z), state (struct G) and the AO-ADMM outer loop
// (functions/cmtf_fun_AOADMM.m:87-476) driving the HIP kernels.  Everything stays
// resident in HBM; the host synchronises once per outer iteration to read the
// objective values and the inner-iteration counters (readback.h).  The members are defined in solver.hip (model, data,
// state), solver_solve.hip (outer loop), solver_objective.hip (objective, device and host half), solver_par2.hip
// (PARAFAC2 blocks), solver_coupled.hip (coupled ADMM loop) and solver_comm.hip (communicator).
#pragma once
#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "admm.h"
#include "common.h"
#include "contract.h"
#include "couple.h"
#include "cpblock.h"
#include "em.h"
#include "heldout.h"
#include "misc.h"
#include "par2.h"
#include "par2_sparse.h"
#include "rank_of.h"
#include "readback.h"
#include "small.h"
#include "sparse.h"
#include "state_snapshot.h"

typedef struct ncclComm* ncclComm_t;

namespace aoadmm {

struct ModeInfo {
  bool defined = false;
  int64_t rows = 0;
  int R = 0;
  bool slabs = false;
  int K = 0;
  std::vector<int64_t> rows_k, off_k;
  int tensor = -1, pos = -1;
  int coupling = -1;
  bool constrained = false;
  ProxSpec prox;
  DevBuf H, H2, Ht, H2t;   // coupling transformation matrices and their transposes
  DevBuf HHt;              // coupling type 2: H*H' (R x R)
  DevBuf eU, eUt, eLam;    // coupling types 1/5: H'*H = eU diag(eLam) eU' (rows x rows, host Jacobi once per model)
  DevBuf eV, eMu;          // coupling types 1/5: eigendecomposition of the R x R system matrix (every outer iteration)
  std::vector<double> H_host;
  int64_t img_rows = 0, img_cols = 0;   // shape of the factor-side coupling image (= shape of coupling_dual_fac)
  QuadPrep quad;           // quadratic regularization: L and its eigendecomposition
  int64_t hr = 0, hc = 0, h2r = 0, h2c = 0;
  double ridge = 0.0;
  DevBuf fac, Z, mu, muD;
  DevBuf facT;             // row-major copy of fac (by-product of the Gram kernel), valid while facT_version == version
  uint64_t facT_version = 0;
  bool has_fac = false, has_Z = false, has_mu = false, has_muD = false;
  int64_t muD_rows = 0, muD_cols = 0;
  uint64_t version = 1;
  // work buffers
  DevBuf A, Ab, gram, C, Bsys, L, Binv, rho, Zold, V, Znew, part, proxws, RHS, TD, TF, tmp, W1, W2;
  const double* Aeff = nullptr;
};

// PARAFAC2 block: K ragged slabs X_k (I x J_k) and the block's internal coupling variables
struct Par2Block {
  int K = 0, I = 0, R = 0;
  std::vector<int64_t> off_h;     // K+1 prefix sums of J_k
  DevBuf off_d;
  int64_t Jtot = 0;
  int Jmax = 0;
  DevBuf X;                       // slabs back to back, fp64
  DevBuf mask;                    // Z.miss{p}{k}: one byte per entry, same layout, 1 = observed
  bool has_mask = false;
  std::vector<char> have_slab;
  // sparse slabs (aoadmm_par2_slab_upload_coo): X, mask and T1 do not exist; every rank of a communicator holds all
  // nonzeros, the block is never slab-sharded and issues no collective
  bool sparse = false;
  Par2Sparse sp;
  DevBuf DeltaB, DeltaBold, P, Pold, muDB;        // state (G.DeltaB, G.P, G.mu_DeltaB)
  bool has_DeltaB = false;
  std::vector<char> have_P, have_mu;
  DevBuf W, T1, GB, Ak, Lk, rhok, part, norms, res, q, regv, Csys, ac, Lc, rhoc, rhomax;
  DevBuf Jrot;                                     // [K][R*R]: last Jacobi rotation per slab (warm start inside a B_k loop)
  // slab sharding over the ranks of a communicator (aoadmm_options.par2_slab_sharding): this rank runs the per-slab
  // kernels on [k0, k1) only; every sum over k is all-reduced, slab-valued state is gathered when the solve ends
  bool slab_sharded = false;
  int k0 = 0, k1 = 0;
  DevBuf psum;                    // R*R+1 partial sums of DeltaB, then 4 residual means
  // coupled C mode: sum(rho_k); H'H, the (K*R)^2 system and its inverse for coupling type 1 (:282-297)
  DevBuf rhosum, HtH, Mbig, Minv, Hs;   // Hs = diag(rho)*H for coupling type 3
  bool have_HtH = false, hth_diag = false;   // hth_diag: H'H is diagonal, HtH holds its K diagonal entries
  P2Dims dims() const {
    P2Dims d;
    d.K = K; d.I = I; d.R = R; d.off = off_d.as<int64_t>(); d.off_h = off_h.data(); d.Jtot = Jtot; d.Jmax = Jmax;
    d.k0 = slab_sharded ? k0 : 0; d.k1 = slab_sharded ? k1 : K;
    return d;
  }
  P2Dims dims_all() const {       // every slab, whatever the sharding (replicated C-mode loop)
    P2Dims d = dims();
    d.k0 = 0; d.k1 = K;
    return d;
  }
};

// Ranking list of one block (aoadmm_tensor_set_ranklist): what Engine::rank_of_run prepares and
// uploads per call, kept on the device with the plan's workspace and the per-query outputs, so that an evaluation inside
// a solve allocates nothing and touches no host memory.
struct RankList {
  int64_t nq = 0;                 // queries; 0: no list
  int mode = -1, nd = 0;
  int64_t I = 0;                  // rows of the target mode
  int64_t listed = 0;             // excluded rows after the per-query removal of repeats
  RankPlan plan;
  DevBuf idx;                     // int32 [nd x nq]; row `mode` holds the targets
  DevBuf eoff, eidx, coff, cq;    // the exclusion lists and their chunk table (plan.chunks > 0)
  DevBuf ws, rank, score, ncand;  // the plan's workspace and the per-query outputs of the last evaluation
  DevBuf part;                    // the metric reduction's partial sums per team (rank_metrics.h)
  bool evaluated = false;         // rank / score / ncand hold an evaluation
  int64_t resident_bytes() const {
    return (int64_t)(idx.bytes + eoff.bytes + eidx.bytes + coff.bytes + cq.bytes + ws.bytes + rank.bytes + score.bytes + ncand.bytes + part.bytes);
  }
  // the rank pass of this list against the factors hf (rank_of_w: the caller names its W and targets instead of idx)
  RankArgs args(const HeldoutFactors& hf) const {
    RankArgs a;
    a.hf = hf; a.mode = mode; a.I = I; a.nq = nq;
    a.idx = idx.as<int>();
    a.target = idx.as<int>() + (size_t)mode * nq;
    if (plan.chunks > 0) {
      a.excl_off = eoff.as<int64_t>();
      a.excl_idx = eidx.as<int>();
      a.chunk_off = coff.as<int64_t>();
      a.chunk_q = cq.as<int>();
    }
    a.workspace = ws.p;
    a.rank = rank.as<int64_t>();
    a.score = score.d();
    a.ncand = ncand.as<int64_t>();
    return a;
  }
  void clear() { *this = RankList(); }
  RankList() = default;
  RankList(RankList&&) = default;
  RankList& operator=(RankList&&) = default;
};

// aoadmm_rank_track: what a solve does with the ranking lists; belongs to the model
struct RankTrack {
  int metric = AOADMM_RANK_NDCG;
  int k = 10, every = 1, patience = 0, criterion = 0;
};

// the exclusion lists of a rank pass as the host prepares them (Engine::rank_prepare_excl)
struct RankExclHost {
  std::vector<int> ex32, chq;           // every query's rows sorted without repeats; the query of every chunk
  std::vector<int64_t> eoff64, choff;   // nq + 1 offsets into ex32 / into the chunks
};

struct TensorInfo {
  bool defined = false;
  bool par2 = false;
  Par2Block p2;
  int nmodes = 0;
  int modes[8] = {0};
  double weight = 1.0;
  CpBlock blk;
  double normsq = 0.0;
  bool normsq_valid = false;
  int last_pos = -1;
  // held-out list (aoadmm_tensor_set_heldout): belongs to the model, not to the data; every evaluation of the objective
  // inside a solve also scores it (heldout.h)
  HeldoutList ho;
  int ho_row_major = -1;        // what the block's last held-out pass gathered from: 1 the row-major factor copies, 0 the
                                // column-major factors, -1 no pass yet
  std::vector<double> ho_trace; // sum (y - m)^2 at iteration 0 .. OuterIterations of the last solve
  RankList rl;                  // ranking list (aoadmm_tensor_set_ranklist): belongs to the model, as the held-out list does
  std::vector<double> rl_trace; // kRankSlots sums per evaluation of the last solve (the iterations: Engine::rank_iters_)
  bool eval_shortcut = false;   // PARAFAC2: the enqueued objective evaluation took the last_mttkrp shortcut (:1254-1260)
  bool eval_list = false;       // marked masked CP block: the enqueued evaluation took the list form
  bool masked() const { return par2 ? p2.has_mask : blk.imputed(); }  // Z.miss{p} or per-entry weights given: the dense EM pass runs
  bool observed_only() const { return !par2 && blk.sparse && blk.sem.on; }   // sparse block whose unstored entries are missing
  bool missing() const { return masked() || observed_only(); }        // the block takes part in the EM step
};

struct CouplingInfo {
  int type = -1;
  std::vector<int> modes;
  DevBuf Delta, DeltaOld, BB, AA, LAA, dD, tmp, coef, rho_ptrs;
  std::vector<const double*> rho_ptrs_host;
  int64_t rows = 0, cols = 0;
  bool has_state = false;
};

// aoadmm_heldout_keep_best: the copy of the solver state at the iteration with the smallest weighted held-out sum
// (DESIGN.md section 9.4).  One table serves both directions: segments [0, nseg) copy the state into `store`, segments
// [nseg, 2 nseg) copy it back.
struct BestKeep {
  bool on = false;
  int iter = -1;                  // iteration `store` holds; -1: nothing kept
  DevBuf store, table;
  std::vector<SnapSeg> segs;      // host copy of the table's first half, as solve_setup built it
  int64_t bytes = 0;              // state bytes of one snapshot (this rank's own slabs of a slab-sharded PARAFAC2 block)
  int64_t launches = 0, moved = 0;   // snapshot launches of the last solve and the bytes they read + wrote
  bool use_dimtree = true;        // aoadmm_options.use_dimtree of the last solve (the restore replays its tensor passes)
};

// which partial contraction an imputing EM pass leaves for the next outer iteration (Engine::em_pass_enqueue)
enum EmFuse {
  kEmFuseNone = 0,     // none: a solve's last iteration, use_dimtree = 0
  kEmFuseAuto = 1,     // the mode whose factor stays unchanged longest
  kEmFuseSecond = 2,   // the second mode whenever that is allowed (the test hook AOADMM_EM_FUSE_SECOND_MODE)
};
// what an EM pass over a CP block ran (aoadmm_resident_em_pass); zeros and fused = -1 for a PARAFAC2 block
struct EmPassInfo {
  EmCpLaunch launch{0, 0, 0, 0, 0};
  int fused = -1;      // contracted tensor position of the fused pass (1 or 2), -1: none
  int walk = 0;        // EmCpArgs::walk
};

struct LocalGroup;
struct SolveRun;                      // what one solve carries from step to step (solver_solve.hip)

// natural-layout array on the device (first dimension padded to X.pad0) -> unpadded doubles on the host (solver.hip)
void download_unpadded(const DenseTensor& X, int64_t rows, int64_t cols, double* out, hipStream_t s);

// coupling images (solver_coupled.hip): Sd(D), Tf(F) and Tf'(Y) for mode `mi` of coupling `ci`; each returns its input
// where the map is the identity and `dst` otherwise
const double* image_d(double* dst, const CouplingInfo& ci, const double* D, const ModeInfo& mi, const AdmmCtl* ctl,
                      hipStream_t s);
const double* image_f(double* dst, const CouplingInfo& ci, const double* F, const ModeInfo& mi, const AdmmCtl* ctl,
                      hipStream_t s);
const double* adjoint_f(double* dst, const CouplingInfo& ci, const double* Y, const ModeInfo& mi, const AdmmCtl* ctl,
                        hipStream_t s);

class Engine {
 public:
  explicit Engine(int device);
  ~Engine();

  // model
  void model_begin(int n_modes, int n_tensors, int n_couplings);
  void set_mode(int mode, int64_t rows, int rank);
  void set_mode_slabs(int mode, int K, const int64_t* rows_k, int rank);
  void add_cp(int p, int n, const int* modes, double weight);
  void add_par2(int p, const int* modes3, double weight);
  void set_constraint(int mode, int type, const double* params, int np, const double* Lmat);
  void set_coupling(int mode, int coupling, const double* H, int64_t hr, int64_t hc, const double* H2,
                    int64_t h2r, int64_t h2c);
  void set_coupling_type(int coupling, int type);
  void set_ridge(const double* ridge);
  void model_end();

  // data
  void tensor_upload(int p, const double* data, int prec, int64_t row0, int64_t local_rows);
  void tensor_upload_coo(int p, int64_t nnz, const int64_t* subs, const double* vals, bool shard = false);
  void tensor_synth(int p, int rank, uint64_t seed, double noise, int prec);
  void par2_slab_upload(int p, int k, const double* Xk);
  void par2_slab_upload_coo(int p, int64_t nnz, const int64_t* subs, const double* vals);
  void tensor_mask_upload(int p, const uint8_t* mask);
  void tensor_weights_upload(int p, const double* W);   // full array, like the mask; null: the block is plain again
  void par2_slab_mask_upload(int p, int k, const uint8_t* mask);
  void set_observed_only(int p, bool on);          // sparse CP block: unstored entries are missing (sparse_em.h)
  // weights in [0, 1] for the stored entries (wts null with nnz = 0: all 1) and one for every unstored entry
  void set_entry_weights(int p, int64_t nnz, const int64_t* subs, const double* wts, double unstored_weight);
  double tensor_normsq(int p);
  // what tensor p keeps on the device: the precision its passes stream, the power-of-two scale of a half block (else 1)
  // and the bytes of its natural array, pass copies, transposed copy and mask (dense CP blocks), of the per-mode copies
  // of the nonzeros this rank holds (sparse CP blocks); 0 for PARAFAC2 blocks
  void tensor_storage_info(int p, int* precision, double* scale, int64_t* resident_bytes);

  // state
  void state_set(int field, int index, int slab, const double* host, int64_t rows, int64_t cols);
  void state_get(int field, int index, int slab, double* host, int64_t rows, int64_t cols);

  // solve
  void solve(const aoadmm_options& opt, aoadmm_result* out);
  void resident_mttkrp(int p, int pos, double* out_host, float* ms);
  void resident_em_step(int p, double stats[3]);   // one EM step of an observed-only block: {sum_Omega (x-m)^2, num, den}
  // One EM pass over the masked dense block p as a solve runs it (aoadmm_resident_em_pass): em_pass_enqueue(p, update,
  // fuse), then what it left.  stats: the four EM statistics in the EmStat order; data / data_t (may be null): the
  // block's natural array / a matrix block's transposed copy, unpadded, as doubles (PARAFAC2: the slabs back to back);
  // mttkrp (may be null): when the pass fused a contraction, the unweighted MTTKRP of the first position of the update
  // sequence finished from the cached T; info[8] = {vec, rmax, fused, walk, strips, jchunks, jlen, that position or -1}
  void resident_em_pass(int p, int update, int fuse, double stats[4], double* data, double* data_t, double* mttkrp,
                        int64_t info[8]);
  // The missing entries of a masked dense CP block as a list (em_list.h).  on: builds the list
  // from the resident mask and marks the block, so that its imputing EM passes walk the list; off: releases both.
  void set_missing_list(int p, bool on);
  // n (may be null): entries of the list; subs (may be null): their subscripts, column-major n x N, in list order
  void missing_list(int p, int64_t* n, int64_t* subs);
  // One list pass over the marked block p as a solve runs it (aoadmm_resident_em_list_pass): stats2 = {num, den};
  // data / data_t as for resident_em_pass
  void resident_em_list_pass(int p, int update, double stats2[2], double* data, double* data_t);
  // held-out scoring (heldout.h)
  void model_at(int p, int64_t n, const int64_t* subs, double* out_host);     // the model of block p at n subscripts
  void set_heldout(int p, int64_t n, const int64_t* subs, const double* vals);   // n = 0 removes the list
  void heldout_stats(int p, double stats[4]);      // {sum (y-m)^2, sum y^2, sum m^2, count} for the current factors
  void heldout_info(int p, int64_t* n, int64_t* resident_bytes, int* row_major) const;
  void heldout_trace(int p, double* out, int cap, int* len, int* best_iter) const;
  // the best held-out iterate: the switch, the copy back into the state, what is kept
  void heldout_keep_best(int on);
  void heldout_restore_best(int* iter);
  void heldout_best_info(int* have, int* iter, int64_t* bytes, int64_t* launches) const;
  // top-k completions along one mode of a CP block (topk.h)
  void topk(int p, int mode, int64_t nq, const int64_t* subs, int k, const int64_t* excl_off, const int64_t* excl_idx,
            int64_t* idx_host, double* val_host);
  // the same with the weights given (W: nq x R column-major on the host) instead of formed from subscripts
  void topk_w(int p, int mode, int64_t nq, const double* W, int k, const int64_t* excl_off, const int64_t* excl_idx,
              int64_t* idx_host, double* val_host);
  void topk_run(const char* what, int p, int mode, int64_t nq, const int64_t* subs, const double* W, int k, const int64_t* excl_off,
                const int64_t* excl_idx, int64_t* idx_host, double* val_host);
  // the place of a target row among a query's candidates (rank_of.h): subs' column `mode` holds
  // the target; _w: the weights given (W: nq x R column-major on the host) with the targets beside them
  void rank_of(int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off, const int64_t* excl_idx, int64_t* rank_host,
               double* score_host, int64_t* ncand_host);
  void rank_of_w(int p, int mode, int64_t nq, const double* W, const int64_t* targets, const int64_t* excl_off, const int64_t* excl_idx,
                 int64_t* rank_host, double* score_host, int64_t* ncand_host);
  void rank_of_run(const char* what, int p, int mode, int64_t nq, const int64_t* subs, const double* W, const int64_t* targets,
                   const int64_t* excl_off, const int64_t* excl_idx, int64_t* rank_host, double* score_host, int64_t* ncand_host);
  // ranking metrics tracked inside a solve (rank_metrics.h)
  void set_ranklist(int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off, const int64_t* excl_idx);   // nq = 0 removes the list
  void ranklist_info(int p, int64_t* nq, int* mode, int64_t* listed, int64_t* resident_bytes) const;
  void rank_track(int metric, int k, int every, int patience, int criterion);
  void rank_trace(int p, int what, double* out, int cap, int* len, int* iters, int* best_iter) const;
  void ranklist_last(int p, int64_t* rank_host, double* score_host, int64_t* ncand_host);
  // new rows along one mode of a CP block from their entries (foldin.h)
  int tensor_rank(int p) const;                    // the number of components of block p (aoadmm_tensor_rank)
  void fold_in(int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals, const aoadmm_foldin_options* opt,
               double* rows_host, int* info_host, int* iters_host, double* gram_host, double* rhs_host);
  // the same under entry weights (null: ones) and a weight for the unlisted cells: the weighted instantiations run
  void fold_in_w(int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals, const double* wts,
                 double unstored_weight, const aoadmm_foldin_options* opt, double* rows_host, int* info_host, int* iters_host,
                 double* gram_host, double* rhs_host);
  void fold_in_run(const char* what, bool weighted, int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals,
                   const double* wts, double alpha, const aoadmm_foldin_options* opt, double* rows_host, int* info_host,
                   int* iters_host, double* gram_host, double* rhs_host);
  // new slabs of a PARAFAC2 block: their rows of C against the fitted A and DeltaB (par2_foldin.h)
  int64_t par2_rows(int p) const;                  // I of PARAFAC2 block p: the rows every slab has (aoadmm_par2_rows)
  void par2_fold_in(int p, int64_t nk, const int64_t* cols, const double* X, const double* c0, const aoadmm_par2_foldin_options* opt,
                    double* C_host, double* B_host, double* P_host, double* res_host, double* xnorm_host, int* iters_host, int* info_host,
                    double* Y_host, double* sys_host, int* path_host);
  // Tucker projection of a resident 3-way CP block and the core consistency of its CP model (core.h, DESIGN.md section
  // 9.9): core (r[0] x r[1] x r[2], column-major) = X x_1 M[0]' x_2 M[1]' x_3 M[2]', M[n] on the host
  void project(int p, const double* const* M, const int64_t* ld, const int* r, double* core_host);
  void core_consistency(int p, double* cc, double* core_host, int* rank_deficient);
  void resident_unfold_gram(int p, int pos, int slab, double* out_host);
  void resident_nvecs(int p, int pos, int r, const aoadmm_nvecs_options* opt, double* U_host, int64_t ldU, double* eig_host,
                      aoadmm_nvecs_info* info);
  void resident_par2_rhs(int p, int pos, double* out_host, float* ms);
  void kernel_stats(int which, int reset, double* ms, int64_t* launches, double* bytes, double* flops);
  // The coupled ADMM loop of coupling c as a solve runs it after the MTTKRPs (aoadmm_op_coupled_loop): A[j] (rows_j x R_j)
  // and Cm[j] (R_j x R_j, weight applied) of the coupling's j-th mode come from the host, the state is the engine's.
  // Every output may be null: rho (n), L / gram (n pointers, R_j x R_j each), slots (n x 8), path (2).
  void coupled_loop_op(int c, const double* const* A, const double* const* Cm, int max_inner, const double* tol,
                       int* inner_iters, double* res, double* rho, double* const* L, double* const* gram, double* slots,
                       int* path);

  // communicator
  void comm_init(const char id[128], int rank, int world, bool share_only = false);
  void comm_init_local(int key, int rank, int world);
  // Unblocks this engine's collectives after a failure on ANOTHER rank of the same process (aoadmm_create_multi):
  // callable from a foreign thread while the engine's own thread waits inside a collective; the next collective
  // throws AOADMM_ERR_RCCL.  The communicator is gone afterwards.
  void comm_abort();
  void comm_info(int* nccl_version, int* comm_ranks, char* lib_path, int cap) const;
  void set_progress(aoadmm_progress_fn fn, void* user, int every) { progress_fn_ = fn; progress_user_ = user; progress_every_ = every; }
  void par2_gather_slabs(TensorInfo& t);
  // (world_ > 1 stays true after an abort took the communicator away: the engine must not fall back to unsharded work)
  bool sharded() const { return world_ > 1 || comm_ != nullptr || local_ != nullptr; }
  void require_half_ok(const TensorInfo& t, int p, bool row_block) const;   // AOADMM_ERR_UNSUPPORTED where AOADMM_PREC_F16 is not available
  void require_usable() const;          // throws AOADMM_ERR_RCCL once comm_abort() has run (sticky)
  bool share_only() const { return share_only_; }
  // One of the engines of a multi-device context (aoadmm_create_multi with more than one device): its data calls fan out
  // from one caller, and AOADMM_PREC_F16 stays refused there (require_half_ok)
  void set_multi_member() { multi_member_ = true; }
  int rank() const { return rank_; }
  int world() const { return world_; }

  hipStream_t stream() const { return stream_; }
  int device() const { return device_; }

  // what the block functions (cpblock.h) use of this engine
  BlockCtx block_ctx() {
    return BlockCtx{stream_, &timers_, rank_, world_, sharded(), allow_xp_, &staging_,
                    [](void* e, const double* send, double* recv, int64_t n) { static_cast<Engine*>(e)->allreduce_from(send, recv, n); },
                    this};
  }
  bool prefetch_next_contraction(const aoadmm_options& opt);   // true: a tensor pass was enqueued
  void allreduce(double* buf, int64_t n);
  void allreduce_from(const double* send, double* recv, int64_t n);   // out of place (send == recv: in place)

 private:
  void check_mode(int m) const;
  // model_end, paragraph by paragraph
  void check_model() const;
  void shape_coupling(int c);              // modes, shapes and checks of one coupling
  void precompute_coupling(int c);         // H*H' / the eigendecomposition of H'*H, once per model
  void alloc_readback();
  void comm_release();                     // destroys the RCCL communicator, if any (solver_comm.hip)
  bool has_missing() const;
  // statistics of tensor p into its EM slots (+ imputation); fuse: EmFuse, honoured where the block allows it
  void em_pass_enqueue(int p, int update, int fuse = kEmFuseNone, EmPassInfo* info = nullptr);
  void sparse_em_enqueue(int p, bool stats_only);  // EM step of an observed-only sparse block into its EM slots
  // list pass of the marked block p: num and den into its EM slots (+ imputation); timed: events of class kStatsEmList
  void em_list_enqueue(int p, int update, bool timed);
  bool has_heldout() const;
  HeldoutFactors heldout_factors(const TensorInfo& t, bool* row_major) const;   // the current fac state of block t as the pass gathers it
  // skip_mode >= 0: that column of subs is neither read nor checked (its part of idx32 stays zero)
  void heldout_check_subs(const TensorInfo& t, int p, int64_t n, const int64_t* subs, std::vector<int>& idx32, int skip_mode = -1) const;
  // The opening of the calls that ask nq queries along one mode of CP block p (top-k, rank-of, the ranking list, fold-in):
  // usable engine, ended model, p, no PARAFAC2 block ("<what>: tensor p is a PARAFAC2 block; <purpose>"), order, mode,
  // nq in [0, 2^31).  (solver_topk.hip)
  TensorInfo& query_block(const char* what, const char* purpose, int p, int mode, int64_t nq);
  // exclusion lists (excl_off not null): offsets non-decreasing from 0, rows in [0, I); ex32: the rows as int32, unsorted
  void check_excl(int p, int64_t I, int64_t nq, const int64_t* excl_off, const int64_t* excl_idx, std::vector<int>& ex32) const;
  // W (nq x R column-major on the host) row-major into `dev`; asynchronous: `rows` lives until the caller synchronises
  void upload_w_rows(const double* W, int64_t nq, int R, std::vector<double>& rows, DevBuf& dev);
  // check_excl, the per-query sort and removal of repeats and the chunk table of the exclusion lists of a rank pass
  void rank_prepare_excl(int p, int64_t I, int64_t nq, const int64_t* excl_off, const int64_t* excl_idx, RankExclHost& h) const;
  // uploads them into l (asynchronously: the caller synchronises before `h` goes)
  void rank_upload_excl(const RankExclHost& h, RankList& l);
  // the device side of nq checked queries (everything of a RankList but `part`); idx32 empty: no subscripts (rank_of_w)
  RankList rank_list_build(const TensorInfo& t, int mode, int64_t nq, int64_t I, const std::vector<int>& idx32, const RankExclHost& xh);
  CpBlock& project_block(const char* what, int p);   // tensor p's block, or the refusal of what cannot be projected
  void project_dense(CpBlock& b, const double* const* M, const int64_t* ld, const int* r, double* G);    // G: device
  void project_sparse(CpBlock& b, const double* const* M, const int64_t* ld, const int* r, double* G);
  bool has_ranklist() const;
  void ranklist_enqueue(int p, double* slots);     // block p's ranking list against the current factors -> kRankSlots sums (device)
  double rank_score(const ArenaView& h) const;     // the pooled mean of the tracked metric over the blocks with a list
  void heldout_enqueue(int p, double* sums);       // block p's list against the current factors -> sums[0..2] (device)
  std::vector<SnapSeg> best_state_segments() const;   // every array aoadmm_state_get can return, as (src, bytes, start)
  void best_build_table();                         // solve_setup: the segment table and the kept buffer of this solve
  void best_snapshot(int iter);                    // record_iteration: the state of iteration `iter` into the kept buffer
  void compute_gram(ModeInfo& mi);
  FactorRef factor_ref(const ModeInfo& o) const {
    return FactorRef{o.fac.d(), o.rows, o.version, o.facT_version == o.version ? o.facT.d() : nullptr};
  }
  void factor_refs(const TensorInfo& t, FactorRef facs[8]) const {
    for (int i = 0; i < t.nmodes; ++i) facs[i] = factor_ref(modes_[t.modes[i]]);
  }
  // outer loop, step by step (solver_solve.hip)
  void solve_setup(const aoadmm_options& opt);
  void decide_slab_sharding(TensorInfo& t, const aoadmm_options& opt);
  void outer_updates(const aoadmm_options& opt, int iter, bool has_miss);
  void update_mode(int m, int cid, const aoadmm_options& opt, int iter);
  void enqueue_readback(SolveRun& r);
  void enqueue_objective(SolveRun& r, int iter);
  void finish_objective(SolveRun& r);
  void record_iteration(SolveRun& r, int iter);
  void update_uncoupled_cp_mode(int m, const aoadmm_options& opt);
  void prepare_mode_system(int m, int nrho, const aoadmm_options& opt);
  // the system of a CP mode in one place for the solver and aoadmm_op_coupled_loop: how often rho/2*I enters a coupled
  // mode's matrix, where sys_build writes, and what follows it (eigenvectors for types 1/5, Aeff)
  int coupled_nrho(int m) const;
  SysBuild mode_sysbuild(int m, int nrho);
  void close_mode_system(int m, const SysBuild& sb, bool build, const double* A);
  void prepare_next_first_mode(const aoadmm_options& opt);
  void ensure_mode_work(ModeInfo& mi);
  // objective (solver_objective.hip): the device half fills the arena, the host half reads its pinned copy
  void eval_objective_enqueue(bool first);
  void check_not_pd(const ArenaView& h) const;
  void objective_from_host(const ArenaView& h, double f[4]) const;
  double rel_missing_from_host(const ArenaView& h) const;
  // coupled ADMM loop (solver_coupled.hip): coupled_admm prepares it and runs one of the three forms
  struct CoupleForm { CouplePath path; int rmax; bool any_pc; };   // rmax: largest rank, cols(Delta) included
  CoupleForm coupled_form(const CouplingInfo& ci);
  void coupled_admm(int c, const aoadmm_options& opt);
  void coupled_one_launch(CouplingInfo& ci, AdmmCtl* ctl, const aoadmm_options& opt, CouplePath path, int rmax);
  void coupled_row_steps(CouplingInfo& ci, AdmmCtl* ctl, const aoadmm_options& opt, int rmax);
  void coupled_generic(CouplingInfo& ci, AdmmCtl* ctl, const aoadmm_options& opt, bool any_pc);
  void coupled_generic_primal(CouplingInfo& ci, ModeInfo& mi, AdmmCtl* ctl, bool first);
  void coupled_generic_delta(CouplingInfo& ci, AdmmCtl* ctl, bool any_pc);
  void coupled_generic_dual(CouplingInfo& ci, int m, AdmmCtl* ctl);
  FinalizeArgs coupled_finalize_args(const CouplingInfo& ci, const aoadmm_options& opt);
  Par2Block* par2_c_block(const ModeInfo& mi);
  // PARAFAC2 (solver_par2.hip)
  void par2_ensure_work(TensorInfo& t);
  void par2_prepare_modeA(int m, int nrho, const aoadmm_options& opt);
  void par2_update_B(int m, const aoadmm_options& opt, int iter);
  void par2_update_C(int m, const aoadmm_options& opt);
  void par2_prepare_C_coupled(int m, int ctype, const aoadmm_options& opt);
  void par2_objective_enqueue(TensorInfo& t);
  // sparse slabs: one pass over the nonzeros (pos 0: the row-sorted copy, 1: the column-sorted copy), counted in timers_.stats[3]
  void par2s_pass(Par2Block& b, int pos, const CooFactor& f, double* out, int64_t ldOut);
  void par2s_rhs_A(TensorInfo& t, double* out);     // out (I x R) = sum_nnz x * B(g,:) .* C(k(g),:)
  void par2s_ensure_Y(TensorInfo& t);               // Y = Xcat' * A for the current A (cached by its version)
  std::vector<int> update_sequence(int p) const;

  int device_ = 0;
  hipStream_t stream_ = nullptr;
  hipStream_t side_ = nullptr;        // objective evaluation beside the prefetched tensor pass (Engine::solve)
  hipEvent_t side_ev_ = nullptr;
  int n_modes_ = 0, n_tensors_ = 0, n_couplings_ = 0;
  bool model_done_ = false;
  bool has_ridge_ = false;
  std::vector<ModeInfo> modes_;
  std::vector<TensorInfo> tensors_;
  std::vector<CouplingInfo> couplings_;
  DevBuf readback_;      // everything the host reads once per outer iteration, in one piece (one copy); a PARAFAC2
                         // block's res, q and regv are views into it
  ArenaLayout arena_;    // its layout (readback.h)
  ArenaView dev_;        // typed pointers into readback_
  DevBuf redws_;         // reduction workspace
  DevBuf ones_;          // a device 1.0 (unit weight where a kernel expects a rho pointer)
  DevBuf emws_;          // EM pass partial sums
  bool allow_xp_ = true;  // options.hip.no_permuted_copy
  DevBuf atbws_;
  DevBuf staging_;
  LaunchTimers timers_;   // event pool and kernel statistics (cpblock.h)
  int ho_best_iter_ = -1;   // iteration of the smallest weighted held-out sum of the last solve (-1: no list was attached)
  BestKeep best_;           // aoadmm_heldout_keep_best
  RankTrack track_;         // aoadmm_rank_track
  bool rank_eval_now_ = false;     // set by solve(): the evaluation being enqueued also evaluates the ranking lists
  std::vector<int> rank_iters_;    // the evaluated iterations of the last solve
  int rank_best_iter_ = -1;        // iteration of the largest pooled score of the last solve (-1: no list was attached)
  int prepared_mode_ = -1;  // mode whose MTTKRP + system build were enqueued ahead (prepare_next_first_mode)
  ncclComm_t comm_ = nullptr;
  mutable std::mutex comm_mu_;          // comm_ / aborted_ against comm_abort() from another worker thread
  std::atomic<bool> aborted_{false};
  std::shared_ptr<LocalGroup> local_;   // process-local group (threads of one process), see solver_comm.hip
  int rank_ = 0, world_ = 1;
  bool multi_member_ = false;           // set_multi_member()
  bool share_only_ = false;             // aoadmm_comm_init_rank_share: rank_/world_ of an N-rank job on a one-rank communicator
  aoadmm_progress_fn progress_fn_ = nullptr;   // options.Display = 'iter'
  void* progress_user_ = nullptr;
  int progress_every_ = 0;

  AdmmCtl* ctl_of_mode(int m) const { return dev_.ctl(m); }
  AdmmCtl* ctl_of_coupling(int c) const { return dev_.ctl(n_modes_ + c); }
  double* resid_slots(int m) const { return dev_.resid(m); }
};

}  // namespace aoadmm
