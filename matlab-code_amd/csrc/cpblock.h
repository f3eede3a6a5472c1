// One dense CP block (tensor or matrix): its resident data, the pass copies, the partial-contraction cache and the
// MTTKRP paths over them.  Nothing here knows the model, the couplings or the outer loop; what a function needs from
// the engine arrives in a BlockCtx.
#pragma once
#include "common.h"
#include "contract.h"
#include "em_list.h"
#include "sparse.h"
#include "sparse_em.h"

#include <functional>

namespace aoadmm {

struct FactorRef {
  const double* p;    // device, column-major
  int64_t ld;
  uint64_t version;
  const double* pT = nullptr;   // optional row-major copy (rows x R) of the same version, written by the Gram kernel
};

constexpr int kStatsEmPass = 4;
constexpr int kStatsHeldout = kStatsEmPass + kCooMaxModes;   // the held-out pass (heldout.h)
constexpr int kStatsTopk = kStatsHeldout + 1;                 // the top-k completions (topk.h) and the ranks of targets (rank_of.h)
constexpr int kStatsFoldin = kStatsTopk + 1;                  // the fold-in of new rows (foldin.h)
// (kStatsFoldin + 1 stays unassigned: aoadmm_kernel_stats has always refused it, and callers that probe one past the
// fold-in class rely on that)
constexpr int kStatsEmList = kStatsFoldin + 2;                // the list pass of aoadmm_resident_em_list_pass (em_list.h)
constexpr int kStatsPar2Foldin = kStatsEmList + 1;            // the fold-in of new PARAFAC2 slabs (par2_foldin.h)
constexpr int kStatsClasses = kStatsPar2Foldin + 1;

struct KernelStats {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double ms = 0.0, bytes = 0.0, flops = 0.0;
  int64_t launches = 0, timed = 0;      // timed <= launches: launches bracketed by an event pair
};

// Event pool and kernel statistics of one engine.  begin()/end() bracket the launches of one MTTKRP step with an event
// pair when the budget allows and count it in `ks` either way.
struct LaunchTimers {
  struct Pair { hipEvent_t e0 = nullptr, e1 = nullptr; };
  std::vector<hipEvent_t> pool;   // timing events are recycled: creating two per tensor pass cost host time in the loop
  // [0] streaming contraction, [1] leading-mode contraction, [2] reductions over T, [3] sparse MTTKRP, the passes over
  // sparse PARAFAC2 slabs and the EM steps of observed-only blocks, [kStatsEmPass + n] the pass of those steps over
  // mode n's copy, [kStatsHeldout] the held-out passes, [kStatsTopk] the top-k completions, [kStatsFoldin] the fold-in of new rows,
  // [kStatsEmList] the op-level list passes of marked masked blocks, [kStatsPar2Foldin] the fold-in of new PARAFAC2 slabs
  KernelStats stats[kStatsClasses];
  bool profile = true;
  bool profile_reductions = false;   // switched on by the first kernel_stats(2, ...) call: two more events per reduction
  hipEvent_t take_event();
  void fold_finished(KernelStats& ks);   // completed pairs are added to ks.ms, their events go back to the pool
  Pair take_pair(KernelStats& ks);       // two events, or none once ks holds 4096 unfinished pairs
  Pair begin(KernelStats& ks, bool timed, hipStream_t s);                    // records e0 when it took a pair
  void end(KernelStats& ks, Pair pr, hipStream_t s, double bytes, double flops);   // records e1, then count()
  void count(KernelStats& ks, Pair pr, double bytes, double flops);
};

// What the block functions use of the engine that calls them
struct BlockCtx {
  hipStream_t stream;
  LaunchTimers* timers;
  int rank, world;
  bool sharded;        // Engine::sharded()
  bool allow_copies;   // options.hip.no_permuted_copy == 0
  DevBuf* staging;     // host-to-device staging of the uploads
  // recv = sum over the ranks of send, enqueued on `stream` (send == recv: in place): Engine::allreduce_from of `comm`
  void (*allreduce_from)(void* comm, const double* send, double* recv, int64_t n);
  void* comm;
};

// 3-way tensors: copy[c] is the resident copy the pass that contracts mode c streams over, so that all three passes
// run the same register-streaming kernel (each the tensor's size again in HBM; 288 GB per GPU).  All are row-blocked
// (misc.hip block_layout_copy): copy[0](j,k,i) = X(i,j,k), copy[1](k,i,j) = X(i,j,k) (one streaming pass instead of K
// batches of an I x J matrix: measured 6.0 ms against 5.4-5.5 ms at 2000^3), copy[2] the rows of X itself.
struct PassCopy {
  DevBuf buf;
  int64_t pad = 0;     // padded extent of the leading uncontracted mode: of J, of K, X.pad0
  bool present = false, refused = false;   // refused is sticky: no room in HBM, or a mode too long for the copy kernels
};

// One dense CP block (tensor or matrix) and its partial-contraction cache.
struct CpBlock {
  DenseTensor X;       // natural layout, first dimension padded
  DenseTensor Xt;      // matrices only: transposed copy (second mode contiguous)
  PassCopy copy[3];
  DevBuf emkr, emkr2;  // order > 3 with Z.miss: Khatri-Rao factor of the merged trailing modes (ping-pong)
  // With a communicator copy[0] is sharded along mode 3 instead of mode 1:
  // rank g holds X(:, :, K_g), contracts ALL of mode 1 and gets a complete T(j, k in K_g, r) of 1/N the size, instead
  // of a partial sum of full size J x K from its rows of mode 1.
  bool xp_ksharded = false;
  int64_t xp_k0 = 0, xp_kloc = 0;
  int nd = 0;
  int64_t dims[8] = {0};   // local sizes (dims[0] = local rows when sharded)
  int64_t full0 = 0;       // global size of the first mode
  int64_t row0 = 0;        // first local row of the first mode
  bool has_data = false;
  // The natural-layout array is only read to build the three pass copies, for ||X||^2, the EM pass and the fallbacks; once
  // all three copies exist (and no mask does) it can go: 4 -> 3 resident copies (maybe_release_natural)
  bool x_released = false;
  // AOADMM_PREC_F16 storage (3-way blocks, block_make_half): the three pass copies hold q = fp16_rn(x * scale), `scale`
  // a power of two, and ARE the data (q / scale); the fp32 natural array they were rounded from is gone (x_released).
  // With a communicator `scale` comes from the WHOLE tensor (the same on every rank) and copy[0] may be xp_ksharded.
  bool half = false;
  double scale = 1.0;
  // dimension-tree cache: T = X x_c F_c, valid while factor c keeps `cached_version`
  int cached_mode = -1;
  uint64_t cached_version = 0;
  ContractPlan plan;
  DevBuf T, frag, scratch, ft, tmpA, tmpB;
  // sharded MTTKRP outputs that are this rank's ROWS of the result (mode 1; mode 3 under xp_ksharded): send buffers whose
  // other rows are zero for good (cleared once), all-reduced out of place into the caller's buffer
  DevBuf own[2];
  size_t own_bytes[2] = {0, 0};
  int64_t own_row0[2] = {-1, -1};
  // Z.miss{p}: one byte per entry in the layout of X (and of Xt for matrices), 1 = observed
  DevBuf mask, maskT;
  bool has_mask = false;
  bool mask_imputed = false;   // an EM pass has written model values over the missing entries of X since the data arrived
  // aoadmm_tensor_set_missing_list: the imputing EM pass walks the list of the missing entries
  // instead of the array.  Belongs to the data and its mask: every upload of either, and of weights, drops it.
  MissingList mlist;
  // Per-entry weights in [0, 1] (aoadmm_tensor_weights_upload): X.data is then Xhat =
  // W o X0 + (1 - W) o M, X0 the data as uploaded and Wt the weights, both in the layout and precision of X (an fp32
  // block keeps fp32 weights); X0t / WtT are their transposed copies beside Xt (matrices).  Never together with a mask.
  DevBuf X0, Wt, X0t, WtT;
  bool has_weights = false;
  bool imputed() const { return has_mask || has_weights; }   // the EM pass rewrites X: no pass copy, no release of X
  void clear_weights() { X0.release(); Wt.release(); X0t.release(); WtT.release(); has_weights = false; }
  // sparse form of Z.object{p}: replaces everything above but nd / dims / has_data.  aoadmm_tensor_upload_coo: every
  // rank of a communicator holds all nonzeros and computes the complete MTTKRP (no collective);
  // aoadmm_tensor_upload_coo_sharded: every rank holds its share of the nonzeros (coo.sharded) and the MTTKRP is an
  // all-reduce of the shares' partial sums, from the block's per-mode send buffers (CooBlock::send)
  bool sparse = false;
  CooBlock coo;
  // observed-only form of a sparse block (aoadmm_tensor_set_observed_only): the unstored entries are missing, not zero
  SparseEm sem;
  // New data has arrived, dense or sparse: no copy, cached contraction or release state of the old data holds.  Frees
  // nothing but the list of the old mask's missing entries (a pass copy's buffer is reused by the next build; the sparse
  // upload releases what it no longer needs).
  void reset_derived() {
    has_data = true; x_released = false; cached_mode = -1; xp_ksharded = false; half = false; scale = 1.0; mask_imputed = false;
    mlist.clear();
    for (PassCopy& c : copy) c.present = c.refused = false;
  }
};

inline int64_t pad_of(int prec, int64_t n) { return round_up(n, prec == AOADMM_PREC_F32 ? 4 : 2); }
// distance (in updates) until tensor position `c` is updated again after position `pos`
int next_update_distance(int pos, int c, const int* seq, int n);
// tiny unsharded block: MTTKRP by the one-launch kernel instead of contraction pass + reduction
inline bool small_direct(bool sharded, const CpBlock& b, int R) {
  return !sharded && !b.half && small_mttkrp_ok(b.X.elems_padded(), b.nd, b.dims, R);
}

// `full_array`: the caller's whole tensor when it holds one (lets a sharded engine take its mode-3 slab as well)
void block_upload(const BlockCtx& cx, CpBlock& b, int nd, const int64_t* dims, const double* host, int prec, int64_t row0,
                  int64_t local_rows, const double* full_array = nullptr);
// Fills `slab` with X(:, :, [k0, k0 + kloc)) of the WHOLE tensor in the natural fp32 layout (all full0 rows, padded to
// pad_of(AOADMM_PREC_F32, full0)): the caller's way to the mode-3 slab of a sharded half block (upload or generator)
using SlabSource = std::function<void(DevBuf& slab, int64_t k0, int64_t kloc)>;
// Turns a freshly uploaded fp32 3-way block into its half form (include/aoadmm_hip.h, AOADMM_PREC_F16): scale from the
// largest magnitude, three half pass copies built one at a time, natural array released.  On a sharded engine the call
// is COLLECTIVE: the largest magnitude and the "not finite" flag of every rank's data (its rows and, with `slab_source`
// where want_ksharded_xp agrees, its mode-3 slab, which becomes the xp_ksharded copy[0]) meet in one all-reduce, so every
// rank gets the same scale and the same verdict.  Throws AOADMM_ERR_INVALID for a non-finite entry anywhere (on every
// rank, after the exchange), AOADMM_ERR_NOMEM / AOADMM_ERR_UNSUPPORTED when a copy cannot be built (this rank alone); the
// block is then left without data.
void block_make_half(const BlockCtx& cx, CpBlock& b, const SlabSource* slab_source = nullptr);
// Gives the dense block weights (CpBlock::has_weights) from `host`, the block's local rows x the other modes, column-major
// fp64: converted to the block's precision, checked on the device while they pass through the staging buffer, and Xhat
// reset to W o X0.  X0 is what the block holds at the first call (later calls replace W alone); a mask is dropped.
// False, with the block as it was, when a weight is not a finite number in [0, 1].
bool block_set_weights(const BlockCtx& cx, CpBlock& b, const double* host);
// false when some host[e], e < n, is not a finite number in [0, 1]: the same check on an array the block keeps only a
// part of (a rank of a communicator checks the whole W, so that every rank reaches the same verdict)
bool block_weights_in_range(const BlockCtx& cx, const double* host, int64_t n);
// the block without its weights: Xhat <- X0
void block_drop_weights(const BlockCtx& cx, CpBlock& b);
// Xhat <- W o X0: where every solve of a weighted block starts
void block_reset_weighted(const BlockCtx& cx, CpBlock& b);
// builds the mode-3-sharded copy[0] from a natural-layout slab X(:, :, [k0, k0 + kloc)) already on the device
void adopt_ksharded_xp(const BlockCtx& cx, CpBlock& b, const void* slab, int64_t k0, int64_t kloc);
bool want_ksharded_xp(const BlockCtx& cx, const CpBlock& b, int64_t K, int64_t* k0, int64_t* kloc);
bool ensure_pass_copy(const BlockCtx& cx, CpBlock& b, int c);   // false: the pass that contracts mode c runs on X
void drop_pass_copies(CpBlock& b);
void maybe_release_natural(const BlockCtx& cx, CpBlock& b, bool normsq_valid);
// makes b.T hold a partial contraction that serves an MTTKRP for tensor position `pos` (3-way blocks)
void ensure_contraction(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, int R, bool use_cache,
                        const int* update_seq, int nseq);
// MTTKRP of a block against factors (device), result scale*mttkrp into out (ld = ldOut)
// `collective` = false: the block holds the whole tensor and the result is complete on this engine (op-level
// entry on an engine that happens to belong to a communicator)
// `tensor_pass` = true: always the tensor-pass kernels, also for blocks small enough for the one-launch kernel
// (the op-level entries, so that their parity tests exercise the pass kernels at every size)
void block_mttkrp(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, int R, double scale, double* out,
                  int64_t ldOut, bool use_cache, const int* update_seq, int nseq, bool collective = true,
                  bool tensor_pass = false, const SysBuild* sys = nullptr, bool* sys_done = nullptr);

}  // namespace aoadmm
