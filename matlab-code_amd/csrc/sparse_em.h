// Observed-only sparse CP blocks: the stored entries of a CooBlock are the observations, every other entry is missing
// and imputed by EM (functions/cmtf_fun_AOADMM.m:408-441) without a dense array.
//   imputed tensor = P_Omega(X) + P_Omega^c(M_old),  M_old = model of the factor snapshot Fo taken at the last EM step
//   MTTKRP_n       = sparse MTTKRP of the residuals (x - m_old) on Omega  +  Fo_n * had_{j != n}(Fo_j' F_j)
//   objective      = sum_Omega (x - m)^2 ;  f_rel_missing from num = ||P_Omega^c(M_new - M_old)||^2 (telescoped) and
//                    den = ||P_Omega^c(M_old)||^2
// Every sum has a fixed order (per-team partials, then one block): two runs return the same bits.
// Weighted form (aoadmm_tensor_set_entry_weights): stored entry e has a weight w_e in [0, 1],
// every unstored entry the weight alpha in [0, 1]; W is the dense array those define.
//   imputed tensor = W o X + (1 - W) o M_old
//   MTTKRP_n       = sparse MTTKRP of r_e = w_e x_e - (w_e - alpha) m_old,e  +  (1 - alpha) Fo_n * had_{j != n}(Fo_j' F_j)
//   objective      = sum_Omega w (x - m)^2 + alpha (||M||^2 - sum_Omega m^2)
//   num / den      = (1 - alpha)^2 (the unweighted ones) + sum_Omega (1 - w)^2 dm^2 / + sum_Omega (1 - w)^2 m_old^2
// A block without weights launches the kernels it launched before the weighted form existed.
#pragma once
#include "common.h"
#include "sparse.h"

namespace aoadmm {

// one factor of the block as the EM unit reads it: column-major (p, ld) and, when current, its row-major copy
struct SemFac {
  const double* p;
  int64_t ld;
  const double* pT;   // rows x R row-major, or null
};

struct SparseEm {
  bool on = false;          // aoadmm_tensor_set_observed_only
  bool have_snap = false;   // an EM step has been taken since the flag was set / the solve began
  int nd = 0, R = 0;
  int64_t nnz = 0;
  int64_t dims[kCooMaxModes] = {0};
  DevBuf res[kCooMaxModes];     // x - m_old in the order of mode n's copy (fp64 [nnz]); weighted: w x - (w - alpha) m_old
  bool weighted = false;        // aoadmm_tensor_set_entry_weights
  double alpha = 0.0;           // weight of every unstored entry
  double wnormsq = 0.0;         // sum_Omega w x^2
  DevBuf wt[kCooMaxModes];      // w in the order of mode n's copy (fp64 [nnz]); absent: every stored weight is 1
  DevBuf snapC[kCooMaxModes];   // Fo_n column-major (dims[n] x R, ld = dims[n])
  DevBuf snapR[kCooMaxModes];   // Fo_n row-major (the pass gathers it)
  // R x R matrices per mode: [0] Fo'Fo, [1] F'F, [2] D'D, [3] D'Fo, [4] Fo'F of the last MTTKRP; then W (R x R)
  DevBuf small;
  DevBuf D;                     // F_n - Fo_n, one mode at a time
  DevBuf part;                  // kSemSums sums per team of the statistics pass
  DevBuf ws;                    // partials of the R x R products
  DevBuf hold;                  // [0]: ||P_Omega^c(M_old)||^2, the next step's den
  double* mat(int which, int n) const { return small.d() + ((size_t)which * kCooMaxModes + n) * R * R; }
  double* W() const { return small.d() + (size_t)5 * kCooMaxModes * R * R; }
  void clear() { *this = SparseEm(); }
  SparseEm() = default;
  SparseEm(SparseEm&&) = default;
  SparseEm& operator=(SparseEm&&) = default;
};

constexpr int kSemSums = 3;     // sum (x-m)^2, sum m^2, sum dm^2 per team
constexpr int kSemSumsW = 5;    // weighted: sum w (x-m)^2, sum m^2, sum (1-w)^2 m^2, sum dm^2, sum (1-w)^2 dm^2

// marks the block observed-only for rank R and allocates the residual arrays and the snapshots; the weights of a block
// that has some stay (sem_reset included)
void sem_enable(SparseEm& e, const CooBlock& b, int R, hipStream_t s);
// Weights for a marked block.  wts (or null: stored weights 1) is a CooBlock built from the caller's list with the
// weights as values; its subscript arrays must equal b's (AOADMM_ERR_INVALID otherwise, e untouched) and its value
// arrays become e.wt.  Ends with sem_reset.
void sem_check_weight_list(const CooBlock& b, const CooBlock& wts, hipStream_t s);
void sem_set_weights(SparseEm& e, const CooBlock& b, CooBlock* wts, double alpha, hipStream_t s);
// forgets the snapshot: the next MTTKRP is that of the starting point (weighted: res = w o x, the MTTKRP of W o X)
void sem_reset(SparseEm& e, const CooBlock& b, hipStream_t s);
// bytes that stay resident for the flag: the residual arrays, the weights and the snapshots
int64_t sem_resident_bytes(const SparseEm& e);

// One EM step with the factors f[0..nd) (mode order), in three parts so that the caller can time the passes:
//   sem_step_begin   D_n = F_n - Fo_n, D_n'D_n and D_n'Fo_n while the old snapshot is there
//   sem_step_pass    the pass over mode pos's copy: residuals x - m; pos = 0 also leaves the statistics' partial sums
//   sem_step_finish  em[kEmObsRes] = sum_Omega (x - m)^2, em[kEmNum], em[kEmDen] (device, the block's EM slots), then
//                    the snapshot
// stats_only: the pass over the first copy and em[kEmObsRes] alone, no residuals and no snapshot (the objective of the
// starting point).
void sem_step_begin(SparseEm& e, const CooBlock& b, const SemFac* f, bool stats_only, hipStream_t s);
void sem_step_pass(SparseEm& e, const CooBlock& b, const SemFac* f, int pos, bool stats_only, hipStream_t s);
void sem_step_finish(SparseEm& e, const SemFac* f, bool stats_only, double* em, hipStream_t s);

// out(:, 0:R-1) += scale * (1 - alpha) * Fo_pos * had_{j != pos}(Fo_j' F_j), after coo_mttkrp over e.res[pos] wrote the
// sparse part (alpha = 0 without weights)
void sem_mttkrp_correct(SparseEm& e, int pos, const SemFac* f, double scale, double* out, int64_t ldOut, hipStream_t s);

// algorithmic bytes and flops of one residual pass (stats: the statistics pass of the mode-1 copy with a snapshot)
double sem_pass_bytes(const SparseEm& e, bool stats, bool with_snapshot, bool writes);
double sem_pass_flops(const SparseEm& e, bool stats, bool with_snapshot);

}  // namespace aoadmm
