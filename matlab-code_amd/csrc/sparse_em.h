// Observed-only sparse CP blocks: the stored entries of a CooBlock are the observations, every other entry is missing
// and imputed by EM (functions/cmtf_fun_AOADMM.m:408-441) without a dense array.
//   imputed tensor = P_Omega(X) + P_Omega^c(M_old),  M_old = model of the factor snapshot Fo taken at the last EM step
//   MTTKRP_n       = sparse MTTKRP of the residuals (x - m_old) on Omega  +  Fo_n * had_{j != n}(Fo_j' F_j)
//   objective      = sum_Omega (x - m)^2 ;  f_rel_missing from num = ||P_Omega^c(M_new - M_old)||^2 (telescoped) and
//                    den = ||P_Omega^c(M_old)||^2
// Every sum has a fixed order (per-team partials, then one block): two runs return the same bits.
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
  DevBuf res[kCooMaxModes];     // x - m_old in the order of mode n's copy (fp64 [nnz])
  DevBuf snapC[kCooMaxModes];   // Fo_n column-major (dims[n] x R, ld = dims[n])
  DevBuf snapR[kCooMaxModes];   // Fo_n row-major (the pass gathers it)
  // R x R matrices per mode: [0] Fo'Fo, [1] F'F, [2] D'D, [3] D'Fo, [4] Fo'F of the last MTTKRP; then W (R x R)
  DevBuf small;
  DevBuf D;                     // F_n - Fo_n, one mode at a time
  DevBuf part;                  // 3 sums per team of the statistics pass
  DevBuf ws;                    // partials of the R x R products
  DevBuf hold;                  // [0]: ||P_Omega^c(M_old)||^2, the next step's den
  double* mat(int which, int n) const { return small.d() + ((size_t)which * kCooMaxModes + n) * R * R; }
  double* W() const { return small.d() + (size_t)5 * kCooMaxModes * R * R; }
  void clear() { *this = SparseEm(); }
  SparseEm() = default;
  SparseEm(SparseEm&&) = default;
  SparseEm& operator=(SparseEm&&) = default;
};

// marks the block observed-only for rank R and allocates the residual arrays and the snapshots
void sem_enable(SparseEm& e, const CooBlock& b, int R);
// bytes that stay resident for the flag: the residual arrays and the snapshots
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

// out(:, 0:R-1) += scale * Fo_pos * had_{j != pos}(Fo_j' F_j), after coo_mttkrp over e.res[pos] wrote the sparse part
void sem_mttkrp_correct(SparseEm& e, int pos, const SemFac* f, double scale, double* out, int64_t ldOut, hipStream_t s);

// algorithmic bytes and flops of one residual pass (stats: the statistics pass of the mode-1 copy with a snapshot)
double sem_pass_bytes(const SparseEm& e, bool stats, bool with_snapshot, bool writes);
double sem_pass_flops(const SparseEm& e, bool stats, bool with_snapshot);

}  // namespace aoadmm
