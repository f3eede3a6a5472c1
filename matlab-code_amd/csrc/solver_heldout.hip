// Engine: held-out scoring (heldout.h).  The list of a block, the model at a list of subscripts,
// the pass a solve enqueues with every evaluation of the objective, and the trace it leaves.
#include "solver.h"

#include <cmath>

namespace aoadmm {

bool Engine::has_heldout() const {
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].ho.n > 0) return true;
  return false;
}

// The current fac state of the block's modes.  The row-major copies of the Gram kernel serve when every one of them is
// current (inside a solve they are), the column-major factors otherwise; the B_k slabs of a PARAFAC2 block have no such
// copy and are always gathered as par2.h stores them.
HeldoutFactors Engine::heldout_factors(const TensorInfo& t, bool* row_major) const {
  HeldoutFactors hf;
  hf.nd = t.nmodes;
  hf.R = modes_[t.modes[0]].R;
  bool all_current = true;
  for (int i = 0; i < t.nmodes; ++i) {
    const ModeInfo& o = modes_[t.modes[i]];
    AO_REQUIRE(o.has_fac, "G.fac{%d} missing", t.modes[i] + 1);
    if (!o.slabs && factor_ref(o).pT == nullptr) all_current = false;
  }
  for (int i = 0; i < t.nmodes; ++i) {
    const ModeInfo& o = modes_[t.modes[i]];
    if (o.slabs) { hf.f[i] = CooFactor{o.fac.d(), 1, 0}; continue; }
    const FactorRef fr = factor_ref(o);
    hf.f[i] = all_current ? CooFactor{fr.pT, (int64_t)hf.R, 1} : CooFactor{fr.p, 1, fr.ld};
  }
  if (t.par2) hf.off = t.p2.off_d.as<int64_t>();   // K + 1 prefix sums of J_k, on the device since add_par2
  if (row_major) *row_major = all_current;
  return hf;
}

// subs: column-major n x N int64, 0-based -> idx32 in the same layout.  A subscript out of range is AOADMM_ERR_INVALID.
void Engine::heldout_check_subs(const TensorInfo& t, int p, int64_t n, const int64_t* subs, std::vector<int>& idx32) const {
  const int nd = t.nmodes;
  AO_REQUIRE(nd >= 2 && nd <= kCooMaxModes, "tensor %d: order %d", p, nd);
  idx32.resize((size_t)nd * n);
  for (int m = 0; m < nd; ++m) {
    const ModeInfo& mi = modes_[t.modes[m]];
    if (mi.slabs) continue;                          // the slab-valued mode is checked against J_k below
    AO_REQUIRE(mi.rows < ((int64_t)1 << 31), "tensor %d: mode %d too long for int32 subscripts", p, m);
    const int64_t* col = subs + (int64_t)m * n;
    for (int64_t e = 0; e < n; ++e) {
      AO_REQUIRE(col[e] >= 0 && col[e] < mi.rows, "tensor %d: subscript %lld of mode %d at entry %lld is outside [0, %lld)", p,
                 (long long)col[e], m, (long long)e, (long long)mi.rows);
      idx32[(size_t)m * n + e] = (int)col[e];
    }
  }
  if (t.par2) {
    const ModeInfo& mB = modes_[t.modes[1]];
    const int64_t* cj = subs + n;
    for (int64_t e = 0; e < n; ++e) {
      const int64_t Jk = mB.rows_k[idx32[(size_t)2 * n + e]];
      AO_REQUIRE(cj[e] >= 0 && cj[e] < Jk, "tensor %d: subscript %lld of mode 1 at entry %lld is outside slab %d of %lld rows", p,
                 (long long)cj[e], (long long)e, idx32[(size_t)2 * n + e], (long long)Jk);
      idx32[(size_t)n + e] = (int)cj[e];
    }
  }
}

void Engine::model_at(int p, int64_t n, const int64_t* subs, double* out_host) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(n >= 0, "n = %lld < 0", (long long)n);
  if (n == 0) return;
  AO_REQUIRE(subs != nullptr && out_host != nullptr, "null subs / out");
  TensorInfo& t = tensors_[p];
  std::vector<int> idx32;
  heldout_check_subs(t, p, n, subs, idx32);
  AO_HIP(hipSetDevice(device_));
  bool row_major = false;
  const HeldoutFactors hf = heldout_factors(t, &row_major);
  t.ho_row_major = row_major ? 1 : 0;
  DevBuf idx, out;
  idx.alloc(idx32.size() * sizeof(int));
  out.alloc((size_t)n * sizeof(double));
  AO_HIP(hipMemcpyAsync(idx.p, idx32.data(), idx32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  KernelStats& ks = timers_.stats[kStatsHeldout];
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  heldout_model_at(hf, idx.as<int>(), n, out.d(), stream_);
  timers_.end(ks, pr, stream_, heldout_pass_bytes(hf.nd, hf.R, n, false), heldout_pass_flops(hf.nd, hf.R, n, false));
  AO_HIP(hipMemcpyAsync(out_host, out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

void Engine::set_heldout(int p, int64_t n, const int64_t* subs, const double* vals) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n = %lld outside [0, 2^31)", (long long)n);
  TensorInfo& t = tensors_[p];
  if (n == 0) { t.ho.clear(); return; }
  AO_REQUIRE(subs != nullptr && vals != nullptr, "null subs / vals");
  std::vector<int> idx32;
  heldout_check_subs(t, p, n, subs, idx32);            // the previous list stays when anything below throws
  for (int64_t e = 0; e < n; ++e)
    AO_REQUIRE(std::isfinite(vals[e]), "tensor %d: held-out value %lld is not finite", p, (long long)e);
  AO_HIP(hipSetDevice(device_));
  HeldoutList l;
  l.nd = t.nmodes; l.n = n;
  l.idx.alloc(idx32.size() * sizeof(int));
  l.val.alloc((size_t)n * sizeof(double));
  l.part.alloc((size_t)kHeldoutSums * heldout_teams(n) * sizeof(double));
  AO_HIP(hipMemcpyAsync(l.idx.p, idx32.data(), idx32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipMemcpyAsync(l.val.p, vals, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  t.ho = std::move(l);
}

void Engine::heldout_enqueue(int p, double* sums) {
  TensorInfo& t = tensors_[p];
  bool row_major = false;
  const HeldoutFactors hf = heldout_factors(t, &row_major);
  KernelStats& ks = timers_.stats[kStatsHeldout];
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  heldout_stats_enqueue(hf, t.ho.idx.as<int>(), t.ho.val.d(), t.ho.n, t.ho.part.d(), sums, stream_);
  timers_.end(ks, pr, stream_, heldout_pass_bytes(hf.nd, hf.R, t.ho.n, true), heldout_pass_flops(hf.nd, hf.R, t.ho.n, true));
  t.ho_row_major = row_major ? 1 : 0;
}

void Engine::heldout_stats(int p, double stats[4]) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(stats != nullptr, "null stats");
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(t.ho.n > 0, "tensor %d has no held-out list (aoadmm_tensor_set_heldout)", p);
  AO_HIP(hipSetDevice(device_));
  heldout_enqueue(p, dev_.heldout(p));
  double h[kHeldoutSums];
  AO_HIP(hipMemcpyAsync(h, dev_.heldout(p), sizeof h, hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  stats[0] = h[kHoRes]; stats[1] = h[kHoY2]; stats[2] = h[kHoM2]; stats[3] = (double)t.ho.n;
}

void Engine::heldout_info(int p, int64_t* n, int64_t* resident_bytes, int* row_major) const {
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  const HeldoutList& l = tensors_[p].ho;
  if (n) *n = l.n;
  if (resident_bytes) *resident_bytes = l.resident_bytes();
  if (row_major) *row_major = tensors_[p].ho_row_major;
}

void Engine::heldout_trace(int p, double* out, int cap, int* len, int* best_iter) const {
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(cap >= 0 && (cap == 0 || out != nullptr), "null trace buffer");
  const std::vector<double>& tr = tensors_[p].ho_trace;
  for (int i = 0; i < cap && i < (int)tr.size(); ++i) out[i] = tr[i];
  if (len) *len = (int)tr.size();
  if (best_iter) *best_iter = tr.empty() ? -1 : ho_best_iter_;
}

}  // namespace aoadmm
