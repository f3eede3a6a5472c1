// Engine: the missing entries of a masked dense CP block as a list (em_list.h).  The mark and
// the list, the pass a solve enqueues in place of the dense imputing pass, and the op-level call around it.
#include "solver.h"

namespace aoadmm {

void Engine::set_missing_list(int p, bool on) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  if (t.par2)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("the missing-entry list is for dense CP blocks: tensor %d is PARAFAC2", p));
  CpBlock& b = t.blk;
  if (b.sparse)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("the missing-entry list is for dense CP blocks: tensor %d holds sparse data (aoadmm_tensor_set_observed_only)", p));
  if (b.has_weights)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("the missing-entry list is not available for a block with per-entry weights (tensor %d)", p));
  if (world_ > 1 || multi_member_)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("the missing-entry list is not available under a communicator of %d ranks or on a multi-device context (tensor %d)", world_, p));
  AO_REQUIRE(b.has_data && b.has_mask, "tensor %d has no mask: upload Z.miss{%d} (aoadmm_tensor_mask_upload) before marking it", p, p + 1);
  if (!on) { b.mlist.clear(); return; }
  AO_HIP(hipSetDevice(device_));
  em_list_build(b.mlist, b.mask.as<uint8_t>(), b.nd, b.dims, b.X.pad0, stream_);   // throws with the block as it was
}

void Engine::missing_list(int p, int64_t* n, int64_t* subs) {
  require_usable();
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  const TensorInfo& t = tensors_[p];
  AO_REQUIRE(!t.par2 && t.blk.mlist.on, "tensor %d is not marked (aoadmm_tensor_set_missing_list)", p);
  const MissingList& l = t.blk.mlist;
  if (n) *n = l.n;
  if (!subs || l.n == 0) return;
  AO_HIP(hipSetDevice(device_));
  std::vector<int> h((size_t)l.n * l.nd);
  AO_HIP(hipMemcpyAsync(h.data(), l.idx.p, h.size() * sizeof(int), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  for (size_t q = 0; q < h.size(); ++q) subs[q] = h[q];
}

void Engine::em_list_enqueue(int p, int update, bool timed) {
  TensorInfo& t = tensors_[p];
  CpBlock& b = t.blk;
  const MissingList& l = b.mlist;
  AO_REQUIRE(l.on && b.has_mask && !b.x_released && l.nd == b.nd, "internal: list pass of tensor %d without its list", p);
  if (world_ > 1)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("tensor %d was marked with aoadmm_tensor_set_missing_list before the engine joined a communicator of %d ranks: unmark it", p, world_));
  EmListArgs a;
  a.idx = l.idx.as<int>(); a.n = l.n;
  a.hf = heldout_factors(t, nullptr);                 // the row-major factor copies when all are current, as the sparse passes do
  a.X = b.X.data.p;
  a.Xt = b.nd == 2 ? b.Xt.data.p : nullptr;
  int64_t st = 1;
  for (int m = 0; m < kCooMaxModes; ++m) {
    a.stride[m] = m < b.nd ? st : 0;
    st *= m == 0 ? b.X.pad0 : b.dims[m];
  }
  a.Jpad = b.nd == 2 ? b.Xt.pad0 : 0;
  a.update = update;
  a.part = l.part.d();
  KernelStats& ks = timers_.stats[kStatsEmList];
  const LaunchTimers::Pair pr = timed ? timers_.begin(ks, timers_.profile, stream_) : LaunchTimers::Pair();
  em_list_pass(a, b.X.prec, dev_.em(p) + kEmNum, dev_.em(p) + kEmDen, stream_);
  if (timed) timers_.end(ks, pr, stream_, em_list_pass_bytes(b.nd, a.hf.R, l.n, b.X.prec, update != 0), em_list_pass_flops(b.nd, a.hf.R, l.n));
  if (update) {
    b.mask_imputed = true;
    b.cached_mode = -1;                               // the data changed: cached partial contractions are stale
  }
}

void Engine::resident_em_list_pass(int p, int update, double stats2[2], double* data, double* data_t) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(stats2 != nullptr, "null stats");
  if (sharded()) throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_resident_em_list_pass runs on one engine without a communicator");
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(!t.par2 && t.blk.mlist.on, "tensor %d is not marked (aoadmm_tensor_set_missing_list)", p);
  for (int i = 0; i < t.nmodes; ++i) AO_REQUIRE(modes_[t.modes[i]].has_fac, "G.fac{%d} missing", t.modes[i] + 1);
  AO_HIP(hipSetDevice(device_));
  em_list_enqueue(p, update != 0, true);
  double h2[2];
  static_assert(kEmNum == 0 && kEmDen == 1, "num and den are the first two EM slots");
  AO_HIP(hipMemcpyAsync(h2, dev_.em(p), sizeof h2, hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  stats2[0] = h2[kEmNum]; stats2[1] = h2[kEmDen];
  CpBlock& b = t.blk;
  int64_t cols = 1;
  for (int i = 1; i < b.nd; ++i) cols *= b.dims[i];
  if (data) download_unpadded(b.X, b.dims[0], cols, data, stream_);
  if (data_t && b.nd == 2) download_unpadded(b.Xt, b.dims[1], b.dims[0], data_t, stream_);
}

}  // namespace aoadmm
