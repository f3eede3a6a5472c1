// Engine: top-k completions of a CP block along one mode (topk.h).
#include "solver.h"
#include "topk.h"

#include <algorithm>

namespace aoadmm {

TensorInfo& Engine::query_block(const char* what, const char* purpose, int p, int mode, int64_t nq) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  if (t.par2) throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s: tensor %d is a PARAFAC2 block; %s", what, p, purpose));
  const int nd = t.nmodes;
  AO_REQUIRE(nd >= 2 && nd <= kCooMaxModes, "tensor %d: order %d", p, nd);
  AO_REQUIRE(mode >= 0 && mode < nd, "tensor %d: mode %d outside [0, %d)", p, mode, nd);
  AO_REQUIRE(nq >= 0 && nq < ((int64_t)1 << 31), "nq = %lld outside [0, 2^31)", (long long)nq);
  return t;
}

void Engine::check_excl(int p, int64_t I, int64_t nq, const int64_t* excl_off, const int64_t* excl_idx, std::vector<int>& ex32) const {
  AO_REQUIRE(excl_off[0] == 0, "excl_off[0] = %lld, not 0", (long long)excl_off[0]);
  for (int64_t q = 0; q < nq; ++q)
    AO_REQUIRE(excl_off[q + 1] >= excl_off[q], "excl_off decreases at query %lld", (long long)q);
  const int64_t ne = excl_off[nq];
  ex32.resize((size_t)ne);
  for (int64_t e = 0; e < ne; ++e) {
    AO_REQUIRE(excl_idx[e] >= 0 && excl_idx[e] < I, "tensor %d: excluded row %lld at position %lld is outside [0, %lld)", p,
               (long long)excl_idx[e], (long long)e, (long long)I);
    ex32[(size_t)e] = (int)excl_idx[e];
  }
}

void Engine::upload_w_rows(const double* W, int64_t nq, int R, std::vector<double>& rows, DevBuf& dev) {
  rows.resize((size_t)nq * R);
  for (int64_t q = 0; q < nq; ++q)
    for (int r = 0; r < R; ++r) rows[(size_t)q * R + r] = W[(size_t)r * nq + q];
  dev.alloc(rows.size() * sizeof(double));
  AO_HIP(hipMemcpyAsync(dev.p, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
}

void Engine::topk(int p, int mode, int64_t nq, const int64_t* subs, int k, const int64_t* excl_off, const int64_t* excl_idx,
                  int64_t* idx_host, double* val_host) {
  topk_run("aoadmm_resident_topk", p, mode, nq, subs, nullptr, k, excl_off, excl_idx, idx_host, val_host);
}

void Engine::topk_w(int p, int mode, int64_t nq, const double* W, int k, const int64_t* excl_off, const int64_t* excl_idx,
                    int64_t* idx_host, double* val_host) {
  topk_run("aoadmm_resident_topk_w", p, mode, nq, nullptr, W, k, excl_off, excl_idx, idx_host, val_host);
}

// subs (the weights are formed on the device) or W (nq x R column-major on the host, uploaded as it is: finite or not)
void Engine::topk_run(const char* what, int p, int mode, int64_t nq, const int64_t* subs, const double* W, int k, const int64_t* excl_off,
                      const int64_t* excl_idx, int64_t* idx_host, double* val_host) {
  const bool given = subs == nullptr && W != nullptr;
  TensorInfo& t = query_block(what, "top-k completions are for CP blocks", p, mode, nq);
  const int nd = t.nmodes;
  AO_REQUIRE(k >= 1 && k <= kTopkMax, "k = %d outside [1, %d]", k, kTopkMax);
  if (nq == 0) return;
  AO_REQUIRE((subs != nullptr || W != nullptr) && idx_host != nullptr && val_host != nullptr, "null subs / W / idx / val");
  AO_REQUIRE(excl_off == nullptr || excl_idx != nullptr || excl_off[nq] == 0, "null excl_idx");
  const int64_t I = modes_[t.modes[mode]].rows;

  // the free mode's column is ignored
  std::vector<int> idx32;
  if (!given) heldout_check_subs(t, p, nq, subs, idx32, mode);

  // the exclusion lists: checked, every list sorted before the upload
  std::vector<int> ex32;
  if (excl_off != nullptr) {
    check_excl(p, I, nq, excl_off, excl_idx, ex32);
    for (int64_t q = 0; q < nq; ++q) std::sort(ex32.begin() + excl_off[q], ex32.begin() + excl_off[q + 1]);
  }

  AO_HIP(hipSetDevice(device_));
  const HeldoutFactors hf = heldout_factors(t, nullptr);
  const TopkPlan pl = topk_plan(I, hf.R, nq, k);
  DevBuf idx, wgiven, eoff, eidx, ws, oidx, oval;
  idx.alloc(idx32.size() * sizeof(int));
  ws.alloc(pl.workspace_bytes);
  oidx.alloc((size_t)nq * k * sizeof(int64_t));
  oval.alloc((size_t)nq * k * sizeof(double));
  if (!given) AO_HIP(hipMemcpyAsync(idx.p, idx32.data(), idx32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  TopkArgs a;
  a.hf = hf; a.mode = mode; a.I = I; a.nq = nq; a.k = k;
  a.idx = idx.as<int>();
  std::vector<double> wrow;                            // the scores kernel reads W row-major
  if (given) {
    upload_w_rows(W, nq, hf.R, wrow, wgiven);
    a.W = wgiven.d();
  }
  if (excl_off != nullptr) {
    eoff.alloc((size_t)(nq + 1) * sizeof(int64_t));
    eidx.alloc(std::max<size_t>(1, ex32.size()) * sizeof(int));
    AO_HIP(hipMemcpyAsync(eoff.p, excl_off, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
    if (!ex32.empty()) AO_HIP(hipMemcpyAsync(eidx.p, ex32.data(), ex32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    a.excl_off = eoff.as<int64_t>();
    a.excl_idx = eidx.as<int>();
  }
  a.workspace = ws.p;
  a.out_idx = oidx.as<int64_t>();
  a.out_val = oval.d();
  KernelStats& ks = timers_.stats[kStatsTopk];
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  topk_enqueue(a, pl, stream_);
  timers_.end(ks, pr, stream_, topk_bytes(nd, hf.R, I, nq, k, pl), topk_flops(hf.R, I, nq));
  // (the outputs are written last: a refusal above leaves them untouched)
  AO_HIP(hipMemcpyAsync(idx_host, oidx.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipMemcpyAsync(val_host, oval.p, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

}  // namespace aoadmm
