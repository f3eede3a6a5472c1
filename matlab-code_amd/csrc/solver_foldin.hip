// Engine: new rows of a CP block along one mode from their entries (foldin.h).
#include "solver.h"
#include "foldin.h"

#include <algorithm>
#include <cmath>

namespace aoadmm {

int Engine::tensor_rank(int p) const {
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  return modes_[tensors_[p].modes[0]].R;
}

void Engine::fold_in(int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals,
                     const aoadmm_foldin_options* opt, double* rows_host, int* info_host, int* iters_host, double* gram_host,
                     double* rhs_host) {
  fold_in_run("aoadmm_resident_fold_in", false, p, mode, nq, nobs, subs, vals, nullptr, 0.0, opt, rows_host, info_host, iters_host,
              gram_host, rhs_host);
}

void Engine::fold_in_w(int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals, const double* wts,
                       double unstored_weight, const aoadmm_foldin_options* opt, double* rows_host, int* info_host, int* iters_host,
                       double* gram_host, double* rhs_host) {
  fold_in_run("aoadmm_resident_fold_in_w", true, p, mode, nq, nobs, subs, vals, wts, unstored_weight, opt, rows_host, info_host,
              iters_host, gram_host, rhs_host);
}

// One implementation for both entries.  weighted: the weighted instantiations of the kernel run (wts null: ones); the
// unweighted entry passes wts = null and alpha = 0 and launches what it always launched.
void Engine::fold_in_run(const char* what, bool weighted, int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs,
                         const double* vals, const double* wts, double alpha, const aoadmm_foldin_options* opt, double* rows_host,
                         int* info_host, int* iters_host, double* gram_host, double* rhs_host) {
  TensorInfo& t = query_block(what, "rows are folded into CP blocks", p, mode, nq);
  const int nd = t.nmodes;
  AO_REQUIRE(nobs >= 0, "nobs = %lld < 0", (long long)nobs);
  FoldinOptions fo;                                    // null: ridge 0, no constraint
  if (opt != nullptr) {
    AO_REQUIRE(std::isfinite(opt->ridge) && opt->ridge >= 0.0, "ridge = %g is negative or not finite", opt->ridge);
    AO_REQUIRE(opt->constraint == 0 || opt->constraint == 1, "constraint = %d is neither 0 (none) nor 1 (non-negativity)", opt->constraint);
    AO_REQUIRE(opt->max_inner >= 1, "max_inner = %d < 1", opt->max_inner);
    AO_REQUIRE(opt->tol_primal >= 0.0 && opt->tol_dual >= 0.0, "negative tolerance (%g, %g)", opt->tol_primal, opt->tol_dual);
    fo.ridge = opt->ridge; fo.constraint = opt->constraint; fo.max_inner = opt->max_inner;
    fo.tol_primal = opt->tol_primal; fo.tol_dual = opt->tol_dual;
  }
  // the convention of aoadmm_tensor_set_entry_weights: weights in [0, 1], the caller normalises and scales ridge with it
  AO_REQUIRE(std::isfinite(alpha) && alpha >= 0.0 && alpha <= 1.0, "unstored_weight = %g outside [0, 1]", alpha);
  if (nq == 0) return;
  AO_REQUIRE(rows_host != nullptr && info_host != nullptr, "null rows / info");
  AO_REQUIRE(nobs == 0 || (subs != nullptr && vals != nullptr), "null subs / vals");

  // the query column against nq, the others against the block's modes, in place
  const int64_t* qcol = subs + (int64_t)mode * nobs;
  for (int64_t e = 0; e < nobs; ++e)
    AO_REQUIRE(qcol[e] >= 0 && qcol[e] < nq, "tensor %d: query number %lld at observation %lld is outside [0, %lld)", p, (long long)qcol[e],
               (long long)e, (long long)nq);
  std::vector<int> idx32;
  heldout_check_subs(t, p, nobs, subs, idx32, mode);
  if (wts != nullptr)
    for (int64_t e = 0; e < nobs; ++e)
      AO_REQUIRE(std::isfinite(wts[e]) && wts[e] >= 0.0 && wts[e] <= 1.0, "tensor %d: weight %g at observation %lld is outside [0, 1]", p, wts[e],
                 (long long)e);

  // the observations in a stable order by query: 4 (N - 1) + 8 bytes each
  const FoldinPlan pl = foldin_plan(nq, nobs, qcol);
  std::vector<int> idx_sorted((size_t)(nd - 1) * nobs);
  std::vector<double> val_sorted((size_t)nobs);
  for (int m = 0, j = 0; m < nd; ++m) {
    if (m == mode) continue;
    const int* src = idx32.data() + (size_t)m * nobs;
    int* dst = idx_sorted.data() + (size_t)j * nobs;
    for (int64_t e = 0; e < nobs; ++e) dst[e] = src[pl.order[(size_t)e]];
    ++j;
  }
  for (int64_t e = 0; e < nobs; ++e) val_sorted[(size_t)e] = vals[pl.order[(size_t)e]];
  std::vector<double> wt_sorted;                       // beside the values: 8 bytes more per observation
  if (wts != nullptr) {
    wt_sorted.resize((size_t)nobs);
    for (int64_t e = 0; e < nobs; ++e) wt_sorted[(size_t)e] = wts[pl.order[(size_t)e]];
  }

  AO_HIP(hipSetDevice(device_));
  const HeldoutFactors hf = heldout_factors(t, nullptr);
  const int R = hf.R;
  const int64_t items = (int64_t)pl.item_q.size(), splits = (int64_t)pl.split_q.size();
  AO_REQUIRE(items < ((int64_t)1 << 31), "%lld work items: too many for one call", (long long)items);
  const bool normal = gram_host != nullptr || rhs_host != nullptr;
  DevBuf idx, val, wt, qoff, iq, ic, pbase, sq, part, orow, oinfo, oit, ogram, orhs, had, gws;
  auto up = [&](DevBuf& b, const void* src, size_t bytes) {
    b.alloc(std::max<size_t>(bytes, 8));
    if (bytes > 0) AO_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, stream_));
  };
  up(idx, idx_sorted.data(), idx_sorted.size() * sizeof(int));
  up(val, val_sorted.data(), val_sorted.size() * sizeof(double));
  if (wts != nullptr) up(wt, wt_sorted.data(), wt_sorted.size() * sizeof(double));
  up(qoff, pl.qoff.data(), pl.qoff.size() * sizeof(int64_t));
  up(iq, pl.item_q.data(), pl.item_q.size() * sizeof(int));
  up(ic, pl.item_chunk.data(), pl.item_chunk.size() * sizeof(int));
  up(pbase, pl.pbase.data(), pl.pbase.size() * sizeof(int64_t));
  up(sq, pl.split_q.data(), pl.split_q.size() * sizeof(int));
  part.alloc(std::max<size_t>((size_t)pl.partials * pl.partial_doubles(R) * sizeof(double), 8));
  orow.alloc((size_t)nq * R * sizeof(double));
  oinfo.alloc((size_t)nq * sizeof(int));
  oit.alloc((size_t)nq * sizeof(int));
  if (gram_host != nullptr) ogram.alloc((size_t)nq * R * R * sizeof(double));
  if (rhs_host != nullptr) orhs.alloc((size_t)nq * R * sizeof(double));

  FoldinArgs a;
  a.hf = hf; a.mode = mode; a.nq = nq; a.nobs = nobs; a.opt = fo;
  a.idx = idx.as<int>(); a.val = val.d(); a.qoff = qoff.as<int64_t>();
  a.item_q = iq.as<int>(); a.item_chunk = ic.as<int>(); a.pbase = pbase.as<int64_t>(); a.split_q = sq.as<int>();
  a.items = items; a.splits = splits;
  a.partial = part.d();
  a.rows = orow.d(); a.info = oinfo.as<int>(); a.iters = oit.as<int>();
  a.gram = gram_host != nullptr ? ogram.d() : nullptr;
  a.rhs = rhs_host != nullptr ? orhs.d() : nullptr;
  a.weighted = weighted; a.wts = wts != nullptr ? wt.d() : nullptr; a.alpha = alpha;
  int64_t other_rows = 0;
  if (alpha != 0.0) {                                  // H from the factors of this call, never from a Gram matrix a solve left
    for (int m = 0; m < nd; ++m) {
      a.frows[m] = modes_[t.modes[m]].rows;
      if (m != mode) other_rows += a.frows[m];
    }
    had.alloc((size_t)R * R * sizeof(double));
    gws.alloc(foldin_gram_ws_doubles(hf, a.frows, mode) * sizeof(double));
    a.H = had.d(); a.gram_ws = gws.d();
  }
  KernelStats& ks = timers_.stats[kStatsFoldin];
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  foldin_enqueue(a, stream_);
  timers_.end(ks, pr, stream_, foldin_bytes(nd, R, nq, nobs, normal, wts != nullptr, alpha, other_rows),
              foldin_flops(nd, R, nq, nobs, alpha, other_rows));
  // The outputs are written last, and only after the device work has succeeded: a refusal or a failure above leaves
  // them untouched.
  std::vector<double> hrow((size_t)nq * R), hgram, hrhs;
  std::vector<int> hinfo((size_t)nq), hit((size_t)nq);
  AO_HIP(hipMemcpyAsync(hrow.data(), orow.p, hrow.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipMemcpyAsync(hinfo.data(), oinfo.p, hinfo.size() * sizeof(int), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipMemcpyAsync(hit.data(), oit.p, hit.size() * sizeof(int), hipMemcpyDeviceToHost, stream_));
  if (gram_host != nullptr) {
    hgram.resize((size_t)nq * R * R);
    AO_HIP(hipMemcpyAsync(hgram.data(), ogram.p, hgram.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
  }
  if (rhs_host != nullptr) {
    hrhs.resize((size_t)nq * R);
    AO_HIP(hipMemcpyAsync(hrhs.data(), orhs.p, hrhs.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
  }
  AO_HIP(hipStreamSynchronize(stream_));
  std::copy(hrow.begin(), hrow.end(), rows_host);
  std::copy(hinfo.begin(), hinfo.end(), info_host);
  if (iters_host != nullptr) std::copy(hit.begin(), hit.end(), iters_host);
  if (gram_host != nullptr) std::copy(hgram.begin(), hgram.end(), gram_host);
  if (rhs_host != nullptr) std::copy(hrhs.begin(), hrhs.end(), rhs_host);
}

}  // namespace aoadmm
