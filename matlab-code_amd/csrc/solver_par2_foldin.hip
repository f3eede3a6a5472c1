// Engine: the rows of C of new slabs of a PARAFAC2 block (par2_foldin.h).
#include "solver.h"
#include "par2_foldin.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace aoadmm {

int64_t Engine::par2_rows(int p) const {
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(tensors_[p].par2, "aoadmm_par2_rows: tensor %d is not a PARAFAC2 block", p);
  return tensors_[p].p2.I;
}

void Engine::par2_fold_in(int p, int64_t nk, const int64_t* cols, const double* X, const double* c0, const aoadmm_par2_foldin_options* opt,
                          double* C_host, double* B_host, double* P_host, double* res_host, double* xnorm_host, int* iters_host,
                          int* info_host, double* Y_host, double* sys_host, int* path_host) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  const TensorInfo& t = tensors_[p];
  AO_REQUIRE(t.par2, "aoadmm_resident_par2_fold_in: tensor %d is not a PARAFAC2 block", p);
  const Par2Block& b = t.p2;
  const ModeInfo& mA = modes_[t.modes[0]];
  AO_REQUIRE(mA.has_fac, "G.fac{%d} missing", t.modes[0] + 1);
  AO_REQUIRE(b.has_DeltaB, "DeltaB{%d} was never set", p + 1);
  AO_REQUIRE(nk >= 0 && nk < ((int64_t)1 << 31), "nk = %lld outside [0, 2^31)", (long long)nk);
  P2FoldinOptions fo;                                  // null: max_iter 50, tol 1e-8, ridge 0, no constraint
  if (opt != nullptr) {
    AO_REQUIRE(opt->max_iter >= 1, "max_iter = %d < 1", opt->max_iter);
    AO_REQUIRE(std::isfinite(opt->tol) && opt->tol >= 0.0, "tol = %g is negative or not finite", opt->tol);
    AO_REQUIRE(std::isfinite(opt->ridge) && opt->ridge >= 0.0, "ridge = %g is negative or not finite", opt->ridge);
    AO_REQUIRE(opt->constraint == 0 || opt->constraint == 1, "constraint = %d is neither 0 (none) nor 1 (non-negativity)", opt->constraint);
    AO_REQUIRE(opt->max_inner >= 1, "max_inner = %d < 1", opt->max_inner);
    AO_REQUIRE(opt->tol_primal >= 0.0 && opt->tol_dual >= 0.0, "negative tolerance (%g, %g)", opt->tol_primal, opt->tol_dual);
    fo.max_iter = opt->max_iter; fo.tol = opt->tol; fo.ridge = opt->ridge; fo.constraint = opt->constraint;
    fo.max_inner = opt->max_inner; fo.tol_primal = opt->tol_primal; fo.tol_dual = opt->tol_dual;
  }
  if (nk == 0) return;
  AO_REQUIRE(cols != nullptr && X != nullptr, "null cols / X");
  AO_REQUIRE(C_host != nullptr && res_host != nullptr && iters_host != nullptr && info_host != nullptr, "null C / res / iters / info");
  const int R = b.R, I = b.I;
  std::vector<int64_t> off((size_t)nk + 1, 0), item0((size_t)nk + 1, 0);
  int Jmax = 0;
  for (int64_t q = 0; q < nk; ++q) {
    AO_REQUIRE(cols[q] >= R, "slab %lld has %lld columns, fewer than R = %d", (long long)q, (long long)cols[q], R);
    AO_REQUIRE(cols[q] <= INT_MAX, "slab %lld has %lld columns: beyond the int range", (long long)q, (long long)cols[q]);
    off[(size_t)q + 1] = off[(size_t)q] + cols[q];
    AO_REQUIRE(off[(size_t)q + 1] <= INT_MAX, "the slabs have more than %d columns together", INT_MAX);
    // the kernels index a slab's J_q x R arrays, and the launcher the call's sum(J_q) x R ones, in int
    AO_REQUIRE(off[(size_t)q + 1] * R <= INT_MAX, "the slabs have more than %d / R columns together (R = %d)", INT_MAX, R);
    item0[(size_t)q + 1] = item0[(size_t)q] + cdiv(cols[q], kP2FoldTile);
    Jmax = std::max(Jmax, (int)cols[q]);
  }
  const int64_t Jtot = off[(size_t)nk], items = item0[(size_t)nk];
  const P2FoldinPath path = par2_foldin_path(I, R, Jmax, nk);
  AO_REQUIRE(items * path.chunks < ((int64_t)1 << 31), "%lld work items: too many for one call", (long long)(items * path.chunks));
  std::vector<int> item_q((size_t)items), item_g((size_t)items);
  for (int64_t q = 0; q < nk; ++q)
    for (int64_t i = item0[(size_t)q]; i < item0[(size_t)q + 1]; ++i) {
      item_q[(size_t)i] = (int)q;
      item_g[(size_t)i] = (int)(i - item0[(size_t)q]);
    }

  AO_HIP(hipSetDevice(device_));
  DevBuf dX, doff, dc0, diq, dig, di0, ypart, xpart, sys, ctl, W, Y, P, B, C, res, xn, it, info;
  auto up = [&](DevBuf& d, const void* src, size_t bytes) {
    d.alloc(std::max<size_t>(bytes, 8));
    if (bytes > 0) AO_HIP(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, stream_));
  };
  const size_t slab = (size_t)Jtot * R * sizeof(double);
  up(dX, X, (size_t)I * Jtot * sizeof(double));
  up(doff, off.data(), off.size() * sizeof(int64_t));
  if (c0 != nullptr) up(dc0, c0, (size_t)nk * R * sizeof(double));
  up(diq, item_q.data(), item_q.size() * sizeof(int));
  up(dig, item_g.data(), item_g.size() * sizeof(int));
  up(di0, item0.data(), item0.size() * sizeof(int64_t));
  if (path.chunks > 1) ypart.alloc(slab * path.chunks);
  xpart.alloc((size_t)items * path.chunks * sizeof(double));
  sys.alloc(par2_foldin_sys_doubles(R) * sizeof(double));
  ctl.alloc(sizeof(AdmmCtl));
  AO_HIP(hipMemsetAsync(ctl.p, 0, sizeof(AdmmCtl), stream_));
  if (!path.alt_lds) W.alloc(slab);
  Y.alloc(slab); P.alloc(slab); B.alloc(slab);
  C.alloc((size_t)nk * R * sizeof(double));
  res.alloc((size_t)nk * sizeof(double));
  xn.alloc((size_t)nk * sizeof(double));
  it.alloc((size_t)nk * sizeof(int));
  info.alloc((size_t)nk * sizeof(int));

  P2FoldinArgs a;
  a.I = I; a.R = R; a.Jmax = Jmax; a.nk = nk; a.Jtot = Jtot;
  const FactorRef fr = factor_ref(mA);
  a.A = fr.p; a.lda = fr.ld;
  a.DeltaB = b.DeltaB.d();
  a.X = dX.d(); a.off = doff.as<int64_t>(); a.c0 = c0 != nullptr ? dc0.d() : nullptr;
  a.opt = fo;
  a.items = items; a.item_q = diq.as<int>(); a.item_g = dig.as<int>(); a.item0 = di0.as<int64_t>();
  a.ypart = path.chunks > 1 ? ypart.d() : nullptr;
  a.xpart = xpart.d(); a.sys = sys.d(); a.ctl = ctl.as<AdmmCtl>();
  a.W = path.alt_lds ? nullptr : W.d();
  a.Y = Y.d(); a.P = P.d(); a.B = B.d(); a.C = C.d(); a.res = res.d(); a.xnorm = xn.d(); a.iters = it.as<int>(); a.info = info.as<int>();

  // The outputs are written last, and only after the device work has succeeded: a refusal or a failure leaves them
  // untouched.  Class 17 counts the call (launch, bytes, flops, its event pair) once the outputs have been read back: the
  // flops need the iterations the slabs took, and a call that fails -- a launch error, a shared system without a factor,
  // a failed read-back -- leaves the class as it was; its two events go back to the pool.
  KernelStats& ks = timers_.stats[kStatsPar2Foldin];
  AdmmCtl hctl;
  std::vector<double> hC((size_t)nk * R), hres((size_t)nk), hxn((size_t)nk), hB, hP, hY, hsys;
  std::vector<int> hit((size_t)nk), hinfo((size_t)nk);
  auto down = [&](void* dst, const DevBuf& d, size_t bytes) {
    AO_HIP(hipMemcpyAsync(dst, d.p, bytes, hipMemcpyDeviceToHost, stream_));
  };
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  try {
    par2_foldin_enqueue(a, stream_);
    if (pr.e0) AO_HIP(hipEventRecord(pr.e1, stream_));
    down(&hctl, ctl, sizeof(AdmmCtl));
    AO_HIP(hipStreamSynchronize(stream_));
    if (hctl.notpd) throw Error(AOADMM_ERR_NOT_PD, "aoadmm_resident_par2_fold_in: (A'A) .* (DeltaB'DeltaB) + shift I is not positive definite");
    down(hC.data(), C, hC.size() * sizeof(double));
    down(hres.data(), res, hres.size() * sizeof(double));
    down(hxn.data(), xn, hxn.size() * sizeof(double));
    down(hit.data(), it, hit.size() * sizeof(int));
    down(hinfo.data(), info, hinfo.size() * sizeof(int));
    if (B_host != nullptr) { hB.resize((size_t)Jtot * R); down(hB.data(), B, slab); }
    if (P_host != nullptr) { hP.resize((size_t)Jtot * R); down(hP.data(), P, slab); }
    if (Y_host != nullptr) { hY.resize((size_t)Jtot * R); down(hY.data(), Y, slab); }
    if (sys_host != nullptr) { hsys.resize((size_t)R * R); down(hsys.data(), sys, hsys.size() * sizeof(double)); }
    AO_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    if (pr.e0) { timers_.pool.push_back(pr.e0); timers_.pool.push_back(pr.e1); }
    throw;
  }
  double iter_cols = 0.0;
  for (int64_t q = 0; q < nk; ++q) iter_cols += (double)hit[(size_t)q] * (double)cols[q];
  timers_.count(ks, pr, par2_foldin_bytes(I, R, nk, Jtot), par2_foldin_flops(I, R, Jtot, iter_cols));
  std::copy(hC.begin(), hC.end(), C_host);
  std::copy(hres.begin(), hres.end(), res_host);
  std::copy(hit.begin(), hit.end(), iters_host);
  std::copy(hinfo.begin(), hinfo.end(), info_host);
  if (xnorm_host != nullptr) std::copy(hxn.begin(), hxn.end(), xnorm_host);
  if (B_host != nullptr) std::copy(hB.begin(), hB.end(), B_host);
  if (P_host != nullptr) std::copy(hP.begin(), hP.end(), P_host);
  if (Y_host != nullptr) std::copy(hY.begin(), hY.end(), Y_host);
  if (sys_host != nullptr) std::copy(hsys.begin(), hsys.end(), sys_host);
  if (path_host != nullptr) {
    path_host[0] = path.y_class();
    path_host[1] = path.alt_class();
  }
}

}  // namespace aoadmm
