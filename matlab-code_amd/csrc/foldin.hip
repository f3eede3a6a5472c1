// Fold-in of new rows along one mode of a CP block: the unweighted instantiations of the kernel (foldin_dev.h), the plan
// of a call and its launches.  See foldin.h and DESIGN.md section 9.6.
#include <algorithm>
#include <cmath>

#include "foldin_dev.h"

namespace aoadmm {

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
FoldinPlan foldin_plan(int64_t nq, int64_t nobs, const int64_t* qcol) {
  FoldinPlan pl;
  pl.nq = nq; pl.nobs = nobs;
  pl.qoff.assign((size_t)nq + 1, 0);
  for (int64_t e = 0; e < nobs; ++e) pl.qoff[(size_t)qcol[e] + 1] += 1;
  for (int64_t q = 0; q < nq; ++q) pl.qoff[(size_t)q + 1] += pl.qoff[(size_t)q];
  // stable: the caller's order inside a query is the summation order
  std::vector<int64_t> cursor(pl.qoff.begin(), pl.qoff.end() - 1);
  pl.order.resize((size_t)nobs);
  for (int64_t e = 0; e < nobs; ++e) pl.order[(size_t)cursor[(size_t)qcol[e]]++] = e;
  // the cut of a query into chunks depends on its own count alone
  pl.pbase.assign((size_t)nq, -1);
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t n = pl.qoff[(size_t)q + 1] - pl.qoff[(size_t)q];
    const int64_t chunks = std::max<int64_t>(1, cdiv(n, kFoldChunk));
    if (chunks > 1) {
      pl.pbase[(size_t)q] = pl.partials;
      pl.partials += chunks;
      pl.split_q.push_back((int)q);
    }
    for (int64_t ch = 0; ch < chunks; ++ch) {
      pl.item_q.push_back((int)q);
      pl.item_chunk.push_back((int)ch);
    }
  }
  return pl;
}

void foldin_enqueue(const FoldinArgs& a, hipStream_t s) {
  const int R = a.hf.R, nd = a.hf.nd;
  AO_REQUIRE(R >= 1 && R <= kMaxRank && nd >= 2 && nd <= kCooMaxModes && a.hf.off == nullptr, "internal: fold-in pass of rank %d, order %d", R, nd);
  AO_REQUIRE(a.mode >= 0 && a.mode < nd && a.nq > 0 && a.nq < ((int64_t)1 << 31) && a.nobs >= 0, "internal: fold-in pass of mode %d", a.mode);
  AO_REQUIRE(a.items >= a.nq && a.items < ((int64_t)1 << 31) && a.splits >= 0 && a.splits <= a.nq, "internal: fold-in plan");
  AO_REQUIRE(a.idx && a.val && a.qoff && a.item_q && a.item_chunk && a.pbase && a.rows && a.info && a.iters, "internal: fold-in buffers");
  AO_REQUIRE(a.splits == 0 || (a.split_q != nullptr && a.partial != nullptr), "internal: fold-in partials");
  AO_REQUIRE(a.weighted || (a.wts == nullptr && a.alpha == 0.0), "internal: fold-in weights on the unweighted pass");
  AO_REQUIRE(a.alpha >= 0.0 && a.alpha <= 1.0 && (a.alpha == 0.0 || (a.H != nullptr && a.gram_ws != nullptr)), "internal: fold-in unstored weight");
  FoldKArgsW ka;
  int j = 0;
  for (int m = 0; m < nd; ++m)
    if (m != a.mode) ka.f[j++] = a.hf.f[m];
  for (; j < kCooMaxModes - 1; ++j) ka.f[j] = CooFactor{nullptr, 0, 0};
  ka.nm = nd - 1; ka.R = R;
  ka.nq = a.nq; ka.nobs = a.nobs;
  ka.ridge = a.opt.ridge; ka.tol_primal = a.opt.tol_primal; ka.tol_dual = a.opt.tol_dual;
  ka.constraint = a.opt.constraint; ka.max_inner = a.opt.max_inner;
  ka.idx = a.idx; ka.val = a.val; ka.qoff = a.qoff;
  ka.item_q = a.item_q; ka.item_chunk = a.item_chunk; ka.pbase = a.pbase; ka.split_q = a.split_q;
  ka.partial = a.partial; ka.rows = a.rows; ka.info = a.info; ka.iters = a.iters; ka.gram = a.gram; ka.rhs = a.rhs;
  ka.wt = a.wts; ka.alpha = a.alpha; ka.H = a.H;
  if (!a.weighted) {                             // the kernels of aoadmm_resident_fold_in, as they were
    launch_foldin_class<false>(ka, a.items, a.splits, s);
    return;
  }
  if (a.alpha != 0.0) foldin_gram_enqueue(a.hf, a.frows, a.mode, a.gram_ws, a.H, s);
  foldin_launch_weighted(ka, a.items, a.splits, s);
}

double foldin_bytes(int nd, int R, int64_t nq, int64_t nobs, bool normal, bool wts, double alpha, int64_t other_rows) {
  return (double)nobs * (4.0 * (nd - 1) + 8.0) + (double)nobs * (nd - 1) * 8.0 * R + (double)nq * (8.0 * R + 8.0) +
         (normal ? (double)nq * 8.0 * ((double)R * R + R) : 0.0) + (wts ? 8.0 * (double)nobs : 0.0) +
         (alpha != 0.0 ? 8.0 * R * (double)other_rows : 0.0);
}

double foldin_flops(int nd, int R, int64_t nq, int64_t nobs, double alpha, int64_t other_rows) {
  return (double)nobs * ((double)R * (R + 1) + 2.0 * R * (nd - 1)) + (double)nq * ((double)R * R * R / 3.0 + 2.0 * R * R) +
         (alpha != 0.0 ? (double)R * R * (double)other_rows : 0.0);
}

}  // namespace aoadmm
