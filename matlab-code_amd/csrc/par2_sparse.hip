// PARAFAC2 blocks with sparse slabs -- see par2_sparse.h.  The passes over the nonzeros are coo_mttkrp (sparse.hip) on
// the 2-way matrix Xcat; the kernels here are the dense Jtot x R and per-slab pieces around them.
#include "par2_sparse.h"

#include <algorithm>

#include "device_utils.h"

namespace aoadmm {

// xn[k] = sum of squares of the coalesced values of slab k.  `col` is the column-sorted copy's key array (global
// column of every nonzero), so slab k is the contiguous range [lower_bound(off[k]), lower_bound(off[k+1])).  One
// workgroup per slab, strided partial sums folded by a fixed tree: the same bits every run.
__global__ __launch_bounds__(256) void par2s_slab_normsq_k(const int* col, const double* val, int64_t nnz, P2Dims d,
                                                           double* xn) {
  __shared__ double red[256];
  const int k = blockIdx.x;
  int64_t range[2];
  for (int e = 0; e < 2; ++e) {
    const int64_t key = d.off[k + e];
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (col[mid] < key) lo = mid + 1; else hi = mid;
    }
    range[e] = lo;
  }
  double acc = 0.0;
  for (int64_t i = range[0] + threadIdx.x; i < range[1]; i += blockDim.x) acc += val[i] * val[i];
  acc = block_sum_pow2(acc, red);
  if (threadIdx.x == 0) xn[k] = acc;
}

void par2s_build(Par2Sparse& sp, const P2Dims& d, int64_t nnz, const int64_t* subs, const double* vals, hipStream_t s) {
  AO_REQUIRE(nnz >= 0, "sparse PARAFAC2 slabs: nnz = %lld < 0", (long long)nnz);
  AO_REQUIRE(nnz == 0 || (subs != nullptr && vals != nullptr), "sparse PARAFAC2 slabs: null subs / vals");
  AO_REQUIRE(d.Jtot < ((int64_t)1 << 31), "sparse PARAFAC2 slabs: sum of J_k = %lld, at most 2^31 - 1", (long long)d.Jtot);
  // (i, j, k) -> (i, g = off[k] + j) on the host, every subscript checked against its own slab.  coo_build then
  // checks (i, g) again and narrows them to int32: two host passes and 24 bytes per nonzero of host scratch in all
  // (2.4 GB at 1e8 nonzeros) -- the price of reusing coo_build as it is; the upload is not on the hot path
  std::vector<int64_t> ig((size_t)2 * nnz);
  const int64_t *si = subs, *sj = subs + nnz, *sk = subs + 2 * nnz;
  for (int64_t n = 0; n < nnz; ++n) {
    const int64_t i = si[n], j = sj[n], k = sk[n];
    if (k < 0 || k >= d.K)
      throw Error(AOADMM_ERR_INVALID, fmt("sparse PARAFAC2 slabs: slab subscript %lld of nonzero %lld is outside [0, %d)",
                                          (long long)k, (long long)n, d.K));
    const int64_t Jk = d.off_h[k + 1] - d.off_h[k];
    if (j < 0 || j >= Jk)
      throw Error(AOADMM_ERR_INVALID, fmt("sparse PARAFAC2 slabs: column subscript %lld of nonzero %lld is outside [0, %lld) of slab %lld",
                                          (long long)j, (long long)n, (long long)Jk, (long long)k));
    if (i < 0 || i >= d.I)
      throw Error(AOADMM_ERR_INVALID, fmt("sparse PARAFAC2 slabs: row subscript %lld of nonzero %lld is outside [0, %d)",
                                          (long long)i, (long long)n, d.I));
    ig[(size_t)n] = i;
    ig[(size_t)nnz + n] = d.off_h[k] + j;
  }
  Par2Sparse nb;
  const int64_t dims[2] = {d.I, d.Jtot};
  coo_build(nb.coo, 2, dims, nnz, ig.data(), vals, s);
  std::vector<int> kofg((size_t)d.Jtot);
  for (int k = 0; k < d.K; ++k)
    for (int64_t g = d.off_h[k]; g < d.off_h[k + 1]; ++g) kofg[(size_t)g] = k;
  nb.kofg.alloc((size_t)d.Jtot * sizeof(int));
  AO_HIP(hipMemcpyAsync(nb.kofg.p, kofg.data(), (size_t)d.Jtot * sizeof(int), hipMemcpyHostToDevice, s));
  nb.xn.alloc((size_t)d.K * sizeof(double));
  if (nb.coo.nnz == 0) {
    AO_HIP(hipMemsetAsync(nb.xn.p, 0, (size_t)d.K * sizeof(double), s));
  } else {
    par2s_slab_normsq_k<<<d.K, 256, 0, s>>>(nb.coo.mode[1].row.as<int>(), nb.coo.mode[1].val.d(), nb.coo.nnz, d, nb.xn.d());
    AO_KERNEL_CHECK();
  }
  AO_HIP(hipStreamSynchronize(s));                   // kofg is a local
  sp = std::move(nb);
}

__global__ void par2s_scale_b_k(const double* B, const double* Cfac, P2Dims d, const int* kofg, double* BC) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d.Jtot * d.R) return;
  const int64_t g = e / d.R;
  const int r = (int)(e % d.R);
  const int k = kofg[g];
  const int64_t o = d.off[k];
  const int64_t Jk = d.off[k + 1] - o;
  BC[e] = B[o * d.R + (g - o) + Jk * r] * Cfac[k + d.K * r];
}
void par2s_scale_b(const double* B, const double* Cfac, const P2Dims& d, const int* kofg, double* BC, hipStream_t s) {
  par2s_scale_b_k<<<blocks_for(d.Jtot * d.R), 256, 0, s>>>(B, Cfac, d, kofg, BC);
  AO_KERNEL_CHECK();
}

__global__ void par2s_ak_k(const double* Y, const double* Cfac, double w, P2Dims d, const int* kofg, double* Ak) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // e = g + Jtot * r: reads of Y coalesced
  if (e >= d.Jtot * d.R) return;
  const int64_t g = e % d.Jtot;
  const int r = (int)(e / d.Jtot);
  const int k = kofg[g];
  const int64_t o = d.off[k];
  const int64_t Jk = d.off[k + 1] - o;
  Ak[o * d.R + (g - o) + Jk * r] = w * Y[e] * Cfac[k + d.K * r];        // w * X_k' * A * diag(C(k,:))   (:193)
}
void par2s_ak(const double* Y, const double* Cfac, double w, const P2Dims& d, const int* kofg, double* Ak, hipStream_t s) {
  par2s_ak_k<<<blocks_for(d.Jtot * d.R), 256, 0, s>>>(Y, Cfac, w, d, kofg, Ak);
  AO_KERNEL_CHECK();
}

// One wavefront per slab, lane r = component r (R <= 64).  Sums over j in four independent partial sums added in a
// fixed order, sums over the components by the fixed-order wave_sum: bitwise reproducible.
__global__ __launch_bounds__(64) void par2s_slab_sums_k(const double* B, const double* Y, P2Dims d, double* sv,
                                                        const double* xn, const double* Cfac, const double* GA,
                                                        const double* GB, double* res) {
  const int k = blockIdx.x, R = d.R, r = threadIdx.x;
  const int64_t o = d.off[k];
  const int Jk = (int)(d.off[k + 1] - o);
  double sr = 0.0;
  if (r < R) {
    const double* b = B + o * R + (int64_t)Jk * r;
    const double* y = Y + o + d.Jtot * r;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = 0;
    for (; j + 3 < Jk; j += 4) {
      a0 += b[j] * y[j]; a1 += b[j + 1] * y[j + 1]; a2 += b[j + 2] * y[j + 2]; a3 += b[j + 3] * y[j + 3];
    }
    for (; j < Jk; ++j) a0 += b[j] * y[j];
    sr = (a0 + a1) + (a2 + a3);
    sv[k + d.K * r] = sr;
  }
  if (res == nullptr) return;
  double cross = 0.0, model = 0.0;
  if (r < R) {
    const double cr = Cfac[k + d.K * r];
    cross = cr * sr;
    const double* gb = GB + (int64_t)k * R * R;
    double t = 0.0;
    for (int q = 0; q < R; ++q) t += GA[q + R * r] * Cfac[k + d.K * q] * gb[q + R * r];
    model = cr * t;
  }
  cross = wave_sum(cross);
  model = wave_sum(model);
  if (r == 0) res[k] = xn[k] - 2.0 * cross + model;
}
void par2s_slab_sums(const double* B, const double* Y, const P2Dims& d, double* sv, const double* xn,
                     const double* Cfac, const double* GA, const double* GB, double* res, hipStream_t s) {
  // one lane per component; aoadmm_model_set_mode already refuses ranks above kMaxRank = 64
  AO_REQUIRE(d.R >= 1 && d.R <= 64, "sparse PARAFAC2 slabs: rank %d outside 1..64", d.R);
  par2s_slab_sums_k<<<d.K, 64, 0, s>>>(B, Y, d, sv, xn, Cfac, GA, GB, res);
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
