// Fold-in under entry weights and a weight for the unlisted cells (foldin.h): the weighted
// instantiations of foldin_k, in a translation unit of their own so that the two halves of the longest compile of the
// library run side by side, and H = had_{m != mode} F_m'F_m, which every query of a call with alpha > 0 receives.
//
// H is computed inside the call from the factors the pass gathers from, whatever their layout: a block of
// foldin_gram_part_k sums the rows of its span in index order into one R x R partial, atb_fin adds the partials in its
// fixed order, foldin_had_k multiplies the Gram matrices in mode order.  The cut into spans depends on the number of rows
// alone and a sum never depends on the strides, so the row-major copies a solve leaves and the column-major factors of an
// upload give the same bits.  No float atomics.
#include <algorithm>

#include "foldin_dev.h"
#include "small.h"

namespace aoadmm {

void foldin_launch_weighted(const FoldKArgsW& ka, int64_t items, int64_t splits, hipStream_t s) {
  launch_foldin_class<true>(ka, items, splits, s);
}

constexpr int kFoldGramRows = 32;            // rows staged per step
constexpr int kFoldGramBlocks = 512;         // at most this many partials per factor
constexpr int kFoldGramThreads = 256;
constexpr int kFoldGramPer = kMaxRank * kMaxRank / kFoldGramThreads;   // outputs per thread

static int foldin_gram_blocks(int64_t I) { return (int)std::min<int64_t>(kFoldGramBlocks, std::max<int64_t>(1, cdiv(I, 8 * kFoldGramRows))); }

size_t foldin_gram_ws_doubles(const HeldoutFactors& hf, const int64_t* rows, int mode) {
  int64_t nb = 1;
  for (int m = 0; m < hf.nd; ++m)
    if (m != mode) nb = std::max<int64_t>(nb, foldin_gram_blocks(rows[m]));
  const size_t RR = (size_t)hf.R * hf.R;
  return RR * (size_t)nb + RR * (size_t)(hf.nd - 1);
}

// part[b] = F(span b, :)' F(span b, :) with the rows added in index order from +0; element (i, r) of F at
// p[i sI + r sR].  Entry (k, n) and entry (n, k) add the same products in the same order.
__global__ __launch_bounds__(kFoldGramThreads) void foldin_gram_part_k(CooFactor F, int64_t I, int R, double* part) {
  __shared__ double tile[kFoldGramRows * (kMaxRank + 1)];   // row-major, padded by 1
  const int Rp = R + 1, RR = R * R;
  const int64_t rpb = (I + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = blockIdx.x * rpb;
  const int64_t i1 = i0 + rpb < I ? i0 + rpb : I;
  double acc[kFoldGramPer];
#pragma unroll
  for (int q = 0; q < kFoldGramPer; ++q) acc[q] = 0.0;
  for (int64_t r0 = i0; r0 < i1; r0 += kFoldGramRows) {
    const int nr = (int)(i1 - r0 < kFoldGramRows ? i1 - r0 : kFoldGramRows);
    __syncthreads();
    for (int e = threadIdx.x; e < nr * R; e += kFoldGramThreads) {
      // the contiguous index of the layout runs fastest
      const int i = F.sR == 1 ? e / R : e % nr, k = F.sR == 1 ? e % R : e / nr;
      tile[i * Rp + k] = F.p[(r0 + i) * F.sI + (int64_t)k * F.sR];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kFoldGramPer; ++q) {
      const int e = threadIdx.x + q * kFoldGramThreads;
      if (e < RR) {
        const int k = e % R, n = e / R;
        double s = acc[q];
        for (int i = 0; i < nr; ++i) s = fma(tile[i * Rp + k], tile[i * Rp + n], s);
        acc[q] = s;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kFoldGramPer; ++q) {
    const int e = threadIdx.x + q * kFoldGramThreads;
    if (e < RR) part[(int64_t)blockIdx.x * RR + e] = acc[q];
  }
}

// H = G_0 .* G_1 .* ... in mode order; entry (i, j) with i <= j defines both triangles
__global__ void foldin_had_k(const double* G, int nm, int R, double* H) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= R * R) return;
  const int i = e % R, j = e / R;
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  double h = G[lo + R * hi];
  for (int m = 1; m < nm; ++m) h *= G[(int64_t)m * R * R + lo + R * hi];
  H[e] = h;
}

void foldin_gram_enqueue(const HeldoutFactors& hf, const int64_t* rows, int mode, double* ws, double* H, hipStream_t s) {
  const int R = hf.R, RR = R * R, nm = hf.nd - 1;
  AO_REQUIRE(R >= 1 && R <= kMaxRank && nm >= 1 && hf.off == nullptr && ws != nullptr && H != nullptr, "internal: fold-in Gram of rank %d", R);
  double* G = ws;                                // nm Gram matrices, then the partials of one factor at a time
  double* part = ws + (size_t)RR * nm;
  int j = 0;
  for (int m = 0; m < hf.nd; ++m) {
    if (m == mode) continue;
    const int64_t I = rows[m];
    AO_REQUIRE(I >= 1, "internal: fold-in Gram of a factor of %lld rows", (long long)I);
    const int nb = foldin_gram_blocks(I);
    double* Gm = G + (size_t)RR * j++;
    foldin_gram_part_k<<<nb, kFoldGramThreads, 0, s>>>(hf.f[m], I, R, nb == 1 ? Gm : part);
    AO_KERNEL_CHECK();
    if (nb > 1) atb_fin(Gm, part, nb, RR, nullptr, s);
  }
  foldin_had_k<<<(unsigned)cdiv(RR, 256), 256, 0, s>>>(G, nm, R, H);
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
