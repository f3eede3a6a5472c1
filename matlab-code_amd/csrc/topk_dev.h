// The free-mode score stream, device side: every score of top-k (topk.hip), of rank-of (rank_of.hip) and of the ranking
// list inside a solve comes from the pieces below.  See DESIGN.md sections 9.5 and 9.7.
//
// Operand map: v_mfma_f64_16x16x4_f64 with 16 rows of F_mode on the row axis and 16 queries on the column axis, the map
// admm_rows_mfma_k uses.  Lane (c = l & 15, q4 = l >> 4) supplies A[row c][k = 4 s + q4] = F_mode(row_c, 4 s + q4) and
// B[k = 4 s + q4][col c] = w_c(4 s + q4) and receives D[row q4 + 4 e][col c], e = 0 .. 3 (the f64 C/D map).
//
// Chain: a score is the chain of KS = ceil(R / 4) MFMAs over s = 0, 1, ... from +0, columns beyond R supplied as zeros on
// both sides.  Its summation order is a function of R alone, whatever the slab, the tile, the query's place in the tile,
// the strides gathered through or the kernel that asks: equal scores compare equal everywhere, which rank-of's bitwise
// agreement with top-k rests on.  KS is compiled in: a chain whose length is a run-time value reads its accumulator back
// after every MFMA.
//
// Loads: unconditional, on clamped addresses (a row the caller clamped into range, a column below R): no branch around a
// load, so the loads of several steps stay in flight.  What a clamp brought in is dropped where it is used: a column
// beyond R as a zero operand of the last step, a row beyond the range by the caller.
#pragma once
#include <type_traits>

#include "topk.h"

namespace aoadmm {

typedef double topk_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kTopkWave = 64;

// w[s] = W[q R + 4 s + q4], or 0 for a query beyond nq (live false) or a column beyond R
template <int KS>
__device__ __forceinline__ void topk_load_w(double (&w)[KS], const double* W, int64_t q, bool live, int R, int q4) {
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int kk = 4 * s + q4;
    w[s] = live && kk < R ? W[q * R + kk] : 0.0;
  }
}

// this lane's A operands of row `row` of F
template <int KS>
__device__ __forceinline__ void topk_load_row(double (&av)[KS], const CooFactor& F, int row, int R, int q4) {
  const double* fp = F.p + (int64_t)row * F.sI;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int kk = 4 * s + q4;
    av[s] = fp[(int64_t)(kk < R ? kk : R - 1) * F.sR];
  }
}

// only the last step can hold columns beyond R: whether this lane's column of it is one of the R
template <int KS>
__device__ __forceinline__ bool topk_last_ok(int R, int q4) { return 4 * (KS - 1) + q4 < R; }

// acc[qt] = the scores of the 16 rows in av against the queries of tile qt
template <int KS, int QT>
__device__ __forceinline__ void topk_chain(topk_f64x4 (&acc)[QT], const double (&av)[KS], const double (&w)[QT][KS], bool last_ok) {
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) acc[qt] = topk_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const double x = s + 1 < KS || last_ok ? av[s] : 0.0;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) acc[qt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, w[qt][s], acc[qt], 0, 0, 0);
  }
}

// rows [rb, re) of slab `slab`: I < 2^31, rows are ints from here on
struct TopkSlab { int rb, re; };
__device__ __forceinline__ TopkSlab topk_slab(int64_t slab, int64_t slab_rows, int64_t I) {
  const int64_t b = slab * slab_rows;
  return TopkSlab{(int)b, (int)(b + slab_rows < I ? b + slab_rows : I)};
}

// The stream over a slab, 16 rows per step: sink(acc, r0) receives the step's scores against w (acc[qt][e] is row
// r0 + q4 + 4 e, query 16 qt + c of the workgroup's tiles; rows >= sl.re are the clamp's).  A ring of D steps' rows with
// fixed roles (no register moves: a move would wait for the load it copies); a role's next load is issued before the
// step that consumes its previous contents.
template <int KS, int QT, class Sink>
__device__ __forceinline__ void topk_stream(const CooFactor& F, int R, TopkSlab sl, const double (&w)[QT][KS], Sink& sink) {
  const int lane = (int)threadIdx.x, c = lane & 15, q4 = lane >> 4;
  const bool last_ok = topk_last_ok<KS>(R, q4);
  auto load_rows = [&](double (&av)[KS], int r0) { topk_load_row(av, F, r0 + c < sl.re ? r0 + c : sl.re - 1, R, q4); };
  constexpr int D = KS <= 8 ? 4 : 2;
  double av[D][KS];
#pragma unroll
  for (int d = 0; d < D; ++d) load_rows(av[d], sl.rb + d * kTopkRows);
  for (int row0 = sl.rb; row0 < sl.re; row0 += D * kTopkRows) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int r0 = row0 + d * kTopkRows;
      if (r0 < sl.re) {                                            // uniform
        double cur[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) cur[s] = av[d][s];
        load_rows(av[d], r0 + D * kTopkRows);
        topk_f64x4 acc[QT];
        topk_chain(acc, cur, w, last_ok);
        sink(acc, r0);
      }
    }
  }
}

// host: f(std::integral_constant<int, KS>) for the chain length of rank R, 1 <= R <= kMaxRank
template <int KS = 1, class F>
void for_topk_steps(int R, F&& f) {
  if constexpr (4 * KS < kMaxRank) {
    if (R > 4 * KS) return for_topk_steps<KS + 1>(R, f);
  }
  f(std::integral_constant<int, KS>{});
}

}  // namespace aoadmm
