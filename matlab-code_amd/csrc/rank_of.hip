// The place of a known target row among a query's candidates: the targets' scores, the counting pass, the exclusion
// pass and the finisher.  See rank_of.h and DESIGN.md section 9.7.
//
// Every score, the target's included, comes from topk_dev.h: the operand map, the clamped gather and the chain that
// topk_scores_k runs, and for rank_count_k the same stream over the slab, so equal scores compare equal and a rank is
// the position top-k gives the row.  This unit is what is done with a score.  Every workgroup is one wave; no kernel
// here uses LDS, a ballot or an atomic.
#include <algorithm>

#include "rank_of.h"
#include "topk_dev.h"

namespace aoadmm {

constexpr int kRankWave = kTopkWave;

struct RankKArgs {
  CooFactor F;            // the free mode's factor
  int R;
  int64_t I, nq, nq_pad, slab_rows, slabs;
  const double* W;        // [nq x R] row-major
  const int* target;      // [nq]
  const int64_t* excl_off;
  const int* excl_idx;
  const int64_t* chunk_off;
  const int* chunk_q;
  double* tscore;         // [nq]: the targets' scores
  int2* cnt;              // [slabs][nq_pad]: (rows that precede the target, rows whose score is not NaN)
  int2* ex;               // [chunks]: the same two counts over a chunk of listed rows
  int64_t* rank;
  double* score;
  int64_t* ncand;
};

// row c of the A operand is F_mode(t_c, .), column c of the B operand is w_c: D[c][c] is score_c(t_c)
template <int KS>
__global__ __launch_bounds__(kRankWave) void rank_target_k(RankKArgs a) {
  const int lane = (int)threadIdx.x, c = lane & 15, q4 = lane >> 4;
  const int64_t q = (int64_t)blockIdx.x * kTopkTile + c;
  const bool live = q < a.nq;
  double x[KS], w[1][KS];
  topk_load_row(x, a.F, live ? a.target[q] : 0, a.R, q4);
  topk_load_w(w[0], a.W, q, live, a.R, q4);
  topk_f64x4 acc[1];
  topk_chain(acc, x, w, topk_last_ok<KS>(a.R, q4));
  // this lane holds D[q4 + 4 e][c]: the diagonal is e = c >> 2 in the lanes with q4 == (c & 3)
  double d = acc[0][0];
#pragma unroll
  for (int e = 1; e < 4; ++e) d = (c >> 2) == e ? acc[0][e] : d;
  if (live && q4 == (c & 3)) a.tscore[q] = d;
}

// KS = ceil(R / 4) MFMA steps, compiled in; QT: query tiles per workgroup
template <int KS, int QT>
__global__ __launch_bounds__(kRankWave) void rank_count_k(RankKArgs a) {
  const int lane = (int)threadIdx.x, c = lane & 15, q4 = lane >> 4;
  const int64_t slab = blockIdx.y;
  const TopkSlab sl = topk_slab(slab, a.slab_rows, a.I);

  double w[QT][KS];
  double sv[QT];                                                  // the target's score and row: the four lanes of a
  int tr[QT];                                                     // column keep identical copies
  int before[QT], notnan[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int64_t q = ((int64_t)blockIdx.x * QT + qt) * kTopkTile + c;
    const bool live = q < a.nq;
    topk_load_w(w[qt], a.W, q, live, a.R, q4);
    sv[qt] = live ? a.tscore[q] : 0.0;
    tr[qt] = live ? a.target[q] : 0;
    before[qt] = notnan[qt] = 0;
  }

  auto step = [&](const topk_f64x4 (&acc)[QT], int r0) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = r0 + q4 + 4 * e;
        const double v = acc[qt][e];
        const bool in = row < sl.re;                               // a row the clamp brought in counts nowhere
        before[qt] += in && (v > sv[qt] || (v == sv[qt] && row < tr[qt])) ? 1 : 0;   // the target itself: neither
        notnan[qt] += in && v == v ? 1 : 0;
      }
  };
  topk_stream(a.F, a.R, sl, w, step);

  // the slab's pair per query: the four lanes of a column hold the four row classes q4 + 4 e
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    int b = before[qt], n = notnan[qt];
    b += __shfl_xor(b, 16); n += __shfl_xor(n, 16);
    b += __shfl_xor(b, 32); n += __shfl_xor(n, 32);
    const int64_t q = ((int64_t)blockIdx.x * QT + qt) * kTopkTile + c;
    if (q4 == 0 && q < a.nq) a.cnt[slab * a.nq_pad + q] = make_int2(b, n);   // a column beyond nq is dropped here
  }
}

// One wave per chunk of one query's listed rows: 16 gathered rows per MFMA step on the row axis, w_q on every column,
// so D[row][0] is the row's score; the lanes of column 0 count.
template <int KS>
__global__ __launch_bounds__(kRankWave) void rank_excl_k(RankKArgs a) {
  const int lane = (int)threadIdx.x, c = lane & 15, q4 = lane >> 4;
  const int64_t ch = blockIdx.x;
  const int64_t q = a.chunk_q[ch];
  const int64_t lb = a.excl_off[q] + (ch - a.chunk_off[q]) * kRankExclChunk;
  const int64_t le = lb + kRankExclChunk < a.excl_off[q + 1] ? lb + kRankExclChunk : a.excl_off[q + 1];   // lb < le
  const double sv = a.tscore[q];
  const int tr = a.target[q];
  double w[1][KS];
  topk_load_w(w[0], a.W, q, true, a.R, q4);
  int before = 0, notnan = 0;
  for (int64_t l0 = lb; l0 < le; l0 += kTopkRows) {
    const int row = a.excl_idx[l0 + c < le ? l0 + c : le - 1];    // clamped: dropped where it is used
    double x[KS];
    topk_load_row(x, a.F, row, a.R, q4);
    topk_f64x4 acc[1];
    topk_chain(acc, x, w, topk_last_ok<KS>(a.R, q4));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = q4 + 4 * e;                                    // D's row: the listed row lane j gathered
      const int rj = __shfl(row, j);
      const double v = acc[0][e];
      const bool in = c == 0 && l0 + j < le && rj != tr;           // the target is a candidate, listed or not
      before += in && (v > sv || (v == sv && rj < tr)) ? 1 : 0;
      notnan += in && v == v ? 1 : 0;
    }
  }
  before += __shfl_xor(before, 16); notnan += __shfl_xor(notnan, 16);
  before += __shfl_xor(before, 32); notnan += __shfl_xor(notnan, 32);
  if (lane == 0) a.ex[ch] = make_int2(before, notnan);
}

// One wave per query: the slabs' pairs minus the chunks' pairs (integer sums: any order)
__global__ __launch_bounds__(kRankWave) void rank_finish_k(RankKArgs a) {
  const int lane = (int)threadIdx.x;
  const int64_t q = blockIdx.x;
  long long before = 0, notnan = 0;
  for (int64_t s = lane; s < a.slabs; s += kRankWave) {
    const int2 p = a.cnt[s * a.nq_pad + q];
    before += p.x; notnan += p.y;
  }
  if (a.chunk_off != nullptr)
    for (int64_t ch = a.chunk_off[q] + lane; ch < a.chunk_off[q + 1]; ch += kRankWave) {
      const int2 p = a.ex[ch];
      before -= p.x; notnan -= p.y;
    }
#pragma unroll
  for (int d = 1; d < kRankWave; d <<= 1) {
    before += __shfl_xor(before, d);
    notnan += __shfl_xor(notnan, d);
  }
  if (lane == 0) {
    const double sv = a.tscore[q];
    a.score[q] = sv;
    a.rank[q] = sv == sv ? (int64_t)before : -1;
    a.ncand[q] = (int64_t)notnan;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// the workspace: where every segment starts, and its size
struct RankWs { size_t W, tscore, cnt, ex, bytes; };
static RankWs rank_ws(int R, int64_t nq, int64_t nq_pad, int64_t slabs, int64_t chunks) {
  RankWs o;
  o.W = 0;
  o.tscore = o.W + align256((size_t)nq * R * sizeof(double));
  o.cnt = o.tscore + align256((size_t)nq * sizeof(double));
  o.ex = o.cnt + align256((size_t)nq_pad * slabs * sizeof(int2));
  o.bytes = o.ex + align256((size_t)chunks * sizeof(int2));
  return o;
}

RankPlan rank_plan(int64_t I, int R, int64_t nq, int64_t chunks) {
  RankPlan pl;
  pl.tp = topk_plan(I, R, nq, 1);      // two tiles per workgroup beyond 16 queries, slabs until the device is full
  pl.nq_pad = pl.tp.qtiles * pl.tp.qt * kTopkTile;
  pl.chunks = chunks;
  pl.workspace_bytes = rank_ws(R, nq, pl.nq_pad, pl.tp.slabs, chunks).bytes;
  return pl;
}

void rank_enqueue(const RankArgs& a, const RankPlan& pl, hipStream_t s) {
  const int R = a.hf.R;
  AO_REQUIRE(R >= 1 && R <= kMaxRank && a.hf.nd >= 2 && a.hf.nd <= kCooMaxModes && a.hf.off == nullptr, "internal: rank pass of rank %d, order %d", R, a.hf.nd);
  AO_REQUIRE(a.mode >= 0 && a.mode < a.hf.nd && a.nq > 0 && a.nq < ((int64_t)1 << 31) && a.I > 0 && a.I < ((int64_t)1 << 31) && a.target != nullptr,
             "internal: rank pass of mode %d", a.mode);
  AO_REQUIRE(pl.tp.slabs >= 1 && pl.tp.slabs <= 65535 && pl.tp.slab_rows % kTopkRows == 0 && pl.tp.slabs * pl.tp.slab_rows >= a.I &&
                 (pl.tp.qt == 1 || pl.tp.qt == 2) && pl.nq_pad >= a.nq && pl.chunks >= 0 && pl.chunks < ((int64_t)1 << 31) &&
                 (pl.chunks == 0 || (a.excl_off != nullptr && a.excl_idx != nullptr && a.chunk_off != nullptr && a.chunk_q != nullptr)),
             "internal: rank plan");
  char* ws = static_cast<char*>(a.workspace);
  const RankWs o = rank_ws(R, a.nq, pl.nq_pad, pl.tp.slabs, pl.chunks);
  double* W = reinterpret_cast<double*>(ws + o.W);

  if (a.W == nullptr) topk_weights_enqueue(a.hf, a.mode, a.nq, a.idx, W, s);

  RankKArgs ka;
  ka.F = a.hf.f[a.mode];
  ka.R = R;
  ka.I = a.I; ka.nq = a.nq; ka.nq_pad = pl.nq_pad; ka.slab_rows = pl.tp.slab_rows; ka.slabs = pl.tp.slabs;
  ka.W = a.W != nullptr ? a.W : W; ka.target = a.target;
  ka.excl_off = a.excl_off; ka.excl_idx = a.excl_idx;
  ka.chunk_off = pl.chunks > 0 ? a.chunk_off : nullptr; ka.chunk_q = a.chunk_q;
  ka.tscore = reinterpret_cast<double*>(ws + o.tscore);
  ka.cnt = reinterpret_cast<int2*>(ws + o.cnt);
  ka.ex = reinterpret_cast<int2*>(ws + o.ex);
  ka.rank = a.rank; ka.score = a.score; ka.ncand = a.ncand;
  for_topk_steps(R, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    rank_target_k<KS><<<(unsigned)cdiv(ka.nq, (int64_t)kTopkTile), kRankWave, 0, s>>>(ka);
    AO_KERNEL_CHECK();
    const dim3 grid((unsigned)pl.tp.qtiles, (unsigned)pl.tp.slabs);
    if (pl.tp.qt == 2) rank_count_k<KS, 2><<<grid, kRankWave, 0, s>>>(ka);
    else rank_count_k<KS, 1><<<grid, kRankWave, 0, s>>>(ka);
    AO_KERNEL_CHECK();
    if (pl.chunks > 0) {
      rank_excl_k<KS><<<(unsigned)pl.chunks, kRankWave, 0, s>>>(ka);
      AO_KERNEL_CHECK();
    }
  });
  rank_finish_k<<<(unsigned)a.nq, kRankWave, 0, s>>>(ka);
  AO_KERNEL_CHECK();
}

double rank_bytes(int nd, int R, int64_t I, int64_t nq, int64_t listed, const RankPlan& plan) {
  return (double)I * R * 8.0 * (double)plan.tp.qtiles + (double)nq * (nd - 1) * (4.0 + 8.0 * R) + (double)(nq + listed) * (4.0 + 8.0 * R) +
         (double)nq * 24.0;
}

double rank_flops(int R, int64_t I, int64_t nq, int64_t listed) {
  return 2.0 * (double)I * (double)nq * R + 2.0 * R * (double)(listed + nq);
}

}  // namespace aoadmm
