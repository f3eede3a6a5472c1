// The place of a known target row among a query's candidates: the targets' scores, the counting pass, the exclusion
// pass and the finisher.  See rank_of.h and DESIGN.md section 9.7.
//
// Every score, the target's included, is one element of the chain of ceil(R / 4) v_mfma_f64_16x16x4_f64 that
// topk_scores_k runs (topk.hip: the operand map, zeros beyond R, the chain from +0), so equal scores compare equal and a
// rank is the position top-k gives the row.  The load ring and the chain of rank_count_k are a copy of topk_scores_k's:
// that kernel is left as it is (DESIGN.md section 9.7 says why).  Every workgroup is one wave; no kernel here uses LDS,
// a ballot or an atomic.
#include <algorithm>

#include "rank_of.h"

namespace aoadmm {

typedef double rank_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kRankWave = 64;

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
  const int R = a.R;
  const int64_t q = (int64_t)blockIdx.x * kTopkTile + c;
  const bool live = q < a.nq;
  const int t = live ? a.target[q] : 0;
  const double* fp = a.F.p + (int64_t)t * a.F.sI;
  double x[KS], w[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int kk = 4 * s + q4;
    const double f = fp[(int64_t)(kk < R ? kk : R - 1) * a.F.sR];
    x[s] = kk < R ? f : 0.0;
    w[s] = live && kk < R ? a.W[q * R + kk] : 0.0;
  }
  rank_f64x4 acc = rank_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[s], w[s], acc, 0, 0, 0);
  // this lane holds D[q4 + 4 e][c]: the diagonal is e = c >> 2 in the lanes with q4 == (c & 3)
  double d = acc[0];
#pragma unroll
  for (int e = 1; e < 4; ++e) d = (c >> 2) == e ? acc[e] : d;
  if (live && q4 == (c & 3)) a.tscore[q] = d;
}

// KS = ceil(R / 4) MFMA steps, compiled in; QT: query tiles per workgroup.  The stream over the slab is topk_scores_k's.
template <int KS, int QT>
__global__ __launch_bounds__(kRankWave) void rank_count_k(RankKArgs a) {
  const int lane = (int)threadIdx.x, c = lane & 15, q4 = lane >> 4;
  const int R = a.R;
  const int64_t slab = blockIdx.y;
  const int rb = (int)(slab * a.slab_rows);                       // I < 2^31: rows are ints from here on
  const int re = (int)(slab * a.slab_rows + a.slab_rows < a.I ? slab * a.slab_rows + a.slab_rows : a.I);
  const bool last_ok = 4 * (KS - 1) + q4 < R;                     // only the last step can hold columns beyond R

  double w[QT][KS];
  double sv[QT];                                                  // the target's score and row: the four lanes of a
  int tr[QT];                                                     // column keep identical copies
  int before[QT], notnan[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int64_t q = ((int64_t)blockIdx.x * QT + qt) * kTopkTile + c;
    const bool live = q < a.nq;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int kk = 4 * s + q4;
      w[qt][s] = live && kk < R ? a.W[q * R + kk] : 0.0;
    }
    sv[qt] = live ? a.tscore[q] : 0.0;
    tr[qt] = live ? a.target[q] : 0;
    before[qt] = notnan[qt] = 0;
  }

  // Unconditional loads on clamped addresses (a row of this slab, a column below R): no branch around a load, so the
  // loads of D steps stay in flight.  What a clamp brought in is dropped where it is used.
  auto load_rows = [&](double (&av)[KS], int r0) {
    const int ar = r0 + c < re ? r0 + c : re - 1;
    const double* fp = a.F.p + (int64_t)ar * a.F.sI;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int kk = 4 * s + q4;
      av[s] = fp[(int64_t)(kk < R ? kk : R - 1) * a.F.sR];
    }
  };

  auto step = [&](const double (&av)[KS], int r0) {
    rank_f64x4 acc[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) acc[qt] = rank_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const double x = s + 1 < KS || last_ok ? av[s] : 0.0;
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) acc[qt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, w[qt][s], acc[qt], 0, 0, 0);
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = r0 + q4 + 4 * e;
        const double v = acc[qt][e];
        const bool in = row < re;                                  // a row the clamp brought in counts nowhere
        before[qt] += in && (v > sv[qt] || (v == sv[qt] && row < tr[qt])) ? 1 : 0;   // the target itself: neither
        notnan[qt] += in && v == v ? 1 : 0;
      }
  };

  // A ring of D steps' rows with fixed roles (no register moves: a move would wait for the load it copies)
  constexpr int D = KS <= 8 ? 4 : 2;
  double av[D][KS];
#pragma unroll
  for (int d = 0; d < D; ++d) load_rows(av[d], rb + d * kTopkRows);
  for (int row0 = rb; row0 < re; row0 += D * kTopkRows) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int r0 = row0 + d * kTopkRows;
      if (r0 < re) {                                               // uniform
        double cur[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) cur[s] = av[d][s];
        load_rows(av[d], r0 + D * kTopkRows);
        step(cur, r0);
      }
    }
  }

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
  const int R = a.R;
  const int64_t ch = blockIdx.x;
  const int64_t q = a.chunk_q[ch];
  const int64_t lb = a.excl_off[q] + (ch - a.chunk_off[q]) * kRankExclChunk;
  const int64_t le = lb + kRankExclChunk < a.excl_off[q + 1] ? lb + kRankExclChunk : a.excl_off[q + 1];   // lb < le
  const double sv = a.tscore[q];
  const int tr = a.target[q];
  double w[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int kk = 4 * s + q4;
    w[s] = kk < R ? a.W[q * R + kk] : 0.0;
  }
  int before = 0, notnan = 0;
  for (int64_t l0 = lb; l0 < le; l0 += kTopkRows) {
    const int row = a.excl_idx[l0 + c < le ? l0 + c : le - 1];    // clamped: dropped where it is used
    const double* fp = a.F.p + (int64_t)row * a.F.sI;
    rank_f64x4 acc = rank_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int kk = 4 * s + q4;
      const double f = fp[(int64_t)(kk < R ? kk : R - 1) * a.F.sR];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(kk < R ? f : 0.0, w[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = q4 + 4 * e;                                    // D's row: the listed row lane j gathered
      const int rj = __shfl(row, j);
      const double v = acc[e];
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
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

RankPlan rank_plan(int64_t I, int R, int64_t nq, int64_t chunks) {
  RankPlan pl;
  pl.tp = topk_plan(I, R, nq, 1);      // two tiles per workgroup beyond 16 queries, slabs until the device is full
  pl.nq_pad = pl.tp.qtiles * pl.tp.qt * kTopkTile;
  pl.chunks = chunks;
  pl.workspace_bytes = align256((size_t)nq * R * sizeof(double)) + align256((size_t)nq * sizeof(double)) +
                       align256((size_t)pl.nq_pad * pl.tp.slabs * sizeof(int2)) + align256((size_t)chunks * sizeof(int2));
  return pl;
}

template <int KS>
static void launch_rank(const RankKArgs& ka, const RankPlan& pl, hipStream_t s) {
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
  double* W = reinterpret_cast<double*>(ws);
  ws += align256((size_t)a.nq * R * sizeof(double));
  double* tscore = reinterpret_cast<double*>(ws);
  ws += align256((size_t)a.nq * sizeof(double));
  int2* cnt = reinterpret_cast<int2*>(ws);
  ws += align256((size_t)pl.nq_pad * pl.tp.slabs * sizeof(int2));
  int2* ex = reinterpret_cast<int2*>(ws);

  if (a.W == nullptr) topk_weights_enqueue(a.hf, a.mode, a.nq, a.idx, W, s);

  RankKArgs ka;
  ka.F = a.hf.f[a.mode];
  ka.R = R;
  ka.I = a.I; ka.nq = a.nq; ka.nq_pad = pl.nq_pad; ka.slab_rows = pl.tp.slab_rows; ka.slabs = pl.tp.slabs;
  ka.W = a.W != nullptr ? a.W : W; ka.target = a.target;
  ka.excl_off = a.excl_off; ka.excl_idx = a.excl_idx;
  ka.chunk_off = pl.chunks > 0 ? a.chunk_off : nullptr; ka.chunk_q = a.chunk_q;
  ka.tscore = tscore; ka.cnt = cnt; ka.ex = ex;
  ka.rank = a.rank; ka.score = a.score; ka.ncand = a.ncand;
  switch ((R + 3) / 4) {
    case 1: launch_rank<1>(ka, pl, s); break;
    case 2: launch_rank<2>(ka, pl, s); break;
    case 3: launch_rank<3>(ka, pl, s); break;
    case 4: launch_rank<4>(ka, pl, s); break;
    case 5: launch_rank<5>(ka, pl, s); break;
    case 6: launch_rank<6>(ka, pl, s); break;
    case 7: launch_rank<7>(ka, pl, s); break;
    case 8: launch_rank<8>(ka, pl, s); break;
    case 9: launch_rank<9>(ka, pl, s); break;
    case 10: launch_rank<10>(ka, pl, s); break;
    case 11: launch_rank<11>(ka, pl, s); break;
    case 12: launch_rank<12>(ka, pl, s); break;
    case 13: launch_rank<13>(ka, pl, s); break;
    case 14: launch_rank<14>(ka, pl, s); break;
    case 15: launch_rank<15>(ka, pl, s); break;
    default: launch_rank<16>(ka, pl, s); break;
  }
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
