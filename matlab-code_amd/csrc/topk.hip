// Top-k completions along one mode: the weights, the fused scores-and-selection pass and the merge.  See topk.h and
// DESIGN.md section 9.5.
//
// Scores: the stream of topk_dev.h (the operand map, the chain from +0, the load ring); this unit is the selection.
//
// Selection: a workgroup is ONE wave, so its candidate buffers are wave-private and every barrier is a one-wave barrier
// in uniform control flow.  Per query: `cap` slots of (score, row) in LDS, a count and a threshold in registers (the
// four lanes of a query's column keep identical copies).  A row is appended when it beats the threshold (rows ascend
// inside a slab, so "beats" is a strict >) and is not excluded; the slot comes from a ballot, not an atomic.  When a
// step could overflow the buffer it is compacted: every entry's rank in the total order is counted against all others
// and the entries of rank < k are written to slot `rank`, which leaves the best k sorted and the k-th as the new
// threshold.
#include <algorithm>
#include <cmath>

#include "topk_dev.h"

namespace aoadmm {

constexpr int kTopkMergeCap = 2 * kTopkMax;      // the merge's buffer: the best k so far and one chunk of 64 candidates

struct TopkKArgs {
  CooFactor F;            // the free mode's factor
  int R, k, cap;
  int64_t I, nq, slab_rows, slabs;
  const double* W;        // [nq x R] row-major
  const int64_t* excl_off;
  const int* excl_idx;
  double* cand_val;       // [nq][slabs][k]
  int* cand_idx;
};

struct TopkWArgs {
  HeldoutFactors hf;
  int mode;
  int64_t nq;
  const int* idx;
  double* W;
};

// w_q(r): the other modes' rows multiplied in mode order, starting from 1
__global__ __launch_bounds__(256) void topk_weights_k(TopkWArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int R = a.hf.R;
  if (t >= a.nq * R) return;
  const int64_t q = t / R;
  const int r = (int)(t - q * R);
  double w = 1.0;
  for (int m = 0; m < a.hf.nd; ++m) {
    if (m == a.mode) continue;
    const int64_t s = a.idx[(int64_t)m * a.nq + q];
    w *= a.hf.f[m].p[s * a.hf.f[m].sI + r * a.hf.f[m].sR];
  }
  a.W[t] = w;
}

// the total order of the answer: larger score first, equal scores by smaller row (no NaN ever reaches a buffer)
__device__ __forceinline__ bool topk_before(double va, int ia, double vb, int ib) { return va > vb || (va == vb && ia < ib); }

// The n <= 128 entries of one buffer -> its best min(n, k), sorted, in slots 0 ..; every lane of the wave calls it, the
// appended entries are visible (a barrier precedes the call), and the result is visible on return.
__device__ void topk_compact(double* V, int* X, int n, int k) {
  const int lane = (int)threadIdx.x;
  const bool h0 = lane < n, h1 = lane + kTopkWave < n;
  double v0 = 0.0, v1 = 0.0;
  int i0 = 0, i1 = 0;
  if (h0) { v0 = V[lane]; i0 = X[lane]; }
  if (h1) { v1 = V[lane + kTopkWave]; i1 = X[lane + kTopkWave]; }
  int r0 = 0, r1 = 0;
#pragma unroll 4
  for (int t = 0; t < n; ++t) {
    const double vt = V[t];
    const int it = X[t];
    r0 += topk_before(vt, it, v0, i0) ? 1 : 0;
    r1 += topk_before(vt, it, v1, i1) ? 1 : 0;
  }
  __syncthreads();
  if (h0 && r0 < k) { V[r0] = v0; X[r0] = i0; }
  if (h1 && r1 < k) { V[r1] = v1; X[r1] = i1; }
  __syncthreads();
}

__device__ __forceinline__ bool topk_excluded(const int* ex, int64_t lo, int64_t hi, int row) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ex[mid] < row) lo = mid + 1; else hi = mid;
  }
  return lo < end && ex[lo] == row;
}

// KS = ceil(R / 4) MFMA steps, compiled in; QT: query tiles per workgroup
template <int KS, int QT>
__global__ __launch_bounds__(kTopkWave) void topk_scores_k(TopkKArgs a) {
  extern __shared__ double topk_lds[];
  double* V = topk_lds;                                           // [QT * 16][cap]
  int* X = reinterpret_cast<int*>(topk_lds + (size_t)QT * kTopkTile * a.cap);
  const int lane = (int)threadIdx.x, c = lane & 15, q4 = lane >> 4;
  const int R = a.R, k = a.k, cap = a.cap;
  const int64_t slab = blockIdx.y;
  const TopkSlab sl = topk_slab(slab, a.slab_rows, a.I);
  const int re = sl.re;
  const double ninf = -__builtin_inf();

  // A query beyond nq never takes a candidate: its threshold is +inf from the start.
  double w[QT][KS];
  int64_t eb[QT], ee[QT];
  int cnt[QT];
  double tv[QT];
  bool act[QT];                                                   // the threshold is the k-th best of >= k candidates
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int64_t q = ((int64_t)blockIdx.x * QT + qt) * kTopkTile + c;
    const bool live = q < a.nq;
    topk_load_w(w[qt], a.W, q, live, R, q4);
    eb[qt] = ee[qt] = 0;
    if (live && a.excl_off != nullptr) { eb[qt] = a.excl_off[q]; ee[qt] = a.excl_off[q + 1]; }
    cnt[qt] = 0;
    tv[qt] = live ? ninf : __builtin_inf();
    act[qt] = !live;
  }

  auto step = [&](const topk_f64x4 (&acc)[QT], int r0) {
    // most steps of a long slab bring no candidate at all: one ballot decides (rows beyond the slab and excluded rows
    // are sorted out below)
    bool any = false;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int e = 0; e < 4; ++e) any = any || acc[qt][e] > tv[qt] || (!act[qt] && acc[qt][e] == ninf);
    if (__ballot(any) == 0ull) return;
    bool need = false;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      double* Vq = V + (size_t)(qt * kTopkTile + c) * cap;
      int* Xq = X + (size_t)(qt * kTopkTile + c) * cap;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // r0 as the scalar it is: folded into the lane's part, the ring's D steps each keep their own four row offsets
        // in VGPRs (6 to 8 more, a wave per SIMD less at <1, 1>, <3, 1> and <6, 2>)
        const int row = __builtin_amdgcn_readfirstlane(r0) + q4 + 4 * e;
        const double v = acc[qt][e];
        bool pred = row < re && (v > tv[qt] || (!act[qt] && v == ninf));   // never a NaN
        if (pred && ee[qt] > eb[qt]) pred = !topk_excluded(a.excl_idx, eb[qt], ee[qt], row);
        const unsigned long long mask = __ballot(pred);
        if (mask != 0ull) {
          const unsigned long long mine = mask & (0x0001000100010001ull << c);   // the four lanes of this query
          const int pos = cnt[qt] + __popcll(mine & ((1ull << lane) - 1ull));
          if (pred) { Vq[pos] = v; Xq[pos] = row; }
          cnt[qt] += __popcll(mine);
        }
      }
      need = need || cnt[qt] > cap - kTopkRows;
    }
    if (__ballot(need) != 0ull) {                                  // uniform: some buffer could overflow in the next step
      __syncthreads();
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        unsigned long long m = __ballot(cnt[qt] > cap - kTopkRows) & 0xFFFFull;   // lanes 0 .. 15: one per query
        while (m != 0ull) {
          const int cq = __ffsll((long long)m) - 1;
          m &= m - 1ull;
          const int n = __shfl(cnt[qt], cq);
          double* Vc = V + (size_t)(qt * kTopkTile + cq) * cap;
          topk_compact(Vc, X + (size_t)(qt * kTopkTile + cq) * cap, n, k);
          if (c == cq) { cnt[qt] = k; act[qt] = true; tv[qt] = Vc[k - 1]; }   // n > cap - 16 >= k
        }
      }
    }
  };

  topk_stream(a.F, R, sl, w, step);

  // the slab's answer: every buffer sorted, k entries per query to this workgroup's own area
  __syncthreads();
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    for (int cq = 0; cq < kTopkTile; ++cq) {
      const int64_t q = ((int64_t)blockIdx.x * QT + qt) * kTopkTile + cq;
      if (q >= a.nq) break;                                        // uniform
      const int n = __shfl(cnt[qt], cq);
      double* Vc = V + (size_t)(qt * kTopkTile + cq) * cap;
      int* Xc = X + (size_t)(qt * kTopkTile + cq) * cap;
      topk_compact(Vc, Xc, n, k);
      const int have = n < k ? n : k;
      const int64_t base = (q * a.slabs + slab) * k;
      for (int j = lane; j < k; j += kTopkWave) {
        a.cand_val[base + j] = j < have ? Vc[j] : ninf;
        a.cand_idx[base + j] = j < have ? Xc[j] : -1;
      }
    }
  }
}

// One wave per (query, group of slabs): the group's candidates in slab order, 64 at a time with four chunks' loads in
// flight, through the same threshold-and-compact buffer.  FINAL: the answer (int64 rows); else k candidates per group
// in the layout it reads, for the next level.
constexpr int kTopkMergeUnroll = 4;
template <bool FINAL>
__global__ __launch_bounds__(kTopkWave) void topk_merge_k(const double* cand_val, const int* cand_idx, int64_t slabs, int64_t per_group,
                                                         int k, double* next_val, int* next_idx, int64_t* out_idx, double* out_val) {
  __shared__ double V[kTopkMergeCap];
  __shared__ int X[kTopkMergeCap];
  const int lane = (int)threadIdx.x;
  const int64_t q = blockIdx.x, g = blockIdx.y, groups = gridDim.y;
  const int64_t s0 = g * per_group, s1 = s0 + per_group < slabs ? s0 + per_group : slabs;
  const int64_t total = (s1 - s0) * k;
  const double* cv = cand_val + (q * slabs + s0) * k;
  const int* ci = cand_idx + (q * slabs + s0) * k;
  int cnt = 0, ti = 0;
  double tv = 0.0;
  bool act = false;
  for (int64_t t0 = 0; t0 < total; t0 += kTopkWave * kTopkMergeUnroll) {
    double vu[kTopkMergeUnroll];
    int iu[kTopkMergeUnroll];
#pragma unroll
    for (int u = 0; u < kTopkMergeUnroll; ++u) {
      const int64_t t = t0 + u * kTopkWave + lane;
      vu[u] = 0.0; iu[u] = -1;
      if (t < total) { vu[u] = cv[t]; iu[u] = ci[t]; }
    }
#pragma unroll
    for (int u = 0; u < kTopkMergeUnroll; ++u) {
      const bool pred = iu[u] >= 0 && (!act || topk_before(vu[u], iu[u], tv, ti));
      const unsigned long long mask = __ballot(pred);
      if (mask == 0ull) continue;
      if (pred) {
        const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
        V[pos] = vu[u]; X[pos] = iu[u];
      }
      cnt += __popcll(mask);
      if (cnt > kTopkMergeCap - kTopkWave) {                       // uniform
        __syncthreads();
        topk_compact(V, X, cnt, k);
        cnt = k; act = true; tv = V[k - 1]; ti = X[k - 1];         // cnt > 64 >= k
      }
    }
  }
  __syncthreads();
  topk_compact(V, X, cnt, k);
  const int have = cnt < k ? cnt : k;
  for (int j = lane; j < k; j += kTopkWave) {
    const double v = j < have ? V[j] : -__builtin_inf();
    const int i = j < have ? X[j] : -1;
    if (FINAL) {
      out_val[q * k + j] = v;
      out_idx[q * k + j] = (int64_t)i;
    } else {
      next_val[(q * groups + g) * k + j] = v;
      next_idx[(q * groups + g) * k + j] = i;
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr int64_t kTopkTargetGroups = 2048;      // workgroups that fill the device: 256 CUs, 8 one-wave groups each
constexpr int64_t kTopkMinSlabRows = 256;        // a slab shorter than this spends its time on the final compaction
constexpr int64_t kTopkMergeGroup = 32;          // slabs one merge workgroup reduces; more slabs take another level

// the workspace: where every segment starts, and its size
struct TopkWs { size_t W, cand_val, cand_idx, pong_val, pong_idx, bytes; };
static TopkWs topk_ws(int R, int64_t nq, int k, int64_t slabs) {
  const size_t c0 = (size_t)nq * slabs * k, c1 = (size_t)nq * cdiv(slabs, kTopkMergeGroup) * k;   // the merge's ping and pong
  TopkWs o;
  o.W = 0;
  o.cand_val = o.W + align256((size_t)nq * R * sizeof(double));
  o.cand_idx = o.cand_val + align256(c0 * sizeof(double));
  o.pong_val = o.cand_idx + align256(c0 * sizeof(int));
  o.pong_idx = o.pong_val + align256(c1 * sizeof(double));
  o.bytes = o.pong_idx + align256(c1 * sizeof(int));
  return o;
}

TopkPlan topk_plan(int64_t I, int R, int64_t nq, int k) {
  TopkPlan pl;
  // two tiles halve the passes over F_mode; beyond k = 32 their buffers (48 KB) leave three waves per CU and one tile wins
  pl.qt = nq > kTopkTile && k <= 32 ? 2 : 1;
  pl.qtiles = cdiv(nq, (int64_t)kTopkTile * pl.qt);
  int64_t slabs = std::max<int64_t>(1, cdiv(kTopkTargetGroups, pl.qtiles));
  slabs = std::min<int64_t>(slabs, std::max<int64_t>(1, cdiv(I, kTopkMinSlabRows)));
  slabs = std::min<int64_t>(slabs, 65535);
  pl.slab_rows = cdiv(cdiv(I, slabs), kTopkRows) * kTopkRows;
  pl.slabs = cdiv(I, pl.slab_rows);
  pl.cap = 2 * std::max(k, kTopkRows);
  pl.lds_bytes = (size_t)pl.qt * kTopkTile * pl.cap * (sizeof(double) + sizeof(int));
  pl.workspace_bytes = topk_ws(R, nq, k, pl.slabs).bytes;
  return pl;
}

void topk_weights_enqueue(const HeldoutFactors& hf, int mode, int64_t nq, const int* idx, double* W, hipStream_t s) {
  TopkWArgs wa;
  wa.hf = hf; wa.mode = mode; wa.nq = nq; wa.idx = idx; wa.W = W;
  topk_weights_k<<<(unsigned)cdiv(nq * hf.R, 256), 256, 0, s>>>(wa);
  AO_KERNEL_CHECK();
}

void topk_enqueue(const TopkArgs& a, const TopkPlan& pl, hipStream_t s) {
  const int R = a.hf.R;
  AO_REQUIRE(R >= 1 && R <= kMaxRank && a.hf.nd >= 2 && a.hf.nd <= kCooMaxModes && a.hf.off == nullptr, "internal: top-k pass of rank %d, order %d", R, a.hf.nd);
  AO_REQUIRE(a.mode >= 0 && a.mode < a.hf.nd && a.k >= 1 && a.k <= kTopkMax && a.nq > 0 && a.I > 0 && a.I < ((int64_t)1 << 31), "internal: top-k pass of mode %d, k = %d", a.mode, a.k);
  AO_REQUIRE(pl.cap >= a.k + kTopkRows && pl.cap <= kTopkMergeCap && pl.lds_bytes <= 64 * 1024 && pl.slabs >= 1 && pl.slabs <= 65535 &&
                 pl.slab_rows % kTopkRows == 0 && pl.slabs * pl.slab_rows >= a.I && pl.qtiles * pl.qt * kTopkTile >= a.nq,
             "internal: top-k plan");
  char* ws = static_cast<char*>(a.workspace);
  const TopkWs o = topk_ws(R, a.nq, a.k, pl.slabs);
  double* W = reinterpret_cast<double*>(ws + o.W);
  double* cand_val = reinterpret_cast<double*>(ws + o.cand_val);
  int* cand_idx = reinterpret_cast<int*>(ws + o.cand_idx);
  double* pong_val = reinterpret_cast<double*>(ws + o.pong_val);
  int* pong_idx = reinterpret_cast<int*>(ws + o.pong_idx);

  if (a.W == nullptr) topk_weights_enqueue(a.hf, a.mode, a.nq, a.idx, W, s);

  TopkKArgs ka;
  ka.F = a.hf.f[a.mode];
  ka.R = R; ka.k = a.k; ka.cap = pl.cap;
  ka.I = a.I; ka.nq = a.nq; ka.slab_rows = pl.slab_rows; ka.slabs = pl.slabs;
  ka.W = a.W != nullptr ? a.W : W; ka.excl_off = a.excl_off; ka.excl_idx = a.excl_idx;
  ka.cand_val = cand_val; ka.cand_idx = cand_idx;
  for_topk_steps(R, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    const dim3 grid((unsigned)pl.qtiles, (unsigned)pl.slabs);
    if (pl.qt == 2) topk_scores_k<KS, 2><<<grid, kTopkWave, pl.lds_bytes, s>>>(ka);
    else topk_scores_k<KS, 1><<<grid, kTopkWave, pl.lds_bytes, s>>>(ka);
    AO_KERNEL_CHECK();
  });

  // levels of 32 slabs per workgroup until one workgroup per query is left; each level's output fits the other buffer
  double* in_val = cand_val;
  int* in_idx = cand_idx;
  double* to_val = pong_val;
  int* to_idx = pong_idx;
  int64_t slabs = pl.slabs;
  while (slabs > kTopkMergeGroup) {
    const int64_t groups = cdiv(slabs, kTopkMergeGroup);
    topk_merge_k<false><<<dim3((unsigned)a.nq, (unsigned)groups), kTopkWave, 0, s>>>(in_val, in_idx, slabs, kTopkMergeGroup, a.k, to_val,
                                                                                    to_idx, nullptr, nullptr);
    AO_KERNEL_CHECK();
    std::swap(in_val, to_val);
    std::swap(in_idx, to_idx);
    slabs = groups;
  }
  topk_merge_k<true><<<dim3((unsigned)a.nq, 1), kTopkWave, 0, s>>>(in_val, in_idx, slabs, slabs, a.k, nullptr, nullptr, a.out_idx, a.out_val);
  AO_KERNEL_CHECK();
}

double topk_bytes(int nd, int R, int64_t I, int64_t nq, int k, const TopkPlan& plan) {
  return (double)I * R * 8.0 * (double)plan.qtiles + (double)nq * (nd - 1) * (4.0 + 8.0 * R) + (double)nq * k * 16.0;
}

double topk_flops(int R, int64_t I, int64_t nq) { return 2.0 * (double)I * (double)nq * R; }

}  // namespace aoadmm
