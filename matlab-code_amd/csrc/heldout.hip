// Held-out scoring: gather kernel over a list of subscripts and the finisher of its sums.  See heldout.h and DESIGN.md
// section 9.4.
#include <algorithm>

#include "heldout.h"

namespace aoadmm {

struct HeldoutArgs {
  const int* idx;       // [nd x n]
  const double* val;    // [n] (STAT == 1)
  int64_t n;
  HeldoutFactors hf;
  double* out;          // [n] (STAT == 0)
  double* part;         // kHeldoutSums per team (STAT == 1)
};

constexpr int kHeldoutUnroll = 4;   // entries whose gathers are in flight together (sparse_em.hip's kSemUnroll)

// the team sum of sem_pass_k: an xor butterfly, every lane ends with the same bits
template <int G>
__device__ __forceinline__ double team_sum(double v) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}

// The team layout of sem_pass_k / mttkrp_coo_k: G lanes walk kCooChunk consecutive entries of the list, lane r owns
// column r of every factor row; lanes beyond R read column R - 1 and contribute +0.
// ND = order (2..4 compiled in; 0: hf.nd at run time, up to kCooMaxModes)
// STAT 0: out[e] = m per entry; 1: three partial sums per team, accumulated in entry order, nothing else written
// P2 1: PARAFAC2 block (ND = 3): the second gather takes its base and stride from off[k]
template <int G, int ND, int STAT, int P2>
__global__ __launch_bounds__(256) void model_at_k(HeldoutArgs a) {
  const int64_t team = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int r = (int)(threadIdx.x % G);
  const int64_t start = team * kCooChunk;
  if (start >= a.n) return;                          // whole teams leave: the butterfly stays inside a team
  const int64_t end = start + kCooChunk < a.n ? start + kCooChunk : a.n;
  constexpr int NMAX = ND > 0 ? ND : kCooMaxModes;
  const int nd = ND > 0 ? ND : a.hf.nd;
  const int R = a.hf.R;
  const bool live = r < R;
  const int rr = live ? r : R - 1;
  double s_res = 0.0, s_y2 = 0.0, s_m2 = 0.0;
  for (int64_t i0 = start; i0 < end; i0 += kHeldoutUnroll) {
    double mu[kHeldoutUnroll], yu[kHeldoutUnroll];
#pragma unroll
    for (int u = 0; u < kHeldoutUnroll; ++u) {
      const int64_t i = i0 + u < end ? i0 + u : end - 1;   // clamped: every address is valid
      int64_t sub[NMAX];
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < nd) sub[n] = a.idx[(int64_t)n * a.n + i];
      double fv[NMAX];
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        if (n < nd) {
          if (P2 && n == 1) {
            constexpr int kmode = P2 ? 2 : 0;          // (an order-2 instance never takes this branch)
            const int64_t base = a.hf.off[sub[kmode]];
            const int64_t Jk = a.hf.off[sub[kmode] + 1] - base;
            fv[n] = a.hf.f[1].p[base * R + sub[1] + Jk * rr];
          } else {
            fv[n] = a.hf.f[n].p[sub[n] * a.hf.f[n].sI + rr * a.hf.f[n].sR];
          }
        }
      }
      if (STAT == 1) yu[u] = a.val[i];
      double m = 1.0;
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < nd) m *= fv[n];
      mu[u] = live ? m : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kHeldoutUnroll; ++u) mu[u] = team_sum<G>(mu[u]);
#pragma unroll
    for (int u = 0; u < kHeldoutUnroll; ++u) {
      if (i0 + u < end) {
        if (STAT == 0) {
          if (r == 0) a.out[i0 + u] = mu[u];
        } else {
          const double e = yu[u] - mu[u];
          s_res += e * e; s_y2 += yu[u] * yu[u]; s_m2 += mu[u] * mu[u];
        }
      }
    }
  }
  if (STAT == 1 && r == 0) {
    a.part[kHeldoutSums * team + 0] = s_res;
    a.part[kHeldoutSums * team + 1] = s_y2;
    a.part[kHeldoutSums * team + 2] = s_m2;
  }
}

// block-wide sum in a fixed order: every thread's value, then a tree over LDS
__device__ double heldout_block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

// One workgroup: the teams' partials in a fixed strided order, as sem_finish_k sums its own
__global__ __launch_bounds__(256) void heldout_finish_k(const double* part, int64_t nteams, double* sums) {
  __shared__ double sh[256];
  double p[kHeldoutSums] = {0.0, 0.0, 0.0};
  for (int64_t t = threadIdx.x; t < nteams; t += 256)
    for (int k = 0; k < kHeldoutSums; ++k) p[k] += part[kHeldoutSums * t + k];
  for (int k = 0; k < kHeldoutSums; ++k) {
    const double v = heldout_block_sum(p[k], sh);
    if (threadIdx.x == 0) sums[k] = v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int G, int STAT>
static void launch_nd(const HeldoutArgs& a, hipStream_t s) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, cdiv(heldout_teams(a.n) * G, 256));
  if (a.hf.off != nullptr) {
    model_at_k<G, 3, STAT, 1><<<grid, 256, 0, s>>>(a);
  } else {
    switch (a.hf.nd) {
      case 2: model_at_k<G, 2, STAT, 0><<<grid, 256, 0, s>>>(a); break;
      case 3: model_at_k<G, 3, STAT, 0><<<grid, 256, 0, s>>>(a); break;
      case 4: model_at_k<G, 4, STAT, 0><<<grid, 256, 0, s>>>(a); break;
      default: model_at_k<G, 0, STAT, 0><<<grid, 256, 0, s>>>(a); break;
    }
  }
  AO_KERNEL_CHECK();
}

template <int STAT>
static void launch(const HeldoutArgs& a, hipStream_t s) {
  const int R = a.hf.R;
  AO_REQUIRE(R >= 1 && R <= kMaxRank && a.hf.nd >= 2 && a.hf.nd <= kCooMaxModes && a.n > 0, "internal: held-out pass of rank %d, order %d", R, a.hf.nd);
  AO_REQUIRE(a.hf.off == nullptr || a.hf.nd == 3, "internal: held-out pass of a PARAFAC2 block of order %d", a.hf.nd);
  if (R <= 4) launch_nd<4, STAT>(a, s);
  else if (R <= 8) launch_nd<8, STAT>(a, s);
  else if (R <= 16) launch_nd<16, STAT>(a, s);
  else if (R <= 32) launch_nd<32, STAT>(a, s);
  else launch_nd<64, STAT>(a, s);
}

void heldout_model_at(const HeldoutFactors& hf, const int* idx, int64_t n, double* out, hipStream_t s) {
  HeldoutArgs a;
  a.idx = idx; a.val = nullptr; a.n = n; a.hf = hf; a.out = out; a.part = nullptr;
  launch<0>(a, s);
}

void heldout_stats_enqueue(const HeldoutFactors& hf, const int* idx, const double* val, int64_t n, double* part, double* sums,
                           hipStream_t s) {
  HeldoutArgs a;
  a.idx = idx; a.val = val; a.n = n; a.hf = hf; a.out = nullptr; a.part = part;
  launch<1>(a, s);
  heldout_finish_k<<<1, 256, 0, s>>>(part, heldout_teams(n), sums);
  AO_KERNEL_CHECK();
}

double heldout_pass_bytes(int nd, int R, int64_t n, bool stats) {
  return (double)n * (4.0 * nd + 8.0) + (double)n * nd * R * 8.0;   // stats: the value is read; else: it is written
}

double heldout_pass_flops(int nd, int R, int64_t n, bool stats) {
  return (double)n * R * nd + (stats ? 8.0 * (double)n : 0.0);
}

}  // namespace aoadmm
