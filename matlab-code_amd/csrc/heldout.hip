// Held-out scoring: gather kernel over a list of subscripts and the finisher of its sums.  See heldout.h and DESIGN.md
// section 9.4.
#include "coo_team.h"
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

constexpr int kHeldoutUnroll = 4;   // entries whose gathers are in flight together

// The team layout of coo_team.h over the list, in the caller's order.
// ND = order (2..4 compiled in; 0: hf.nd at run time, up to kCooMaxModes)
// STAT 0: out[e] = m per entry; 1: three partial sums per team, accumulated in entry order, nothing else written
// P2 1: PARAFAC2 block (ND = 3): the second gather takes its base and stride from off[k]
template <int G, int ND, int STAT, int P2>
__global__ __launch_bounds__(256) void model_at_k(HeldoutArgs a) {
  const int R = a.hf.R;
  const CooTeam<G> t(a.n, R);
  if (t.idle()) return;
  const int64_t end = t.end();
  const int rr = t.rr();
  const bool live = t.live();
  constexpr int NMAX = ND > 0 ? ND : kCooMaxModes;
  const int nd = ND > 0 ? ND : a.hf.nd;
  double s_res = 0.0, s_y2 = 0.0, s_m2 = 0.0;
  for (int64_t i0 = t.start; i0 < end; i0 += kHeldoutUnroll) {
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
            fv[n] = coo_at(a.hf.f[n], sub[n], rr);
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
          if (t.r == 0) a.out[i0 + u] = mu[u];
        } else {
          const double e = yu[u] - mu[u];
          s_res += e * e; s_y2 += yu[u] * yu[u]; s_m2 += mu[u] * mu[u];
        }
      }
    }
  }
  if (STAT == 1 && t.r == 0) {
    a.part[kHeldoutSums * t.team + 0] = s_res;
    a.part[kHeldoutSums * t.team + 1] = s_y2;
    a.part[kHeldoutSums * t.team + 2] = s_m2;
  }
}

// One workgroup: the teams' partials in a fixed strided order, then the fixed tree of coo_block_sum
__global__ __launch_bounds__(256) void heldout_finish_k(const double* part, int64_t nteams, double* sums) {
  __shared__ double sh[256];
  double p[kHeldoutSums] = {0.0, 0.0, 0.0};
  for (int64_t t = threadIdx.x; t < nteams; t += 256)
    for (int k = 0; k < kHeldoutSums; ++k) p[k] += part[kHeldoutSums * t + k];
  for (int k = 0; k < kHeldoutSums; ++k) {
    const double v = coo_block_sum(p[k], sh);
    if (threadIdx.x == 0) sums[k] = v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int STAT>
static void launch(const HeldoutArgs& a, hipStream_t s) {
  const int R = a.hf.R;
  AO_REQUIRE(R >= 1 && R <= kMaxRank && a.hf.nd >= 2 && a.hf.nd <= kCooMaxModes && a.n > 0, "internal: held-out pass of rank %d, order %d", R, a.hf.nd);
  AO_REQUIRE(a.hf.off == nullptr || a.hf.nd == 3, "internal: held-out pass of a PARAFAC2 block of order %d", a.hf.nd);
  for_team_width(R, [&](auto g) {
    constexpr int G = decltype(g)::value;
    const unsigned grid = coo_team_grid(a.n, G);
    if (a.hf.off != nullptr) {
      model_at_k<G, 3, STAT, 1><<<grid, 256, 0, s>>>(a);
    } else {
      for_order<2>(a.hf.nd, [&](auto nd) { model_at_k<G, decltype(nd)::value, STAT, 0><<<grid, 256, 0, s>>>(a); });
    }
  });
  AO_KERNEL_CHECK();
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
