// Ranking-metric sums from ranks: the team pass over the queries and its one-workgroup finisher.  See rank_metrics.h and
// DESIGN.md section 9.8.
#include "coo_team.h"
#include "rank_metrics.h"

namespace aoadmm {

constexpr int kRankMetricsTeam = 64;     // a team is one wavefront: its loads of 64 consecutive queries are one line each
constexpr int kRankMetricsUnroll = 4;    // kCooChunk / 64: the whole chunk's loads are in flight together

// The team layout of coo_team.h over the queries, as model_at_k<..., STAT = 1> walks a held-out list, with one
// difference: a query has no columns to spread over the lanes, so lane r takes the queries start + r, + 64, + 128, ...
// of its team's chunk (in that order), and the team's sum is the xor butterfly of the lanes' sums.  Every team writes
// its own kRankUsed partials.
__global__ __launch_bounds__(256) void rank_metrics_k(const int64_t* __restrict__ rank, const int64_t* __restrict__ ncand, int64_t n,
                                                      int64_t k, double* __restrict__ part) {
  constexpr int G = kRankMetricsTeam;
  const CooTeam<G> t(n, G);
  if (t.idle()) return;
  const int64_t end = t.end();
  double s[kRankUsed];
#pragma unroll
  for (int j = 0; j < kRankUsed; ++j) s[j] = 0.0;
  for (int64_t i0 = t.start; i0 < end; i0 += (int64_t)G * kRankMetricsUnroll) {
    int64_t rk[kRankMetricsUnroll], nc[kRankMetricsUnroll];
#pragma unroll
    for (int u = 0; u < kRankMetricsUnroll; ++u) {
      const int64_t i = i0 + (int64_t)u * G + t.r;
      const int64_t ic = i < end ? i : end - 1;          // clamped: every address is valid
      rk[u] = rank[ic];
      nc[u] = ncand[ic];
    }
#pragma unroll
    for (int u = 0; u < kRankMetricsUnroll; ++u) {
      const bool in = i0 + (int64_t)u * G + t.r < end && rk[u] >= 0;
      const bool hit = in && rk[u] < k;
      const bool pair = in && nc[u] >= 2;
      const double r = (double)rk[u];
      s[kRankN] += in ? 1.0 : 0.0;
      s[kRankNAuc] += pair ? 1.0 : 0.0;
      s[kRankHits] += hit ? 1.0 : 0.0;
      s[kRankNdcg] += hit ? 1.0 / log2(r + 2.0) : 0.0;
      s[kRankMrr] += in ? 1.0 / (r + 1.0) : 0.0;
      s[kRankAuc] += pair ? 1.0 - r / ((double)nc[u] - 1.0) : 0.0;
    }
  }
#pragma unroll
  for (int j = 0; j < kRankUsed; ++j) s[j] = team_sum<G>(s[j]);
  if (t.r == 0) {
#pragma unroll
    for (int j = 0; j < kRankUsed; ++j) part[(int64_t)kRankUsed * t.team + j] = s[j];
  }
}

// One workgroup: the teams' partials in a fixed strided order, then the fixed tree of coo_block_sum (heldout_finish_k's
// order); the spare slots are written as zeros
__global__ __launch_bounds__(256) void rank_metrics_finish_k(const double* __restrict__ part, int64_t nteams, double* __restrict__ slots) {
  __shared__ double sh[256];
  double p[kRankUsed];
#pragma unroll
  for (int j = 0; j < kRankUsed; ++j) p[j] = 0.0;
  for (int64_t t = threadIdx.x; t < nteams; t += 256)
#pragma unroll
    for (int j = 0; j < kRankUsed; ++j) p[j] += part[(int64_t)kRankUsed * t + j];
#pragma unroll
  for (int j = 0; j < kRankUsed; ++j) {
    const double v = coo_block_sum(p[j], sh);
    if (threadIdx.x == 0) slots[j] = v;
  }
  if ((int)threadIdx.x >= kRankUsed && (int)threadIdx.x < kRankSlots) slots[threadIdx.x] = 0.0;
}

void rank_metrics_enqueue(const int64_t* rank, const int64_t* ncand, int64_t n, int64_t k, double* part, double* slots,
                          hipStream_t s) {
  AO_REQUIRE(rank != nullptr && ncand != nullptr && part != nullptr && slots != nullptr && n >= 1 && k >= 1, "internal: ranking-metric sums over %lld queries at k = %lld",
             (long long)n, (long long)k);
  static_assert(kCooChunk == kRankMetricsTeam * kRankMetricsUnroll, "one trip of the walk covers a team's chunk");
  rank_metrics_k<<<coo_team_grid(n, kRankMetricsTeam), 256, 0, s>>>(rank, ncand, n, k, part);
  AO_KERNEL_CHECK();
  rank_metrics_finish_k<<<1, 256, 0, s>>>(part, rank_metrics_teams(n), slots);
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
