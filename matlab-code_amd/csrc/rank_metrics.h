// From ranks to ranking-metric sums on the device: what ranking.ranking_metrics computes on the
// host from the output of rank_of.h, as eight doubles that ride in a solve's read-back (readback.h, RankSlot).
//   n      = #{q : rank[q] >= 0}                       n_auc = #{q : rank[q] >= 0 and ncand[q] >= 2}
//   hits   = #{q : 0 <= rank[q] < k}                   ndcg  = sum over those of 1 / log2(rank[q] + 2)
//   mrr    = sum over rank[q] >= 0 of 1 / (rank[q] + 1)
//   auc    = sum over the n_auc queries of 1 - rank[q] / (ncand[q] - 1)
// Counts are doubles holding integers (exact below 2^53).  Two launches: rank_metrics_k leaves kRankUsed partial sums
// per team of kCooChunk queries, rank_metrics_finish_k (one workgroup) adds them in heldout_finish_k's order.  Every
// sum has a fixed order, there is no atomic and no dependence between workgroups: the bits are a function of
// (rank, ncand, k) alone.
#pragma once
#include "common.h"
#include "readback.h"
#include "sparse.h"

namespace aoadmm {

inline int64_t rank_metrics_teams(int64_t n) { return cdiv(n, kCooChunk); }
inline size_t rank_metrics_part_bytes(int64_t n) { return (size_t)kRankUsed * (size_t)rank_metrics_teams(n) * sizeof(double); }

// rank, ncand: device int64 [n], n >= 1; k >= 1; part: rank_metrics_part_bytes(n); slots: kRankSlots doubles (device)
void rank_metrics_enqueue(const int64_t* rank, const int64_t* ncand, int64_t n, int64_t k, double* part, double* slots,
                          hipStream_t s);

}  // namespace aoadmm
