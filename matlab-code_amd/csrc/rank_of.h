// The place of a known target row among the candidates of a query.  With w_q and score_q(i) of
// topk.h -- the same bits: the same product order for w_q, the same chain of ceil(R / 4) v_mfma_f64_16x16x4_f64 -- and a
// target row t_q per query:
//   score[q] = score_q(t_q)
//   rank[q]  = #{candidates c != t_q : score_q(c) > score[q], or score_q(c) == score[q] and c < t_q}; -1: score[q] is NaN
//   ncand[q] = #candidates
// where the candidates of q are the rows whose score is not NaN and that are not in q's exclusion list, and t_q itself
// whenever its score is not NaN (listed or not).  rank[q] is the 0-based place of t_q in top-k's total order.
// Launches: the weights (topk_weights_k's rule, skipped when W is given), the targets' scores, the counting pass over
// (query tiles) x (row slabs) that leaves two integers per slab and query, the pass over the exclusion lists, and the
// finisher.  The counting pass counts every row of F_mode; the exclusion pass counts the listed rows, and the finisher
// subtracts them: no row is looked up in a list.  Integer sums: the answer's bits are a function of the inputs only.
#pragma once
#include "common.h"
#include "heldout.h"
#include "topk.h"

namespace aoadmm {

constexpr int kRankExclChunk = 1024;   // listed rows one wave of the exclusion pass scores: 64 MFMA steps of 16 rows

struct RankPlan {
  TopkPlan tp;                         // qt, qtiles, slabs, slab_rows by topk_plan's rule at its smallest k (no buffers here)
  int64_t nq_pad = 0;                  // qtiles * qt * 16
  int64_t chunks = 0;                  // workgroups of the exclusion pass
  size_t workspace_bytes = 0;          // W, the targets' scores, the slabs' pairs, the chunks' pairs
};
RankPlan rank_plan(int64_t I, int R, int64_t nq, int64_t chunks);

struct RankArgs {
  HeldoutFactors hf;                   // the block's factors as Engine::heldout_factors hands them out
  int mode = 0;
  int64_t I = 0;                       // rows of the free mode
  int64_t nq = 0;
  const int* idx = nullptr;            // device int32 [nd x nq] or null when W is given; row `mode` is not read here
  const int* target = nullptr;         // device int32 [nq], every entry in [0, I)
  const double* W = nullptr;           // device [nq x R] row-major or null; given: the weights launch is skipped
  const int64_t* excl_off = nullptr;   // device [nq + 1] or null: no exclusions
  const int* excl_idx = nullptr;       // device, every query's list sorted ascending WITHOUT repeats
  const int64_t* chunk_off = nullptr;  // device [nq + 1]: the chunks of query q are chunk_off[q] .. chunk_off[q + 1] - 1
  const int* chunk_q = nullptr;        // device [chunks]: the query of a chunk
  void* workspace = nullptr;           // plan.workspace_bytes
  int64_t* rank = nullptr;             // device [nq]
  double* score = nullptr;             // device [nq]
  int64_t* ncand = nullptr;            // device [nq]
};
void rank_enqueue(const RankArgs& a, const RankPlan& plan, hipStream_t s);

// algorithmic bytes (F_mode streamed once per query tile, the rows gathered for the weights, the targets and the listed
// rows, the answer) and flops 2 I nq R + 2 R (listed rows + nq)
double rank_bytes(int nd, int R, int64_t I, int64_t nq, int64_t listed, const RankPlan& plan);
double rank_flops(int R, int64_t I, int64_t nq, int64_t listed);

}  // namespace aoadmm
