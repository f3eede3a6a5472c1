// Top-k completions of a CP block along one mode.  For query q with a subscript for every mode
// but `mode`:
//   w_q(r) = prod_{m != mode} F_m(s_{q,m}, r),   score_q(i) = sum_r F_mode(i, r) w_q(r),   0 <= i < I_mode
// and the answer is the k rows that come first in the total order "larger score first, equal scores by smaller row"
// among the rows that are not in q's exclusion list and whose score is not NaN; (-1, -inf) pads a short answer.
// Three launches: the weights W (nq x R), the fused scores-and-selection pass over (row slabs) x (query tiles) that
// leaves k candidates per slab and query in a workspace, and the merge of the slabs' candidates.  The I_mode x nq
// score array never exists; the workspace is O(nq R + nq k slabs).  No float atomics, no dependence between the
// workgroups of a launch; a score's summation order depends on R alone, so the answer's bits are a function of the
// inputs only.
#pragma once
#include "common.h"
#include "heldout.h"

namespace aoadmm {

constexpr int kTopkMax = 64;         // k <= 64
constexpr int kTopkTile = 16;        // queries per MFMA tile: the column axis of v_mfma_f64_16x16x4_f64
constexpr int kTopkRows = 16;        // rows of F_mode per MFMA step; slabs are cut at multiples of it

struct TopkPlan {
  int qt = 1;                        // MFMA tiles per workgroup: 16 qt queries share one stream over the slab
  int64_t qtiles = 0, slabs = 0, slab_rows = 0;
  int cap = 0;                       // candidate buffer per query, >= k + kTopkRows
  size_t lds_bytes = 0;
  size_t workspace_bytes = 0;        // W, the slabs' candidates
};
TopkPlan topk_plan(int64_t I, int R, int64_t nq, int k);

struct TopkArgs {
  HeldoutFactors hf;                 // the block's factors as Engine::heldout_factors hands them out
  int mode = 0;
  int64_t I = 0;                     // rows of the free mode
  int64_t nq = 0;
  int k = 0;
  const int* idx = nullptr;          // device int32 [nd x nq]; row `mode` is not read
  const double* W = nullptr;         // device [nq x R] row-major or null; given: the weights launch is skipped, idx unused
  const int64_t* excl_off = nullptr; // device [nq + 1] or null: no exclusions
  const int* excl_idx = nullptr;     // device, every query's list sorted ascending
  void* workspace = nullptr;         // plan.workspace_bytes
  int64_t* out_idx = nullptr;        // device [nq x k]
  double* out_val = nullptr;         // device [nq x k]
};
void topk_enqueue(const TopkArgs& a, const TopkPlan& plan, hipStream_t s);
// the weights launch alone: W[q x R row-major] from idx (device int32 [nd x nq]; row `mode` is not read)
void topk_weights_enqueue(const HeldoutFactors& hf, int mode, int64_t nq, const int* idx, double* W, hipStream_t s);

// algorithmic bytes (F_mode streamed once per query tile, the gathered rows, the answer) and flops 2 I nq R
double topk_bytes(int nd, int R, int64_t I, int64_t nq, int k, const TopkPlan& plan);
double topk_flops(int R, int64_t I, int64_t nq);

}  // namespace aoadmm
