// Engine: ranking metrics tracked inside a solve (rank_metrics.h).  The resident ranking list of a
// block, the evaluation a solve enqueues beside the objective, the settings and the trace it leaves.
#include "solver.h"
#include "rank_metrics.h"

#include <cmath>

namespace aoadmm {

bool Engine::has_ranklist() const {
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].rl.nq > 0) return true;
  return false;
}

// Arguments and validation are those of rank_of_run with subscripts; everything is checked and prepared before the
// previous list is touched.
void Engine::set_ranklist(int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off, const int64_t* excl_idx) {
  TensorInfo& t = query_block("aoadmm_tensor_set_ranklist", "ranks of held-out entries are for CP blocks", p, mode, nq);
  if (nq == 0) { t.rl.clear(); return; }
  AO_REQUIRE(subs != nullptr, "null subs");
  AO_REQUIRE(excl_off == nullptr || excl_idx != nullptr || excl_off[nq] == 0, "null excl_idx");
  const int64_t I = modes_[t.modes[mode]].rows;
  AO_REQUIRE(I < ((int64_t)1 << 31), "tensor %d: mode %d too long for int32 rows", p, mode);
  std::vector<int> idx32;
  heldout_check_subs(t, p, nq, subs, idx32);             // every column is range-checked: column `mode` holds the targets
  RankExclHost xh;
  rank_prepare_excl(p, I, nq, excl_off, excl_idx, xh);

  AO_HIP(hipSetDevice(device_));
  RankList l = rank_list_build(t, mode, nq, I, idx32, xh);
  l.part.alloc(rank_metrics_part_bytes(nq));
  AO_HIP(hipStreamSynchronize(stream_));                 // the host arrays go out of scope
  t.rl = std::move(l);
}

void Engine::ranklist_info(int p, int64_t* nq, int* mode, int64_t* listed, int64_t* resident_bytes) const {
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  const RankList& l = tensors_[p].rl;
  if (nq) *nq = l.nq;
  if (mode) *mode = l.nq > 0 ? l.mode : -1;
  if (listed) *listed = l.nq > 0 ? l.listed : 0;
  if (resident_bytes) *resident_bytes = l.nq > 0 ? l.resident_bytes() : 0;
}

void Engine::rank_track(int metric, int k, int every, int patience, int criterion) {
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(metric == AOADMM_RANK_HIT || metric == AOADMM_RANK_NDCG || metric == AOADMM_RANK_MRR || metric == AOADMM_RANK_AUC,
             "aoadmm_rank_track: metric = %d is no AOADMM_RANK_*", metric);
  AO_REQUIRE(k >= 1, "aoadmm_rank_track: k = %d outside [1, 2^31)", k);
  AO_REQUIRE(every >= 1, "aoadmm_rank_track: every = %d < 1", every);
  AO_REQUIRE(patience >= 0, "aoadmm_rank_track: patience = %d < 0", patience);
  AO_REQUIRE(criterion == 0 || criterion == 1, "aoadmm_rank_track: criterion = %d is neither 0 nor 1", criterion);
  AO_REQUIRE(patience == 0 || criterion == 1, "aoadmm_rank_track: patience = %d needs criterion = 1", patience);
  track_.metric = metric; track_.k = k; track_.every = every; track_.patience = patience; track_.criterion = criterion;
}

// The launches of a rank_of call against the fac state this evaluation uses (inside a solve: the row-major copies), then
// the two launches of the metric reduction into the arena.  Nothing is allocated or uploaded.
void Engine::ranklist_enqueue(int p, double* slots) {
  TensorInfo& t = tensors_[p];
  RankList& l = t.rl;
  const HeldoutFactors hf = heldout_factors(t, nullptr);
  const RankArgs a = l.args(hf);
  KernelStats& ks = timers_.stats[kStatsTopk];           // one launch count per list and evaluation, as a rank_of call
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  rank_enqueue(a, l.plan, stream_);
  rank_metrics_enqueue(a.rank, a.ncand, l.nq, track_.k, l.part.d(), slots, stream_);
  timers_.end(ks, pr, stream_, rank_bytes(l.nd, hf.R, l.I, l.nq, l.listed, l.plan), rank_flops(hf.R, l.I, l.nq, l.listed));
  l.evaluated = true;
}

// S of an evaluation from the landed arena: sum_p sum_p / sum_p n_p (n_auc for AUC); 0 / 0 is NaN
double Engine::rank_score(const ArenaView& h) const {
  const int num_slot = track_.metric == AOADMM_RANK_HIT ? kRankHits : track_.metric == AOADMM_RANK_NDCG ? kRankNdcg
                     : track_.metric == AOADMM_RANK_MRR ? kRankMrr : kRankAuc;
  const int den_slot = track_.metric == AOADMM_RANK_AUC ? kRankNAuc : kRankN;
  double num = 0.0, den = 0.0;
  for (int p = 0; p < n_tensors_; ++p) {
    if (tensors_[p].rl.nq == 0) continue;
    num += h.rank(p)[num_slot];
    den += h.rank(p)[den_slot];
  }
  return den > 0.0 ? num / den : std::nan("");
}

void Engine::rank_trace(int p, int what, double* out, int cap, int* len, int* iters, int* best_iter) const {
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(what >= 0 && what < kRankUsed, "aoadmm_rank_trace: what = %d is no AOADMM_RANKSUM_*", what);
  AO_REQUIRE(cap >= 0 && (cap == 0 || out != nullptr), "null trace buffer");
  const std::vector<double>& tr = tensors_[p].rl_trace;
  const int n = (int)(tr.size() / kRankSlots);
  for (int e = 0; e < cap && e < n; ++e) {
    out[e] = tr[(size_t)e * kRankSlots + what];
    if (iters) iters[e] = rank_iters_[(size_t)e];
  }
  if (len) *len = n;
  if (best_iter) *best_iter = n == 0 ? -1 : rank_best_iter_;
}

void Engine::ranklist_last(int p, int64_t* rank_host, double* score_host, int64_t* ncand_host) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  const RankList& l = tensors_[p].rl;
  AO_REQUIRE(l.nq > 0, "tensor %d has no ranking list (aoadmm_tensor_set_ranklist)", p);
  AO_REQUIRE(l.evaluated, "tensor %d: the ranking list has not been evaluated yet (aoadmm_solve evaluates it)", p);
  AO_HIP(hipSetDevice(device_));
  if (rank_host) AO_HIP(hipMemcpyAsync(rank_host, l.rank.p, (size_t)l.nq * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  if (score_host) AO_HIP(hipMemcpyAsync(score_host, l.score.p, (size_t)l.nq * sizeof(double), hipMemcpyDeviceToHost, stream_));
  if (ncand_host) AO_HIP(hipMemcpyAsync(ncand_host, l.ncand.p, (size_t)l.nq * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

}  // namespace aoadmm
