// Engine: the place of a held-out target row among a query's candidates (rank_of.h).
#include "solver.h"
#include "rank_of.h"

#include <algorithm>

namespace aoadmm {

void Engine::rank_of(int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off, const int64_t* excl_idx, int64_t* rank_host,
                     double* score_host, int64_t* ncand_host) {
  rank_of_run("aoadmm_resident_rank_of", p, mode, nq, subs, nullptr, nullptr, excl_off, excl_idx, rank_host, score_host, ncand_host);
}

void Engine::rank_of_w(int p, int mode, int64_t nq, const double* W, const int64_t* targets, const int64_t* excl_off,
                       const int64_t* excl_idx, int64_t* rank_host, double* score_host, int64_t* ncand_host) {
  rank_of_run("aoadmm_resident_rank_of_w", p, mode, nq, nullptr, W, targets, excl_off, excl_idx, rank_host, score_host, ncand_host);
}

// The exclusion lists of a rank pass: checked (check_excl), every list sorted and stripped of repeats (a repeated row
// must not be subtracted twice), then cut into the chunks of the exclusion pass.  Shared by rank_of_run (per call) and
// set_ranklist (once per list).
void Engine::rank_prepare_excl(int p, int64_t I, int64_t nq, const int64_t* excl_off, const int64_t* excl_idx, RankExclHost& h) const {
  std::vector<int>& ex32 = h.ex32;
  std::vector<int>& chq = h.chq;
  std::vector<int64_t>& eoff64 = h.eoff64;
  std::vector<int64_t>& choff = h.choff;
  ex32.clear(); chq.clear(); eoff64.clear(); choff.clear();
  if (excl_off == nullptr) return;
  check_excl(p, I, nq, excl_off, excl_idx, ex32);
  eoff64.assign((size_t)nq + 1, 0);
  choff.assign((size_t)nq + 1, 0);
  int64_t out = 0;
  for (int64_t q = 0; q < nq; ++q) {
    std::sort(ex32.begin() + excl_off[q], ex32.begin() + excl_off[q + 1]);
    const auto last = std::unique(ex32.begin() + excl_off[q], ex32.begin() + excl_off[q + 1]);
    out = std::copy(ex32.begin() + excl_off[q], last, ex32.begin() + out) - ex32.begin();   // out <= excl_off[q]: moves left
    eoff64[(size_t)q + 1] = out;
    const int64_t nch = cdiv(out - eoff64[(size_t)q], (int64_t)kRankExclChunk);
    choff[(size_t)q + 1] = choff[(size_t)q] + nch;
    chq.insert(chq.end(), (size_t)nch, (int)q);
  }
  ex32.resize((size_t)out);
  AO_REQUIRE(choff[(size_t)nq] < ((int64_t)1 << 31), "%lld chunks of excluded rows: more than one launch holds", (long long)choff[(size_t)nq]);
}

void Engine::rank_upload_excl(const RankExclHost& h, RankList& l) {
  if (h.chq.empty()) return;
  const size_t offs = (size_t)(l.nq + 1) * sizeof(int64_t);
  l.eoff.alloc(offs);
  l.eidx.alloc(h.ex32.size() * sizeof(int));
  l.coff.alloc(offs);
  l.cq.alloc(h.chq.size() * sizeof(int));
  AO_HIP(hipMemcpyAsync(l.eoff.p, h.eoff64.data(), offs, hipMemcpyHostToDevice, stream_));
  AO_HIP(hipMemcpyAsync(l.eidx.p, h.ex32.data(), h.ex32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipMemcpyAsync(l.coff.p, h.choff.data(), offs, hipMemcpyHostToDevice, stream_));
  AO_HIP(hipMemcpyAsync(l.cq.p, h.chq.data(), h.chq.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
}

// The device side of nq checked queries: the plan, the subscripts (idx32 empty: rank_of_w, which has none), the lists,
// the workspace and the per-query outputs.  The uploads are asynchronous: the caller synchronises before idx32 and xh go.
RankList Engine::rank_list_build(const TensorInfo& t, int mode, int64_t nq, int64_t I, const std::vector<int>& idx32, const RankExclHost& xh) {
  RankList l;
  l.nq = nq; l.mode = mode; l.nd = t.nmodes; l.I = I;
  l.listed = (int64_t)xh.ex32.size();
  l.plan = rank_plan(I, modes_[t.modes[0]].R, nq, (int64_t)xh.chq.size());
  l.ws.alloc(l.plan.workspace_bytes);
  l.rank.alloc((size_t)nq * sizeof(int64_t));
  l.score.alloc((size_t)nq * sizeof(double));
  l.ncand.alloc((size_t)nq * sizeof(int64_t));
  if (!idx32.empty()) {
    l.idx.alloc(idx32.size() * sizeof(int));
    AO_HIP(hipMemcpyAsync(l.idx.p, idx32.data(), idx32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  }
  rank_upload_excl(xh, l);
  return l;
}

// subs (column `mode` holds the target; the weights are formed on the device) or W (nq x R column-major on the host,
// uploaded as it is) with targets
void Engine::rank_of_run(const char* what, int p, int mode, int64_t nq, const int64_t* subs, const double* W, const int64_t* targets,
                         const int64_t* excl_off, const int64_t* excl_idx, int64_t* rank_host, double* score_host, int64_t* ncand_host) {
  const bool given = subs == nullptr && W != nullptr;
  TensorInfo& t = query_block(what, "ranks of held-out entries are for CP blocks", p, mode, nq);
  if (nq == 0) return;
  AO_REQUIRE((subs != nullptr || (W != nullptr && targets != nullptr)) && rank_host != nullptr && score_host != nullptr,
             "null subs / W / targets / rank / score");
  AO_REQUIRE(excl_off == nullptr || excl_idx != nullptr || excl_off[nq] == 0, "null excl_idx");
  const int64_t I = modes_[t.modes[mode]].rows;
  AO_REQUIRE(I < ((int64_t)1 << 31), "tensor %d: mode %d too long for int32 rows", p, mode);

  // every column is range-checked: column `mode` holds the targets
  std::vector<int> idx32, tgt32;
  if (!given) {
    heldout_check_subs(t, p, nq, subs, idx32);
  } else {
    tgt32.resize((size_t)nq);
    for (int64_t q = 0; q < nq; ++q) {
      AO_REQUIRE(targets[q] >= 0 && targets[q] < I, "tensor %d: target %lld of query %lld is outside [0, %lld)", p, (long long)targets[q],
                 (long long)q, (long long)I);
      tgt32[(size_t)q] = (int)targets[q];
    }
  }
  RankExclHost xh;
  rank_prepare_excl(p, I, nq, excl_off, excl_idx, xh);

  AO_HIP(hipSetDevice(device_));
  const HeldoutFactors hf = heldout_factors(t, nullptr);
  const RankList l = rank_list_build(t, mode, nq, I, idx32, xh);
  RankArgs a = l.args(hf);
  DevBuf tgt, wgiven;
  std::vector<double> wrow;
  if (given) {
    upload_w_rows(W, nq, hf.R, wrow, wgiven);
    tgt.alloc(tgt32.size() * sizeof(int));
    AO_HIP(hipMemcpyAsync(tgt.p, tgt32.data(), tgt32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    a.idx = nullptr;
    a.W = wgiven.d();
    a.target = tgt.as<int>();
  }
  KernelStats& ks = timers_.stats[kStatsTopk];           // counted with the top-k completions: no class of its own
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  rank_enqueue(a, l.plan, stream_);
  timers_.end(ks, pr, stream_, rank_bytes(l.nd, hf.R, I, nq, l.listed, l.plan), rank_flops(hf.R, I, nq, l.listed));
  // (the outputs are written last: a refusal above leaves them untouched)
  AO_HIP(hipMemcpyAsync(rank_host, l.rank.p, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipMemcpyAsync(score_host, l.score.p, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, stream_));
  if (ncand_host != nullptr) AO_HIP(hipMemcpyAsync(ncand_host, l.ncand.p, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

}  // namespace aoadmm
