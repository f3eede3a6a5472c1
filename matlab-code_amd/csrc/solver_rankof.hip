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

// The exclusion lists of a rank pass: offsets non-decreasing from 0, rows in range; every list sorted and stripped of
// repeats (a repeated row must not be subtracted twice), then cut into the chunks of the exclusion pass.  Shared by
// rank_of_run (per call) and set_ranklist (once per list).
void Engine::rank_prepare_excl(int p, int64_t I, int64_t nq, const int64_t* excl_off, const int64_t* excl_idx, RankExclHost& h) const {
  std::vector<int>& ex32 = h.ex32;
  std::vector<int>& chq = h.chq;
  std::vector<int64_t>& eoff64 = h.eoff64;
  std::vector<int64_t>& choff = h.choff;
  ex32.clear(); chq.clear(); eoff64.clear(); choff.clear();
  if (excl_off == nullptr) return;
  AO_REQUIRE(excl_off[0] == 0, "excl_off[0] = %lld, not 0", (long long)excl_off[0]);
  for (int64_t q = 0; q < nq; ++q)
    AO_REQUIRE(excl_off[q + 1] >= excl_off[q], "excl_off decreases at query %lld", (long long)q);
  const int64_t ne = excl_off[nq];
  ex32.resize((size_t)ne);
  for (int64_t e = 0; e < ne; ++e) {
    AO_REQUIRE(excl_idx[e] >= 0 && excl_idx[e] < I, "tensor %d: excluded row %lld at position %lld is outside [0, %lld)", p,
               (long long)excl_idx[e], (long long)e, (long long)I);
    ex32[(size_t)e] = (int)excl_idx[e];
  }
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

void Engine::rank_upload_excl(const RankExclHost& h, int64_t nq, DevBuf& eoff, DevBuf& eidx, DevBuf& coff, DevBuf& cq, RankArgs& a) {
  if (h.chq.empty()) return;
  eoff.alloc((size_t)(nq + 1) * sizeof(int64_t));
  eidx.alloc(h.ex32.size() * sizeof(int));
  coff.alloc((size_t)(nq + 1) * sizeof(int64_t));
  cq.alloc(h.chq.size() * sizeof(int));
  AO_HIP(hipMemcpyAsync(eoff.p, h.eoff64.data(), (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipMemcpyAsync(eidx.p, h.ex32.data(), h.ex32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipMemcpyAsync(coff.p, h.choff.data(), (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipMemcpyAsync(cq.p, h.chq.data(), h.chq.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  a.excl_off = eoff.as<int64_t>();
  a.excl_idx = eidx.as<int>();
  a.chunk_off = coff.as<int64_t>();
  a.chunk_q = cq.as<int>();
}

// subs (column `mode` holds the target; the weights are formed on the device) or W (nq x R column-major on the host,
// uploaded as it is) with targets
void Engine::rank_of_run(const char* what, int p, int mode, int64_t nq, const int64_t* subs, const double* W, const int64_t* targets,
                         const int64_t* excl_off, const int64_t* excl_idx, int64_t* rank_host, double* score_host, int64_t* ncand_host) {
  const bool given = subs == nullptr && W != nullptr;
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  if (t.par2)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s: tensor %d is a PARAFAC2 block; ranks of held-out entries are for CP blocks", what, p));
  const int nd = t.nmodes;
  AO_REQUIRE(nd >= 2 && nd <= kCooMaxModes, "tensor %d: order %d", p, nd);
  AO_REQUIRE(mode >= 0 && mode < nd, "tensor %d: mode %d outside [0, %d)", p, mode, nd);
  AO_REQUIRE(nq >= 0 && nq < ((int64_t)1 << 31), "nq = %lld outside [0, 2^31)", (long long)nq);
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
  const int64_t listed = (int64_t)xh.ex32.size(), chunks = (int64_t)xh.chq.size();

  AO_HIP(hipSetDevice(device_));
  const HeldoutFactors hf = heldout_factors(t, nullptr);
  const RankPlan pl = rank_plan(I, hf.R, nq, chunks);
  DevBuf idx, tgt, wgiven, eoff, eidx, coff, cq, ws, orank, oscore, oncand;
  ws.alloc(pl.workspace_bytes);
  orank.alloc((size_t)nq * sizeof(int64_t));
  oscore.alloc((size_t)nq * sizeof(double));
  oncand.alloc((size_t)nq * sizeof(int64_t));
  RankArgs a;
  a.hf = hf; a.mode = mode; a.I = I; a.nq = nq;
  std::vector<double> wrow;                            // the kernels read W row-major
  if (!given) {
    idx.alloc(idx32.size() * sizeof(int));
    AO_HIP(hipMemcpyAsync(idx.p, idx32.data(), idx32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    a.idx = idx.as<int>();
    a.target = idx.as<int>() + (size_t)mode * nq;
  } else {
    const int R = hf.R;
    wrow.resize((size_t)nq * R);
    for (int64_t q = 0; q < nq; ++q)
      for (int r = 0; r < R; ++r) wrow[(size_t)q * R + r] = W[(size_t)r * nq + q];
    wgiven.alloc(wrow.size() * sizeof(double));
    tgt.alloc(tgt32.size() * sizeof(int));
    AO_HIP(hipMemcpyAsync(wgiven.p, wrow.data(), wrow.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
    AO_HIP(hipMemcpyAsync(tgt.p, tgt32.data(), tgt32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    a.W = wgiven.d();
    a.target = tgt.as<int>();
  }
  rank_upload_excl(xh, nq, eoff, eidx, coff, cq, a);
  a.workspace = ws.p;
  a.rank = orank.as<int64_t>();
  a.score = oscore.d();
  a.ncand = oncand.as<int64_t>();
  KernelStats& ks = timers_.stats[kStatsTopk];           // counted with the top-k completions: no class of its own
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  rank_enqueue(a, pl, stream_);
  timers_.end(ks, pr, stream_, rank_bytes(nd, hf.R, I, nq, listed, pl), rank_flops(hf.R, I, nq, listed));
  // (the outputs are written last: a refusal above leaves them untouched)
  AO_HIP(hipMemcpyAsync(rank_host, orank.p, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipMemcpyAsync(score_host, oscore.p, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, stream_));
  if (ncand_host != nullptr) AO_HIP(hipMemcpyAsync(ncand_host, oncand.p, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

}  // namespace aoadmm
