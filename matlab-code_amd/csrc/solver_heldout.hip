// Engine: held-out scoring (heldout.h).  The list of a block, the model at a list of subscripts,
// the pass a solve enqueues with every evaluation of the objective, and the trace it leaves.
#include "solver.h"

#include <cmath>

namespace aoadmm {

bool Engine::has_heldout() const {
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].ho.n > 0) return true;
  return false;
}

// The current fac state of the block's modes.  The row-major copies of the Gram kernel serve when every one of them is
// current (inside a solve they are), the column-major factors otherwise; the B_k slabs of a PARAFAC2 block have no such
// copy and are always gathered as par2.h stores them.
HeldoutFactors Engine::heldout_factors(const TensorInfo& t, bool* row_major) const {
  HeldoutFactors hf;
  hf.nd = t.nmodes;
  hf.R = modes_[t.modes[0]].R;
  bool all_current = true;
  for (int i = 0; i < t.nmodes; ++i) {
    const ModeInfo& o = modes_[t.modes[i]];
    AO_REQUIRE(o.has_fac, "G.fac{%d} missing", t.modes[i] + 1);
    if (!o.slabs && factor_ref(o).pT == nullptr) all_current = false;
  }
  for (int i = 0; i < t.nmodes; ++i) {
    const ModeInfo& o = modes_[t.modes[i]];
    if (o.slabs) { hf.f[i] = CooFactor{o.fac.d(), 1, 0}; continue; }
    const FactorRef fr = factor_ref(o);
    hf.f[i] = all_current ? CooFactor{fr.pT, (int64_t)hf.R, 1} : CooFactor{fr.p, 1, fr.ld};
  }
  if (t.par2) hf.off = t.p2.off_d.as<int64_t>();   // K + 1 prefix sums of J_k, on the device since add_par2
  if (row_major) *row_major = all_current;
  return hf;
}

// subs: column-major n x N int64, 0-based -> idx32 in the same layout.  A subscript out of range is AOADMM_ERR_INVALID.
// skip_mode: the column a caller gives another meaning (the free mode of a top-k query, the query number of a fold-in).
void Engine::heldout_check_subs(const TensorInfo& t, int p, int64_t n, const int64_t* subs, std::vector<int>& idx32, int skip_mode) const {
  const int nd = t.nmodes;
  AO_REQUIRE(nd >= 2 && nd <= kCooMaxModes, "tensor %d: order %d", p, nd);
  idx32.resize((size_t)nd * n);
  for (int m = 0; m < nd; ++m) {
    const ModeInfo& mi = modes_[t.modes[m]];
    if (mi.slabs || m == skip_mode) continue;        // the slab-valued mode is checked against J_k below
    AO_REQUIRE(mi.rows < ((int64_t)1 << 31), "tensor %d: mode %d too long for int32 subscripts", p, m);
    const int64_t* col = subs + (int64_t)m * n;
    for (int64_t e = 0; e < n; ++e) {
      AO_REQUIRE(col[e] >= 0 && col[e] < mi.rows, "tensor %d: subscript %lld of mode %d at entry %lld is outside [0, %lld)", p,
                 (long long)col[e], m, (long long)e, (long long)mi.rows);
      idx32[(size_t)m * n + e] = (int)col[e];
    }
  }
  if (t.par2) {
    const ModeInfo& mB = modes_[t.modes[1]];
    const int64_t* cj = subs + n;
    for (int64_t e = 0; e < n; ++e) {
      const int64_t Jk = mB.rows_k[idx32[(size_t)2 * n + e]];
      AO_REQUIRE(cj[e] >= 0 && cj[e] < Jk, "tensor %d: subscript %lld of mode 1 at entry %lld is outside slab %d of %lld rows", p,
                 (long long)cj[e], (long long)e, idx32[(size_t)2 * n + e], (long long)Jk);
      idx32[(size_t)n + e] = (int)cj[e];
    }
  }
}

void Engine::model_at(int p, int64_t n, const int64_t* subs, double* out_host) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(n >= 0, "n = %lld < 0", (long long)n);
  if (n == 0) return;
  AO_REQUIRE(subs != nullptr && out_host != nullptr, "null subs / out");
  TensorInfo& t = tensors_[p];
  std::vector<int> idx32;
  heldout_check_subs(t, p, n, subs, idx32);
  AO_HIP(hipSetDevice(device_));
  bool row_major = false;
  const HeldoutFactors hf = heldout_factors(t, &row_major);
  t.ho_row_major = row_major ? 1 : 0;
  DevBuf idx, out;
  idx.alloc(idx32.size() * sizeof(int));
  out.alloc((size_t)n * sizeof(double));
  AO_HIP(hipMemcpyAsync(idx.p, idx32.data(), idx32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  KernelStats& ks = timers_.stats[kStatsHeldout];
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  heldout_model_at(hf, idx.as<int>(), n, out.d(), stream_);
  timers_.end(ks, pr, stream_, heldout_pass_bytes(hf.nd, hf.R, n, false), heldout_pass_flops(hf.nd, hf.R, n, false));
  AO_HIP(hipMemcpyAsync(out_host, out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

void Engine::set_heldout(int p, int64_t n, const int64_t* subs, const double* vals) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n = %lld outside [0, 2^31)", (long long)n);
  TensorInfo& t = tensors_[p];
  if (n == 0) { t.ho.clear(); return; }
  AO_REQUIRE(subs != nullptr && vals != nullptr, "null subs / vals");
  std::vector<int> idx32;
  heldout_check_subs(t, p, n, subs, idx32);            // the previous list stays when anything below throws
  for (int64_t e = 0; e < n; ++e)
    AO_REQUIRE(std::isfinite(vals[e]), "tensor %d: held-out value %lld is not finite", p, (long long)e);
  AO_HIP(hipSetDevice(device_));
  HeldoutList l;
  l.nd = t.nmodes; l.n = n;
  l.idx.alloc(idx32.size() * sizeof(int));
  l.val.alloc((size_t)n * sizeof(double));
  l.part.alloc((size_t)kHeldoutSums * heldout_teams(n) * sizeof(double));
  AO_HIP(hipMemcpyAsync(l.idx.p, idx32.data(), idx32.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipMemcpyAsync(l.val.p, vals, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  t.ho = std::move(l);
}

void Engine::heldout_enqueue(int p, double* sums) {
  TensorInfo& t = tensors_[p];
  bool row_major = false;
  const HeldoutFactors hf = heldout_factors(t, &row_major);
  KernelStats& ks = timers_.stats[kStatsHeldout];
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  heldout_stats_enqueue(hf, t.ho.idx.as<int>(), t.ho.val.d(), t.ho.n, t.ho.part.d(), sums, stream_);
  timers_.end(ks, pr, stream_, heldout_pass_bytes(hf.nd, hf.R, t.ho.n, true), heldout_pass_flops(hf.nd, hf.R, t.ho.n, true));
  t.ho_row_major = row_major ? 1 : 0;
}

void Engine::heldout_stats(int p, double stats[4]) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(stats != nullptr, "null stats");
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(t.ho.n > 0, "tensor %d has no held-out list (aoadmm_tensor_set_heldout)", p);
  AO_HIP(hipSetDevice(device_));
  heldout_enqueue(p, dev_.heldout(p));
  double h[kHeldoutSums];
  AO_HIP(hipMemcpyAsync(h, dev_.heldout(p), sizeof h, hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  stats[0] = h[kHoRes]; stats[1] = h[kHoY2]; stats[2] = h[kHoM2]; stats[3] = (double)t.ho.n;
}

void Engine::heldout_info(int p, int64_t* n, int64_t* resident_bytes, int* row_major) const {
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  const HeldoutList& l = tensors_[p].ho;
  if (n) *n = l.n;
  if (resident_bytes) *resident_bytes = l.resident_bytes();
  if (row_major) *row_major = tensors_[p].ho_row_major;
}

void Engine::heldout_trace(int p, double* out, int cap, int* len, int* best_iter) const {
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(cap >= 0 && (cap == 0 || out != nullptr), "null trace buffer");
  const std::vector<double>& tr = tensors_[p].ho_trace;
  for (int i = 0; i < cap && i < (int)tr.size(); ++i) out[i] = tr[i];
  if (len) *len = (int)tr.size();
  if (best_iter) *best_iter = tr.empty() ? -1 : ho_best_iter_;
}

// ---------------------------------------------------------------------------
// the best held-out iterate (aoadmm_heldout_keep_best / aoadmm_heldout_restore_best)
// ---------------------------------------------------------------------------
// Every array aoadmm_state_get can return, in a fixed order; dst is filled in by best_build_table.  Of a slab-sharded
// PARAFAC2 block the slab-valued arrays contribute this rank's slabs [k0, k1) only: the others are stale until the
// gather that ends a solve, and the gather that follows a restore overwrites them again.
std::vector<SnapSeg> Engine::best_state_segments() const {
  std::vector<SnapSeg> segs;
  int64_t start = 0;
  auto add = [&](const DevBuf& buf, int64_t first, int64_t count) {
    if (count <= 0) return;
    AO_REQUIRE(buf.p != nullptr && (size_t)(first + count) * sizeof(double) <= buf.bytes, "internal: state array of %lld doubles in a buffer of %zu bytes",
               (long long)(first + count), buf.bytes);
    const int64_t bytes = count * (int64_t)sizeof(double);
    segs.push_back(SnapSeg{buf.as<char>() + first * (int64_t)sizeof(double), nullptr, bytes, start});
    start += bytes;
  };
  for (int m = 0; m < n_modes_; ++m) {
    const ModeInfo& mi = modes_[m];
    int64_t first = 0, count = mi.rows * mi.R;
    if (mi.slabs && mi.tensor >= 0 && tensors_[mi.tensor].p2.slab_sharded) {
      const Par2Block& b = tensors_[mi.tensor].p2;
      first = b.off_h[b.k0] * b.R;
      count = (b.off_h[b.k1] - b.off_h[b.k0]) * b.R;
    }
    if (mi.has_fac) add(mi.fac, first, count);
    if (mi.has_Z) add(mi.Z, first, count);
    if (mi.has_mu) add(mi.mu, first, count);
    if (mi.has_muD) add(mi.muD, 0, mi.muD_rows * mi.muD_cols);
  }
  for (int c = 0; c < n_couplings_; ++c)
    if (couplings_[c].has_state) add(couplings_[c].Delta, 0, couplings_[c].rows * couplings_[c].cols);
  for (int p = 0; p < n_tensors_; ++p) {
    if (!tensors_[p].par2) continue;
    const Par2Block& b = tensors_[p].p2;
    const int64_t first = b.slab_sharded ? b.off_h[b.k0] * b.R : 0;
    const int64_t count = (b.slab_sharded ? b.off_h[b.k1] - b.off_h[b.k0] : b.Jtot) * b.R;
    if (b.has_DeltaB) add(b.DeltaB, 0, (int64_t)b.R * b.R);
    add(b.P, first, count);
    add(b.muDB, first, count);
  }
  return segs;
}

void Engine::best_build_table() {
  best_.segs = best_state_segments();
  const int n = (int)best_.segs.size();
  int64_t cursor = 0;
  std::vector<int64_t> slot(n);
  for (int i = 0; i < n; ++i) {
    slot[i] = snapshot_slot_offset(cursor, best_.segs[i].src);
    cursor = slot[i] + best_.segs[i].bytes;
  }
  best_.store.ensure((size_t)cursor);
  std::vector<SnapSeg> both(2 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    SnapSeg& s = best_.segs[i];
    s.dst = best_.store.as<char>() + slot[i];
    both[i] = s;
    both[n + i] = SnapSeg{s.dst, const_cast<char*>(s.src), s.bytes, s.start};
  }
  best_.table.ensure(both.size() * sizeof(SnapSeg));
  // (the stream is synchronised before `both` goes out of scope: the first read-back of the solve has not been enqueued)
  AO_HIP(hipMemcpyAsync(best_.table.p, both.data(), both.size() * sizeof(SnapSeg), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  best_.bytes = n > 0 ? best_.segs[n - 1].start + best_.segs[n - 1].bytes : 0;
  best_.launches = 0;
  best_.moved = 0;
}

void Engine::best_snapshot(int iter) {
  (void)iter;
  state_snapshot_copy(best_.table.as<SnapSeg>(), (int)best_.segs.size(), best_.bytes, stream_);
  best_.launches += 1;
  best_.moved += 2 * best_.bytes;
}

void Engine::heldout_keep_best(int on) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(on == 0 || on == 1, "aoadmm_heldout_keep_best: on = %d is neither 0 nor 1", on);
  AO_HIP(hipSetDevice(device_));
  if (on == 0) { best_ = BestKeep(); return; }        // releases the copy
  best_.on = true;
}

// The kept state back into the engine's state.  What is derived from the factors follows their versions, as after
// aoadmm_state_set: the row-major copies, the cached tensor pass and the sparse slabs' Y are stale once the version
// moves, and the next solve computes the Gram matrices (of the B_k too) before anything reads them.
void Engine::heldout_restore_best(int* iter) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(best_.on && best_.iter >= 0, "no best iterate is kept: call aoadmm_heldout_keep_best(ctx, 1) and aoadmm_solve first");
  AO_HIP(hipSetDevice(device_));
  const std::vector<SnapSeg> now = best_state_segments();
  AO_REQUIRE(now.size() == best_.segs.size(), "internal: the state has %zu arrays, the kept copy %zu", now.size(), best_.segs.size());
  for (size_t i = 0; i < now.size(); ++i)
    AO_REQUIRE(now[i].src == best_.segs[i].src && now[i].bytes == best_.segs[i].bytes, "internal: state array %zu moved since the solve", i);
  const int n = (int)best_.segs.size();
  state_snapshot_copy(best_.table.as<SnapSeg>() + n, n, best_.bytes, stream_);
  for (ModeInfo& mi : modes_) mi.version++;
  prepared_mode_ = -1;
  for (int p = 0; p < n_tensors_; ++p) {
    TensorInfo& t = tensors_[p];
    if (!t.par2) {
      // The cached tensor pass: a solve of `iter` iterations ends with the partial contraction its last passes left, and
      // the next solve's first MTTKRP reduces over it (another contracted mode would give other rounding).  The passes of
      // one iteration are replayed on the restored factors; the factors do not move in between, which for three modes
      // leaves the same hits and misses.  (Z.miss: the final EM pass leaves no cached pass; iteration 0: none was made.)
      CpBlock& b = t.blk;
      const int R = modes_[t.modes[0]].R;
      b.cached_mode = -1;
      if (best_.iter > 0 && !t.masked() && !b.sparse && b.nd == 3 && !small_direct(sharded(), b, R)) {
        FactorRef facs[8];
        factor_refs(t, facs);
        const std::vector<int> seq = update_sequence(p);
        for (int pos : seq) ensure_contraction(block_ctx(), b, pos, facs, R, best_.use_dimtree, seq.data(), (int)seq.size());
      }
    }
    // Z.miss: the imputed entries of the data are those of the last iteration's model.  One imputation pass with the
    // restored factors writes what the EM step of iteration `iter` wrote (iteration 0 took no EM step: the data a solve
    // of 0 iterations leaves cannot be brought back, the entries stay as the last iteration left them).
    if (t.masked() && best_.iter > 0) em_pass_enqueue(p, 1);
    // observed-only: the next solve starts from missing entries at 0 whatever an earlier one left (solve_setup)
    if (t.observed_only()) sem_reset(t.blk.sem, t.blk.coo, stream_);
    if (t.par2) par2_gather_slabs(t);                 // slab-sharded: the other ranks' slabs, as at the end of a solve
  }
  AO_HIP(hipStreamSynchronize(stream_));
  if (iter) *iter = best_.iter;
}

void Engine::heldout_best_info(int* have, int* iter, int64_t* bytes, int64_t* launches) const {
  if (have) *have = best_.on && best_.iter >= 0 ? 1 : 0;
  if (iter) *iter = best_.on ? best_.iter : -1;
  if (bytes) *bytes = best_.moved;
  if (launches) *launches = best_.launches;
}

}  // namespace aoadmm
