// Dense CP block: upload, pass copies, partial-contraction cache and the MTTKRP paths (see cpblock.h).
#include "cpblock.h"
#include "em.h"
#include "misc.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace aoadmm {

// ---- launch timing ---------------------------------------------------------
hipEvent_t LaunchTimers::take_event() {
  if (pool.empty()) {
    for (int i = 0; i < 64; ++i) {
      hipEvent_t e = nullptr;
      AO_HIP(hipEventCreate(&e));
      pool.push_back(e);
    }
  }
  hipEvent_t e = pool.back();
  pool.pop_back();
  return e;
}

// pairs whose second event has completed are added to ks.ms and their events go back to the pool (no synchronisation)
void LaunchTimers::fold_finished(KernelStats& ks) {
  size_t keep = 0;
  for (size_t i = 0; i < ks.pending.size(); ++i) {
    auto& pr = ks.pending[i];
    float t = 0.f;
    if (hipEventQuery(pr.second) == hipSuccess && hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) {
      ks.ms += t;
      pool.push_back(pr.first);
      pool.push_back(pr.second);
    } else {
      ks.pending[keep++] = pr;
    }
  }
  ks.pending.resize(keep);
}

LaunchTimers::Pair LaunchTimers::take_pair(KernelStats& ks) {
  Pair pr;
  if (ks.pending.size() >= 512) fold_finished(ks);     // a long solve never holds more than a few hundred events
  if (ks.pending.size() < 4096) { pr.e0 = take_event(); pr.e1 = take_event(); }
  return pr;
}

LaunchTimers::Pair LaunchTimers::begin(KernelStats& ks, bool timed, hipStream_t s) {
  Pair pr;
  if (timed) pr = take_pair(ks);
  if (pr.e0) AO_HIP(hipEventRecord(pr.e0, s));
  return pr;
}

void LaunchTimers::end(KernelStats& ks, Pair pr, hipStream_t s, double bytes, double flops) {
  if (pr.e0) AO_HIP(hipEventRecord(pr.e1, s));
  count(ks, pr, bytes, flops);
}

void LaunchTimers::count(KernelStats& ks, Pair pr, double bytes, double flops) {
  if (pr.e0) { ks.pending.emplace_back(pr.e0, pr.e1); ks.timed++; }
  ks.launches++;
  ks.bytes += bytes;
  ks.flops += flops;
}

// the events bracket the contraction kernel only (launch_contract records them)
static void timed_contract(const BlockCtx& cx, const void* X, int prec, const ContractPlan& pl, const double* F, int64_t ldF,
                           void* frag, void* T) {
  LaunchTimers& tm = *cx.timers;
  KernelStats& ks = tm.stats[pl.lead ? 1 : 0];
  LaunchTimers::Pair pr;
  static const bool no_events = getenv("AOADMM_NO_PASS_EVENTS") != nullptr;   // measurement only (tools/gap_analysis.py)
  // Every 4th pass is bracketed by events (the three kinds of pass alternate with period 3, so the sample cycles through
  // them): the records cost ~4 us of launch gap on each side of a pass -- nothing at 2000^3, 1 % of an iteration at one
  // rank's share of 8 GPUs.  kernel_stats() returns the mean of the timed launches times the launch count.
  // AOADMM_PASS_EVENT_EVERY=1 times every pass (the profile tools).
  static const int every = [] { const char* e = getenv("AOADMM_PASS_EVENT_EVERY"); const int v = e ? atoi(e) : 4; return v < 1 ? 1 : v; }();
  if (tm.profile && !no_events && ks.launches % every == 0) pr = tm.take_pair(ks);
  launch_contract(X, prec, pl, F, ldF, frag, T, cx.stream, pr.e0, pr.e1);
  tm.count(ks, pr, pl.algorithmic_bytes(prec), pl.flops());
}

// ---- data ------------------------------------------------------------------
static size_t blocked_bytes(int64_t M, int64_t C, size_t es) { return (size_t)round_up(M, kRowBlockElems) * C * es; }

// host array (rows x ncols, column-major fp64) -> dst in `prec` with the rows padded to `pad`, through the staging buffer
// (`bad01`: device flag raised when a value is not a finite number in [0, 1] -- the weights' way in)
static void upload_padded(const BlockCtx& cx, void* dst, int prec, int64_t pad, const double* host, int64_t rows, int64_t ncols,
                          int* bad01 = nullptr) {
  DevBuf& staging = *cx.staging;
  const int64_t chunk_cols = std::max<int64_t>(1, (int64_t)(64ll << 20) / rows);   // ~512 MB of doubles
  staging.ensure((size_t)std::min(chunk_cols, ncols) * rows * sizeof(double));
  for (int64_t c0 = 0; c0 < ncols; c0 += chunk_cols) {
    const int64_t nc = std::min(chunk_cols, ncols - c0);
    AO_HIP(hipMemcpyAsync(staging.p, host + c0 * rows, (size_t)nc * rows * sizeof(double), hipMemcpyHostToDevice, cx.stream));
    pad_convert(dst, prec, pad, staging.d(), rows, nc, c0, cx.stream);
    if (bad01) em_w_check(staging.d(), nc * rows, bad01, cx.stream);
    AO_HIP(hipStreamSynchronize(cx.stream));
  }
}

void block_upload(const BlockCtx& cx, CpBlock& b, int nd, const int64_t* dims, const double* host, int prec, int64_t row0,
                  int64_t local_rows, const double* full_array) {
  AO_REQUIRE(nd >= 2 && nd <= 8, "tensor order %d unsupported", nd);
  // AOADMM_PREC_F16: the entries are rounded to fp32 exactly as for AOADMM_PREC_F32, then block_make_half takes over
  const bool half = prec == AOADMM_PREC_F16;
  if (half) {
    AO_REQUIRE(nd == 3, "internal: half storage is for 3-way blocks (the callers refuse the rest)");
    prec = AOADMM_PREC_F32;
  }
  AO_REQUIRE(prec == AOADMM_PREC_F64 || prec == AOADMM_PREC_F32, "bad precision id %d", prec);
  AO_REQUIRE(row0 >= 0 && local_rows > 0 && row0 + local_rows <= dims[0], "bad row block [%lld,+%lld) of %lld",
             (long long)row0, (long long)local_rows, (long long)dims[0]);
  hipStream_t s = cx.stream;
  DevBuf& staging = *cx.staging;
  b.nd = nd;
  b.full0 = dims[0];
  b.row0 = row0;
  b.dims[0] = local_rows;
  int64_t ncols = 1;
  for (int i = 1; i < nd; ++i) { b.dims[i] = dims[i]; ncols *= dims[i]; }
  b.X.prec = prec; b.X.nd = nd;
  for (int i = 0; i < nd; ++i) b.X.dims[i] = b.dims[i];
  b.X.pad0 = pad_of(prec, local_rows);
  b.X.data.alloc((size_t)b.X.elems_padded() * b.X.elem_size());
  // host block layout: local_rows x ncols column-major (the caller extracted its rows)
  upload_padded(cx, b.X.data.p, prec, b.X.pad0, host, local_rows, ncols);
  if (nd == 2) {
    // transposed copy for the second mode (matrices are small next to tensors)
    b.Xt.prec = prec; b.Xt.nd = 2;
    b.Xt.dims[0] = dims[1]; b.Xt.dims[1] = local_rows;
    b.Xt.pad0 = pad_of(prec, dims[1]);
    b.Xt.data.alloc((size_t)b.Xt.pad0 * local_rows * b.Xt.elem_size());
    AO_REQUIRE(ncols * local_rows <= (int64_t)(1ll << 28), "matrix block too large for the transposed copy");
    staging.ensure((size_t)ncols * local_rows * sizeof(double));
    AO_HIP(hipMemcpyAsync(staging.p, host, (size_t)ncols * local_rows * sizeof(double), hipMemcpyHostToDevice, s));
    transpose_convert(b.Xt.data.p, prec, b.Xt.pad0, staging.d(), local_rows, ncols, s);
    AO_HIP(hipStreamSynchronize(s));
  }
  b.reset_derived();
  if (half) {                                         // no fp32 copy is ever built: peak 4 + 3 * 2 bytes per entry
    const SlabSource from_host = [&](DevBuf& slab, int64_t k0, int64_t kloc) {
      const int64_t I = dims[0], J = dims[1], Ipf = pad_of(AOADMM_PREC_F32, I);
      slab.alloc((size_t)Ipf * J * kloc * sizeof(float));
      upload_padded(cx, slab.p, AOADMM_PREC_F32, Ipf, full_array + (size_t)I * J * k0, I, J * kloc);   // contiguous in the caller's array
    };
    block_make_half(cx, b, full_array != nullptr ? &from_host : nullptr);
    return;
  }
  if (nd == 3 && full_array != nullptr) {             // the caller holds the whole tensor: mode-3 slab for the mode-1 pass
    int64_t k0 = 0, kloc = 0;
    if (want_ksharded_xp(cx, b, dims[2], &k0, &kloc)) {
      const int64_t I = dims[0], J = dims[1], Ipf = pad_of(prec, I);
      DevBuf slab;
      slab.alloc((size_t)Ipf * J * kloc * b.X.elem_size());
      upload_padded(cx, slab.p, prec, Ipf, full_array + (size_t)I * J * k0, I, J * kloc);   // X(:, :, k0 : k0+kloc) is contiguous
      adopt_ksharded_xp(cx, b, slab.p, k0, kloc);
      AO_HIP(hipStreamSynchronize(s));                // slab is a local
    }
  }
  if (nd == 3) { (void)ensure_pass_copy(cx, b, 1); (void)ensure_pass_copy(cx, b, 2); }   // one-off set-up cost belongs to the upload
}

// ---- per-entry weights -------------------------------------------------------
void block_reset_weighted(const BlockCtx& cx, CpBlock& b) {
  em_w_reset(b.X.data.p, b.X0.p, b.Wt.p, b.X.prec, b.X.elems_padded(), cx.stream);
  if (b.nd == 2) em_w_reset(b.Xt.data.p, b.X0t.p, b.WtT.p, b.Xt.prec, b.Xt.pad0 * b.dims[0], cx.stream);
  b.cached_mode = -1;
}

bool block_weights_in_range(const BlockCtx& cx, const double* host, int64_t n) {
  DevBuf& staging = *cx.staging;
  DevBuf flag;
  flag.alloc(sizeof(int));
  AO_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), cx.stream));
  const int64_t chunk = (int64_t)(64ll << 20);         // 512 MB of doubles, as upload_padded
  staging.ensure((size_t)std::min(chunk, n) * sizeof(double));
  for (int64_t e0 = 0; e0 < n; e0 += chunk) {
    const int64_t ne = std::min(chunk, n - e0);
    AO_HIP(hipMemcpyAsync(staging.p, host + e0, (size_t)ne * sizeof(double), hipMemcpyHostToDevice, cx.stream));
    em_w_check(staging.d(), ne, flag.as<int>(), cx.stream);
    AO_HIP(hipStreamSynchronize(cx.stream));           // the staging buffer is reused
  }
  int bad = 0;
  AO_HIP(hipMemcpy(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost));
  return bad == 0;
}

bool block_set_weights(const BlockCtx& cx, CpBlock& b, const double* host) {
  hipStream_t s = cx.stream;
  const int prec = b.X.prec;
  const int64_t rows = b.dims[0];
  int64_t ncols = 1;
  for (int i = 1; i < b.nd; ++i) ncols *= b.dims[i];
  const size_t bytes = (size_t)b.X.elems_padded() * b.X.elem_size();
  const size_t bytes_t = b.nd == 2 ? (size_t)b.Xt.pad0 * rows * b.Xt.elem_size() : 0;
  DevBuf W, WT, X0, X0t, flag;                         // the block changes only once everything is in place
  flag.alloc(sizeof(int));
  AO_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
  W.alloc(bytes);
  upload_padded(cx, W.p, prec, b.X.pad0, host, rows, ncols, flag.as<int>());
  if (b.nd == 2) {
    WT.alloc(bytes_t);
    cx.staging->ensure((size_t)ncols * rows * sizeof(double));
    AO_HIP(hipMemcpyAsync(cx.staging->p, host, (size_t)ncols * rows * sizeof(double), hipMemcpyHostToDevice, s));
    transpose_convert(WT.p, prec, b.Xt.pad0, cx.staging->d(), rows, ncols, s);
  }
  if (!b.has_weights) {                                // the data as the block holds it becomes X0
    X0.alloc(bytes);
    AO_HIP(hipMemcpyAsync(X0.p, b.X.data.p, bytes, hipMemcpyDeviceToDevice, s));
    if (b.nd == 2) {
      X0t.alloc(bytes_t);
      AO_HIP(hipMemcpyAsync(X0t.p, b.Xt.data.p, bytes_t, hipMemcpyDeviceToDevice, s));
    }
  }
  int bad = 0;
  AO_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));                     // the verdict is read back once, behind the last chunk
  if (bad) return false;
  if (!b.has_weights) { b.X0 = std::move(X0); b.X0t = std::move(X0t); }
  b.Wt = std::move(W); b.WtT = std::move(WT);
  b.has_weights = true;
  b.has_mask = false; b.mask.release(); b.maskT.release();   // w = 0 is the spelling of "missing"
  b.mlist.clear();                                     // the list was the mask's
  drop_pass_copies(b);                                 // the imputation would have to update them too
  block_reset_weighted(cx, b);
  AO_HIP(hipStreamSynchronize(s));
  return true;
}

void block_drop_weights(const BlockCtx& cx, CpBlock& b) {
  if (!b.has_weights) return;
  AO_HIP(hipMemcpyAsync(b.X.data.p, b.X0.p, (size_t)b.X.elems_padded() * b.X.elem_size(), hipMemcpyDeviceToDevice, cx.stream));
  if (b.nd == 2)
    AO_HIP(hipMemcpyAsync(b.Xt.data.p, b.X0t.p, (size_t)b.Xt.pad0 * b.dims[0] * b.Xt.elem_size(), hipMemcpyDeviceToDevice, cx.stream));
  AO_HIP(hipStreamSynchronize(cx.stream));
  b.clear_weights();
  b.cached_mode = -1;
}

// ---- half storage ----------------------------------------------------------
static bool room_for(size_t bytes);

void block_make_half(const BlockCtx& cx, CpBlock& b, const SlabSource* slab_source) {
  AO_REQUIRE(b.nd == 3 && b.X.prec == AOADMM_PREC_F32 && b.X.data.p && !b.imputed(),
             "internal: half storage is built from an unmasked fp32 3-way block");
  hipStream_t s = cx.stream;
  auto drop = [&] {                                    // the fp32 array is not the data: nothing valid is left
    drop_pass_copies(b);
    b.X.data.release();
    b.has_data = false; b.half = false; b.scale = 1.0; b.x_released = false; b.cached_mode = -1;
  };
  auto fail = [&](int code, const std::string& msg) { drop(); throw Error(code, msg); };
  drop_pass_copies(b);
  for (PassCopy& c : b.copy) c.refused = false;
  // largest magnitude and "not finite" over everything this rank holds: its rows, then its mode-3 slab (rows of other
  // ranks: they keep the values of a lone rank-share engine finite too, which learns nothing from peers)
  DevBuf stat, slab;
  int64_t k0 = 0, kloc = 0;
  bool ksh = false;
  uint32_t h2[2] = {0, 0};
  try {
    stat.alloc(2 * sizeof(uint32_t));
    tensor_absmax_f32(stat.as<uint32_t>(), b.X.data.as<float>(), b.X.elems_padded(), s);
    if (slab_source) {
      BlockCtx with_copies = cx;                       // the copies are the data: options.hip.no_permuted_copy has no say
      with_copies.allow_copies = true;
      ksh = want_ksharded_xp(with_copies, b, b.dims[2], &k0, &kloc);
    }
    if (ksh) {
      (*slab_source)(slab, k0, kloc);
      tensor_absmax_f32(stat.as<uint32_t>(), slab.as<float>(), pad_of(AOADMM_PREC_F32, b.full0) * b.dims[1] * kloc, s, true);
    }
    AO_HIP(hipMemcpyAsync(h2, stat.p, sizeof h2, hipMemcpyDeviceToHost, s));
    AO_HIP(hipStreamSynchronize(s));
  } catch (...) { drop(); throw; }                     // (a lone failure, like any out-of-memory in front of a collective)
  float amax;
  std::memcpy(&amax, &h2[0], sizeof amax);
  double gmax = (double)amax;
  bool bad = h2[1] != 0;
  if (cx.sharded) {
    // One sum all-reduce of world + 1 doubles: slot g holds rank g's maximum (zero from everyone else), the last slot
    // counts the ranks that saw a non-finite entry.  Every sum has one nonzero term or is a small integer: exact, and the
    // same bits on every rank.  Nothing above fails for a reason the data gives, so every rank gets here.
    std::vector<double> v((size_t)cx.world + 1, 0.0);
    v[(size_t)cx.rank] = gmax;
    v[(size_t)cx.world] = bad ? 1.0 : 0.0;
    try {
      DevBuf ex;
      ex.alloc(v.size() * sizeof(double));
      AO_HIP(hipMemcpyAsync(ex.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, s));
      cx.allreduce_from(cx.comm, ex.d(), ex.d(), (int64_t)v.size());
      AO_HIP(hipMemcpyAsync(v.data(), ex.p, v.size() * sizeof(double), hipMemcpyDeviceToHost, s));
      AO_HIP(hipStreamSynchronize(s));
    } catch (...) { drop(); throw; }
    gmax = *std::max_element(v.begin(), v.begin() + cx.world);
    bad = v[(size_t)cx.world] != 0.0;
  }
  if (bad) fail(AOADMM_ERR_INVALID, "half-precision storage: the tensor holds an entry that is not finite");
  // scale: a = max |x| = m * 2^E, m in [0.5, 1)  ->  s = 2^(15 - E), kept a normal fp32 number; all zeros: s = 1
  double scale = 1.0;
  if (gmax > 0.0) {
    int E;
    (void)std::frexp(gmax, &E);
    scale = std::ldexp(1.0, std::min(127, std::max(-126, 15 - E)));
  }
  const int64_t I = b.dims[0], J = b.dims[1], K = b.dims[2];
  for (int c = 0; c < 3; ++c) {
    PassCopy& pc = b.copy[c];
    const bool from_slab = c == 0 && ksh;              // rank g's X(:, :, K_g) with ALL of mode 1 (CpBlock::xp_ksharded)
    const int64_t pad = pad_of(AOADMM_PREC_F32, b.dims[(c + 1) % 3]);
    const size_t bytes = (size_t)(from_slab ? half_copy_elems(pad * kloc, b.full0) : half_copy_elems(pad * b.dims[(c + 2) % 3], b.dims[c])) * 2;
    if (!room_for(bytes)) fail(AOADMM_ERR_NOMEM, fmt("half-precision storage: no room in device memory for the pass copy of mode %d (%zu bytes)", c + 1, bytes));
    try { pc.buf.alloc(bytes); } catch (...) { drop(); throw; }
    pc.pad = pad;
    const bool ok = from_slab ? half_layout_copy(slab.p, pc.buf.p, 0, b.full0, pad_of(AOADMM_PREC_F32, b.full0), J, kloc, pad, (float)scale, s)
                              : half_layout_copy(b.X.data.p, pc.buf.p, c, I, b.X.pad0, J, K, pad, (float)scale, s);
    if (!ok)
      fail(AOADMM_ERR_UNSUPPORTED, fmt("half-precision storage: a mode of the tensor is too long for the copy kernels (pass copy of mode %d)", c + 1));
    pc.present = true;
    if (from_slab) {
      b.xp_ksharded = true; b.xp_k0 = k0; b.xp_kloc = kloc;
      AO_HIP(hipStreamSynchronize(s));                 // the copy was built from it on this stream
      slab.release();                                  // before the two other copies are allocated
    }
  }
  AO_HIP(hipStreamSynchronize(s));                     // the copies were built from it on this stream
  b.X.data.release();                                  // whatever AOADMM_RELEASE_NATURAL says: the fp32 array is not the data
  b.x_released = true; b.half = true; b.scale = scale; b.cached_mode = -1;
}

// ---- pass copies -----------------------------------------------------------
static bool room_for(size_t bytes) {
  size_t free_b = 0, total_b = 0;
  return hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= bytes + (size_t)(4ull << 30);
}

// Mode-3 sharding of the mode-1 pass's copy: every rank must reach the same verdict (the collectives that follow the
// pass differ: own rows of mode 3 instead of partial sums).
bool want_ksharded_xp(const BlockCtx& cx, const CpBlock& b, int64_t K, int64_t* k0, int64_t* kloc) {
  if (!cx.sharded || cx.world <= 1 || !cx.allow_copies || b.imputed() || b.nd != 3) return false;
  const int64_t per = cdiv(K, cx.world);
  if (per * (cx.world - 1) >= K) return false;        // some rank would own no slab
  *k0 = per * cx.rank;
  *kloc = std::min<int64_t>(K, *k0 + per) - *k0;
  return true;
}
void adopt_ksharded_xp(const BlockCtx& cx, CpBlock& b, const void* slab, int64_t k0, int64_t kloc) {
  const int64_t Ifull = b.full0, J = b.dims[1];
  const int prec = b.X.prec;
  PassCopy& pc = b.copy[0];
  pc.pad = pad_of(prec, J);
  pc.buf.alloc(blocked_bytes(pc.pad * kloc, Ifull, b.X.elem_size()));
  AO_REQUIRE(block_layout_copy(slab, pc.buf.p, 1, prec, Ifull, pad_of(prec, Ifull), J, kloc, pc.pad, cx.stream),
             "tensor mode too long for the copy kernels");
  pc.present = true; b.xp_ksharded = true; b.xp_k0 = k0; b.xp_kloc = kloc;
}

// The resident copy for the pass that contracts mode c, built from X on first use (at upload: 0, 1, 2 in this order).
// Refused when the mask of an EM problem would have to be kept in sync, when the caller opted out, or when HBM cannot
// hold it next to a 4 GiB reserve.  Copy 1 is only built beside copy 0; copy 2 stands alone.
bool ensure_pass_copy(const BlockCtx& cx, CpBlock& b, int c) {
  PassCopy& pc = b.copy[c];
  if (pc.present) return true;
  if (pc.refused) return false;
  if (c == 1 ? !ensure_pass_copy(cx, b, 0) : (!cx.allow_copies || b.imputed() || b.nd != 3)) return false;
  // rows: the two uncontracted modes in cyclic order after c, the first of them padded; columns: mode c
  const int64_t I = b.dims[0], J = b.dims[1], K = b.dims[2];
  const int64_t pad = c == 0 ? pad_of(b.X.prec, J) : (c == 1 ? pad_of(b.X.prec, K) : b.X.pad0);
  const size_t bytes = blocked_bytes(pad * b.dims[(c + 2) % 3], b.dims[c], b.X.elem_size());
  if (!room_for(bytes)) { pc.refused = true; return false; }
  pc.buf.alloc(bytes);
  pc.pad = pad;
  if (!block_layout_copy(b.X.data.p, pc.buf.p, (c + 1) % 3, b.X.prec, I, b.X.pad0, J, K, c == 2 ? 0 : pad, cx.stream)) {
    pc.buf.release(); pc.refused = true; return false;
  }
  pc.present = true;
  return true;
}

// Releases Z.object{p} in its natural layout once every tensor pass has its own resident copy.  A 2000^3 double array is
// 64 GB: with the natural array and three copies a MATLAB caller sat at 256 of 288 GB before any workspace.  Policy:
// AOADMM_RELEASE_NATURAL=1 always, =0 never, default: when less HBM is free than the array itself occupies.  Afterwards
// Z.miss cannot be attached without uploading the data again, and aoadmm_resident_unfold_gram answers
// AOADMM_ERR_UNSUPPORTED (the caller falls back to the host-array form).
void maybe_release_natural(const BlockCtx& cx, CpBlock& b, bool normsq_valid) {
  const bool all_copies = b.copy[0].present && b.copy[1].present && b.copy[2].present;
  if (b.sparse || b.x_released || b.nd != 3 || !all_copies || b.imputed() || !normsq_valid || !b.X.data.p) return;
  const char* pe = getenv("AOADMM_RELEASE_NATURAL");   // read per solve (the test suite switches it inside one process)
  const int policy = pe ? (atoi(pe) != 0 ? 1 : -1) : 0;
  if (policy < 0) return;
  if (policy == 0) {
    size_t free_b = 0, total_b = 0;
    const size_t mine = (size_t)b.X.elems_padded() * b.X.elem_size();
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b >= mine) return;
  }
  AO_HIP(hipStreamSynchronize(cx.stream));           // the copies were built from it on this stream
  b.X.data.release();
  b.x_released = true;
}

void drop_pass_copies(CpBlock& b) {
  for (int c = 0; c < 3; ++c) {
    PassCopy& pc = b.copy[c];
    if (!pc.present) continue;
    pc.buf.release(); pc.present = false; b.cached_mode = -1;
    if (c == 0) b.xp_ksharded = false;
  }
}

// ---- tensor pass -----------------------------------------------------------
int next_update_distance(int pos, int c, const int* seq, int n) {
  if (!seq || n <= 0) return c;            // no information: prefer the last mode
  int at = -1;
  for (int i = 0; i < n; ++i)
    if (seq[i] == pos) at = i;
  if (at < 0) return c;
  for (int d = 1; d <= n; ++d)
    if (seq[(at + d) % n] == c) return d;
  return n + 1;                              // never updated
}

// Tensor pass for a 3-way block (a cached partial contraction is reused while its factor is unchanged)
void ensure_contraction(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, int R, bool use_cache,
                        const int* update_seq, int nseq) {
  const int prec = b.X.prec;
  const int64_t I = b.dims[0], Ip = b.X.pad0, J = b.dims[1], K = b.dims[2];
  if (b.x_released) use_cache = true;                  // only the pass copies are resident (maybe_release_natural)
  const bool hit = use_cache && b.cached_mode >= 0 && b.cached_mode != pos &&
                   facs[b.cached_mode].version == b.cached_version;
  if (hit) return;
  // which mode to contract: any mode but `pos`; prefer the one whose factor stays unchanged longest so
  // that the partial contraction also serves the next update (cycle 3->{1,2}, 2->{3,1}, 1->{2,3}:
  // 1.5 tensor reads per outer iteration).  The leading mode needs the LDS-transposed kernel (fp32 only).
  int c = -1, best = -1;
  for (int cand = 2; cand >= 0; --cand) {
    if (cand == pos) continue;
    // contracting mode 1 needs its pass copy (any precision) or the LDS-transposed kernel (fp32 only)
    if (cand == 0 && !(use_cache && (prec == AOADMM_PREC_F32 || ensure_pass_copy(cx, b, 0)))) continue;
    const int dist = next_update_distance(pos, cand, update_seq, nseq);
    if (dist > best) { best = dist; c = cand; }
  }
  ContractPlan pl;
  const double* Fc = c == 0 ? facs[0].p + (cx.sharded ? b.row0 : 0) : facs[c].p;
  if (b.half) {                                        // the half copies are the data: always a pass on copy c
    AO_REQUIRE(b.copy[c].present, "internal: half block without its pass copy of mode %d", c + 1);
    const bool ksh = c == 0 && b.xp_ksharded;          // this rank's slab of mode 3 and ALL of mode 1, as below
    const int64_t M = b.copy[c].pad * (ksh ? b.xp_kloc : b.dims[(c + 2) % 3]), C = ksh ? b.full0 : b.dims[c];
    const int64_t MB = kRowBlockElems;
    pl = make_plan(round_up(M, MB) / MB, MB * round_up(C, kHalfGroupCols), MB, MB, C, R, AOADMM_PREC_F16);
    pl.on_copy = true;
    pl.xscale = b.scale;
    if (ksh) Fc = facs[0].p;
    b.T.ensure(pl.t_bytes()); b.frag.ensure(pl.frag_bytes(AOADMM_PREC_F16));
    timed_contract(cx, b.copy[c].buf.p, AOADMM_PREC_F16, pl, Fc, facs[c].ld, b.frag.p, b.T.p);
    b.cached_mode = c; b.cached_version = facs[c].version; b.plan = pl;
    return;
  }
  if (use_cache && ensure_pass_copy(cx, b, c)) {       // (mode 1 is only ever chosen with use_cache)
    // a pass on a row-blocked copy: one "batch" per row block, each a contiguous MB x C matrix.  With a communicator
    // copy 0 holds this rank's slab of mode 3 and ALL of mode 1 (CpBlock::xp_ksharded): a complete T of 1/N the size
    const bool ksh = c == 0 && b.xp_ksharded;
    const int64_t M = b.copy[c].pad * (ksh ? b.xp_kloc : b.dims[(c + 2) % 3]), C = ksh ? b.full0 : b.dims[c];
    const int64_t MB = kRowBlockElems;
    pl = make_plan(round_up(M, MB) / MB, MB * C, MB, MB, C, R, prec);
    pl.on_copy = true;
    if (ksh) Fc = facs[0].p;
  } else {                                             // on X itself
    if (c == 2) pl = make_plan(1, 0, Ip * J, Ip * J, K, R, prec);
    else if (c == 1) pl = make_plan(K, Ip * J, Ip, Ip, J, R, prec);
    else pl = make_lead_plan(J * K, Ip, I, R);
  }
  b.T.ensure(pl.t_bytes()); b.frag.ensure(pl.frag_bytes(prec));
  timed_contract(cx, pl.on_copy ? b.copy[c].buf.p : b.X.data.p, prec, pl, Fc, facs[c].ld, b.frag.p, b.T.p);
  b.cached_mode = c; b.cached_version = facs[c].version; b.plan = pl;
}

// ---- MTTKRP ----------------------------------------------------------------
// Where a path writes its result: the caller's buffer, or this rank's rows of a send buffer of the block (`send`)
struct MttkrpOut { double* p; int64_t ld; const double* send; };

// "Every rank fills its own rows of a zeroed buffer; the all-reduce is the all-gather": the zeroed buffer is a send
// buffer of the block that is cleared ONCE -- the rows of other ranks are never written, the own rows are overwritten
// by every MTTKRP -- and the all-reduce goes from it into `out` (a fill in front of every such MTTKRP was 5 us on the
// critical path, two per outer iteration).
static MttkrpOut own_rows_buffer(const BlockCtx& cx, CpBlock& b, int which, int64_t rows_full, int64_t row_first, int R) {
  DevBuf& ob = b.own[which];
  const size_t need = (size_t)rows_full * R * sizeof(double);
  if (b.own_bytes[which] != need || b.own_row0[which] != row_first) {    // (another rank's rows would stay behind)
    if (b.own_bytes[which] != need) ob.alloc(need);
    AO_HIP(hipMemsetAsync(ob.p, 0, need, cx.stream));
    b.own_bytes[which] = need;
    b.own_row0[which] = row_first;
  }
  return MttkrpOut{ob.d() + row_first, rows_full, ob.d()};
}

// out = sum over the ranks, from the own-rows send buffer (ld = rows) when there is one, else in place; column by column
// when the caller's leading dimension differs
static void mttkrp_allreduce(const BlockCtx& cx, const double* send, double* out, int64_t ldOut, int64_t rows_full, int R) {
  const double* src = send ? send : out;
  const int64_t ldS = send ? rows_full : ldOut;
  if (ldOut == rows_full) cx.allreduce_from(cx.comm, src, out, rows_full * R);
  else for (int r = 0; r < R; ++r) cx.allreduce_from(cx.comm, src + ldS * r, out + ldOut * r, rows_full);
}

// tiny block: the whole MTTKRP in one launch (contract.hip small_mttkrp_k), no partial-contraction cache
static void mttkrp_tiny(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, int R, double scale, double* out,
                        int64_t ldOut, const SysBuild* sys, bool* sys_done) {
  const int64_t I = b.dims[0], Ip = b.X.pad0, J = b.dims[1], K = b.nd == 3 ? b.dims[2] : 1;
  const int64_t st[3] = {1, Ip, Ip * J};
  const int64_t ext[3] = {I, J, K};
  int ia = pos == 0 ? 1 : 0, ib = pos == 2 ? 1 : 2;
  SmallMttkrp sm;
  sm.X = b.X.data.p;
  sm.sn = st[pos]; sm.sa = st[ia]; sm.Na = (int)ext[ia];
  sm.Fa = facs[ia].p; sm.lda = facs[ia].ld;
  if (b.nd == 3) { sm.sb = st[ib]; sm.Nb = (int)ext[ib]; sm.Fb = facs[ib].p; sm.ldb = facs[ib].ld; }
  else { sm.sb = 0; sm.Nb = 1; sm.Fb = nullptr; sm.ldb = 0; }
  sm.R = R; sm.scale = scale; sm.out = out; sm.ldOut = ldOut;
  const bool rode = small_mttkrp(sm, b.X.prec, ext[pos], cx.stream, sys);
  if (sys_done) *sys_done = rode;
}

// matrices: one pass over X (first mode) or over its transposed copy; F0: the first factor at this rank's rows
static void mttkrp_matrix(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, const double* F0, int R,
                          double scale, MttkrpOut o) {
  const int prec = b.X.prec;
  const int64_t I = b.dims[0], J = b.dims[1];
  const DenseTensor& X = pos == 0 ? b.X : b.Xt;
  const int64_t rows = pos == 0 ? I : J;
  ContractPlan pl = make_plan(1, 0, X.pad0, X.pad0, pos == 0 ? J : I, R, prec);
  b.T.ensure(pl.t_bytes()); b.frag.ensure(pl.frag_bytes(prec));
  timed_contract(cx, X.data.p, prec, pl, pos == 0 ? facs[1].p : F0, facs[1 - pos].ld, b.frag.p, b.T.p);
  launch_t_to_colmajor(b.T.p, pl.tprec, pl.nchunk, pl.trows(), rows, R, scale, o.p, o.ld, cx.stream);
  b.cached_mode = -1;
}

// 3-way: tensor pass (or its cached result), then one reduction over T
static void mttkrp_3way(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, const double* F0, int R, double scale,
                        bool use_cache, const int* update_seq, int nseq, bool sharded, MttkrpOut& o, const SysBuild* sys,
                        bool* sys_done) {
  const int64_t I = b.dims[0], Ip = b.X.pad0, J = b.dims[1], K = b.dims[2];
  ensure_contraction(cx, b, pos, facs, R, use_cache, update_seq, nseq);
  const int c = b.cached_mode;
  const ContractPlan& pl = b.plan;
  // the mode-1 pass on a copy sharded along mode 3: T(j, k in K_g, r) is complete; mode 3's output is this rank's rows
  const bool ksh = sharded && pl.on_copy && c == 0 && b.xp_ksharded;
  // T rows are (a + Apad*bb) with (a, bb) the two uncontracted modes in the order the pass's copy stores them:
  // tensor order on X and on copies 0 and 2, (k, i) on copy 1
  int ia = c == 0 ? 1 : 0, ib = c == 2 ? 1 : 2;
  if (pl.on_copy && c == 1) { ia = 2; ib = 0; }
  const int64_t ext[3] = {I, J, ksh ? b.xp_kloc : K};
  const int64_t An = ext[ia], Bn = ext[ib];
  const int64_t Apad = pl.on_copy ? b.copy[c].pad : (ia == 0 ? Ip : J);
  // factor of a mode: the first mode's factor is addressed at this rank's rows (the third mode's too under `ksh`)
  auto fac_p = [&](int m) { return m == 0 ? F0 : (m == 2 && ksh ? facs[2].p + b.xp_k0 : facs[m].p); };
  auto fac_pT = [&](int m) -> const double* {
    if (!facs[m].pT) return nullptr;
    if (m == 2 && ksh) return facs[2].pT + b.xp_k0 * R;
    return facs[m].pT + ((m == 0 && sharded) ? b.row0 * R : 0);
  };
  if (ksh && pos == 2) o = own_rows_buffer(cx, b, 1, K, b.xp_k0, R);   // own rows of the zeroed send buffer; the all-reduce is the all-gather
  // the reduction over T is timed like the passes (kernel_stats slot 2): it reads all of T once
  LaunchTimers& tm = *cx.timers;
  const LaunchTimers::Pair pr = tm.begin(tm.stats[2], tm.profile && tm.profile_reductions, cx.stream);
  bool rode;
  if (pos == ia) {
    b.scratch.ensure(reduce_outer_scratch_bytes(An, Bn, R));
    b.ft.ensure(reduce_factor_scratch_bytes(Bn, R));
    rode = launch_reduce_outer(b.T.p, pl.tprec, pl.nchunk, pl.trows(), An, Apad, Bn, R, fac_p(ib), facs[ib].ld, scale,
                               o.p, o.ld, b.scratch.d(), b.ft.d(), cx.stream, fac_pT(ib), 0, sys);
  } else {
    AO_REQUIRE(pos == ib, "internal: cached contraction cannot serve this mode");
    b.ft.ensure(reduce_factor_scratch_bytes(An, R));
    rode = launch_reduce_inner(b.T.p, pl.tprec, pl.nchunk, pl.trows(), An, Apad, Bn, R, fac_p(ia), facs[ia].ld, scale,
                               o.p, o.ld, b.ft.d(), cx.stream, fac_pT(ia), 0, sys);
  }
  if (sys_done) *sys_done = rode;
  tm.end(tm.stats[2], pr, cx.stream, (double)pl.t_bytes(), 0.0);
}

// N-way (N > 3): contract the last mode (the one before it when pos is last) on the matrix cores with all
// leading modes merged into the unfolding row, then fold the remaining modes one at a time over T: trailing
// modes with reduce_outer (down to pos), leading modes with reduce_inner (up to pos), each fold leaving a
// smaller T in the same [row][r] layout (fp64).  No partial-contraction reuse for these: N passes per iteration.
static void mttkrp_nway(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, const double* F0, int R, double scale,
                        MttkrpOut o) {
  const int prec = b.X.prec;
  const int64_t I = b.dims[0], Ip = b.X.pad0;
  hipStream_t s = cx.stream;
  const int N = b.nd;
  const int c = pos == N - 1 ? N - 2 : N - 1;
  int64_t lead = Ip;                                  // merged size of the modes before c (first one padded)
  for (int m = 1; m < c; ++m) lead *= b.dims[m];
  ContractPlan pl = (c == N - 1) ? make_plan(1, 0, lead, lead, b.dims[c], R, prec)
                                 : make_plan(b.dims[N - 1], lead * b.dims[c], lead, lead, b.dims[c], R, prec);
  b.T.ensure(pl.t_bytes()); b.frag.ensure(pl.frag_bytes(prec));
  timed_contract(cx, b.X.data.p, prec, pl, c == 0 ? F0 : facs[c].p, facs[c].ld, b.frag.p, b.T.p);
  // remaining modes in memory order, with their padded extents inside T
  int rem[8], nrem = 0;
  int64_t ext[8];
  for (int m = 0; m < N; ++m)
    if (m != c) { rem[nrem] = m; ext[nrem] = m == 0 ? Ip : b.dims[m]; ++nrem; }
  const void* Tin = b.T.p;
  int tprec = pl.tprec, nchunk = pl.nchunk;
  int64_t trows = pl.trows();
  int flip = 0;
  auto tbuf = [&](int64_t rows) {
    DevBuf& d = flip ? b.tmpB : b.tmpA;
    flip ^= 1;
    d.ensure((size_t)rows * R * sizeof(double));
    return d.d();
  };
  // fold trailing modes above pos (last remaining mode first)
  while (nrem > 1 && rem[nrem - 1] != pos) {
    const int mb = rem[nrem - 1];
    int64_t Arows = 1;
    for (int q = 0; q < nrem - 1; ++q) Arows *= ext[q];
    const bool last = nrem == 2;                      // after this fold only `pos` remains (it is rem[0])
    double* dst = last ? o.p : tbuf(Arows);
    const int64_t An = last ? (rem[0] == 0 ? I : b.dims[rem[0]]) : Arows;
    b.scratch.ensure(reduce_outer_scratch_bytes(An, b.dims[mb], R));
    b.ft.ensure(reduce_factor_scratch_bytes(b.dims[mb], R));
    launch_reduce_outer(Tin, tprec, nchunk, trows, An, Arows, b.dims[mb], R, facs[mb].p, facs[mb].ld,
                        last ? scale : 1.0, dst, last ? o.ld : 0, b.scratch.d(), b.ft.d(), s, nullptr, last ? 0 : 1);
    if (last) { nrem = 1; break; }
    Tin = dst; tprec = AOADMM_PREC_F64; nchunk = 1; trows = Arows;
    --nrem;
  }
  // fold leading modes below pos (first remaining mode first)
  while (nrem > 1) {
    const int ma = rem[0];
    int64_t Brows = 1;
    for (int q = 1; q < nrem; ++q) Brows *= ext[q];
    const bool last = nrem == 2;                      // after this fold only `pos` remains (it is rem[1])
    double* dst = last ? o.p : tbuf(Brows);
    const int64_t An = ma == 0 ? I : b.dims[ma];
    b.ft.ensure(reduce_factor_scratch_bytes(An, R));
    launch_reduce_inner(Tin, tprec, nchunk, trows, An, ext[0], Brows, R, ma == 0 ? F0 : facs[ma].p, facs[ma].ld,
                        last ? scale : 1.0, dst, last ? o.ld : 0, b.ft.d(), s, nullptr, last ? 0 : 1);
    Tin = dst; tprec = AOADMM_PREC_F64; nchunk = 1; trows = Brows;
    for (int q = 0; q + 1 < nrem; ++q) { rem[q] = rem[q + 1]; ext[q] = ext[q + 1]; }
    --nrem;
  }
  b.cached_mode = -1;
}

// MTTKRP of a sparse block (sparse.hip): factors gathered through their row-major copy when it is current.
// span_only: the share of a sharded block, into the rows of its span alone
static void sparse_mttkrp(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, int R, double scale, double* out,
                          int64_t ldOut, bool span_only) {
  CooFactor f[kCooMaxModes];
  int k = 0;
  for (int m = 0; m < b.nd; ++m) {
    if (m == pos) continue;
    f[k++] = facs[m].pT ? CooFactor{facs[m].pT, (int64_t)R, 1} : CooFactor{facs[m].p, 1, facs[m].ld};
  }
  LaunchTimers& tm = *cx.timers;
  const LaunchTimers::Pair pr = tm.begin(tm.stats[3], tm.profile, cx.stream);
  // observed-only block after an EM step: the imputed tensor is the residuals on the stored entries plus the snapshot's
  // model everywhere (sparse_em.h); before the first step the missing entries are 0 and this is the plain MTTKRP
  // a weighted block reads its residual array from the start: W o X before the first step (sem_reset)
  const bool imputed = b.sem.on && b.sem.have_snap;
  coo_mttkrp(b.coo, pos, f, R, scale, out, ldOut, cx.stream, span_only,
             imputed || (b.sem.on && b.sem.weighted) ? b.sem.res[pos].d() : nullptr);
  double bytes = coo_mttkrp_bytes(b.coo, pos, R), flops = coo_mttkrp_flops(b.coo, R);
  if (imputed) {
    AO_REQUIRE(b.sem.R == R, "observed-only block was marked for rank %d, the MTTKRP has rank %d", b.sem.R, R);
    SemFac sf[kCooMaxModes];
    for (int m = 0; m < b.nd; ++m) sf[m] = SemFac{facs[m].p, facs[m].ld, facs[m].pT};
    sem_mttkrp_correct(b.sem, pos, sf, scale, out, ldOut, cx.stream);
    for (int m = 0; m < b.nd; ++m) {                  // Fo_j'F_j of the other modes, then Fo_pos * W
      bytes += (m == pos ? 3.0 : 2.0) * (double)b.dims[m] * R * 8.0;
      flops += 2.0 * (double)b.dims[m] * R * R;
    }
  }
  tm.end(tm.stats[3], pr, cx.stream, bytes, flops);
}

// The send buffer of mode `pos` of a sharded sparse block (dims[pos] x R, leading dimension dims[pos]).  Invariant of
// every all-reduce from it: the rows outside the share's span are zero.  The span is fixed for the life of the CooBlock
// (a new upload, a new cut or a new model makes a new block without buffers), coo_mttkrp's span form writes inside the
// span only, and a buffer made for another R is made and cleared again here.
static double* sparse_send_buffer(const BlockCtx& cx, CooBlock& c, int pos, int R) {
  DevBuf& sb = c.send[pos];
  if (c.send_R[pos] != R || !sb.p) {
    const size_t need = (size_t)c.dims[pos] * R * sizeof(double);
    c.send_R[pos] = 0;
    sb.alloc(need);
    AO_HIP(hipMemsetAsync(sb.p, 0, need, cx.stream));
    c.send_R[pos] = R;
  }
  return sb.d();
}

// Sharded sparse block: this rank's partial MTTKRP into its span of the send buffer, all-reduced into `out` (the
// own-rows pattern of the dense path; neighbouring spans may share their boundary rows, which the sum completes).
// Every rank comes here for every MTTKRP, with an empty share too.
static void sparse_mttkrp_sharded(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, int R, double scale,
                                  double* out, int64_t ldOut, bool collective) {
  CooBlock& c = b.coo;
  AO_REQUIRE(collective, "internal: a sharded sparse block has no MTTKRP outside a collective");
  AO_REQUIRE(c.cut_rank == cx.rank && c.cut_world == cx.world,
             "sparse block was cut for rank %d of %d, the engine is now rank %d of %d: upload again", c.cut_rank, c.cut_world,
             cx.rank, cx.world);
  double* send = sparse_send_buffer(cx, c, pos, R);
  sparse_mttkrp(cx, b, pos, facs, R, scale, send, c.dims[pos], true);
  mttkrp_allreduce(cx, send, out, ldOut, c.dims[pos], R);
}

void block_mttkrp(const BlockCtx& cx, CpBlock& b, int pos, const FactorRef* facs, int R, double scale, double* out,
                  int64_t ldOut, bool use_cache, const int* update_seq, int nseq, bool collective, bool tensor_pass,
                  const SysBuild* sys, bool* sys_done) {
  if (sys_done) *sys_done = false;
  AO_REQUIRE(b.has_data, "tensor has no data");
  AO_REQUIRE(pos >= 0 && pos < b.nd, "mttkrp: mode %d out of range", pos);
  if (b.sparse) {                  // no cache, no rider; replicated: complete on every rank, no collective
    if (b.coo.sharded) sparse_mttkrp_sharded(cx, b, pos, facs, R, scale, out, ldOut, collective);
    else sparse_mttkrp(cx, b, pos, facs, R, scale, out, ldOut, false);
    return;
  }
  const bool sharded = collective && cx.sharded;
  const int64_t out_rows_full = (pos == 0) ? b.full0 : b.dims[pos];
  MttkrpOut o{out, ldOut, nullptr};
  if (sharded && pos == 0) o = own_rows_buffer(cx, b, 0, out_rows_full, b.row0, R);
  const double* F0 = facs[0].p + (sharded ? b.row0 : 0);     // local rows of the first factor
  if (!tensor_pass && small_direct(cx.sharded, b, R)) {
    mttkrp_tiny(cx, b, pos, facs, R, scale, out, ldOut, sys, sys_done);
    return;
  }
  if (b.nd == 2) mttkrp_matrix(cx, b, pos, facs, F0, R, scale, o);
  else if (b.nd == 3) mttkrp_3way(cx, b, pos, facs, F0, R, scale, use_cache, update_seq, nseq, sharded, o, sys, sys_done);
  else mttkrp_nway(cx, b, pos, facs, F0, R, scale, o);
  if (sharded) mttkrp_allreduce(cx, o.send, out, ldOut, out_rows_full, R);
}

}  // namespace aoadmm
