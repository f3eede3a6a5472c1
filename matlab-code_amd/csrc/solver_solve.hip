// Engine: the AO-ADMM outer loop (functions/cmtf_fun_AOADMM.m:87-476) and its stopping rule
// (functions/evaluate_stopping_conditions.m) as a sequence of steps.  This file launches no kernel of its own.
#include "solver.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <set>

namespace aoadmm {

// The first tensor pass of the next outer iteration does not depend on the host's stopping decision, so
// it is enqueued before the host waits for the objective values: the round trip hides behind it.
bool Engine::prefetch_next_contraction(const aoadmm_options& opt) {
  if (!opt.use_dimtree) return false;
  for (int cid = -1; cid < n_couplings_; ++cid) {
    for (int p = 0; p < n_tensors_; ++p)
      for (int m = 0; m < n_modes_; ++m) {
        const ModeInfo& mi = modes_[m];
        if (mi.coupling != cid || mi.tensor != p) continue;
        TensorInfo& t = tensors_[p];                      // first mode the next iteration updates
        if (t.par2 || t.blk.sparse || t.blk.nd != 3 || small_direct(sharded(), t.blk, mi.R)) return false;
        FactorRef facs[8];
        factor_refs(t, facs);
        std::vector<int> seq = update_sequence(p);
        const KernelStats* ks = timers_.stats;
        const int64_t before = ks[0].launches + ks[1].launches;
        ensure_contraction(block_ctx(), t.blk, mi.pos, facs, mi.R, true, seq.data(), (int)seq.size());
        return ks[0].launches + ks[1].launches > before;     // false: the cached pass still serves
      }
  }
  return false;
}

std::vector<int> Engine::update_sequence(int p) const {
  // order in which the positions of tensor p are updated inside one outer iteration:
  // uncoupled modes first, then coupling ids ascending (cmtf_fun_AOADMM.m:10,89-93)
  std::vector<int> seq;
  const TensorInfo& t = tensors_[p];
  for (int cid = -1; cid < n_couplings_; ++cid)
    for (int i = 0; i < t.nmodes; ++i)
      if (modes_[t.modes[i]].coupling == cid) seq.push_back(i);
  return seq;
}

// ---------------------------------------------------------------------------
// per-mode pieces of the outer loop
// ---------------------------------------------------------------------------
void Engine::ensure_mode_work(ModeInfo& mi) {
  const size_t nR = (size_t)mi.rows * mi.R * sizeof(double), RR = (size_t)mi.R * mi.R * sizeof(double);
  mi.A.ensure(nR); mi.Ab.ensure(nR);
  mi.gram.ensure(RR); mi.C.ensure(RR); mi.Bsys.ensure(RR); mi.L.ensure(RR); mi.Binv.ensure(RR);
  mi.rho.ensure(64);
  mi.Zold.ensure(nR); mi.V.ensure(nR); mi.Znew.ensure(nR); mi.RHS.ensure(nR); mi.TD.ensure(nR); mi.tmp.ensure(nR);
  mi.part.ensure((size_t)admm_partials(mi.rows) * 4 * sizeof(double));
  if (mi.constrained) mi.proxws.ensure(prox_ws_bytes(mi.prox.type, mi.rows, mi.R));
  mi.facT.ensure(nR);
  atbws_.ensure(admm_mode_ws_bytes(mi.rows, mi.R));    // covers atb_ws_bytes: the Gram kernel and the loop's fold partials
}

// Gram of the current factor (:66, :148); the same kernel leaves a row-major copy of the factor for the T
// reductions, recorded as belonging to the factor's current version.  (A constrained CP mode gets both from
// admm_mode_update, whose last kernel also closes the mode's ADMM loop.)
void Engine::compute_gram(ModeInfo& mi) {
  mi.facT.ensure((size_t)mi.rows * mi.R * sizeof(double));
  atb_small(mi.gram.d(), mi.fac.d(), mi.rows, mi.fac.d(), mi.rows, mi.rows, mi.R, mi.R, atbws_.d(), nullptr, stream_,
            mi.facT.d());
  mi.facT_version = mi.version;
}

// system of a coupled mode: +rho/2*I (types 0, 3, 4: :269, :336, :358), +rho/2*H*H' (type 2, :314), nothing for the
// Sylvester types 1, 5 (:288-293, :377-382); +rho/2*I more if constrained
int Engine::coupled_nrho(int m) const {
  const int cty = couplings_[modes_[m].coupling].type;
  const int con = modes_[m].constrained ? 1 : 0;
  return (cty == 0 || cty == 3 || cty == 4) ? 1 + con : (cty == 2 ? con : 0);
}

// sys_build of CP mode m into the mode's own buffers; the caller names the source of C (grams or Cpre), w and bsum_half
SysBuild Engine::mode_sysbuild(int m, int nrho) {
  ModeInfo& mi = modes_[m];
  SysBuild sb;
  sb.ngram = 0;
  sb.Cpre = nullptr;
  sb.w = 1.0;
  sb.ridge = has_ridge_ ? mi.ridge : 0.0;
  sb.bsum_half = 0.0;
  sb.rho_scale = 1.0;
  sb.nrho = nrho;
  sb.R = mi.R;
  sb.C = mi.C.d(); sb.rho = mi.rho.d(); sb.Bsys = mi.Bsys.d(); sb.L = mi.L.d();
  sb.Binv = nrho > 0 ? mi.Binv.d() : nullptr;
  sb.ctl = ctl_of_mode(m);
  const int cty = mi.coupling >= 0 ? couplings_[mi.coupling].type : -1;
  if (cty == 2) sb.Madd = mi.HHt.d();
  return sb;
}

// what follows the right-hand side A of mode m: the system unless it rode in the MTTKRP's launch, and for the
// Sylvester types the eigenvectors of the system matrix
void Engine::close_mode_system(int m, const SysBuild& sb, bool build, const double* A) {
  ModeInfo& mi = modes_[m];
  if (build) sys_build(sb, stream_);
  const int cty = mi.coupling >= 0 ? couplings_[mi.coupling].type : -1;
  if (cty == 1 || cty == 5) {                       // B = V diag(mu) V' for the Sylvester solve of the inner loop
    mi.eV.ensure((size_t)mi.R * mi.R * sizeof(double)); mi.eMu.ensure((size_t)mi.R * sizeof(double));
    sym_eig_small(mi.Bsys.d(), mi.R, mi.eMu.d(), mi.eV.d(), stream_);
  }
  mi.Aeff = A;
}

void Engine::prepare_mode_system(int m, int nrho, const aoadmm_options& opt) {
  ModeInfo& mi = modes_[m];
  TensorInfo& t = tensors_[mi.tensor];
  if (t.par2) {                      // first PARAFAC2 mode: same system, different A and C (:159-178)
    AO_REQUIRE(mi.pos == 0, "internal: only the first PARAFAC2 mode goes through the CP-style system");
    par2_prepare_modeA(m, nrho, opt);
    return;
  }
  FactorRef facs[8];
  factor_refs(t, facs);
  std::vector<int> seq = update_sequence(mi.tensor);
  SysBuild sb = mode_sysbuild(m, nrho);
  for (int i = 0; i < t.nmodes; ++i)
    if (i != mi.pos) sb.grams[sb.ngram++] = modes_[t.modes[i]].gram.d();     // :98-103, :109,:112
  sb.w = t.weight;
  sb.bsum_half = opt.bsum ? opt.bsum_weight / 2 : 0.0;
  // The system needs the Gram matrices only: it rides in the launch of the reduction that finishes the MTTKRP (one
  // extra workgroup) when that path is taken, else it gets its own launch behind the MTTKRP.
  bool rode = false;
  block_mttkrp(block_ctx(), t.blk, mi.pos, facs, mi.R, t.weight, mi.A.d(), mi.rows, opt.use_dimtree != 0, seq.data(), (int)seq.size(), true,
               false, &sb, &rode);
  close_mode_system(m, sb, !rode, mi.A.d());
  t.last_pos = mi.pos;                                                        // :121-123
  if (opt.bsum) {                                                             // :124-127
    Coef c[2] = {coef(1.0), coef(opt.bsum_weight / 2)};
    const double* x[2] = {mi.A.d(), mi.fac.d()};
    ew_lincomb(mi.Ab.d(), mi.rows * mi.R, 2, c, x, nullptr, stream_);
    mi.Aeff = mi.Ab.d();
  }
}

// see enqueue_objective(): the first uncoupled CP mode of the next iteration, prepared ahead
void Engine::prepare_next_first_mode(const aoadmm_options& opt) {
  for (int p = 0; p < n_tensors_; ++p)
    for (int m = 0; m < n_modes_; ++m) {
      const ModeInfo& mi = modes_[m];
      if (mi.coupling != -1 || mi.tensor != p) continue;
      if (tensors_[p].par2 && mi.pos != 0) return;  // a PARAFAC2 B_k or C mode comes first: nothing ahead
      prepare_mode_system(m, mi.constrained ? 1 : 0, opt);   // (the first PARAFAC2 mode goes through the same call, :159-178)
      prepared_mode_ = m;
      return;
    }
}

void Engine::update_uncoupled_cp_mode(int m, const aoadmm_options& opt) {
  ModeInfo& mi = modes_[m];
  if (prepared_mode_ == m) prepared_mode_ = -1;     // MTTKRP and system were enqueued at the end of the last iteration
  else prepare_mode_system(m, mi.constrained ? 1 : 0, opt);
  if (!mi.constrained) {
    // G.fac{m} = A{m}/B{m}  (:134): B is symmetric positive definite -> Cholesky solve
    row_solve(mi.fac.d(), mi.rows, mi.Aeff, mi.rows, mi.L.d(), mi.rows, mi.R, nullptr, stream_);
    mi.version++;
    compute_gram(mi);                                                           // :148
    return;
  }
  // the ADMM loop on the path admm_path() names, the Gram matrix (:148) and the row-major copy
  AdmmMode am;
  am.A = mi.Aeff; am.L = mi.L.d(); am.Binv = mi.Binv.d(); am.rho = mi.rho.d();
  am.fac = mi.fac.d(); am.Z = mi.Z.d(); am.mu = mi.mu.d();
  am.rows = mi.rows; am.R = mi.R; am.prox = mi.prox;
  admm_mode_update(am, mi.part.d(), mi.V.d(), mi.Znew.d(), mi.proxws.d(), mi.gram.d(), mi.facT.d(), atbws_.d(),
                   ctl_of_mode(m), opt.MaxInnerIters, opt.innerRelPrTol_constr, opt.innerRelDualTol_constr, stream_);
  mi.version++;
  mi.facT_version = mi.version;
}

static bool stop_one(double f, double fo, const aoadmm_options& o) {
  const double rel = fo > 0 ? std::fabs(fo - f) / fo : std::fabs(fo - f);    // evaluate_stopping_conditions.m:8-15
  return f < o.AbsFuncTol || rel < o.OuterRelTol;
}

// ---------------------------------------------------------------------------
// the outer loop
// ---------------------------------------------------------------------------
namespace {
// pinned landing area + event: the host waits for the objective values only, not for work enqueued
// behind them (prefetch_next_contraction)
struct Landing {
  void* p = nullptr; hipEvent_t ev = nullptr;
  Landing() = default;
  Landing(const Landing&) = delete;
  Landing& operator=(const Landing&) = delete;
  ~Landing() { if (p) (void)hipHostFree(p); if (ev) (void)hipEventDestroy(ev); }
  void alloc(size_t bytes) {
    AO_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    AO_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
};
}  // namespace

struct SolveRun {
  const aoadmm_options& opt;
  aoadmm_result* out;
  Landing pin;
  ArenaView host;                                   // the arena as it landed in pin.p
  bool has_miss = false;
  double f[4] = {0, 0, 0, 0};                       // f_tensors, f_couplings, f_constraints, f_PAR2_couplings
  double f_rel_missing = 0.0;
  bool has_ho = false;                              // some block has a held-out list
  double ho_best = 0.0;                             // smallest H_i = sum_p w_p sum (y - m)^2 so far ...
  int ho_bad = 0;                                   // ... and the iterations since that were not strictly below it
  bool has_rl = false;                              // some block has a ranking list
  bool rk_select = false;                           // aoadmm_rank_track criterion = 1: S selects the kept iterate and may stop the solve
  double rk_best = 0.0;                             // largest pooled score S so far ...
  int rk_bad = 0;                                   // ... and the evaluations since that did not improve on it
  std::chrono::steady_clock::time_point t0;
};

// State checks and everything a solve needs before its first evaluation: work buffers, the Gram matrices (:62-81),
// Znorm_const, the PARAFAC2 blocks' sharding and their B_k Gram matrices.
void Engine::solve_setup(const aoadmm_options& opt) {
  prepared_mode_ = -1;                                // nothing prepared ahead by an earlier solve is valid for this state
  if (opt.no_permuted_copy != 0)
    for (int p = 0; p < n_tensors_; ++p)
      AO_REQUIRE(tensors_[p].par2 || !tensors_[p].blk.half,
                 "options.hip.no_permuted_copy = 1 cannot be honoured: tensor %d is stored in half precision and its pass copies are the data", p);
  allow_xp_ = opt.no_permuted_copy == 0;
  if (!allow_xp_)
    for (int p = 0; p < n_tensors_; ++p)
      drop_pass_copies(tensors_[p].blk);
  for (int p = 0; p < n_tensors_; ++p) {
    AO_REQUIRE(tensors_[p].blk.has_data, "tensor %d has no data (Z.object{%d})", p, p + 1);
  }
  for (int m = 0; m < n_modes_; ++m) {
    ModeInfo& mi = modes_[m];
    AO_REQUIRE(mi.has_fac, "G.fac{%d} missing", m + 1);
    if (mi.constrained) AO_REQUIRE(mi.has_Z && mi.has_mu, "G.constraint_fac{%d} / constraint_dual_fac{%d} missing", m + 1, m + 1);
    if (mi.coupling >= 0) {
      AO_REQUIRE(mi.has_muD && mi.muD_rows == mi.img_rows && mi.muD_cols == mi.img_cols, "G.coupling_dual_fac{%d} missing or mis-sized", m + 1);
      AO_REQUIRE(couplings_[mi.coupling].has_state, "G.coupling_fac{%d} missing", mi.coupling + 1);
    }
    ensure_mode_work(mi);
    if (!mi.slabs) compute_gram(mi);                                         // :62-81
  }
  for (int p = 0; p < n_tensors_; ++p) {
    TensorInfo& t = tensors_[p];
    if (t.par2) {
      for (int k = 0; k < t.p2.K; ++k)
        AO_REQUIRE(t.p2.have_P[k] && t.p2.have_mu[k], "G.P{%d}{%d} / G.mu_DeltaB{%d}{%d} missing", p + 1, k + 1, p + 1, k + 1);
    }
    // a weighted block starts every solve from Xhat = W o X0 (M_old = 0), whatever an earlier solve imputed
    if (!t.par2 && t.blk.has_weights) block_reset_weighted(block_ctx(), t.blk);
    (void)tensor_normsq(p);          // Znorm_const{p}; a masked block needs the factors (statistics-only EM pass)
    if (t.observed_only()) {         // a solve starts with the missing entries at 0: no snapshot of an earlier one
      const CpBlock& b = t.blk;
      AO_REQUIRE(!b.coo.sharded && b.coo.nnz > 0 && b.sem.nnz == b.coo.nnz, "tensor %d: observed-only needs a replicated sparse block with stored entries", p);
      AO_REQUIRE(b.sem.R == modes_[t.modes[0]].R, "tensor %d was marked observed-only for rank %d", p, b.sem.R);
      sem_reset(t.blk.sem, b.coo, stream_);
    }
  }
  for (int p = 0; p < n_tensors_; ++p) {
    TensorInfo& t = tensors_[p];
    if (!t.par2) continue;
    Par2Block& b = t.p2;
    AO_REQUIRE(b.has_DeltaB, "G.DeltaB{%d} missing", p + 1);
    par2_ensure_work(t);
    decide_slab_sharding(t, opt);
    par2_gram(modes_[t.modes[1]].fac.d(), b.dims(), b.GB.d(), stream_);      // :71-73
    t.last_pos = 2;
  }
  // per PARAFAC2 block: K + 1 slab residuals (+ the not-PD flag of sharded slabs), 4 K gap sums, K regulariser values --
  // read back with everything else behind ONE event (three more copies into pageable memory with a stream
  // synchronisation each left the GPU idle for ~60 us per outer iteration of config 4).  par2_ensure_work calls
  // ensure() on them: had it outgrown a view, the block would keep its sums in a buffer of its own.
  for (int p = 0; p < n_tensors_; ++p) {
    if (!tensors_[p].par2) continue;
    const Par2Block& b = tensors_[p].p2;
    AO_REQUIRE(b.res.d() == dev_.p2_res(p) && b.q.d() == dev_.p2_q(p) && b.regv.d() == dev_.p2_regv(p),
               "read-back arena: PARAFAC2 block %d keeps its sums elsewhere", p);
  }
  if (best_.on) {                                     // after decide_slab_sharding: a rank keeps its own slabs
    best_build_table();
    best_.use_dimtree = opt.use_dimtree != 0;
  }
}

// slabs over the ranks or every slab on every rank (aoadmm_options.par2_slab_sharding)
void Engine::decide_slab_sharding(TensorInfo& t, const aoadmm_options& opt) {
  Par2Block& b = t.p2;
  const ModeInfo& mB = modes_[t.modes[1]];
  // (a held-out list is scored inside the solve from this rank's B_k: the block is repeated then)
  const bool can = sharded() && world_ > 1 && !b.has_mask && !b.sparse && t.ho.n == 0 && !(mB.constrained && mB.prox.type == AOADMM_C_TPARAFAC2) &&
                   modes_[t.modes[2]].coupling < 0;     // a coupled C mode needs every row system on every rank
  const bool want = opt.par2_slab_sharding > 0 || (opt.par2_slab_sharding == 0 && b.K / world_ >= 1024);
  const int per = (int)cdiv(b.K, world_);
  // every rank must own a slab, and every rank must reach the same verdict: otherwise repeat the block
  b.slab_sharded = can && want && (int64_t)per * (world_ - 1) < b.K;
  b.k0 = std::min(b.K, per * rank_);
  b.k1 = std::min(b.K, b.k0 + per);
}

// one mode's turn inside the schedule of outer_updates
void Engine::update_mode(int m, int cid, const aoadmm_options& opt, int iter) {
  const bool par2 = tensors_[modes_[m].tensor].par2;
  if (par2 && modes_[m].pos == 1) par2_update_B(m, opt, iter);             // :191-218
  else if (par2 && modes_[m].pos == 2 && cid < 0) par2_update_C(m, opt);   // :219-248
  else if (par2 && modes_[m].pos == 2) par2_prepare_C_coupled(m, couplings_[cid].type, opt);
  else if (cid < 0) update_uncoupled_cp_mode(m, opt);
  else prepare_mode_system(m, coupled_nrho(m), opt);
}

// What the imputing EM pass of an iteration fuses.  The test hook (read per call) asks for the second mode, so that the
// strip's walk along mode 2 with the fused contraction is exercised by models whose update order would never pick it.
static int em_fuse_choice(bool next_pass_follows) {
  if (!next_pass_follows) return kEmFuseNone;
  return getenv("AOADMM_EM_FUSE_SECOND_MODE") != nullptr ? kEmFuseSecond : kEmFuseAuto;
}

// One outer iteration's updates: every mode in the schedule of :89-93, the coupled ADMM loops, then the EM passes.
void Engine::outer_updates(const aoadmm_options& opt, int iter, bool has_miss) {
  for (ModeInfo& mq : modes_) mq.quad.dirty = true;   // rho moves once per outer iteration ('quadratic regularization', non-symmetric L)
  if (iter == 3)                                      // by now every pass of the schedule has run once: all copies exist
    for (int p = 0; p < n_tensors_; ++p)
      if (!tensors_[p].par2) maybe_release_natural(block_ctx(), tensors_[p].blk, tensors_[p].normsq_valid);
  for (int cid = -1; cid < n_couplings_; ++cid) {                            // :89 (0 = uncoupled first)
    std::vector<int> cm;
    for (int m = 0; m < n_modes_; ++m)
      if (modes_[m].coupling == cid) cm.push_back(m);
    if (cm.empty()) continue;
    std::set<int> ps;
    for (int m : cm) ps.insert(modes_[m].tensor);
    for (int p : ps)                                                         // :91
      for (int m : cm)                                                       // :93
        if (modes_[m].tensor == p) update_mode(m, cid, opt, iter);
    if (cid >= 0) {
      coupled_admm(cid, opt);                                                // :277 / :366
      for (int m : cm) { modes_[m].version++; compute_gram(modes_[m]); }      // :393-403
    }
  }
  if (has_miss)                                                              // EM imputation (:408-441)
    for (int p = 0; p < n_tensors_; ++p) {
      if (tensors_[p].masked()) em_pass_enqueue(p, 1, em_fuse_choice(opt.use_dimtree != 0 && iter < opt.MaxOuterIters));
      else if (tensors_[p].observed_only()) sparse_em_enqueue(p, false);
    }
}

void Engine::enqueue_readback(SolveRun& r) {
  AO_HIP(hipMemcpyAsync(r.pin.p, readback_.p, readback_.bytes, hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipEventRecord(r.pin.ev, stream_));
}

// The objective of iteration `iter` and its read-back, with whatever of the next iteration can hide the host's wait.
void Engine::enqueue_objective(SolveRun& r, int iter) {
  const aoadmm_options& opt = r.opt;
  if (iter >= opt.MaxOuterIters) {
    eval_objective_enqueue(false);                                           // :447
    enqueue_readback(r);
    return;
  }
  // The objective needs nothing the first tensor pass of the next iteration writes (frag, T), and that pass does
  // not depend on the stopping decision: the pass goes onto the main stream, the objective kernels and their
  // read-back onto the side stream behind an event, and the main stream takes up its small kernels again only
  // when the objective is through (they overwrite what it reads).  ~50 us per iteration off the critical path.
  // (Only when a pass is actually launched: the cross-stream wait alone costs ~40 us.)
  AO_HIP(hipEventRecord(side_ev_, stream_));
  if (prefetch_next_contraction(opt)) {
    AO_HIP(hipStreamWaitEvent(side_, side_ev_, 0));
    std::swap(stream_, side_);
    try {
      eval_objective_enqueue(false);                                         // :447
      enqueue_readback(r);
    } catch (...) { std::swap(stream_, side_); throw; }
    std::swap(stream_, side_);
    AO_HIP(hipStreamWaitEvent(stream_, r.pin.ev, 0));
  } else {
    eval_objective_enqueue(false);                                           // :447
    enqueue_readback(r);
    // No pass to hide behind: the host now waits ~45 us for the read-back before it can enqueue anything, and the
    // GPU would sit idle.  The MTTKRP (reductions over the cached T) and the system build of the next iteration's
    // first mode depend on no stopping decision and write only that mode's scratch (A, C, rho, B, L, inv, ctl --
    // behind the read-back of this iteration's loop counters in stream order): enqueue them now.
    if (!r.has_miss) prepare_next_first_mode(opt);
  }
}

// host half of an evaluation: wait for the read-back, then the not-PD flags and f[4] from its pinned copy
void Engine::finish_objective(SolveRun& r) {
  AO_HIP(hipEventSynchronize(r.pin.ev));
  check_not_pd(r.host);
  objective_from_host(r.host, r.f);
}

// iteration `iter` (0: the starting point) into the result arrays
void Engine::record_iteration(SolveRun& r, int iter) {
  aoadmm_result* out = r.out;
  if (out->func_val_conv) out->func_val_conv[iter] = r.f[0];
  if (out->func_coupl_conv) out->func_coupl_conv[iter] = r.f[1];
  if (out->func_constr_conv) out->func_constr_conv[iter] = r.f[2];
  if (out->func_PAR2_coupl) out->func_PAR2_coupl[iter] = r.f[3];
  if (out->time_at_it)
    out->time_at_it[iter] = iter == 0 ? 0.0 : std::chrono::duration<double>(std::chrono::steady_clock::now() - r.t0).count();
  if (out->func_rel_missing && (iter == 0 || r.has_miss)) out->func_rel_missing[iter] = r.f_rel_missing;
  if (r.has_ho) {                                    // the held-out sums came in the same read-back
    double H = 0.0;
    for (int p = 0; p < n_tensors_; ++p) {
      TensorInfo& t = tensors_[p];
      if (t.ho.n == 0) continue;
      const double v = r.host.heldout(p)[kHoRes];
      t.ho_trace.push_back(v);
      H += t.weight * v;
    }
    if (iter == 0 || H < r.ho_best) {
      r.ho_best = H; ho_best_iter_ = iter; r.ho_bad = 0;
      // The device still holds the state of iteration `iter`: what was enqueued ahead of this read-back (the prefetched
      // tensor pass, prepare_next_first_mode) writes scratch only, and the next iteration's updates follow the copy in
      // stream order.
      if (best_.on && !r.rk_select) best_snapshot(iter);
    } else {
      ++r.ho_bad;
    }
  }
  if (r.has_rl && iter % track_.every == 0) {        // the ranking sums came in the same read-back (other iterations: stale slots)
    for (int p = 0; p < n_tensors_; ++p) {
      TensorInfo& t = tensors_[p];
      if (t.rl.nq == 0) continue;
      const double* v = r.host.rank(p);
      t.rl_trace.insert(t.rl_trace.end(), v, v + kRankSlots);
    }
    rank_iters_.push_back(iter);
    const double S = rank_score(r.host);
    // larger is better and the comparison is strict; a NaN never becomes the best, a NaN best yields to the first number
    if (iter == 0 || S > r.rk_best || (std::isnan(r.rk_best) && !std::isnan(S))) {
      r.rk_best = S; rank_best_iter_ = iter; r.rk_bad = 0;
      if (best_.on && r.rk_select) best_snapshot(iter);     // the same place and the same reason as above
    } else {
      ++r.rk_bad;
    }
  }
  if (iter == 0 || !out->innerIters) return;
  for (int m = 0; m < n_modes_; ++m) {
    const ModeInfo& mi = modes_[m];
    double v;
    if (mi.coupling >= 0) v = r.host.ctl(n_modes_ + mi.coupling)->iters;     // :392
    else if (mi.slabs) v = r.host.ctl(m)->iters;                             // :215
    else if (mi.constrained) v = r.host.ctl(m)->iters;                       // :146
    else v = 1;                                                              // :138
    out->innerIters[(int64_t)(iter - 1) * n_modes_ + m] = v;
  }
}

void Engine::solve(const aoadmm_options& opt, aoadmm_result* out) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(out != nullptr, "null result");
  AO_REQUIRE(opt.MaxOuterIters >= 0 && opt.MaxInnerIters >= 1, "bad iteration limits");
  const bool has_ho = has_heldout();
  AO_REQUIRE(opt.heldout_patience >= 0, "heldout_patience = %d < 0", opt.heldout_patience);
  AO_REQUIRE(opt.heldout_patience == 0 || has_ho, "heldout_patience = %d needs a held-out list (aoadmm_tensor_set_heldout)", opt.heldout_patience);
  const bool has_rl = has_ranklist();
  const bool rk_select = track_.criterion == 1;
  AO_REQUIRE(!rk_select || has_rl, "aoadmm_rank_track criterion = 1 needs a ranking list (aoadmm_tensor_set_ranklist)");
  AO_REQUIRE(!rk_select || opt.heldout_patience == 0, "aoadmm_rank_track criterion = 1 and heldout_patience = %d: one rule selects the model", opt.heldout_patience);
  AO_REQUIRE(!best_.on || (rk_select ? has_rl : has_ho), "aoadmm_heldout_keep_best needs a held-out list (aoadmm_tensor_set_heldout)");
  AO_HIP(hipSetDevice(device_));
  ho_best_iter_ = -1;
  rank_best_iter_ = -1;
  rank_iters_.clear();
  best_.iter = -1;
  for (TensorInfo& t : tensors_) { t.ho_trace.clear(); t.rl_trace.clear(); }
  struct EvalFlag {                                   // rank_eval_now_ does not outlive the solve, however it ends
    bool& f;
    ~EvalFlag() { f = false; }
  } eval_flag{rank_eval_now_};
  solve_setup(opt);
  SolveRun r{opt, out};
  r.has_miss = has_missing();
  r.has_ho = has_ho;
  r.has_rl = has_rl;
  r.rk_select = rk_select;
  r.pin.alloc(readback_.bytes);
  r.host = arena_.at(r.pin.p);

  rank_eval_now_ = has_rl;                                                     // iteration 0 is always evaluated
  eval_objective_enqueue(true);                                                // :32
  enqueue_readback(r);
  finish_objective(r);
  r.f_rel_missing = std::nan("");                                              // :30
  record_iteration(r, 0);
  const bool report = progress_fn_ != nullptr && progress_every_ > 0;
  if (report) progress_fn_(progress_user_, 0, r.f, r.f_rel_missing);           // :53-59
  r.t0 = std::chrono::steady_clock::now();

  const double* f = r.f;
  double fo[4];
  int iter = 1;
  bool stop = false, ho_stop = false, rk_stop = false;
  while (iter <= opt.MaxOuterIters && !stop && !ho_stop && !rk_stop) {         // :87
    outer_updates(opt, iter, r.has_miss);
    for (int i = 0; i < 4; ++i) fo[i] = f[i];
    rank_eval_now_ = has_rl && iter % track_.every == 0;
    enqueue_objective(r, iter);
    finish_objective(r);
    if (r.has_miss) r.f_rel_missing = rel_missing_from_host(r.host);           // :436-440
    record_iteration(r, iter);
    stop = stop_one(f[0], fo[0], opt) && stop_one(f[1], fo[1], opt) && stop_one(f[2], fo[2], opt) &&
           stop_one(f[3], fo[3], opt);                                         // :456
    if (r.has_miss) stop = stop && (r.f_rel_missing < opt.OuterRelTol);        // :457-459
    ho_stop = opt.heldout_patience > 0 && r.ho_bad >= opt.heldout_patience;    // held-out early stopping (heldout.h)
    rk_stop = rk_select && track_.patience > 0 && r.rk_bad >= track_.patience;   // counts evaluations (rank_metrics.h)
    if (report && iter % progress_every_ == 0) progress_fn_(progress_user_, iter, r.f, r.f_rel_missing);   // :462-468
    ++iter;
  }
  out->f_tensors = f[0]; out->f_couplings = f[1]; out->f_constraints = f[2]; out->f_PAR2_couplings = f[3];
  out->f_rel_missing = r.f_rel_missing;
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].par2) par2_gather_slabs(tensors_[p]);
  AO_HIP(hipStreamSynchronize(stream_));
  if (best_.on) best_.iter = rk_select ? rank_best_iter_ : ho_best_iter_;   // the solve came through: the kept copy may be restored
  out->OuterIterations = iter - 1;
  out->exit_code = iter > opt.MaxOuterIters ? 0 : stop ? 1 : ho_stop ? 2 : 3;  // make_exit_flag.m:4-5; 2: heldout_patience, 3: rank patience
  for (int i = 0; i < 4; ++i) out->exit_abs[i] = f[i] < opt.AbsFuncTol ? 1 : 0;
}
}  // namespace aoadmm
