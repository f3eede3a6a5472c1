// Engine: PARAFAC2 block updates (functions/cmtf_fun_AOADMM.m:157-250, :509-589) on the device.
#include <algorithm>
#include <cstring>

#include "solver.h"

namespace aoadmm {

void Engine::add_par2(int p, const int* modes3, double weight) {
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  t.defined = true; t.par2 = true; t.nmodes = 3; t.weight = weight;
  for (int i = 0; i < 3; ++i) {
    check_mode(modes3[i]);
    ModeInfo& mi = modes_[modes3[i]];
    AO_REQUIRE(mi.defined, "mode %d undefined", modes3[i]);
    AO_REQUIRE(mi.tensor < 0, "mode %d already belongs to tensor %d", modes3[i], mi.tensor);
    AO_REQUIRE(mi.slabs == (i == 1), "PARAFAC2: only the second mode is slab-valued (mode %d)", modes3[i]);
    t.modes[i] = modes3[i];
    mi.tensor = p;
    mi.pos = i;
  }
  const ModeInfo& mA = modes_[modes3[0]];
  const ModeInfo& mB = modes_[modes3[1]];
  const ModeInfo& mC = modes_[modes3[2]];
  // check_data_input.m:22-26: size of mode C must equal the number of slabs
  AO_REQUIRE(mC.rows == mB.K, "size mismatch in PARAFAC2 model betwwen mode C and Bk");
  AO_REQUIRE(mA.R == mB.R && mA.R == mC.R, "modes of tensor %d disagree on the rank", p);
  Par2Block& b = t.p2;
  b.K = mB.K; b.I = (int)mA.rows; b.R = mA.R;
  b.off_h = mB.off_k;
  b.Jtot = mB.rows;
  b.Jmax = 0;
  for (int k = 0; k < b.K; ++k) {
    // cmtf_AOADMM.m:55-65
    AO_REQUIRE(mB.rows_k[k] >= b.R, "Number of components for PARAFAC2 is larger than size of slice %d of data tensor %d.", k + 1, p + 1);
    b.Jmax = std::max<int>(b.Jmax, (int)mB.rows_k[k]);
  }
  b.off_d.alloc((size_t)(b.K + 1) * sizeof(int64_t));
  AO_HIP(hipMemcpyAsync(b.off_d.p, b.off_h.data(), (size_t)(b.K + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  // b.X (I x sum J_k doubles) is allocated by the first dense upload: a block with sparse slabs never has one
  b.have_slab.assign(b.K, 0);
  b.have_P.assign(b.K, 0);
  b.have_mu.assign(b.K, 0);
}

void Engine::par2_slab_upload(int p, int k, const double* Xk) {
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_ && tensors_[p].par2, "tensor %d is not a PARAFAC2 block", p);
  AO_REQUIRE(Xk != nullptr, "null slab");
  AO_HIP(hipSetDevice(device_));
  Par2Block& b = tensors_[p].p2;
  AO_REQUIRE(k == AOADMM_ALL_SLABS || (k >= 0 && k < b.K), "slab %d out of range", k);
  const bool all = k == AOADMM_ALL_SLABS;                  // I x sum(J_k): the slabs back to back
  AO_REQUIRE(all || !b.sparse, "tensor %d holds sparse slabs: one dense slab cannot replace part of them (upload all slabs)", p);
  b.X.ensure((size_t)b.I * b.Jtot * sizeof(double));
  if (b.sparse) {                                          // a dense upload of every slab replaces the sparse form
    b.sp.clear();
    b.sparse = false;
  }
  const int64_t o = all ? 0 : b.off_h[k];
  const int64_t Jk = all ? b.Jtot : b.off_h[k + 1] - b.off_h[k];
  AO_HIP(hipMemcpyAsync(b.X.d() + (int64_t)b.I * o, Xk, (size_t)b.I * Jk * sizeof(double), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  if (all) b.have_slab.assign(b.K, 1); else b.have_slab[k] = 1;
  tensors_[p].blk.has_data = std::all_of(b.have_slab.begin(), b.have_slab.end(), [](char c) { return c != 0; });
  tensors_[p].normsq_valid = false;
}

void Engine::par2_slab_mask_upload(int p, int k, const uint8_t* mask) {
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_ && tensors_[p].par2, "tensor %d is not a PARAFAC2 block", p);
  AO_REQUIRE(mask != nullptr, "null mask");
  AO_HIP(hipSetDevice(device_));
  Par2Block& b = tensors_[p].p2;
  AO_REQUIRE(!b.sparse, "Missing data (Z.miss) not supported for sparse PARAFAC2 slabs. Convert to full slabs first. (Z.object{%d})", p + 1);
  AO_REQUIRE(k == AOADMM_ALL_SLABS || (k >= 0 && k < b.K), "slab %d out of range", k);
  if (!b.has_mask) {
    b.mask.alloc((size_t)b.I * b.Jtot);
    AO_HIP(hipMemsetAsync(b.mask.p, 1, (size_t)b.I * b.Jtot, stream_));     // slabs without a mask: fully observed
    b.has_mask = true;
  }
  const int64_t o = k == AOADMM_ALL_SLABS ? 0 : b.off_h[k];
  const int64_t Jk = k == AOADMM_ALL_SLABS ? b.Jtot : b.off_h[k + 1] - b.off_h[k];
  AO_HIP(hipMemcpyAsync(b.mask.as<uint8_t>() + (int64_t)b.I * o, mask, (size_t)b.I * Jk, hipMemcpyHostToDevice, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  tensors_[p].normsq_valid = false;
}

// Z.object{p}{k} as sparse matrices (par2_sparse.h): all slabs in one call; drops the dense slabs and their mask.
void Engine::par2_slab_upload_coo(int p, int64_t nnz, const int64_t* subs, const double* vals) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_ && tensors_[p].par2, "tensor %d is not a PARAFAC2 block", p);
  AO_HIP(hipSetDevice(device_));
  Par2Block& b = tensors_[p].p2;
  Par2Sparse sp;
  par2s_build(sp, b.dims_all(), nnz, subs, vals, stream_);        // validates before anything of the old form is dropped
  b.X.release(); b.mask.release(); b.T1.release();
  b.has_mask = false;
  b.sp = std::move(sp);
  b.sparse = true;
  b.have_slab.assign(b.K, 1);
  tensors_[p].blk.has_data = true;
  tensors_[p].normsq_valid = false;
}

void Engine::par2s_pass(Par2Block& b, int pos, const CooFactor& f, double* out, int64_t ldOut) {
  KernelStats& ks = timers_.stats[3];
  const LaunchTimers::Pair pr = timers_.begin(ks, timers_.profile, stream_);
  coo_mttkrp(b.sp.coo, pos, &f, b.R, 1.0, out, ldOut, stream_);
  timers_.end(ks, pr, stream_, coo_mttkrp_bytes(b.sp.coo, pos, b.R), coo_mttkrp_flops(b.sp.coo, b.R));
}

void Engine::par2s_rhs_A(TensorInfo& t, double* out) {
  Par2Block& b = t.p2;
  const P2Dims d = b.dims_all();
  b.sp.BC.ensure((size_t)b.Jtot * b.R * sizeof(double));
  par2s_scale_b(modes_[t.modes[1]].fac.d(), modes_[t.modes[2]].fac.d(), d, b.sp.kofg.as<int>(), b.sp.BC.d(), stream_);
  par2s_pass(b, 0, CooFactor{b.sp.BC.d(), (int64_t)b.R, 1}, out, b.I);
}

void Engine::par2s_ensure_Y(TensorInfo& t) {
  Par2Block& b = t.p2;
  const ModeInfo& mA = modes_[t.modes[0]];
  if (b.sp.y_valid && b.sp.y_version == mA.version) return;
  b.sp.Y.ensure((size_t)b.Jtot * b.R * sizeof(double));
  b.sp.s.ensure((size_t)b.K * b.R * sizeof(double));
  const CooFactor f = mA.facT_version == mA.version ? CooFactor{mA.facT.d(), (int64_t)b.R, 1}
                                                    : CooFactor{mA.fac.d(), 1, mA.rows};
  par2s_pass(b, 1, f, b.sp.Y.d(), b.Jtot);
  b.sp.y_valid = true;
  b.sp.y_version = mA.version;
}

// The unweighted right-hand side of one tensor mode of a block with sparse slabs against the current factors
// (operator-level tests and timing): 0: I x R, 1: Jtot x R in the slab layout, 2: K x R.
void Engine::resident_par2_rhs(int p, int pos, double* out_host, float* ms) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_ && tensors_[p].par2, "tensor %d is not a PARAFAC2 block", p);
  AO_REQUIRE(pos >= 0 && pos < 3, "tensor mode %d out of range", pos);
  AO_HIP(hipSetDevice(device_));
  TensorInfo& t = tensors_[p];
  Par2Block& b = t.p2;
  AO_REQUIRE(b.sparse, "tensor %d does not hold sparse slabs (aoadmm_par2_slab_upload_coo)", p);
  for (int i = 0; i < 3; ++i) AO_REQUIRE(modes_[t.modes[i]].has_fac, "G.fac{%d} missing", t.modes[i] + 1);
  ModeInfo& mA = modes_[t.modes[0]];
  ModeInfo& mB = modes_[t.modes[1]];
  ModeInfo& mC = modes_[t.modes[2]];
  ensure_mode_work(mA);
  b.Ak.ensure((size_t)b.Jtot * b.R * sizeof(double));
  const P2Dims d = b.dims_all();
  // events from the engine's pool, handed back on every path (the timing tool calls this in a loop)
  struct Pair {
    std::vector<hipEvent_t>& pool;
    hipEvent_t e0, e1;
    ~Pair() { pool.push_back(e0); pool.push_back(e1); }
  };
  hipEvent_t ev0 = timers_.take_event();
  hipEvent_t ev1 = nullptr;
  try { ev1 = timers_.take_event(); } catch (...) { timers_.pool.push_back(ev0); throw; }
  Pair ev{timers_.pool, ev0, ev1};
  AO_HIP(hipEventRecord(ev.e0, stream_));
  const double* res = nullptr;
  int64_t n = 0;
  if (pos == 0) {
    par2s_rhs_A(t, mA.tmp.d());
    res = mA.tmp.d(); n = (int64_t)b.I * b.R;
  } else {
    b.sp.y_valid = false;                               // a full evaluation: the pass over the nonzeros included
    par2s_ensure_Y(t);
    if (pos == 1) {
      par2s_ak(b.sp.Y.d(), mC.fac.d(), 1.0, d, b.sp.kofg.as<int>(), b.Ak.d(), stream_);
      res = b.Ak.d(); n = b.Jtot * b.R;
    } else {
      par2s_slab_sums(mB.fac.d(), b.sp.Y.d(), d, b.sp.s.d(), nullptr, nullptr, nullptr, nullptr, nullptr, stream_);
      res = b.sp.s.d(); n = (int64_t)b.K * b.R;
    }
  }
  AO_HIP(hipEventRecord(ev.e1, stream_));
  AO_HIP(hipEventSynchronize(ev.e1));
  float tms = 0.f;
  AO_HIP(hipEventElapsedTime(&tms, ev.e0, ev.e1));
  if (ms) *ms = tms;
  if (out_host) {
    AO_HIP(hipMemcpyAsync(out_host, res, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
    AO_HIP(hipStreamSynchronize(stream_));
  }
}

void Engine::par2_ensure_work(TensorInfo& t) {
  Par2Block& b = t.p2;
  const size_t RR = (size_t)b.R * b.R * sizeof(double);
  const size_t cat = (size_t)b.Jtot * b.R * sizeof(double);
  b.DeltaBold.ensure(RR); b.Pold.ensure(cat); b.W.ensure(cat); b.Ak.ensure(cat);
  if (!b.sparse) b.T1.ensure((size_t)b.K * b.I * b.R * sizeof(double));     // X_k B_k: sparse slabs never form it
  b.GB.ensure((size_t)b.K * RR); b.Lk.ensure((size_t)b.K * RR); b.Lc.ensure((size_t)b.K * RR);
  b.rhok.ensure((size_t)b.K * 8); b.rhoc.ensure((size_t)b.K * 8); b.rhomax.ensure(64);
  b.part.ensure((size_t)b.K * RR); b.norms.ensure((size_t)b.K * 8 * 8);
  b.res.ensure((size_t)(b.K + 1) * 8); b.q.ensure((size_t)b.K * 4 * 8); b.regv.ensure((size_t)b.K * 8);
  b.Csys.ensure(RR); b.ac.ensure((size_t)b.K * b.R * 8);
  b.psum.ensure(RR + 128);                       // R*R+1 sums of DeltaB, then (at R*R+8) four residual means
  ModeInfo& mB = modes_[t.modes[1]];
  const size_t nB = (size_t)mB.rows * mB.R * sizeof(double);
  mB.Zold.ensure(nB); mB.V.ensure(nB);
  size_t pw = 16;
  if (mB.constrained) pw = prox_ws_bytes(mB.prox.type, b.Jmax, b.R);
  mB.proxws.ensure(pw);
}

// mode A: MTTKRP and Hadamard analogue from the slabs (:160-178), then the common system build
void Engine::par2_prepare_modeA(int m, int nrho, const aoadmm_options& opt) {
  ModeInfo& mi = modes_[m];
  TensorInfo& t = tensors_[mi.tensor];
  Par2Block& b = t.p2;
  const P2Dims d = b.dims();
  ModeInfo& mB = modes_[t.modes[1]];
  ModeInfo& mC = modes_[t.modes[2]];
  if (b.sparse) {                                     // one pass over the row-sorted nonzeros; Csys needs no data
    par2s_rhs_A(t, mi.tmp.d());
    par2_modeA_csys(mC.fac.d(), b.GB.d(), d, b.Csys.d(), stream_);
  } else {
    par2_mode_a(b.X.d(), mB.fac.d(), mC.fac.d(), b.GB.d(), d, b.T1.d(), mi.tmp.d(), b.Csys.d(), stream_);
  }
  if (b.slab_sharded) {                               // sums over this rank's slabs -> sums over all slabs
    allreduce(mi.tmp.d(), mi.rows * mi.R);
    allreduce(b.Csys.d(), (int64_t)b.R * b.R);
  }
  {
    Coef c[1] = {coef(t.weight)};                     // A{m} = w*A{m}  (:169); last_mttkrp = A/w
    const double* x[1] = {mi.tmp.d()};
    ew_lincomb(mi.A.d(), mi.rows * mi.R, 1, c, x, nullptr, stream_);
  }
  SysBuild sb;
  sb.ngram = 0;
  sb.Cpre = b.Csys.d();
  sb.w = t.weight;
  sb.ridge = has_ridge_ ? mi.ridge : 0.0;
  sb.bsum_half = opt.bsum ? opt.bsum_weight / 2 : 0.0;
  sb.rho_scale = 1.0;
  sb.nrho = nrho;
  sb.R = mi.R;
  sb.C = mi.C.d(); sb.rho = mi.rho.d(); sb.Bsys = mi.Bsys.d(); sb.L = mi.L.d();
  sb.Binv = nrho > 0 ? mi.Binv.d() : nullptr;
  sb.ctl = ctl_of_mode(m);
  sys_build(sb, stream_);
  t.last_pos = 0;                                     // last_m(p) = 1  (:168)
  mi.Aeff = mi.A.d();
  if (opt.bsum) {
    Coef c[2] = {coef(1.0), coef(opt.bsum_weight / 2)};
    const double* x[2] = {mi.A.d(), mi.fac.d()};
    ew_lincomb(mi.Ab.d(), mi.rows * mi.R, 2, c, x, nullptr, stream_);
    mi.Aeff = mi.Ab.d();
  }
}

// mode B (:191-218) + ADMM_B_Parafac2 (:509-589)
void Engine::par2_update_B(int m, const aoadmm_options& opt, int iter) {
  ModeInfo& mi = modes_[m];
  TensorInfo& t = tensors_[mi.tensor];
  Par2Block& b = t.p2;
  const P2Dims d = b.dims();
  ModeInfo& mA = modes_[t.modes[0]];
  ModeInfo& mC = modes_[t.modes[2]];
  AdmmCtl* ctl = ctl_of_mode(m);
  const bool constr = mi.constrained && iter >= opt.iter_start_PAR2Bkconstraint;        // :209, :527
  if (b.sparse) {                                     // Y = Xcat' A: a pass over the column-sorted nonzeros if A moved
    par2s_ensure_Y(t);
    par2s_ak(b.sp.Y.d(), mC.fac.d(), t.weight, d, b.sp.kofg.as<int>(), b.Ak.d(), stream_);
  } else {
    par2_xta(b.X.d(), mA.fac.d(), mC.fac.d(), t.weight, d, b.Ak.d(), stream_);
  }
  t.last_pos = 1;                                                                        // last_m(p) = 2
  P2BLoop g;
  g.GA = mA.gram.d(); g.Cfac = mC.fac.d();
  g.w = t.weight; g.ridge = has_ridge_ ? mi.ridge : 0.0;
  g.bsum = opt.bsum != 0; g.bsum_half = opt.bsum ? opt.bsum_weight / 2 : 0.0;
  g.rho_scale = opt.has_increase_factor_rhoBk ? opt.increase_factor_rhoBk : 1.0;
  g.Ak = b.Ak.d(); g.rho = b.rhok.d(); g.L = b.Lk.d();
  g.a.B = mi.fac.d(); g.a.P = b.P.d(); g.a.Pold = b.Pold.d(); g.a.mu = b.muDB.d(); g.a.W = b.W.d();
  g.a.DeltaB = b.DeltaB.d(); g.a.DeltaBold = b.DeltaBold.d(); g.a.part = b.part.d();
  g.a.norms = b.norms.d();
  b.Jrot.ensure((size_t)b.K * b.R * b.R * sizeof(double));
  g.a.Jrot = b.Jrot.d();
  g.constrained = constr;
  g.prox = mi.prox;
  g.Z = mi.Z.d(); g.muZ = mi.mu.d(); g.Zold = mi.Zold.d(); g.V = mi.V.d(); g.prox_ws = mi.proxws.d();
  g.max_inner = opt.MaxInnerIters;
  g.tol_pr_coupl = opt.innerRelPrTol_coupl; g.tol_pr_constr = opt.innerRelPrTol_constr;
  g.tol_du_coupl = opt.innerRelDualTol_coupl; g.tol_du_constr = opt.innerRelDualTol_constr;
  g.GB = b.GB.d();
  g.psum = b.slab_sharded ? b.psum.d() : nullptr;
  g.part4 = b.slab_sharded ? b.psum.d() + (int64_t)b.R * b.R + 8 : nullptr;
  g.allreduce = [this](double* buf, int64_t n) { allreduce(buf, n); };
  par2_b_loop(g, d, ctl, stream_);                    // systems, ADMM_B_Parafac2, Gram matrices of the new B_k (:194-218)
  mi.version++;
}

// mode C, uncoupled (:219-248; constrained rows through ADMM_constrained_only :602-606)
void Engine::par2_update_C(int m, const aoadmm_options& opt) {
  ModeInfo& mi = modes_[m];
  TensorInfo& t = tensors_[mi.tensor];
  Par2Block& b = t.p2;
  const P2Dims d = b.dims();
  ModeInfo& mA = modes_[t.modes[0]];
  ModeInfo& mB = modes_[t.modes[1]];
  AdmmCtl* ctl = ctl_of_mode(m);
  const size_t RR = (size_t)b.R * b.R;
  if (b.slab_sharded) {                               // rows of the other ranks arrive through the all-reduce
    AO_HIP(hipMemsetAsync(b.ac.p, 0, (size_t)b.K * b.R * 8, stream_));
    AO_HIP(hipMemsetAsync(b.rhoc.p, 0, (size_t)b.K * 8, stream_));
    AO_HIP(hipMemsetAsync(b.Lc.p, 0, (size_t)b.K * RR * 8, stream_));
  }
  if (b.sparse) {                                     // diag(A' X_k B_k) from Y: no pass while A has not moved
    par2s_ensure_Y(t);
    par2s_slab_sums(mB.fac.d(), b.sp.Y.d(), d, b.sp.s.d(), nullptr, nullptr, nullptr, nullptr, nullptr, stream_);
    par2_c_system_pre(b.sp.s.d(), mA.gram.d(), b.GB.d(), t.weight, has_ridge_ ? mi.ridge : 0.0,
                      opt.bsum ? opt.bsum_weight / 2 : 0.0, mi.constrained ? 1 : 0, 0, d, mi.fac.d(), b.ac.d(),
                      b.rhoc.d(), b.Lc.d(), ctl, stream_);
  } else {
    P2CSys cs;
    cs.X = b.X.d(); cs.A = mA.fac.d(); cs.B = mB.fac.d(); cs.GA = mA.gram.d(); cs.GB = b.GB.d(); cs.Cfac = mi.fac.d();
    cs.w = t.weight; cs.ridge = has_ridge_ ? mi.ridge : 0.0; cs.bsum_half = opt.bsum ? opt.bsum_weight / 2 : 0.0;
    cs.nrho = mi.constrained ? 1 : 0; cs.raw = 0;
    cs.T1 = b.T1.d(); cs.a = b.ac.d(); cs.rho = b.rhoc.d(); cs.L = b.Lc.d();
    par2_c_systems(cs, d, ctl, stream_);
  }
  if (b.slab_sharded) {
    allreduce(b.ac.d(), (int64_t)b.K * b.R);
    allreduce(b.rhoc.d(), b.K);
    allreduce(b.Lc.d(), (int64_t)b.K * RR);
  }
  t.last_pos = 2;                                                                        // last_m(p) = 3
  P2CSolve g;                                         // the K x R row systems are solved on every rank
  g.a = b.ac.d(); g.rho = b.rhoc.d(); g.L = b.Lc.d();
  g.fac = mi.fac.d(); g.Z = mi.Z.d(); g.mu = mi.mu.d();
  g.constrained = mi.constrained; g.prox = mi.prox;
  g.max_inner = opt.MaxInnerIters; g.tol_pr = opt.innerRelPrTol_constr; g.tol_du = opt.innerRelDualTol_constr;
  g.rhomax = b.rhomax.d();
  g.Zold = mi.Zold.d(); g.V = mi.V.d(); g.prox_ws = mi.proxws.d(); g.slots = resid_slots(m); g.red_ws = redws_.d();
  par2_c_solve(g, b.dims_all(), ctl, stream_);        // single solve, one-workgroup loop or launched loop (par2_c_path)
  mi.version++;
}

// mode C inside a coupling (:253-385): right-hand sides a_k, rho_k and the systems the coupled ADMM needs --
// types 0, 3, 4: per-row Cholesky factors of w*C_k + rho_k/2*I (+ rho_k/2*I if constrained) (:260-267, :327-334, :349-356);
// type 2: the same with rho_k/2*H*H' for the coupling term (:305-312);
// types 1, 5: the (K*R) x (K*R) system blkdiag(w*C_k) + rhoC/2*kron(H'H, I) (+ rhoC/2*I), rhoC = mean(rho) (:282-297, :371-385)
void Engine::par2_prepare_C_coupled(int m, int ctype, const aoadmm_options& opt) {
  ModeInfo& mi = modes_[m];
  TensorInfo& t = tensors_[mi.tensor];
  Par2Block& b = t.p2;
  const P2Dims d = b.dims();
  ModeInfo& mA = modes_[t.modes[0]];
  ModeInfo& mB = modes_[t.modes[1]];
  AdmmCtl* ctl = ctl_of_mode(m);
  const int con = mi.constrained ? 1 : 0;
  const P2CCoupledKind ck = par2_c_coupled_kind(ctype, con);
  const bool big = ck.raw != 0;                       // H*C = ...: one (K*R) x (K*R) system instead of K row systems
  b.rhosum.ensure(64);
  if (b.sparse) {
    par2s_ensure_Y(t);
    par2s_slab_sums(mB.fac.d(), b.sp.Y.d(), d, b.sp.s.d(), nullptr, nullptr, nullptr, nullptr, nullptr, stream_);
    par2_c_system_pre(b.sp.s.d(), mA.gram.d(), b.GB.d(), t.weight, has_ridge_ ? mi.ridge : 0.0,
                      opt.bsum ? opt.bsum_weight / 2 : 0.0, ck.nrho, ck.raw, d, mi.fac.d(), b.ac.d(), b.rhoc.d(),
                      b.Lc.d(), ctl, stream_, ck.madd ? mi.HHt.d() : nullptr);
  } else {
    P2CSys cs;
    cs.X = b.X.d(); cs.A = mA.fac.d(); cs.B = mB.fac.d(); cs.GA = mA.gram.d(); cs.GB = b.GB.d(); cs.Cfac = mi.fac.d();
    cs.w = t.weight; cs.ridge = has_ridge_ ? mi.ridge : 0.0; cs.bsum_half = opt.bsum ? opt.bsum_weight / 2 : 0.0;
    cs.nrho = ck.nrho; cs.raw = ck.raw; cs.Madd = ck.madd ? mi.HHt.d() : nullptr;
    cs.T1 = b.T1.d(); cs.a = b.ac.d(); cs.rho = b.rhoc.d(); cs.L = b.Lc.d();
    par2_c_systems(cs, d, ctl, stream_);
  }
  // max(rho) for the prox (:1424); mean(rho) takes the place of the scalar rho of a CP mode (:284, :712), sum(rho)
  // weighs this mode in the Delta update (:736)
  par2_rho_max(b.rhoc.d(), b.K, b.rhomax.d(), stream_, mi.rho.d(), b.rhosum.d());
  t.last_pos = 2;                                                              // last_m(p) = 3
  mi.Aeff = b.ac.d();
  if (big) {
    const int n = b.K * b.R;
    AO_REQUIRE(mi.hc == b.K, "coupling matrix of the PARAFAC2 C mode has %lld columns, the mode has %d rows", (long long)mi.hc, b.K);
    if (!b.have_HtH) {
      // H'H once per model, on the host: when it is diagonal (H selects or scales rows -- every sampling-rate
      // coupling, script 14) kron(H'H, I) is diagonal too and the (K*R)-system falls apart into K row systems
      const int64_t hr = mi.hr;
      std::vector<double> hth((size_t)b.K * b.K, 0.0);
      bool diag = true;
      for (int a = 0; a < b.K; ++a)
        for (int c2 = 0; c2 < b.K; ++c2) {
          double acc = 0.0;
          for (int64_t q = 0; q < hr; ++q) acc += mi.H_host[(size_t)q + (size_t)hr * a] * mi.H_host[(size_t)q + (size_t)hr * c2];
          hth[(size_t)a + (size_t)b.K * c2] = acc;
          if (a != c2 && acc != 0.0) diag = false;
        }
      b.hth_diag = diag;
      if (diag) {
        std::vector<double> dd(b.K);
        for (int a = 0; a < b.K; ++a) dd[a] = hth[(size_t)a + (size_t)b.K * a];
        b.HtH.ensure((size_t)b.K * 8);
        AO_HIP(hipMemcpyAsync(b.HtH.p, dd.data(), (size_t)b.K * 8, hipMemcpyHostToDevice, stream_));
      } else {
        b.HtH.ensure((size_t)b.K * b.K * 8);
        AO_HIP(hipMemcpyAsync(b.HtH.p, hth.data(), hth.size() * 8, hipMemcpyHostToDevice, stream_));
      }
      AO_HIP(hipStreamSynchronize(stream_));          // hth / dd are locals
      b.have_HtH = true;
    }
    if (!b.hth_diag) {
      AO_REQUIRE(n <= kDenseMaxN, "PARAFAC2 C mode coupled with type %d through a matrix whose H'H is not diagonal: K*R = %d exceeds the dense-system limit %d", ctype, n, kDenseMaxN);
      b.Mbig.ensure((size_t)n * n * 8); b.Minv.ensure((size_t)n * n * 8);
    }
    par2_c_coupled_big(b.Lc.d(), b.HtH.d(), b.hth_diag, mi.rho.d(), con, b.K, b.R, b.hth_diag ? nullptr : b.Mbig.d(), ctl,
                       stream_);
    if (!b.hth_diag) dense_spd_inverse(b.Mbig.d(), b.Minv.d(), n, ctl, stream_);
  }
}

// objective pieces of a PARAFAC2 block that do not go through the last_mttkrp shortcut (:1262-1264, :1355, :1337)
void Engine::par2_objective_enqueue(TensorInfo& t) {
  Par2Block& b = t.p2;
  const P2Dims d = b.dims();
  ModeInfo& mA = modes_[t.modes[0]];
  ModeInfo& mB = modes_[t.modes[1]];
  ModeInfo& mC = modes_[t.modes[2]];
  const bool regs = mB.constrained && prox_has_reg_value(mB.prox.type);
  if (b.slab_sharded) {                               // per-slab values of the other ranks arrive through the all-reduce
    AO_HIP(hipMemsetAsync(b.res.p, 0, (size_t)b.K * 8, stream_));
    AO_HIP(hipMemsetAsync(b.q.p, 0, (size_t)b.K * 4 * 8, stream_));
    if (regs) AO_HIP(hipMemsetAsync(b.regv.p, 0, (size_t)b.K * 8, stream_));
  }
  if (b.sparse) {
    // ||X_k - A D_k B_k'||^2 = ||X_k||^2 - 2 sum_r C(k,r) s(k,r) + <GA, (c_k c_k') .* GB_k>, s from Y (the CP blocks'
    // move): no pass of its own unless A moved since Y was formed, and then the next B_k update reuses Y
    par2s_ensure_Y(t);
    par2s_slab_sums(mB.fac.d(), b.sp.Y.d(), d, b.sp.s.d(), b.sp.xn.d(), mC.fac.d(), mA.gram.d(), b.GB.d(), b.res.d(), stream_);
  }
  P2Objective og;                                     // residual (dense slabs), gaps, reg_func values
  og.X = b.sparse ? nullptr : b.X.d(); og.A = mA.fac.d(); og.B = mB.fac.d(); og.Cfac = mC.fac.d();
  og.P = b.P.d(); og.DeltaB = b.DeltaB.d(); og.Z = mB.constrained ? mB.Z.d() : nullptr;
  og.reg_type = regs ? mB.prox.type : AOADMM_C_NONE; og.eta = mB.prox.p0;
  og.res = b.res.d(); og.q = b.q.d(); og.regv = b.regv.d();
  par2_objective(og, d, stream_);
  if (b.slab_sharded) {
    // res[K] carries the not-positive-definite flags of this block's modes, so that a Cholesky failure in one
    // rank's slabs stops every rank (check_not_pd) instead of leaving the others waiting in a collective
    par2_collect_notpd(ctl_of_mode(t.modes[0]), ctl_of_mode(t.modes[1]), ctl_of_mode(t.modes[2]), b.res.d() + b.K, stream_);
    allreduce(b.res.d(), b.K + 1);
    allreduce(b.q.d(), (int64_t)b.K * 4);
    if (regs) allreduce(b.regv.d(), b.K);
  }
}

// End of a solve with slab-sharded blocks: every rank receives the slabs the others updated (G.fac{B}, G.P,
// G.mu_DeltaB and, if B_k is constrained, its split and dual variables), so aoadmm_state_get returns the same
// struct on every rank.
void Engine::par2_gather_slabs(TensorInfo& t) {
  Par2Block& b = t.p2;
  if (!b.slab_sharded) return;
  ModeInfo& mB = modes_[t.modes[1]];
  const int64_t n = b.Jtot * b.R, e0 = b.off_h[b.k0] * b.R, e1 = b.off_h[b.k1] * b.R;
  auto gather = [&](DevBuf& buf) {
    if (e0 > 0) AO_HIP(hipMemsetAsync(buf.p, 0, (size_t)e0 * 8, stream_));
    if (e1 < n) AO_HIP(hipMemsetAsync(buf.d() + e1, 0, (size_t)(n - e1) * 8, stream_));
    allreduce(buf.d(), n);
  };
  gather(mB.fac); gather(b.P); gather(b.muDB);
  if (mB.constrained && mB.has_Z) { gather(mB.Z); gather(mB.mu); }
  mB.version++;
}

}  // namespace aoadmm
