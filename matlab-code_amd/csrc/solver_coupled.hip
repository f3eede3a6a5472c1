// Engine: the coupled ADMM inner loop (functions/cmtf_fun_AOADMM.m:625-1075), one function per form of the loop.  The
// kernels and their launchers are in couple.{h,hip}.
#include <algorithm>

#include "solver.h"

namespace aoadmm {

// The six linear couplings (cmtf_fun_AOADMM.m:625-1075) in one form:  Tf_m(C_m) = Sd_m(Delta)
//   type 0: C = Delta | 1: H*C = Delta | 2: C*H = Delta | 3: C = H*Delta | 4: C = Delta*H | 5: H*C = Delta*H2
// Sd: the Delta-side image for mode m (shape img_rows x img_cols)
const double* image_d(double* dst, const CouplingInfo& ci, const double* D, const ModeInfo& mi,
                      const AdmmCtl* ctl, hipStream_t s) {
  switch (ci.type) {
    case 3: gemm_small(dst, mi.rows, mi.H.d(), mi.hr, D, ci.rows, mi.rows, (int)ci.rows, mi.R, 0, coef(1.0), 0.0, ctl, s); return dst;
    case 4: gemm_small(dst, mi.rows, D, ci.rows, mi.H.d(), mi.hr, ci.rows, (int)ci.cols, mi.R, 0, coef(1.0), 0.0, ctl, s); return dst;
    case 5: gemm_small(dst, ci.rows, D, ci.rows, mi.H2.d(), mi.h2r, ci.rows, (int)ci.cols, mi.R, 0, coef(1.0), 0.0, ctl, s); return dst;
    default: return D;                               // types 0, 1, 2: Sd is the identity
  }
}
// Tf: the factor-side image (same shape); types 0, 3, 4 are the identity and return F itself
const double* image_f(double* dst, const CouplingInfo& ci, const double* F, const ModeInfo& mi,
                      const AdmmCtl* ctl, hipStream_t s) {
  if (ci.type == 1 || ci.type == 5) {
    gemm_small(dst, mi.hr, mi.H.d(), mi.hr, F, mi.rows, mi.hr, (int)mi.rows, mi.R, 0, coef(1.0), 0.0, ctl, s);
    return dst;
  }
  if (ci.type == 2) {
    gemm_small(dst, mi.rows, F, mi.rows, mi.H.d(), mi.hr, mi.rows, mi.R, (int)mi.hc, 0, coef(1.0), 0.0, ctl, s);
    return dst;
  }
  return F;
}
// Tf': adjoint of the factor-side map applied to Y (img shape) -> rows x R ; identity for types 0, 3, 4
const double* adjoint_f(double* dst, const CouplingInfo& ci, const double* Y, const ModeInfo& mi,
                        const AdmmCtl* ctl, hipStream_t s) {
  if (ci.type == 1 || ci.type == 5) {               // H' * Y
    gemm_small(dst, mi.rows, mi.Ht.d(), mi.hc, Y, mi.img_rows, mi.rows, (int)mi.hr, mi.R, 0, coef(1.0), 0.0, ctl, s);
    return dst;
  }
  if (ci.type == 2) {                                // Y * H'
    gemm_small(dst, mi.rows, Y, mi.rows, mi.H.d(), mi.hr, mi.rows, (int)mi.hc, mi.R, 1, coef(1.0), 0.0, ctl, s);
    return dst;
  }
  return Y;
}

// the PARAFAC2 block whose C mode `mi` is, or null
Par2Block* Engine::par2_c_block(const ModeInfo& mi) {
  return (tensors_[mi.tensor].par2 && mi.pos == 2) ? &tensors_[mi.tensor].p2 : nullptr;
}

// iteration limit and the four inner tolerances: WgLoopArgs and FinalizeArgs name them alike
template <class Args>
static void set_loop_limits(Args& a, const aoadmm_options& opt) {
  a.max_inner = opt.MaxInnerIters;
  a.tol_pr_coupl = opt.innerRelPrTol_coupl; a.tol_pr_constr = opt.innerRelPrTol_constr;
  a.tol_du_coupl = opt.innerRelDualTol_coupl; a.tol_du_constr = opt.innerRelDualTol_constr;
}
// what closes an inner iteration of the launch-per-step forms: every mode of the coupling with its residual slots
FinalizeArgs Engine::coupled_finalize_args(const CouplingInfo& ci, const aoadmm_options& opt) {
  FinalizeArgs fa;
  fa.nmodes = (int)ci.modes.size();
  set_loop_limits(fa, opt);
  for (int j = 0; j < fa.nmodes; ++j) {
    fa.slots[j] = resid_slots(ci.modes[j]);
    fa.constrained[j] = modes_[ci.modes[j]].constrained ? 1 : 0;
    fa.coupled[j] = 1;
  }
  return fa;
}

// which form runs coupling ci: couple_path() on what the model says about its modes
Engine::CoupleForm Engine::coupled_form(const CouplingInfo& ci) {
  int rmax = (int)ci.cols;                            // largest rank, cols(Delta) included
  bool any_pc = false;                                // a PARAFAC2 C mode in this coupling (types 0 and 1 only)
  bool local_prox = true;                             // every constrained mode's prox runs inside the loop kernels
  for (int m : ci.modes) {
    const ModeInfo& mj = modes_[m];
    any_pc = any_pc || par2_c_block(mj) != nullptr;
    rmax = std::max(rmax, mj.R);
    local_prox = local_prox && (!mj.constrained || prox_is_fusable(mj.prox.type));
  }
  return CoupleForm{couple_path(ci.type, (int)ci.modes.size(), ci.rows, rmax, any_pc, local_prox), rmax, any_pc};
}

void Engine::coupled_admm(int c, const aoadmm_options& opt) {
  CouplingInfo& ci = couplings_[c];
  AdmmCtl* ctl = ctl_of_coupling(c);
  const int n = (int)ci.modes.size();
  const int ty = ci.type;
  const int64_t nD = ci.rows * ci.cols;
  ci.DeltaOld.ensure(nD * 8); ci.BB.ensure(nD * 8); ci.dD.ensure(nD * 8); ci.tmp.ensure(nD * 8);
  ci.coef.ensure(64 * 8);
  const int64_t qa = ty == 3 ? ci.rows : ci.cols;    // order of the Delta normal equations (types 3 / 4, 5)
  ci.AA.ensure((size_t)qa * qa * 8); ci.LAA.ensure((size_t)qa * qa * 8);
  for (int j = 0; j < n; ++j) {                       // image-shaped work buffers
    ModeInfo& mi = modes_[ci.modes[j]];
    const size_t nimg = (size_t)std::max(mi.rows * mi.R, mi.img_rows * mi.img_cols) * sizeof(double);
    mi.TD.ensure(nimg); mi.TF.ensure(nimg); mi.tmp.ensure(nimg); mi.W1.ensure(nimg); mi.W2.ensure(nimg);
  }
  // per-outer-iteration constants
  std::vector<const double*> hp(n);
  for (int j = 0; j < n; ++j) {
    const ModeInfo& mj = modes_[ci.modes[j]];
    Par2Block* pb = par2_c_block(mj);
    hp[j] = pb ? pb->rhosum.d() : mj.rho.d();         // type 1 weighs a C mode with sum(rho) (:736)
  }
  const CoupleForm form = coupled_form(ci);
  const CouplePath path = form.path;
  const int rmax = form.rmax;
  const bool any_pc = form.any_pc;
  // reset the loop control (the per-mode sys_build calls reset their own blocks); types 0-2: in coupling_coefs_k below
  if (!(ty == 0 || ty == 1 || ty == 2) && path != CouplePath::Regs) ctl_reset(ctl, stream_);
  DevBuf& rho_ptrs = ci.rho_ptrs;                     // pointers never change once the work buffers exist
  if (ci.rho_ptrs_host != hp) {
    rho_ptrs.ensure(8 * sizeof(double*));
    AO_HIP(hipMemcpyAsync(rho_ptrs.p, hp.data(), n * sizeof(double*), hipMemcpyHostToDevice, stream_));
    AO_HIP(hipStreamSynchronize(stream_));            // hp is a local
    ci.rho_ptrs_host = hp;
  }
  const double* rho_last = modes_[ci.modes[n - 1]].rho.d();   // type 5: rhoC = mean(rho{mm}) with the stale loop variable (:1032)
  if (ty == 0 || ty == 1 || ty == 2) {
    if (path != CouplePath::Regs) coupling_coefs(ci.coef.d(), rho_ptrs.as<const double*>(), n, ctl, stream_);
  } else if (ty == 4 || ty == 5) {
    AAArgs aa, aaa;                                   // aaa: the PARAFAC2 C mode's H*H' kept apart (:946-948)
    aa.n = 0; aa.Rc = (int)ci.cols; aaa.n = 0; aaa.Rc = (int)ci.cols;
    for (int j = 0; j < n; ++j) {
      const ModeInfo& mj = modes_[ci.modes[j]];
      AAArgs& dst = par2_c_block(mj) ? aaa : aa;
      dst.H[dst.n] = ty == 4 ? mj.H.d() : mj.H2.d();
      dst.rho[dst.n] = (&dst == &aaa) ? ones_.d() : (ty == 4 ? hp[j] : rho_last);
      dst.R[dst.n] = mj.R;
      dst.n++;
    }
    coupling_AA(ci.AA.d(), aa, stream_);
    // with a C mode LAA holds AAA: the per-row systems are factored in the Delta step
    if (aaa.n > 0) coupling_AA(ci.LAA.d(), aaa, stream_);
    else chol_only(ci.LAA.d(), ci.AA.d(), (int)ci.cols, ctl, stream_);
  }
  if (path == CouplePath::Regs || path == CouplePath::Wg) coupled_one_launch(ci, ctl, opt, path, rmax);
  else if (path == CouplePath::RowSteps) coupled_row_steps(ci, ctl, opt, rmax);
  else coupled_generic(ci, ctl, opt, any_pc);
}

// the whole loop in one launch of one workgroup (CouplePath::Regs, CouplePath::Wg)
void Engine::coupled_one_launch(CouplingInfo& ci, AdmmCtl* ctl, const aoadmm_options& opt, CouplePath path, int rmax) {
  const int n = (int)ci.modes.size(), ty = ci.type;
  WgLoopArgs wa;
  wa.n = n; wa.q = (int)ci.cols; wa.type = ty; wa.rows = ci.rows;
  wa.Delta = ci.Delta.d(); wa.DeltaOld = ci.DeltaOld.d(); wa.dD = ci.dD.d(); wa.coefs = ci.coef.d(); wa.LAA = ci.LAA.d();
  set_loop_limits(wa, opt);
  wa.ctl = ctl;
  wa.self_start = path == CouplePath::Regs;         // that kernel opens the loop itself: nothing was launched in front of it
  for (int j = 0; j < n; ++j) {
    ModeInfo& mi = modes_[ci.modes[j]];
    WgLoopMode& wm = wa.m[j];
    wm.Aeff = mi.Aeff; wm.L = mi.L.d(); wm.rho = mi.rho.d(); wm.H = ty == 4 ? mi.H.d() : nullptr;
    wm.fac = mi.fac.d(); wm.muD = mi.muD.d(); wm.Z = mi.Z.d(); wm.mu = mi.mu.d(); wm.Zold = mi.Zold.d();
    wm.slots = resid_slots(ci.modes[j]);
    wm.R = mi.R; wm.constrained = mi.constrained ? 1 : 0; wm.ptype = mi.prox.type; wm.p0 = mi.prox.p0; wm.p1 = mi.prox.p1;
  }
  couple_loop_one_launch(wa, path, rmax, stream_);
}

// row-local coupling, one launch per step (CouplePath::RowSteps)
void Engine::coupled_row_steps(CouplingInfo& ci, AdmmCtl* ctl, const aoadmm_options& opt, int rmax) {
  const int n = (int)ci.modes.size(), ty = ci.type, q = (int)ci.cols;
  const int64_t rows = ci.rows;
  RowCouple rc[8];
  RowDelta rd;
  rd.n = n;
  for (int j = 0; j < n; ++j) {
    ModeInfo& mi = modes_[ci.modes[j]];
    rc[j].Aeff = mi.Aeff; rc[j].L = mi.L.d(); rc[j].rho = mi.rho.d(); rc[j].H = ty == 4 ? mi.H.d() : nullptr;
    rc[j].fac = mi.fac.d(); rc[j].muD = mi.muD.d(); rc[j].Z = mi.Z.d(); rc[j].mu = mi.mu.d();
    rc[j].R = mi.R; rc[j].constrained = mi.constrained ? 1 : 0;
    rd.fac[j] = mi.fac.d(); rd.muD[j] = mi.muD.d(); rd.rho[j] = mi.rho.d(); rd.H[j] = rc[j].H; rd.R[j] = mi.R;
  }
  const FinalizeArgs fa = coupled_finalize_args(ci, opt);
  for (int it = 0; it < opt.MaxInnerIters; ++it) {
    for (int j = 0; j < n; ++j)                       // primal: Sd(Delta), right-hand side and row solve in one kernel
      couple_primal_rows(rc[j], ci.Delta.d(), rows, q, ty, rmax, ctl, stream_);
    couple_delta_rows(rd, ci.Delta.d(), ci.DeltaOld.d(), ci.dD.d(), ci.coef.d(), ci.LAA.d(), rows, q, ty, rmax, ctl,
                      stream_);                       // Delta_old, Delta, dD
    for (int j = 0; j < n; ++j) {                     // duals, constraints, residual sums
      ModeInfo& mi = modes_[ci.modes[j]];
      double* sl = resid_slots(ci.modes[j]);
      couple_dual_rows(rc[j], ci.Delta.d(), ci.dD.d(), rows, q, ty, rmax, sl + 4, redws_.d(), ctl, stream_);
      if (mi.constrained)
        constraint_update(mi.prox, mi.fac.d(), mi.Z.d(), mi.mu.d(), mi.Zold.d(), mi.V.d(), mi.rows, mi.R, mi.rho.d(), 1.0,
                          mi.proxws.d(), sl, redws_.d(), ctl, stream_);
      else
        sumsq_diff(sl + 1, mi.fac.d(), nullptr, mi.rows * mi.R, redws_.d(), ctl, stream_);
    }
    admm_finalize_generic(fa, ctl, stream_);
  }
}

// any coupling (CouplePath::Generic): an inner iteration is the three steps below
void Engine::coupled_generic(CouplingInfo& ci, AdmmCtl* ctl, const aoadmm_options& opt, bool any_pc) {
  const FinalizeArgs fa = coupled_finalize_args(ci, opt);
  for (int it = 0; it < opt.MaxInnerIters; ++it) {
    for (int m : ci.modes) coupled_generic_primal(ci, modes_[m], ctl, it == 0);
    coupled_generic_delta(ci, ctl, any_pc);
    for (int m : ci.modes) coupled_generic_dual(ci, m, ctl);
    admm_finalize_generic(fa, ctl, stream_);
  }
}

// ---- primal update of one mode (:635-658, :713-730, :783-800, :853-870, :913-936, :1004-1020)
void Engine::coupled_generic_primal(CouplingInfo& ci, ModeInfo& mi, AdmmCtl* ctl, bool first) {
  const int ty = ci.type;
  const int64_t nm = mi.rows * mi.R, ni = mi.img_rows * mi.img_cols;
  // Sd(Delta): after the first inner iteration the image computed in the dual step below is still current
  const double* TD = (first || ty == 0 || ty == 1 || ty == 2) ? image_d(mi.TD.d(), ci, ci.Delta.d(), mi, ctl, stream_)
                                                                 : mi.TD.d();
  Par2Block* pb = par2_c_block(mi);
  if (pb && ty != 1 && ty != 5) {
    // row k: A_inner = a_k + rho_k/2*Tf'(Sd(Delta) - mu_Delta)(k,:) [+ rho_k/2*(Z - mu)(k,:)], solved with L_k
    // (:638-645, :785-792, :850-857, :916-923); Tf' is the identity except for type 2 (right-multiplication by H')
    if (ty == 2) {
      Coef c2[2] = {coef(1.0), coef(-1.0)};
      const double* x2[2] = {TD, mi.muD.d()};
      ew_lincomb(mi.tmp.d(), ni, 2, c2, x2, ctl, stream_);
      const double* adj = adjoint_f(mi.TF.d(), ci, mi.tmp.d(), mi, ctl, stream_);
      Coef cf[3] = {coef(1.0), coef(1.0), coef(-1.0)};
      const double* x[3] = {adj, mi.Z.d(), mi.mu.d()};
      ew_lincomb(mi.RHS.d(), nm, mi.constrained ? 3 : 1, cf, x, ctl, stream_);
    } else {
      Coef cf[4] = {coef(1.0), coef(-1.0), coef(1.0), coef(-1.0)};
      const double* x[4] = {TD, mi.muD.d(), mi.Z.d(), mi.mu.d()};
      ew_lincomb(mi.RHS.d(), nm, mi.constrained ? 4 : 2, cf, x, ctl, stream_);
    }
    par2_c_rowsolve(pb->ac.d(), pb->rhoc.d(), pb->Lc.d(), mi.RHS.d(), nullptr, 1, pb->dims_all(), mi.fac.d(), ctl, stream_);
    return;
  }
  if (ty == 0 || ty == 3 || ty == 4) {
    Coef cf[5] = {coef(1.0), coef(mi.rho.d(), 0.5), coef(mi.rho.d(), -0.5), coef(mi.rho.d(), 0.5), coef(mi.rho.d(), -0.5)};
    const double* x[5] = {mi.Aeff, TD, mi.muD.d(), mi.Z.d(), mi.mu.d()};
    ew_lincomb(mi.RHS.d(), nm, mi.constrained ? 5 : 3, cf, x, ctl, stream_);
  } else {
    Coef c2[2] = {coef(1.0), coef(-1.0)};
    const double* x2[2] = {TD, mi.muD.d()};
    ew_lincomb(mi.tmp.d(), ni, 2, c2, x2, ctl, stream_);                   // Sd(Delta) - mu_Delta
    const double* adj = adjoint_f(mi.TF.d(), ci, mi.tmp.d(), mi, ctl, stream_);
    Coef cf[4] = {coef(1.0), coef(mi.rho.d(), 0.5), coef(mi.rho.d(), 0.5), coef(mi.rho.d(), -0.5)};
    const double* x[4] = {mi.Aeff, adj, mi.Z.d(), mi.mu.d()};
    ew_lincomb(mi.RHS.d(), nm, mi.constrained ? 4 : 2, cf, x, ctl, stream_);
  }
  if (pb && (ty == 1 || ty == 5)) {
    // vec(C') = (blkdiag(B_k) + rhoC/2*kron(H'H,I) [+ rhoC/2*I]) \ vec(A_inner') (:714-722); mi.rho holds rhoC
    if (pb->hth_diag)                             // H'H diagonal: the system is K row systems (solver_par2.hip)
      par2_c_rowsolve(mi.RHS.d(), pb->rhoc.d(), pb->Lc.d(), nullptr, nullptr, 0, pb->dims_all(), mi.fac.d(), ctl, stream_);
    else
      dense_symv_rows(pb->Minv.d(), mi.RHS.d(), mi.fac.d(), pb->K, pb->R, ctl, stream_);
  } else if (ty == 1 || ty == 5) {
    // sylvester(B2, B, A_inner) (:707, :1016) with B2 = rho/2*H'H (+ rho/2*I if constrained) = U (..) U',
    // B = V diag(mu) V':  X = U * ((U' A_inner V) ./ (beta_i + mu_j)) * V'
    gemm_small(mi.W1.d(), mi.rows, mi.eUt.d(), mi.rows, mi.RHS.d(), mi.rows, mi.rows, (int)mi.rows, mi.R, 0, coef(1.0), 0.0, ctl, stream_);
    gemm_small(mi.W2.d(), mi.rows, mi.W1.d(), mi.rows, mi.eV.d(), mi.R, mi.rows, mi.R, mi.R, 0, coef(1.0), 0.0, ctl, stream_);
    sylv_scale(mi.W2.d(), mi.rows, mi.R, mi.eLam.d(), mi.eMu.d(), mi.rho.d(), 1.0, mi.constrained ? 1.0 : 0.0, ctl, stream_);
    gemm_small(mi.W1.d(), mi.rows, mi.W2.d(), mi.rows, mi.eV.d(), mi.R, mi.rows, mi.R, mi.R, 1, coef(1.0), 0.0, ctl, stream_);
    gemm_small(mi.fac.d(), mi.rows, mi.eU.d(), mi.rows, mi.W1.d(), mi.rows, mi.rows, (int)mi.rows, mi.R, 0, coef(1.0), 0.0, ctl, stream_);
  } else {
    row_solve(mi.fac.d(), mi.rows, mi.RHS.d(), mi.rows, mi.L.d(), mi.rows, mi.R, ctl, stream_);
  }
}

// ---- Delta update
void Engine::coupled_generic_delta(CouplingInfo& ci, AdmmCtl* ctl, bool any_pc) {
  const int n = (int)ci.modes.size(), ty = ci.type;
  const int64_t nD = ci.rows * ci.cols;
  const double* rho_last = modes_[ci.modes[n - 1]].rho.d();   // type 5: rhoC, see coupled_admm
  {
    Coef c1[1] = {coef(1.0)};
    const double* x1[1] = {ci.Delta.d()};
    ew_lincomb(ci.DeltaOld.d(), nD, 1, c1, x1, ctl, stream_);
  }
  if ((ty == 0 || ty == 2) && any_pc) {             // per-row weights rho_j(k) (:666-675, :805-811)
    RowMeanArgs ra;
    ra.n = n; ra.rows = ci.rows; ra.cols = (int)ci.cols;
    for (int j = 0; j < n; ++j) {
      ModeInfo& mi = modes_[ci.modes[j]];
      Par2Block* pb = par2_c_block(mi);
      ra.fac[j] = image_f(mi.TF.d(), ci, mi.fac.d(), mi, ctl, stream_); ra.mu[j] = mi.muD.d();
      ra.rho[j] = pb ? pb->rhoc.d() : mi.rho.d();
      ra.vec[j] = pb ? 1 : 0;
    }
    coupling_rowmean(ci.Delta.d(), ra, ctl, stream_);
  } else if (ty == 0 || ty == 1 || ty == 2) {       // weighted mean of Tf(C_j) + mu_j (:661-675, :735-741, :805-811)
    for (int j = 0; j < n; ++j) {
      ModeInfo& mi = modes_[ci.modes[j]];
      const double* tf = image_f(mi.TF.d(), ci, mi.fac.d(), mi, ctl, stream_);
      if (j == 0) {
        Coef cf[2] = {coef(ci.coef.d() + j, 1.0), coef(ci.coef.d() + j, 1.0)};
        const double* x[2] = {tf, mi.muD.d()};
        ew_lincomb(ci.Delta.d(), nD, 2, cf, x, ctl, stream_);
      } else {
        Coef cf[3] = {coef(1.0), coef(ci.coef.d() + j, 1.0), coef(ci.coef.d() + j, 1.0)};
        const double* x[3] = {ci.Delta.d(), tf, mi.muD.d()};
        ew_lincomb(ci.Delta.d(), nD, 3, cf, x, ctl, stream_);
      }
    }
  } else if (ty == 3) {                             // Delta = AA \ BB (:875-885)
    for (int j = 0; j < n; ++j) {
      ModeInfo& mi = modes_[ci.modes[j]];
      Coef cf[2] = {coef(1.0), coef(1.0)};
      const double* x[2] = {mi.fac.d(), mi.muD.d()};
      ew_lincomb(mi.tmp.d(), mi.rows * mi.R, 2, cf, x, ctl, stream_);
      if (Par2Block* pb = par2_c_block(mi)) {           // rows weighted by rho_k: H'*diag(rho)*H and H'*diag(rho)*(C + mu)
        pb->Hs.ensure((size_t)mi.hr * mi.hc * 8);
        rows_scale(pb->Hs.d(), mi.H.d(), pb->rhoc.d(), mi.hr, mi.hc, ctl, stream_);
        rows_scale(mi.tmp.d(), mi.tmp.d(), pb->rhoc.d(), mi.rows, mi.R, ctl, stream_);
        gemm_small(ci.AA.d(), ci.rows, mi.Ht.d(), mi.hc, pb->Hs.d(), mi.hr, ci.rows, (int)mi.rows, (int)ci.rows, 0,
                   coef(1.0), j == 0 ? 0.0 : 1.0, ctl, stream_);
        gemm_small(ci.BB.d(), ci.rows, mi.Ht.d(), mi.hc, mi.tmp.d(), mi.rows, ci.rows, (int)mi.rows, mi.R, 0,
                   coef(1.0), j == 0 ? 0.0 : 1.0, ctl, stream_);
        continue;
      }
      gemm_small(ci.AA.d(), ci.rows, mi.Ht.d(), mi.hc, mi.H.d(), mi.hr, ci.rows, (int)mi.rows, (int)ci.rows, 0,
                 coef(mi.rho.d(), 1.0), j == 0 ? 0.0 : 1.0, ctl, stream_);
      gemm_small(ci.BB.d(), ci.rows, mi.Ht.d(), mi.hc, mi.tmp.d(), mi.rows, ci.rows, (int)mi.rows, mi.R, 0,
                 coef(mi.rho.d(), 1.0), j == 0 ? 0.0 : 1.0, ctl, stream_);
    }
    spd_solve_left(ci.AA.d(), ci.rows, ci.BB.d(), (int)ci.cols, ctl, stream_);
    Coef c1[1] = {coef(1.0)};
    const double* x1[1] = {ci.BB.d()};
    ew_lincomb(ci.Delta.d(), nD, 1, c1, x1, ctl, stream_);
  } else {                                          // types 4, 5: Delta = BB / AA (:939-963, :1026-1054)
    for (int j = 0; j < n; ++j) {
      ModeInfo& mi = modes_[ci.modes[j]];
      const double* tf = image_f(mi.TF.d(), ci, mi.fac.d(), mi, ctl, stream_);
      Coef cf[2] = {coef(1.0), coef(1.0)};
      const double* x[2] = {tf, mi.muD.d()};
      ew_lincomb(mi.tmp.d(), mi.img_rows * mi.img_cols, 2, cf, x, ctl, stream_);
      // BB += rho_j * (Tf(C_j) + mu_j) * H_j'   (:955 ; :1048 with H2 and rhoC)
      if (ty == 4 && par2_c_block(mi)) {                // rows weighted by rho_k (:955)
        rows_scale(mi.tmp.d(), mi.tmp.d(), par2_c_block(mi)->rhoc.d(), mi.rows, mi.R, ctl, stream_);
        gemm_small(ci.BB.d(), ci.rows, mi.tmp.d(), mi.rows, mi.H.d(), mi.hr, ci.rows, mi.R, (int)ci.cols, 1,
                   coef(1.0), j == 0 ? 0.0 : 1.0, ctl, stream_);
      } else if (ty == 4)
        gemm_small(ci.BB.d(), ci.rows, mi.tmp.d(), mi.rows, mi.H.d(), mi.hr, ci.rows, mi.R, (int)ci.cols, 1,
                   coef(mi.rho.d(), 1.0), j == 0 ? 0.0 : 1.0, ctl, stream_);
      else
        gemm_small(ci.BB.d(), ci.rows, mi.tmp.d(), mi.img_rows, mi.H2.d(), mi.h2r, ci.rows, mi.R, (int)ci.cols, 1,
                   coef(rho_last, 1.0), j == 0 ? 0.0 : 1.0, ctl, stream_);
    }
    if (any_pc) {                                   // Delta(k,:) = BB(k,:) / (AA + rho_k*AAA)  (:957-961, :1049-1052)
      const Par2Block* pb = nullptr;
      for (int j = 0; j < n; ++j)
        if (Par2Block* q = par2_c_block(modes_[ci.modes[j]])) pb = q;
      delta_rowwise_solve(ci.Delta.d(), ci.BB.d(), ci.rows, (int)ci.cols, ci.AA.d(), ci.LAA.d(), pb->rhoc.d(), ctl, stream_);
    } else
      row_solve(ci.Delta.d(), ci.rows, ci.BB.d(), ci.rows, ci.LAA.d(), ci.rows, (int)ci.cols, ctl, stream_);
  }
  {
    Coef cf[2] = {coef(1.0), coef(-1.0)};
    const double* x[2] = {ci.Delta.d(), ci.DeltaOld.d()};
    ew_lincomb(ci.dD.d(), nD, 2, cf, x, ctl, stream_);
  }
}

// ---- dual, constraint and residual pieces of mode m (:678-692 and the same block of every case)
void Engine::coupled_generic_dual(CouplingInfo& ci, int m, AdmmCtl* ctl) {
  const int ty = ci.type;
  ModeInfo& mi = modes_[m];
  double* sl = resid_slots(m);
  const int64_t nm = mi.rows * mi.R, ni = mi.img_rows * mi.img_cols;
  const double* TD = image_d(mi.TD.d(), ci, ci.Delta.d(), mi, ctl, stream_);
  const double* tf = image_f(mi.TF.d(), ci, mi.fac.d(), mi, ctl, stream_);
  // mu_Delta += Tf(C) - Sd(Delta); sl[4] = ||Tf(C) - Sd(Delta)||^2, sl[5] = ||mu_Delta||^2, sl[7] = ||den||^2 with
  // den = H*C (:1125) / C*H (:1143) for types 1, 2, else C
  coupling_dual(mi.muD.d(), tf, TD, ni, mi.fac.d(), nm, ty == 1 || ty == 2, sl + 4, redws_.d(), ctl, stream_);
  if (mi.constrained) {
    Par2Block* pb = par2_c_block(mi);                 // a C mode's prox gets max(rho) (:1423-1424)
    constraint_update(mi.prox, mi.fac.d(), mi.Z.d(), mi.mu.d(), mi.Zold.d(), mi.V.d(), mi.rows, mi.R,
                      pb ? pb->rhomax.d() : mi.rho.d(), 1.0, mi.proxws.d(), sl, redws_.d(), ctl, stream_);
  } else
    sumsq_diff(sl + 1, mi.fac.d(), nullptr, nm, redws_.d(), ctl, stream_);
  const double* dimg = image_d(mi.tmp.d(), ci, ci.dD.d(), mi, ctl, stream_);
  sumsq_diff(sl + 6, dimg, nullptr, ni, redws_.d(), ctl, stream_);
}

// aoadmm_op_coupled_loop: per mode what update_mode -> prepare_mode_system does behind the MTTKRP (A and C given),
// then coupled_admm and the Gram matrices, exactly as outer_updates runs them
void Engine::coupled_loop_op(int c, const double* const* A, const double* const* Cm, int max_inner, const double* tol,
                             int* inner_iters, double* res, double* rho, double* const* L, double* const* gram,
                             double* slots, int* path) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  if (sharded() || multi_member_)
    throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_op_coupled_loop runs on one engine without a communicator");
  AO_REQUIRE(c >= 0 && c < n_couplings_, "coupling %d out of range", c);
  AO_REQUIRE(A && Cm && tol && max_inner >= 1, "bad arguments");
  AO_HIP(hipSetDevice(device_));
  CouplingInfo& ci = couplings_[c];
  const int n = (int)ci.modes.size();
  for (int j = 0; j < n; ++j) {
    const int m = ci.modes[j];
    const ModeInfo& mi = modes_[m];
    if (tensors_[mi.tensor].par2)
      throw Error(AOADMM_ERR_UNSUPPORTED, fmt("aoadmm_op_coupled_loop: mode %d belongs to a PARAFAC2 block, whose systems come from the block", m + 1));
    AO_REQUIRE(A[j] && Cm[j], "mode %d: A or C missing", m + 1);
    AO_REQUIRE(mi.has_fac, "G.fac{%d} missing", m + 1);
    if (mi.constrained) AO_REQUIRE(mi.has_Z && mi.has_mu, "G.constraint_fac{%d} / constraint_dual_fac{%d} missing", m + 1, m + 1);
    AO_REQUIRE(mi.has_muD && mi.muD_rows == mi.img_rows && mi.muD_cols == mi.img_cols, "G.coupling_dual_fac{%d} missing or mis-sized", m + 1);
  }
  AO_REQUIRE(ci.has_state, "G.coupling_fac{%d} missing", c + 1);
  aoadmm_options opt{};
  opt.MaxInnerIters = max_inner;
  opt.innerRelPrTol_coupl = tol[0]; opt.innerRelPrTol_constr = tol[1];
  opt.innerRelDualTol_coupl = tol[2]; opt.innerRelDualTol_constr = tol[3];
  std::vector<DevBuf> cpre(n);
  for (int j = 0; j < n; ++j) {
    const int m = ci.modes[j];
    ModeInfo& mi = modes_[m];
    ensure_mode_work(mi);
    mi.quad.dirty = true;                             // rho may have moved ('quadratic regularization', non-symmetric L)
    const size_t nR = (size_t)mi.rows * mi.R * sizeof(double), RR = (size_t)mi.R * mi.R * sizeof(double);
    cpre[j].alloc(RR);
    AO_HIP(hipMemcpyAsync(mi.A.p, A[j], nR, hipMemcpyHostToDevice, stream_));
    AO_HIP(hipMemcpyAsync(cpre[j].p, Cm[j], RR, hipMemcpyHostToDevice, stream_));
    SysBuild sb = mode_sysbuild(m, coupled_nrho(m));
    sb.Cpre = cpre[j].d();
    close_mode_system(m, sb, true, mi.A.d());
  }
  AO_HIP(hipStreamSynchronize(stream_));              // the host arrays are the caller's
  const CoupleForm form = coupled_form(ci);
  coupled_admm(c, opt);                                                        // :277 / :366
  for (int m : ci.modes) { modes_[m].version++; compute_gram(modes_[m]); }    // :393-403
  std::vector<AdmmCtl> h((size_t)n + 1);
  for (int j = 0; j < n; ++j)
    AO_HIP(hipMemcpyAsync(&h[j], ctl_of_mode(ci.modes[j]), sizeof(AdmmCtl), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipMemcpyAsync(&h[n], ctl_of_coupling(c), sizeof(AdmmCtl), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  for (const AdmmCtl& k : h)
    if (k.notpd) throw Error(AOADMM_ERR_NOT_PD, "Matrix must be positive definite.");
  if (inner_iters) *inner_iters = h[n].iters;
  if (res) for (int i = 0; i < 4; ++i) res[i] = h[n].res[i];
  if (path) {
    path[0] = (int)form.path;
    path[1] = form.path == CouplePath::Generic ? 0 : couple_rank_class(form.rmax);
  }
  for (int j = 0; j < n; ++j) {
    const ModeInfo& mi = modes_[ci.modes[j]];
    const size_t RR = (size_t)mi.R * mi.R * sizeof(double);
    if (rho) AO_HIP(hipMemcpyAsync(rho + j, mi.rho.p, sizeof(double), hipMemcpyDeviceToHost, stream_));
    if (L && L[j]) AO_HIP(hipMemcpyAsync(L[j], mi.L.p, RR, hipMemcpyDeviceToHost, stream_));
    if (gram && gram[j]) AO_HIP(hipMemcpyAsync(gram[j], mi.gram.p, RR, hipMemcpyDeviceToHost, stream_));
    if (slots) AO_HIP(hipMemcpyAsync(slots + 8 * j, resid_slots(ci.modes[j]), 8 * sizeof(double), hipMemcpyDeviceToHost, stream_));
  }
  AO_HIP(hipStreamSynchronize(stream_));
}

}  // namespace aoadmm
