// Engine: the objective (CMTF_AOADMM_func_eval, functions/cmtf_fun_AOADMM.m:1213-1363).  The device half enqueues the
// reductions into the named slots of the read-back arena (readback.h); the host half reads the same slots from the
// pinned copy of the arena once the read-back has landed.
#include "solver.h"

#include <algorithm>
#include <cmath>

namespace aoadmm {

// ---------------------------------------------------------------------------
// device half: enqueue every reduction of one evaluation
// ---------------------------------------------------------------------------
void Engine::eval_objective_enqueue(bool first) {
  ReduceBatch rb;                                  // every plain reduction of this evaluation in one launch
  auto flush = [&]() {
    reduce_batch(rb, redws_.d(), stream_);
    rb = ReduceBatch();
  };
  // a batch holds kReduceBatchMax tasks and the model sets no cap on blocks or modes (20 coupled matrices are 40 tasks
  // before the first mode): a full batch is launched before the next task goes in.  Only models that did not fit one
  // batch before reach this, so the batches, and with them the summation order, of every other model stay as they were
  auto push = [&](const ReduceTask& k) {
    if (rb.n == kReduceBatchMax) flush();
    rb.add(k);
  };
  auto add = [&](int kind, double* slot, const double* x, const double* y, int64_t n) {
    ReduceTask k;
    k.kind = kind; k.slot = slot; k.x = x; k.y = y; k.n = n;
    push(k);
  };
  for (int p = 0; p < n_tensors_; ++p)           // held-out lists: scored against the fac state this evaluation uses
    if (tensors_[p].ho.n > 0) heldout_enqueue(p, dev_.heldout(p));
  if (rank_eval_now_)                            // ranking lists, at the iterations aoadmm_rank_track names: the same fac state
    for (int p = 0; p < n_tensors_; ++p)
      if (tensors_[p].rl.nq > 0) ranklist_enqueue(p, dev_.rank(p));
  for (int p = 0; p < n_tensors_; ++p) {
    TensorInfo& t = tensors_[p];
    const bool masked = t.masked();
    if (masked && first) em_pass_enqueue(p, 0);  // observed-entry residual (:1224-1226, :1249-1252); later
                                                 // evaluations reuse the statistics of the EM update pass
    if (t.observed_only()) {                     // likewise over the stored entries of an observed-only sparse block
      if (first) sparse_em_enqueue(p, true);
      continue;
    }
    if (t.par2) {
      par2_objective_enqueue(t);                 // direct residual (:1262-1264) + internal-coupling gaps (:1355)
      t.eval_shortcut = !masked && !first && t.last_pos == 0;   // remembered for objective_from_host: last_pos may move on before
      if (t.eval_shortcut) {                                // shortcut through last_mttkrp / last_had (:1254-1260)
        ModeInfo& lm = modes_[t.modes[0]];
        double* sp = dev_.tensor_obj(p);
        add(RT_DOT, sp + kObjMttkrpDot, lm.A.d(), lm.fac.d(), lm.rows * lm.R);
        add(RT_DOT, sp + kObjHadDot, lm.C.d(), lm.gram.d(), (int64_t)lm.R * lm.R);
      }
      continue;
    }
    // A marked block's imputing pass walked its list and left no observed-entry residual: later evaluations take the
    // two dot products an unmasked block gets and objective_from_host combines them with the list's sums
    t.eval_list = masked && !first && t.blk.mlist.on;
    if (masked && !t.eval_list) continue;
    if (first) {
      // cp_func.m:47-55 / pca_func.m:29-39: same formula with the first mode's MTTKRP
      ModeInfo& m0 = modes_[t.modes[0]];
      FactorRef facs[8];
      factor_refs(t, facs);
      std::vector<int> seq = update_sequence(p);
      block_mttkrp(block_ctx(), t.blk, 0, facs, m0.R, t.weight, m0.A.d(), m0.rows, true, seq.data(), (int)seq.size());
      SysBuild sb;
      sb.ngram = 0;
      for (int i = 1; i < t.nmodes; ++i) sb.grams[sb.ngram++] = modes_[t.modes[i]].gram.d();
      sb.Cpre = nullptr; sb.w = t.weight; sb.ridge = 0; sb.bsum_half = 0; sb.rho_scale = 1; sb.nrho = 1; sb.R = m0.R;
      sb.C = m0.C.d(); sb.rho = m0.rho.d(); sb.Bsys = m0.Bsys.d(); sb.L = m0.L.d(); sb.ctl = nullptr;
      sys_build(sb, stream_);
      t.last_pos = 0;
    }
    ModeInfo& lm = modes_[t.modes[t.last_pos]];
    double* sp = dev_.tensor_obj(p);
    add(RT_DOT, sp + kObjMttkrpDot, lm.A.d(), lm.fac.d(), lm.rows * lm.R);     // f_2 * w
    add(RT_DOT, sp + kObjHadDot, lm.C.d(), lm.gram.d(), (int64_t)lm.R * lm.R);  // f_3
  }
  for (int m = 0; m < n_modes_; ++m) {
    ModeInfo& mi = modes_[m];
    if (mi.slabs) continue;                      // per-slab ratios come from par2_b_gaps
    double* sm = dev_.mode_obj(m);
    const int64_t nm = mi.rows * mi.R;
    add(RT_SUMSQ_DIFF, sm + kObjFacSq, mi.fac.d(), nullptr, nm);
    if (mi.constrained) {
      add(RT_SUMSQ_DIFF, sm + kObjFacZSq, mi.fac.d(), mi.Z.d(), nm);
      const int ty = mi.prox.type;
      if (ty == AOADMM_C_L2_REG) {
        reg_value(sm + kObjRegValue, ty, mi.prox.p0, mi.fac.d(), mi.rows, mi.R, redws_.d(), stream_);
      } else if (ty == AOADMM_C_QUADRATIC) {       // eta*trace(x'*L*x) (:67): L*x into the prox workspace, then <x, L*x>
        gemm_small(mi.proxws.d(), mi.rows, mi.prox.Lmat, mi.rows, mi.fac.d(), mi.rows, mi.rows, (int)mi.rows, mi.R, 0,
                   coef(1.0), 0.0, nullptr, stream_);
        ReduceTask k;
        k.kind = RT_DOT; k.slot = sm + kObjRegValue; k.x = mi.fac.d(); k.y = mi.proxws.d(); k.n = nm; k.scale = mi.prox.p0;
        push(k);
      } else if (ty == AOADMM_C_L1_REG || ty == AOADMM_C_L0_REG || ty == AOADMM_C_RIDGE || ty == AOADMM_C_GL_SMOOTH ||
                 ty == AOADMM_C_TV) {
        ReduceTask k;
        k.kind = RT_REG; k.aux = ty; k.slot = sm + kObjRegValue; k.x = mi.fac.d(); k.rows = mi.rows; k.R = mi.R; k.scale = mi.prox.p0;
        push(k);
      }
    }
    if (mi.coupling >= 0) {                        // :1303-1329
      CouplingInfo& ci = couplings_[mi.coupling];
      const size_t nimg = (size_t)std::max(nm, mi.img_rows * mi.img_cols) * sizeof(double);
      mi.TD.ensure(nimg); mi.TF.ensure(nimg);
      const double* td = image_d(mi.TD.d(), ci, ci.Delta.d(), mi, nullptr, stream_);
      const double* tf = image_f(mi.TF.d(), ci, mi.fac.d(), mi, nullptr, stream_);
      add(RT_SUMSQ_DIFF, sm + kObjCouplGap, tf, td, mi.img_rows * mi.img_cols);
      if (tf != mi.fac.d()) add(RT_SUMSQ_DIFF, sm + kObjImageSq, tf, nullptr, mi.img_rows * mi.img_cols);   // ||H*C|| / ||C*H||
    }
    if (rb.n >= kReduceBatchMax - 4) flush();    // many modes: start the next batch
  }
  flush();
}

// ---------------------------------------------------------------------------
// host half: the same slots, read from the pinned copy `h` of the arena
// ---------------------------------------------------------------------------
void Engine::check_not_pd(const ArenaView& h) const {
  for (int i = 0; i < arena_.n_ctl(); ++i)
    if (h.ctl(i)->notpd)
      throw Error(AOADMM_ERR_NOT_PD, "Cholesky failed: system matrix is not positive definite (chol in cmtf_fun_AOADMM.m:142/273/362)");
  for (int p = 0; p < n_tensors_; ++p) {
    const TensorInfo& t = tensors_[p];
    if (t.par2 && t.p2.slab_sharded && h.p2_res(p)[t.p2.K] > 0)   // some rank's slabs hit a non-positive-definite system (the slot is only written then)
      throw Error(AOADMM_ERR_NOT_PD, "Cholesky failed in a PARAFAC2 slab system on another rank (chol in cmtf_fun_AOADMM.m:212/240)");
  }
}

void Engine::objective_from_host(const ArenaView& h, double f[4]) const {
  double ft = 0.0, fpar = 0.0, fcon = 0.0;
  int ncon = 0;
  for (int p = 0; p < n_tensors_; ++p) {
    const TensorInfo& t = tensors_[p];
    const double* sp = h.tensor_obj(p);
    const bool masked = t.missing();
    if (t.par2) {
      const Par2Block& b = t.p2;
      const double* res = h.p2_res(p);
      const double* q = h.p2_q(p);
      double fp = 0.0;
      if (masked) fp = h.em(p)[kEmObsRes];                                                    // :1249-1252
      else if (t.eval_shortcut) fp = t.normsq - 2.0 * (sp[kObjMttkrpDot] / t.weight) + sp[kObjHadDot];   // :1254-1260
      else for (int k = 0; k < b.K; ++k) fp += res[k];                                        // :1262-1264
      ft += t.weight * fp;                                                                    // :1267
      const ModeInfo& mB = modes_[t.modes[1]];
      double gp = 0.0, gz = 0.0, nb2 = 0.0;
      for (int k = 0; k < b.K; ++k) {
        const double* qk = q + kSlabSums * k;
        const double nb = std::sqrt(qk[kSlabNormB]);
        gp += std::sqrt(qk[kSlabGapP]) / nb;                                                  // :1355
        gz += std::sqrt(qk[kSlabGapZ]) / nb;                                                  // :1337
        nb2 += qk[kSlabNormB];
      }
      fpar += gp;
      if (mB.constrained && mB.prox.type == AOADMM_C_TPARAFAC2) {        // t_smoothness_penalty.m via reg_func (:1276-1277)
        double pen = 0.0;
        for (int k = 1; k < b.K; ++k) pen += q[kSlabSums * k + kSlabSmooth];
        ft += mB.prox.p0 * pen;
      }
      if (mB.constrained && prox_has_reg_value(mB.prox.type)) {          // sum_k reg_func(B_k) (:1279-1281)
        const double* rv = h.p2_regv(p);
        for (int k = 0; k < b.K; ++k) ft += rv[k];
      }
      if (mB.constrained) {
        const double g = gz / b.K;                                                            // :1339
        fcon += g;
        if (g != 0.0) ++ncon;
        if (has_ridge_) ft += mB.ridge * nb2;                                                 // :1292-1295 (quirk: only if constrained)
      }
    } else if (masked && t.eval_list) {
      // ||miss.*(X - M)||^2 = ||Xhat - M||^2 - num with Xhat the array the iteration's last MTTKRP ran on (its missing
      // entries still held the previous imputation, whose squares are den) and normsq = ||miss.*X||^2
      const double f2 = sp[kObjMttkrpDot] / t.weight;
      const double res = (t.normsq + h.em(p)[kEmDen]) - 2.0 * f2 + sp[kObjHadDot] - h.em(p)[kEmNum];
      ft += t.weight * (res > 0.0 ? res : 0.0);
    } else if (masked) {
      ft += t.weight * h.em(p)[kEmObsRes];                                   // :1224-1226 = w * ||miss.*(X - M)||^2
    } else {
      const double f2 = sp[kObjMttkrpDot] / t.weight;                       // last_mttkrp = A*1/w (:121)
      ft += t.weight * (t.normsq - 2.0 * f2 + sp[kObjHadDot]);               // :1235-1241
    }
  }
  if (fpar > 0) {                                                            // :1360-1362 (quirk: K of the LAST tensor)
    const TensorInfo& tl = tensors_[n_tensors_ - 1];
    fpar /= tl.par2 ? tl.p2.K : 1;
  }
  std::vector<double> cp(n_couplings_, 0.0);
  for (int m = 0; m < n_modes_; ++m) {
    const ModeInfo& mi = modes_[m];
    if (mi.slabs) continue;
    const double* sm = h.mode_obj(m);
    const double nf = std::sqrt(sm[kObjFacSq]);
    if (mi.constrained) {
      const int ty = mi.prox.type;
      if (prox_has_reg_value(ty)) ft += sm[kObjRegValue];                    // reg_func (:1272-1288)
      const double g = std::sqrt(sm[kObjFacZSq]) / nf;                      // :1341
      fcon += g;
      if (g != 0.0) ++ncon;
    }
    if (has_ridge_) ft += mi.ridge * sm[kObjFacSq];                          // :1297
    if (mi.coupling >= 0) {                                                  // :1309-1323
      const int cty = couplings_[mi.coupling].type;
      const double den = (cty == 1 || cty == 2 || cty == 5) ? std::sqrt(sm[kObjImageSq]) : nf;   // ||H*C|| / ||C*H||
      cp[mi.coupling] += std::sqrt(sm[kObjCouplGap]) / den;
    }
  }
  double fc = 0.0; int nc = 0;
  for (double v : cp) { fc += v; if (v != 0.0) ++nc; }
  if (fc > 0) fc /= nc;                                                      // :1327-1329 (the non-zero entries only)
  if (fcon > 0) fcon /= ncon;                                                // :1346-1348 (likewise)
  f[0] = ft; f[1] = fc; f[2] = fcon; f[3] = fpar;
}

// relative change of the imputed entries over the masked tensors (:436-440), from the EM statistics
double Engine::rel_missing_from_host(const ArenaView& h) const {
  double num = 0.0, den = 0.0;
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].missing()) { num += h.em(p)[kEmNum]; den += h.em(p)[kEmDen]; }
  return den > 0 ? std::sqrt(num / den) : std::sqrt(num);
}
}  // namespace aoadmm
