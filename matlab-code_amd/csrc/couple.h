// The coupled ADMM inner loop (functions/cmtf_fun_AOADMM.m:625-1075) on the device: the kernels of every form of the
// loop and their launchers.  Nothing here knows the engine or the model: a launcher takes device pointers and sizes and
// works out its own grid and LDS size.  The engine side is solver_coupled.hip.
#pragma once
#include "admm.h"
#include "common.h"
#include "small.h"

namespace aoadmm {

// Which form runs the inner loop.  Row-local forms: types 0 and 4, ranks and cols(Delta) up to 16, no PARAFAC2 C
// mode.  Small problems among them whose proxes all run inside the kernels take the whole loop in one launch of one
// workgroup: one row per thread with the state in registers (couple_loop_wg_regs_k, which opens the loop and forms
// rho_j / sum rho itself) or the LDS form (couple_loop_wg_k).  The others launch row kernels per step; everything
// else takes the generic loop.
// The values are those of AOADMM_CPATH_* (aoadmm_op_coupled_loop reports them).
enum class CouplePath {
  Regs = AOADMM_CPATH_REGS, Wg = AOADMM_CPATH_WG, RowSteps = AOADMM_CPATH_ROWSTEPS, Generic = AOADMM_CPATH_GENERIC
};
// `rmax`: largest rank, cols(Delta) included; `local_prox`: every constrained mode's prox runs inside the loop kernels
CouplePath couple_path(int type, int n_modes, int64_t rows, int rmax, bool any_par2_c, bool local_prox);
// The row kernels are instantiated for ranks (and cols(Delta)) up to 4, 8 and 16: the class of `rmax` <= 16.  Every
// launcher of a row-local form picks its instance by this (the registers kernel exists for 4 and 8 only, which is all
// couple_path() sends it).
int couple_rank_class(int rmax);

// ---- pieces of the generic loop (any coupling type)
// coef[j] = rho_j / sum rho, coef[n] = sum rho (:661-675); also opens the loop (what ctl_reset does: one launch fewer)
void coupling_coefs(double* coef, const double* const* rhos, int n, AdmmCtl* ctl, hipStream_t s);
struct AAArgs { const double* H[8]; const double* rho[8]; int R[8]; int n; int Rc; };
// AA = sum_j rho_j * H_j * H_j'   (:941-954 ; :1033-1047 with H2 and the common rhoC)
void coupling_AA(double* AA, const AAArgs& a, hipStream_t s);
// mu_Delta += Tf(C) - Sd(Delta) for one mode (tf, td: ni entries) with out[0] = ||Tf(C) - Sd(Delta)||^2, out[1] =
// ||mu_Delta||^2, out[3] = ||den||^2, den = Tf(C) (img_den) or C (fac, nm entries); `ws`: 3 doubles per block
void coupling_dual(double* muD, const double* tf, const double* td, int64_t ni, const double* fac, int64_t nm,
                   bool img_den, double* out, double* ws, const AdmmCtl* ctl, hipStream_t s);
// Delta(k,:) = sum_j rho_j(k) * (C_j + mu_j)(k,:) / sum_j rho_j(k)   (:661-675): rho_j is a K-vector for a PARAFAC2
// C mode (vec[j] = 1) and a scalar otherwise
struct RowMeanArgs { const double* fac[8]; const double* mu[8]; const double* rho[8]; int vec[8]; int n; int64_t rows; int cols; };
void coupling_rowmean(double* Delta, const RowMeanArgs& a, const AdmmCtl* ctl, hipStream_t s);
// out(k,c) = rho_k * in(k,c)  (rows of a K x cols matrix scaled by the rho vector of a PARAFAC2 C mode)
void rows_scale(double* out, const double* in, const double* rho, int64_t rows, int64_t cols, const AdmmCtl* ctl,
                hipStream_t s);
// Delta(k,:) = BB(k,:) / (AA + rho_k*AAA)   (:957-961): one workgroup per row, q x q system in LDS
void delta_rowwise_solve(double* Delta, const double* BB, int64_t rows, int q, const double* AA, const double* AAA,
                         const double* rho, AdmmCtl* ctl, hipStream_t s);

// ---------------------------------------------------------------------------
// Couplings of type 0 (C = Delta) and 4 (C = Delta*H) are row-local: row i of every coupled factor, of Delta and of
// the duals only ever meets row i.  One thread per row then does a whole step in registers, which turns the
// 27 launches of an inner iteration (two modes, generic path below) into 11.  RMAX bounds both R and cols(Delta).
struct RowCouple {
  // per mode
  const double* Aeff; const double* L; const double* rho; const double* H;   // H: q x R (type 4), unused for type 0
  double* fac; double* muD; const double* Z; const double* mu;
  int R, constrained;
};
// primal step of one mode: Sd(Delta), right-hand side and row solve in one kernel (:647-651, :925-929)
void couple_primal_rows(const RowCouple& m, const double* Delta, int64_t rows, int q, int type, int rmax,
                        const AdmmCtl* ctl, hipStream_t s);
struct RowDelta {
  const double* fac[8]; const double* muD[8]; const double* rho[8]; const double* H[8];
  int R[8];
  int n;
};
// Delta_old = Delta ; Delta = weighted mean (type 0, :661-675) or BB / AA (type 4, :939-963) ; dD = Delta - Delta_old
void couple_delta_rows(const RowDelta& a, double* Delta, double* DeltaOld, double* dD, const double* coefs,
                       const double* LAA, int64_t rows, int q, int type, int rmax, const AdmmCtl* ctl, hipStream_t s);
// mu_Delta += C - Sd(Delta) and the four sums of the coupling residuals (:1099-1115, :1175-1191) for one mode:
// out[0] = ||C - Sd(Delta)||^2, out[1] = ||mu_Delta||^2, out[2] = ||Sd(dD)||^2, out[3] = ||C||^2; `ws`: 4 doubles per block
void couple_dual_rows(const RowCouple& m, const double* Delta, const double* dD, int64_t rows, int q, int type, int rmax,
                      double* out, double* ws, const AdmmCtl* ctl, hipStream_t s);

// ---------------------------------------------------------------------------
// The whole inner loop of a row-local coupling (types 0 and 4) in ONE launch, for the sizes the example scripts use
// (rows of Delta up to a few thousand, ranks up to 16).  For these couplings every step of an inner iteration --
// the primal solves of all coupled modes (:647-651, :925-929), the Delta update (:661-675, :939-963), the coupling
// duals (:679, :967) and, with an element-/row-wise prox, update_constraint (:1420-1429) -- touches row i of every
// matrix only, so thread i carries row i through the iteration without meeting another thread; the workgroup meets
// once per iteration to add up the residual sums (:1099-1115, :1175-1191, :1079-1096) and to evaluate the while
// condition (:630).  The launch-per-step form (couple_primal / couple_delta / couple_dual + constraint_update +
// finalize: 12 launches per inner iteration for two constrained modes) is kept for larger problems.
struct WgLoopMode {
  const double* Aeff; const double* L; const double* rho; const double* H;
  double *fac, *muD, *Z, *mu, *Zold;
  double* slots;        // 8 residual sums of this mode (see FinalizeArgs)
  int R, constrained, ptype;
  double p0, p1;
};
struct WgLoopArgs {
  WgLoopMode m[4];
  int n, q, type, max_inner;
  int64_t rows;
  double *Delta, *DeltaOld, *dD;
  const double* coefs;
  const double* LAA;
  double tol_pr_coupl, tol_pr_constr, tol_du_coupl, tol_du_constr;
  AdmmCtl* ctl;
  int self_start = 0;       // registers kernel: opens the loop itself and takes rho_j / sum rho from the modes' rho
                            // (no ctl_reset / coupling_coefs_k launch in front of it)
};
// `path`: Regs (rows <= 256, rmax <= 8, a.n <= 3) or Wg (rmax <= 16), as couple_path() decided
void couple_loop_one_launch(const WgLoopArgs& a, CouplePath path, int rmax, hipStream_t s);

}  // namespace aoadmm
