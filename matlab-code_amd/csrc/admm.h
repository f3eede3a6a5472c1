// ADMM inner-loop kernels (functions/cmtf_fun_AOADMM.m:591-623,1420-1429); the proximal operators they apply are
// declared in prox.h.
#pragma once
#include "common.h"
#include "small.h"
#include "loopctl.h"
#include "prox.h"

namespace aoadmm {

// The whole ADMM_constrained_only loop (:596-622) for a CP mode, enqueued without host synchronisation:
//   element-wise prox, up to 4096 rows and 10 inner iterations : two launches for the whole loop (admm_rows_mfma_k);
//   other fusable prox : one row-parallel kernel per inner iteration (fac, Z, mu, residual partial sums);
//   other prox         : primal kernel -> column/matrix prox kernel -> dual kernel per inner iteration.
// In the per-iteration forms the loop condition is evaluated on the device at the head of each iteration (admm.hip
// admm_continue).  admm_path() below is the one place that chooses.
// `part` holds admm_partials(rows) * 4 doubles; `V`,`Znew` are rows*R scratch (non-fusable only).
struct AdmmMode {
  const double* A;      // MTTKRP (+bsum term)            rows x R
  const double* L;      // chol factor                     R x R
  const double* Binv = nullptr;   // inv(L*L') when available (well-conditioned ADMM systems)
  const double* rho;    // device scalar
  double *fac, *Z, *mu; // rows x R each
  int64_t rows;
  int R;
  ProxSpec prox;
};
int admm_partials(int64_t rows);
// `deferred_end`: when given, the closing evaluation of the loop is not launched; the caller hands the
// record to the next kernel it runs anyway (atb_small's `close`).
// `gf` (optional): when the loop takes the two-launch row-local path its second launch also leaves the partial Gram
// matrices of the new factor in gf->ws ([nb][R*R], nb returned) and the row-major copy in gf->At; the caller finishes
// with atb_fin.  gf->nb stays 0 when the path was not taken.
struct GramFold {
  double* ws = nullptr;
  double* At = nullptr;
  int nb = 0;
};
// Which kernels run the loop of one constrained CP mode.  Decided from the inputs alone, in one place: admm_mode_update
// and admm_constrained_loop branch on admm_path(); the solver and the op-level entry (capi.hip aoadmm_op_admm_mode) call
// admm_mode_update and only report what it returns.  The values are part of the C ABI (include/aoadmm_hip.h
// AOADMM_PATH_*).
enum AdmmPath {
  kAdmmPathWg = 0,          // admm_loop_wg_k: the whole loop in one workgroup (admm_loop_wg)
  kAdmmPathMfma = 1,        // admm_rows_mfma_k: the two-launch speculative loop
  kAdmmPathRowsFused = 2,   // admm_rows_k with the element-/row-wise prox inside
  kAdmmPathRowsColProx = 3, // admm_rows_k -> prox_apply -> dual_update_k
  kAdmmPathRowsTv = 4,      // admm_rows_k -> TV prox with the dual update inside
  kAdmmPathRowL = 5         // admm_rowL_k: triangular solves, for callers without inv(L*L')
};
// `have_binv`: inv(L*L') is available (the solver always has it for a constrained mode); `have_prox_ws`: a prox
// workspace of prox_ws_bytes() is passed.
AdmmPath admm_path(int64_t rows, int R, int ptype, int max_inner, bool have_binv, bool have_prox_ws);
// Runs every path but kAdmmPathWg (that one has its own entry below and leaves Gram matrix and row-major copy itself).
void admm_constrained_loop(const AdmmMode& m, double* part, double* V, double* Znew, double* prox_ws,
                           AdmmCtl* ctl, int max_inner, double tol_pr, double tol_du, hipStream_t s,
                           LoopEnd* deferred_end = nullptr, GramFold* gf = nullptr);

// One-workgroup form of the same loop for short modes (admm.hip admm_loop_wg_k): rows <= 256 and R <= 16; element-/row-wise
// prox or the column-norm family.  One launch for the loop, the Gram matrix and the
// row-major copy of the new factor.
struct WgLoopU {
  const double* A;          // right-hand side, rows x R column-major (ld = rows)
  const double* Binv;       // inv(L*L'), R x R (shared system; unused with per_row)
  const double* L;          // with per_row: the rows' Cholesky factors, [rows][R*R]
  const double* rho;        // device scalar, or one value per row with per_row
  const double* rho_prox;   // device scalar the prox sees (max(rho) for a PARAFAC2 C mode, :1423-1424); null with
                            // per_row: the kernel takes the maximum of the rows' rho itself
  double *fac, *Z, *mu;     // rows x R each
  int64_t rows;
  int R;
  int per_row;              // 1: row k has its own system L_k and rho_k (:602-606)
  int ptype;
  double p0, p1;
  int max_inner;
  double tol_pr, tol_du;
  AdmmCtl* ctl;             // active != 0 on entry; receives iters, res[1], res[3], active = 0
  int reset = 0;            // 1: run whatever ctl holds (the caller would otherwise launch ctl_reset first)
  double* gram;             // out: fac'*fac (R x R), or null
  double* facT;             // out: row-major copy of fac (rows x R), or null
};
bool admm_loop_wg_ok(int64_t rows, int R, int ptype, int max_inner);
void admm_loop_wg(const WgLoopU& a, hipStream_t s);

// One constrained CP mode's update from the system on, as the solver runs it: the loop on the path admm_path() names
// (admm_loop_wg or admm_constrained_loop), then whatever that path still owes.  Every path leaves fac'*fac in `gram`
// (R x R) and the row-major copy of fac in `facT` (rows x R) and has closed the loop in `ctl`.  `gram_ws` holds
// admm_mode_ws_bytes(); `part`, `V`, `Znew`, `prox_ws` as for admm_constrained_loop.  Returns the path taken.
size_t admm_mode_ws_bytes(int64_t rows, int R);
AdmmPath admm_mode_update(const AdmmMode& m, double* part, double* V, double* Znew, double* prox_ws,
                          double* gram, double* facT, double* gram_ws,
                          AdmmCtl* ctl, int max_inner, double tol_pr, double tol_du, hipStream_t s);

// generic pieces for the coupled / PARAFAC2 loops -------------------------------
// (Z,mu) <- update_constraint (:1420-1429): Zold kept in `Zold`; slots[0..3] receive
// ||fac-Z||^2, ||fac||^2, ||mu||^2, ||Z-Zold||^2
void constraint_update(const ProxSpec& ps, const double* fac, double* Z, double* mu, double* Zold,
                       double* V, int64_t rows, int R, const double* rho_dev, double rho_mul,
                       double* prox_ws, double* slots, double* red_ws, const AdmmCtl* ctl,
                       hipStream_t s);

// residual bookkeeping at the end of a generic inner iteration; per participating mode a block of
// 8 slots: [0]=||fac-Z||^2 [1]=||fac||^2 [2]=||mu||^2 [3]=||Z-Zold||^2
//          [4]=||Tf(fac)-Sd(Delta)||^2 [5]=||mu_Delta||^2 [6]=||Sd(Delta-Delta_old)||^2
//          [7]=denominator of the primal coupling residual (||fac||^2, or ||Tf(fac)||^2 for types 1, 2)
struct FinalizeArgs {
  const double* slots[8];
  int constrained[8];
  int coupled[8];
  int nmodes;
  int max_inner;
  double tol_pr_coupl, tol_pr_constr, tol_du_coupl, tol_du_constr;
};
void admm_finalize_generic(const FinalizeArgs& fa, AdmmCtl* ctl, hipStream_t s);

}  // namespace aoadmm
