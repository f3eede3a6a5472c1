// PARAFAC2 slab kernels (functions/cmtf_fun_AOADMM.m:157-250 block updates, :509-589 ADMM_B_Parafac2,
// :1247-1268 / :1351-1362 objective pieces).  A PARAFAC2 block is K slabs X_k (I x J_k, ragged J_k);
// slabs are stored back to back, slab k at element offset I*off[k] (column-major I x J_k); slab-valued
// factors (B_k, P_k, mu_k, Z_k ...) are stored back to back too, slab k at off[k]*R (column-major J_k x R).
// All kernels run one workgroup per slab; sizes are small (cfg4: I=40, J_k<=120, R=3, K=256), so these
// are latency-bound and plain fp64 VALU code.
#pragma once
#include <functional>

#include "admm.h"
#include "common.h"
#include "small.h"

namespace aoadmm {

struct P2Dims {
  int K, I, R;
  const int64_t* off;   // device, K+1 prefix sums of J_k
  const int64_t* off_h; // the same on the host
  int64_t Jtot;
  int Jmax;
  int k0, k1;           // slabs this rank works on: [k0, k1) = [0, K) unless the block is slab-sharded
};
// all-reduce hook for slab-sharded blocks (Engine::allreduce on the library's stream)
using P2AllReduce = std::function<void(double*, int64_t)>;

// T1[k] = X_k * B_k  (I x R each)
void par2_xkb(const double* X, const double* B, const P2Dims& d, double* T1, hipStream_t s);
// GB[k] = B_k' * B_k  (R x R each)
void par2_gram(const double* B, const P2Dims& d, double* GB, hipStream_t s);
// Amt(i,r) = sum_k T1[k](i,r)*C(k,r) ; Csys(r,q) = sum_k C(k,r)C(k,q)GB[k](r,q)        (:160-165)
void par2_modeA_combine(const double* T1, const double* Cfac, const double* GB, const P2Dims& d, double* Amt,
                        double* Csys, hipStream_t s);
// Ak = w * X_k' * A * D_k  (J_k x R, concatenated)                                       (:193)
void par2_xta(const double* X, const double* A, const double* Cfac, double w, const P2Dims& d, double* Ak,
              hipStream_t s);
// per slab: C_k = D_k GA D_k, rho_k, B_k = w C_k + rho_k/2 (1+constr) I + ridge + bsum/2, L_k = chol   (:194-212)
void par2_b_system(const double* GA, const double* Cfac, double w, double ridge, double bsum_half, double rho_scale,
                   int nrho, const P2Dims& d, double* rho, double* L, AdmmCtl* ctl, hipStream_t s);

struct P2BArgs {
  const double *Ak, *L, *rho;          // rhs, chol factors [K][R*R], rho[K]
  double *B, *P, *Pold, *mu, *W;       // concatenated J_k x R
  double *DeltaB, *DeltaBold, *part;   // R x R, R x R, [K][R*R]
  const double *Z, *muZ;               // constraint variables (nullable)
  double* norms;                       // [K][8]
  int use_constr;
  // One-sided Jacobi of the polar factor (:532-534), warm start: the rotation the previous inner iteration ended with
  // ([K][R*R], column-major per slab) is applied first, so the sweeps start from almost orthogonal columns.  A speed
  // hint only (any orthogonal start gives the same polar factor).  null: cold start from the identity.
  double* Jrot = nullptr;
  int jrot_valid = 0;                  // 0: Jrot holds nothing yet (first inner iteration): cold start, then store
};
// Which kernels run the B_k loop of a block.  Decided from the inputs alone, in one place: par2_b_loop_folded,
// par2_b_iteration and the op-level entry (capi.hip aoadmm_op_par2_b_loop) all branch on par2_b_path().  The values are
// part of the C ABI (include/aoadmm_hip.h AOADMM_P2SLAB_*).
enum P2SlabKernel {
  kP2SlabRegs1 = 0,   // par2_b_slab_regs_k<1> / par2_b_slab_fold_regs_k<1>: R <= 4, Jmax <= 64
  kP2SlabRegs2 = 1,   // <2>: R <= 4, Jmax <= 128
  kP2SlabRegs4 = 2,   // <4>: R <= 4, Jmax <= 256
  kP2SlabLds4 = 3,    // par2_b_slab_k<4> / par2_b_slab_fold_k<4>: R <= 4, Jmax > 256
  kP2SlabLds8 = 4,    // <8>: R in 5..8
  kP2SlabLds16 = 5,   // par2_b_slab_k<16>: R in 9..16
  kP2SlabLds64 = 6    // par2_b_slab_k<kMaxRank>: R >= 17
};
struct P2BPath {
  int folded;      // 1: two launches per inner iteration (par2_b_loop_folded); 0: four (par2_b_iteration, ...)
  int slab;        // P2SlabKernel
  int in_lds;      // LDS forms: 1 when W_k is staged in LDS, 0 when it is rotated in place (no warm start then)
  int dual_fold;   // folded: the par2_b_dual_fold_k class, 16 or 64; else 0
};
P2BPath par2_b_path(const P2Dims& d, bool constrained, bool sharded);
// one inner iteration of ADMM_B_Parafac2 up to (not including) the constraint update   (:525-547, :582-585)
// psum (R*R+1 doubles) != nullptr: slabs are sharded, DeltaB's sums go through `allreduce`
void par2_b_iteration(const P2BArgs& a, const P2Dims& d, const AdmmCtl* ctl, hipStream_t s, double* psum,
                      const P2AllReduce& allreduce);
// The whole loop without B_k constraints on unsharded slabs, R <= 8 (par2_b_path().folded): two launches per inner
// iteration (the sum over the slabs and the while test ride at the head of the next kernel) and one closing launch; ctl
// must have been reset.
void par2_b_loop_folded(const P2BArgs& a, const P2Dims& d, AdmmCtl* ctl, int max_inner, double tol_pr_coupl,
                        double tol_pr_constr, double tol_du_coupl, double tol_du_constr, hipStream_t s);
constexpr int kTsmoothMaxK = 64;       // tPARAFAC2: each thread keeps the eliminated diagonal of the K x K system
// Z_k = prox(B_k + muZ_k, rho_k) ; muZ_k += B_k - Z_k ; norms[k][4..6] = ||B-Z||^2, ||muZ||^2, ||Z-Zold||^2   (:566-579)
void par2_b_constraint(const ProxSpec& ps, const double* B, double* Z, double* muZ, double* Zold, double* V,
                       const double* rho, const P2Dims& d, double* prox_ws, double* norms, const AdmmCtl* ctl,
                       hipStream_t s);
// residual averages over the slabs + loop condition (:520, :558-585)
void par2_b_finalize(const double* norms, const P2Dims& d, int use_constr, AdmmCtl* ctl, int max_inner,
                     double tol_pr_coupl, double tol_pr_constr, double tol_du_coupl, double tol_du_constr, hipStream_t s,
                     double* part4, const P2AllReduce& allreduce);

// Mode B from the right-hand side on (:194-218): the slab systems (par2_b_system, which opens the loop in ctl), the bsum
// term of the right-hand side (:204-207), ADMM_B_Parafac2 on the path par2_b_path() names, and the Gram matrices of the
// new B_k.  Engine::par2_update_B and aoadmm_op_par2_b_loop both run exactly this.
struct P2BLoop {
  const double *GA, *Cfac;                  // A'A (R x R), C (K x R)
  double w, ridge, bsum_half, rho_scale;    // block weight, ridge, bsum_weight/2 (0 without bsum), increase_factor_rhoBk
  bool bsum = false;
  double* Ak;                               // w X_k' A D_k; with bsum: += bsum_half * B (:204-207)
  double *rho, *L;                          // out: rho_k [K], chol factors [K][R*R]
  P2BArgs a;                                // B, P, Pold, mu, W, DeltaB, DeltaBold, part, norms, Jrot (the rest is filled in)
  bool constrained = false;                 // B_k constraint active in this outer iteration (:209, :527)
  ProxSpec prox;
  double *Z = nullptr, *muZ = nullptr, *Zold = nullptr, *V = nullptr, *prox_ws = nullptr;
  int max_inner;
  double tol_pr_coupl, tol_pr_constr, tol_du_coupl, tol_du_constr;
  double* GB;                               // out: B_k' B_k [K][R*R]
  double *psum = nullptr, *part4 = nullptr; // slabs sharded over ranks: R*R+1 sums of DeltaB, four residual means
  P2AllReduce allreduce;
};
void par2_b_loop(const P2BLoop& g, const P2Dims& d, AdmmCtl* ctl, hipStream_t s);

// mode C: a(k,r) = w * sum_i A(i,r) T1[k](i,r) ; C_k = GA .* GB[k] ; rho_k ; B_k (+rho_k/2 I if constrained) ; chol  (:221-240)
// nrho = how many rho_k/2*I terms the system gets (constraint, exact coupling :262-264); Madd (R x R, optional) enters
// as + rho_k/2*Madd (coupling type 2: H*H', :307); raw = 1: L receives B_k itself
void par2_c_system(const double* A, const double* T1, const double* GA, const double* GB, double w, double ridge,
                   double bsum_half, int nrho, int raw, const P2Dims& d, const double* Cfac, double* a, double* rho,
                   double* L, AdmmCtl* ctl, hipStream_t s, const double* Madd = nullptr);
// Sparse slabs (par2_sparse.h): the data never enters these kernels.
// Csys alone -- the half of par2_modeA_combine that needs no data (:164)
void par2_modeA_csys(const double* Cfac, const double* GB, const P2Dims& d, double* Csys, hipStream_t s);
// par2_c_system with the data term given: a(k,r) = w * sv(k,r) + bsum_half * C(k,r), sv(k,r) = (A' X_k B_k)(r,r) (K x R)
void par2_c_system_pre(const double* sv, const double* GA, const double* GB, double w, double ridge, double bsum_half,
                       int nrho, int raw, const P2Dims& d, const double* Cfac, double* a, double* rho, double* L,
                       AdmmCtl* ctl, hipStream_t s, const double* Madd = nullptr);
// rhomax = max_k rho_k (:1424); separate because a slab-sharded block gathers rho first
void par2_rho_max(const double* rho, int K, double* rhomax, hipStream_t s, double* rhomean = nullptr,
                  double* rhosum = nullptr);
// (K*R) x (K*R) system of a C mode coupled through H*C = Delta (:283-293); HtH = H'*H (K x K), rhoC = mean(rho) on the device
// the same system when H'H = diag(d): K independent row systems, L (holding B_k) is overwritten by chol(B_k + rhoC/2*(d_k [+1])*I)
void par2_c_rowsys_diag(double* L, const double* d, const double* rhoC, int constrained, int K, int R, AdmmCtl* ctl,
                        hipStream_t s);
void par2_c_big_system(const double* Bk, const double* HtH, const double* rhoC, int constrained, int K, int R, double* M,
                       hipStream_t s);
// row k: rhs = a_k (+ rho_k/2 (Z(k,:) - mu(k,:))) ; C(k,:) = L_k'\(L_k\rhs)      (:236, :604-605)
void par2_c_rowsolve(const double* a, const double* rho, const double* L, const double* Z, const double* mu,
                     int use_admm, const P2Dims& d, double* Cfac, const AdmmCtl* ctl, hipStream_t s);

// The steps of a dense block outside the B_k loop, each written once: Engine::par2_prepare_modeA / par2_update_C /
// par2_prepare_C_coupled / par2_objective_enqueue and the op-level entries (capi.hip aoadmm_op_par2_mode_a / _mode_c /
// _objective) run exactly these.
// Tile width `ew` par2_modeA_combine launches with for this block, and par2_modeA_csys for this rank
int par2_modeA_tile_width(const P2Dims& d);
int par2_modeA_csys_tile_width(const P2Dims& d);
// mode A from dense slabs (:160-165): T1 = X_k B_k, then Amt and Csys (par2_xkb, par2_modeA_combine)
void par2_mode_a(const double* X, const double* B, const double* Cfac, const double* GB, const P2Dims& d, double* T1,
                 double* Amt, double* Csys, hipStream_t s);

// mode C from dense slabs, up to the systems (:219-240, coupled :260-312): T1 = X_k B_k, then par2_c_system
struct P2CSys {
  const double *X, *A, *B, *GA, *GB, *Cfac;   // slabs, A (I x R), B_k, A'A, B_k'B_k [K][R*R], C (K x R)
  double w, ridge, bsum_half;
  int nrho = 0, raw = 0;                      // see par2_c_system
  const double* Madd = nullptr;
  double *T1, *a, *rho, *L;                   // out: [K][I*R], K x R, K, [K][R*R]
};
void par2_c_systems(const P2CSys& g, const P2Dims& d, AdmmCtl* ctl, hipStream_t s);
// What par2_c_system builds for a C mode inside a coupling of type `ctype` (:260-267, :305-312, :282-297): per-row
// factors with nrho = 1 + constrained (types 0, 3, 4), the same with Madd = H*H' and nrho = constrained (type 2), or
// the raw B_k for the (K*R)-system of types 1 and 5
struct P2CCoupledKind { int nrho, raw, madd; };
P2CCoupledKind par2_c_coupled_kind(int ctype, int constrained);
// types 1, 5 behind the raw B_k: K row systems when H'H is diagonal (HtH holds the K diagonal entries, L is factored in
// place), else the dense (K*R) x (K*R) system M from HtH (K x K)
void par2_c_coupled_big(double* L, const double* HtH, bool hth_diag, const double* rhoC, int constrained, int K, int R,
                        double* M, AdmmCtl* ctl, hipStream_t s);

// Which form the uncoupled C update takes.  Decided from the inputs alone, in one place (par2_c_path); the values are
// part of the C ABI (include/aoadmm_hip.h AOADMM_P2C_*).
enum P2CPath {
  kP2CSingle = 0,     // unconstrained: one par2_c_rowsolve (:236)
  kP2CWgLoop = 1,     // admm_loop_wg_k<RM, 256, 2>: K <= 256 rows, R <= 16, element-/row-wise or column-norm prox
  kP2CLaunched = 2    // par2_c_rowsolve + constraint_update + admm_finalize_generic per inner iteration
};
P2CPath par2_c_path(int K, int R, bool constrained, int ptype, int max_inner);
int par2_c_rowsolve_class(int R);             // RMAX of par2_c_rowsolve_k: 4, 8, 16 or kMaxRank
// The uncoupled C update behind the systems (:236, :602-606 with max(rho) in the prox, :1423-1424)
struct P2CSolve {
  const double *a, *rho, *L;                  // K x R, K, [K][R*R]
  double *fac, *Z = nullptr, *mu = nullptr;   // K x R each
  bool constrained = false;
  ProxSpec prox;
  int max_inner;
  double tol_pr, tol_du;                      // innerRelPrTol_constr, innerRelDualTol_constr
  double* rhomax;                             // device scalar (written unless the one-workgroup loop runs)
  double *Zold = nullptr, *V = nullptr, *prox_ws = nullptr;   // launched loop: K x R, K x R, prox_ws_bytes
  double *slots = nullptr, *red_ws = nullptr;                 // launched loop: 8 residual slots, 4096 doubles
};
P2CPath par2_c_solve(const P2CSolve& g, const P2Dims& dall, AdmmCtl* ctl, hipStream_t s);

// objective pieces of a block (:1262-1264, :1355, :1337, :1279-1281): par2_residual (X != nullptr), par2_b_gaps,
// par2_reg_values (reg_type with a reg_func value, else AOADMM_C_NONE)
struct P2Objective {
  const double *X, *A, *B, *Cfac, *P, *DeltaB, *Z;   // Z nullable
  int reg_type = AOADMM_C_NONE;
  double eta = 0.0;
  double *res, *q, *regv;                     // out: K, [K][4], K
};
void par2_objective(const P2Objective& g, const P2Dims& d, hipStream_t s);

// res[k] = ||X_k - A D_k B_k'||_F^2                                                       (:1262-1264)
void par2_residual(const double* X, const double* A, const double* B, const double* Cfac, const P2Dims& d,
                   double* res, hipStream_t s);
// regv[k] = reg_func(B_k) of a regularisation-type constraint on the B_k mode            (:1279-1281)
void par2_reg_values(const double* B, int type, double eta, const P2Dims& d, double* regv, hipStream_t s);
// q[k][0..3] = ||B_k - P_k DeltaB||^2, ||B_k||^2, ||B_k - Z_k||^2 (Z nullable), ||B_k - B_{k-1}||^2 (0 for k = 0 and for
// neighbours of different size; t_smoothness_penalty.m)                                  (:1355, :1337)
void par2_b_gaps(const double* B, const double* P, const double* DeltaB, const double* Z, const P2Dims& d,
                 double* q, hipStream_t s);

// out[0] = 1 if any of the three loop-control records carries the not-positive-definite flag
void par2_collect_notpd(const AdmmCtl* a, const AdmmCtl* b, const AdmmCtl* c, double* out, hipStream_t s);

}  // namespace aoadmm
