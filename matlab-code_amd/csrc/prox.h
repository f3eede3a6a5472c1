// The proximal operator catalogue (functions/constraints_to_prox.m:13-91): prox.hip, and iso.hip for the isotonic /
// unimodal projections and the parallel graph-Laplacian solve.
#pragma once
#include <vector>
#include "common.h"
#include "small.h"
#include "loopctl.h"

namespace aoadmm {

struct ProxSpec {
  int type = AOADMM_C_NONE;
  double p0 = 0.0, p1 = 0.0;       // constraint parameters (eta | l,u | nn)
  // AOADMM_C_QUADRATIC only (device pointers, see QuadPrep): L = U diag(w) U'
  const double* Lmat = nullptr;
  const double* LU = nullptr;
  const double* LUt = nullptr;
  const double* Lw = nullptr;
  struct QuadPrep* quad = nullptr; // non-symmetric L: the prox refreshes (2*eta/rho*L + I)^-1 through it when rho moved
};

// 'quadratic regularization' (constraints_to_prox.m:62-67): prox(x,rho) = (2*eta/rho*L + I) \ x with a fixed
// user matrix L.  rho changes every outer iteration, L does not: L is diagonalised once on the host
// (symmetric L required) and the prox becomes U * diag(1/(2*eta/rho*w_i + 1)) * U' * x, two small GEMMs.
// A non-symmetric L has no orthogonal eigenbasis: whenever 2*eta/rho may have moved (once per outer iteration: rho is
// fixed inside an inner loop; the engine sets `dirty`) the prox inverts 2*eta/rho*L + I ON THE DEVICE by Gauss-Jordan
// elimination with row pivoting (what MATLAB's `\` pivots on; prox.hip quad_gj_step_k, rho read from device memory, no
// host synchronisation) and is then one small GEMM.  The reference factorises the same matrix in EVERY prox call.
struct QuadPrep {
  DevBuf L, U, Ut, w;
  DevBuf Minv, Mwork, piv, pval;   // non-symmetric L: the two buffers the elimination alternates between, pivot rows, pivot value
  bool nonsym = false;
  bool dirty = true;               // the cached inverse may belong to another rho
  const double* key_rho = nullptr; // what the cached inverse was built for
  double key_mul = 0.0, key_eta = 0.0;
  const double* result = nullptr;
  int64_t n = 0;
  void build(const double* L_host, int64_t rows, hipStream_t s);
  void attach(ProxSpec& ps) {
    ps.Lmat = L.d(); ps.LU = U.d(); ps.LUt = Ut.d(); ps.Lw = w.d();
    ps.quad = nonsym ? this : nullptr;
  }
  // (g*L + I)^-1 for g = 2*eta/(rho*rho_mul), column-major n x n on the device; rebuilt when dirty or asked for another rho
  const double* refresh(double eta, const double* rho_dev, double rho_mul, hipStream_t s);
};

// iso.hip: workgroup-parallel isotonic / unimodal projections and the path-Laplacian smoothness prox
// mode 0: non-decreasing, 1: non-increasing, 2: unimodal (nonneg != 0: with projection onto x >= 0)
size_t iso_ws_bytes(int64_t rows, int R);
void prox_iso(const double* V, int64_t ldv, double* Z, int64_t ldz, int64_t rows, int R, int mode, double nonneg,
              double* ws, const AdmmCtl* ctl, hipStream_t s);
// beyond 4096 rows the reduction runs in `ws` (prox_gl_ws_doubles); false: no workspace (the caller solves sequentially)
bool prox_gl_pcr(const double* V, int64_t ldv, double* Z, int64_t ldz, int64_t rows, int R, double eta, const double* rho,
                 double rho_mul, const AdmmCtl* ctl, hipStream_t s, double* ws = nullptr);
size_t prox_gl_ws_doubles(int64_t rows, int R);

bool prox_is_fusable(int type);   // element-wise or row-wise: folded into the primal kernel
// constraints with a reg_func entry (constraints_to_prox.m): their value enters f_tensors (cmtf_fun_AOADMM.m:1272-1288)
inline bool prox_has_reg_value(int t) {
  return t == AOADMM_C_L1_REG || t == AOADMM_C_L0_REG || t == AOADMM_C_L2_REG || t == AOADMM_C_RIDGE ||
         t == AOADMM_C_GL_SMOOTH || t == AOADMM_C_TV || t == AOADMM_C_QUADRATIC;
}
size_t prox_ws_bytes(int type, int64_t rows, int R);

// Z_out = prox(V, rho) for any catalogue entry; rho read from device memory.
void prox_apply(const ProxSpec& ps, const double* V, int64_t ldv, double* Zout, int64_t ldz,
                int64_t rows, int R, const double* rho_dev, double rho_mul, double* ws,
                const AdmmCtl* ctl, hipStream_t s, const double* warm = nullptr, int64_t ldw = 0);
// `warm`: optional previous value of the prox output (same shape); only a speed hint (TV warm start)

// The TV prox with the dual update of an ADMM iteration inside (one launch instead of prox + dual kernel): available
// for LDS-resident columns, or with a workspace of prox_ws_bytes() (`have_ws`) for the same arrays in global memory.
bool prox_tv_dual_ok(int type, int64_t rows, bool have_ws);
// V = fac + mu (rows x R, ld = rows).  Z (warm start in, new Z out) and mu are updated in place; part[R][4] receives
// ||fac-Z||^2, ||fac||^2, ||mu||^2, ||Z-Zold||^2 per column.
void prox_tv_dual(const ProxSpec& ps, const double* V, int64_t rows, int R, const double* rho, double* prox_ws,
                  double* Z, double* mu, double* part, const AdmmCtl* ctl, hipStream_t s);

}  // namespace aoadmm
