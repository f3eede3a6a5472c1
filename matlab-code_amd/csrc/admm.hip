// ADMM inner loops on gfx950; the proximal operators they call live in prox.hip / iso.hip (prox.h).
// Reference: functions/cmtf_fun_AOADMM.m:591-623 (ADMM_constrained_only), :1420-1429
// (update_constraint), :1079-1096 (eval_res_ADMM_constr).
#include <type_traits>

#include "admm.h"
#include "device_utils.h"
#include "loopctl.h"
#include "prox_dev.h"

namespace aoadmm {

// ===========================================================================
// fused primal (+ dual) step, thread per row
// ===========================================================================
template <int RMAX>
__device__ __forceinline__ void row_solve_regs2(double (&x)[RMAX], const double* Lsh, int R) {
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
    if (j < R) {
      double v = x[j];
#pragma unroll
      for (int q = 0; q < j; ++q) v -= Lsh[j + R * q] * x[q];
      x[j] = v / Lsh[j + R * j];
    }
  }
#pragma unroll
  for (int j = RMAX - 1; j >= 0; --j) {
    if (j < R) {
      double v = x[j];
#pragma unroll
      for (int q = j + 1; q < RMAX; ++q)
        if (q < R) v -= Lsh[q + R * j] * x[q];
      x[j] = v / Lsh[j + R * j];
    }
  }
}

// ---------------------------------------------------------------------------
// Loop control without a kernel of its own.  The residuals of inner iteration k-1 are four sums that
// iteration k-1 leaves as per-block partials in part[(k-1)&1]; the first thing every block of iteration
// k's first kernel does is add them up (same data, same order => same decision in every block) and
// evaluate eval_res_ADMM_constr (:1079-1096) + the while condition (:600).  Block 0 records the
// outcome in ctl.  The later kernels of iteration k only look at ctl->active.
// ---------------------------------------------------------------------------
static constexpr int kRowThreads = 64;

struct FusedArgs {
  const double *A, *L, *rho, *Binv;
  double *fac, *Z, *mu, *V, *part;
  AdmmCtl* ctl;
  int64_t rows;
  int R, fused, ptype;
  int it, max_inner, nparts_prev;
  double p0, p1, tol_pr, tol_du;
};

// One inner iteration of ADMM_constrained_only for 64 rows per 256-thread block: wave w owns output
// columns [w*CPW, (w+1)*CPW) of those rows (lane = row), so the per-row solve fac = A_inner*inv(L*L')
// is spread over four waves and no thread carries more than R + 5*CPW operands in registers.
// A_inner (:608) is exchanged through LDS, inv(L*L') is broadcast from LDS.  With an element-/row-wise
// prox the kernel also does update_constraint (:1420-1429) and the residual partial sums; otherwise it
// writes fac and V = fac + mu for the column prox kernel.
// The kernel is latency-bound (2000 x 20 operands): every global load it needs -- operands, system
// matrix, the previous iteration's partial sums -- is issued in ONE round trip before the loop decision.
static constexpr int kRowBlock = 256;
template <int CPW, bool EXACT>
__global__ __launch_bounds__(kRowBlock) void admm_rows_k(FusedArgs a) {
  constexpr int RMAX = 4 * CPW;
  extern __shared__ double lds[];                   // Binv[R*R] | rhs[64][RP] | red[4][4]
  const int R = EXACT ? RMAX : a.R;
  const int RP = R | 1;
  double* Bsh = lds;
  double* rsh = lds + R * R;
  double* red = rsh + 64 * RP;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t stride = (int64_t)gridDim.x * 64;
  int64_t i = (int64_t)blockIdx.x * 64 + lane;
  bool have = i < a.rows;
  // loads are unconditional on clamped (always valid) addresses: no exec-mask branches in the prologue,
  // values of padding lanes / padding columns are never stored
  double av[CPW], mu[CPW], zo[CPW];
#pragma unroll
  for (int k = 0; k < CPW; ++k) {
    const int c = w * CPW + k;
    const int64_t o = (have ? i : a.rows - 1) + a.rows * (c < R ? c : 0);
    zo[k] = a.Z[o]; mu[k] = a.mu[o]; av[k] = a.A[o];
  }
  constexpr int NL = (RMAX * RMAX + kRowBlock - 1) / kRowBlock;
  double lb[NL];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int e = t + kRowBlock * k;
    lb[k] = a.Binv[e < R * R ? e : 0];
  }
  const double rho = a.rho[0];
  const bool go = admm_continue(a.part + (int64_t)((a.it + 1) & 1) * kMaxParts * 4, a.nparts_prev, a.it, a.max_inner,
                                a.tol_pr, a.tol_du, a.ctl, blockIdx.x == 0 && t == 0);
  if (!go) return;                                  // block-uniform
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int e = t + kRowBlock * k;
    if (e < R * R) Bsh[e] = lb[k];
  }
  const double rh = rho / 2;
  const ElemProx ep = elem_prox_of(a.ptype, a.p0, a.p1, rho);
  double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (;;) {
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
      const int c = w * CPW + k;
      if (c < R) rsh[lane * RP + c] = av[k] + rh * (zo[k] - mu[k]);       // A_inner = A + rho/2*(Z - mu)   (:608)
    }
    __syncthreads();
    double rhs[RMAX];
#pragma unroll
    for (int q = 0; q < RMAX; ++q) rhs[q] = q < R ? rsh[lane * RP + q] : 0.0;
    double x[CPW];
#pragma unroll
    for (int k = 0; k < CPW; ++k) {                  // fac = A_inner * inv(L*L')       (:609)
      const int c = w * CPW + k;
      double acc = 0.0;
      if (c < R) {
#pragma unroll
        for (int q = 0; q < RMAX; ++q)
          if (q < R) acc += rhs[q] * Bsh[q + R * c];
      }
      x[k] = acc;
    }
    if (a.fused) {
      double z[CPW];
#pragma unroll
      for (int k = 0; k < CPW; ++k) z[k] = x[k] + mu[k];
      if (a.ptype == AOADMM_C_SIMPLEX_ROW) {
        // the projection needs the whole row: exchange fac + mu through LDS, every thread of a row finds
        // the same threshold (exact nested-active-set iteration) and applies it to its own columns
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CPW; ++k) {
          const int c = w * CPW + k;
          if (c < R) rsh[lane * RP + c] = z[k];
        }
        __syncthreads();
        double v[RMAX];
#pragma unroll
        for (int q = 0; q < RMAX; ++q) v[q] = q < R ? rsh[lane * RP + q] : 0.0;
        simplex_regs<RMAX>(v, R, a.p0);
#pragma unroll
        for (int k = 0; k < CPW; ++k) {
          const int c = w * CPW + k;
          z[k] = 0.0;
#pragma unroll
          for (int q = 0; q < RMAX; ++q)
            if (q == c) z[k] = v[q];
        }
      } else {
#pragma unroll
        for (int k = 0; k < CPW; ++k) z[k] = elem_prox(ep, z[k]);
      }
      if (have) {
#pragma unroll
        for (int k = 0; k < CPW; ++k) {
          const int c = w * CPW + k;
          if (c < R) {
            const int64_t o = i + a.rows * c;
            const double mn = mu[k] + x[k] - z[k];     // mu = mu + fac - Z              (:1428)
            a.fac[o] = x[k];
            a.Z[o] = z[k];
            a.mu[o] = mn;
            const double d = x[k] - z[k];
            s1 += d * d;
            s2 += x[k] * x[k];
            s3 += mn * mn;
            const double e = z[k] - zo[k];
            s4 += e * e;
          }
        }
      }
    } else if (have) {
#pragma unroll
      for (int k = 0; k < CPW; ++k) {
        const int c = w * CPW + k;
        if (c < R) {
          const int64_t o = i + a.rows * c;
          a.fac[o] = x[k];
          a.V[o] = x[k] + mu[k];
        }
      }
    }
    i += stride;
    if (i - lane >= a.rows) break;                    // block-uniform
    have = i < a.rows;
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
      const int c = w * CPW + k;
      const int64_t o = (have ? i : a.rows - 1) + a.rows * (c < R ? c : 0);
      zo[k] = a.Z[o]; mu[k] = a.mu[o]; av[k] = a.A[o];
    }
    __syncthreads();                                  // rsh is rewritten at the top of the loop
  }
  if (a.fused) {
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);   // fixed-order DPP tree
    if (lane == 0) { red[w * 4 + 0] = s1; red[w * 4 + 1] = s2; red[w * 4 + 2] = s3; red[w * 4 + 3] = s4; }
    __syncthreads();
    if (t < 4) {
      a.part[((int64_t)(a.it & 1) * kMaxParts + blockIdx.x) * 4 + t] = red[t] + red[4 + t] + red[8 + t] + red[12 + t];
    }
  }
}

// ---------------------------------------------------------------------------
// The whole inner loop of an element-wise-prox mode in TWO launches instead of MaxInnerIters, on the matrix cores.
// With an element-wise prox every row of (fac, Z, mu) evolves on its own; only the residual test of the while
// condition (:600) couples the rows.  Pass 1 (FINAL = false) runs all MaxInnerIters iterations for its 64 rows in
// registers and stores nothing but the four residual partial sums of every iteration.  Pass 2 (FINAL = true) adds
// the partial sums up (same data, same order in every block: same decision everywhere), finds the iteration k* after
// which the reference loop stops, repeats exactly k* iterations -- the same instructions on the same operands, hence
// the same bits -- and stores fac, Z, mu.  Block 0 records k* and the residuals of iteration k* in ctl.  Pass 2 also
// leaves what the Gram kernel would compute next: the block's partial Gram matrix F_b'F_b and the row-major copy of
// its rows of the factor (the caller adds the partials with atb_fin).
//
// The row solve fac = A_inner * inv(L*L') (:609) is computed transposed, fac' = Binv * A_inner' (Binv is symmetric),
// with v_mfma_f64_16x16x4_f64: a wave owns 16 rows; lane (r = l&15, q = l>>4) supplies B[k = 4s+q][n = r] =
// A_inner(row r, column 4s+q) and receives D[m = q+4i (+16mt)][n = r] = fac(row r, column 4(4mt+i)+q) -- the SAME
// columns {4s+q} it supplies.  So a lane keeps A, Z, mu, fac of its row for the columns c = q (mod 4) in registers
// for the whole loop and the element-wise prox and dual update are lane-local: no LDS exchange, no barrier inside
// an iteration (the VALU form staged A_inner through LDS and read 20 + 100 LDS words per thread and iteration:
// ~4 us per iteration at 2000 x 20 against ~0.4 us here).
struct SpecExtra {
  double* gram_ws;      // [gridDim.x][R*R] partial Gram matrices (FINAL only; may be null)
  double* At;           // rows x R row-major copy of fac (FINAL only; may be null)
};
typedef double f64x4_t __attribute__((ext_vector_type(4)));
static constexpr int kSpecMaxInner = 10;      // beyond this the work thrown away after an early exit could matter
static constexpr int kSpecThreads = 64;       // one wave = 16 rows per workgroup: no barrier anywhere in the kernel
static constexpr int kSpecPartJ = 4;          // a lane adds up to 4 partial sums per iteration: <= 256 workgroups
template <int KS, bool FINAL>
__global__ __launch_bounds__(kSpecThreads) void admm_rows_mfma_k(FusedArgs a, SpecExtra ex) {
  constexpr int MT = (KS + 3) / 4;
  extern __shared__ double rsh[];                   // FINAL: [16][RP] tile of the new factor for the Gram partial
  const int R = a.R;
  const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
  const int64_t i = (int64_t)blockIdx.x * 16 + r;
  const bool have = i < a.rows;
  const int nparts = gridDim.x;
  double av[KS], mu[KS], zo[KS], x[KS], bi[MT][KS];
  // every global load of the kernel in one round trip, on clamped (always valid) addresses
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int c = 4 * s + q;
    const int64_t o = (have ? i : a.rows - 1) + a.rows * (c < R ? c : 0);
    zo[s] = a.Z[o]; mu[s] = a.mu[o]; av[s] = a.A[o];
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int m = 16 * mt + r, k = 4 * s + q;
      bi[mt][s] = a.Binv[(m < R ? m : 0) + R * (k < R ? k : 0)];
    }
  const double rho = a.rho[0];
  int niter = a.max_inner;
  if (FINAL) {
    // k*: the first iteration whose residuals end the loop (eval_res_ADMM_constr :1079-1096, while condition :600).
    // Branch-free loads (clamped indices, masked adds) so that all of them are in flight together.
    double S[kSpecMaxInner][4];
#pragma unroll
    for (int it = 0; it < kSpecMaxInner; ++it) {
      const int itc = it < a.max_inner ? it : a.max_inner - 1;
      double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
      for (int j = 0; j < kSpecPartJ; ++j) {
        const int b = lane + 64 * j;
        const bool ok = b < nparts;
        const f64x4_t v = *reinterpret_cast<const f64x4_t*>(a.part + ((int64_t)itc * nparts + (ok ? b : 0)) * 4);
        s0 += ok ? v[0] : 0.0; s1 += ok ? v[1] : 0.0; s2 += ok ? v[2] : 0.0; s3 += ok ? v[3] : 0.0;
      }
      S[it][0] = s0; S[it][1] = s1; S[it][2] = s2; S[it][3] = s3;
    }
    double pr = 0.0, du = 0.0;
    int ks = a.max_inner;
    bool found = false;
#pragma unroll
    for (int it = 1; it <= kSpecMaxInner; ++it) {    // (no early break: with one the array S went to scratch memory)
      double s0 = S[it - 1][0], s1 = S[it - 1][1], s2 = S[it - 1][2], s3 = S[it - 1][3];
      s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);   // the same total in every lane
      if (!found && it <= a.max_inner) {
        pr = sqrt(s0) / sqrt(s1);                                            // :1085
        const double sc = sqrt(s2);
        du = sc > 0 ? sqrt(s3) / sc : sqrt(s3);                              // :1087-1092
        if (!(it < a.max_inner && (pr > a.tol_pr || du > a.tol_du))) { ks = it; found = true; }
      }
    }
    niter = ks;
    if (blockIdx.x == 0 && lane == 0) {
      a.ctl->res[1] = pr;
      a.ctl->res[3] = du;
      a.ctl->iters = ks;
      a.ctl->active = 0;
    }
  }
  // padding columns (4s+q >= R) and padding rows of Binv carry zeros: they add nothing to the products
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (4 * s + q >= R) { av[s] = 0.0; zo[s] = 0.0; mu[s] = 0.0; }
    x[s] = 0.0;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      if (16 * mt + r >= R || 4 * s + q >= R) bi[mt][s] = 0.0;
  }
  const double rh = rho / 2;
  const ElemProx ep = elem_prox_of(a.ptype, a.p0, a.p1, rho);
  for (int it = 0; it < niter; ++it) {
    double ain[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) ain[s] = av[s] + rh * (zo[s] - mu[s]);       // A_inner = A + rho/2*(Z - mu)   (:608)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {                                          // fac = A_inner * inv(L*L')       (:609)
      f64x4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(bi[mt][s], ain[s], acc, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * mt + e < KS) x[4 * mt + e] = acc[e];
    }
    double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const double z = elem_prox(ep, x[s] + mu[s]);                            // Z = prox(fac + mu)              (:1425)
      const double mn = mu[s] + x[s] - z;                                      // mu = mu + fac - Z               (:1428)
      if (have && 4 * s + q < R) {
        const double d = x[s] - z;
        s1 += d * d;
        s2 += x[s] * x[s];
        s3 += mn * mn;
        const double e = z - zo[s];
        s4 += e * e;
        mu[s] = mn;
        zo[s] = z;
      }
    }
    if (!FINAL) {
      s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);   // fixed-order DPP tree
      if (lane == 0) {
        f64x4_t v = {s1, s2, s3, s4};
        *reinterpret_cast<f64x4_t*>(a.part + ((int64_t)it * nparts + blockIdx.x) * 4) = v;
      }
    }
  }
  if (!FINAL) return;
  if (have) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int c = 4 * s + q;
      if (c < R) {
        const int64_t o = i + a.rows * c;
        a.fac[o] = x[s];
        a.Z[o] = zo[s];
        a.mu[o] = mu[s];
      }
    }
  }
  if (ex.gram_ws == nullptr) return;
  // Row-major copy of the wave's 16 rows and their partial Gram matrix G_b = F_b'F_b (what atb_part_k would do
  // next).  The tile goes through the wave's LDS (a wave's LDS operations complete in order: no barrier); the Gram
  // partial is MFMA work as well: D[m][n] = sum_k F(k, m) F(k, n) with the 16 rows as the reduction index.
  const int RP = R | 1;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int c = 4 * s + q;
    if (c < R) rsh[r * RP + c] = have ? x[s] : 0.0;
  }
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int nr = (int)((a.rows - r0 < 16) ? (a.rows - r0) : 16);
  if (ex.At)
    for (int e = lane; e < nr * R; e += kSpecThreads) {
      const int ii = e / R, k = e - ii * R;
      ex.At[(r0 + ii) * R + k] = rsh[ii * RP + k];
    }
  double fo[MT][4];                                   // F(row 4s + q, column 16mt + r), s = 0..3
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = 16 * mt + r;
      fo[mt][s] = c < R ? rsh[(4 * s + q) * RP + c] : 0.0;
    }
  double* G = ex.gram_ws + (int64_t)blockIdx.x * R * R;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < MT; ++nt) {
      f64x4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fo[mt][s], fo[nt][s], acc, 0, 0, 0);
      const int n = 16 * nt + r;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = 16 * mt + q + 4 * e;
        if (m < R && n < R) G[m + R * n] = acc[e];
      }
    }
}

// (A one-launch form of this loop -- the workgroups meeting at a grid barrier instead of a kernel boundary, the result of
// pass 1 kept in registers when the loop ran to its cap -- was built and measured in round 3: 735 GPU tests green, but no
// faster: 1.279 against 1.274 ms per iteration at one rank's share of 8 GPUs, 7.92 against 7.94 ms at one GPU.  The
// workgroups sit on eight dies with separate L2s; an agent-scope barrier (release fence = L2 write-back, atomics and
// acquire loads that go past the L2) costs about what the kernel boundary costs, ~10 us.  Not kept.)
// Thread-per-row variant for the triangular-solve path (no explicit inverse available: op-level entry)
template <int RMAX>
__global__ __launch_bounds__(kRowThreads) void admm_rowL_k(FusedArgs a) {
  extern __shared__ double Lsh[];
  const int R = a.R;
  for (int e = threadIdx.x; e < R * R; e += kRowThreads) Lsh[e] = a.L[e];
  const double rho = a.rho[0];
  const bool go = admm_continue(a.part + (int64_t)((a.it + 1) & 1) * kMaxParts * 4, a.nparts_prev, a.it, a.max_inner,
                                a.tol_pr, a.tol_du, a.ctl, blockIdx.x == 0 && threadIdx.x == 0);
  if (!go) return;
  __syncthreads();
  const double rh = rho / 2;
  const ElemProx ep = elem_prox_of(a.ptype, a.p0, a.p1, rho);
  double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < a.rows; i += (int64_t)gridDim.x * kRowThreads) {
    double x[RMAX], mu[RMAX], zo[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      x[r] = 0; mu[r] = 0; zo[r] = 0;
      if (r < R) {
        const int64_t o = i + a.rows * r;
        zo[r] = a.Z[o];
        mu[r] = a.mu[o];
        x[r] = a.A[o] + rh * (zo[r] - mu[r]);       // A_inner = A + rho/2*(Z - mu)   (:608)
      }
    }
    row_solve_regs2<RMAX>(x, Lsh, R);               // fac = (A_inner/L')/L            (:609)
    if (a.fused) {
      double z[RMAX];
#pragma unroll
      for (int r = 0; r < RMAX; ++r) z[r] = x[r] + mu[r];
      if (a.ptype == AOADMM_C_SIMPLEX_ROW) {
        simplex_regs<RMAX>(z, R, a.p0);
      } else {
#pragma unroll
        for (int r = 0; r < RMAX; ++r) z[r] = elem_prox(ep, z[r]);
      }
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        if (r < R) {
          const int64_t o = i + a.rows * r;
          const double mn = mu[r] + x[r] - z[r];     // mu = mu + fac - Z              (:1428)
          a.fac[o] = x[r];
          a.Z[o] = z[r];
          a.mu[o] = mn;
          const double d = x[r] - z[r];
          s1 += d * d;
          s2 += x[r] * x[r];
          s3 += mn * mn;
          const double e = z[r] - zo[r];
          s4 += e * e;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        if (r < R) {
          const int64_t o = i + a.rows * r;
          a.fac[o] = x[r];
          a.V[o] = x[r] + mu[r];
        }
      }
    }
  }
  if (a.fused) {
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);   // fixed-order DPP tree
    if (threadIdx.x == 0) {
      double* pb = a.part + ((int64_t)(a.it & 1) * kMaxParts + blockIdx.x) * 4;
      pb[0] = s1; pb[1] = s2; pb[2] = s3; pb[3] = s4;
    }
  }
}

int admm_partials(int64_t rows) {
  (void)rows;
  return 2 * kMaxParts;                             // both parities
}

// records the residuals / iteration count of the last executed inner iteration when the loop ran to
// MaxInnerIters (an earlier exit was recorded by the iteration that detected it).  The solver folds this
// into the Gram kernel that follows every mode update (atb_small); the kernel is for callers without one.
__global__ void admm_loop_end_k(LoopEnd le) { loop_end_eval(le); }

// element-wise dual update after a column-wise prox: mu += fac - Znew ; Z <- Znew ; partial norms
__global__ void dual_update_k(const double* fac, double* Z, double* mu, const double* Znew, int64_t n,
                              double* part, const AdmmCtl* ctl) {   // part: this iteration's parity block
  CTL_GUARD(ctl);
  __shared__ double red[4][4];
  double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double x = fac[i], z = Znew[i], zo = Z[i];
    const double mn = mu[i] + x - z;
    mu[i] = mn;
    Z[i] = z;
    const double d = x - z, e = z - zo;
    s1 += d * d; s2 += x * x; s3 += mn * mn; s4 += e * e;
  }
  s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = s1; red[1][w] = s2; red[2][w] = s3; red[3][w] = s4; }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += red[threadIdx.x][k];
    part[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;
  }
}

// ===========================================================================
// host-side composition
// ===========================================================================
template <int CPW>
static void launch_rows(const FusedArgs& a, unsigned blocks, hipStream_t s) {
  const int RP = a.R | 1;
  const size_t sh = ((size_t)a.R * a.R + (size_t)64 * RP + 16) * sizeof(double);
  if (sh > 65536) {                                   // R = 61..64: just above the default dynamic-LDS limit
    ensure_dynamic_lds(reinterpret_cast<const void*>(admm_rows_k<CPW, true>), (int)sh);
    ensure_dynamic_lds(reinterpret_cast<const void*>(admm_rows_k<CPW, false>), (int)sh);
  }
  if (a.R == 4 * CPW) admm_rows_k<CPW, true><<<blocks, kRowBlock, sh, s>>>(a);
  else admm_rows_k<CPW, false><<<blocks, kRowBlock, sh, s>>>(a);
}
template <int KS>
static void launch_rows_mfma(const FusedArgs& a, const SpecExtra& ex, bool fin, unsigned blocks, hipStream_t s) {
  const size_t sh = fin ? (size_t)16 * (a.R | 1) * sizeof(double) : 0;
  if (fin) admm_rows_mfma_k<KS, true><<<blocks, kSpecThreads, sh, s>>>(a, ex);
  else admm_rows_mfma_k<KS, false><<<blocks, kSpecThreads, sh, s>>>(a, ex);
}
static void launch_rows_mfma_any(const FusedArgs& a, const SpecExtra& ex, bool fin, unsigned blocks, hipStream_t s) {
  const int need = (a.R + 3) / 4;
  if (need <= 1) launch_rows_mfma<1>(a, ex, fin, blocks, s);
  else if (need <= 2) launch_rows_mfma<2>(a, ex, fin, blocks, s);
  else if (need <= 3) launch_rows_mfma<3>(a, ex, fin, blocks, s);
  else if (need <= 4) launch_rows_mfma<4>(a, ex, fin, blocks, s);
  else if (need <= 5) launch_rows_mfma<5>(a, ex, fin, blocks, s);
  else if (need <= 6) launch_rows_mfma<6>(a, ex, fin, blocks, s);
  else launch_rows_mfma<8>(a, ex, fin, blocks, s);
}
static void launch_row_iteration(const FusedArgs& a, unsigned blocks, hipStream_t s) {
  if (a.Binv) {
    const int need = (a.R + 3) / 4;
    if (need <= 1) launch_rows<1>(a, blocks, s);
    else if (need <= 2) launch_rows<2>(a, blocks, s);
    else if (need <= 3) launch_rows<3>(a, blocks, s);
    else if (need <= 4) launch_rows<4>(a, blocks, s);
    else if (need <= 5) launch_rows<5>(a, blocks, s);
    else if (need <= 6) launch_rows<6>(a, blocks, s);
    else if (need <= 8) launch_rows<8>(a, blocks, s);
    else if (need <= 12) launch_rows<12>(a, blocks, s);
    else launch_rows<16>(a, blocks, s);
  } else {
    const size_t sh = (size_t)a.R * a.R * sizeof(double);
    if (a.R <= 8) admm_rowL_k<8><<<blocks, kRowThreads, sh, s>>>(a);
    else if (a.R <= 16) admm_rowL_k<16><<<blocks, kRowThreads, sh, s>>>(a);
    else if (a.R <= 32) admm_rowL_k<32><<<blocks, kRowThreads, sh, s>>>(a);
    else admm_rowL_k<64><<<blocks, kRowThreads, sh, s>>>(a);
  }
}

// ---------------------------------------------------------------------------
// Short modes: the whole ADMM_constrained_only loop (:596-622) in ONE launch of one workgroup, thread = row, the row's
// operands (A, Z, mu, fac) in registers for the length of the loop.  Per inner iteration: A_inner (:608), the solve
// (:609; inv(L*L') or L from LDS, or the row's own factor for the per-row systems of a PARAFAC2 C mode, :602-606),
// update_constraint (:1420-1429) for the element-/row-wise catalogue and the column-norm family (column sums through
// one workgroup reduction), the four sums of eval_res_ADMM_constr (:1079-1096) through a second one, and the while
// test (:600) -- every thread holds the same totals, so the decision needs no further exchange.  At the end the
// kernel also leaves the Gram matrix of the new factor and its row-major copy (what atb_small would compute, :148).
// Replaces 2 launches per loop (element-wise prox), 3 per inner iteration (column-norm prox, PARAFAC2 C mode) plus
// the two Gram launches.  Sums run over waves in a fixed order: results do not depend on timing.
// ---------------------------------------------------------------------------
static constexpr int kWgLoopRows = 256;             // one row per thread: longer modes keep the multi-workgroup loops
static bool prox_is_colnorm(int t) {
  return t == AOADMM_C_L2_BALL || t == AOADMM_C_NONNEG_L2_BALL || t == AOADMM_C_NONNEG_L2_SPHERE || t == AOADMM_C_L2_REG;
}

// totals of NV per-thread values over the workgroup, the same in every thread (butterfly inside the wave, waves in
// index order through LDS)
template <int NV, int NW>
__device__ __forceinline__ void wg_sum(double (&v)[NV], double* red /* [NW][NV] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
  if (NW == 1) return;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[w * NV + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double x = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) x += red[q * NV + k];
    v[k] = x;
  }
  __syncthreads();
}

// SOLVE: 0 = inv(L*L') shared by all rows, 2 = one Cholesky factor per row.  For 0 the matrix sits in LDS as an
// RMAX x RMAX block padded with zeros and the row operands are padded with zeros, so the solve is straight-line code
// without rank tests; a padded column stays exactly zero.
template <int RMAX, int NT, int SOLVE>
__global__ __launch_bounds__(NT) void admm_loop_wg_k(WgLoopU a) {
  constexpr int NW = NT / 64;
  extern __shared__ double lds[];                    // M[RMAX*RMAX] | red[NW][max(RMAX,4)] | fsh[rows][RP] (Gram)
  constexpr int NRED = RMAX > 4 ? RMAX : 4;
  double* Msh = lds;
  double* red = lds + RMAX * RMAX;
  double* fsh = red + NW * NRED;
  AdmmCtl* ctl = a.ctl;
  if (!a.reset && ctl->active == 0) return;          // a failed factorisation (sys_build) leaves the state untouched
  const int t = threadIdx.x;
  const int R = a.R;
  const int64_t rows = a.rows;
  const bool have = t < rows;
  const int64_t i = have ? t : rows - 1;             // clamped: padding threads compute on the last row, store nothing
  double av[RMAX], z[RMAX], mu[RMAX], x[RMAX];
#pragma unroll
  for (int c = 0; c < RMAX; ++c) {
    const bool ok = c < R;
    const int64_t o = i + rows * (ok ? c : 0);
    av[c] = ok ? a.A[o] : 0.0; z[c] = ok ? a.Z[o] : 0.0; mu[c] = ok ? a.mu[o] : 0.0;
    x[c] = 0.0;
  }
  if (SOLVE != 2) {
    for (int e = t; e < RMAX * RMAX; e += NT) {
      const int r = e % RMAX, c = e / RMAX;
      Msh[e] = (r < R && c < R) ? a.Binv[r + R * c] : 0.0;
    }
  }
  const double rho = SOLVE == 2 ? a.rho[i] : a.rho[0];
  double rho_prox;                                   // max(rho) of a PARAFAC2 C mode (:1423-1424); rho otherwise
  if (SOLVE == 2 && a.rho_prox == nullptr) {         // the rows' own rho are this block's registers: max without a launch
    double mx = rho;                                 // padding threads hold the last row's value
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int q = 1; q < NW; ++q) mx = fmax(mx, red[q]);
    rho_prox = mx;
    __syncthreads();                                 // red is reused by the loop
  } else {
    rho_prox = a.rho_prox[0];
  }
  const double rh = rho / 2;
  const ElemProx ep = elem_prox_of(a.ptype, a.p0, a.p1, rho_prox);
  const bool colnorm = a.ptype == AOADMM_C_L2_BALL || a.ptype == AOADMM_C_NONNEG_L2_BALL ||
                       a.ptype == AOADMM_C_NONNEG_L2_SPHERE || a.ptype == AOADMM_C_L2_REG;
  const bool clampv = a.ptype == AOADMM_C_NONNEG_L2_BALL || a.ptype == AOADMM_C_NONNEG_L2_SPHERE;
  __syncthreads();
  double pr = 0.0, du = 0.0;
  int it = 0;
  for (;;) {
    // the system matrix is re-read (LDS / L1) every iteration: hoisted out of the loop its entries alone would take
    // more registers than the row operands (compiler barrier)
    asm volatile("" ::: "memory");
    // A_inner = A + rho/2*(Z - mu) (:608) and the solve (:609)
#pragma unroll
    for (int c = 0; c < RMAX; ++c) x[c] = av[c] + rh * (z[c] - mu[c]);
    if (SOLVE == 2) {
      const double* Lk = a.L + i * (int64_t)R * R;
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        if (r < R) {
          double v = x[r];
#pragma unroll
          for (int q = 0; q < RMAX; ++q)
            if (q < r) v -= Lk[r + R * q] * x[q];
          x[r] = v / Lk[r + R * r];
        }
      }
#pragma unroll
      for (int r = RMAX - 1; r >= 0; --r) {
        if (r < R) {
          double v = x[r];
#pragma unroll
          for (int q = 0; q < RMAX; ++q)
            if (q > r && q < R) v -= Lk[q + R * r] * x[q];
          x[r] = v / Lk[r + R * r];
        }
      }
    } else {
      double y[RMAX];
#pragma unroll
      for (int c = 0; c < RMAX; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < RMAX; ++q) acc += x[q] * Msh[q + RMAX * c];
        y[c] = acc;
      }
#pragma unroll
      for (int c = 0; c < RMAX; ++c) x[c] = y[c];
    }
    // update_constraint (:1420-1429): Z = prox(fac + mu), mu += fac - Z
    double zn[RMAX];
#pragma unroll
    for (int c = 0; c < RMAX; ++c) zn[c] = x[c] + mu[c];
    if (colnorm) {
      double cs[RMAX];
#pragma unroll
      for (int c = 0; c < RMAX; ++c) {
        const double y = clampv ? fmax(zn[c], 0.0) : zn[c];
        cs[c] = have ? y * y : 0.0;
      }
      wg_sum<RMAX, NW>(cs, red);
#pragma unroll
      for (int c = 0; c < RMAX; ++c) {
        if (c >= R) { zn[c] = 0.0; continue; }       // uniform
        const double nrm = sqrt(cs[c]);
        const double y = clampv ? fmax(zn[c], 0.0) : zn[c];
        if (a.ptype == AOADMM_C_NONNEG_L2_SPHERE) {
          if (nrm == 0.0) {
            // all-zero column: unit vector at the first maximum of the input (prox_normalized_nonneg.m:5-7)
            double bv = have ? zn[c] : -INFINITY;
            int bi = have ? t : 0x7fffffff;
            for (int off = 32; off > 0; off >>= 1) {
              const double ov = __shfl_xor(bv, off);
              const int oi = __shfl_xor(bi, off);
              if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (NW > 1) {
              int* ired = reinterpret_cast<int*>(red + NW);
              if ((t & 63) == 0) { red[t >> 6] = bv; ired[t >> 6] = bi; }
              __syncthreads();
              bv = red[0]; bi = ired[0];
              for (int q = 1; q < NW; ++q)
                if (red[q] > bv || (red[q] == bv && ired[q] < bi)) { bv = red[q]; bi = ired[q]; }
              __syncthreads();
            }
            zn[c] = t == bi ? 1.0 : 0.0;
          } else {
            zn[c] = y / nrm;
          }
        } else {
          double scale;
          if (a.ptype == AOADMM_C_L2_REG) {
            const double g = a.p0 / rho_prox;
            scale = nrm > g ? 1.0 - g / nrm : 0.0;
          } else {
            scale = nrm > a.p0 ? a.p0 / nrm : 1.0;
          }
          zn[c] = y * scale;
        }
      }
    } else if (a.ptype == AOADMM_C_SIMPLEX_ROW) {
      simplex_regs<RMAX>(zn, R, a.p0);
#pragma unroll
      for (int c = 0; c < RMAX; ++c) zn[c] = c < R ? zn[c] : 0.0;
    } else {
#pragma unroll
      for (int c = 0; c < RMAX; ++c) zn[c] = c < R ? elem_prox(ep, zn[c]) : 0.0;
    }
    double sm[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < RMAX; ++c) {
      const double mn = mu[c] + x[c] - zn[c];
      const double d = x[c] - zn[c], e = zn[c] - z[c];
      if (have) { sm[0] += d * d; sm[1] += x[c] * x[c]; sm[2] += mn * mn; sm[3] += e * e; }
      mu[c] = mn; z[c] = zn[c];
    }
    wg_sum<4, NW>(sm, red);
    pr = sqrt(sm[0]) / sqrt(sm[1]);                                          // :1085
    const double sc = sqrt(sm[2]);
    du = sc > 0 ? sqrt(sm[3]) / sc : sqrt(sm[3]);                            // :1087-1092
    ++it;
    if (!(it < a.max_inner && (pr > a.tol_pr || du > a.tol_du))) break;      // :600
  }
  if (have) {
#pragma unroll
    for (int c = 0; c < RMAX; ++c) {
      if (c < R) {
        const int64_t o = i + rows * c;
        a.fac[o] = x[c]; a.Z[o] = z[c]; a.mu[o] = mu[c];
      }
    }
  }
  if (t == 0) {
    ctl->res[0] = 0.0; ctl->res[1] = pr; ctl->res[2] = 0.0; ctl->res[3] = du;
    ctl->iters = it;
    ctl->active = 0;
  }
  if (a.gram == nullptr) return;
  // Gram matrix fac'*fac (:148) and the row-major copy of fac: rows through LDS, one (p, q) pair per wave at a time
  constexpr int RP = RMAX | 1;
  if (have) {
#pragma unroll
    for (int c = 0; c < RMAX; ++c) {
      fsh[t * RP + c] = x[c];
      if (c < R && a.facT) a.facT[(int64_t)t * R + c] = x[c];
    }
  }
  __syncthreads();
  const int lane = t & 63, w = t >> 6;
  const int npairs = R * (R + 1) / 2;
  for (int e = w; e < npairs; e += NW) {
    int p = 0, rem = e;                                // e -> (p, q), p <= q, row-wise over the upper triangle
    while (rem >= R - p) { rem -= R - p; ++p; }
    const int q = p + rem;
    double acc = 0.0;
    for (int64_t r0 = lane; r0 < rows; r0 += 64) acc += fsh[r0 * RP + p] * fsh[r0 * RP + q];
    acc = wave_sum(acc);
    if (lane == 0) { a.gram[p + R * q] = acc; a.gram[q + R * p] = acc; }
  }
}

size_t admm_loop_wg_lds(int rmax, int nt, int64_t rows, bool gram) {
  const int nred = rmax > 4 ? rmax : 4;
  return ((size_t)rmax * rmax + (size_t)(nt / 64) * nred + (gram ? (size_t)rows * (rmax | 1) : 0)) * sizeof(double);
}

bool admm_loop_wg_ok(int64_t rows, int R, int ptype, int max_inner) {
  if (max_inner < 1) return false;
  if (!(prox_is_fusable(ptype) || prox_is_colnorm(ptype))) return false;
  return rows <= kWgLoopRows && R <= 16;
}

void admm_loop_wg(const WgLoopU& a, hipStream_t s) {
  AO_REQUIRE(admm_loop_wg_ok(a.rows, a.R, a.ptype, a.max_inner), "admm_loop_wg: mode too large for the one-workgroup loop");
  const bool gram = a.gram != nullptr;
  AO_REQUIRE(a.per_row ? a.L != nullptr : a.Binv != nullptr, "admm_loop_wg: the shared system comes as inv(L*L'), per-row systems as factors");
  auto go = [&](auto rm) {
    constexpr int RM = decltype(rm)::value;
    const size_t lds = admm_loop_wg_lds(RM, kWgLoopRows, a.rows, gram);
    if (!a.per_row) admm_loop_wg_k<RM, kWgLoopRows, 0><<<1, kWgLoopRows, lds, s>>>(a);
    else admm_loop_wg_k<RM, kWgLoopRows, 2><<<1, kWgLoopRows, lds, s>>>(a);
  };
  if (a.R <= 4) go(std::integral_constant<int, 4>());
  else if (a.R <= 8) go(std::integral_constant<int, 8>());
  else go(std::integral_constant<int, 16>());
  AO_KERNEL_CHECK();
}

AdmmPath admm_path(int64_t rows, int R, int ptype, int max_inner, bool have_binv, bool have_prox_ws) {
  if (!have_binv) return kAdmmPathRowL;
  if (admm_loop_wg_ok(rows, R, ptype, max_inner)) return kAdmmPathWg;
  if (prox_is_fusable(ptype)) {
    // element-wise prox: the whole loop in two launches (admm_rows_mfma_k).  One wave per 16 rows; pass 2 adds the
    // partial sums of an iteration with kSpecPartJ loads per lane (tiles <= 256) and pass 1 leaves max_inner * tiles of
    // them in `part` (2 * kMaxParts slots); the simplex projection needs the whole row in one thread.
    const int64_t tiles = cdiv(rows, 16);
    if (ptype != AOADMM_C_SIMPLEX_ROW && R <= 32 && tiles <= 64 * kSpecPartJ && max_inner <= kSpecMaxInner &&
        (int64_t)max_inner * tiles <= 2 * kMaxParts)
      return kAdmmPathMfma;
    return kAdmmPathRowsFused;
  }
  return prox_tv_dual_ok(ptype, rows, have_prox_ws) ? kAdmmPathRowsTv : kAdmmPathRowsColProx;
}

void admm_constrained_loop(const AdmmMode& m, double* part, double* V, double* Znew, double* prox_ws,
                           AdmmCtl* ctl, int max_inner, double tol_pr, double tol_du, hipStream_t s,
                           LoopEnd* deferred_end, GramFold* gf) {
  const AdmmPath path = admm_path(m.rows, m.R, m.prox.type, max_inner, m.Binv != nullptr, prox_ws != nullptr);
  AO_REQUIRE(path != kAdmmPathWg, "admm_constrained_loop: this mode belongs to the one-workgroup loop (admm_loop_wg)");
  FusedArgs a;
  a.A = m.A; a.L = m.L; a.Binv = m.Binv; a.rho = m.rho; a.fac = m.fac; a.Z = m.Z; a.mu = m.mu; a.V = V; a.part = part;
  a.ctl = ctl;
  a.rows = m.rows; a.R = m.R; a.ptype = m.prox.type; a.p0 = m.prox.p0; a.p1 = m.prox.p1;
  a.fused = prox_is_fusable(m.prox.type) ? 1 : 0;
  a.max_inner = max_inner; a.tol_pr = tol_pr; a.tol_du = tol_du;
  int64_t nblk = cdiv(m.rows, kRowThreads);
  if (nblk > kMaxParts) nblk = kMaxParts;
  const unsigned blocks = (unsigned)nblk;
  const int64_t n = m.rows * m.R;
  int64_t nbd = cdiv(n, 1024);
  if (nbd > 64) nbd = 64;
  if (path == kAdmmPathMfma) {
    const int64_t tiles = cdiv(m.rows, 16);            // one wave per 16 rows
    SpecExtra ex{nullptr, nullptr};
    launch_rows_mfma_any(a, ex, false, (unsigned)tiles, s);
    AO_KERNEL_CHECK();
    if (gf && gf->ws) { ex.gram_ws = gf->ws; ex.At = gf->At; gf->nb = (int)tiles; }
    launch_rows_mfma_any(a, ex, true, (unsigned)tiles, s);
    AO_KERNEL_CHECK();
    if (deferred_end) *deferred_end = LoopEnd();    // the loop is closed: pass 2 recorded iters / residuals
    return;
  }
  // prox + dual in one kernel (without inv(L*L') the primal kernel differs, the rest of the chain does not)
  const bool tv_fused = path == kAdmmPathRowsTv || (path == kAdmmPathRowL && prox_tv_dual_ok(m.prox.type, m.rows, prox_ws != nullptr));
  const int nparts = a.fused ? (int)blocks : (tv_fused ? m.R : (int)nbd);
  for (int it = 0; it < max_inner; ++it) {
    a.it = it;
    a.nparts_prev = nparts;
    launch_row_iteration(a, blocks, s);
    AO_KERNEL_CHECK();
    double* part_it = part + (int64_t)(it & 1) * kMaxParts * 4;   // this iteration's parity block
    if (tv_fused) {
      prox_tv_dual(m.prox, V, m.rows, m.R, m.rho, prox_ws, m.Z, m.mu, part_it, ctl, s);
    } else if (!a.fused) {
      prox_apply(m.prox, V, m.rows, Znew, m.rows, m.rows, m.R, m.rho, 1.0, prox_ws, ctl, s, m.Z, m.rows);
      dual_update_k<<<(unsigned)nbd, 256, 0, s>>>(m.fac, m.Z, m.mu, Znew, n, part_it, ctl);
      AO_KERNEL_CHECK();
    }
  }
  LoopEnd le;
  le.part = part; le.nparts = nparts; le.max_inner = max_inner; le.tol_pr = tol_pr; le.tol_du = tol_du; le.ctl = ctl;
  if (deferred_end) {
    *deferred_end = le;
  } else {
    admm_loop_end_k<<<1, 64, 0, s>>>(le);
    AO_KERNEL_CHECK();
  }
}

size_t admm_mode_ws_bytes(int64_t rows, int R) {    // the loop's Gram partials ([tiles][R*R]) or the Gram kernel's workspace
  const size_t fold = (size_t)cdiv(rows, 16) * R * R * sizeof(double), atb = atb_ws_bytes(rows, R, R);
  return fold > atb ? fold : atb;
}

AdmmPath admm_mode_update(const AdmmMode& m, double* part, double* V, double* Znew, double* prox_ws,
                          double* gram, double* facT, double* gram_ws,
                          AdmmCtl* ctl, int max_inner, double tol_pr, double tol_du, hipStream_t s) {
  const AdmmPath path = admm_path(m.rows, m.R, m.prox.type, max_inner, m.Binv != nullptr, prox_ws != nullptr);
  if (path == kAdmmPathWg) {
    // short mode: loop, Gram matrix and row-major copy in one launch of one workgroup
    WgLoopU wa;
    wa.A = m.A; wa.Binv = m.Binv; wa.L = m.L; wa.rho = m.rho; wa.rho_prox = m.rho; wa.fac = m.fac; wa.Z = m.Z; wa.mu = m.mu;
    wa.rows = m.rows; wa.R = m.R; wa.per_row = 0; wa.ptype = m.prox.type; wa.p0 = m.prox.p0; wa.p1 = m.prox.p1;
    wa.max_inner = max_inner; wa.tol_pr = tol_pr; wa.tol_du = tol_du; wa.ctl = ctl; wa.gram = gram; wa.facT = facT;
    admm_loop_wg(wa, s);
    return path;
  }
  LoopEnd le;
  GramFold gf{gram_ws, facT};
  admm_constrained_loop(m, part, V, Znew, prox_ws, ctl, max_inner, tol_pr, tol_du, s, &le, &gf);
  // :148 from the partials the loop's last launch left, or by the Gram kernel, which then also closes the loop
  if (gf.nb > 0) atb_fin(gram, gram_ws, gf.nb, m.R * m.R, nullptr, s);
  else atb_small(gram, m.fac, m.rows, m.fac, m.rows, m.rows, m.R, m.R, gram_ws, nullptr, s, facT, le.ctl ? &le : nullptr);
  return path;
}

__global__ void copy_add_k(double* V, double* Zold, const double* fac, const double* Z, const double* mu, int64_t n,
                           const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    V[i] = fac[i] + mu[i];
    Zold[i] = Z[i];
  }
}
// mu += fac - Z (:1063) and the four sums of eval_res_ADMM_constr in the same pass:
// ||fac-Z||^2, ||fac||^2, ||mu||^2, ||Z-Zold||^2.  One block writes the slots itself; several blocks leave
// per-block partial sums that dual_sums_fin_k adds in block order.
__global__ __launch_bounds__(256) void dual_sums_k(const double* fac, const double* Z, double* mu, const double* Zold,
                                                   int64_t n, double* slots, double* ws, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  __shared__ double sh4[4];
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double f = fac[i], z = Z[i];
    const double m = mu[i] + f - z;
    mu[i] = m;
    const double dz = z - Zold[i];
    s0 += (f - z) * (f - z); s1 += f * f; s2 += m * m; s3 += dz * dz;
  }
  s0 = block256_sum(s0, sh4); s1 = block256_sum(s1, sh4); s2 = block256_sum(s2, sh4); s3 = block256_sum(s3, sh4);
  if (threadIdx.x == 0) {
    double* o = gridDim.x == 1 ? slots : ws + 4 * (int64_t)blockIdx.x;
    o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
  }
}
__global__ void dual_sums_fin_k(double* slots, const double* ws, int nb, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  if (threadIdx.x >= 4) return;
  double t = 0.0;
  for (int b = 0; b < nb; ++b) t += ws[4 * b + threadIdx.x];
  slots[threadIdx.x] = t;
}

// update_constraint (:1420-1429) with an element-/row-wise prox in ONE launch of one workgroup (thread = row):
// Zold = Z, Z = prox(fac + mu, rho), mu += fac - Z and the four sums of eval_res_ADMM_constr.  The three-launch form
// below (fac + mu, prox, dual + sums) is ~12 us of launches per call; the coupled and PARAFAC2 loops of the example
// scripts call it 4-15 times per outer iteration.
template <int RMAX>
__global__ __launch_bounds__(256) void constraint_update_rows_k(ColArgs a, const double* fac, double* mu, double* Zold,
                                                               double* slots, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  __shared__ double sh4[4];
  const double rho = a.rho[0] * a.rho_mul;
  const int R = a.R;
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int64_t i = threadIdx.x; i < a.rows; i += 256) {
    double f[RMAX], m[RMAX], zo[RMAX], z[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const bool ok = r < R;
      f[r] = ok ? fac[i + a.rows * r] : 0.0;
      m[r] = ok ? mu[i + a.rows * r] : 0.0;
      zo[r] = ok ? a.Z[i + a.ldz * r] : 0.0;
      z[r] = f[r] + m[r];
    }
    if (a.type == AOADMM_C_SIMPLEX_ROW) {
      simplex_regs<RMAX>(z, R, a.p0);
    } else {
#pragma unroll
      for (int r = 0; r < RMAX; ++r) z[r] = prox_elem(a.type, z[r], a.p0, a.p1, rho);
    }
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
      if (r < R) {
        const double mn = m[r] + f[r] - z[r];
        Zold[i + a.rows * r] = zo[r];
        a.Z[i + a.ldz * r] = z[r];
        mu[i + a.rows * r] = mn;
        const double dz = z[r] - zo[r];
        s0 += (f[r] - z[r]) * (f[r] - z[r]); s1 += f[r] * f[r]; s2 += mn * mn; s3 += dz * dz;
      }
  }
  s0 = block256_sum(s0, sh4); s1 = block256_sum(s1, sh4); s2 = block256_sum(s2, sh4); s3 = block256_sum(s3, sh4);
  if (threadIdx.x == 0) { slots[0] = s0; slots[1] = s1; slots[2] = s2; slots[3] = s3; }
}

void constraint_update(const ProxSpec& ps, const double* fac, double* Z, double* mu, double* Zold,
                       double* V, int64_t rows, int R, const double* rho_dev, double rho_mul,
                       double* prox_ws, double* slots, double* red_ws, const AdmmCtl* ctl,
                       hipStream_t s) {
  if (prox_is_fusable(ps.type) && rows <= 8192 && R <= 32) {
    ColArgs a;
    a.V = nullptr; a.Z = Z; a.ldv = rows; a.ldz = rows; a.rows = rows; a.R = R; a.type = ps.type;
    a.p0 = ps.p0; a.p1 = ps.p1; a.rho = rho_dev; a.rho_mul = rho_mul; a.ws = nullptr;
    if (R <= 4) constraint_update_rows_k<4><<<1, 256, 0, s>>>(a, fac, mu, Zold, slots, ctl);
    else if (R <= 8) constraint_update_rows_k<8><<<1, 256, 0, s>>>(a, fac, mu, Zold, slots, ctl);
    else if (R <= 16) constraint_update_rows_k<16><<<1, 256, 0, s>>>(a, fac, mu, Zold, slots, ctl);
    else constraint_update_rows_k<32><<<1, 256, 0, s>>>(a, fac, mu, Zold, slots, ctl);
    AO_KERNEL_CHECK();
    return;
  }
  const int64_t n = rows * R;
  int64_t nb = cdiv(n, 256);
  if (nb > 1024) nb = 1024;
  copy_add_k<<<(unsigned)nb, 256, 0, s>>>(V, Zold, fac, Z, mu, n, ctl);
  AO_KERNEL_CHECK();
  prox_apply(ps, V, rows, Z, rows, rows, R, rho_dev, rho_mul, prox_ws, ctl, s, Zold, rows);   // Z = prox(fac+mu, rho)
  int64_t nr = cdiv(n, 2048);
  if (nr > 64) nr = 64;
  dual_sums_k<<<(unsigned)nr, 256, 0, s>>>(fac, Z, mu, Zold, n, slots, red_ws, ctl);
  AO_KERNEL_CHECK();
  if (nr > 1) {
    dual_sums_fin_k<<<1, 64, 0, s>>>(slots, red_ws, (int)nr, ctl);
    AO_KERNEL_CHECK();
  }
}

__global__ void admm_finalize_generic_k(FinalizeArgs fa, AdmmCtl* ctl) {
  if (ctl->active == 0) return;
  if (threadIdx.x != 0) return;
  double prc = 0, duc = 0, prz = 0, duz = 0;
  int nc = 0, nz = 0;
  for (int m = 0; m < fa.nmodes; ++m) {
    const double* s = fa.slots[m];
    if (fa.coupled[m]) {                        // eval_res_ADMM_coupl_case* (:1099-1210)
      prc += sqrt(s[4]) / sqrt(s[7]);             // [7] = ||C||^2, or ||H*C||^2 / ||C*H||^2 for types 1, 2
      const double sc = sqrt(s[5]);
      duc += sc > 0 ? sqrt(s[6]) / sc : sqrt(s[6]);
      ++nc;
    }
    if (fa.constrained[m]) {                    // eval_res_ADMM_constr (:1079-1096)
      prz += sqrt(s[0]) / sqrt(s[1]);
      const double sc = sqrt(s[2]);
      duz += sc > 0 ? sqrt(s[3]) / sc : sqrt(s[3]);
      ++nz;
    }
  }
  if (nc) { prc /= nc; duc /= nc; }
  if (nz) { prz /= nz; duz /= nz; }             // else 0 (:690-691)
  ctl->res[0] = prc; ctl->res[1] = prz; ctl->res[2] = duc; ctl->res[3] = duz;
  const int it = ctl->iters + 1;
  ctl->iters = it;
  ctl->active = (it < fa.max_inner && (prc > fa.tol_pr_coupl || prz > fa.tol_pr_constr ||
                                       duc > fa.tol_du_coupl || duz > fa.tol_du_constr)) ? 1 : 0;
}
void admm_finalize_generic(const FinalizeArgs& fa, AdmmCtl* ctl, hipStream_t s) {
  admm_finalize_generic_k<<<1, 64, 0, s>>>(fa, ctl);
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
