// Coupled ADMM inner loop: kernels and launchers, see couple.h.
#include "couple.h"
#include "device_utils.h"
#include "prox_dev.h"

#include <algorithm>
#include <type_traits>

namespace aoadmm {

CouplePath couple_path(int type, int n_modes, int64_t rows, int rmax, bool any_par2_c, bool local_prox) {
  CouplePath path = CouplePath::Generic;
  if ((type == 0 || type == 4) && !any_par2_c && rmax <= 16) {
    if (n_modes <= 4 && rows <= 2048 && local_prox)
      path = rows <= 256 && rmax <= 8 && n_modes <= 3 ? CouplePath::Regs : CouplePath::Wg;
    else path = CouplePath::RowSteps;
  }
  return path;
}

int couple_rank_class(int rmax) { return rmax <= 4 ? 4 : rmax <= 8 ? 8 : 16; }

template <class F>
static void by_rmax(int rmax, F&& launch) {
  const int cls = couple_rank_class(rmax);
  if (cls == 4) launch(std::integral_constant<int, 4>());
  else if (cls == 8) launch(std::integral_constant<int, 8>());
  else launch(std::integral_constant<int, 16>());
}

__global__ void coupling_coefs_k(double* coef, const double* const* rhos, int n, AdmmCtl* ctl) {
  // coef[j] = rho_j / sum rho  (:661-675); also opens the coupled loop (what ctl_reset does: one launch fewer)
  if (threadIdx.x == 1) {
    ctl->active = 1;
    ctl->iters = 0;
    ctl->res[0] = ctl->res[1] = ctl->res[2] = ctl->res[3] = 0.0;
  }
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += rhos[j][0];
    for (int j = 0; j < n; ++j) coef[j] = 1.0 / s * rhos[j][0];
    coef[n] = s;
  }
}

// mu_Delta += Tf(C) - Sd(Delta) (:679 and the same line of every case) with the sums the coupling residuals need in
// the same pass: out[0] = ||Tf(C) - Sd(Delta)||^2, out[1] = ||mu_Delta||^2, out[3] = ||den||^2 (den = Tf(C) or C,
// :1099-1210); out[2] (the dual numerator) is filled by the caller.  One workgroup for n <= 2048, else per-block
// partial sums added in block order by coupling_dual_fin_k.
__global__ __launch_bounds__(256) void coupling_dual_k(double* muD, const double* tf, const double* td, int64_t ni,
                                                       const double* den, int64_t nden, double* out, double* ws,
                                                       const AdmmCtl* ctl) {
  if (ctl != nullptr && ctl->active == 0) return;
  __shared__ double sh4[4];
  double s0 = 0, s1 = 0, s2 = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = first; i < ni; i += stride) {
    const double g = tf[i] - td[i];
    const double m = muD[i] + g;
    muD[i] = m;
    s0 += g * g; s1 += m * m;
  }
  for (int64_t i = first; i < nden; i += stride) s2 += den[i] * den[i];
  s0 = block256_sum(s0, sh4); s1 = block256_sum(s1, sh4); s2 = block256_sum(s2, sh4);
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) { out[0] = s0; out[1] = s1; out[3] = s2; }
    else { double* w = ws + 3 * (int64_t)blockIdx.x; w[0] = s0; w[1] = s1; w[2] = s2; }
  }
}
__global__ void coupling_dual_fin_k(double* out, const double* ws, int nb, const AdmmCtl* ctl) {
  if (ctl != nullptr && ctl->active == 0) return;
  if (threadIdx.x >= 3) return;
  double t = 0.0;
  for (int b = 0; b < nb; ++b) t += ws[3 * b + threadIdx.x];
  out[threadIdx.x == 2 ? 3 : threadIdx.x] = t;
}

__global__ void coupling_rowmean_k(double* Delta, RowMeanArgs a, const AdmmCtl* ctl) {
  if (ctl != nullptr && ctl->active == 0) return;
  const int64_t tot = a.rows * a.cols;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = e % a.rows;
    double acc = 0.0, sr = 0.0;
    for (int j = 0; j < a.n; ++j) {
      const double rj = a.vec[j] ? a.rho[j][k] : a.rho[j][0];
      acc += rj * (a.fac[j][e] + a.mu[j][e]);
      sr += rj;
    }
    Delta[e] = 1.0 / sr * acc;
  }
}

// out(k,c) = rho_k * in(k,c)  (rows of a K x cols matrix scaled by the rho vector of a PARAFAC2 C mode)
__global__ void rows_scale_k(double* out, const double* in, const double* rho, int64_t rows, int64_t cols,
                             const AdmmCtl* ctl) {
  if (ctl != nullptr && ctl->active == 0) return;
  const int64_t tot = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x)
    out[e] = rho[e % rows] * in[e];
}
// Delta(k,:) = BB(k,:) / (AA + rho_k*AAA)   (:957-961): one workgroup per row, q x q system in LDS
__global__ void delta_rowwise_solve_k(double* Delta, const double* BB, int64_t rows, int q, const double* AA,
                                      const double* AAA, const double* rho, AdmmCtl* ctl) {
  if (ctl->active == 0) return;
  extern __shared__ double sh[];                      // q*q matrix, then q right-hand side
  double* M = sh;
  double* x = sh + q * q;
  const int64_t k = blockIdx.x;
  for (int e = threadIdx.x; e < q * q; e += blockDim.x) M[e] = AA[e] + rho[k] * AAA[e];
  for (int c = threadIdx.x; c < q; c += blockDim.x) x[c] = BB[k + rows * c];
  __syncthreads();
  const bool ok = chol_lds(M, q);
  if (!ok) { if (threadIdx.x == 0) ctl->notpd = 1; return; }
  if (threadIdx.x == 0) {                             // x * inv(L*L'): forward with L, backward with L'
    for (int c = 0; c < q; ++c) {
      double v = x[c];
      for (int p = 0; p < c; ++p) v -= M[c + q * p] * x[p];
      x[c] = v / M[c + q * c];
    }
    for (int c = q - 1; c >= 0; --c) {
      double v = x[c];
      for (int p = c + 1; p < q; ++p) v -= M[p + q * c] * x[p];
      x[c] = v / M[c + q * c];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < q; c += blockDim.x) Delta[k + rows * c] = x[c];
}

__global__ void coupling_AA_k(double* AA, AAArgs a) {
  // AA = sum_j rho_j * H_j * H_j'   (:941-954 ; :1033-1047 with H2 and the common rhoC)
  const int Rc = a.Rc;
  for (int e = threadIdx.x; e < Rc * Rc; e += blockDim.x) {
    const int i = e % Rc, k = e / Rc;
    double acc = 0.0;
    for (int j = 0; j < a.n; ++j) {
      double t = 0.0;
      for (int q = 0; q < a.R[j]; ++q) t += a.H[j][i + Rc * q] * a.H[j][k + Rc * q];
      acc += a.rho[j][0] * t;
    }
    AA[e] = acc;
  }
}

void coupling_coefs(double* coef, const double* const* rhos, int n, AdmmCtl* ctl, hipStream_t s) {
  coupling_coefs_k<<<1, 64, 0, s>>>(coef, rhos, n, ctl);
  AO_KERNEL_CHECK();
}
void coupling_AA(double* AA, const AAArgs& a, hipStream_t s) {
  coupling_AA_k<<<1, 256, 0, s>>>(AA, a);
  AO_KERNEL_CHECK();
}
void coupling_dual(double* muD, const double* tf, const double* td, int64_t ni, const double* fac, int64_t nm,
                   bool img_den, double* out, double* ws, const AdmmCtl* ctl, hipStream_t s) {
  int64_t nr = cdiv(std::max(ni, nm), 2048);
  if (nr > 64) nr = 64;
  coupling_dual_k<<<(unsigned)nr, 256, 0, s>>>(muD, tf, td, ni, img_den ? tf : fac, img_den ? ni : nm, out, ws, ctl);
  AO_KERNEL_CHECK();
  if (nr > 1) {
    coupling_dual_fin_k<<<1, 64, 0, s>>>(out, ws, (int)nr, ctl);
    AO_KERNEL_CHECK();
  }
}
void coupling_rowmean(double* Delta, const RowMeanArgs& a, const AdmmCtl* ctl, hipStream_t s) {
  int64_t nb = cdiv(a.rows * a.cols, 256);
  if (nb > 1024) nb = 1024;
  coupling_rowmean_k<<<(unsigned)nb, 256, 0, s>>>(Delta, a, ctl);
  AO_KERNEL_CHECK();
}
void rows_scale(double* out, const double* in, const double* rho, int64_t rows, int64_t cols, const AdmmCtl* ctl,
                hipStream_t s) {
  int64_t nb = cdiv(rows * cols, 256);
  if (nb > 1024) nb = 1024;
  rows_scale_k<<<(unsigned)nb, 256, 0, s>>>(out, in, rho, rows, cols, ctl);
  AO_KERNEL_CHECK();
}
void delta_rowwise_solve(double* Delta, const double* BB, int64_t rows, int q, const double* AA, const double* AAA,
                         const double* rho, AdmmCtl* ctl, hipStream_t s) {
  delta_rowwise_solve_k<<<(unsigned)rows, 64, (size_t)(q * q + q) * sizeof(double), s>>>(Delta, BB, rows, q, AA, AAA, rho, ctl);
  AO_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------
// row-local couplings, one launch per step (RowCouple, RowDelta: couple.h)
template <int RMAX>
__global__ __launch_bounds__(64) void couple_primal_rows_k(RowCouple m, const double* Delta, int64_t rows, int q, int type,
                                                           const AdmmCtl* ctl) {
  if (ctl != nullptr && ctl->active == 0) return;
  extern __shared__ double sh[];                      // L (R*R), H (q*R)
  const int R = m.R;
  double* Lsh = sh;
  double* Hsh = sh + R * R;
  for (int e = threadIdx.x; e < R * R; e += blockDim.x) Lsh[e] = m.L[e];
  if (type == 4)
    for (int e = threadIdx.x; e < q * R; e += blockDim.x) Hsh[e] = m.H[e];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const double rh = m.rho[0] / 2;
  double d[RMAX], x[RMAX];
#pragma unroll
  for (int c = 0; c < RMAX; ++c) d[c] = c < q ? Delta[i + rows * c] : 0.0;
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    x[r] = 0.0;
    if (r < R) {
      double td;
      if (type == 4) {                                // (Delta*H)(i,r)  (:925)
        td = 0.0;
#pragma unroll
        for (int c = 0; c < RMAX; ++c)
          if (c < q) td += d[c] * Hsh[c + q * r];
      } else {
        td = d[r];                                    // :647
      }
      double v = m.Aeff[i + rows * r] + rh * (td - m.muD[i + rows * r]);
      if (m.constrained) v += rh * (m.Z[i + rows * r] - m.mu[i + rows * r]);
      x[r] = v;
    }
  }
#pragma unroll
  for (int r = 0; r < RMAX; ++r)                      // x * inv(L*L')  (:651, :929)
    if (r < R) {
      double v = x[r];
#pragma unroll
      for (int p = 0; p < RMAX; ++p)
        if (p < r) v -= Lsh[r + R * p] * x[p];
      x[r] = v / Lsh[r + R * r];
    }
#pragma unroll
  for (int r = RMAX - 1; r >= 0; --r)
    if (r < R) {
      double v = x[r];
#pragma unroll
      for (int p = 0; p < RMAX; ++p)
        if (p > r && p < R) v -= Lsh[p + R * r] * x[p];
      x[r] = v / Lsh[r + R * r];
    }
#pragma unroll
  for (int r = 0; r < RMAX; ++r)
    if (r < R) m.fac[i + rows * r] = x[r];
}

// Delta_old = Delta ; Delta = weighted mean (type 0, :661-675) or BB / AA (type 4, :939-963) ; dD = Delta - Delta_old
template <int RMAX>
__global__ __launch_bounds__(64) void couple_delta_rows_k(RowDelta a, double* Delta, double* DeltaOld, double* dD,
                                                          const double* coefs, const double* LAA, int64_t rows, int q,
                                                          int type, const AdmmCtl* ctl) {
  if (ctl != nullptr && ctl->active == 0) return;
  extern __shared__ double sh[];                      // LAA (q*q), then H_j (q*R_j) back to back
  double* Lsh = sh;
  if (type == 4) {
    for (int e = threadIdx.x; e < q * q; e += blockDim.x) Lsh[e] = LAA[e];
    int off = q * q;
    for (int j = 0; j < a.n; ++j) {
      for (int e = threadIdx.x; e < q * a.R[j]; e += blockDim.x) sh[off + e] = a.H[j][e];
      off += q * a.R[j];
    }
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  double bb[RMAX];
#pragma unroll
  for (int c = 0; c < RMAX; ++c) bb[c] = 0.0;
  int off = q * q;
  for (int j = 0; j < a.n; ++j) {
    if (type == 4) {
      const double rj = a.rho[j][0];
      double t[RMAX];
#pragma unroll
      for (int r = 0; r < RMAX; ++r) t[r] = r < a.R[j] ? a.fac[j][i + rows * r] + a.muD[j][i + rows * r] : 0.0;
      const double* Hj = sh + off;
#pragma unroll
      for (int c = 0; c < RMAX; ++c)
        if (c < q) {
          double acc = 0.0;
#pragma unroll
          for (int r = 0; r < RMAX; ++r)
            if (r < a.R[j]) acc += t[r] * Hj[c + q * r];
          bb[c] = (j == 0 ? 0.0 : bb[c]) + rj * acc;                               // :955, same order as the gemm path
        }
      off += q * a.R[j];
    } else {
      const double cj = coefs[j];                     // rho_j / sum rho
#pragma unroll
      for (int c = 0; c < RMAX; ++c)
        if (c < q) {
          const double v = cj * a.fac[j][i + rows * c] + cj * a.muD[j][i + rows * c];
          bb[c] = j == 0 ? v : bb[c] + v;
        }
    }
  }
  if (type == 4) {                                    // Delta(i,:) = bb * inv(LAA*LAA')
#pragma unroll
    for (int c = 0; c < RMAX; ++c)
      if (c < q) {
        double v = bb[c];
#pragma unroll
        for (int p = 0; p < RMAX; ++p)
          if (p < c) v -= Lsh[c + q * p] * bb[p];
        bb[c] = v / Lsh[c + q * c];
      }
#pragma unroll
    for (int c = RMAX - 1; c >= 0; --c)
      if (c < q) {
        double v = bb[c];
#pragma unroll
        for (int p = 0; p < RMAX; ++p)
          if (p > c && p < q) v -= Lsh[p + q * c] * bb[p];
        bb[c] = v / Lsh[c + q * c];
      }
  }
#pragma unroll
  for (int c = 0; c < RMAX; ++c)
    if (c < q) {
      const double old = Delta[i + rows * c];
      DeltaOld[i + rows * c] = old;
      Delta[i + rows * c] = bb[c];
      dD[i + rows * c] = bb[c] - old;
    }
}

// mu_Delta += C - Sd(Delta) and the four sums of the coupling residuals (:1099-1115, :1175-1191) for one mode:
// out[0] = ||C - Sd(Delta)||^2, out[1] = ||mu_Delta||^2, out[2] = ||Sd(dD)||^2, out[3] = ||C||^2
template <int RMAX>
__global__ __launch_bounds__(256) void couple_dual_rows_k(RowCouple m, const double* Delta, const double* dD, int64_t rows,
                                                          int q, int type, double* out, double* ws, const AdmmCtl* ctl) {
  if (ctl != nullptr && ctl->active == 0) return;
  extern __shared__ double sh[];                      // H (q*R)
  __shared__ double sh4[4];
  const int R = m.R;
  if (type == 4)
    for (int e = threadIdx.x; e < q * R; e += blockDim.x) sh[e] = m.H[e];
  __syncthreads();
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
    double d[RMAX], dd[RMAX];
#pragma unroll
    for (int c = 0; c < RMAX; ++c) { d[c] = c < q ? Delta[i + rows * c] : 0.0; dd[c] = c < q ? dD[i + rows * c] : 0.0; }
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
      if (r < R) {
        double td, tdd;
        if (type == 4) {
          td = 0.0; tdd = 0.0;
#pragma unroll
          for (int c = 0; c < RMAX; ++c)
            if (c < q) { td += d[c] * sh[c + q * r]; tdd += dd[c] * sh[c + q * r]; }
        } else { td = d[r]; tdd = dd[r]; }
        const double f = m.fac[i + rows * r];
        const double g = f - td;
        const double mm = m.muD[i + rows * r] + g;                                  // :679, :967
        m.muD[i + rows * r] = mm;
        s0 += g * g; s1 += mm * mm; s2 += tdd * tdd; s3 += f * f;
      }
  }
  s0 = block256_sum(s0, sh4); s1 = block256_sum(s1, sh4); s2 = block256_sum(s2, sh4); s3 = block256_sum(s3, sh4);
  if (threadIdx.x == 0) {
    double* o = gridDim.x == 1 ? out : ws + 4 * (int64_t)blockIdx.x;
    o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
  }
}
__global__ void couple_dual_fin_k(double* out, const double* ws, int nb, const AdmmCtl* ctl) {
  if (ctl != nullptr && ctl->active == 0) return;
  if (threadIdx.x >= 4) return;
  double t = 0.0;
  for (int b = 0; b < nb; ++b) t += ws[4 * b + threadIdx.x];
  out[threadIdx.x] = t;
}

void couple_primal_rows(const RowCouple& m, const double* Delta, int64_t rows, int q, int type, int rmax,
                        const AdmmCtl* ctl, hipStream_t s) {
  const size_t lds = ((size_t)m.R * m.R + (size_t)q * m.R) * sizeof(double);
  by_rmax(rmax, [&](auto tag) {
    couple_primal_rows_k<decltype(tag)::value><<<(unsigned)cdiv(rows, 64), 64, lds, s>>>(m, Delta, rows, q, type, ctl);
  });
  AO_KERNEL_CHECK();
}
void couple_delta_rows(const RowDelta& a, double* Delta, double* DeltaOld, double* dD, const double* coefs,
                       const double* LAA, int64_t rows, int q, int type, int rmax, const AdmmCtl* ctl, hipStream_t s) {
  size_t lds = (size_t)q * q;
  for (int j = 0; j < a.n; ++j) lds += (size_t)q * a.R[j];
  by_rmax(rmax, [&](auto tag) {
    couple_delta_rows_k<decltype(tag)::value><<<(unsigned)cdiv(rows, 64), 64, lds * sizeof(double), s>>>(
        a, Delta, DeltaOld, dD, coefs, LAA, rows, q, type, ctl);
  });
  AO_KERNEL_CHECK();
}
void couple_dual_rows(const RowCouple& m, const double* Delta, const double* dD, int64_t rows, int q, int type, int rmax,
                      double* out, double* ws, const AdmmCtl* ctl, hipStream_t s) {
  int64_t nr = cdiv(rows, 2048);
  if (nr > 64) nr = 64;
  by_rmax(rmax, [&](auto tag) {
    couple_dual_rows_k<decltype(tag)::value><<<(unsigned)nr, 256, (size_t)q * m.R * sizeof(double), s>>>(
        m, Delta, dD, rows, q, type, out, ws, ctl);
  });
  AO_KERNEL_CHECK();
  if (nr > 1) {
    couple_dual_fin_k<<<1, 64, 0, s>>>(out, ws, (int)nr, ctl);
    AO_KERNEL_CHECK();
  }
}

// ---------------------------------------------------------------------------
// row-local couplings, the whole loop in one launch (WgLoopArgs: couple.h)
template <int RMAX>
__global__ __launch_bounds__(256) void couple_loop_wg_k(WgLoopArgs a) {
  extern __shared__ double sh[];                      // LAA (q*q) | per mode: L (R*R), H (q*R)
  __shared__ double red[4][32];
  __shared__ int go;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int q = a.q, type = a.type;
  const int64_t rows = a.rows;
  int offL[4], offH[4];
  {
    int off = q * q;
    for (int j = 0; j < a.n; ++j) { offL[j] = off; off += a.m[j].R * a.m[j].R; offH[j] = off; off += q * a.m[j].R; }
    if (type == 4)
      for (int e = t; e < q * q; e += 256) sh[e] = a.LAA[e];
    for (int j = 0; j < a.n; ++j) {
      const int R = a.m[j].R;
      for (int e = t; e < R * R; e += 256) sh[offL[j] + e] = a.m[j].L[e];
      if (type == 4)
        for (int e = t; e < q * R; e += 256) sh[offH[j] + e] = a.m[j].H[e];
    }
  }
  if (t == 0) go = a.ctl->active;
  __syncthreads();
  int it = 0;
  while (go) {
    double sums[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) sums[j][k] = 0.0;
    for (int64_t i = t; i < rows; i += 256) {
      double d[RMAX];
#pragma unroll
      for (int c = 0; c < RMAX; ++c) d[c] = c < q ? a.Delta[i + rows * c] : 0.0;
      // ---- primal updates
      for (int j = 0; j < a.n; ++j) {
        const WgLoopMode& m = a.m[j];
        const int R = m.R;
        const double* Lsh = sh + offL[j];
        const double* Hsh = sh + offH[j];
        const double rh = m.rho[0] / 2;
        double x[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
          x[r] = 0.0;
          if (r < R) {
            double td;
            if (type == 4) {                          // (Delta*H)(i,r)  (:925)
              td = 0.0;
#pragma unroll
              for (int c = 0; c < RMAX; ++c)
                if (c < q) td += d[c] * Hsh[c + q * r];
            } else {
              td = d[r];                              // :647
            }
            double v = m.Aeff[i + rows * r] + rh * (td - m.muD[i + rows * r]);
            if (m.constrained) v += rh * (m.Z[i + rows * r] - m.mu[i + rows * r]);
            x[r] = v;
          }
        }
#pragma unroll
        for (int r = 0; r < RMAX; ++r)                // x * inv(L*L')  (:651, :929)
          if (r < R) {
            double v = x[r];
#pragma unroll
            for (int p = 0; p < RMAX; ++p)
              if (p < r) v -= Lsh[r + R * p] * x[p];
            x[r] = v / Lsh[r + R * r];
          }
#pragma unroll
        for (int r = RMAX - 1; r >= 0; --r)
          if (r < R) {
            double v = x[r];
#pragma unroll
            for (int p = 0; p < RMAX; ++p)
              if (p > r && p < R) v -= Lsh[p + R * r] * x[p];
            x[r] = v / Lsh[r + R * r];
          }
#pragma unroll
        for (int r = 0; r < RMAX; ++r)
          if (r < R) m.fac[i + rows * r] = x[r];
      }
      // ---- Delta
      double bb[RMAX];
#pragma unroll
      for (int c = 0; c < RMAX; ++c) bb[c] = 0.0;
      for (int j = 0; j < a.n; ++j) {
        const WgLoopMode& m = a.m[j];
        if (type == 4) {
          const double rj = m.rho[0];
          double tt[RMAX];
#pragma unroll
          for (int r = 0; r < RMAX; ++r) tt[r] = r < m.R ? m.fac[i + rows * r] + m.muD[i + rows * r] : 0.0;
          const double* Hj = sh + offH[j];
#pragma unroll
          for (int c = 0; c < RMAX; ++c)
            if (c < q) {
              double acc = 0.0;
#pragma unroll
              for (int r = 0; r < RMAX; ++r)
                if (r < m.R) acc += tt[r] * Hj[c + q * r];
              bb[c] = (j == 0 ? 0.0 : bb[c]) + rj * acc;                           // :955
            }
        } else {
          const double cj = a.coefs[j];               // rho_j / sum rho
#pragma unroll
          for (int c = 0; c < RMAX; ++c)
            if (c < q) {
              const double v = cj * m.fac[i + rows * c] + cj * m.muD[i + rows * c];
              bb[c] = j == 0 ? v : bb[c] + v;
            }
        }
      }
      if (type == 4) {                                // Delta(i,:) = bb * inv(LAA*LAA')
        const double* Lsh = sh;
#pragma unroll
        for (int c = 0; c < RMAX; ++c)
          if (c < q) {
            double v = bb[c];
#pragma unroll
            for (int p = 0; p < RMAX; ++p)
              if (p < c) v -= Lsh[c + q * p] * bb[p];
            bb[c] = v / Lsh[c + q * c];
          }
#pragma unroll
        for (int c = RMAX - 1; c >= 0; --c)
          if (c < q) {
            double v = bb[c];
#pragma unroll
            for (int p = 0; p < RMAX; ++p)
              if (p > c && p < q) v -= Lsh[p + q * c] * bb[p];
            bb[c] = v / Lsh[c + q * c];
          }
      }
      double dd[RMAX];
#pragma unroll
      for (int c = 0; c < RMAX; ++c) {
        dd[c] = 0.0;
        if (c < q) {
          a.DeltaOld[i + rows * c] = d[c];
          a.Delta[i + rows * c] = bb[c];
          dd[c] = bb[c] - d[c];
          a.dD[i + rows * c] = dd[c];
        }
      }
      // ---- coupling duals, constraints, residual sums
      for (int j = 0; j < a.n; ++j) {
        const WgLoopMode& m = a.m[j];
        const int R = m.R;
        const double* Hsh = sh + offH[j];
        double f[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
          f[r] = 0.0;
          if (r < R) {
            double td, tdd;
            if (type == 4) {
              td = 0.0; tdd = 0.0;
#pragma unroll
              for (int c = 0; c < RMAX; ++c)
                if (c < q) { td += bb[c] * Hsh[c + q * r]; tdd += dd[c] * Hsh[c + q * r]; }
            } else { td = bb[r]; tdd = dd[r]; }
            f[r] = m.fac[i + rows * r];
            const double g = f[r] - td;
            const double mm = m.muD[i + rows * r] + g;                              // :679, :967
            m.muD[i + rows * r] = mm;
            sums[j][4] += g * g; sums[j][5] += mm * mm; sums[j][6] += tdd * tdd; sums[j][7] += f[r] * f[r];
          }
        }
        if (m.constrained) {                          // update_constraint (:1420-1429)
          const double rho = m.rho[0];
          double zo[RMAX], mu[RMAX], z[RMAX];
#pragma unroll
          for (int r = 0; r < RMAX; ++r) {
            zo[r] = r < R ? m.Z[i + rows * r] : 0.0;
            mu[r] = r < R ? m.mu[i + rows * r] : 0.0;
            z[r] = f[r] + mu[r];
          }
          if (m.ptype == AOADMM_C_SIMPLEX_ROW) {
            simplex_regs<RMAX>(z, R, m.p0);
          } else {
#pragma unroll
            for (int r = 0; r < RMAX; ++r) z[r] = prox_elem(m.ptype, z[r], m.p0, m.p1, rho);
          }
#pragma unroll
          for (int r = 0; r < RMAX; ++r)
            if (r < R) {
              const double mn = mu[r] + f[r] - z[r];
              m.Zold[i + rows * r] = zo[r];
              m.Z[i + rows * r] = z[r];
              m.mu[i + rows * r] = mn;
              const double dz = z[r] - zo[r];
              sums[j][0] += (f[r] - z[r]) * (f[r] - z[r]); sums[j][1] += f[r] * f[r]; sums[j][2] += mn * mn; sums[j][3] += dz * dz;
            }
        } else {
#pragma unroll
          for (int r = 0; r < RMAX; ++r) sums[j][1] += f[r] * f[r];
        }
      }
    }
    // ---- the workgroup's sums (fixed order: lanes by DPP tree, then the four waves in order)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double v = wave_sum(sums[j][k]);
        if (lane == 0) red[w][j * 8 + k] = v;
      }
    __syncthreads();
    if (t < 32) {
      const double tot = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
      red[0][t] = tot;
      const int j = t >> 3;
      if (j < a.n) a.m[j].slots[t & 7] = tot;
    }
    __syncthreads();
    if (t == 0) {                                     // eval_res_ADMM_coupl_case0/4 + eval_res_ADMM_constr, while condition
      double prc = 0, duc = 0, prz = 0, duz = 0;
      int nz = 0;
      for (int j = 0; j < a.n; ++j) {
        const double* sj = &red[0][j * 8];
        prc += sqrt(sj[4]) / sqrt(sj[7]);
        const double sc = sqrt(sj[5]);
        duc += sc > 0 ? sqrt(sj[6]) / sc : sqrt(sj[6]);
        if (a.m[j].constrained) {
          prz += sqrt(sj[0]) / sqrt(sj[1]);
          const double sz = sqrt(sj[2]);
          duz += sz > 0 ? sqrt(sj[3]) / sz : sqrt(sj[3]);
          ++nz;
        }
      }
      prc /= a.n; duc /= a.n;
      if (nz) { prz /= nz; duz /= nz; }
      ++it;
      a.ctl->res[0] = prc; a.ctl->res[1] = prz; a.ctl->res[2] = duc; a.ctl->res[3] = duz;
      a.ctl->iters = it;
      const int cont = (it < a.max_inner && (prc > a.tol_pr_coupl || prz > a.tol_pr_constr || duc > a.tol_du_coupl ||
                                             duz > a.tol_du_constr)) ? 1 : 0;
      a.ctl->active = cont;
      go = cont;
    }
    __syncthreads();
  }
}

// Register-resident form of couple_loop_wg_k for rows <= 256 (one row per thread) and NM coupled modes: the rows of A,
// fac, mu_Delta, Z, mu of every coupled mode and the row of Delta are loaded once, live in registers for the whole
// loop and are stored once.  An inner iteration is then arithmetic plus one workgroup reduction, with no memory round
// trip (the global-memory form re-reads its own stores from L2 several times per iteration: 25 us per iteration
// against a few us here at 50 rows x 4 columns).
// Everything is padded to RMAX with zeros -- the small matrices in LDS (L_j, H_j, L_AA as RMAX x RMAX blocks), the
// reciprocal diagonals (0 beyond the rank) and the register rows -- so the loop body is straight-line code: a padded
// column contributes exact zeros to every sum and is never stored.  (The first version tested `r < R` and `c < q` at
// every step: ~5000 instructions, 700 of them branches, 10 us per inner iteration; PMC: 15 cycles per instruction on
// the one wave per SIMD.)  T4: coupling type 4 (C = Delta*H), else type 0 (C = Delta).
template <int RMAX, int NM, bool T4>
__global__ __launch_bounds__(256) void couple_loop_wg_regs_k(WgLoopArgs a) {
  constexpr int RR = RMAX * RMAX;
  __shared__ double Lsh[NM][RR];                      // L_j, column-major with leading dimension RMAX
  __shared__ double Hsh[NM][RR];                      // H_j(c, r) at c + RMAX*r
  __shared__ double LAAsh[RR];
  __shared__ double red[4][8 * NM];
  __shared__ double invd[NM + 1][RMAX];               // reciprocal diagonals of L_j and of LAA: the substitutions multiply
  __shared__ int go;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int q = a.q;
  const int64_t rows = a.rows;
  const int64_t i = t;
  const bool have = i < rows;
  const int64_t ic = have ? i : rows - 1;             // clamped: padding threads compute on a valid row, store nothing
  for (int e = t; e < RR; e += 256) {
    const int r = e % RMAX, c = e / RMAX;
    LAAsh[e] = (T4 && r < q && c < q) ? a.LAA[r + q * c] : 0.0;
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int R = a.m[j].R;
      Lsh[j][e] = (r < R && c < R) ? a.m[j].L[r + R * c] : 0.0;
      Hsh[j][e] = (T4 && r < q && c < R) ? a.m[j].H[r + q * c] : 0.0;
    }
  }
  __syncthreads();
  if (t < RMAX) {
#pragma unroll
    for (int j = 0; j < NM; ++j) invd[j][t] = t < a.m[j].R ? 1.0 / Lsh[j][t + RMAX * t] : 0.0;
    invd[NM][t] = (T4 && t < q) ? 1.0 / LAAsh[t + RMAX * t] : 0.0;
  }
  double d[RMAX], av[NM][RMAX], f[NM][RMAX], md[NM][RMAX], z[NM][RMAX], mu[NM][RMAX], zo[NM][RMAX], rh[NM], rho[NM], cj[NM];
  ElemProx ep[NM];
#pragma unroll
  for (int c = 0; c < RMAX; ++c) d[c] = c < q ? a.Delta[ic + rows * c] : 0.0;
#pragma unroll
  for (int j = 0; j < NM; ++j) {
    const WgLoopMode& m = a.m[j];
    rho[j] = m.rho[0];
    rh[j] = rho[j] / 2;
    cj[j] = (T4 || a.self_start) ? 0.0 : a.coefs[j];  // rho_j / sum rho
    ep[j] = elem_prox_of(m.ptype, m.p0, m.p1, rho[j]);
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const bool ok = r < m.R;
      const int64_t o = ic + rows * (ok ? r : 0);
      av[j][r] = ok ? m.Aeff[o] : 0.0;
      f[j][r] = ok ? m.fac[o] : 0.0;
      md[j][r] = ok ? m.muD[o] : 0.0;
      z[j][r] = (ok && m.constrained) ? m.Z[o] : 0.0;
      mu[j][r] = (ok && m.constrained) ? m.mu[o] : 0.0;
      zo[j][r] = z[j][r];
    }
  }
  if (!T4 && a.self_start) {                          // coupling_coefs_k's arithmetic: 1 / sum(rho) * rho_j, modes in order
    double srho = 0.0;
#pragma unroll
    for (int j = 0; j < NM; ++j) srho += rho[j];
#pragma unroll
    for (int j = 0; j < NM; ++j) cj[j] = 1.0 / srho * rho[j];
  }
  double dold[RMAX], dd[RMAX];
#pragma unroll
  for (int c = 0; c < RMAX; ++c) { dold[c] = d[c]; dd[c] = 0.0; }
  if (t == 0) go = a.self_start ? 1 : a.ctl->active;
  __syncthreads();
  int it = 0;
  bool ran = false;
  while (go) {
    ran = true;
    double sums[NM][8];
#pragma unroll
    for (int j = 0; j < NM; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) sums[j][k] = 0.0;
    // ---- primal updates
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const WgLoopMode& m = a.m[j];
      double x[RMAX];
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        double td;
        if (T4) {                                     // (Delta*H)(i,r)  (:925)
          td = 0.0;
#pragma unroll
          for (int c = 0; c < RMAX; ++c) td += d[c] * Hsh[j][c + RMAX * r];
        } else {
          td = d[r];                                  // :647
        }
        double v = av[j][r] + rh[j] * (td - md[j][r]);
        if (m.constrained) v += rh[j] * (z[j][r] - mu[j][r]);
        x[r] = v;
      }
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {                // x * inv(L*L')  (:651, :929)
        double v = x[r];
#pragma unroll
        for (int p = 0; p < r; ++p) v -= Lsh[j][r + RMAX * p] * x[p];
        x[r] = v * invd[j][r];
      }
#pragma unroll
      for (int r = RMAX - 1; r >= 0; --r) {
        double v = x[r];
#pragma unroll
        for (int p = r + 1; p < RMAX; ++p) v -= Lsh[j][p + RMAX * r] * x[p];
        x[r] = v * invd[j][r];
      }
#pragma unroll
      for (int r = 0; r < RMAX; ++r) f[j][r] = x[r];
    }
    // ---- Delta
    double bb[RMAX];
#pragma unroll
    for (int c = 0; c < RMAX; ++c) bb[c] = 0.0;
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      if (T4) {
#pragma unroll
        for (int c = 0; c < RMAX; ++c) {
          double acc = 0.0;
#pragma unroll
          for (int r = 0; r < RMAX; ++r) acc += (f[j][r] + md[j][r]) * Hsh[j][c + RMAX * r];
          bb[c] = (j == 0 ? 0.0 : bb[c]) + rho[j] * acc;                           // :955
        }
      } else {
#pragma unroll
        for (int c = 0; c < RMAX; ++c) {
          const double v = cj[j] * f[j][c] + cj[j] * md[j][c];
          bb[c] = j == 0 ? v : bb[c] + v;
        }
      }
    }
    if (T4) {                                         // Delta(i,:) = bb * inv(LAA*LAA')
#pragma unroll
      for (int c = 0; c < RMAX; ++c) {
        double v = bb[c];
#pragma unroll
        for (int p = 0; p < c; ++p) v -= LAAsh[c + RMAX * p] * bb[p];
        bb[c] = v * invd[NM][c];
      }
#pragma unroll
      for (int c = RMAX - 1; c >= 0; --c) {
        double v = bb[c];
#pragma unroll
        for (int p = c + 1; p < RMAX; ++p) v -= LAAsh[p + RMAX * c] * bb[p];
        bb[c] = v * invd[NM][c];
      }
    }
#pragma unroll
    for (int c = 0; c < RMAX; ++c) {
      const double nv = (T4 || c < q) ? bb[c] : 0.0;  // type 0: columns beyond q carry nothing
      dold[c] = d[c];
      dd[c] = nv - d[c];
      d[c] = nv;
    }
    // ---- coupling duals, constraints, residual sums
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const WgLoopMode& m = a.m[j];
      const int R = m.R;
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        double td, tdd;
        if (T4) {
          td = 0.0; tdd = 0.0;
#pragma unroll
          for (int c = 0; c < RMAX; ++c) { td += d[c] * Hsh[j][c + RMAX * r]; tdd += dd[c] * Hsh[j][c + RMAX * r]; }
        } else { td = r < R ? d[r] : 0.0; tdd = r < R ? dd[r] : 0.0; }
        const double g = f[j][r] - td;
        const double mm = md[j][r] + g;                                             // :679, :967
        md[j][r] = mm;
        if (have) { sums[j][4] += g * g; sums[j][5] += mm * mm; sums[j][6] += tdd * tdd; sums[j][7] += f[j][r] * f[j][r]; }
      }
      if (m.constrained) {                            // update_constraint (:1420-1429)
        double zn[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) { zo[j][r] = z[j][r]; zn[r] = f[j][r] + mu[j][r]; }
        if (m.ptype == AOADMM_C_SIMPLEX_ROW) {
          simplex_regs<RMAX>(zn, R, m.p0);
        } else {
#pragma unroll
          for (int r = 0; r < RMAX; ++r) zn[r] = r < R ? elem_prox(ep[j], zn[r]) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
          const double mn = mu[j][r] + f[j][r] - zn[r];
          const double dz = zn[r] - zo[j][r];
          if (have) {
            sums[j][0] += (f[j][r] - zn[r]) * (f[j][r] - zn[r]); sums[j][1] += f[j][r] * f[j][r]; sums[j][2] += mn * mn;
            sums[j][3] += dz * dz;
          }
          z[j][r] = zn[r];
          mu[j][r] = mn;
        }
      } else if (have) {
#pragma unroll
        for (int r = 0; r < RMAX; ++r) sums[j][1] += f[j][r] * f[j][r];
      }
    }
    // ---- the workgroup's sums (fixed order: lanes by DPP tree, then the four waves in order)
#pragma unroll
    for (int j = 0; j < NM; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double v = wave_sum(sums[j][k]);
        if (lane == 0) red[w][j * 8 + k] = v;
      }
    __syncthreads();
    if (t < 8 * NM) {
      const double tot = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
      red[0][t] = tot;
      a.m[t >> 3].slots[t & 7] = tot;
    }
    __syncthreads();
    // eval_res_ADMM_coupl_case0/4 + eval_res_ADMM_constr: the 4*NM ratios (two square roots and a division each, ~100
    // dependent fp64 instructions) on 4*NM lanes side by side, then one lane adds them in mode order and decides --
    // the whole workgroup waits for this
    if (t < 4 * NM) {
      const int j = t >> 2, which = t & 3;            // 0: primal coupling, 1: dual coupling, 2: primal constr., 3: dual constr.
      const double* sj = &red[0][j * 8];
      double v;
      if (which == 0) v = sqrt(sj[4]) / sqrt(sj[7]);
      else if (which == 2) v = sqrt(sj[0]) / sqrt(sj[1]);
      else {
        const double num = sqrt(which == 1 ? sj[6] : sj[3]), sc = sqrt(which == 1 ? sj[5] : sj[2]);
        v = sc > 0 ? num / sc : num;
      }
      red[1][t] = v;
    }
    __syncthreads();
    if (t == 0) {                                     // while condition
      double prc = 0, duc = 0, prz = 0, duz = 0;
      int nz = 0;
      for (int j = 0; j < NM; ++j) {
        prc += red[1][4 * j];
        duc += red[1][4 * j + 1];
        if (a.m[j].constrained) {
          prz += red[1][4 * j + 2];
          duz += red[1][4 * j + 3];
          ++nz;
        }
      }
      prc /= NM; duc /= NM;
      if (nz) { prz /= nz; duz /= nz; }
      ++it;
      a.ctl->res[0] = prc; a.ctl->res[1] = prz; a.ctl->res[2] = duc; a.ctl->res[3] = duz;
      a.ctl->iters = it;
      const int cont = (it < a.max_inner && (prc > a.tol_pr_coupl || prz > a.tol_pr_constr || duc > a.tol_du_coupl ||
                                             duz > a.tol_du_constr)) ? 1 : 0;
      a.ctl->active = cont;
      go = cont;
    }
    __syncthreads();
  }
  if (!ran || !have) return;
#pragma unroll
  for (int c = 0; c < RMAX; ++c)
    if (c < q) { a.Delta[i + rows * c] = d[c]; a.DeltaOld[i + rows * c] = dold[c]; a.dD[i + rows * c] = dd[c]; }
#pragma unroll
  for (int j = 0; j < NM; ++j) {
    const WgLoopMode& m = a.m[j];
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
      if (r < m.R) {
        const int64_t o = i + rows * r;
        m.fac[o] = f[j][r];
        m.muD[o] = md[j][r];
        if (m.constrained) { m.Z[o] = z[j][r]; m.mu[o] = mu[j][r]; m.Zold[o] = zo[j][r]; }
      }
  }
}

template <int RMAX>
static void launch_loop_regs(const WgLoopArgs& a, hipStream_t s) {
  auto go = [&](auto nm) {
    if (a.type == 4) couple_loop_wg_regs_k<RMAX, decltype(nm)::value, true><<<1, 256, 0, s>>>(a);
    else couple_loop_wg_regs_k<RMAX, decltype(nm)::value, false><<<1, 256, 0, s>>>(a);
  };
  if (a.n == 1) go(std::integral_constant<int, 1>());
  else if (a.n == 2) go(std::integral_constant<int, 2>());
  else go(std::integral_constant<int, 3>());
}
void couple_loop_one_launch(const WgLoopArgs& a, CouplePath path, int rmax, hipStream_t s) {
  if (path == CouplePath::Regs) {
    if (couple_rank_class(rmax) == 4) launch_loop_regs<4>(a, s);
    else launch_loop_regs<8>(a, s);
  } else {
    size_t lds = (size_t)a.q * a.q;                   // LAA | per mode: L, H
    for (int j = 0; j < a.n; ++j) lds += (size_t)a.m[j].R * a.m[j].R + (size_t)a.q * a.m[j].R;
    by_rmax(rmax, [&](auto tag) { couple_loop_wg_k<decltype(tag)::value><<<1, 256, lds * sizeof(double), s>>>(a); });
  }
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
