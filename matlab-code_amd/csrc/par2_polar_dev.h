// The polar factor of one PARAFAC2 slab on one wave, shared by the B_k loop (par2.hip) and the fold-in of new slabs
// (par2_foldin.hip).  See par2.h.
#pragma once
#include "par2.h"

#include "device_utils.h"

namespace aoadmm {

static constexpr int kP2Threads = 64;

// P_k = U*V' of svd(W_k,'econ') (:532-534) by one-sided (Hestenes) Jacobi: W*Jrot has orthogonal
// columns, U = W*Jrot/sigma, V = Jrot.  One wave per slab: the three column products of a pair are reduced by a
// butterfly over the 64 lanes, which leaves bit-identical sums in every lane, so each lane derives the rotation
// itself and nothing is exchanged through memory.  W_k is staged in LDS when it fits (in_lds), else rotated in place.
static_assert(kP2Threads == 64, "par2_polar_dev reduces over exactly one wavefront");
__device__ inline double wave_sum64(double v) { return wave_sum(v); }   // DPP tree (device_utils.h), the same bits in every lane
__device__ __forceinline__ void par2_polar_dev(double* W, double* P, const P2Dims& d, int k, int in_lds, double* Jr,
                                              double* Jwarm = nullptr, int warm_valid = 0) {
  const int R = d.R, lane = threadIdx.x;  // Jr: R*R, then W_k (n*R) when in_lds
  const int64_t o = d.off[k];
  const int n = (int)(d.off[k + 1] - o);
  double* Pk = P + o * R;
  double* Wk = W + o * R;
  if (in_lds) {
    double* Wl = Jr + R * R;
    for (int e = lane; e < n * R; e += 64) Wl[e] = Wk[e];
    Wk = Wl;
  }
  const bool warm = Jwarm != nullptr && warm_valid && in_lds;   // needs the untouched copy in global memory as source
  for (int e = lane; e < R * R; e += 64) Jr[e] = warm ? Jwarm[(int64_t)k * R * R + e] : ((e % R == e / R) ? 1.0 : 0.0);
  __syncthreads();
  if (warm) {
    // W <- W * J_prev, row by row (each lane owns its rows): the columns are almost orthogonal before the first sweep
    const double* Wg = W + o * R;                      // the slab as the primal step left it
    for (int e = lane; e < n * R; e += 64) {
      const int i = e % n, p = e / n;
      double acc = 0.0;
      for (int q = 0; q < R; ++q) acc += Wg[i + n * q] * Jr[q + R * p];
      Wk[e] = acc;
    }
    __syncthreads();
  }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < R - 1; ++p)
      for (int q = p + 1; q < R; ++q) {
        double* wp = Wk + n * p;
        double* wq = Wk + n * q;
        double al = 0, be = 0, ga = 0;
        for (int i = lane; i < n; i += 64) { al += wp[i] * wp[i]; be += wq[i] * wq[i]; ga += wp[i] * wq[i]; }
        al = wave_sum64(al); be = wave_sum64(be); ga = wave_sum64(ga);
        if (ga != 0.0 && fabs(ga) > 1e-15 * sqrt(al * be)) {           // uniform over the wave
          const double zeta = (be - al) / (2.0 * ga);
          const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t);
          const double sn = c * t;
          rotated = true;
          for (int i = lane; i < n; i += 64) {
            const double x = wp[i], y = wq[i];
            wp[i] = c * x - sn * y;
            wq[i] = sn * x + c * y;
          }
          for (int i = lane; i < R; i += 64) {
            const double x = Jr[i + R * p], y = Jr[i + R * q];
            Jr[i + R * p] = c * x - sn * y;
            Jr[i + R * q] = sn * x + c * y;
          }
        }
      }
    if (!rotated) break;
  }
  for (int p = 0; p < R; ++p) {
    double* wp = Wk + n * p;
    double al = 0;
    for (int i = lane; i < n; i += 64) al += wp[i] * wp[i];
    const double sg = sqrt(wave_sum64(al));
    for (int i = lane; i < n; i += 64) wp[i] = sg > 0 ? wp[i] / sg : 0.0;
  }
  __syncthreads();
  if (Jwarm != nullptr)
    for (int e = lane; e < R * R; e += 64) Jwarm[(int64_t)k * R * R + e] = Jr[e];
  for (int e = lane; e < n * R; e += 64) {
    const int i = e % n, r = e / n;
    double acc = 0.0;
    for (int q = 0; q < R; ++q) acc += Wk[i + n * q] * Jr[r + R * q];
    Pk[e] = acc;
  }
}

}  // namespace aoadmm
