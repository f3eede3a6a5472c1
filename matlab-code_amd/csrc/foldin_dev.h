// Fold-in, device side: the normal equations per (query, chunk) on the matrix pipe and the one-wave solve, shared by the
// unweighted instantiations (foldin.hip) and the weighted ones (foldin_w.hip).  See foldin.h and DESIGN.md section 9.6.
//
// Normal equations: v_mfma_f64_16x16x4_f64 with the operand map of topk_scores_k.  In a step of four observations lane
// (c = l & 15, q4 = l >> 4) holds z_e(c + 16 t) of observation e = 4 s + q4 for every column tile t.  That one register is
// A[row c][k = q4] of tile row t and B[k = q4][col c] of tile column t, so G tile (ti, tj) takes mfma(z[ti], z[tj], acc)
// and lane l receives G(16 ti + q4 + 4 r, 16 tj + c) in register r (the fp64 C/D map: col = lane & 15, row =
// (lane >> 4) + 4 reg).  Only tiles ti <= tj are accumulated; a diagonal tile is symmetric to the bit (both triangles sum
// the same products in the same order) and the others are mirrored.  b takes T more MFMAs against a B operand that holds
// x_e in column 0.  Observations beyond the chunk and columns beyond R enter as zero operands: an entry of G is one chain
// of MFMAs over the steps of its chunk from +0.
//
// Weighted (WT): the A operand of tile row ti is (w_e - alpha) z[ti], rounded once, the B operand stays z[tj], and b
// multiplies z against w_e x_e.  Entry (i, j) with i <= j is the chain of ((w_e - alpha) z_e(i)) * z_e(j); in a diagonal
// tile the entries below the diagonal are dropped and (i, j) is mirrored, so the image is symmetric to the bit.  alpha H
// is added once per query, as fma(alpha, H(i, j), S(i, j)), after the stored part S is complete: in the launch that
// accumulated a query of one chunk, or after the partials (the stored part only) have been summed in chunk order.
//
// Solve: lane t keeps row t of G + shift I in registers (right-looking Cholesky with readlane broadcasts, as
// small_dev.h); L goes through LDS once so that lane t also holds column t, which makes both substitutions a chain of
// readlane broadcasts; the row ADMM loop for non-negativity runs on the wave with butterfly norms and a uniform exit.
#pragma once
#include "foldin.h"
#include "small_dev.h"

namespace aoadmm {

typedef double fold_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kFoldWave = 64;
constexpr int kFoldUnroll = 4;       // steps whose gathers are in flight together (twice as many up to R = 32; weighted: up to R = 16)

struct FoldKArgs {
  CooFactor f[kCooMaxModes - 1];     // the other modes' factors in mode order
  int nm, R;
  int64_t nq, nobs;
  double ridge, tol_primal, tol_dual;
  int constraint, max_inner;
  const int* idx;
  const double* val;
  const int64_t* qoff;
  const int* item_q;
  const int* item_chunk;
  const int64_t* pbase;
  const int* split_q;
  double* partial;
  double* rows;
  int* info;
  int* iters;
  double* gram;
  double* rhs;
};
// what the weighted instantiations take on top; the unweighted kernels keep the arguments they always had
struct FoldKArgsW : FoldKArgs {
  const double* wt;                  // sorted list beside val; null: all ones
  double alpha;                      // the weight of an unlisted cell
  const double* H;                   // R x R, had_{m != mode} F_m'F_m; read when alpha != 0
};
template <bool WT> struct FoldKArgsOf { typedef FoldKArgs type; };
template <> struct FoldKArgsOf<true> { typedef FoldKArgsW type; };

// every lane receives the same bits: each stage adds the two halves of a pair in both lanes
__device__ __forceinline__ double fold_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One query on one full wave.  Gs: the R x R normal matrix in LDS, column-major with leading dimension 16 T (both
// triangles); bs: its right-hand side.  Writes the query's outputs.  Gs is overwritten by L.
template <int T>
__device__ __forceinline__ void foldin_solve_dev(double* Gs, const double* bs, int64_t q, const FoldKArgs& a) {
  constexpr int RP = kFoldTile * T;
  const int R = a.R, t = (int)threadIdx.x;
  const bool mine = t < R;
  if (a.gram != nullptr) {
    double* g = a.gram + q * (int64_t)R * R;
    for (int i = t; i < R * R; i += kFoldWave) g[i] = Gs[(i % R) + RP * (i / R)];
  }
  const double bt = mine ? bs[mine ? t : 0] : 0.0;
  if (a.rhs != nullptr && mine) a.rhs[q + a.nq * t] = bt;

  double row[RP];                                // row t of G, then of G + shift I, then of L
#pragma unroll
  for (int c = 0; c < RP; ++c) {
    const double g = Gs[(mine ? t : 0) + RP * (c < R ? c : 0)];
    row[c] = mine && c < R ? g : 0.0;
  }
  double tr = 0.0;                               // the diagonal summed in index order by every lane
#pragma unroll
  for (int r = 0; r < RP; ++r)
    if (r < R) tr += readlane_d(row[r], r);
  const double rho = a.constraint == 1 ? tr / R : 0.0;
  const double shift = a.constraint == 1 ? a.ridge + rho / 2 : a.ridge;
#pragma unroll
  for (int c = 0; c < RP; ++c)
    if (c == t && mine) row[c] += shift;

  bool ok = true;
  double myinv = 0.0;                            // 1 / L(t, t)
#pragma unroll
  for (int j = 0; j < RP; ++j) {
    if (j < R && ok) {
      const double d = readlane_d(row[j], j);
      if (!(d > 0.0)) {
        ok = false;
      } else {
        const double inv = rsqrt(d);
        const double dj = d * inv;
        const double lij = row[j] * inv;
        row[j] = (t == j) ? dj : lij;
        if (t == j) myinv = inv;
#pragma unroll
        for (int k = j + 1; k < RP; ++k)
          if (k < R) row[k] -= lij * readlane_d(lij, k);
      }
    }
  }

  // column t of L beside row t: L(j, t) for j > t
  __syncthreads();
  if (mine) {
#pragma unroll
    for (int k = 0; k < RP; ++k)
      if (k <= t) Gs[t + RP * k] = row[k];
  }
  __syncthreads();
  double col[RP];
#pragma unroll
  for (int j = 0; j < RP; ++j) {
    const double l = Gs[(j < R ? j : 0) + RP * (mine ? t : 0)];
    col[j] = mine && j < R && j > t ? l : 0.0;
  }

  // L L' u = rhs with one entry per lane: the forward substitution broadcasts y_j and lane t > j subtracts L(t, j) y_j,
  // the backward one broadcasts u_j and lane t < j subtracts L(j, t) u_j
  auto solve = [&](double v) {
    double y = 0.0;
#pragma unroll
    for (int j = 0; j < RP; ++j) {
      if (j < R) {
        const double yj = readlane_d(v * myinv, j);
        if (t == j) y = yj;
        if (t > j) v -= row[j] * yj;
      }
    }
    double u = 0.0;
#pragma unroll
    for (int j = RP - 1; j >= 0; --j) {
      if (j < R) {
        const double uj = readlane_d(y * myinv, j);
        if (t == j) u = uj;
        if (t < j) y -= col[j] * uj;
      }
    }
    return u;
  };

  // One call site for the solve: without a constraint rho = 0 and z = mu = 0, so the first system is (G + ridge I) u = b
  // and the loop is left after it.
  double out = 0.0;
  int it = 0;
  if (ok) {
    double zc = 0.0, mu = 0.0;
    double rp, rd;
    do {
      const double u = solve(bt + rho / 2 * (zc - mu));   // a lane beyond R holds zeros throughout
      out = u;
      if (a.constraint == 0) break;              // uniform
      const double zold = zc;
      const double s = u + mu;
      zc = s > 0.0 ? s : (s == s ? 0.0 : s);     // max(s, 0), a NaN stays
      mu = (mu + u) - zc;
      const double nu = sqrt(fold_wave_sum(u * u));
      const double npr = sqrt(fold_wave_sum((u - zc) * (u - zc)));
      const double ndu = sqrt(fold_wave_sum((zc - zold) * (zc - zold)));
      const double nmu = sqrt(fold_wave_sum(mu * mu));
      rp = npr / nu;
      rd = nmu > 0.0 ? ndu / nmu : ndu;         // unscaled when the dual is zero, as the reference
      out = zc;                                  // the feasible row
      ++it;
    } while (it < a.max_inner && (rp > a.tol_primal || rd > a.tol_dual));   // uniform: every lane holds the same norms
  }
  if (mine) a.rows[q + a.nq * t] = ok ? out : __builtin_nan("");
  if (t == 0) {
    a.info[q] = ok ? 0 : 1;
    a.iters[q] = it;
  }
}

// The normal equations of one work item (sum_partials = 0: accumulated from its chunk) or of one split query
// (sum_partials = 1: its partials summed in chunk order from +0) as the LDS image the solve reads.  Returns the query to
// solve, or -1 when the work item was one chunk of a longer query and left its partial in the workspace.  T = ceil(R / 16)
// column tiles, compiled in.  WT: entry weights and the weight of the unlisted cells (the head of this file).  The weighted
// R <= 32 class keeps four steps in flight, not eight: with eight it needs 218 + 40 registers, two over what two waves per
// SIMD can have, and the pass takes 1.6 times as long; with four it takes 166.
template <int T, bool WT>
__device__ __forceinline__ int64_t foldin_normal_dev(const typename FoldKArgsOf<WT>::type& a, int sum_partials, double* Gs, double* bs) {
  constexpr int RP = kFoldTile * T, NT = T * (T + 1) / 2, U = (WT ? T <= 1 : T <= 2) ? 2 * kFoldUnroll : kFoldUnroll;
  const int lane = (int)threadIdx.x, c = lane & 15, q4 = lane >> 4;
  const int R = a.R;
  const int64_t PD = (int64_t)R * R + R;
  bool unlisted = false;                         // uniform: alpha H joins the stored part
  if constexpr (WT) unlisted = a.alpha != 0.0;
  if (sum_partials != 0) {                       // uniform: the partials of a split query in chunk order from +0
    const int64_t q = a.split_q[blockIdx.x];
    const int64_t nall = a.qoff[q + 1] - a.qoff[q];
    const int64_t chunks = (nall + kFoldChunk - 1) / kFoldChunk;
    const double* P = a.partial + a.pbase[q] * PD;
    for (int i = lane; i < (int)PD; i += kFoldWave) {
      double sum = 0.0;
#pragma unroll 8
      for (int64_t ch = 0; ch < chunks; ++ch) sum += P[ch * PD + i];   // (unrolled: the loads of eight chunks in flight)
      if (i < R * R) {
        if constexpr (WT)
          if (unlisted) sum = fma(a.alpha, a.H[i], sum);
        Gs[(i % R) + RP * (i / R)] = sum;
      } else {
        bs[i - R * R] = sum;
      }
    }
    __syncthreads();
    return q;
  }
  const int64_t q = a.item_q[blockIdx.x];
  const int chunk = a.item_chunk[blockIdx.x];
  const int64_t e0 = a.qoff[q] + (int64_t)chunk * kFoldChunk;
  const int64_t qe = a.qoff[q + 1];
  const int n = (int)((qe - e0 < kFoldChunk) ? qe - e0 : kFoldChunk);   // 0 for a query without observations
  const int steps = (n + 3) / 4;

  fold_f64x4 acc[NT], bacc[T];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = fold_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < T; ++k) bacc[k] = fold_f64x4{0.0, 0.0, 0.0, 0.0};

  for (int s0 = 0; s0 < steps; s0 += U) {
    // Unconditional loads on clamped addresses (an observation of this chunk, a column below R); what a clamp brought in
    // is dropped where it is used.
    double z[U][T], x[U];
    [[maybe_unused]] double wa[WT ? U : 1];
    int64_t ec[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = 4 * (s0 + u) + q4;
      live[u] = e < n;
      ec[u] = e0 + (live[u] ? e : 0);
      x[u] = a.val[ec[u]];
      if constexpr (WT) wa[u] = a.wt != nullptr ? a.wt[ec[u]] : 1.0;   // uniform
#pragma unroll
      for (int t = 0; t < T; ++t) z[u][t] = 1.0;
    }
    // every mode's subscripts first, then every mode's rows: two memory round trips per U steps whatever the order
    int ix[kCooMaxModes - 1][U];
#pragma unroll
    for (int m = 0; m < kCooMaxModes - 1; ++m) {
      if (m < a.nm) {                            // uniform
        const int* im = a.idx + (int64_t)m * a.nobs;
#pragma unroll
        for (int u = 0; u < U; ++u) ix[m][u] = im[ec[u]];
      }
    }
    if constexpr (WT) {                          // w x and w - alpha while the subscripts are on their way
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u] = wa[u] * x[u];
        wa[u] = wa[u] - a.alpha;
      }
    }
#pragma unroll
    for (int m = 0; m < kCooMaxModes - 1; ++m) {
      if (m < a.nm) {                            // uniform
        const CooFactor F = a.f[m];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const double* fp = F.p + (int64_t)ix[m][u] * F.sI;
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const int cc = c + kFoldTile * t;
            z[u][t] *= fp[(int64_t)(cc < R ? cc : R - 1) * F.sR];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s0 + u < steps) {                      // uniform
        double zz[T];
#pragma unroll
        for (int t = 0; t < T; ++t) zz[t] = live[u] && c + kFoldTile * t < R ? z[u][t] : 0.0;
        const double xx = live[u] && c == 0 ? x[u] : 0.0;
        int k = 0;
        if constexpr (WT) {                      // the scaled operand of one tile row at a time, just before its MFMAs
#pragma unroll
          for (int ti = 0; ti < T; ++ti) {
            const double za = live[u] && c + kFoldTile * ti < R ? wa[u] * z[u][ti] : 0.0;
#pragma unroll
            for (int tj = ti; tj < T; ++tj, ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(za, zz[tj], acc[k], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int ti = 0; ti < T; ++ti)
#pragma unroll
            for (int tj = ti; tj < T; ++tj, ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(zz[ti], zz[tj], acc[k], 0, 0, 0);
        }
#pragma unroll
        for (int ti = 0; ti < T; ++ti) bacc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(zz[ti], xx, bacc[ti], 0, 0, 0);
      }
    }
  }

  // the accumulators as the LDS image of G (both triangles) and b
  {
    int k = 0;
#pragma unroll
    for (int ti = 0; ti < T; ++ti)
#pragma unroll
      for (int tj = ti; tj < T; ++tj, ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = kFoldTile * ti + q4 + 4 * r, gj = kFoldTile * tj + c;
          if constexpr (WT) {                    // entry (i, j), i <= j, defines both triangles
            if (gi <= gj) {
              Gs[gi + RP * gj] = acc[k][r];
              Gs[gj + RP * gi] = acc[k][r];
            }
          } else {
            Gs[gi + RP * gj] = acc[k][r];
            if (ti != tj) Gs[gj + RP * gi] = acc[k][r];
          }
        }
    if (c == 0) {
#pragma unroll
      for (int ti = 0; ti < T; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[kFoldTile * ti + q4 + 4 * r] = bacc[ti][r];
    }
  }
  __syncthreads();

  const int64_t pb = a.pbase[q];
  if (pb < 0) {                                  // uniform: the query's only chunk
    if constexpr (WT) {
      if (unlisted) {
        for (int i = lane; i < R * R; i += kFoldWave) {
          double* g = Gs + (i % R) + RP * (i / R);
          *g = fma(a.alpha, a.H[i], *g);
        }
        __syncthreads();
      }
    }
    return q;
  }
  double* P = a.partial + (pb + chunk) * PD;
  for (int i = lane; i < R * R; i += kFoldWave) P[i] = Gs[(i % R) + RP * (i / R)];
  if (lane < R) P[(int64_t)R * R + lane] = bs[lane];
  return -1;
}

// One wave per work item (sum_partials = 0) or per split query (sum_partials = 1).  Both launches of a call run this
// kernel, so the solve exists once per rank class and a query's bits cannot depend on the path that brought its normal
// equations to LDS.
// The weighted instantiations up to R = 32 name the waves per SIMD their unweighted twins reach (3 and 2).  With that the
// compiler keeps the accumulators of the R <= 32 class in VGPRs (166 registers, three waves) where it otherwise takes
// 166 + 40 AGPRs and two waves, and a call with alpha > 0 is 0.35 ms shorter on 10^5 queries.  The value 1 is the default.
template <int T, bool WT>
__global__ __launch_bounds__(kFoldWave) __attribute__((amdgpu_waves_per_eu(WT ? (T == 1 ? 3 : T == 2 ? 2 : 1) : 1))) void foldin_k(typename FoldKArgsOf<WT>::type a, int sum_partials) {
  constexpr int RP = kFoldTile * T;
  __shared__ double Gs[RP * RP];
  __shared__ double bs[RP];
  const int64_t q = foldin_normal_dev<T, WT>(a, sum_partials, Gs, bs);
  if (q < 0) return;                             // uniform: one chunk of a longer query, its partial is written
  foldin_solve_dev<T>(Gs, bs, q, a);
}

template <int T, bool WT>
static void launch_foldin(const typename FoldKArgsOf<WT>::type& ka, int64_t items, int64_t splits, hipStream_t s) {
  foldin_k<T, WT><<<(unsigned)items, kFoldWave, 0, s>>>(ka, 0);
  AO_KERNEL_CHECK();
  if (splits > 0) {
    foldin_k<T, WT><<<(unsigned)splits, kFoldWave, 0, s>>>(ka, 1);
    AO_KERNEL_CHECK();
  }
}

template <bool WT>
static void launch_foldin_class(const typename FoldKArgsOf<WT>::type& ka, int64_t items, int64_t splits, hipStream_t s) {
  switch ((ka.R + kFoldTile - 1) / kFoldTile) {
    case 1: launch_foldin<1, WT>(ka, items, splits, s); break;
    case 2: launch_foldin<2, WT>(ka, items, splits, s); break;
    case 3: launch_foldin<3, WT>(ka, items, splits, s); break;
    default: launch_foldin<4, WT>(ka, items, splits, s); break;
  }
}

// foldin_w.hip: the weighted instantiations of foldin_k
void foldin_launch_weighted(const FoldKArgsW& ka, int64_t items, int64_t splits, hipStream_t s);

}  // namespace aoadmm
