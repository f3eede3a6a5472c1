// The proximal operator catalogue on gfx950 (functions/constraints_to_prox.m:13-91): every prox but the isotonic /
// unimodal projections and the parallel graph-Laplacian solve, which live in iso.hip.
#include <type_traits>

#include "prox.h"
#include "device_utils.h"
#include "hosteig.h"
#include "prox_dev.h"

namespace aoadmm {

// ===========================================================================
// column-wise prox kernels: one block per column
// ===========================================================================
__device__ __forceinline__ double block_sum(double v, double* sh) {
  // fixed-order tree over blockDim.x (power of two <= 256)
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int st = blockDim.x >> 1; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// l2-ball family, l2 regularisation, non-negative sphere (:37,:40,:43,:56)
__global__ void prox_colnorm_k(ColArgs a, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  __shared__ double sh[256];
  __shared__ double shv[256];
  __shared__ int shi[256];
  const int r = blockIdx.x;
  const double* v = a.V + a.ldv * r;
  double* z = a.Z + a.ldz * r;
  const bool clamp = a.type == AOADMM_C_NONNEG_L2_BALL || a.type == AOADMM_C_NONNEG_L2_SPHERE;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) {
    double y = v[i];
    if (clamp) y = fmax(y, 0.0);
    acc += y * y;
  }
  const double nrm = sqrt(block_sum(acc, sh));
  if (a.type == AOADMM_C_NONNEG_L2_SPHERE) {
    if (nrm == 0.0) {
      // [~,maxcoord] = max(X(:,r)) : first maximum (prox_normalized_nonneg.m:6-7)
      double bv = -INFINITY;
      int64_t bi = 0;
      for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x)
        if (v[i] > bv) { bv = v[i]; bi = i; }
      shv[threadIdx.x] = bv;
      shi[threadIdx.x] = (int)bi;
      __syncthreads();
      if (threadIdx.x == 0) {
        double best = shv[0];
        int64_t besti = shi[0];
        for (int t = 1; t < (int)blockDim.x; ++t)
          if (shv[t] > best || (shv[t] == best && shi[t] < besti)) { best = shv[t]; besti = shi[t]; }
        shi[0] = (int)besti;
      }
      __syncthreads();
      const int64_t arg = shi[0];
      for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) z[i] = (i == arg) ? 1.0 : 0.0;
    } else {
      for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) z[i] = fmax(v[i], 0.0) / nrm;
    }
    return;
  }
  double scale;
  if (a.type == AOADMM_C_L2_REG) {
    const double g = a.p0 / (a.rho[0] * a.rho_mul);
    scale = nrm > g ? 1.0 - g / nrm : 0.0;
  } else {
    scale = nrm > a.p0 ? a.p0 / nrm : 1.0;
  }
  for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) {
    double y = v[i];
    if (clamp) y = fmax(y, 0.0);
    z[i] = y * scale;
  }
}

// simplex column-wise / l1-ball (:21,:34): parallel fixed-point for the exact threshold
__global__ void prox_simplex_col_k(ColArgs a, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  __shared__ double sh[256];
  const int r = blockIdx.x;
  const double* v = a.V + a.ldv * r;
  double* z = a.Z + a.ldz * r;
  const bool l1 = a.type == AOADMM_C_L1_BALL;
  const double eta = a.p0;
  if (l1) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) acc += fabs(v[i]);
    const double n1 = block_sum(acc, sh);
    if (!(n1 > eta)) {
      for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) z[i] = v[i];
      return;
    }
  }
  double tau = -INFINITY;
  double cnt_prev = -1.0;
  for (int64_t it = 0; it <= a.rows; ++it) {
    double s = 0.0, c = 0.0;
    for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) {
      const double y = l1 ? fabs(v[i]) : v[i];
      if (y > tau) { s += y; c += 1.0; }
    }
    const double S = block_sum(s, sh);
    const double Cn = block_sum(c, sh);
    if (Cn == cnt_prev || Cn == 0.0) break;
    cnt_prev = Cn;
    tau = (S - eta) / Cn;
  }
  for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) {
    if (l1) {
      const double w = fmax(fabs(v[i]) - tau, 0.0);
      z[i] = v[i] > 0 ? w : (v[i] < 0 ? -w : 0.0);
    } else {
      z[i] = fmax(v[i] - tau, 0.0);
    }
  }
}

// ---- sequential column algorithms (one thread per task, data in LDS or L2-resident scratch)

// Exact 1-D TV prox: L. Condat, IEEE SPL 20(11) 2013 (restated; TV_Condat_v2 at prox_TV.m:7
// returns the same unique minimiser).
__device__ void tv1d_condat_dev(const double* y, double* x, int64_t n, double lam) {
  if (n <= 0) return;
  if (!(lam > 0.0)) {
    for (int64_t i = 0; i < n; ++i) x[i] = y[i];
    return;
  }
  int64_t k = 0, k0 = 0, km = 0, kp = 0;
  double vmin = y[0] - lam, vmax = y[0] + lam, umin = lam, umax = -lam;
  for (;;) {
    if (k == n - 1) {
      if (umin < 0.0) {
        do { x[k0++] = vmin; } while (k0 <= km);
        k = km = kp = k0;
        vmin = y[k];
        umin = lam;
        umax = vmin + umin - vmax;
      } else if (umax > 0.0) {
        do { x[k0++] = vmax; } while (k0 <= kp);
        k = km = kp = k0;
        vmax = y[k];
        umax = -lam;
        umin = vmax + umax - vmin;
      } else {
        vmin += umin / (double)(k - k0 + 1);
        do { x[k0++] = vmin; } while (k0 <= k);
        return;
      }
    } else {
      umin += y[k + 1] - vmin;
      if (umin < -lam) {
        do { x[k0++] = vmin; } while (k0 <= km);
        k = km = kp = k0;
        vmin = y[k];
        vmax = vmin + 2.0 * lam;
        umin = lam;
        umax = -lam;
      } else {
        umax += y[k + 1] - vmax;
        if (umax > lam) {
          do { x[k0++] = vmax; } while (k0 <= kp);
          k = km = kp = k0;
          vmax = y[k];
          vmin = vmax - 2.0 * lam;
          umin = lam;
          umax = -lam;
        } else {
          ++k;
          if (umin >= lam) {
            km = k;
            vmin += (umin - lam) / (double)(km - k0 + 1);
            umin = lam;
          }
          if (umax <= -lam) {
            kp = k;
            vmax += (umax + lam) / (double)(kp - k0 + 1);
            umax = -lam;
          }
        }
      }
    }
  }
}

__global__ void prox_tv_k(ColArgs a, int use_lds, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  extern __shared__ double dyn[];
  const int r = blockIdx.x;
  const double* v = a.V + a.ldv * r;
  double* z = a.Z + a.ldz * r;
  const double lam = a.p0 / (a.rho[0] * a.rho_mul);     // prox_TV(x, eta/rho)  (:80)
  if (use_lds) {
    double* y = dyn;
    double* x = dyn + a.rows;
    for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) y[i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0) tv1d_condat_dev(y, x, a.rows, lam);
    __syncthreads();
    for (int64_t i = threadIdx.x; i < a.rows; i += blockDim.x) z[i] = x[i];
  } else {
    if (threadIdx.x == 0) tv1d_condat_dev(v, z, a.rows, lam);
  }
}

// Parallel exact TV prox for one column per 256-thread block (active-set / split-merge form of the
// same optimality system Condat's scan solves).  With u_i = sum_{t<=i}(y_t - x_t) the minimiser of
// 0.5||x-y||^2 + lam*sum|x_{i+1}-x_i| is characterised by |u_i| <= lam, u_{n-1} = 0 and
// u_i = -lam*sign(x_{i+1}-x_i) at every jump.  A guess of the jump set J (signs in {-1,0,+1}) fixes the
// segment values  v_S = (sum_S y + lam*(J[b] - J[a-1])) / |S| ; jumps whose sign disagrees with
// v_right - v_left are merged, segments whose interior |u| exceeds lam are split at the worst point.
// The fixed point satisfies the KKT system, i.e. is the unique minimiser; if the iteration cap is hit
// thread 0 falls back to the sequential scan, so the result is exact either way.  Inside the ADMM loop
// J is warm-started from the previous Z column, which usually converges in 1-3 rounds.
static constexpr int kTvParMax = 6400;       // rows of a column whose working arrays fit LDS (25 bytes per row, below)

// The iteration is built on prefix sums so that no step is sequential in a
// segment's length: with Pc[i] = sum_{t<i} (y_t - c) (c = mean(y), which keeps the prefix sums small) the value
// of segment [sa, sb] is  c + (Pc[sb+1] - Pc[sa] + lam*(J[sb] - J[sa-1])) / len  and the dual at an interior
// point is  u_i = -lam*J[sa-1] + (Pc[i+1] - Pc[sa]) - (v - c)*(i - sa + 1),  both O(1).  A round is: scan the
// segment starts, one thread per segment for the values, one per boundary for the merge test, every thread
// walks its own 8-16 entries for the split test and the per-segment worst violation is found with a 64-bit
// LDS max (magnitude bits above, index in the low 12 bits).  ~8 barriers per round, 1-3 rounds warm-started.
// With `fz` the kernel also does the dual update of the ADMM iteration for its column (mu = V - Z_new,
// Z <- Z_new) and the four residual sums, which removes the separate dual kernel.
struct TvFused {
  double* Z = nullptr;      // in: previous Z (warm start), out: new Z
  double* mu = nullptr;     // in/out
  double* part = nullptr;   // [R][4]: ||fac-Z||^2, ||fac||^2, ||mu||^2, ||Z-Zold||^2 of this column
  int64_t ld = 0;
};
// kTvThreads threads per column (256 for short columns, 1024 above 1024 rows: every phase walks a thread's chunk of
// ceil(n / kTvThreads) entries sequentially through LDS, so four times the threads is close to four times fewer
// dependent LDS round trips; measured at 2000 rows in DESIGN.md section 4.4).
// GLOBAL: columns beyond kTvParMax rows keep the same working arrays in a per-column slice of the prox workspace
// (L2-resident: 37 bytes per row) instead of LDS, so a long mode does not drop to the one-thread scan; the index field
// of the split key widens to 24 bits.
static __host__ __device__ inline size_t tv_ws_doubles(int64_t rows) {
  return ((size_t)(4 * rows + 2) * 8 + (size_t)(rows + 2) * 4 + (size_t)rows + 64 + 7) / 8;
}
template <int kTvThreads, int MEM = 0>
__global__ __launch_bounds__(kTvThreads) void prox_tv_fast_k(ColArgs a, const double* warm, int64_t ldw, TvFused fz,
                                                             const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  constexpr int NW = kTvThreads / 64;
  constexpr bool GLOBAL = MEM != 0;                                // columns beyond the LDS-resident 4096 rows
  // split key: magnitude bits of the worst |u| above, entry index below.  LDS-resident columns: 32 bits (float
  // magnitude, 13-bit index -- the key only ranks violations, any violating entry is a valid split point); workspace
  // forms: 64 bits with a 24-bit index
  typedef typename std::conditional<GLOBAL, unsigned long long, unsigned>::type KeyT;
  constexpr KeyT kIdxMask = GLOBAL ? (KeyT)0xffffffull : (KeyT)0x1fffu;
  extern __shared__ double lds_dyn[];
  __shared__ int wsum[NW];
  __shared__ double dsum[NW];
  __shared__ int flag_merge[2], flag_split[2];          // alternate by round: the reset of one never races with the read of the other
  const int n = (int)a.rows;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int r = blockIdx.x;
  const double* vin = a.V + a.ldv * r;
  double* z = a.Z + a.ldz * r;
  const double lam = a.p0 / (a.rho[0] * a.rho_mul);
  // working arrays: y (n), Pc (n + 1), val (n), best (n), start (n + 1 ints), J (n bytes) -- 37 bytes per row.
  //   MEM 0: all in LDS (<= 6400 rows) at 25 bytes per row: the input is staged in the slots of Pc (the prefix sums
  //          replace it in place, every thread its own chunk; the dual update takes the input from registers and the
  //          sequential fallback reads it from global memory again) and the split keys are 32 bits wide.  Round 3: the
  //          limit was 4096 rows at 37 bytes, and 6000 rows ran the hybrid form at 51 us per in-loop call.
  //   MEM 2: the arrays every phase of a round walks (Pc, start, J: 13 bytes per row) in LDS, y / val / best in the
  //          column's slice of the prox workspace (<= kTvHybridMax rows; round 2 had all six in the workspace there and
  //          every phase was a chain of L2 round trips: 90 us per in-loop call at 6000 rows against 22 us at 2000)
  //   MEM 1: all in the workspace (L2-resident)
  double* gws = GLOBAL ? a.ws + (size_t)blockIdx.x * tv_ws_doubles(a.rows) : nullptr;
  double *y, *Pc, *val;
  KeyT* best;
  int* start;
  signed char* J;
  if constexpr (MEM == 2) {
    y = gws; val = gws + n; best = reinterpret_cast<KeyT*>(gws + 2 * n);
    Pc = lds_dyn;                                                  // n + 1
    start = reinterpret_cast<int*>(lds_dyn + n + 1);               // n + 1
    J = reinterpret_cast<signed char*>(start + n + 1);             // n
  } else if constexpr (MEM == 0) {
    Pc = lds_dyn;                                                  // n + 1
    y = Pc;                                                        // the input, until the prefix sums take its place
    val = lds_dyn + n + 1;                                         // n
    best = reinterpret_cast<KeyT*>(val + n);                       // n (32-bit keys)
    start = reinterpret_cast<int*>(best + n);                      // n + 1
    J = reinterpret_cast<signed char*>(start + n + 1);             // n
  } else {
    double* dyn = gws;
    y = dyn;                                                       // n
    Pc = dyn + n;                                                  // n + 1
    val = dyn + 2 * n + 1;                                         // n
    best = reinterpret_cast<KeyT*>(dyn + 3 * n + 1);               // n
    start = reinterpret_cast<int*>(dyn + 4 * n + 1);               // n + 1
    J = reinterpret_cast<signed char*>(start + n + 1);             // n
  }
  const int chunk = (n + kTvThreads - 1) / kTvThreads;
  const int c0 = min(n, t * chunk), c1 = min(n, c0 + chunk);
  constexpr int kKeep = GLOBAL ? 1 : 8;                            // entries per thread of an LDS-resident column (launcher: rows <= 8 * threads)
  double keep_mu[kKeep], keep_z[kKeep];                            // old mu / old Z of the entries t + k*kTvThreads (fz only)
  double keep_y[kKeep];                                            // MEM 0: the input of the same entries (its LDS slots become Pc)
  // ---- load (coalesced, all loads of a thread independent: a chunk-ordered loop would serialise 8-16 memory
  // round trips), mean, centred prefix sums.  The warm-start column is staged in `val` the same way.
  {
    // every load of the thread is issued before the first LDS store, on clamped (always valid) addresses and without
    // an exec-mask branch in between: written as `for (i = t; i < n; i += 256) y[i] = vin[i]` the compiler emitted one
    // s_waitcnt vmcnt(0) per element, i.e. 8-16 dependent memory round trips before the kernel could start
    const double* wv = warm ? warm + ldw * r : vin;      // no warm start: a second read of the column, discarded
    // With `fz` the dual update at the end needs the old mu and the old Z of the same entries (t + k*kTvThreads): they
    // are fetched here, in the kernel's first round trip, and wait in registers (fz.Z is the warm-start column) -- read
    // at the end they were one more dependent memory round trip per call.
    const double* mv = fz.mu ? fz.mu + fz.ld * r : vin;
    const double* zv = fz.Z ? fz.Z + fz.ld * r : vin;    // (the same column as `wv` in the ADMM loop: the load hits the same lines)
    auto stage = [&](auto kper_tag) {
      constexpr int KP = decltype(kper_tag)::value;
      double ry[KP], rw[KP];
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const int i = min(t + k * kTvThreads, n - 1);
        ry[k] = vin[i];
        rw[k] = wv[i];
        if (k < kKeep) { keep_mu[k] = mv[i]; keep_z[k] = zv[i]; keep_y[k] = ry[k]; }
      }
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const int i = t + k * kTvThreads;
        if (i < n) { y[i] = ry[k]; val[i] = rw[k]; }
      }
    };
    if constexpr (GLOBAL) {
      for (int i0 = 0; i0 < n; i0 += 8 * kTvThreads) {  // eight independent loads of each column per round trip
        double ry[8], rw[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int i = min(i0 + t + k * kTvThreads, n - 1);
          ry[k] = vin[i];
          rw[k] = wv[i];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int i = i0 + t + k * kTvThreads;
          if (i < n) { y[i] = ry[k]; val[i] = rw[k]; }
        }
      }
    } else if (n <= kTvThreads) stage(std::integral_constant<int, 1>());
    else if (n <= 2 * kTvThreads) stage(std::integral_constant<int, 2>());
    else if (n <= 4 * kTvThreads) stage(std::integral_constant<int, 4>());
    else stage(std::integral_constant<int, 8>());
  }
  __syncthreads();
  double loc = 0.0;
  for (int i = c0; i < c1; ++i) loc += y[i];
  auto block_scan_d = [&](double v, double& total) {               // exclusive scan over threads, fixed order
    double inc = v;
    inc = wave_scan_incl(inc);
    if (lane == 63) dsum[w] = inc;
    __syncthreads();
    double base = 0.0, all = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) { if (q < w) base += dsum[q]; all += dsum[q]; }
    total = all;
    __syncthreads();
    return base + inc - v;
  };
  // ONE scan gives the mean and the centred prefix sums: the exclusive prefix of the plain sums at the thread's first
  // entry, less c times the number of entries before it, is the prefix of the centred values (the difference of the two
  // forms is a rounding of size |prefix| * 2^-53, far below the 1e-13 slack of `thr`; two scans were two more barriers)
  const double* sol = val;                                          // where the solution ends up (val, or Pc after the expansion)
  double tot;
  const double before = block_scan_d(loc, tot);
  const double c = n > 0 ? tot / n : 0.0;
  if (!(lam > 0.0)) {
    for (int i = c0; i < c1; ++i) val[i] = y[i];
  } else {
    double run = before - c * (double)c0;
    for (int i = c0; i < c1; ++i) { const double yi = y[i]; Pc[i] = run; run += yi - c; }   // (MEM 0: y[i] IS Pc[i])
    if (c1 == n && c0 < n) Pc[n] = run;                            // the thread holding the last entry
    // ---- warm start of the jump set
    if (warm) {
      for (int i = c0; i < c1; ++i) {
        if (i < n - 1) { const double d = val[i + 1] - val[i]; J[i] = d > 0 ? 1 : (d < 0 ? -1 : 0); }
        else J[i] = 0;
      }
    } else {
      for (int i = c0; i < c1; ++i) J[i] = 0;
    }
    __syncthreads();
    const double thr = lam * (1.0 + 1e-11) + 1e-13 * (fabs(c) + 1.0);
    const int max_rounds = 4 * n + 64;
    bool converged = false;
    for (int round = 0; round < max_rounds; ++round) {
      // 1. segment starts: i == 0 or a jump between i-1 and i
      int cnt = 0;
      for (int i = c0; i < c1; ++i) cnt += (i == 0 || J[i - 1] != 0) ? 1 : 0;
      int inc = cnt;
      inc = wave_scan_incl(inc);
      if (lane == 63) wsum[w] = inc;
      const int fp = round & 1;
      if (t == 0) { flag_merge[fp] = 0; flag_split[fp] = 0; }
      __syncthreads();
      int base = 0;
      for (int q = 0; q < w; ++q) base += wsum[q];
      const int first_seg = base + inc - cnt;                      // starts before this thread's chunk
      {
        int pos = first_seg;
        for (int i = c0; i < c1; ++i)
          if (i == 0 || J[i - 1] != 0) start[pos++] = i;
      }
      int nseg = 0;
#pragma unroll
      for (int q = 0; q < NW; ++q) nseg += wsum[q];
      if (t == 0) start[nseg] = n;
      __syncthreads();
      // 2. segment values
      for (int sgi = t; sgi < nseg; sgi += kTvThreads) {
        const int sa = start[sgi], sb = start[sgi + 1] - 1;
        const double sl = sa == 0 ? 0.0 : (double)J[sa - 1];
        const double sr = sb == n - 1 ? 0.0 : (double)J[sb];
        val[sgi] = c + (Pc[sb + 1] - Pc[sa] + lam * (sr - sl)) / (double)(sb - sa + 1);
        best[sgi] = (KeyT)0;
      }
      __syncthreads();
      // 3. merge jumps whose sign disagrees with the values on both sides
      for (int sgi = t; sgi + 1 < nseg; sgi += kTvThreads) {
        const int jp = start[sgi + 1] - 1;
        if ((double)J[jp] * (val[sgi + 1] - val[sgi]) <= 0.0) { J[jp] = 0; flag_merge[fp] = 1; }
      }
      __syncthreads();
      const int merged = flag_merge[fp];                           // (reset again two rounds on, behind several barriers)
      // 4. split segments whose interior dual leaves [-lam, lam]: per-segment worst violation.  In the same round as the
      // merges, for the segments no merge touched (a boundary whose J is zero now was merged: the segment's value is
      // stale): a round that only merged followed by a round that only split were two rounds (3.2 us each at 2000 rows)
      // for what is one change of the jump set between two ADMM iterations -- typically 3 rounds per call before, 2 now.
      {
        int sgi = first_seg - ((c0 < c1 && (c0 == 0 || J[c0 - 1] != 0)) ? 0 : 1);   // segment of entry c0
        for (int i = c0; i < c1; ++i) {
          if (i != c0 && J[i - 1] != 0) ++sgi;
          const int sa = start[sgi], sb = start[sgi + 1] - 1;
          if (i >= sb) continue;                                   // the segment's last entry carries the jump itself
          if (merged && ((sa > 0 && J[sa - 1] == 0) || (sb < n - 1 && J[sb] == 0))) continue;
          const double u0 = sa == 0 ? 0.0 : -lam * (double)J[sa - 1];
          const double u = u0 + (Pc[i + 1] - Pc[sa]) - (val[sgi] - c) * (double)(i - sa + 1);
          const double au = fabs(u);
          if (au > thr) {
            KeyT key;
            if constexpr (GLOBAL) key = ((KeyT)__double_as_longlong(au) & ~kIdxMask) | (KeyT)i;
            else key = ((KeyT)__float_as_uint((float)au) & ~kIdxMask) | (KeyT)i;       // au > thr >= 1e-13: never a zero key
            atomicMax(&best[sgi], key);
          }
        }
      }
      __syncthreads();
      for (int sgi = t; sgi < nseg; sgi += kTvThreads) {
        const KeyT b = best[sgi];
        if (b != (KeyT)0) {
          const int i = (int)(b & kIdxMask);
          const int sa = start[sgi];
          const double u0 = sa == 0 ? 0.0 : -lam * (double)J[sa - 1];
          const double u = u0 + (Pc[i + 1] - Pc[sa]) - (val[sgi] - c) * (double)(i - sa + 1);
          J[i] = u > 0 ? -1 : 1;
          flag_split[fp] = 1;
        }
      }
      __syncthreads();
      const int split = flag_split[fp];
      if (!split && !merged) { converged = true; break; }
    }
    if (converged) {
      // expand: entry i takes the value of its segment (val is indexed by segment; write through `best` as doubles
      // would alias, so expand into y, which is no longer needed)
      int sgi = 0;
      {
        int cnt = 0;
        for (int i = c0; i < c1; ++i) cnt += (i == 0 || J[i - 1] != 0) ? 1 : 0;
        int inc = cnt;
        inc = wave_scan_incl(inc);
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int base = 0;
        for (int q = 0; q < w; ++q) base += wsum[q];
        sgi = base + inc - cnt - ((c0 < c1 && (c0 == 0 || J[c0 - 1] != 0)) ? 0 : 1);
      }
      for (int i = c0; i < c1; ++i) {
        if (i != c0 && J[i - 1] != 0) ++sgi;
        Pc[i] = val[sgi];                                          // Pc is free now: holds the solution
      }
      sol = Pc;
    } else {
      __syncthreads();
      if (t == 0) tv1d_condat_dev(MEM == 0 ? vin : y, val, n, lam);   // exact sequential fallback (MEM 0: the LDS copy of the input is gone)
    }
  }
  __syncthreads();
  // ---- write the column; optionally the ADMM dual update and residual sums for it
  if (fz.Z == nullptr) {
    for (int i = t; i < n; i += kTvThreads) z[i] = sol[i];
    return;
  }
  double* Zc = fz.Z + fz.ld * r;
  double* muc = fz.mu + fz.ld * r;
  double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  auto dual = [&](auto kper_tag) {
    constexpr int KP = decltype(kper_tag)::value;      // entries per thread, by the same size classes as above
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int i = t + k * kTvThreads;
      if (i < n) {
        const double zn = sol[i], vv = MEM == 0 ? keep_y[k < kKeep ? k : 0] : y[i];
        const double mo = keep_mu[k < kKeep ? k : 0], zo = keep_z[k < kKeep ? k : 0];   // fetched with the column
        const double x = vv - mo;                      // fac = V - mu_old
        const double mn = vv - zn;                     // mu + fac - Z   (:1428)
        Zc[i] = zn;
        muc[i] = mn;
        const double d = x - zn, e = zn - zo;
        s1 += d * d; s2 += x * x; s3 += mn * mn; s4 += e * e;
      }
    }
  };
  if constexpr (GLOBAL) {
    for (int i0 = 0; i0 < n; i0 += 4 * kTvThreads) {
      double mo[4], zo[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = min(i0 + t + k * kTvThreads, n - 1);
        mo[k] = muc[i];
        zo[k] = Zc[i];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + t + k * kTvThreads;
        if (i < n) {
          const double zn = sol[i], vv = y[i];
          const double x = vv - mo[k];
          const double mn = vv - zn;
          Zc[i] = zn;
          muc[i] = mn;
          const double d = x - zn, e = zn - zo[k];
          s1 += d * d; s2 += x * x; s3 += mn * mn; s4 += e * e;
        }
      }
    }
  } else if (n <= kTvThreads) dual(std::integral_constant<int, 1>());
  else if (n <= 2 * kTvThreads) dual(std::integral_constant<int, 2>());
  else if (n <= 4 * kTvThreads) dual(std::integral_constant<int, 4>());
  else dual(std::integral_constant<int, 8>());
  // the four residual sums of the column in one reduction (one barrier instead of eight)
  __shared__ double q4sum[NW][4];
  double q4[4] = {s1, s2, s3, s4};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = q4[q];
    v = wave_sum(v);
    if (lane == 0) q4sum[w][q] = v;
  }
  __syncthreads();
  if (t < 4) {
    double tot4 = 0.0;
#pragma unroll
    for (int k = 0; k < NW; ++k) tot4 += q4sum[k][t];
    fz.part[(int64_t)r * 4 + t] = tot4;
  }
}

// isotonic / unimodal projections and the parallel GL solve live in iso.hip

// GL smoothness on columns longer than the cyclic-reduction kernel of iso.hip takes: one thread per column
// GL smoothness: (2*eta/rho*L + I) \ x with the path-graph Laplacian (:68-76): Thomas algorithm
__global__ void prox_gl_k(ColArgs a, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  if (threadIdx.x != 0) return;
  const int r = blockIdx.x;
  const int64_t n = a.rows;
  const double* v = a.V + a.ldv * r;
  double* z = a.Z + a.ldz * r;
  double* cp = a.ws + (int64_t)r * n;
  const double s2 = 2.0 * (a.p0 / (a.rho[0] * a.rho_mul));
  if (n == 1) { z[0] = v[0] / (s2 * 1.0 + 1.0); return; }
  const double off = -s2;
  double diag = s2 * 1.0 + 1.0;
  cp[0] = off / diag;
  z[0] = v[0] / diag;
  for (int64_t i = 1; i < n; ++i) {
    const double d = ((i == n - 1) ? s2 * 1.0 : s2 * 2.0) + 1.0;
    const double m = d - off * cp[i - 1];
    cp[i] = off / m;
    z[i] = (v[i] - off * z[i - 1]) / m;
  }
  for (int64_t i = n - 2; i >= 0; --i) z[i] -= cp[i] * z[i + 1];
}

// orthonormal columns: U*V' of the thin SVD W = U S V' (project_ortho.m:3-4), i.e. the polar factor of W.
// One-sided Jacobi preconditioned through the Gram matrix: a one-sided Jacobi SVD looks for an orthogonal J with W*J =
// U*S (orthogonal columns); instead of rotating the rows x R matrix pair by pair (190 pairs x ~10 sweeps x a pass
// over 2000 rows each: 7.7 ms at 2000 x 20 in one workgroup), pass 1 takes J1 from the eigenvectors of G = W'W
// (R x R, one wave: sym_eig_small) and forms W1 = W*J1 with one small GEMM; pass 2 and 3 repeat that on W1, W2, whose
// Gram matrices are already diagonal up to rounding of size eps*||W||^2 -- Jacobi on such a matrix is accurate in the
// relative sense, so the cond(W)^2 error of a single Gram-eigen step is removed.  That needs the RELATIVE stopping rule
// |a_pq| <= 1e-15*sqrt(a_pp*a_qq) (sym_eig_small's `relative`): under the norm-wise rule the other callers use, a Gram
// matrix whose off-diagonal part is eps*||W||^2 has converged before its first sweep, passes 2 and 3 did nothing and
// the columns of the small singular values stayed non-orthogonal by eps*cond(W)^2 (measured: 3e-6 from the SVD's polar
// factor at 40 x 12, cond 1e6; 1.3e-11 with the relative rule, the error of numpy's own SVD).  Then S = column norms
// (the last eigenvalues), U = W3/S and Z = U*(J1*J2*J3)'.  Columns with S = 0 give zero columns, as before.
__global__ void ortho_m_k(double* M, const double* Jt, const double* G, int R, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);                                      // M(r,c) = Jt(c,r) / S_r with S_r^2 = G(r,r)
  for (int e = threadIdx.x; e < R * R; e += blockDim.x) {
    const int r = e % R, c = e / R;
    const double g = G[r + R * r];
    const double sg = g > 0.0 ? sqrt(g) : 0.0;
    M[r + R * c] = sg > 0.0 ? Jt[c + R * r] / sg : 0.0;
  }
}
static size_t ortho_ws_doubles(int64_t rows, int R) {
  return (size_t)2 * rows * R + atb_ws_bytes(rows, R, R) / sizeof(double) + (size_t)5 * R * R + 64;
}
static void prox_ortho(const double* V, int64_t ldv, double* Z, int64_t ldz, int64_t rows, int R, double* ws, const AdmmCtl* ctl,
                       hipStream_t s) {
  double* Wa = ws;
  double* Wb = Wa + rows * R;
  double* aws = Wb + rows * R;
  double* G = aws + atb_ws_bytes(rows, R, R) / sizeof(double);
  double* Q = G + R * R;
  double* Ja = Q + R * R;
  double* Jb = Ja + R * R;
  double* M = Jb + R * R;
  double* wv = M;                                      // eigenvalues are not needed: M's storage takes them
  const double* W = V;
  int64_t ldw = ldv;
  const double* Jt = nullptr;                          // accumulated rotation J1*J2*...
  for (int pass = 0; pass < 3; ++pass) {
    atb_small(G, W, ldw, W, ldw, rows, R, R, aws, ctl, s);
    sym_eig_small(G, R, wv, Q, s, ctl, true);         // relative stopping rule, see above
    double* Wn = (W == Wa) ? Wb : Wa;
    gemm_small(Wn, rows, W, ldw, Q, R, rows, R, R, 0, coef(1.0), 0.0, ctl, s);          // W <- W*Q
    double* Jn = (Jt == Ja) ? Jb : Ja;
    if (pass == 0) AO_HIP(hipMemcpyAsync(Jn, Q, (size_t)R * R * sizeof(double), hipMemcpyDeviceToDevice, s));
    else gemm_small(Jn, R, Jt, R, Q, R, R, R, R, 0, coef(1.0), 0.0, ctl, s);            // J <- J*Q
    Jt = Jn;
    W = Wn; ldw = rows;
  }
  atb_small(G, W, ldw, W, ldw, rows, R, R, aws, ctl, s);                                 // squared column norms on its diagonal
  ortho_m_k<<<1, 256, 0, s>>>(M, Jt, G, R, ctl);
  AO_KERNEL_CHECK();
  gemm_small(Z, ldz, W, ldw, M, R, rows, R, R, 0, coef(1.0), 0.0, ctl, s);               // Z = (W/S)*J'
}

// element-wise or row-wise: the ADMM loop kernels apply these themselves (prox_dev.h)
bool prox_is_fusable(int t) {
  return t == AOADMM_C_NONNEG || t == AOADMM_C_BOX || t == AOADMM_C_L1_REG || t == AOADMM_C_L0_REG ||
         t == AOADMM_C_RIDGE || t == AOADMM_C_SIMPLEX_ROW;
}

// stand-alone element-wise / row-wise prox (op-level entry and the generic loops)
template <int RMAX>
__global__ void prox_rows_k(ColArgs a, const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.rows) return;
  const double rho = a.rho[0] * a.rho_mul;
  double z[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) z[r] = r < a.R ? a.V[i + a.ldv * r] : 0.0;
  if (a.type == AOADMM_C_SIMPLEX_ROW) {
    simplex_regs<RMAX>(z, a.R, a.p0);
  } else {
#pragma unroll
    for (int r = 0; r < RMAX; ++r) z[r] = prox_elem(a.type, z[r], a.p0, a.p1, rho);
  }
#pragma unroll
  for (int r = 0; r < RMAX; ++r)
    if (r < a.R) a.Z[i + a.ldz * r] = z[r];
}

// ---- 'quadratic regularization' ------------------------------------------------------------------
void QuadPrep::build(const double* L_host, int64_t rows, hipStream_t s) {
  AO_REQUIRE(L_host != nullptr && rows > 0, "quadratic regularization needs its matrix L");
  if (rows > 4096) throw Error(AOADMM_ERR_UNSUPPORTED, "quadratic regularization: matrices beyond 4096 x 4096 are not prepared on the device");
  n = rows;
  std::vector<double> A(L_host, L_host + (size_t)rows * rows), wv, Uv;
  double asym = 0.0, nrm = 0.0;
  for (int64_t j = 0; j < rows; ++j)
    for (int64_t i = 0; i < rows; ++i) {
      const double d = A[(size_t)i + (size_t)rows * j] - A[(size_t)j + (size_t)rows * i];
      asym += d * d; nrm += A[(size_t)i + (size_t)rows * j] * A[(size_t)i + (size_t)rows * j];
    }
  const size_t nn = (size_t)rows * rows * sizeof(double);
  if (std::sqrt(asym) > 1e-12 * std::sqrt(nrm)) {      // no orthogonal eigenbasis: inverse per value of rho (refresh)
    nonsym = true;
    dirty = true;
    L.alloc(nn); Minv.alloc(nn); Mwork.alloc(nn);
    piv.alloc((size_t)rows * sizeof(int)); pval.alloc(sizeof(double));
    AO_HIP(hipMemcpyAsync(L.p, L_host, nn, hipMemcpyHostToDevice, s));
    AO_HIP(hipStreamSynchronize(s));
    return;
  }
  nonsym = false;
  const int sweeps = host_sym_eig(rows, A, wv, Uv);
  AO_REQUIRE(sweeps >= 0, "eigendecomposition of the quadratic-regularization matrix did not converge");
  std::vector<double> Utv((size_t)rows * rows);
  for (int64_t j = 0; j < rows; ++j)
    for (int64_t i = 0; i < rows; ++i) Utv[(size_t)j + (size_t)rows * i] = Uv[(size_t)i + (size_t)rows * j];
  L.alloc(nn); U.alloc(nn); Ut.alloc(nn); w.alloc((size_t)rows * sizeof(double));
  AO_HIP(hipMemcpyAsync(L.p, L_host, nn, hipMemcpyHostToDevice, s));
  AO_HIP(hipMemcpyAsync(U.p, Uv.data(), nn, hipMemcpyHostToDevice, s));
  AO_HIP(hipMemcpyAsync(Ut.p, Utv.data(), nn, hipMemcpyHostToDevice, s));
  AO_HIP(hipMemcpyAsync(w.p, wv.data(), (size_t)rows * sizeof(double), hipMemcpyHostToDevice, s));
  AO_HIP(hipStreamSynchronize(s));
}

// ---- non-symmetric L: (g*L + I)^-1 on the device, g = 2*eta/rho read from device memory (no host round trip) ----
// Gauss-Jordan inversion with row pivoting (what MATLAB's `\` pivots on), one elimination step per launch pair:
//   quad_pivot_k    (one workgroup)  p = argmax_{i >= k} |A(i,k)| (first maximum), pivot value
//   quad_gj_step_k  (whole chip)     B = step k applied to A, out of place (rows k and p change places on the way, so no
//                                    workgroup reads what another one writes); A and B swap roles every step
// and at the end the row exchanges are undone as column exchanges (quad_unswap_k, one thread per row).  2n launches
// and 2 n^2 doubles of traffic per step: n = 4096 costs ~0.25 s per refresh (once per outer iteration; the host version
// it replaces took tens of seconds and stalled the stream), n = 41 (the parity test) ~0.4 ms.  A zero pivot gives
// Inf/NaN like MATLAB's `\` on a singular matrix.
__global__ void quad_build_k(const double* __restrict__ L, double* __restrict__ A, int64_t n, double eta,
                             const double* rho, double rho_mul) {
  const double g = 2.0 * (eta / (rho[0] * rho_mul));
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * n; e += (int64_t)gridDim.x * blockDim.x)
    A[e] = g * L[e] + ((e % n == e / n) ? 1.0 : 0.0);
}
__global__ __launch_bounds__(1024) void quad_pivot_k(const double* __restrict__ A, int64_t n, int64_t k, int* piv, double* pv) {
  __shared__ double bv[16];
  __shared__ int64_t bi[16];
  const double* col = A + n * k;
  double best = -1.0;
  int64_t at = k;
  for (int64_t i = k + threadIdx.x; i < n; i += 1024) {
    const double v = fabs(col[i]);
    if (v > best || !(v == v)) { best = v == v ? v : 1e308 * 10.0; at = i; if (!(v == v)) break; }   // NaN wins (it propagates)
  }
  // first maximum: larger value, then smaller index
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o);
    const int64_t oi = __shfl_xor(at, o);
    if (ov > best || (ov == best && oi < at)) { best = ov; at = oi; }
  }
  if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = at; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w)
      if (bv[w] > best || (bv[w] == best && bi[w] < at)) { best = bv[w]; at = bi[w]; }
    piv[k] = (int)at;
    pv[0] = col[at];
  }
}
static constexpr int kGjCols = 8;                     // columns per workgroup of a Gauss-Jordan step
__global__ __launch_bounds__(256) void quad_gj_step_k(const double* __restrict__ A, double* __restrict__ B, int64_t n, int64_t k,
                                                      const int* __restrict__ piv, const double* __restrict__ pv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.y * kGjCols;
  const int64_t p = piv[k];
  const double inv = 1.0 / pv[0];
  if (i >= n) return;
  const int64_t s = (i == p) ? k : i;                  // row i after the exchange of rows k and p (i != k)
  const double f = A[s + n * k];
#pragma unroll
  for (int c = 0; c < kGjCols; ++c) {
    const int64_t j = j0 + c;
    if (j >= n) break;
    const double r = (j == k ? 1.0 : A[p + n * j]) * inv;       // new row k
    B[i + n * j] = (i == k) ? r : ((j == k ? 0.0 : A[s + n * j]) - f * r);
  }
}
__global__ void quad_unswap_k(double* A, int64_t n, const int* __restrict__ piv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int64_t k = n - 1; k >= 0; --k) {
    const int64_t p = piv[k];
    if (p != k) { const double t = A[i + n * k]; A[i + n * k] = A[i + n * p]; A[i + n * p] = t; }
  }
}

const double* QuadPrep::refresh(double eta, const double* rho_dev, double rho_mul, hipStream_t s) {
  AO_REQUIRE(nonsym && n > 0 && Minv.p && Mwork.p, "quadratic regularization: non-symmetric matrix not prepared");
  // rho is fixed inside an ADMM loop and moves once per outer iteration: the engine marks the cache dirty at the head of
  // every outer iteration (Engine::solve), build() does for the op-level entries; a different rho pointer / multiplier /
  // eta is a different matrix as well
  if (!dirty && key_rho == rho_dev && key_mul == rho_mul && key_eta == eta) return result;
  const int64_t N = n;
  double* a = Minv.d();
  double* b = Mwork.d();
  int64_t nb = cdiv(N * N, 256);
  if (nb > 4096) nb = 4096;
  quad_build_k<<<(unsigned)nb, 256, 0, s>>>(L.d(), a, N, eta, rho_dev, rho_mul);
  AO_KERNEL_CHECK();
  const dim3 grid((unsigned)cdiv(N, 256), (unsigned)cdiv(N, kGjCols));
  for (int64_t k = 0; k < N; ++k) {
    quad_pivot_k<<<1, 1024, 0, s>>>(a, N, k, piv.as<int>(), pval.d());
    quad_gj_step_k<<<grid, 256, 0, s>>>(a, b, N, k, piv.as<int>(), pval.d());
    std::swap(a, b);
  }
  AO_KERNEL_CHECK();
  quad_unswap_k<<<(unsigned)cdiv(N, 256), 256, 0, s>>>(a, N, piv.as<int>());
  AO_KERNEL_CHECK();
  result = a;
  dirty = false; key_rho = rho_dev; key_mul = rho_mul; key_eta = eta;
  return result;
}

// W(i,:) *= 1 / (2*eta/rho*w_i + 1)
__global__ void quad_scale_k(double* W, int64_t rows, int R, const double* w, double eta, const double* rho, double rho_mul,
                             const AdmmCtl* ctl) {
  CTL_GUARD(ctl);
  const double g = 2.0 * (eta / (rho[0] * rho_mul));
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < rows * R; e += (int64_t)gridDim.x * blockDim.x)
    W[e] = W[e] / (g * w[e % rows] + 1.0);
}

static constexpr int64_t kTvLdsRows = 8192;

size_t prox_ws_bytes(int type, int64_t rows, int R) {
  switch (type) {
    case AOADMM_C_NONDECREASING:
    case AOADMM_C_NONINCREASING:
    case AOADMM_C_UNIMODAL: return iso_ws_bytes(rows, R);
    case AOADMM_C_GL_SMOOTH: return prox_gl_ws_doubles(rows, R) * sizeof(double);
    case AOADMM_C_ORTHONORMAL: return ortho_ws_doubles(rows, R) * sizeof(double);
    case AOADMM_C_QUADRATIC: return (size_t)R * rows * sizeof(double);
    case AOADMM_C_TV: return rows > kTvParMax ? (size_t)R * tv_ws_doubles(rows) * sizeof(double) : 16;
    default: return 16;
  }
}

// Pc, start and J of a column in LDS (13 bytes per row): up to 12 000 rows beside the kernel's static LDS
static constexpr int64_t kTvHybridMax = 12000;
static size_t tv_hybrid_lds(int64_t rows) { return (size_t)(rows + 1) * 8 + (size_t)(rows + 2) * 4 + (size_t)rows + 64; }
static size_t tv_fast_lds(int64_t rows) {            // Pc + val doubles, 32-bit keys, start, J
  return (size_t)(2 * rows + 1) * 8 + (size_t)rows * 4 + (size_t)(rows + 2) * 4 + (size_t)rows + 64;
}
static void tv_fast_launch(const ColArgs& a, const double* warm, int64_t ldw, const TvFused& fz, const AdmmCtl* ctl,
                           hipStream_t s) {
  if (a.rows > kTvParMax) {
    AO_REQUIRE(a.ws != nullptr && a.rows < (int64_t(1) << 24), "TV prox: %lld rows need the global workspace (below 2^24 rows)",
               (long long)a.rows);
    if (a.rows <= kTvHybridMax) {
      ensure_dynamic_lds(reinterpret_cast<const void*>(prox_tv_fast_k<1024, 2>), (int)tv_hybrid_lds(kTvHybridMax));
      prox_tv_fast_k<1024, 2><<<a.R, 1024, tv_hybrid_lds(a.rows), s>>>(a, warm, ldw, fz, ctl);
    } else {
      prox_tv_fast_k<1024, 1><<<a.R, 1024, 0, s>>>(a, warm, ldw, fz, ctl);
    }
  } else if (a.rows > 1024) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(prox_tv_fast_k<1024>), (int)tv_fast_lds(kTvParMax));
    prox_tv_fast_k<1024><<<a.R, 1024, tv_fast_lds(a.rows), s>>>(a, warm, ldw, fz, ctl);
  } else {
    prox_tv_fast_k<256><<<a.R, 256, tv_fast_lds(a.rows), s>>>(a, warm, ldw, fz, ctl);
  }
  AO_KERNEL_CHECK();
}

// what prox_tv_fast_k takes: LDS-resident columns, or the same arrays in the prox workspace
bool prox_tv_dual_ok(int type, int64_t rows, bool have_ws) {
  return type == AOADMM_C_TV && (rows <= kTvParMax || (have_ws && rows < (int64_t(1) << 24)));
}

void prox_apply(const ProxSpec& ps, const double* V, int64_t ldv, double* Zout, int64_t ldz,
                int64_t rows, int R, const double* rho_dev, double rho_mul, double* ws,
                const AdmmCtl* ctl, hipStream_t s, const double* warm, int64_t ldw) {
  ColArgs a;
  a.V = V; a.Z = Zout; a.ldv = ldv; a.ldz = ldz; a.rows = rows; a.R = R; a.type = ps.type;
  a.p0 = ps.p0; a.p1 = ps.p1; a.rho = rho_dev; a.rho_mul = rho_mul; a.ws = ws;
  if (rows <= 0 || R <= 0) return;
  switch (ps.type) {
    case AOADMM_C_NONNEG: case AOADMM_C_BOX: case AOADMM_C_L1_REG: case AOADMM_C_L0_REG:
    case AOADMM_C_RIDGE: case AOADMM_C_SIMPLEX_ROW: {
      const unsigned blocks = (unsigned)cdiv(rows, 128);
      if (R <= 8) prox_rows_k<8><<<blocks, 128, 0, s>>>(a, ctl);
      else if (R <= 16) prox_rows_k<16><<<blocks, 128, 0, s>>>(a, ctl);
      else if (R <= 32) prox_rows_k<32><<<blocks, 128, 0, s>>>(a, ctl);
      else prox_rows_k<64><<<blocks, 128, 0, s>>>(a, ctl);
      break;
    }
    case AOADMM_C_L2_BALL: case AOADMM_C_NONNEG_L2_BALL: case AOADMM_C_NONNEG_L2_SPHERE: case AOADMM_C_L2_REG:
      prox_colnorm_k<<<R, 256, 0, s>>>(a, ctl);
      break;
    case AOADMM_C_SIMPLEX_COL: case AOADMM_C_L1_BALL:
      prox_simplex_col_k<<<R, 256, 0, s>>>(a, ctl);
      break;
    case AOADMM_C_TV: {
      if (prox_tv_dual_ok(ps.type, rows, ws != nullptr)) {
        tv_fast_launch(a, warm, ldw, TvFused(), ctl, s);
        break;
      }
      const int use_lds = rows <= kTvLdsRows;
      const size_t sh = use_lds ? (size_t)2 * rows * sizeof(double) : 0;
      ensure_dynamic_lds(reinterpret_cast<const void*>(prox_tv_k), (int)(2 * kTvLdsRows * sizeof(double)));
      prox_tv_k<<<R, 64, sh, s>>>(a, use_lds, ctl);
      break;
    }
    case AOADMM_C_NONDECREASING: prox_iso(V, ldv, Zout, ldz, rows, R, 0, 0.0, ws, ctl, s); break;
    case AOADMM_C_NONINCREASING: prox_iso(V, ldv, Zout, ldz, rows, R, 1, 0.0, ws, ctl, s); break;
    case AOADMM_C_UNIMODAL: prox_iso(V, ldv, Zout, ldz, rows, R, 2, ps.p0, ws, ctl, s); break;
    case AOADMM_C_GL_SMOOTH:
      if (!prox_gl_pcr(V, ldv, Zout, ldz, rows, R, ps.p0, rho_dev, rho_mul, ctl, s, ws)) prox_gl_k<<<R, 64, 0, s>>>(a, ctl);
      break;
    case AOADMM_C_ORTHONORMAL: prox_ortho(V, ldv, Zout, ldz, rows, R, ws, ctl, s); break;
    case AOADMM_C_QUADRATIC: {                       // (2*eta/rho*L + I) \ x = U diag(1/(2 eta/rho w + 1)) U' x   (:66)
      if (ps.quad) {                                 // non-symmetric L: Z = (2*eta/rho*L + I)^-1 * V, inverse cached per rho
        const double* Mi = ps.quad->refresh(ps.p0, rho_dev, rho_mul, s);
        gemm_small(Zout, ldz, Mi, rows, V, ldv, rows, (int)rows, R, 0, coef(1.0), 0.0, ctl, s);
        break;
      }
      AO_REQUIRE(ps.LU && ps.LUt && ps.Lw, "quadratic regularization: matrix not prepared");
      gemm_small(ws, rows, ps.LUt, rows, V, ldv, rows, (int)rows, R, 0, coef(1.0), 0.0, ctl, s);
      int64_t nb = cdiv(rows * R, 256);
      if (nb > 1024) nb = 1024;
      quad_scale_k<<<(unsigned)nb, 256, 0, s>>>(ws, rows, R, ps.Lw, ps.p0, rho_dev, rho_mul, ctl);
      AO_KERNEL_CHECK();
      gemm_small(Zout, ldz, ps.LU, rows, ws, rows, rows, (int)rows, R, 0, coef(1.0), 0.0, ctl, s);
      break;
    }
    default:
      throw Error(AOADMM_ERR_UNSUPPORTED, fmt("constraint id %d has no device prox (route to the MATLAB path)", ps.type));
  }
  AO_KERNEL_CHECK();
}

void prox_tv_dual(const ProxSpec& ps, const double* V, int64_t rows, int R, const double* rho, double* prox_ws,
                  double* Z, double* mu, double* part, const AdmmCtl* ctl, hipStream_t s) {
  ColArgs a;
  a.V = V; a.Z = Z; a.ldv = rows; a.ldz = rows; a.rows = rows; a.R = R; a.type = ps.type;   // (a.Z: the kernel writes through fz)
  a.p0 = ps.p0; a.p1 = ps.p1; a.rho = rho; a.rho_mul = 1.0; a.ws = prox_ws;
  TvFused fz;
  fz.Z = Z; fz.mu = mu; fz.part = part; fz.ld = rows;
  tv_fast_launch(a, Z, rows, fz, ctl, s);                                                   // warm start: the previous Z
}

}  // namespace aoadmm

