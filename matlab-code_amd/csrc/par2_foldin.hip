// Fold-in of new slabs into a fitted PARAFAC2 block -- see par2_foldin.h and DESIGN.md section 9.10.
#include "par2_foldin.h"

#include "par2_polar_dev.h"
#include "small_dev.h"

namespace aoadmm {

typedef double p2f_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kP2FoldWave = 64;
// leading dimension of the staged rows in LDS: 4 mod 32, so that the operand read of a step -- column c = l & 15, row
// 4 s + (l >> 4) -- puts the 64 lanes on 64 different doubles (4 c + q4 modulo the 32 double-wide banks: two lanes each,
// the minimum for 64 lanes of 8 bytes); the staging stores run along the lanes and are conflict-free at any value
constexpr int kP2FoldLd = kP2FoldStage + 4;

P2FoldinPath par2_foldin_path(int64_t I, int R, int Jmax, int64_t nk) {
  (void)nk;
  P2FoldinPath p;
  p.tiles = (R + kP2FoldTile - 1) / kP2FoldTile;
  p.chunks = (int)std::max<int64_t>(1, cdiv(I, kP2FoldChunkRows));
  p.alt_lds = ((size_t)R * R + 2 * (size_t)Jmax * R) * sizeof(double) <= kP2FoldLdsBudget ? 1 : 0;
  return p;
}
size_t par2_foldin_sys_doubles(int R) { return 2 * (size_t)R * R + 1; }

// ---------------------------------------------------------------------------
// S = (A'A) .* (DeltaB'DeltaB), rho, L.  Entry (r, q) of each Gram matrix is four interleaved chains over the rows, added
// as (a0 + a1) + (a2 + a3): the same products in the same order for (r, q) and (q, r), so S is symmetric to the bit.
__global__ __launch_bounds__(256) void par2_fold_system_k(P2FoldinArgs a) {
  extern __shared__ double M[];
  __shared__ double rho_s;
  const int R = a.R, RR = R * R;
  for (int e = threadIdx.x; e < RR; e += blockDim.x) {
    const int r = e % R, q = e / R;
    const double* ar = a.A + a.lda * r;
    const double* aq = a.A + a.lda * q;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
    int i = 0;
    for (; i + 3 < a.I; i += 4) {
      g0 += ar[i] * aq[i]; g1 += ar[i + 1] * aq[i + 1]; g2 += ar[i + 2] * aq[i + 2]; g3 += ar[i + 3] * aq[i + 3];
    }
    for (; i < a.I; ++i) g0 += ar[i] * aq[i];
    const double ga = (g0 + g1) + (g2 + g3);
    double db = 0.0;
    for (int j = 0; j < R; ++j) db += a.DeltaB[j + R * r] * a.DeltaB[j + R * q];
    const double sv = ga * db;
    a.sys[e] = sv;
    M[e] = sv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int r = 0; r < R; ++r) t += M[r + R * r];
    rho_s = t / R;
    a.sys[2 * RR] = rho_s;
  }
  __syncthreads();
  const double shift = a.opt.constraint == 1 ? a.opt.ridge + rho_s / 2 : a.opt.ridge;
  for (int r = threadIdx.x; r < R; r += blockDim.x) M[r + R * r] += shift;
  __syncthreads();
  const bool ok = chol_lds(M, R);
  if (ok)
    for (int e = threadIdx.x; e < RR; e += blockDim.x) a.sys[RR + e] = M[e];
  else if (threadIdx.x == 0) a.ctl->notpd = 1;
}

// ---------------------------------------------------------------------------
// Y = X_q' A for 16 columns of one slab (and one chunk of rows).  Lane l = (c = l & 15, q4 = l >> 4).  A stage is 64 rows of
// I: lane l loads row i0 + l of the 16 slab columns and of the R factor columns (consecutive lanes, consecutive addresses)
// and leaves them in LDS; a step of four rows then takes X(i0 + 4 s + q4, j0 + c) as the A operand (row c <-> slab column)
// and A(i0 + 4 s + q4, 16 t + c) as the B operand of tile t, so that lane l receives Y(j0 + q4 + 4 reg, 16 t + c).  Rows
// beyond the chunk, columns beyond J_q and beyond R enter as zero operands: their loads go to clamped (valid) addresses
// and what they bring is replaced by 0.0 where it is stored to LDS, never multiplied.
template <int T>
__global__ __launch_bounds__(kP2FoldWave) void par2_fold_y_k(P2FoldinArgs a, int chunks) {
  constexpr int RP = kP2FoldTile * T;
  __shared__ double Xs[kP2FoldTile * kP2FoldLd];
  __shared__ double As[RP * kP2FoldLd];
  const int lane = (int)threadIdx.x, c = lane & 15, q4 = lane >> 4;
  const int64_t item = (int64_t)blockIdx.x / chunks;
  const int ch = (int)((int64_t)blockIdx.x % chunks);
  const int q = a.item_q[item], g = a.item_g[item];
  const int64_t o = a.off[q];
  const int n = (int)(a.off[q + 1] - o);
  const int j0 = kP2FoldTile * g;
  const int R = a.R;
  const int64_t I = a.I;
  const double* Xq = a.X + I * o;
  const int64_t ib = (int64_t)ch * kP2FoldChunkRows;
  const int64_t ie = ib + kP2FoldChunkRows < I ? ib + kP2FoldChunkRows : I;

  p2f_f64x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = p2f_f64x4{0.0, 0.0, 0.0, 0.0};
  double xx = 0.0;
  // the rows of a stage travel global -> registers -> LDS; the loads of the next stage are issued before the MFMA steps
  // of this one, so a stage's memory latency overlaps the previous stage's arithmetic (the wave still waits for what is
  // left of it at the head of every stage)
  // (at most 32 factor columns ride in registers: with more the T = 4 class spills; the others are staged when used)
  constexpr int PF = RP < 32 ? RP : 32;
  double xv[kP2FoldTile], av[PF];
  // Unconditional loads on clamped addresses (a row of this chunk, a column below J_q, below R), so that all of a
  // stage's loads are in flight together; what a clamp brought in is replaced by a zero where it is stored.
  auto load_stage = [&](int64_t i0) {
    const int64_t ic = i0 + lane < ie ? i0 + lane : ie - 1;
#pragma unroll
    for (int jj = 0; jj < kP2FoldTile; ++jj) xv[jj] = Xq[ic + I * (j0 + jj < n ? j0 + jj : n - 1)];
#pragma unroll
    for (int r = 0; r < PF; ++r) av[r] = a.A[ic + a.lda * (r < R ? r : R - 1)];
  };
  load_stage(ib);
  for (int64_t i0 = ib; i0 < ie; i0 += kP2FoldStage) {
    const bool live = i0 + lane < ie;
#pragma unroll
    for (int jj = 0; jj < kP2FoldTile; ++jj) {
      const double xz = live && j0 + jj < n ? xv[jj] : 0.0;
      Xs[jj * kP2FoldLd + lane] = xz;
      xx = fma(xz, xz, xx);
    }
#pragma unroll
    for (int r = 0; r < PF; ++r) As[r * kP2FoldLd + lane] = live && r < R ? av[r] : 0.0;
    if constexpr (RP > PF) {
      const int64_t i = i0 + lane;
#pragma unroll 8
      for (int r = PF; r < RP; ++r) {
        double v = 0.0;
        if (i < ie && r < R) v = a.A[i + a.lda * r];
        As[r * kP2FoldLd + lane] = v;
      }
    }
    __syncthreads();
    if (i0 + kP2FoldStage < ie) load_stage(i0 + kP2FoldStage);   // uniform
    const int rows = (int)(ie - i0 < kP2FoldStage ? ie - i0 : kP2FoldStage);
    const int steps = (rows + 3) / 4;                // uniform; rows past the chunk are zeros in LDS
    for (int s = 0; s < steps; ++s) {
      const double x = Xs[c * kP2FoldLd + 4 * s + q4];
#pragma unroll
      for (int t = 0; t < T; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, As[(kP2FoldTile * t + c) * kP2FoldLd + 4 * s + q4], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  double* out = (chunks > 1 ? a.ypart + (int64_t)ch * a.Jtot * R : a.Y) + o * R;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int j = j0 + q4 + 4 * reg, r = kP2FoldTile * t + c;
      if (j < n && r < R) out[j + (int64_t)n * r] = acc[t][reg];
    }
  xx = wave_sum(xx);
  if (lane == 0) a.xpart[item * chunks + ch] = xx;
}

// chunked: Y = the chunks' partials added in chunk order from the first
__global__ void par2_fold_ysum_k(P2FoldinArgs a, int chunks) {
  const int64_t tot = a.Jtot * a.R;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
    double v = a.ypart[e];
    for (int ch = 1; ch < chunks; ++ch) v += a.ypart[(int64_t)ch * tot + e];
    a.Y[e] = v;
  }
}

// ---------------------------------------------------------------------------
// The alternation of one slab on one wave.  Dynamic LDS (doubles): Jr (R R, the rotation of par2_polar_dev), DeltaB, L, S
// (R R each), c (64), the two offsets par2_polar_dev reads (2), then with in_lds Y_q and W (Jmax R each).  Lane t holds
// entry t of every R-vector (c, b, u, z, mu).  The two substitutions broadcast one entry per step; the norms are
// butterfly sums that leave the same bits in every lane, so every exit is uniform.
__global__ __launch_bounds__(kP2FoldWave) void par2_fold_alt_k(P2FoldinArgs a, int chunks, int in_lds) {
  extern __shared__ double sh[];
  if (a.ctl->notpd != 0) return;                     // uniform: the shared system has no factor
  const int q = (int)blockIdx.x, R = a.R, RR = R * R, lane = (int)threadIdx.x;
  double* Jr = sh;
  double* Ds = Jr + RR;
  double* Ls = Ds + RR;
  double* Ss = Ls + RR;
  double* cs = Ss + RR;
  int64_t* off2 = reinterpret_cast<int64_t*>(cs + kP2FoldWave);
  double* Ys = cs + kP2FoldWave + 2;
  double* Ws = Ys + (int64_t)a.Jmax * R;
  const int64_t o = a.off[q];
  const int n = (int)(a.off[q + 1] - o);
  const int64_t base = o * R;
  for (int e = lane; e < RR; e += kP2FoldWave) {
    Ds[e] = a.DeltaB[e];
    Ss[e] = a.sys[e];
    Ls[e] = a.sys[RR + e];
  }
  if (lane == 0) { off2[0] = 0; off2[1] = n; }
  const double rho = a.sys[2 * RR];
  const double* Yq = in_lds ? Ys : a.Y + base;
  double* Wq = in_lds ? Ws : a.W + base;
  if (in_lds)
    for (int e = lane; e < n * R; e += kP2FoldWave) Ys[e] = a.Y[base + e];
  double xn;
  {                                                  // ||X_q||^2: the parts of the slab's work items, lane-strided, then the wave
    const int64_t p0 = a.item0[q] * chunks, p1 = a.item0[q + 1] * chunks;
    double acc = 0.0;
    for (int64_t e = p0 + lane; e < p1; e += kP2FoldWave) acc += a.xpart[e];
    xn = wave_sum(acc);
  }
  __syncthreads();
  const bool mine = lane < R;
  const int lc = mine ? lane : 0;
  const double myinv = mine ? 1.0 / Ls[lc + R * lc] : 0.0;
  double c = mine ? (a.c0 != nullptr ? a.c0[q + a.nk * lc] : 1.0) : 0.0;
  P2Dims dd;
  dd.K = 1; dd.I = a.I; dd.R = R; dd.off = off2; dd.off_h = nullptr; dd.Jtot = n; dd.Jmax = n; dd.k0 = 0; dd.k1 = 1;

  // L L' u = v with one entry per lane: the forward substitution broadcasts y_j and lane t > j subtracts L(t, j) y_j, the
  // backward one broadcasts u_j and lane t < j subtracts L(j, t) u_j
  auto solve = [&](double v) {
    double y = 0.0;
    for (int j = 0; j < R; ++j) {
      const double yj = readlane_d(v * myinv, j);
      if (lane == j) y = yj;
      if (mine && lane > j) v -= Ls[lc + R * j] * yj;
    }
    double u = 0.0;
    for (int j = R - 1; j >= 0; --j) {
      const double uj = readlane_d(y * myinv, j);
      if (lane == j) u = uj;
      if (lane < j) y -= Ls[j + R * lc] * uj;
    }
    return u;
  };

  int it = 0, lost = 0;
  double b = 0.0;
  for (;;) {
    cs[lane] = c;
    __syncthreads();
    for (int e = lane; e < n * R; e += kP2FoldWave) {  // W = Y diag(c) DeltaB'
      const int j = e % n, r = e / n;
      double acc = 0.0;
      for (int s = 0; s < R; ++s) acc += (Yq[j + n * s] * cs[s]) * Ds[r + R * s];
      Wq[e] = acc;
    }
    __syncthreads();
    par2_polar_dev(Wq, a.P + base, dd, 0, 0, Jr);    // in place (LDS or workspace), cold start; P_q to its output
    __syncthreads();
    for (int p = 0; p < R; ++p) {                    // a column the polar factor zeroed: W lost it
      double al = 0.0;
      for (int i = lane; i < n; i += kP2FoldWave) al += Wq[i + n * p] * Wq[i + n * p];
      if (wave_sum(al) == 0.0) lost = 1;
    }
    const double* Pq = a.P + base;
    double* Bq = a.B + base;
    for (int r = 0; r < R; ++r) {                    // B = P DeltaB, b(r) = sum_j Y(j, r) B(j, r)
      double acc = 0.0;
      for (int j = lane; j < n; j += kP2FoldWave) {
        double bv = 0.0;
        for (int s = 0; s < R; ++s) bv += Pq[j + n * s] * Ds[s + R * r];
        Bq[j + n * r] = bv;
        acc += Yq[j + n * r] * bv;
      }
      const double br = wave_sum(acc);
      if (lane == r) b = br;
    }
    const double cold = c;
    if (a.opt.constraint == 0) {                     // uniform
      c = solve(b);
    } else {                                         // the cold-started row loop of foldin_solve_dev
      double zc = 0.0, mu = 0.0, rp, rd;
      int inner = 0;
      do {
        const double u = solve(b + rho / 2 * (zc - mu));
        const double zold = zc;
        const double s = u + mu;
        zc = s > 0.0 ? s : (s == s ? 0.0 : s);       // max(s, 0), a NaN stays
        mu = (mu + u) - zc;
        const double nu = sqrt(wave_sum(u * u));
        const double npr = sqrt(wave_sum((u - zc) * (u - zc)));
        const double ndu = sqrt(wave_sum((zc - zold) * (zc - zold)));
        const double nmu = sqrt(wave_sum(mu * mu));
        rp = npr / nu;
        rd = nmu > 0.0 ? ndu / nmu : ndu;
        ++inner;
      } while (inner < a.opt.max_inner && (rp > a.opt.tol_primal || rd > a.opt.tol_dual));
      c = zc;
    }
    ++it;
    const double diff = sqrt(wave_sum((c - cold) * (c - cold)));
    const double nc = sqrt(wave_sum(c * c));
    if (it >= a.opt.max_iter || diff <= a.opt.tol * nc) break;   // uniform
    __syncthreads();
  }
  __syncthreads();
  cs[lane] = c;
  __syncthreads();
  double sc = 0.0;
  if (mine)
    for (int s = 0; s < R; ++s) sc += Ss[lc + R * s] * cs[s];
  const double cb = wave_sum(c * b);
  const double csc = wave_sum(c * sc);
  if (mine) a.C[q + a.nk * lc] = c;
  if (lane == 0) {
    a.res[q] = xn - 2.0 * cb + csc;
    a.xnorm[q] = xn;
    a.iters[q] = it;
    a.info[q] = lost;
  }
}

template <int T>
static void launch_y(const P2FoldinArgs& a, int chunks, hipStream_t s) {
  par2_fold_y_k<T><<<(unsigned)(a.items * chunks), kP2FoldWave, 0, s>>>(a, chunks);
  AO_KERNEL_CHECK();
}

void par2_foldin_enqueue(const P2FoldinArgs& a, hipStream_t s) {
  const P2FoldinPath path = par2_foldin_path(a.I, a.R, a.Jmax, a.nk);
  const int R = a.R;
  // (the caller has checked that items x chunks work items fit one grid)
  par2_fold_system_k<<<1, 256, (size_t)R * R * sizeof(double), s>>>(a);
  AO_KERNEL_CHECK();
  switch (path.tiles) {
    case 1: launch_y<1>(a, path.chunks, s); break;
    case 2: launch_y<2>(a, path.chunks, s); break;
    case 3: launch_y<3>(a, path.chunks, s); break;
    default: launch_y<4>(a, path.chunks, s); break;
  }
  if (path.chunks > 1) {
    par2_fold_ysum_k<<<blocks_for(std::min<int64_t>(a.Jtot * R, (int64_t)1 << 20)), 256, 0, s>>>(a, path.chunks);
    AO_KERNEL_CHECK();
  }
  const size_t lds = (4 * (size_t)R * R + kP2FoldWave + 2 + (path.alt_lds ? 2 * (size_t)a.Jmax * R : 0)) * sizeof(double);
  if (lds > 32 * 1024) ensure_dynamic_lds(reinterpret_cast<const void*>(&par2_fold_alt_k), (int)lds);
  par2_fold_alt_k<<<(unsigned)a.nk, kP2FoldWave, lds, s>>>(a, path.chunks, path.alt_lds);
  AO_KERNEL_CHECK();
}

double par2_foldin_bytes(int I, int R, int64_t nk, int64_t Jtot) {
  // the slabs, A, and the outputs: Y, P, B (Jtot R each), C (nk R), res, xnorm, iters, info
  return 8.0 * ((double)I * Jtot + (double)I * R + 3.0 * Jtot * R + (double)nk * R + 2.0 * nk) + 8.0 * nk;
}
double par2_foldin_flops(int I, int R, int64_t Jtot, double iter_cols) {
  // Y, then per iteration and slab column: W, P and B (2 R^2 each) and one sweep's worth of rotations (3 R^2)
  return 2.0 * I * Jtot * R + iter_cols * 9.0 * R * R;
}

}  // namespace aoadmm
