// EM missing-data pass (see em.h).  Reference: functions/cmtf_fun_AOADMM.m:408-441 (imputation and
// f_rel_missing), :1224-1226 / :1249-1252 (objective over the observed entries), cmtf_AOADMM.m:133-148
// (Znorm_const of the masked data).
//
// CP block: one workgroup owns a strip of 256*VEC first-mode rows at one third-mode index k and walks the
// second mode.  A thread keeps its VEC rows of A, pre-multiplied by C(k,:), in registers; rows of B are
// staged through LDS 64 at a time and broadcast.  The model value is VEC*R FMAs per vector of entries, the
// tensor is read once (16-byte loads), the mask is ONE BIT per entry (packed on the device when Z.miss arrives: at
// 1000^3 the byte-per-entry mask was 1 GB of the pass's 9 GB), and only 128-byte lines that contain a missing entry are
// written back: the pass is bound by HBM like the contractions.
// The walk is written once: the strip kernel em_cp_vec_k (R <= 32) and the one-row kernel em_cp_k (beyond) share the
// geometry (EmWalk), the prologue, the tile staging, the line write-back and the epilogue, and take what differs per
// entry from a policy: EmMasked (data + mask bits; the only one that can fuse the contraction) or EmWeighted (X0, W and
// Xhat of a block with per-entry weights, EmCpArgs::X0 / Wt).
#include "em.h"

#include <algorithm>
#include <type_traits>

namespace aoadmm {

template <typename T, int VEC> struct EmVec;
template <> struct EmVec<float, 4> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct EmVec<double, 2> { typedef double type __attribute__((ext_vector_type(2))); };
template <typename T> struct EmVec<T, 1> { typedef T type __attribute__((ext_vector_type(1))); };   // the one-row kernel

// Z.miss as one bit per entry (bit e of the padded layout in byte e >> 3, position e & 7), 1 = observed.  A thread's VEC
// entries start at a multiple of VEC, so they sit in one byte.
__global__ void em_mask_pack_k(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ bits, int64_t n) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // output byte
  const int64_t e0 = o * 8;
  if (e0 >= n) return;
  unsigned v = 0;
  if (e0 + 8 <= n) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(bytes + e0);     // hipMalloc-aligned base, e0 multiple of 8
#pragma unroll
    for (int q = 0; q < 8; ++q) v |= (((w >> (8 * q)) & 0xff) != 0 ? 1u : 0u) << q;
  } else {
    for (int q = 0; q < 8; ++q) v |= ((e0 + q < n ? bytes[e0 + q] : 1) != 0 ? 1u : 0u) << q;   // past the end: observed
  }
  bits[o] = (uint8_t)v;
}
void em_mask_pack(const uint8_t* bytes, uint8_t* bits, int64_t n, hipStream_t s) {
  const int64_t nb = cdiv(n, (int64_t)8);
  em_mask_pack_k<<<(unsigned)cdiv(nb, (int64_t)256), 256, 0, s>>>(bytes, bits, n);
  AO_KERNEL_CHECK();
}

static constexpr int kEmThreads = 256;
static constexpr int kEmJTile = 64;

__device__ __forceinline__ double em_block_sum(double v, double* sh4) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
  __syncthreads();
  return r;
}

// The end of every pass kernel: the workgroup's four statistics, summed in fixed order, into its slot w of the workspace
__device__ __forceinline__ void em_store_stats(double num, double den, double ores, double ox2, double* sh4, double* w) {
  num = em_block_sum(num, sh4); den = em_block_sum(den, sh4);
  ores = em_block_sum(ores, sh4); ox2 = em_block_sum(ox2, sh4);
  if (threadIdx.x == 0) {
    w[0] = num; w[1] = den; w[2] = ores; w[3] = ox2;
  }
}

// acc + a * b[h] on both rows of a register pair: v_pk_fma_f32 reading one half of the pair `b` for both lanes
// (op_sel), so a broadcast LDS value needs no copy into a second register -- the compiler's form of `a * splat(b)` spent
// a v_mov and a register per rank column on it.
typedef float em_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ em_f2 pk_fma_lo(em_f2 a, em_f2 b, em_f2 acc) {
  em_f2 d;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b), "v"(acc));
  return d;
}
__device__ __forceinline__ em_f2 pk_fma_hi(em_f2 a, em_f2 b, em_f2 acc) {
  em_f2 d;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(d) : "v"(a), "v"(b), "v"(acc));
  return d;
}

// m + sum_r areg[r] * brow[r]   (brow: one row of the LDS tile, the same for every lane)
template <typename T, int VEC, int RMAX, typename XV>
__device__ __forceinline__ XV em_row_dot(const XV* areg, const T* brow, XV m) {
  if constexpr (std::is_same<T, float>::value && VEC == 4) {
    em_f2 m01 = m.xy, m23 = m.zw;
#pragma unroll
    for (int r = 0; r < RMAX; r += 2) {
      const em_f2 b2 = *reinterpret_cast<const em_f2*>(brow + r);
      m01 = pk_fma_lo(areg[r].xy, b2, m01); m23 = pk_fma_lo(areg[r].zw, b2, m23);
      m01 = pk_fma_hi(areg[r + 1].xy, b2, m01); m23 = pk_fma_hi(areg[r + 1].zw, b2, m23);
    }
    XV o;
    o.xy = m01; o.zw = m23;
    return o;
  } else {
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const T b = brow[r];
      XV bb;
#pragma unroll
      for (int v = 0; v < VEC; ++v) bb[v] = b;
      m = __builtin_elementwise_fma(areg[r], bb, m);
    }
    return m;
  }
}

// tacc[r] += x * brow[r]
template <typename T, int VEC, int RMAX, typename XV>
__device__ __forceinline__ void em_row_axpy(XV* tacc, const T* brow, XV x) {
  if constexpr (std::is_same<T, float>::value && VEC == 4) {
    const em_f2 x01 = x.xy, x23 = x.zw;
#pragma unroll
    for (int r = 0; r < RMAX; r += 2) {
      const em_f2 b2 = *reinterpret_cast<const em_f2*>(brow + r);
      tacc[r].xy = pk_fma_lo(x01, b2, tacc[r].xy); tacc[r].zw = pk_fma_lo(x23, b2, tacc[r].zw);
      tacc[r + 1].xy = pk_fma_hi(x01, b2, tacc[r + 1].xy); tacc[r + 1].zw = pk_fma_hi(x23, b2, tacc[r + 1].zw);
    }
  } else {
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const T b = brow[r];
      XV bb;
#pragma unroll
      for (int v = 0; v < VEC; ++v) bb[v] = b;
      tacc[r] = __builtin_elementwise_fma(x, bb, tacc[r]);
    }
  }
}

// Where a thread of a pass kernel stands: the strip can walk the second mode at a fixed third-mode index (walk = 1) or
// the third mode at a fixed second-mode index (walk = 2, steps of Ipad*J elements).  The walk is cut into jchunks pieces
// of jlen positions; a thread owns the VEC rows from i0 on.
// The shared pieces below take EmCpArgs and EmWalk BY VALUE: with the kernel-argument struct handed on by reference the
// fused R = 20 fp32 instantiation went from 20 to 52 bytes of scratch per lane (profiles/em_strip_once.md).
template <int VEC> struct EmWalk {
  bool wj;                                                               // walking the second mode
  int64_t f;                                                             // the fixed index (k, or j when walking k)
  const double *Ff, *Fw;                                                 // factors of the fixed mode (scales the rows of A) and of the walked mode (rows through LDS)
  int64_t ldf, ldw;
  int64_t step;                                                          // elements between two walk positions
  int chunk;
  int64_t i0, jbeg, jend;
  int64_t base;                                                          // first element at the fixed index
  bool in_range;                                                         // Ipad is a multiple of VEC
  __device__ __forceinline__ EmWalk(EmCpArgs a, int jchunks, int64_t jlen) {
    wj = a.walk != 2;
    f = blockIdx.y;
    const int64_t NW = wj ? a.J : a.K;
    Ff = wj ? a.C : a.B;
    ldf = wj ? a.ldC : a.ldB;
    Fw = wj ? a.B : a.C;
    ldw = wj ? a.ldB : a.ldC;
    step = wj ? a.Ipad : a.Ipad * a.J;
    chunk = blockIdx.x % jchunks;
    i0 = ((int64_t)(blockIdx.x / jchunks) * kEmThreads + threadIdx.x) * VEC;
    jbeg = chunk * jlen;
    jend = jbeg + jlen < NW ? jbeg + jlen : NW;
    base = (wj ? a.Ipad * a.J : a.Ipad) * f;
    in_range = i0 < a.Ipad;
  }
  // row i0 + v is padding (i >= I; the arrays hold zeros there); padmask: bit v set for such a row
  __device__ __forceinline__ bool pad(EmCpArgs a, int v) const { return i0 + v >= a.I; }
  __device__ __forceinline__ unsigned padmask(EmCpArgs a) const {
    unsigned m = 0;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (pad(a, v)) m |= 1u << v;
    return m;
  }
};

// Prologue: areg[r][v] = A(i0+v, r) * Ff(f, r), zero for padding rows and for r >= R
template <typename T, int VEC, int RMAX, bool FUSE, typename XV>
__device__ __forceinline__ void em_load_rows(EmCpArgs a, const EmWalk<VEC> g, XV* areg) {
  const int R = a.R;
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    const int rr = r < R ? r : 0;
    const double c = g.Ff ? g.Ff[g.f + g.ldf * rr] : 1.0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const bool valid = g.i0 + v < a.I;
      const int64_t i = valid ? g.i0 + v : a.I - 1;
      areg[r][v] = (r < R && valid) ? (T)(a.A[i + a.ldA * rr] * c) : (T)0;
    }
    // the fp64 loads of this prologue must not all be in flight at once: 2 * VEC * RMAX registers on top of tacc
    if constexpr (FUSE) { if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0); }
  }
}

// Rows j0 .. j0+63 of the walked mode's factor into the LDS tile, zero past jend and for r >= R
template <typename T, int VEC, int RMAX>
__device__ __forceinline__ void em_stage_tile(T (*Bsh)[RMAX], const EmWalk<VEC> g, int R, int64_t j0) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int e = t; e < kEmJTile * RMAX; e += kEmThreads) {
    const int jj = e / RMAX, r = e - jj * RMAX;
    Bsh[jj][r] = (r < R && j0 + jj < g.jend) ? (T)g.Fw[j0 + jj + g.ldw * r] : (T)0;
  }
  __syncthreads();
}

// Write-back of the strip kernel.  Only 128-byte lines in which some lane's vector `changes` go back (at 1-5 % missing
// most lines hold no missing entry; whole lines, so nothing is read-modified-written in L2 -- storing single 16-byte
// vectors was slower than storing everything).  The wave's 1024 bytes start 16-byte aligned: lane l shares its line with
// the lanes of the same (l + s) >> 3, s = the first lane's 16-byte slot inside its line; lines cut by the wave's ends go
// back if this wave's part of them changes.
template <typename XV>
__device__ __forceinline__ void em_line_store(bool changes, XV xn, XV* dst) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long bal = __ballot(changes);
  const unsigned s16 = (unsigned)(((reinterpret_cast<uintptr_t>(dst) >> 4) - lane) & 7u);
  const unsigned g = (lane + s16) >> 3;
  const unsigned grp = g < 8 ? (unsigned)((bal << s16) >> (8 * g)) & 0xffu : (unsigned)(bal >> (64 - s16)) & 0xffu;
  if (grp) __builtin_nontemporal_store(xn, dst);
}

// ---- entry policies ---------------------------------------------------------------------------------------------------------
// What a pass reads per vector of entries and what it makes of it.  A policy names its ring slot, loads one for a walk
// position w (the strip kernel streams, the one-row kernel's loads are plain), and evaluates it against the model
// vector m: the new value, whether it differs from what is stored (`changes`), and the four statistics' accumulators.
template <int VEC, typename XV>
__device__ __forceinline__ XV em_load(const XV* p) {
  if constexpr (VEC > 1) return __builtin_nontemporal_load(p);
  else return *p;
}

// Masked block: the data and the byte that holds this thread's VEC mask bits.  Padding rows are forced 'observed': they
// add exact zeros and are written back unchanged.
template <typename T, int VEC> struct EmMasked {
  typedef typename EmVec<T, VEC>::type XV;
  static constexpr bool kFuses = true;
  static constexpr unsigned kFull = (1u << VEC) - 1u;
  struct Slot { XV x; unsigned m; };                                     // m: the byte that holds this thread's VEC mask bits
  T* X;
  const uint8_t* M;                                                      // bits: entry e at byte e >> 3, position e & 7
  int64_t i0, step, mbase;                                               // mbase: this thread's first entry at walk position 0
  unsigned sh0, shs, padmask;                                            // position inside the byte at walk position w: (sh0 + shs*w) & 7
  __device__ __forceinline__ EmMasked(EmCpArgs a, const EmWalk<VEC> g)
      : X(reinterpret_cast<T*>(a.X) + g.base), M(a.mask), i0(g.i0), step(g.step), mbase(g.base + g.i0),
        sh0((unsigned)(mbase & 7)), shs((unsigned)(g.step & 7)), padmask(g.padmask(a)) {}
  __device__ __forceinline__ XV* at(int64_t w) const { return reinterpret_cast<XV*>(X + i0 + step * w); }
  __device__ __forceinline__ Slot load(int64_t w) const {
    const int64_t o = i0 + step * w;
    return {em_load<VEC>(reinterpret_cast<const XV*>(X + o)), M[(mbase + step * w) >> 3]};
  }
  __device__ __forceinline__ XV eval(const Slot& q, int64_t w, XV m, bool& changes, XV& s_ores, XV& s_ox2, XV& s_num,
                                     XV& s_den) const {
    const XV xv = q.x;
    const unsigned mv = ((q.m >> ((sh0 + shs * (unsigned)w) & 7u)) & kFull) | padmask;
    const XV d = xv - m;
    XV od, ox, xn;                                                       // residual / value where observed, else 0
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const bool observed = ((mv >> v) & 1u) != 0;
      od[v] = observed ? d[v] : (T)0;
      ox[v] = observed ? xv[v] : (T)0;
      xn[v] = observed ? xv[v] : m[v];
    }
    const XV md = d - od, mx = xv - ox;                                  // the same where missing (exact)
    s_ores = __builtin_elementwise_fma(od, od, s_ores);
    s_ox2 = __builtin_elementwise_fma(ox, ox, s_ox2);
    s_num = __builtin_elementwise_fma(md, md, s_num);
    s_den = __builtin_elementwise_fma(mx, mx, s_den);
    changes = mv != kFull;
    return xn;
  }
};

// One vector of entries of the weighted pass (em.h EmCpArgs::X0 / Wt): the new value and the four terms' accumulators.
// Products and differences are rounded one by one -- contracted, q = fma(-w, x0, xh) would be the rounding residue of
// em_w_reset's product instead of 0 in a solve's first pass, and f_rel_missing divides by the sum of q^2 -- and the
// multiply-adds written as such are fused.  With w in {0, 1}, xh = x0 where w = 1 and zeros in x0 where w = 0 every term
// is the masked policy's, bit for bit: w = 1 gives q = 0, p = 0 and wd = d; w = 0 gives q = xh, wd = 0 and xn = p = m.
template <typename T, typename XV>
__device__ __forceinline__ XV em_w_entry(XV x0, XV w, XV xh, XV m, XV& s_ores, XV& s_ox2, XV& s_num, XV& s_den) {
#pragma clang fp contract(off)
  const XV wx = w * x0;
  const XV q = xh - wx;                                                    // (1 - w) m_old
  const XV p = ((T)1 - w) * m;
  const XV d = x0 - m;
  const XV wd = w * d;
  const XV n = p - q;
  s_ores = __builtin_elementwise_fma(wd, d, s_ores);
  s_ox2 = __builtin_elementwise_fma(wx, x0, s_ox2);
  s_num = __builtin_elementwise_fma(n, n, s_num);
  s_den = __builtin_elementwise_fma(q, q, s_den);
  return __builtin_elementwise_fma(w, x0, p);
}

// Weighted block: three streams in (X0, W, Xhat), Xhat out.  A vector changes when some weight in it is not 1; under unit
// weights xh = x0 and stays.  Padding rows get w = 1 (X0 and Xhat hold zeros there).
template <typename T, int VEC> struct EmWeighted {
  typedef typename EmVec<T, VEC>::type XV;
  static constexpr bool kFuses = false;                                  // 2 * R register vectors and three streams do not fit
  struct Slot { XV x0, w, xh; };
  T* X;
  const T *X0, *W;
  int64_t i0, step;
  bool pad[VEC];
  __device__ __forceinline__ EmWeighted(EmCpArgs a, const EmWalk<VEC> g)
      : X(reinterpret_cast<T*>(a.X) + g.base), X0(reinterpret_cast<const T*>(a.X0) + g.base),
        W(reinterpret_cast<const T*>(a.Wt) + g.base), i0(g.i0), step(g.step) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) pad[v] = g.pad(a, v);
  }
  __device__ __forceinline__ XV* at(int64_t w) const { return reinterpret_cast<XV*>(X + i0 + step * w); }
  __device__ __forceinline__ Slot load(int64_t w) const {
    const int64_t o = i0 + step * w;
    return {em_load<VEC>(reinterpret_cast<const XV*>(X0 + o)), em_load<VEC>(reinterpret_cast<const XV*>(W + o)),
            em_load<VEC>(reinterpret_cast<const XV*>(X + o))};
  }
  __device__ __forceinline__ XV eval(const Slot& q, int64_t, XV m, bool& changes, XV& s_ores, XV& s_ox2, XV& s_num,
                                     XV& s_den) const {
    XV w = q.w;
    changes = false;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      w[v] = pad[v] ? (T)1 : w[v];
      changes |= w[v] != (T)1;
    }
    XV xn = em_w_entry<T, XV>(q.x0, w, q.xh, m, s_ores, s_ox2, s_num, s_den);
#pragma unroll
    for (int v = 0; v < VEC; ++v) xn[v] = w[v] == (T)1 ? q.x0[v] : xn[v];   // the data itself, also beside a model value that is not finite
    return xn;
  }
};

// Strip kernel for R <= 32.  Everything in the column loop is branch-free vector arithmetic in the tensor's
// precision (v_pk_*_f32 for fp32): the first version spent ~330 vector instructions per 16-byte vector of entries
// (a register ring shifted with moves, one branch per entry, fp64 statistics) and was bound by instruction issue
// at 4.3 TB/s, not by memory.
//   * VEC rows of A (times C(k,:)) per thread, held as R vectors areg[r]; B rows broadcast from LDS (ds_read_b128)
//   * the policy's loads run PD columns ahead in a statically indexed register ring (the column loop is unrolled by PD)
//   * the four statistics are accumulated per 64-column tile in the tensor's precision (64 terms per accumulator
//     lane) and join the fp64 sums once per tile
//   * write-back by 128-byte line (em_line_store): at 20 % missing every line qualifies, at 1 % about a quarter
//   * with FUSE it also accumulates, from the values it writes back, the partial contraction of the walked mode
//     T(i, f, r) = sum_w x_new(i, w, f) W(w, r)  -- the tensor pass the next outer iteration would start with
//     (contract.h ContractPlan: T is [chunk][i + Ipad*f][R] in the tensor's precision, one chunk per piece of the walk)
template <typename T, int VEC, int RMAX, bool FUSE, template <typename, int> class POL>
__global__ __launch_bounds__(kEmThreads, FUSE ? 2 : 1) void em_cp_vec_k(EmCpArgs a, int jchunks, int64_t jlen, double* ws) {
  static_assert(!FUSE || (POL<T, VEC>::kFuses && RMAX <= kEmFuseMaxRank), "no fused form of this pass");
  typedef typename EmVec<T, VEC>::type XV;
  typedef typename POL<T, VEC>::Slot Slot;
  __shared__ __attribute__((aligned(16))) T Bsh[kEmJTile][RMAX];
  __shared__ double sh4[4];
  const int R = a.R;
  const EmWalk<VEC> g(a, jchunks, jlen);
  XV areg[RMAX];                                                         // areg[r][v] = A(i0+v, r) * Ff(f, r)
  em_load_rows<T, VEC, RMAX, FUSE>(a, g, areg);
  const POL<T, VEC> pol(a, g);
  const XV zero = {};
  XV tacc[FUSE ? RMAX : 1];
#pragma unroll
  for (int r = 0; r < (FUSE ? RMAX : 1); ++r) tacc[r] = zero;
  double num = 0, den = 0, ores = 0, ox2 = 0;
  for (int64_t j0 = g.jbeg; j0 < g.jend; j0 += kEmJTile) {
    em_stage_tile<T, VEC, RMAX>(Bsh, g, R, j0);
    const int nj = (int)((g.jend - j0 < kEmJTile) ? (g.jend - j0) : kEmJTile);
    if (!g.in_range) continue;
    constexpr int PD = 4;                              // columns in flight
    Slot ring[PD];
#pragma unroll
    for (int p = 0; p < PD; ++p) ring[p] = pol.load(j0 + (p < nj ? p : nj - 1));
    XV s_ores = zero, s_ox2 = zero, s_num = zero, s_den = zero;
    for (int jj = 0; jj < nj; jj += PD) {
#pragma unroll
      for (int p = 0; p < PD; ++p) {
        const int jc = jj + p;                                           // wave-uniform
        const Slot q = ring[p];
        ring[p] = pol.load(j0 + (jc + PD < nj ? jc + PD : nj - 1));      // clamped: the last loads are discarded
        if (jc < nj) {
          const XV m = em_row_dot<T, VEC, RMAX, XV>(areg, &Bsh[jc][0], zero);
          bool changes;
          const XV xn = pol.eval(q, j0 + jc, m, changes, s_ores, s_ox2, s_num, s_den);
          if (a.update) em_line_store(changes, xn, pol.at(j0 + jc));
          if constexpr (FUSE) em_row_axpy<T, VEC, RMAX, XV>(tacc, &Bsh[jc][0], xn);
        }
        // 2 * RMAX vectors are live across the loop: keep the scheduler from interleaving the columns of one
        // unrolled group (it held four columns' temporaries at once and spilled at R = 20)
        if constexpr (FUSE) __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      ores += (double)s_ores[v]; ox2 += (double)s_ox2[v]; num += (double)s_num[v]; den += (double)s_den[v];
    }
  }
  if constexpr (FUSE) {
    if (g.in_range) {
      // rows i0 .. i0+VEC-1 of T at fixed index f: VEC*R contiguous values per thread, consecutive threads adjacent
      T* Tt = reinterpret_cast<T*>(a.T) + (int64_t)g.chunk * a.t_chunk_stride + (g.i0 + a.Ipad * g.f) * R;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if (R == RMAX && (RMAX * sizeof(T)) % 16 == 0) {
          constexpr int W = 16 / sizeof(T);
          typedef T TV __attribute__((ext_vector_type(W)));
#pragma unroll
          for (int r = 0; r < RMAX; r += W) {
            TV o;
#pragma unroll
            for (int q = 0; q < W; ++q) o[q] = tacc[r + q][v];
            *reinterpret_cast<TV*>(Tt + (int64_t)v * R + r) = o;
          }
        } else {
#pragma unroll
          for (int r = 0; r < RMAX; ++r)
            if (r < R) Tt[(int64_t)v * R + r] = tacc[r][v];
        }
      }
    }
  }
  em_store_stats(num, den, ores, ox2, sh4, ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// One row per thread, for R > 32 (the rows of A no longer fit in registers VEC at a time): the policies at VEC = 1, no
// ring, each entry's terms (the squares, rounded once) straight into the fp64 sums, stores by entry.
template <typename T, int RMAX, template <typename, int> class POL>
__global__ __launch_bounds__(kEmThreads) void em_cp_k(EmCpArgs a, int jchunks, int64_t jlen, double* ws) {
  typedef typename EmVec<T, 1>::type XV;
  __shared__ T Bsh[kEmJTile][RMAX];
  __shared__ double sh4[4];
  const EmWalk<1> g(a, jchunks, jlen);
  XV areg[RMAX];
  em_load_rows<T, 1, RMAX, false>(a, g, areg);
  const POL<T, 1> pol(a, g);
  const XV zero = {};
  double num = 0, den = 0, ores = 0, ox2 = 0;
  for (int64_t j0 = g.jbeg; j0 < g.jend; j0 += kEmJTile) {
    em_stage_tile<T, 1, RMAX>(Bsh, g, a.R, j0);
    const int nj = (int)((g.jend - j0 < kEmJTile) ? (g.jend - j0) : kEmJTile);
    if (g.i0 >= a.I) continue;                                           // padding rows are skipped
    for (int jj = 0; jj < nj; ++jj) {
      const XV m = em_row_dot<T, 1, RMAX, XV>(areg, &Bsh[jj][0], zero);
      XV t_ores = zero, t_ox2 = zero, t_num = zero, t_den = zero;
      bool changes;
      const XV xn = pol.eval(pol.load(j0 + jj), j0 + jj, m, changes, t_ores, t_ox2, t_num, t_den);
      ores += (double)t_ores[0]; ox2 += (double)t_ox2[0]; num += (double)t_num[0]; den += (double)t_den[0];
      if (a.update && changes) *pol.at(j0 + jj) = xn;
    }
  }
  em_store_stats(num, den, ores, ox2, sh4, ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

template <typename T>
__global__ void em_w_reset_k(T* __restrict__ xh, const T* __restrict__ x0, const T* __restrict__ w, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) xh[e] = w[e] * x0[e];
}
void em_w_reset(void* xh, const void* x0, const void* w, int prec, int64_t n, hipStream_t s) {
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(n, (int64_t)256), 65536);
  if (prec == AOADMM_PREC_F32) em_w_reset_k<float><<<blocks, 256, 0, s>>>((float*)xh, (const float*)x0, (const float*)w, n);
  else em_w_reset_k<double><<<blocks, 256, 0, s>>>((double*)xh, (const double*)x0, (const double*)w, n);
  AO_KERNEL_CHECK();
}

__global__ void em_w_check_k(const double* __restrict__ w, int64_t n, int* flag) {
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    bad |= !(w[e] >= 0.0 && w[e] <= 1.0);                                // a NaN fails both comparisons
  if (bad) *flag = 1;
}
void em_w_check(const double* w, int64_t n, int* flag, hipStream_t s) {
  em_w_check_k<<<(unsigned)std::min<int64_t>(cdiv(n, (int64_t)256), 65536), 256, 0, s>>>(w, n, flag);
  AO_KERNEL_CHECK();
}

// out4[q] = sum_b ws[b][q], fixed order (256 threads, strided partial sums then a tree)
__global__ __launch_bounds__(256) void em_sum4_k(const double* ws, int64_t nb, double* out4) {
  __shared__ double sh4[4];
  double s[4] = {0, 0, 0, 0};
  for (int64_t b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += ws[b * 4 + q];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double tot = em_block_sum(s[q], sh4);
    if (threadIdx.x == 0) out4[q] = tot;
  }
}

// The walk is cut into pieces of whole 64-column tiles so that the launch has several thousand workgroups:
// with one workgroup per (strip, k) a matrix block would be one workgroup per strip.  A fused pass writes one chunk of T per
// piece, so it only cuts when the launch would not fill the chip, and never runs a piece past the contraction kernels'
// bound of 2048 terms accumulated in fp32.
static constexpr int64_t kEmTargetBlocks = 6144;
static constexpr int64_t kEmFuseBlocks = 768;
static constexpr int64_t kEmFuseMaxRun = 2048;
static void em_chunking(int64_t strips, int64_t NW, int64_t NF, bool fuse, int* jchunks, int64_t* jlen) {
  const int64_t tiles = cdiv(NW, (int64_t)kEmJTile);
  int64_t want = cdiv(fuse ? kEmFuseBlocks : kEmTargetBlocks, strips * NF);
  if (fuse && want < cdiv(NW, kEmFuseMaxRun)) want = cdiv(NW, kEmFuseMaxRun);
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  *jlen = cdiv(tiles, want) * kEmJTile;
  *jchunks = (int)cdiv(NW, *jlen);
}

static bool em_wide(const EmCpArgs& a) { return a.R <= 32; }
static int em_vec(const EmCpArgs& a, int prec) { return !em_wide(a) ? 1 : (prec == AOADMM_PREC_F32 ? 4 : 2); }

bool em_cp_can_fuse(const EmCpArgs& a, int prec) {
  (void)prec;
  return a.R <= kEmFuseMaxRank && a.C != nullptr;    // 2 * R vectors of registers per thread (rows of A and of T)
}

EmCpLaunch em_cp_launch_of(const EmCpArgs& a, int prec, bool fuse) {
  const bool wj = a.walk != 2;
  EmCpLaunch l;
  l.vec = em_vec(a, prec);
  l.rmax = em_wide(a) ? (a.R + 3) / 4 * 4 : 64;      // em_cp_launch's classes; em_cp_k<T, 64>
  l.strips = cdiv(a.Ipad, (int64_t)kEmThreads * l.vec);
  em_chunking(l.strips, wj ? a.J : a.K, wj ? a.K : a.J, fuse, &l.jchunks, &l.jlen);
  return l;
}

int em_cp_fused_chunks(const EmCpArgs& a, int prec) { return em_cp_launch_of(a, prec, true).jchunks; }

size_t em_cp_ws_bytes(int64_t Ipad, int64_t J, int64_t K) {
  // strips <= cdiv(Ipad, 256) (VEC >= 1), the fixed index runs over J or K, pieces <= cdiv(kEmTargetBlocks, strips * fixed):
  // never more workgroups than this
  return (size_t)(cdiv(Ipad, (int64_t)kEmThreads) * (J > K ? J : K) + kEmTargetBlocks) * 4 * sizeof(double);
}

// The kernel of one precision and policy for the launch `l`: the strip kernel of its rank class, fused where the policy
// and the class have a fused form (em_cp_pass has refused a fused pass that has none), or the one-row kernel
template <typename T, template <typename, int> class POL>
static void em_cp_launch(const EmCpArgs& a, const EmCpLaunch& l, bool fuse, double* ws, dim3 grid, hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  const auto strip = [&](auto rmax) {
    constexpr int RMAX = decltype(rmax)::value;
    if constexpr (POL<T, VEC>::kFuses && RMAX <= kEmFuseMaxRank) {
      if (fuse) return em_cp_vec_k<T, VEC, RMAX, true, POL><<<grid, kEmThreads, 0, s>>>(a, l.jchunks, l.jlen, ws);
    }
    em_cp_vec_k<T, VEC, RMAX, false, POL><<<grid, kEmThreads, 0, s>>>(a, l.jchunks, l.jlen, ws);
  };
  switch (l.rmax) {                                  // rank rounded up to a multiple of 4 (one ds_read_b128 of fp32)
    case 4: strip(std::integral_constant<int, 4>()); break;
    case 8: strip(std::integral_constant<int, 8>()); break;
    case 12: strip(std::integral_constant<int, 12>()); break;
    case 16: strip(std::integral_constant<int, 16>()); break;
    case 20: strip(std::integral_constant<int, 20>()); break;
    case 24: strip(std::integral_constant<int, 24>()); break;
    case 28: strip(std::integral_constant<int, 28>()); break;
    case 32: strip(std::integral_constant<int, 32>()); break;
    default: em_cp_k<T, 64, POL><<<grid, kEmThreads, 0, s>>>(a, l.jchunks, l.jlen, ws); break;
  }
}

void em_cp_pass(const EmCpArgs& a, int prec, double* ws, double* out4, hipStream_t s) {
  AO_REQUIRE(a.R >= 1 && a.R <= kMaxRank && a.I > 0 && a.J > 0 && a.K > 0, "em_cp_pass: bad sizes");
  const bool fuse = a.T != nullptr;
  const bool weighted = a.Wt != nullptr;
  AO_REQUIRE(!weighted || (a.X0 != nullptr && !fuse), "em_cp_pass: a weighted block needs X0 and takes no fused contraction");
  const bool wj = a.walk != 2;
  AO_REQUIRE((wj ? a.K : a.J) <= 65535, "em_cp_pass: mode too long for one launch");   // grid.y = the fixed index
  AO_REQUIRE(!fuse || em_cp_can_fuse(a, prec), "em_cp_pass: this block cannot take the fused contraction");
  AO_REQUIRE(wj || a.C != nullptr, "em_cp_pass: a matrix block has no third mode to walk");
  const EmCpLaunch l = em_cp_launch_of(a, prec, fuse);
  const dim3 grid((unsigned)(l.strips * l.jchunks), (unsigned)(wj ? a.K : a.J));
  AO_REQUIRE((size_t)grid.x * grid.y * 4 * sizeof(double) <= em_cp_ws_bytes(a.Ipad, a.J, a.K), "em_cp_pass: workspace");
  if (prec == AOADMM_PREC_F32) {
    if (weighted) em_cp_launch<float, EmWeighted>(a, l, fuse, ws, grid, s);
    else em_cp_launch<float, EmMasked>(a, l, fuse, ws, grid, s);
  } else {
    if (weighted) em_cp_launch<double, EmWeighted>(a, l, fuse, ws, grid, s);
    else em_cp_launch<double, EmMasked>(a, l, fuse, ws, grid, s);
  }
  AO_KERNEL_CHECK();
  em_sum4_k<<<1, 256, 0, s>>>(ws, (int64_t)grid.x * grid.y, out4);
  AO_KERNEL_CHECK();
}

// PARAFAC2: one workgroup per slab, M_k = A diag(C(k,:)) B_k'  (:423-433, :1249-1252)
__global__ __launch_bounds__(256) void em_par2_k(EmPar2Args a, double* ws) {
  __shared__ double sh4[4];
  const int k = blockIdx.x;
  const int64_t o = a.off[k];
  const int Jk = (int)(a.off[k + 1] - o);
  double* X = a.X + (int64_t)a.I * o;
  const uint8_t* M = a.mask + (int64_t)a.I * o;
  const double* Bk = a.B + o * a.R;
  double num = 0, den = 0, ores = 0, ox2 = 0;
  for (int e = threadIdx.x; e < a.I * Jk; e += 256) {
    const int j = e / a.I, i = e - j * a.I;
    double m = 0.0;
    for (int r = 0; r < a.R; ++r) m += a.A[i + (int64_t)a.I * r] * a.C[k + (int64_t)a.K * r] * Bk[j + (int64_t)Jk * r];
    const double x = X[e];
    if (M[e]) {
      ores += (x - m) * (x - m);
      ox2 += x * x;
    } else {
      num += (m - x) * (m - x);
      den += x * x;
      if (a.update) X[e] = m;
    }
  }
  em_store_stats(num, den, ores, ox2, sh4, ws + (int64_t)k * 4);
}

void em_par2_pass(const EmPar2Args& a, double* ws, double* out4, hipStream_t s) {
  em_par2_k<<<a.K, 256, 0, s>>>(a, ws);
  AO_KERNEL_CHECK();
  em_sum4_k<<<1, 256, 0, s>>>(ws, a.K, out4);
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
