// Tensor-pass kernels for gfx950 (MI355X).
//
// The hot operation of AO-ADMM is mttkrp(X,U,n) (reference call site
// functions/cmtf_fun_AOADMM.m:97, third-party Tensor Toolbox).  Here it is
// split into
//   (1) one streaming pass over the tensor that contracts ONE mode with its
//       factor matrix on the matrix cores (contract16_f32 / contract_f64; the
//       LDS-transposed contract_lead16_f32 when the contracted mode is the
//       contiguous one and no mode-permuted copy exists), giving T[m][r], and
//   (2) a small elementwise-multiply-and-reduce over T (reduce_inner / _outer).
// (1) reads every tensor element exactly once with 16-byte coalesced loads
// straight into MFMA operand registers (the unfolding's row index is the
// contiguous one, so no LDS staging is needed); T is ~R/C of the tensor
// bytes.  T is reusable for two modes (dimension tree), which is what cuts
// the tensor reads per outer iteration from 3 to 1.5.
//
// f32: v_mfma_f32_16x16x4_f32, lane l holds A[row l&15][k=l>>4], B[k=l>>4][col l&15];
//      a lane's float4 load gives rows 4*(l&15)+v (v=0..3) of column k, i.e. four
//      MFMA row tiles.  f64: v_mfma_f64_16x16x4_f64, same operand map; a double2 load
//      gives rows 2*(l&15)+v.  (A first version used v_mfma_f32_32x32x2_f32: at R = 20 it
//      issues 32 columns of matrix work per entry and ran 5.8 ms per 2000^3 pass against
//      5.2 ms for 16 MFMA columns + 4 on the vector pipe.)
#include "contract.h"
#include "device_utils.h"
#include "small_dev.h"

#include <algorithm>
#include <cstdlib>

namespace aoadmm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

static constexpr int kTileRows = 128;     // rows of the unfolding per wave
static constexpr int kGroup = 8;          // reduction columns per pipeline stage

// ---------------------------------------------------------------------------
// operand packing: factor matrix (C x R, fp64 col-major) -> MFMA B fragments
// ---------------------------------------------------------------------------
// arguments of the register-streaming contractions (contract16_f32, contract_f64)
struct KArgs {
  const void* X;
  const void* frag;
  void* T;             // float (f32 tensors) or double (f64 tensors), [nchunk][trows][R]
  int64_t tiles_per_batch, ntiles, batch_stride, M, ld, C, Cg, trows;
  int groups_per_chunk, R;
  int flush_every;     // contract16_f32<1, *, true>: steady-state loop rounds (24 columns each) between two flushes of the
                       // fp32 accumulators into the fp64 second-level sums
};

// ---------------------------------------------------------------------------
// f32 contraction, 16-column tiles: v_mfma_f32_16x16x4_f32 for the first 16*NT columns of the factor and,
// when the rank leaves 1..4 columns over (R = 20: the headline configuration), packed-fp32 VALU FMAs for
// those instead of a second, mostly empty MFMA tile.  At R = 20 the 32x32x2 form issues 32 columns of
// matrix work per tensor element; this kernel issues 16 on the matrix pipe + 4 on the vector pipe, which
// halves the matrix-pipe time the streaming loads have to overlap with.
//   A operand: lane l holds A[row l&15][k = l>>4]; a lane's float4 load gives rows 4*(l&15)+v of column
//   c + (l>>4): MFMA row tile (half, v) holds rows 64*half + 4*j + v, j = 0..15.
//   B operand: lane l holds F[c + (l>>4)][16nt + (l&15)]  (packed float2 per 8-column group: kk = 0, 1).
//   Extra columns: lane l multiplies its four rows by F[c + (l>>4)][16NT + e], e = 0..3 (one float4 per
//   4-column group, shared by the 16 lanes of a quarter wave); the four k-quarters are added at the end.
// ---------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

// main: frag[nt][g][lane] float2 = F[8g + 4kk + (lane>>4)][16nt + (lane&15)], kk = 0,1
// extra (after the main block): fe[g][kk][q] float4 = F[8g + 4kk + q][16NT + e], e = 0..3
__global__ void pack_frag16_f32(const double* __restrict__ F, int64_t ldF, int64_t C, int R, int NT, int EX,
                                int64_t Cg, float* __restrict__ frag) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nmain = (int64_t)NT * Cg * 128;
  if (idx < nmain) {
    const int kk = idx & 1;
    const int lane = (idx >> 1) & 63;
    const int64_t g = (idx >> 7) % Cg;
    const int nt = (int)((idx >> 7) / Cg);
    const int64_t c = 8 * g + 4 * kk + (lane >> 4);
    const int r = 16 * nt + (lane & 15);
    frag[idx] = (c < C && r < R) ? (float)F[c + ldF * r] : 0.f;
  } else if (EX && idx < nmain + Cg * 32) {
    const int64_t j = idx - nmain;
    const int e = j & 3, q = (j >> 2) & 3, kk = (j >> 4) & 1;
    const int64_t g = j >> 5;
    const int64_t c = 8 * g + 4 * kk + q;
    const int r = 16 * NT + e;
    frag[idx] = (c < C && r < R) ? (float)F[c + ldF * r] : 0.f;
  }
}

// Sum over the four 16-lane quarters of a wave of FOUR values at once, dealt out: quarter q of the result holds the
// total of value q (lanes l, l^16, l^32, l^48 hold partial sums of the same rows).  gfx950's half-exchange permutes do it
// in 3 swaps + 3 adds: v_permlane16_swap (odd rows of the first operand <-> even rows of the second) on (a, b) and
// (c, d), then v_permlane32_swap (upper half of the first <-> lower half of the second) on the two sums.
__device__ __forceinline__ float quarter_sum4(float a, float b, float c, float d) {
  const auto ab = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  const auto cd = __builtin_amdgcn_permlane16_swap(__float_as_uint(c), __float_as_uint(d), false, false);
  const float s_ab = __uint_as_float(ab[0]) + __uint_as_float(ab[1]);   // rows: a01, b01, a23, b23
  const float s_cd = __uint_as_float(cd[0]) + __uint_as_float(cd[1]);   // rows: c01, d01, c23, d23
  const auto x = __builtin_amdgcn_permlane32_swap(__float_as_uint(s_ab), __float_as_uint(s_cd), false, false);
  return __uint_as_float(x[0]) + __uint_as_float(x[1]);                 // rows: a, b, c, d
}

// L2 (NT = 1 only, i.e. R <= 20: the headline rank): two-level accumulation.  The MFMA adds into an fp32 accumulator;
// a run of 500 dependent adds (2000 columns) leaves a relative error of ~13 * 2^-24 in an entry of T, which after the
// reductions and 25 outer iterations showed as 2e-8..6e-8 in the factors against the fp64 tensor mode -- outside the
// 1e-8 of north_star.  With L2 the fp32 accumulators are flushed every `flush_every` loop rounds (kFlushEvery = 3: 72
// columns = 18 adds) into fp64 sums and cleared: the 32 MFMA accumulators of a lane into the wave's own 16 KB slice of
// LDS ([acc index][lane] doubles, conflict-free), the 32 packed-FMA accumulators of the leftover columns are first added over the four k-quarters
// of the wave (quarter_sum4) and then into 8 fp64 registers (the VGPR budget at two waves per SIMD, 256, has no room
// for 64 more register pairs: the kernel uses 202).
// What is left is the rounding of the finished sum to the fp32 entry of T (2^-25 relative, independent per entry).
// The flush is ~130 VALU/LDS instructions per 144 MFMAs of a wave and overlaps with the other wave's matrix work.
constexpr int kFlushEvery = 3;
template <int NT, bool EX, bool L2 = false>
__global__ __launch_bounds__(256, NT <= 2 ? 2 : 1) void contract16_f32(KArgs a) {
  static_assert(!L2 || NT == 1, "two-level accumulation exists for one 16-column tile (R <= 20)");
  const int lane = threadIdx.x & 63;
  const int64_t wt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wt >= a.ntiles) return;                       // wave-uniform
  const int chunk = blockIdx.y;
  const int64_t b = wt / a.tiles_per_batch;
  const int64_t m0 = (wt - b * a.tiles_per_batch) * kTileRows;
  const int r16 = lane & 15, q = lane >> 4;
  int64_t row0 = m0 + 4 * r16, row1 = m0 + 64 + 4 * r16;
  if (row0 >= a.M) row0 = m0;                        // padding lanes re-read a valid row; never stored
  if (row1 >= a.M) row1 = m0;
  const int64_t g0 = (int64_t)chunk * a.groups_per_chunk;
  int64_t g1 = g0 + a.groups_per_chunk;
  if (g1 > a.Cg) g1 = a.Cg;
  const int64_t gfull = (a.C / kGroup < g1) ? a.C / kGroup : g1;   // groups with all 8 columns valid
  const float* X = reinterpret_cast<const float*>(a.X) + b * a.batch_stride;
  const float* xp0 = X + row0 + (kGroup * g0 + q) * a.ld;
  const float* xp1 = X + row1 + (kGroup * g0 + q) * a.ld;
  const int64_t ld4 = 4 * a.ld;
  const f32x2* fp = reinterpret_cast<const f32x2*>(a.frag) + g0 * 64 + lane;
  const int64_t fnt = a.Cg * 64;                     // float2 stride between N tiles
  const f32x4* fe = reinterpret_cast<const f32x4*>(reinterpret_cast<const f32x2*>(a.frag) + (int64_t)NT * a.Cg * 64) + g0 * 8 + q;

  f32x4 acc[NT][2][4];
  f32x2 accE[2][4][2];                                // [half][v][column pair]
  // in-place packed FMA with the low / high float of X broadcast to both halves
#define AO_PKFMA_LO(ACC, X2, E2) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(ACC) : "v"(X2), "v"(E2));
#define AO_PKFMA_HI(ACC, X2, E2) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(ACC) : "v"(X2), "v"(E2));
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      accE[h][v][0] = f32x2{0.f, 0.f};
      accE[h][v][1] = f32x2{0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt][h][v] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  // second-level sums (L2): [(h*4 + v)*4 + i][lane] doubles in the wave's 16 KB LDS slice; leftover columns in registers
  extern __shared__ __attribute__((aligned(16))) float t_lds[];
  double* l2 = reinterpret_cast<double*>(t_lds) + (threadIdx.x >> 6) * 2048 + lane;
  double accE2[2][4];                                 // lane (r16, q): row 64h + 4 r16 + v, leftover column q
  if (L2) {
#pragma unroll
    for (int k = 0; k < 32; ++k) l2[k * 64] = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 4; ++v) accE2[h][v] = 0.0;
  }
  // eight accumulators per batch (sched_barrier in between): all 32 LDS reads at once would need 64 more registers
#define AO_FLUSH()                                                                                   \
  {                                                                                                  \
    _Pragma("unroll") for (int h = 0; h < 2; ++h) {                                                  \
      _Pragma("unroll") for (int vb = 0; vb < 4; vb += 2) {                                          \
        _Pragma("unroll") for (int v = vb; v < vb + 2; ++v)                                          \
          _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                            \
            l2[((h * 4 + v) * 4 + i) * 64] += (double)acc[0][h][v][i];                               \
            acc[0][h][v][i] = 0.f;                                                                   \
          }                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                           \
      }                                                                                              \
    }                                                                                                \
    if (EX) {      /* the four k-quarters of a row's four leftover columns, added and dealt out: quarter q keeps column q */ \
      _Pragma("unroll") for (int h = 0; h < 2; ++h)                                                  \
        _Pragma("unroll") for (int v = 0; v < 4; ++v) {                                              \
          accE2[h][v] += (double)quarter_sum4(accE[h][v][0][0], accE[h][v][0][1], accE[h][v][1][0], accE[h][v][1][1]); \
          accE[h][v][0] = f32x2{0.f, 0.f};                                                           \
          accE[h][v][1] = f32x2{0.f, 0.f};                                                           \
        }                                                                                            \
    }                                                                                                \
  }
  // register ring of three 8-column stages; x index s = 2*kk + half
  f32x4 x0[4], x1[4], x2[4], e0[2], e1[2], e2[2];
  f32x2 f0[NT], f1[NT], f2[NT];
  const int64_t ng = gfull > g0 ? gfull - g0 : 0;
  const int64_t gstep = kGroup * a.ld;
#define AO_LOAD1(XS, GI, S)                                                                          \
  XS[S] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>((((S) & 1) ? xp1 : xp0) + (GI) * gstep + ((S) >> 1) * ld4));
#define AO_LOADF(FS, ES, GI)                                                                         \
  {                                                                                                  \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) FS[nt] = fp[(GI) * 64 + nt * fnt];            \
    if (EX) { ES[0] = fe[(GI) * 8]; ES[1] = fe[(GI) * 8 + 4]; }                                      \
  }
#define AO_LOAD_STAGE(XS, FS, ES, GI)                                                                \
  { AO_LOAD1(XS, GI, 0) AO_LOAD1(XS, GI, 1) AO_LOAD1(XS, GI, 2) AO_LOAD1(XS, GI, 3) AO_LOADF(FS, ES, GI) }
#define AO_FMA_S(XS, FS, ES, S)                                                                      \
  {                                                                                                  \
    _Pragma("unroll") for (int v = 0; v < 4; ++v) {                                                  \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                              \
        acc[nt][(S) & 1][v] = __builtin_amdgcn_mfma_f32_16x16x4f32(XS[S][v], FS[nt][(S) >> 1], acc[nt][(S) & 1][v], 0, 0, 0); \
    }                                                                                                \
    if (EX) {      /* accE[half][v][0..3] += x[v] * e[0..3]: two packed FMAs per row, x broadcast by op_sel */ \
      const f32x2 xlo_ = __builtin_shufflevector(XS[S], XS[S], 0, 1), xhi_ = __builtin_shufflevector(XS[S], XS[S], 2, 3); \
      const f32x2 ea_ = __builtin_shufflevector(ES[(S) >> 1], ES[(S) >> 1], 0, 1);                   \
      const f32x2 eb_ = __builtin_shufflevector(ES[(S) >> 1], ES[(S) >> 1], 2, 3);                   \
      AO_PKFMA_LO(accE[(S) & 1][0][0], xlo_, ea_) AO_PKFMA_LO(accE[(S) & 1][0][1], xlo_, eb_)        \
      AO_PKFMA_HI(accE[(S) & 1][1][0], xlo_, ea_) AO_PKFMA_HI(accE[(S) & 1][1][1], xlo_, eb_)        \
      AO_PKFMA_LO(accE[(S) & 1][2][0], xhi_, ea_) AO_PKFMA_LO(accE[(S) & 1][2][1], xhi_, eb_)        \
      AO_PKFMA_HI(accE[(S) & 1][3][0], xhi_, ea_) AO_PKFMA_HI(accE[(S) & 1][3][1], xhi_, eb_)        \
    }                                                                                                \
  }
#define AO_COMPUTE_STAGE(XS, FS, ES) { AO_FMA_S(XS, FS, ES, 0) AO_FMA_S(XS, FS, ES, 1) AO_FMA_S(XS, FS, ES, 2) AO_FMA_S(XS, FS, ES, 3) }
  // consume stage (XC,FC,EC) while fetching stage GI into (XL,FL,EL): one load between MFMA groups
#define AO_MIX_STAGE(XC, FC, EC, XL, FL, EL, GI)                                                     \
  {                                                                                                  \
    AO_FMA_S(XC, FC, EC, 0) AO_LOAD1(XL, GI, 0) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 1) AO_LOAD1(XL, GI, 1) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 2) AO_LOAD1(XL, GI, 2) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 3) AO_LOAD1(XL, GI, 3) AO_LOADF(FL, EL, GI) __builtin_amdgcn_sched_barrier(0); \
  }
  // The same stage, every load pinned in the order the steady state issues them (x[0..3], fragment, leftover-column
  // fragments).  The compiler derives the loop's s_waitcnt operands from the loads pending on EVERY path into the loop
  // header and keeps the strictest: with a conditional, freely scheduled prologue in front of it the header got a static
  // vmcnt(2) and the ring was drained once per revolution.  The steady loop is therefore entered only through this
  // prologue (ng >= 5: both stages are in range), and chunks too short for it never pass the loop header.
#define AO_LOAD_STAGE_ORDERED(XS, FS, ES, GI)                                                        \
  {                                                                                                  \
    AO_LOAD1(XS, GI, 0) __builtin_amdgcn_sched_barrier(0);                                           \
    AO_LOAD1(XS, GI, 1) __builtin_amdgcn_sched_barrier(0);                                           \
    AO_LOAD1(XS, GI, 2) __builtin_amdgcn_sched_barrier(0);                                           \
    AO_LOAD1(XS, GI, 3) __builtin_amdgcn_sched_barrier(0);                                           \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                              \
      FS[nt] = fp[(GI) * 64 + nt * fnt];                                                             \
      __builtin_amdgcn_sched_barrier(0);                                                             \
    }                                                                                                \
    if (EX) {                                                                                        \
      ES[0] = fe[(GI) * 8];                                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      ES[1] = fe[(GI) * 8 + 4];                                                                      \
      __builtin_amdgcn_sched_barrier(0);                                                             \
    }                                                                                                \
  }
  int64_t g = 0;
  int since_flush = 0;
  if (ng >= 5) {
    AO_LOAD_STAGE_ORDERED(x0, f0, e0, 0)
    AO_LOAD_STAGE_ORDERED(x1, f1, e1, 1)
    do {                                             // steady state: every prefetch is in range
      AO_MIX_STAGE(x0, f0, e0, x2, f2, e2, g + 2)
      AO_MIX_STAGE(x1, f1, e1, x0, f0, e0, g + 3)
      AO_MIX_STAGE(x2, f2, e2, x1, f1, e1, g + 4)
      if (L2 && ++since_flush == a.flush_every) {    // the next stages' loads are in flight behind this
        since_flush = 0;
        AO_FLUSH()
      }
      g += 3;
    } while (g + 5 <= ng);
  } else {                                           // 0..4 full groups: no steady state
    if (ng > 0) AO_LOAD_STAGE(x0, f0, e0, 0)
    if (ng > 1) AO_LOAD_STAGE(x1, f1, e1, 1)
  }
  if (g + 3 <= ng) {                                 // one drained round
    if (g + 2 < ng) AO_LOAD_STAGE(x2, f2, e2, g + 2)
    AO_COMPUTE_STAGE(x0, f0, e0)
    if (g + 3 < ng) AO_LOAD_STAGE(x0, f0, e0, g + 3)
    AO_COMPUTE_STAGE(x1, f1, e1)
    if (g + 4 < ng) AO_LOAD_STAGE(x1, f1, e1, g + 4)
    AO_COMPUTE_STAGE(x2, f2, e2)
    g += 3;
  }
  if (g < ng) AO_COMPUTE_STAGE(x0, f0, e0)
  if (g + 1 < ng) AO_COMPUTE_STAGE(x1, f1, e1)
  g = gfull > g0 ? gfull : g0;
  // ragged tail group: columns >= C are clamped (finite data) and meet zero B fragments
  if (g < g1) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int64_t c = kGroup * g + 4 * (s >> 1) + q;
      if (c >= a.C) c = a.C - 1;
      x0[s] = *reinterpret_cast<const f32x4*>(X + ((s & 1) ? row1 : row0) + c * a.ld);
    }
    {
      const f32x2* fpt = reinterpret_cast<const f32x2*>(a.frag) + g * 64 + lane;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) f0[nt] = fpt[nt * fnt];
      if (EX) {
        const f32x4* fet = reinterpret_cast<const f32x4*>(reinterpret_cast<const f32x2*>(a.frag) + (int64_t)NT * a.Cg * 64) + g * 8 + q;
        e0[0] = fet[0]; e0[1] = fet[4];
      }
    }
    AO_COMPUTE_STAGE(x0, f0, e0)
  }
  if (L2) AO_FLUSH()
#undef AO_FLUSH
#undef AO_PKFMA_LO
#undef AO_PKFMA_HI
#undef AO_LOAD1
#undef AO_LOADF
#undef AO_LOAD_STAGE
#undef AO_LOAD_STAGE_ORDERED
#undef AO_FMA_S
#undef AO_COMPUTE_STAGE
#undef AO_MIX_STAGE
  // epilogue.  16x16 C/D map: col = lane&15, row j = 4*(lane>>4) + reg; tile (half, v) row j is unfolding row
  // m0 + 64*half + 4*j + v.  The wave's 128 x R tile of T is ONE contiguous range of 512*R bytes, so it is assembled
  // in the wave's own slice of LDS and leaves as 16-byte, fully coalesced stores of whole cache lines.  (Storing the
  // C/D registers directly -- 4-byte stores, 64-byte pieces of 80-byte rows -- cost 0.4-1.1 ms of a 5.3 ms pass at
  // 2000^3: partial lines are read-modified-written in L2 and trickle into HBM between the reads, and how much that
  // hurts depends on where X and T happen to lie; tools/micro/pass_placement.hip)
  // (with L2 the wave's T tile takes the place of its second-level sums: 128*R*4 <= 16 KB, read out completely first)
  float* tl = L2 ? t_lds + (threadIdx.x >> 6) * 4096 : t_lds + (threadIdx.x >> 6) * (kTileRows * a.R);
  if (L2) {
    double d2[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) d2[k] = l2[k * 64];
    __builtin_amdgcn_sched_barrier(0);               // every read of the sums before the first write of the tile
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[0][h][v][i] = (float)d2[(h * 4 + v) * 4 + i];
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r = 16 * nt + r16;
    if (r < a.R) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int i = 0; i < 4; ++i) tl[(64 * h + 4 * (4 * q + i) + v) * a.R + r] = acc[nt][h][v][i];
    }
  }
  if (EX) {
    // add the four k-quarters (lanes l, l^16, l^32, l^48 hold the same rows), quarter 0 stores
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (L2) continue;                            // already added over the quarters at every flush
          float t = accE[h][v][e >> 1][e & 1];
          t += __shfl_xor(t, 16);
          t += __shfl_xor(t, 32);
          accE[h][v][e >> 1][e & 1] = t;
        }
    const int ne = a.R - 16 * NT;                    // 1..4 live extra columns
    if (L2) {
      if (q < ne) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int v = 0; v < 4; ++v) tl[(64 * h + 4 * r16 + v) * a.R + 16 * NT + q] = (float)accE2[h][v];
      }
    } else if (q == 0) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < ne) tl[(64 * h + 4 * r16 + v) * a.R + 16 * NT + e] = accE[h][v][e >> 1][e & 1];
    }
  }
  // a wave's LDS operations complete in order: its own writes are visible to its reads without a barrier
  {
    const int64_t rows_here = (a.M - m0 < kTileRows) ? a.M - m0 : kTileRows;      // multiple of 4 (padded layout)
    const int n16 = (int)(rows_here * a.R / 4);
    f32x4* dst = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.T) + ((int64_t)chunk * a.trows + b * a.M + m0) * a.R);
    const f32x4* src = reinterpret_cast<const f32x4*>(tl);
    // streaming stores: plain (write-back) stores left dirty lines of T in L2 whose evictions cut into the read stream
    // (5.1-5.8 ms per 2000^3 pass depending on where X and T lie; 4.8-5.2 ms with non-temporal stores)
    for (int c = lane; c < n16; c += 64) __builtin_nontemporal_store(src[c], dst + c);
  }
}

// ---------------------------------------------------------------------------
// f32 contraction of the LEADING (contiguous) mode:  T(m, r) = sum_i X[i + ld*m] * F(i, r)
// ---------------------------------------------------------------------------
// Used only when the resident copy for the pass that contracts mode 1 (cpblock.h CpBlock::copy[0]) is unavailable.  The
// reduction index is the contiguous one, so MFMA A operands (one unfolding row per lane) cannot be loaded
// straight from HBM: a workgroup streams a [128 rows m] x [64 i] tile (128 segments of 256 contiguous bytes)
// through registers into LDS (row stride 68 floats: ds_read_b128 of 16 rows at one column offset hits 16
// distinct 16-byte slots).  The four waves split the REDUCTION, not the rows, so one B fragment serves all row
// tiles (with rows split over waves B traffic equalled the tensor traffic and the kernel ran 25 % slower); B
// fragments are fetched one chunk ahead (their L2 latency cannot hide behind 0.4 us of MFMA work per chunk);
// the four partial tiles are summed through LDS and written as one contiguous block of T.  Loads of chunks
// c+2 / c+3 are in flight while chunk c is consumed; one barrier per chunk (double-buffered LDS).
static constexpr int kLeadRows = 128;   // unfolding rows per workgroup
static constexpr int kLeadKC = 64;      // reduction elements per chunk
static constexpr int kLeadStride = 68;  // LDS row stride in floats

struct LArgs {
  const float* X;
  const float* frag;
  float* T;
  int64_t M, ld, C, Cg;      // rows of the unfolding, row stride, reduction length, groups of 8
  int chunks_per_slice;      // 64-element chunks per accumulation slice (blockIdx.y)
  int R;
};

// ---------------------------------------------------------------------------
// Leading-mode contraction with 16-column tiles (same idea as contract16_f32): wave w multiplies all 128
// rows of the staged tile by the 16 i of its slice with v_mfma_f32_16x16x4_f32 (lane (j, q) holds row
// 16*tile + j, reduction index 4q + t in step t of its ds_read_b128).  Half the matrix-pipe work of the
// 32-column form at R <= 16.  (Leftover columns on the vector pipe, as in contract16_f32, did not pay here:
// the staging registers leave no room for the extra accumulators -- 6.4-6.8 ms against 6.2 ms for a second
// MFMA tile at R = 20.)
//   frag[nt][g16][lane] float4, component t = F[16 g16 + 4(lane>>4) + t][16nt + (lane&15)]
// ---------------------------------------------------------------------------
__global__ void pack_frag_lead16_f32(const double* __restrict__ F, int64_t ldF, int64_t C, int R, int NT,
                                     int64_t Cg16, float* __restrict__ frag) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nmain = (int64_t)NT * Cg16 * 256;
  if (idx < nmain) {
    const int t = idx & 3;
    const int lane = (idx >> 2) & 63;
    const int64_t g = (idx >> 8) % Cg16;
    const int nt = (int)((idx >> 8) / Cg16);
    const int64_t c = 16 * g + 4 * (lane >> 4) + t;
    const int r = 16 * nt + (lane & 15);
    frag[idx] = (c < C && r < R) ? (float)F[c + ldF * r] : 0.f;
  }
}

template <int NT>
__global__ __launch_bounds__(256, NT <= 2 ? 2 : 1) void contract_lead16_f32(LArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];      // [2][kLeadRows][kLeadStride]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * kLeadRows;
  const int slice = blockIdx.y;
  const int64_t nchunks_total = (a.C + kLeadKC - 1) / kLeadKC;
  const int64_t c0 = (int64_t)slice * a.chunks_per_slice;
  int64_t c1 = c0 + a.chunks_per_slice;
  if (c1 > nchunks_total) c1 = nchunks_total;
  const int64_t Cg16 = (a.C + 15) / 16;               // the packed fragments hold Cg16 + 1 groups, the last all zero
  // staging map: 8 x 16-byte loads per thread, thread -> (row = (tid>>4) + 16q, 4 floats at 4*(tid&15))
  const int srow = tid >> 4, scol = 4 * (tid & 15);
  // row q of this thread is m0 + srow + 16q, clamped to the last row in the tail tile (re-read, never
  // stored).  The eight row pointers are rebuilt at every load from one base and an opaque copy of the row
  // stride (otherwise the compiler hoists them: 16 VGPRs this kernel does not have)
  const unsigned mlast = (unsigned)((a.M - 1 - m0 < kLeadRows - 1) ? (a.M - 1 - m0) : (kLeadRows - 1));
  const float* xblk = a.X + m0 * a.ld;
  const int64_t last4 = a.ld - 4;                    // last 16-byte aligned group inside a row
  f32x4 acc[NT][8];
#pragma unroll
  for (int tl = 0; tl < 8; ++tl)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt][tl] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int r16 = lane & 15, q4 = lane >> 4;
  const f32x4* fbase = reinterpret_cast<const f32x4*>(a.frag) + lane;
  const int64_t fnt = (Cg16 + 1) * 64;
  f32x4 sA[8], sB[8];
  f32x4 fA[NT], fB[NT];
#define AO_LEAD_LOAD1(ST, CH, Q)                                                                     \
  {                                                                                                  \
    int64_t i_ = (CH) * kLeadKC + scol;                                                              \
    if (i_ > last4) i_ = last4;                                                                      \
    unsigned mq_ = srow + 16 * (Q);                                                                  \
    if (mq_ > mlast) mq_ = mlast;                                                                    \
    unsigned ldo_ = (unsigned)a.ld;                                                                  \
    asm volatile("" : "+s"(ldo_));                                                                   \
    ST[Q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(xblk + (uint64_t)mq_ * ldo_ + i_)); \
  }
#define AO_LEAD_LOAD(ST, CH) { _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) AO_LEAD_LOAD1(ST, CH, q_) }
#define AO_LEAD_WRITE(ST, BUF)                                                                       \
  {                                                                                                  \
    float* base_ = lds + (BUF) * (kLeadRows * kLeadStride);                                          \
    _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_)                                                 \
      *reinterpret_cast<f32x4*>(base_ + (srow + 16 * q_) * kLeadStride + scol) = ST[q_];             \
  }
  // B fragments of this wave's 16-i group, fetched one chunk ahead
#define AO_LEAD_FRAG(FV, CH)                                                                         \
  {                                                                                                  \
    int64_t gg = (CH) * (kLeadKC / 16) + w;                                                          \
    if (gg > Cg16) gg = Cg16;                                          /* ragged last chunk: the zero group */ \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) FV[nt] = fbase[nt * fnt + gg * 64];            \
  }
#define AO_LEAD_TILE(XV, TL, FV)                                                                     \
  {                                                                                                  \
    _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                    \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                              \
        acc[nt][TL] = __builtin_amdgcn_mfma_f32_16x16x4f32(XV[t], FV[nt][t], acc[nt][TL], 0, 0, 0);  \
  }
  // consume this wave's 16 i of chunk CH from LDS buffer BUF; meanwhile fetch the next chunk's fragments
  // (if NF) and refill register set ST with chunk CHN (if PF): one staging load per row tile
#define AO_LEAD_COMPUTE(BUF, CH, FV, FVN, NF, ST, CHN, PF)                                           \
  {                                                                                                  \
    const float* xs_ = lds + (BUF) * (kLeadRows * kLeadStride) + r16 * kLeadStride + 16 * w + 4 * q4; \
    if (NF) AO_LEAD_FRAG(FVN, (CH) + 1)                                                              \
    _Pragma("unroll") for (int hb = 0; hb < 2; ++hb) {                                               \
      f32x4 xv_[4];                                                                                  \
      _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)           /* (macro arguments mention the caller's k) */ \
        xv_[j_] = *reinterpret_cast<const f32x4*>(xs_ + 16 * (4 * hb + j_) * kLeadStride);           \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                             \
        AO_LEAD_TILE(xv_[j_], 4 * hb + j_, FV)                                                       \
        if (PF) AO_LEAD_LOAD1(ST, CHN, 4 * hb + j_)                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                           \
      }                                                                                              \
    }                                                                                                \
  }
  const int64_t n = c1 > c0 ? c1 - c0 : 0;
  if (n > 0) {
    AO_LEAD_LOAD(sA, c0)
    AO_LEAD_FRAG(fA, c0)
    AO_LEAD_WRITE(sA, 0)
  }
  if (n > 1) AO_LEAD_LOAD(sA, c0 + 1)
  if (n > 2) AO_LEAD_LOAD(sB, c0 + 2)
  __syncthreads();
#pragma nounroll
  for (int64_t k = 0; k < n; k += 2) {
    if (k + 1 < n) AO_LEAD_WRITE(sA, 1)
    if (k + 3 < n) AO_LEAD_COMPUTE(0, c0 + k, fA, fB, true, sA, c0 + k + 3, true)
    else if (k + 1 < n) AO_LEAD_COMPUTE(0, c0 + k, fA, fB, true, sA, c0, false)
    else AO_LEAD_COMPUTE(0, c0 + k, fA, fB, false, sA, c0, false)
    __syncthreads();
    if (k + 1 >= n) break;
    if (k + 2 < n) AO_LEAD_WRITE(sB, 0)
    if (k + 4 < n) AO_LEAD_COMPUTE(1, c0 + k + 1, fB, fA, true, sB, c0 + k + 4, true)
    else if (k + 2 < n) AO_LEAD_COMPUTE(1, c0 + k + 1, fB, fA, true, sB, c0, false)
    else AO_LEAD_COMPUTE(1, c0 + k + 1, fB, fA, false, sB, c0, false)
    __syncthreads();
  }
#undef AO_LEAD_LOAD1
#undef AO_LEAD_LOAD
#undef AO_LEAD_WRITE
#undef AO_LEAD_FRAG
#undef AO_LEAD_TILE
#undef AO_LEAD_COMPUTE
  // sum the four waves' partial tiles through LDS, 16 columns per round, region w: [128][17];
  // the 128 x R block of T is contiguous in memory and is written with flat coalesced stores
  __syncthreads();
  constexpr int kEpiStride = 17;
  float* Tc = a.T + (int64_t)slice * a.M * a.R + m0 * a.R;
  const int64_t rows_here = (a.M - m0 < kLeadRows) ? (a.M - m0) : kLeadRows;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    float* reg = lds + w * (kLeadRows * kEpiStride);
#pragma unroll
    for (int tl = 0; tl < 8; ++tl)
#pragma unroll
      for (int i = 0; i < 4; ++i) reg[(16 * tl + 4 * q4 + i) * kEpiStride + r16] = acc[nt][tl][i];
    __syncthreads();
    int ncol = a.R - 16 * nt;                        // columns of this round
    if (ncol > 16) ncol = 16;
    const int total = (int)rows_here * ncol;
    for (int e = tid; e < total; e += 256) {
      const int row = e / ncol, col = e - row * ncol;
      const float* p = lds + row * kEpiStride + col;
      const float v = (p[0] + p[kLeadRows * kEpiStride]) + (p[2 * kLeadRows * kEpiStride] + p[3 * kLeadRows * kEpiStride]);
      Tc[(int64_t)row * a.R + 16 * nt + col] = v;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// f64 contraction (parity mode): v_mfma_f64_16x16x4_f64, same structure as contract16_f32
// ---------------------------------------------------------------------------
//   A operand: lane (r2 = l&15, q = l>>4) holds A[row r2][k = q]; a lane's double2 load brings rows 32j + 2*r2 + v
//   (v = 0, 1) of column c + q, so a wave owns 64 rows (j = 0, 1): 512 bytes per column, as in the fp32 kernel.
//   B operand: lane (r2, q) holds F[c + q][16nt + r2].  C/D map of the f64 MFMA: col = l&15, tile row = (l>>4) + 4*reg.
//   Leftover columns (R mod 16 in 1..4, R > 16: R = 20 is the headline rank) go to the vector pipe: lane (r2, q)
//   multiplies its rows by F[c + q][16NT + e], e = 0..3 (v_fma_f64 runs at the MFMA's fp64 rate on this chip), the four
//   k-quarters are added at the end.  A second, mostly empty MFMA tile doubled the matrix-pipe time: 6.5 ms of matrix
//   work against an 8.1 ms HBM floor at 2000^3, R = 20 (round 1: 14.0 ms per pass).
//   Register ring of three 8-column stages with the next stages' loads issued between MFMA groups (two stages, each
//   refilled in place between its own MFMA groups, in the leftover-column form: three need 290 registers).  The steady
//   loops are entered only through an ordered prologue (see contract16_f32); the T tile is assembled in LDS
//   and stored with coalesced streaming stores (see contract16_f32).  2000^3, R = 20: 10.1-10.3 ms per pass
//   (6.3-6.4 TB/s algorithmic); MFMA tiles only with three stages: 10.2-10.3 ms (tools/micro/pass_f64.hip).
static constexpr int kTileRows64 = 64;

// main: frag[nt][g][lane] double2 = F[8g + 4e + (lane>>4)][16nt + (lane&15)], e = 0, 1
// extra (after the main block): fe[g][e][q] double4 = F[8g + 4e + q][16NT + c], c = 0..3
__global__ void pack_frag_f64(const double* __restrict__ F, int64_t ldF, int64_t C, int R, int NT, int EX,
                              int64_t Cg, double* __restrict__ frag) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nmain = (int64_t)NT * Cg * 128;
  if (idx < nmain) {
    const int e = idx & 1;
    const int lane = (idx >> 1) & 63;
    const int64_t g = (idx >> 7) % Cg;
    const int nt = (int)((idx >> 7) / Cg);
    const int64_t c = 8 * g + 4 * e + (lane >> 4);
    const int r = 16 * nt + (lane & 15);
    frag[idx] = (c < C && r < R) ? F[c + ldF * r] : 0.0;
  } else if (EX && idx < nmain + Cg * 32) {
    const int64_t j = idx - nmain;
    const int col = j & 3, q = (j >> 2) & 3, e = (j >> 4) & 1;
    const int64_t g = j >> 5;
    const int64_t c = 8 * g + 4 * e + q;
    const int r = 16 * NT + col;
    frag[idx] = (c < C && r < R) ? F[c + ldF * r] : 0.0;
  }
}

template <int NT, bool EX>
__global__ __launch_bounds__(256, NT <= 2 ? 2 : 1) void contract_f64(KArgs a) {
  constexpr int RING = EX ? 2 : 3;                   // the leftover-column form has no registers for a third stage
  const int lane = threadIdx.x & 63;
  const int64_t wt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wt >= a.ntiles) return;                        // wave-uniform
  const int chunk = blockIdx.y;
  const int64_t b = wt / a.tiles_per_batch;
  const int64_t m0 = (wt - b * a.tiles_per_batch) * kTileRows64;
  const int r2 = lane & 15, q = lane >> 4;
  int64_t row0 = m0 + 2 * r2, row1 = m0 + 32 + 2 * r2;
  if (row0 >= a.M) row0 = m0;                        // padding lanes re-read a valid row; never stored
  if (row1 >= a.M) row1 = m0;
  const int64_t g0 = (int64_t)chunk * a.groups_per_chunk;
  int64_t g1 = g0 + a.groups_per_chunk;
  if (g1 > a.Cg) g1 = a.Cg;
  const int64_t gfull = (a.C / kGroup < g1) ? a.C / kGroup : g1;   // groups with all 8 columns valid
  const double* X = reinterpret_cast<const double*>(a.X) + b * a.batch_stride;
  const double* xp0 = X + row0 + (kGroup * g0 + q) * a.ld;
  const double* xp1 = X + row1 + (kGroup * g0 + q) * a.ld;
  const int64_t ld4 = 4 * a.ld;
  const f64x2* fp = reinterpret_cast<const f64x2*>(a.frag) + g0 * 64 + lane;
  const int64_t fnt = a.Cg * 64;                     // double2 stride between N tiles
  const f64x4* fe = reinterpret_cast<const f64x4*>(reinterpret_cast<const f64x2*>(a.frag) + (int64_t)NT * a.Cg * 64) + g0 * 8 + q;

  f64x4 acc[NT][2][2];                               // [nt][j][v]
  f64x4 accE[2][2];                                  // [j][v], the four leftover columns
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      accE[j][v] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt][j][v] = f64x4{0.0, 0.0, 0.0, 0.0};
    }

  // register ring of three 8-column stages; x index s = 2*e + j (e: column half of the group, j: row half of the tile)
  f64x2 x0[4], x1[4], x2[4];
  f64x4 e0[2], e1[2], e2[2];
  f64x2 f0[NT], f1[NT], f2[NT];
  const int64_t ng = gfull > g0 ? gfull - g0 : 0;
  const int64_t gstep = kGroup * a.ld;
#define AO_LOAD1(XS, GI, S)                                                                          \
  XS[S] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>((((S) & 1) ? xp1 : xp0) + (GI) * gstep + ((S) >> 1) * ld4));
#define AO_LOADF(FS, ES, GI)                                                                         \
  {                                                                                                  \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) FS[nt] = fp[(GI) * 64 + nt * fnt];            \
    if (EX) { ES[0] = fe[(GI) * 8]; ES[1] = fe[(GI) * 8 + 4]; }                                      \
  }
#define AO_LOAD_STAGE(XS, FS, ES, GI)                                                                \
  { AO_LOAD1(XS, GI, 0) AO_LOAD1(XS, GI, 1) AO_LOAD1(XS, GI, 2) AO_LOAD1(XS, GI, 3) AO_LOADF(FS, ES, GI) }
#define AO_FMA_S(XS, FS, ES, S)                                                                      \
  {                                                                                                  \
    _Pragma("unroll") for (int v = 0; v < 2; ++v) {                                                  \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                              \
        acc[nt][(S) & 1][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(XS[S][v], FS[nt][(S) >> 1], acc[nt][(S) & 1][v], 0, 0, 0); \
      if (EX) {                                                                                      \
        _Pragma("unroll") for (int c = 0; c < 4; ++c)                                                \
          accE[(S) & 1][v][c] = __builtin_fma(XS[S][v], ES[(S) >> 1][c], accE[(S) & 1][v][c]);       \
      }                                                                                              \
    }                                                                                                \
  }
#define AO_COMPUTE_STAGE(XS, FS, ES) { AO_FMA_S(XS, FS, ES, 0) AO_FMA_S(XS, FS, ES, 1) AO_FMA_S(XS, FS, ES, 2) AO_FMA_S(XS, FS, ES, 3) }
#define AO_MIX_STAGE(XC, FC, EC, XL, FL, EL, GI)                                                     \
  {                                                                                                  \
    AO_FMA_S(XC, FC, EC, 0) AO_LOAD1(XL, GI, 0) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 1) AO_LOAD1(XL, GI, 1) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 2) AO_LOAD1(XL, GI, 2) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 3) AO_LOAD1(XL, GI, 3) AO_LOADF(FL, EL, GI) __builtin_amdgcn_sched_barrier(0); \
  }
  // every load of a stage pinned in the steady state's order: the only way into a steady loop (see contract16_f32)
#define AO_LOAD_STAGE_ORDERED(XS, FS, ES, GI)                                                        \
  {                                                                                                  \
    AO_LOAD1(XS, GI, 0) __builtin_amdgcn_sched_barrier(0);                                           \
    AO_LOAD1(XS, GI, 1) __builtin_amdgcn_sched_barrier(0);                                           \
    AO_LOAD1(XS, GI, 2) __builtin_amdgcn_sched_barrier(0);                                           \
    AO_LOAD1(XS, GI, 3) __builtin_amdgcn_sched_barrier(0);                                           \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                              \
      FS[nt] = fp[(GI) * 64 + nt * fnt];                                                             \
      __builtin_amdgcn_sched_barrier(0);                                                             \
    }                                                                                                \
    if (EX) {                                                                                        \
      ES[0] = fe[(GI) * 8];                                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      ES[1] = fe[(GI) * 8 + 4];                                                                      \
      __builtin_amdgcn_sched_barrier(0);                                                             \
    }                                                                                                \
  }
  int64_t g = 0;
  if (RING == 3) {
    if (ng >= 5) {
      AO_LOAD_STAGE_ORDERED(x0, f0, e0, 0)
      AO_LOAD_STAGE_ORDERED(x1, f1, e1, 1)
      do {                                           // steady state: every prefetch is in range
        AO_MIX_STAGE(x0, f0, e0, x2, f2, e2, g + 2)
        AO_MIX_STAGE(x1, f1, e1, x0, f0, e0, g + 3)
        AO_MIX_STAGE(x2, f2, e2, x1, f1, e1, g + 4)
        g += 3;
      } while (g + 5 <= ng);
    } else {                                         // 0..4 full groups: no steady state
      if (ng > 0) AO_LOAD_STAGE(x0, f0, e0, 0)
      if (ng > 1) AO_LOAD_STAGE(x1, f1, e1, 1)
    }
    if (g + 3 <= ng) {                               // one drained round
      if (g + 2 < ng) AO_LOAD_STAGE(x2, f2, e2, g + 2)
      AO_COMPUTE_STAGE(x0, f0, e0)
      if (g + 3 < ng) AO_LOAD_STAGE(x0, f0, e0, g + 3)
      AO_COMPUTE_STAGE(x1, f1, e1)
      if (g + 4 < ng) AO_LOAD_STAGE(x1, f1, e1, g + 4)
      AO_COMPUTE_STAGE(x2, f2, e2)
      g += 3;
    }
    if (g < ng) AO_COMPUTE_STAGE(x0, f0, e0)
    if (g + 1 < ng) AO_COMPUTE_STAGE(x1, f1, e1)
  } else {                                           // two stages: the leftover-column form has no room for a third
    // consume stage (XC, FC, EC) and refill it in place with stage GI: an x register is free as soon as its MFMA group
    // has read it, the fragments after the last group
#define AO_MIX2_STAGE(XC, FC, EC, GI)                                                                \
  {                                                                                                  \
    AO_FMA_S(XC, FC, EC, 0) AO_LOAD1(XC, GI, 0) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 1) AO_LOAD1(XC, GI, 1) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 2) AO_LOAD1(XC, GI, 2) __builtin_amdgcn_sched_barrier(0);                   \
    AO_FMA_S(XC, FC, EC, 3) AO_LOAD1(XC, GI, 3) AO_LOADF(FC, EC, GI) __builtin_amdgcn_sched_barrier(0); \
  }
    if (ng >= 4) {
      AO_LOAD_STAGE_ORDERED(x0, f0, e0, 0)
      AO_LOAD_STAGE_ORDERED(x1, f1, e1, 1)
      do {                                           // steady state: every prefetch is in range
        AO_MIX2_STAGE(x0, f0, e0, g + 2)
        AO_MIX2_STAGE(x1, f1, e1, g + 3)
        g += 2;
      } while (g + 4 <= ng);
      AO_COMPUTE_STAGE(x0, f0, e0)                   // stages g and g + 1 are loaded; one more may follow
      if (g + 2 < ng) AO_LOAD_STAGE(x0, f0, e0, g + 2)
      AO_COMPUTE_STAGE(x1, f1, e1)
      if (g + 2 < ng) AO_COMPUTE_STAGE(x0, f0, e0)
    } else {                                         // 0..3 full groups: no steady state
      if (ng > 0) AO_LOAD_STAGE(x0, f0, e0, 0)
      if (ng > 1) {
        AO_LOAD_STAGE(x1, f1, e1, 1)
        AO_COMPUTE_STAGE(x0, f0, e0)
        if (ng > 2) AO_LOAD_STAGE(x0, f0, e0, 2)
        AO_COMPUTE_STAGE(x1, f1, e1)
        if (ng > 2) AO_COMPUTE_STAGE(x0, f0, e0)
      } else if (ng > 0) {
        AO_COMPUTE_STAGE(x0, f0, e0)
      }
    }
#undef AO_MIX2_STAGE
  }
  g = gfull > g0 ? gfull : g0;
  // ragged tail group: columns >= C are clamped (finite data) and meet zero B fragments
  if (g < g1) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int64_t c = kGroup * g + 4 * (s >> 1) + q;
      if (c >= a.C) c = a.C - 1;
      x0[s] = *reinterpret_cast<const f64x2*>(X + ((s & 1) ? row1 : row0) + c * a.ld);
    }
    {
      const f64x2* fpt = reinterpret_cast<const f64x2*>(a.frag) + g * 64 + lane;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) f0[nt] = fpt[nt * fnt];
      if (EX) {
        const f64x4* fet = reinterpret_cast<const f64x4*>(reinterpret_cast<const f64x2*>(a.frag) + (int64_t)NT * a.Cg * 64) + g * 8 + q;
        e0[0] = fet[0]; e0[1] = fet[4];
      }
    }
    AO_COMPUTE_STAGE(x0, f0, e0)
  }
#undef AO_LOAD1
#undef AO_LOADF
#undef AO_LOAD_STAGE
#undef AO_LOAD_STAGE_ORDERED
#undef AO_FMA_S
#undef AO_COMPUTE_STAGE
#undef AO_MIX_STAGE
  // epilogue: C/D map of the f64 MFMA: col = lane&15, tile row rho = (lane>>4) + 4*reg; tile (j, v) row rho is
  // unfolding row m0 + 32j + 2*rho + v.  The wave's 64 x R tile is assembled in its LDS slice and stored as whole lines.
  extern __shared__ __attribute__((aligned(16))) double t_lds64[];
  double* tl = t_lds64 + (threadIdx.x >> 6) * (kTileRows64 * a.R);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r = 16 * nt + r2;
    if (r < a.R) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
          for (int i = 0; i < 4; ++i) tl[(32 * j + 2 * (q + 4 * i) + v) * a.R + r] = acc[nt][j][v][i];
    }
  }
  if (EX) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int c = 0; c < 4; ++c) {                 // add the four k-quarters; quarter 0 stores
          double t = accE[j][v][c];
          t += __shfl_xor(t, 16);
          t += __shfl_xor(t, 32);
          accE[j][v][c] = t;
        }
    if (q == 0) {
      const int ne = a.R - 16 * NT;                  // 1..4 live extra columns
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < ne) tl[(32 * j + 2 * r2 + v) * a.R + 16 * NT + c] = accE[j][v][c];
    }
  }
  {
    const int64_t rows_here = (a.M - m0 < kTileRows64) ? a.M - m0 : kTileRows64;   // multiple of 2 (padded layout)
    const int n16 = (int)(rows_here * a.R / 2);
    f64x2* dst = reinterpret_cast<f64x2*>(reinterpret_cast<double*>(a.T) + ((int64_t)chunk * a.trows + b * a.M + m0) * a.R);
    const f64x2* src = reinterpret_cast<const f64x2*>(tl);
    for (int c = lane; c < n16; c += 64) __builtin_nontemporal_store(src[c], dst + c);
  }
}

// ---------------------------------------------------------------------------
// fp16 contraction (AOADMM_PREC_F16 storage): v_mfma_f32_16x16x32_f16 on a half pass copy
// ---------------------------------------------------------------------------
// The copy (misc.hip half_layout_copy) holds q = fp16(x * s) in 512-row blocks whose columns are grouped by 32: element
// (m, c) of a block sits at (c / 32) * 512 * 32 + (m % 512) * 32 + c % 32 halves, columns padded with zeros to a multiple
// of 32.  A row of a group is 64 bytes, so lane l's 16-byte load at row (l & 15), byte (l >> 4) * 16 is exactly the A
// operand of the MFMA: A[row l&15][k = 8(l>>4) + j], j = 0..7; a 16-row tile of a group is 1 KB contiguous, a wave's 128
// rows 8 KB.  B: lane l holds F[k = 8(l>>4) + j][col l&15].  C/D: col = lane&15, row = 4(lane>>4) + reg.
//   The factor keeps ~22 bits: column r is scaled by a power of two t_r (its largest entry lands in [2^14, 2^15)) and
//   split into hi = fp16(F t_r) and lo = fp16(F t_r - hi); both fragments are multiplied into the SAME fp32 accumulator.
//   t_r is found on the device (frag16_scales_k), nothing is read back.  The epilogue multiplies by 1/t_r and 1/s (powers
//   of two: exact) and leaves T in fp32 in the layout of contract16_f32 on a copy, so every reduction runs unchanged.
//   NT = ceil(R / 16) column tiles, no vector-pipe leftovers: a wave issues 16 NT MFMAs of 16 cycles per 8 KB it loads.
//   Register ring of three 32-column stages, the next stages' loads issued between the MFMA groups (as contract16_f32).
// frag workspace: [0, 512) double t_r[64]; [512, 768) float 1/t_r[64]; from byte 1024 on
//   frag[g][nt][f][lane] f16x8, element j = (f ? lo : hi) of F[32g + 8(lane>>4) + j][16nt + (lane&15)] * t_r
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
static constexpr int kGroup16 = 32;                 // reduction columns per MFMA and per pipeline stage
static constexpr int64_t kGroupHalves = kGroup16 * 512;   // halves of one column group of a 512-row block
static constexpr int kFragHeader16 = 1024;          // bytes in front of the fragments
static constexpr int kScaleExp16 = 15;              // largest scaled magnitude in [2^14, 2^15)

__global__ __launch_bounds__(256) void frag16_scales_k(const double* __restrict__ F, int64_t ldF, int64_t C, double* __restrict__ tsc,
                                                      float* __restrict__ tinv) {
  __shared__ double sh[256];
  const int r = blockIdx.x;
  double mx = 0.0;
  for (int64_t c = threadIdx.x; c < C; c += 256) mx = fmax(mx, fabs(F[c + ldF * r]));
  sh[threadIdx.x] = mx;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mx = sh[0];
    int e = 0;
    if (mx > 0.0 && mx <= 1.7976931348623157e308) {   // a zero (or non-finite) column keeps t_r = 1
      int ex;
      (void)frexp(mx, &ex);
      e = kScaleExp16 - ex;
      e = e > 110 ? 110 : (e < -110 ? -110 : e);       // 1 / t_r stays a normal fp32 number
    }
    tsc[r] = ldexp(1.0, e);
    tinv[r] = (float)ldexp(1.0, -e);
  }
}

__global__ void pack_frag16_f16(const double* __restrict__ F, int64_t ldF, int64_t C, int R, int NT, int64_t Cg,
                                const double* __restrict__ tsc, f16x8* __restrict__ frag) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Cg * NT * 128) return;
  const int lane = idx & 63, f = (idx >> 6) & 1;
  const int nt = (int)((idx >> 7) % NT);
  const int64_t g = (idx >> 7) / NT;
  const int r = 16 * nt + (lane & 15);
  const double t = r < R ? tsc[r] : 1.0;
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t c = kGroup16 * g + 8 * (lane >> 4) + j;
    const double v = (c < C && r < R) ? F[c + ldF * r] * t : 0.0;
    const _Float16 hi = (_Float16)v;
    o[j] = f ? (_Float16)(v - (double)hi) : hi;
  }
  frag[idx] = o;
}

struct KArgs16 {
  const _Float16* X;
  const void* frag;
  float* T;            // [nchunk][trows][R]
  int64_t ntiles, Cg, trows;
  int groups_per_chunk, R;
  float inv_s;         // 1 / s of the block
};

template <int NT>
__global__ __launch_bounds__(256, NT <= 2 ? 2 : 1) void contract16_f16(KArgs16 a) {
  const int lane = threadIdx.x & 63;
  const int64_t wt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wt >= a.ntiles) return;                        // wave-uniform
  const int chunk = blockIdx.y;
  const int64_t blk = wt >> 2;                        // four 128-row wave tiles per 512-row block
  const int m0 = (int)(wt & 3) * kTileRows;
  const int r16 = lane & 15, q = lane >> 4;
  const int64_t g0 = (int64_t)chunk * a.groups_per_chunk;
  int64_t g1 = g0 + a.groups_per_chunk;
  if (g1 > a.Cg) g1 = a.Cg;
  const int64_t ng = g1 > g0 ? g1 - g0 : 0;           // every group is whole: the copy pads its columns with zeros
  const _Float16* xp = a.X + (blk * a.Cg + g0) * kGroupHalves + (m0 + r16) * kGroup16 + 8 * q;
  const f16x8* fp = reinterpret_cast<const f16x8*>(reinterpret_cast<const char*>(a.frag) + kFragHeader16) + g0 * (NT * 128) + lane;

  f32x4 acc[NT][8];                                   // [nt][16-row tile]
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[nt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  f16x8 x0[8], x1[8], x2[8];
  f16x8 f0[NT][2], f1[NT][2], f2[NT][2];
#define AO_LOAD1(XS, GI, TL) XS[TL] = __builtin_nontemporal_load(reinterpret_cast<const f16x8*>(xp + (GI) * kGroupHalves + (TL) * (16 * kGroup16)));
#define AO_LOADF(FS, GI)                                                                             \
  {                                                                                                  \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                              \
      FS[nt][0] = fp[(GI) * (NT * 128) + nt * 128];                                                  \
      FS[nt][1] = fp[(GI) * (NT * 128) + nt * 128 + 64];                                             \
    }                                                                                                \
  }
#define AO_LOAD_STAGE(XS, FS, GI)                                                                    \
  { _Pragma("unroll") for (int tl_ = 0; tl_ < 8; ++tl_) AO_LOAD1(XS, GI, tl_) AO_LOADF(FS, GI) }
#define AO_FMA_T(XS, FS, TL)                                                                         \
  {                                                                                                  \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                              \
      acc[nt][TL] = __builtin_amdgcn_mfma_f32_16x16x32_f16(XS[TL], FS[nt][0], acc[nt][TL], 0, 0, 0); \
      acc[nt][TL] = __builtin_amdgcn_mfma_f32_16x16x32_f16(XS[TL], FS[nt][1], acc[nt][TL], 0, 0, 0); \
    }                                                                                                \
  }
#define AO_COMPUTE_STAGE(XS, FS) { _Pragma("unroll") for (int tl_ = 0; tl_ < 8; ++tl_) AO_FMA_T(XS, FS, tl_) }
  // consume stage (XC, FC) while fetching stage GI into (XL, FL): one load between MFMA groups
#define AO_MIX_STAGE(XC, FC, XL, FL, GI)                                                             \
  {                                                                                                  \
    _Pragma("unroll") for (int tl_ = 0; tl_ < 8; ++tl_) {                                            \
      AO_FMA_T(XC, FC, tl_) AO_LOAD1(XL, GI, tl_)                                                    \
      if (tl_ == 7) AO_LOADF(FL, GI)                                                                 \
      __builtin_amdgcn_sched_barrier(0);                                                             \
    }                                                                                                \
  }
  // every load of a stage pinned in the steady state's order: the only way into the steady loop (see contract16_f32)
#define AO_LOAD_STAGE_ORDERED(XS, FS, GI)                                                            \
  {                                                                                                  \
    _Pragma("unroll") for (int tl_ = 0; tl_ < 8; ++tl_) {                                            \
      AO_LOAD1(XS, GI, tl_)                                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                             \
    }                                                                                                \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                              \
      FS[nt][0] = fp[(GI) * (NT * 128) + nt * 128];                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      FS[nt][1] = fp[(GI) * (NT * 128) + nt * 128 + 64];                                             \
      __builtin_amdgcn_sched_barrier(0);                                                             \
    }                                                                                                \
  }
  int64_t g = 0;
  if (ng >= 5) {
    AO_LOAD_STAGE_ORDERED(x0, f0, 0)
    AO_LOAD_STAGE_ORDERED(x1, f1, 1)
    do {                                             // steady state: every prefetch is in range
      AO_MIX_STAGE(x0, f0, x2, f2, g + 2)
      AO_MIX_STAGE(x1, f1, x0, f0, g + 3)
      AO_MIX_STAGE(x2, f2, x1, f1, g + 4)
      g += 3;
    } while (g + 5 <= ng);
  } else {                                           // 0..4 groups: no steady state
    if (ng > 0) AO_LOAD_STAGE(x0, f0, 0)
    if (ng > 1) AO_LOAD_STAGE(x1, f1, 1)
  }
  if (g + 3 <= ng) {                                 // one drained round
    if (g + 2 < ng) AO_LOAD_STAGE(x2, f2, g + 2)
    AO_COMPUTE_STAGE(x0, f0)
    if (g + 3 < ng) AO_LOAD_STAGE(x0, f0, g + 3)
    AO_COMPUTE_STAGE(x1, f1)
    if (g + 4 < ng) AO_LOAD_STAGE(x1, f1, g + 4)
    AO_COMPUTE_STAGE(x2, f2)
    g += 3;
  }
  if (g < ng) AO_COMPUTE_STAGE(x0, f0)
  if (g + 1 < ng) AO_COMPUTE_STAGE(x1, f1)
#undef AO_LOAD1
#undef AO_LOADF
#undef AO_LOAD_STAGE
#undef AO_LOAD_STAGE_ORDERED
#undef AO_FMA_T
#undef AO_COMPUTE_STAGE
#undef AO_MIX_STAGE
  // epilogue: tile t row j = 4q + reg is row m0 + 16t + j of the block; descaled by 1/t_r and 1/s (exact), assembled in
  // the wave's LDS slice and stored as whole lines (see contract16_f32)
  extern __shared__ __attribute__((aligned(16))) float t_lds[];
  float* tl = t_lds + (threadIdx.x >> 6) * (kTileRows * a.R);
  const float* tinv = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.frag) + 512);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r = 16 * nt + r16;
    if (r < a.R) {
      const float ti = tinv[r];
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) tl[(16 * t + 4 * q + i) * a.R + r] = acc[nt][t][i] * ti * a.inv_s;
    }
  }
  // a wave's LDS operations complete in order: its own writes are visible to its reads without a barrier
  {
    const int n16 = kTileRows * a.R / 4;
    f32x4* dst = reinterpret_cast<f32x4*>(a.T + ((int64_t)chunk * a.trows + blk * 512 + m0) * a.R);
    const f32x4* src = reinterpret_cast<const f32x4*>(tl);
    for (int c = lane; c < n16; c += 64) __builtin_nontemporal_store(src[c], dst + c);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int nt_of(int R, int prec) {
  const int w = prec == AOADMM_PREC_F32 ? 32 : 16;   // (fp16: 16-column tiles)
  return (R + w - 1) / w;
}
static int tile_rows(int prec) { return prec == AOADMM_PREC_F64 ? kTileRows64 : kTileRows; }

size_t ContractPlan::frag_bytes(int prec) const {
  if (prec == AOADMM_PREC_F16)                        // header + hi and lo fragments of every 32-column group
    return (size_t)kFragHeader16 + (size_t)cdiv(C, kGroup16) * nt_of(R, prec) * 2048;
  const int64_t Cg = cdiv(C, kGroup);
  // f32: the 32-column layout needs nt32*1024 B per group, the 16-column layout nt16*512 + 128 (extras)
  return (size_t)(nt_of(R, prec) * 1024 + 1152) * Cg + 8192;
}

ContractPlan make_plan(int64_t nbatch, int64_t batch_stride, int64_t M, int64_t ld, int64_t C, int R,
                       int prec) {
  ContractPlan p;
  const bool half = prec == AOADMM_PREC_F16;
  p.tprec = half ? AOADMM_PREC_F32 : prec;            // a half operand accumulates in fp32 inside the MFMA: T is fp32
  p.nbatch = nbatch; p.batch_stride = batch_stride; p.M = M; p.ld = ld; p.C = C; p.R = R;
  const int gcols = half ? kGroup16 : kGroup;         // columns per group
  const int64_t Cg = cdiv(C, gcols);
  const int64_t ntiles = nbatch * cdiv(M, tile_rows(prec));
  int64_t nchunk = 1;
  // f32 (and f16) accumulate in fp32 inside the MFMA: keep one accumulation run <= 2048 terms;
  // partial sums of different chunks are added in fp64 by the reduce kernels.
  if (prec != AOADMM_PREC_F64) nchunk = cdiv(Cg, 2048 / gcols);
  // few row tiles (short mode): split the reduction to fill the 256 CUs
  if (ntiles < 2048) {
    int64_t want = cdiv(2048, ntiles);
    const int64_t gmin = 128 / gcols;
    int64_t maxc = Cg / gmin > 0 ? Cg / gmin : 1;   // keep >= 128 columns per chunk
    if (want > maxc) want = maxc;
    if (want > nchunk) nchunk = want;
  }
  if (nchunk > 65535) nchunk = 65535;
  p.nchunk = (int)nchunk;
  return p;
}

ContractPlan make_lead_plan(int64_t M, int64_t ld, int64_t C, int R) {
  ContractPlan p;
  p.tprec = AOADMM_PREC_F32;
  p.nbatch = 1; p.batch_stride = 0; p.M = M; p.ld = ld; p.C = C; p.R = R;
  p.lead = true;
  const int64_t nch = cdiv(C, kLeadKC);
  p.nchunk = (int)cdiv(nch, 2048 / kLeadKC);        // <= 2048 fp32-accumulated terms per slice
  return p;
}

static void launch_contract_lead(const void* X, const ContractPlan& pl, const double* F, int64_t ldF, void* frag_ws,
                                 void* T, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  const int64_t Cg = cdiv(pl.C, kGroup);
  AO_REQUIRE(pl.ld % 4 == 0 && pl.ld >= 4, "f32 layout must be padded to 4");
  LArgs a;
  a.X = (const float*)X; a.frag = (const float*)frag_ws; a.T = (float*)T;
  a.M = pl.M; a.ld = pl.ld; a.C = pl.C; a.Cg = Cg; a.R = pl.R;
  a.chunks_per_slice = (int)cdiv(cdiv(pl.C, kLeadKC), pl.nchunk);
  const int64_t nblk = cdiv(pl.M, kLeadRows);
  AO_REQUIRE(nblk < (int64_t)2147483647, "tensor too large for one launch");
  dim3 grid((unsigned)nblk, (unsigned)pl.nchunk);
  const size_t sh = (size_t)2 * kLeadRows * kLeadStride * sizeof(float);
  const int nt16 = (pl.R + 15) / 16;
  const int64_t Cg16 = cdiv(pl.C, 16) + 1;           // + one all-zero group: the ragged last chunk multiplies by it
  const int64_t total = (int64_t)nt16 * Cg16 * 256;
  pack_frag_lead16_f32<<<(unsigned)cdiv(total, 256), 256, 0, s>>>(F, ldF, pl.C, pl.R, nt16, Cg16, (float*)frag_ws);
  AO_KERNEL_CHECK();
#define AO_SET(K) ensure_dynamic_lds(reinterpret_cast<const void*>(K), (int)sh);
  if (nt16 == 1) AO_SET(contract_lead16_f32<1>)
  else if (nt16 == 2) AO_SET(contract_lead16_f32<2>)
  else if (nt16 == 3) AO_SET(contract_lead16_f32<3>)
  else if (nt16 == 4) AO_SET(contract_lead16_f32<4>)
#undef AO_SET
  if (ev0) AO_HIP(hipEventRecord(ev0, s));
  if (nt16 == 1) contract_lead16_f32<1><<<grid, 256, sh, s>>>(a);
  else if (nt16 == 2) contract_lead16_f32<2><<<grid, 256, sh, s>>>(a);
  else if (nt16 == 3) contract_lead16_f32<3><<<grid, 256, sh, s>>>(a);
  else if (nt16 == 4) contract_lead16_f32<4><<<grid, 256, sh, s>>>(a);
  else throw Error(AOADMM_ERR_UNSUPPORTED, "rank > 64 not supported");
  if (ev1) AO_HIP(hipEventRecord(ev1, s));
  AO_KERNEL_CHECK();
}

// pass on a half pass copy: scales, fragments, contract16_f16
static void launch_contract_half(const void* X, const ContractPlan& pl, const double* F, int64_t ldF, void* frag_ws,
                                 void* T, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  AO_REQUIRE(pl.on_copy && !pl.lead && pl.M == 512 && pl.ld == 512 && pl.tprec == AOADMM_PREC_F32,
             "internal: a half operand is streamed from its pass copies only");
  const int64_t Cg = cdiv(pl.C, kGroup16);
  AO_REQUIRE(pl.batch_stride == 512 * kGroup16 * Cg && pl.nbatch > 0 && pl.C > 0, "internal: half pass copy and plan disagree");
  const int NT = nt_of(pl.R, AOADMM_PREC_F16);
  char* ws = reinterpret_cast<char*>(frag_ws);
  double* tsc = reinterpret_cast<double*>(ws);
  float* tinv = reinterpret_cast<float*>(ws + 512);
  frag16_scales_k<<<(unsigned)pl.R, 256, 0, s>>>(F, ldF, pl.C, tsc, tinv);
  AO_KERNEL_CHECK();
  pack_frag16_f16<<<(unsigned)cdiv(Cg * NT * 128, 256), 256, 0, s>>>(F, ldF, pl.C, pl.R, NT, Cg, tsc,
                                                                    reinterpret_cast<f16x8*>(ws + kFragHeader16));
  AO_KERNEL_CHECK();
  KArgs16 a;
  a.X = reinterpret_cast<const _Float16*>(X); a.frag = frag_ws; a.T = reinterpret_cast<float*>(T);
  a.ntiles = pl.nbatch * 4; a.Cg = Cg; a.trows = pl.trows();
  a.groups_per_chunk = (int)cdiv(Cg, pl.nchunk);
  a.R = pl.R;
  a.inv_s = (float)(1.0 / pl.xscale);                 // s is a normal fp32 power of two: exact
  AO_REQUIRE(pl.nbatch < (int64_t)2147483647, "tensor too large for one launch");
  const dim3 grid((unsigned)pl.nbatch, (unsigned)pl.nchunk);
  const size_t tsh = (size_t)4 * kTileRows * pl.R * sizeof(float);   // T tile of each of the four waves
#define AO_GO(K) { if (tsh > 65536) ensure_dynamic_lds(reinterpret_cast<const void*>(K), (int)tsh); if (ev0) AO_HIP(hipEventRecord(ev0, s)); K<<<grid, 256, tsh, s>>>(a); }
  if (NT == 1) AO_GO(contract16_f16<1>)
  else if (NT == 2) AO_GO(contract16_f16<2>)
  else if (NT == 3) AO_GO(contract16_f16<3>)
  else if (NT == 4) AO_GO(contract16_f16<4>)
  else throw Error(AOADMM_ERR_UNSUPPORTED, "rank > 64 not supported");
#undef AO_GO
  if (ev1) AO_HIP(hipEventRecord(ev1, s));
  AO_KERNEL_CHECK();
}

void launch_contract(const void* X, int prec, const ContractPlan& pl, const double* F, int64_t ldF,
                     void* frag_ws, void* T, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  AO_REQUIRE(pl.R >= 1 && pl.R <= kMaxRank, "rank %d outside [1,%d]", pl.R, kMaxRank);
  if (prec == AOADMM_PREC_F16) {                      // half operand, fp32 T
    launch_contract_half(X, pl, F, ldF, frag_ws, T, s, ev0, ev1);
    return;
  }
  AO_REQUIRE(prec == AOADMM_PREC_F32 || prec == AOADMM_PREC_F64, "bad precision id %d", prec);
  AO_REQUIRE(pl.tprec == prec, "contraction plan and tensor precision disagree");
  if (pl.lead) {
    AO_REQUIRE(prec == AOADMM_PREC_F32, "leading-mode contraction exists for fp32 tensors only");
    launch_contract_lead(X, pl, F, ldF, frag_ws, T, s, ev0, ev1);
    return;
  }
  const int64_t Cg = cdiv(pl.C, kGroup);
  KArgs a;
  a.X = X; a.frag = frag_ws; a.T = T;
  a.tiles_per_batch = cdiv(pl.M, tile_rows(prec));
  a.ntiles = pl.nbatch * a.tiles_per_batch;
  a.batch_stride = pl.batch_stride; a.M = pl.M; a.ld = pl.ld; a.C = pl.C; a.Cg = Cg;
  a.trows = pl.trows();
  a.groups_per_chunk = (int)cdiv(Cg, pl.nchunk);
  a.R = pl.R;
  AO_REQUIRE(a.ntiles > 0 && pl.C > 0, "empty contraction");
  dim3 grid((unsigned)cdiv(a.ntiles, 4), (unsigned)pl.nchunk);
  AO_REQUIRE(cdiv(a.ntiles, 4) < (int64_t)2147483647, "tensor too large for one launch");
  if (prec == AOADMM_PREC_F32) {
    AO_REQUIRE(pl.ld % 4 == 0 && pl.M % 4 == 0 && pl.batch_stride % 4 == 0, "f32 layout must be padded to 4");
    // 16-column tiles; 1..4 leftover columns go to the vector pipe
    const int rem = pl.R % 16;
    const bool ex = pl.R > 16 && rem >= 1 && rem <= 4;
    const int nt16 = ex ? pl.R / 16 : (pl.R + 15) / 16;
    const int64_t total = (int64_t)nt16 * Cg * 128 + (ex ? Cg * 32 : 0);
    pack_frag16_f32<<<(unsigned)cdiv(total, 256), 256, 0, s>>>(F, ldF, pl.C, pl.R, nt16, ex ? 1 : 0, Cg, (float*)frag_ws);
    AO_KERNEL_CHECK();
    size_t tsh = (size_t)4 * kTileRows * pl.R * sizeof(float);   // T tile of each of the four waves
    // two-level accumulation for R <= 20 (see the kernel)
    a.flush_every = kFlushEvery;
    if (nt16 == 1) tsh = (size_t)4 * 16384;
#define AO_GO(K) { if (tsh > 65536) ensure_dynamic_lds(reinterpret_cast<const void*>(K), (int)tsh); if (ev0) AO_HIP(hipEventRecord(ev0, s)); K<<<grid, 256, tsh, s>>>(a); }
    if (nt16 == 1 && !ex) AO_GO((contract16_f32<1, false, true>))
    else if (nt16 == 1) AO_GO((contract16_f32<1, true, true>))
    else if (nt16 == 2 && !ex) AO_GO((contract16_f32<2, false>))
    else if (nt16 == 2) AO_GO((contract16_f32<2, true>))
    else if (nt16 == 3 && !ex) AO_GO((contract16_f32<3, false>))
    else if (nt16 == 3) AO_GO((contract16_f32<3, true>))
    else if (nt16 == 4) AO_GO((contract16_f32<4, false>))
    else throw Error(AOADMM_ERR_UNSUPPORTED, "rank > 64 not supported");
#undef AO_GO
  } else {
    AO_REQUIRE(pl.ld % 2 == 0 && pl.M % 2 == 0 && pl.batch_stride % 2 == 0, "f64 layout must be padded to 2");
    // 16-column tiles; 1..4 leftover columns go to the vector pipe
    const int rem = pl.R % 16;
    const bool ex = pl.R > 16 && rem >= 1 && rem <= 4;
    const int nt16 = ex ? pl.R / 16 : (pl.R + 15) / 16;
    const int64_t total = (int64_t)nt16 * Cg * 128 + (ex ? Cg * 32 : 0);
    pack_frag_f64<<<(unsigned)cdiv(total, 256), 256, 0, s>>>(F, ldF, pl.C, pl.R, nt16, ex ? 1 : 0, Cg, (double*)frag_ws);
    AO_KERNEL_CHECK();
    const size_t tsh = (size_t)4 * kTileRows64 * pl.R * sizeof(double);   // T tile of each of the four waves
#define AO_GO(K) { if (tsh > 65536) ensure_dynamic_lds(reinterpret_cast<const void*>(K), (int)tsh); if (ev0) AO_HIP(hipEventRecord(ev0, s)); K<<<grid, 256, tsh, s>>>(a); }
    if (nt16 == 1 && !ex) AO_GO((contract_f64<1, false>))
    else if (nt16 == 1) AO_GO((contract_f64<1, true>))
    else if (nt16 == 2 && !ex) AO_GO((contract_f64<2, false>))
    else if (nt16 == 2) AO_GO((contract_f64<2, true>))
    else if (nt16 == 3 && !ex) AO_GO((contract_f64<3, false>))
    else if (nt16 == 3) AO_GO((contract_f64<3, true>))
    else if (nt16 == 4) AO_GO((contract_f64<4, false>))
    else throw Error(AOADMM_ERR_UNSUPPORTED, "rank > 64 not supported");
#undef AO_GO
  }
  if (ev1) AO_HIP(hipEventRecord(ev1, s));
  AO_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------
// reductions over T (fp64 accumulation, deterministic summation order)
// ---------------------------------------------------------------------------
// T is read with the factor in the SAME row-major [row][r] order (the factor is transposed into a small
// scratch first): both operands of every product come from one flat, fully coalesced index, instead of
// 20-64 scattered cache lines per wave load of the column-major factor.  Each thread keeps four
// independent accumulators, i.e. four loads of each stream in flight.
__global__ void factor_rowmajor_k(const double* __restrict__ F, int64_t ldF, int64_t rows, int R,
                                  double* __restrict__ Ft) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;    // over rows * R, row fastest
  if (idx >= rows * R) return;
  const int r = (int)(idx / rows);
  const int64_t a = idx - (int64_t)r * rows;
  Ft[a * R + r] = F[a + ldF * r];
}
static void factor_rowmajor(const double* F, int64_t ldF, int64_t rows, int R, double* Ft, hipStream_t s) {
  factor_rowmajor_k<<<(unsigned)cdiv(rows * R, 256), 256, 0, s>>>(F, ldF, rows, R, Ft);
  AO_KERNEL_CHECK();
}

// VEC consecutive r per thread (16-byte loads of T when the rank allows it: VEC = 4 for fp32, 2 for fp64)
template <typename TT, int VEC> struct TVec;
template <> struct TVec<float, 4> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct TVec<float, 1> { typedef float type; };
template <> struct TVec<double, 2> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct TVec<double, 1> { typedef double type; };
template <typename TT, int VEC>
__device__ __forceinline__ void fma_vec(double (&acc)[VEC], const TT* __restrict__ tp, const double* __restrict__ fp) {
  typedef typename TVec<TT, VEC>::type V;
  const V tv = __builtin_nontemporal_load(reinterpret_cast<const V*>(tp));
  if constexpr (VEC == 1) {
    acc[0] += (double)tv * fp[0];
  } else {
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] += (double)tv[v] * fp[v];
  }
}

// The same product with the loads split from the arithmetic: a loop body issues ALL its loads (tensor-side and
// factor-side) before the first FMA.  Written as fma_vec calls back to back, the compiler re-used one register set
// and put s_waitcnt vmcnt(0) between the groups, i.e. one 16-byte tensor load in flight per thread (4 TB/s).
template <typename TT, int VEC>
struct RVec {
  typename TVec<TT, VEC>::type t;
  double f[VEC];
  __device__ __forceinline__ void load(const TT* __restrict__ tp, const double* __restrict__ fp) {
    t = __builtin_nontemporal_load(reinterpret_cast<const typename TVec<TT, VEC>::type*>(tp));   // T is read once per pass
#pragma unroll
    for (int v = 0; v < VEC; ++v) f[v] = fp[v];
  }
  __device__ __forceinline__ void fma(double (&acc)[VEC]) const {
    if constexpr (VEC == 1) {
      acc[0] += (double)t * f[0];
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += (double)t[v] * f[v];
    }
  }
};

// one block per b; the A x R slab of T and the row-major factor are walked with the same flat index.
// blockDim * VEC is a multiple of R, so a thread's r's are fixed while its a advances.
template <typename TT, int VEC>
__global__ void reduce_inner_k(const TT* __restrict__ T, int nchunk, int64_t trows, int64_t A, int64_t Apad, int R,
                               const double* __restrict__ FaT, double scale, double* __restrict__ out,
                               int64_t ldOut, int rowmajor, int has_sys, SysBuild sys) {
  extern __shared__ double sh[];                      // blockDim * VEC
  // the extra workgroup (small_dev.h) is the FIRST one: dispatched first, its 10 us of dependent latency run beside the
  // reduction (as the last workgroup it started when the others were nearly through and lengthened the kernel by 6-12 us)
  if (has_sys && blockIdx.x == 0) { sys_build_rider(sys); return; }
  const int64_t b = (int64_t)blockIdx.x - has_sys;
  const int t = threadIdx.x;
  const int64_t n = A * R, step = (int64_t)blockDim.x * VEC;
  double s0[VEC], s1[VEC], s2[VEC], s3[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) { s0[v] = 0; s1[v] = 0; s2[v] = 0; s3[v] = 0; }
  for (int ch = 0; ch < nchunk; ++ch) {
    const TT* Tb = T + ((int64_t)ch * trows + Apad * b) * R;
    int64_t e = (int64_t)t * VEC;
    for (; e + 3 * step < n; e += 4 * step) {
      RVec<TT, VEC> q0, q1, q2, q3;
      q0.load(Tb + e, FaT + e);
      q1.load(Tb + e + step, FaT + e + step);
      q2.load(Tb + e + 2 * step, FaT + e + 2 * step);
      q3.load(Tb + e + 3 * step, FaT + e + 3 * step);
      __builtin_amdgcn_sched_barrier(0);               // keep the eight loads ahead of the arithmetic
      q0.fma(s0); q1.fma(s1); q2.fma(s2); q3.fma(s3);
    }
    for (; e < n; e += step) fma_vec<TT, VEC>(s0, Tb + e, FaT + e);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) sh[t * VEC + v] = (s0[v] + s1[v]) + (s2[v] + s3[v]);
  __syncthreads();
  if (t < R) {                                        // flat slot q holds r = q % R
    const int nA = blockDim.x * VEC / R;
    double tot = 0.0;
    for (int i = 0; i < nA; ++i) tot += sh[i * R + t];
    if (rowmajor) out[b * R + t] = scale * tot;       // T layout [b][r] for a further fold (N-way tensors)
    else out[b + ldOut * t] = scale * tot;
  }
}

// Two slabs (b, b+1) per block: the factor row is loaded once and used for both, which halves the L2 -> CU traffic
// of the factor side (fp64 factor entries are twice the bytes of the fp32 T entries they multiply).
template <typename TT, int VEC>
__global__ void reduce_inner2_k(const TT* __restrict__ T, int nchunk, int64_t trows, int64_t A, int64_t Apad, int64_t B,
                                int R, const double* __restrict__ FaT, double scale, double* __restrict__ out,
                                int64_t ldOut, int rowmajor, int has_sys, SysBuild sys) {
  extern __shared__ double sh[];                      // 2 * blockDim * VEC
  if (has_sys && blockIdx.x == 0) { sys_build_rider(sys); return; }   // the extra workgroup, dispatched first (see reduce_inner_k)
  const int64_t b0 = 2 * ((int64_t)blockIdx.x - has_sys);
  const bool two = b0 + 1 < B;
  const int64_t b1 = two ? b0 + 1 : b0;
  const int t = threadIdx.x;
  const int64_t n = A * R, step = (int64_t)blockDim.x * VEC;
  double a0[VEC], a1[VEC], c0[VEC], c1[VEC];           // slab b0: a0 + a1, slab b1: c0 + c1
#pragma unroll
  for (int v = 0; v < VEC; ++v) { a0[v] = 0; a1[v] = 0; c0[v] = 0; c1[v] = 0; }
  for (int ch = 0; ch < nchunk; ++ch) {
    const TT* Ta = T + ((int64_t)ch * trows + Apad * b0) * R;
    const TT* Tc = T + ((int64_t)ch * trows + Apad * b1) * R;
    int64_t e = (int64_t)t * VEC;
    for (; e + step < n; e += 2 * step) {
      RVec<TT, VEC> q0, q1, p0, p1;
      q0.load(Ta + e, FaT + e);
      q1.load(Ta + e + step, FaT + e + step);
      p0.t = __builtin_nontemporal_load(reinterpret_cast<const typename TVec<TT, VEC>::type*>(Tc + e));
      p1.t = __builtin_nontemporal_load(reinterpret_cast<const typename TVec<TT, VEC>::type*>(Tc + e + step));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int v = 0; v < VEC; ++v) { p0.f[v] = q0.f[v]; p1.f[v] = q1.f[v]; }
      q0.fma(a0); q1.fma(a1); p0.fma(c0); p1.fma(c1);
    }
    for (; e < n; e += step) {
      RVec<TT, VEC> q0, p0;
      q0.load(Ta + e, FaT + e);
      p0.t = __builtin_nontemporal_load(reinterpret_cast<const typename TVec<TT, VEC>::type*>(Tc + e));
#pragma unroll
      for (int v = 0; v < VEC; ++v) p0.f[v] = q0.f[v];
      q0.fma(a0); p0.fma(c0);
    }
  }
  const int nt = blockDim.x * VEC;
#pragma unroll
  for (int v = 0; v < VEC; ++v) { sh[t * VEC + v] = a0[v] + a1[v]; sh[nt + t * VEC + v] = c0[v] + c1[v]; }
  __syncthreads();
  if (t < 2 * R) {                                    // flat slot q holds r = q % R
    const int which = t / R, r = t % R;
    if (which == 0 || two) {
      const int nA = nt / R;
      double tot = 0.0;
      for (int i = 0; i < nA; ++i) tot += sh[which * nt + i * R + r];
      const int64_t b = which ? b1 : b0;
      if (rowmajor) out[b * R + r] = scale * tot;
      else out[b + ldOut * r] = scale * tot;
    }
  }
}

size_t reduce_factor_scratch_bytes(int64_t rows, int R) { return (size_t)rows * R * sizeof(double); }

template <typename TT, int VEC>
static void launch_inner_t(const void* T, int nchunk, int64_t trows, int64_t A, int64_t Apad, int64_t B, int R,
                           const double* FaT, double scale, double* out, int64_t ldOut, hipStream_t s, int rowmajor,
                           const SysBuild* sys) {
  const int hs = sys ? 1 : 0;
  const SysBuild sb = sys ? *sys : SysBuild();
  const int rq = R / VEC;                             // threads per row of T
  int threads = 256 / rq * rq;
  if (threads < rq) threads = rq;
  if (threads * VEC < R) threads = (R + VEC - 1) / VEC;
  if (B >= 1024 && 2 * R <= threads) {                // enough slabs to fill the chip with half as many blocks
    reduce_inner2_k<TT, VEC><<<(unsigned)((B + 1) / 2 + hs), threads, (size_t)2 * threads * VEC * sizeof(double), s>>>(
        (const TT*)T, nchunk, trows, A, Apad, B, R, FaT, scale, out, ldOut, rowmajor, hs, sb);
    return;
  }
  reduce_inner_k<TT, VEC><<<(unsigned)(B + hs), threads, (size_t)threads * VEC * sizeof(double), s>>>(
      (const TT*)T, nchunk, trows, A, Apad, R, FaT, scale, out, ldOut, rowmajor, hs, sb);
}

static bool sys_can_ride(const SysBuild* sys, int threads_min = 64) {
  return sys != nullptr && sys->R >= 1 && sys->R <= kSysRiderMaxR && threads_min >= 64;
}

bool launch_reduce_inner(const void* T, int tprec, int nchunk, int64_t trows, int64_t A, int64_t Apad,
                         int64_t B, int R, const double* Fa, int64_t ldFa, double scale,
                         double* out, int64_t ldOut, double* ft_scratch, hipStream_t s, const double* FaT,
                         int rowmajor_out, const SysBuild* sys) {
  AO_REQUIRE((int64_t)B < 2147483647ll, "reduce_inner: too many output rows for one launch");
  // the rider needs one full wave in the extra workgroup: blocks here have >= R / VEC threads, 240-256 in practice
  {
    const int vec = tprec == AOADMM_PREC_F32 ? (R % 4 == 0 ? 4 : 1) : (R % 2 == 0 ? 2 : 1);
    const int rq = R / vec;
    int threads = 256 / rq * rq;
    if (threads < rq) threads = rq;
    if (threads * vec < R) threads = (R + vec - 1) / vec;
    if (!sys_can_ride(sys, threads)) sys = nullptr;
  }
  if (FaT) ft_scratch = const_cast<double*>(FaT);    // row-major copy already maintained by the caller
  else factor_rowmajor(Fa, ldFa, A, R, ft_scratch, s);
  // 16-byte loads need every slab (Apad*R elements) and every chunk (trows*R) to start 16-byte aligned
  if (tprec == AOADMM_PREC_F32) {
    if (R % 4 == 0) launch_inner_t<float, 4>(T, nchunk, trows, A, Apad, B, R, ft_scratch, scale, out, ldOut, s, rowmajor_out, sys);
    else launch_inner_t<float, 1>(T, nchunk, trows, A, Apad, B, R, ft_scratch, scale, out, ldOut, s, rowmajor_out, sys);
  } else {
    if (R % 2 == 0) launch_inner_t<double, 2>(T, nchunk, trows, A, Apad, B, R, ft_scratch, scale, out, ldOut, s, rowmajor_out, sys);
    else launch_inner_t<double, 1>(T, nchunk, trows, A, Apad, B, R, ft_scratch, scale, out, ldOut, s, rowmajor_out, sys);
  }
  AO_KERNEL_CHECK();
  return sys != nullptr;
}

// out(a, r) = sum_b T[a + Apad*b][r] * Fb(b, r): block = TA consecutive rows a x (R/VEC) r-groups, grid.y
// slices of b; partial sums per slice are added in slice order by reduce_outer_fin.
static void outer_geometry(int64_t A, int64_t B, int R, int vec, int& TA, int64_t& nblkA, int& SB) {
  const int rq = (R + vec - 1) / vec;
  TA = 256 / rq;
  if (TA < 1) TA = 1;
  nblkA = cdiv(A, TA);
  int64_t sb = cdiv(2048, nblkA);
  if (sb > 64) sb = 64;
  if (sb > B) sb = B;
  if (sb < 1) sb = 1;
  SB = (int)sb;
}
static int outer_vec(int tprec, int R) {
  if (tprec == AOADMM_PREC_F32) return R % 4 == 0 ? 4 : 1;
  return R % 2 == 0 ? 2 : 1;
}

size_t reduce_outer_scratch_bytes(int64_t A, int64_t B, int R) {
  size_t worst = 0;
  for (int vec : {1, 2, 4}) {
    int TA, SB; int64_t nb;
    outer_geometry(A, B, R, vec, TA, nb, SB);
    worst = std::max(worst, (size_t)SB * A * R * sizeof(double));
  }
  return worst;
}

template <typename TT, int VEC>
__global__ void reduce_outer_k(const TT* __restrict__ T, int nchunk, int64_t trows, int64_t A,
                               int64_t Apad, int64_t B, int R, int TA, const double* __restrict__ FbT,
                               double* __restrict__ part, int has_sys, SysBuild sys) {
  if (has_sys && blockIdx.x == 0) {                   // the extra column of workgroups (dispatched first): one of them builds the system
    if (blockIdx.y == 0) sys_build_rider(sys);
    return;
  }
  const int t = threadIdx.x;
  const int rq = R / VEC;
  const int al = t / rq, r = (t - al * rq) * VEC;
  const int64_t a = ((int64_t)blockIdx.x - has_sys) * TA + al;
  const int SB = gridDim.y, sb = blockIdx.y;
  const int64_t bper = (B + SB - 1) / SB;
  const int64_t b0 = sb * bper;
  int64_t b1 = b0 + bper;
  if (b1 > B) b1 = B;
  if (al >= TA || a >= A) return;
  const int64_t bs = Apad * R;                       // T stride between consecutive b
  double s0[VEC], s1[VEC], s2[VEC], s3[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) { s0[v] = 0; s1[v] = 0; s2[v] = 0; s3[v] = 0; }
  for (int ch = 0; ch < nchunk; ++ch) {
    const TT* Tc = T + (int64_t)ch * trows * R + a * R + r;
    const double* Fr = FbT + r;
    int64_t b = b0;
    for (; b + 3 < b1; b += 4) {
      RVec<TT, VEC> q0, q1, q2, q3;
      q0.load(Tc + bs * b, Fr + b * R);
      q1.load(Tc + bs * (b + 1), Fr + (b + 1) * R);
      q2.load(Tc + bs * (b + 2), Fr + (b + 2) * R);
      q3.load(Tc + bs * (b + 3), Fr + (b + 3) * R);
      __builtin_amdgcn_sched_barrier(0);
      q0.fma(s0); q1.fma(s1); q2.fma(s2); q3.fma(s3);
    }
    for (; b < b1; ++b) fma_vec<TT, VEC>(s0, Tc + bs * b, Fr + b * R);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) part[((int64_t)sb * A + a) * R + r + v] = (s0[v] + s1[v]) + (s2[v] + s3[v]);
}

__global__ void reduce_outer_fin(const double* __restrict__ part, int SB, int64_t A, int R, double scale,
                                 double* __restrict__ out, int64_t ldOut, int rowmajor) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= A * R) return;
  const int64_t a = idx / R;
  const int r = (int)(idx - a * R);
  // eight slices per step, their loads issued together: with two per step the up to 64 slices were 32 dependent L2
  // round trips (11 us for 40,000 outputs); the sum keeps the even/odd pairing of the two-accumulator form
  double t0 = 0.0, t1 = 0.0;
  int s = 0;
  const int64_t ar = A * R;
  for (; s + 7 < SB; s += 8) {
    const double v0 = part[(int64_t)s * ar + idx], v1 = part[(int64_t)(s + 1) * ar + idx];
    const double v2 = part[(int64_t)(s + 2) * ar + idx], v3 = part[(int64_t)(s + 3) * ar + idx];
    const double v4 = part[(int64_t)(s + 4) * ar + idx], v5 = part[(int64_t)(s + 5) * ar + idx];
    const double v6 = part[(int64_t)(s + 6) * ar + idx], v7 = part[(int64_t)(s + 7) * ar + idx];
    t0 += v0; t1 += v1; t0 += v2; t1 += v3; t0 += v4; t1 += v5; t0 += v6; t1 += v7;
  }
  for (; s + 1 < SB; s += 2) {
    t0 += part[(int64_t)s * ar + idx];
    t1 += part[(int64_t)(s + 1) * ar + idx];
  }
  if (s < SB) t0 += part[(int64_t)s * ar + idx];
  if (rowmajor) out[idx] = scale * (t0 + t1);         // T layout [a][r] for a further fold (N-way tensors)
  else out[a + ldOut * r] = scale * (t0 + t1);
}

template <typename TT, int VEC>
static void launch_outer_t(const void* T, int nchunk, int64_t trows, int64_t A, int64_t Apad, int64_t B, int R,
                           const double* FbT, double* scratch, int& SB, hipStream_t s, const SysBuild* sys) {
  int TA; int64_t nb;
  outer_geometry(A, B, R, VEC, TA, nb, SB);
  int threads = TA * (R / VEC);
  threads = (threads + 63) / 64 * 64;
  const int hs = sys ? 1 : 0;
  reduce_outer_k<TT, VEC><<<dim3((unsigned)(nb + hs), (unsigned)SB), threads, 0, s>>>((const TT*)T, nchunk, trows, A, Apad, B,
                                                                                    R, TA, FbT, scratch, hs, sys ? *sys : SysBuild());
}

bool launch_reduce_outer(const void* T, int tprec, int nchunk, int64_t trows, int64_t A, int64_t Apad,
                         int64_t B, int R, const double* Fb, int64_t ldFb, double scale,
                         double* out, int64_t ldOut, double* scratch, double* ft_scratch, hipStream_t s,
                         const double* FbT, int rowmajor_out, const SysBuild* sys) {
  if (!sys_can_ride(sys)) sys = nullptr;
  if (FbT) ft_scratch = const_cast<double*>(FbT);
  else factor_rowmajor(Fb, ldFb, B, R, ft_scratch, s);
  int SB = 1;
  const int vec = outer_vec(tprec, R);
  if (tprec == AOADMM_PREC_F32) {
    if (vec == 4) launch_outer_t<float, 4>(T, nchunk, trows, A, Apad, B, R, ft_scratch, scratch, SB, s, sys);
    else launch_outer_t<float, 1>(T, nchunk, trows, A, Apad, B, R, ft_scratch, scratch, SB, s, sys);
  } else {
    if (vec == 2) launch_outer_t<double, 2>(T, nchunk, trows, A, Apad, B, R, ft_scratch, scratch, SB, s, sys);
    else launch_outer_t<double, 1>(T, nchunk, trows, A, Apad, B, R, ft_scratch, scratch, SB, s, sys);
  }
  AO_KERNEL_CHECK();
  reduce_outer_fin<<<(unsigned)cdiv(A * R, 256), 256, 0, s>>>(scratch, SB, A, R, scale, out, ldOut, rowmajor_out);
  AO_KERNEL_CHECK();
  return sys != nullptr;
}

// ---------------------------------------------------------------------------
// Tiny blocks (the example scripts' 50 x 30 x 40 tensors and 50 x 70 matrices): a whole MTTKRP (:97) in ONE launch.
// The matrix-core path needs three (factor fragments, partial contraction, reduction over T), each of them 3-5 us of
// latency for microseconds of work.  One workgroup per output row n: the threads walk the (a, b) pairs of the two
// other modes, the factors of those modes sit in LDS, R accumulators per thread, one workgroup reduction at the end
// (fixed order).  Accumulation in fp64 whatever the tensor's precision.
// ---------------------------------------------------------------------------
template <typename TT, int RMAX>
__global__ __launch_bounds__(256) void small_mttkrp_k(SmallMttkrp a, int has_sys, SysBuild sys) {
  extern __shared__ double sf[];                     // Fa [Na][R] | Fb [Nb][R] | red [4][RMAX]
  if (has_sys && blockIdx.x == 0) { sys_build_rider(sys); return; }   // the mode's R x R system rides along (small_dev.h)
  const int row = (int)blockIdx.x - has_sys;
  const int R = a.R, Na = a.Na, Nb = a.Nb;
  double* fa = sf;
  double* fb = sf + (size_t)Na * R;
  double* red = fb + (size_t)(Nb > 0 ? Nb : 1) * R;
  for (int e = threadIdx.x; e < Na * R; e += 256) { const int i = e / R, r = e - i * R; fa[e] = a.Fa[i + a.lda * r]; }
  for (int e = threadIdx.x; e < Nb * R; e += 256) { const int i = e / R, r = e - i * R; fb[e] = a.Fb ? a.Fb[i + a.ldb * r] : 1.0; }
  __syncthreads();
  const TT* X = reinterpret_cast<const TT*>(a.X) + (int64_t)row * a.sn;
  double acc[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) acc[r] = 0.0;
  const int npairs = Na * Nb;
  for (int p = threadIdx.x; p < npairs; p += 256) {
    const int ia = p % Na, ib = p / Na;
    const double x = (double)X[(int64_t)ia * a.sa + (int64_t)ib * a.sb];
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
      if (r < R) acc[r] += x * (fa[ia * R + r] * fb[ib * R + r]);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    const double v = wave_sum(acc[r]);
    if (lane == 0) red[w * RMAX + r] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < R) {
    const int r = threadIdx.x;
    const double tot = (red[r] + red[RMAX + r]) + (red[2 * RMAX + r] + red[3 * RMAX + r]);
    a.out[row + a.ldOut * r] = a.scale * tot;
  }
}

bool small_mttkrp_ok(int64_t elems, int nd, const int64_t* dims, int R) {
  // switch read on every call (not cached): the test suite runs the solver tests both ways in one process, so that
  // the tensor-pass kernels and the partial-contraction cache stay covered at the sizes the oracle can follow
  const bool off = getenv("AOADMM_NO_SMALL_MTTKRP") != nullptr;
  if (off || elems > kSmallMttkrpElems || !(nd == 2 || nd == 3) || R > 16) return false;
  int64_t sum = 0;                                   // the factors of the two other modes sit in LDS, whatever the target
  for (int i = 0; i < nd; ++i) sum += dims[i];
  return (size_t)(sum * R + 64) * sizeof(double) <= 40 * 1024;
}

bool small_mttkrp(const SmallMttkrp& a, int prec, int64_t rows, hipStream_t s, const SysBuild* sys) {
  if (!sys_can_ride(sys)) sys = nullptr;
  const int hs = sys ? 1 : 0;
  const SysBuild sb = sys ? *sys : SysBuild();
  AO_REQUIRE(a.R >= 1 && a.R <= 16 && rows >= 1 && a.Na >= 1 && a.Nb >= 1, "small_mttkrp: bad sizes");
  const int rmax = a.R <= 4 ? 4 : (a.R <= 8 ? 8 : 16);
  const size_t lds = ((size_t)(a.Na + a.Nb) * a.R + 4 * rmax) * sizeof(double);
  AO_REQUIRE(lds <= 48 * 1024, "small_mttkrp: factors do not fit LDS");
#define AO_SM(TT, RM) small_mttkrp_k<TT, RM><<<(unsigned)(rows + hs), 256, lds, s>>>(a, hs, sb)
  if (prec == AOADMM_PREC_F32) { if (rmax == 4) AO_SM(float, 4); else if (rmax == 8) AO_SM(float, 8); else AO_SM(float, 16); }
  else { if (rmax == 4) AO_SM(double, 4); else if (rmax == 8) AO_SM(double, 8); else AO_SM(double, 16); }
#undef AO_SM
  AO_KERNEL_CHECK();
  return sys != nullptr;
}

template <typename TT>
__global__ void t_to_colmajor_k(const TT* __restrict__ T, int nchunk, int64_t trows, int64_t A, int R,
                                double scale, double* __restrict__ out, int64_t ldOut) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= A * R) return;
  const int64_t a = idx / R;
  const int r = (int)(idx - a * R);
  double tot = 0.0;
  for (int ch = 0; ch < nchunk; ++ch) tot += (double)T[(int64_t)ch * trows * R + idx];
  out[a + ldOut * r] = scale * tot;
}

void launch_t_to_colmajor(const void* T, int tprec, int nchunk, int64_t trows, int64_t A, int R, double scale,
                          double* out, int64_t ldOut, hipStream_t s) {
  const unsigned nb = (unsigned)cdiv(A * R, 256);
  if (tprec == AOADMM_PREC_F32) t_to_colmajor_k<float><<<nb, 256, 0, s>>>((const float*)T, nchunk, trows, A, R, scale, out, ldOut);
  else t_to_colmajor_k<double><<<nb, 256, 0, s>>>((const double*)T, nchunk, trows, A, R, scale, out, ldOut);
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
