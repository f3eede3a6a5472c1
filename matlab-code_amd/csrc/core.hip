// Core fold over a partial contraction (core.h).
//
// Stage 1 operand map of v_mfma_f64_16x16x4_f64, the one topk.hip uses: lane (c = l & 15, q4 = l >> 4) supplies
// A[row c][k = q4] = Ma(a0 + q4, 16 pt + c) and B[k = q4][col c] = T(a0 + q4, 16 ct + c) and receives
// D[row q4 + 4 e][col c], e = 0 .. 3: the (p, r) tile (pt, ct) of V for one b.  A workgroup is one (b, segment of An);
// its waves share the ceil(Ra / 16) * ceil(Rc / 16) tiles, at most kCoreTilesPerWave each.  A tile's sum runs over the
// chunks and, inside a chunk, over a in steps of four from the segment's first row: its order is a function of the
// shapes alone.
#include "core.h"

namespace aoadmm {

typedef double core_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kCoreWave = 64;
constexpr int kCoreMaxWaves = 4;
constexpr int kCoreTilesPerWave = 4;   // 16 tiles at Ra = Rc = 64 over 4 waves

template <class TT, int NT>
__global__ __launch_bounds__(kCoreWave* kCoreMaxWaves) void core_fold1_k(CoreFold f) {
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63;
  constexpr int U = NT == 1 ? 8 : (NT == 2 ? 4 : 2);   // steps of four rows whose loads are in flight together: U * NT = 6 .. 8 per operand
  const int c = lane & 15, q4 = lane >> 4;
  const int64_t b = blockIdx.x, seg = blockIdx.y;
  const int64_t a_lo = seg * kCoreSeg;
  const int64_t a_hi = a_lo + kCoreSeg < f.An ? a_lo + kCoreSeg : f.An;
  const int RcT = (f.Rc + 15) >> 4, ntiles = ((f.Ra + 15) >> 4) * RcT;

  bool live[NT], bok[NT];
  int acol[NT], brow0[NT], bcol[NT];
  int64_t boff[NT];
  core_f64x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int t = wave + nw * i;
    live[i] = t < ntiles;                              // wave-uniform
    const int pt = live[i] ? t / RcT : 0, ct = live[i] ? t % RcT : 0;
    acol[i] = 16 * pt + c;                             // < ldMaT: the copy is padded with zero columns
    brow0[i] = 16 * pt;
    bcol[i] = 16 * ct + c;
    bok[i] = bcol[i] < f.Rc;
    boff[i] = (int64_t)(bok[i] ? bcol[i] : f.Rc - 1) * f.sCol;
    acc[i] = core_f64x4{0.0, 0.0, 0.0, 0.0};
  }
  const TT* T = static_cast<const TT*>(f.T);
  for (int ch = 0; ch < f.nchunk; ++ch) {
    const TT* Tc = T + (int64_t)ch * f.chunk_stride + f.Apad * b * f.sRow;
    for (int64_t a0 = a_lo; a0 < a_hi; a0 += 4 * U) {
      // The loads of U steps are issued before the first MFMA, so that U rows of T are in flight per wave (one step at
      // a time the fold waits out one HBM round trip per four rows).  Unconditional loads on clamped addresses; what a
      // clamp brought in is replaced by zero.  The MFMAs run in the order of a: unrolling moves no bit.
      double av[U][NT];
      TT tv[U][NT];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t ar = a0 + 4 * u + q4;
        ok[u] = ar < a_hi;
        const int64_t arc = ok[u] ? ar : a_hi - 1;
        const double* mrow = f.MaT + arc * f.ldMaT;
        const TT* trow = Tc + arc * f.sRow;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          av[u][i] = mrow[acol[i]];                    // (a dead tile reads tile 0's addresses: in bounds, unused)
          tv[u][i] = trow[boff[i]];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (a0 + 4 * u >= a_hi) break;                 // wave-uniform
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          if (!live[i]) continue;
          acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(ok[u] ? av[u][i] : 0.0, ok[u] && bok[i] ? (double)tv[u][i] : 0.0,
                                                        acc[i], 0, 0, 0);
        }
      }
    }
  }
  double* V = f.ws + ((int64_t)seg * f.Bn + b) * f.Ra * f.Rc;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (!live[i] || !bok[i]) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int p = brow0[i] + q4 + 4 * e;
      if (p < f.Ra) V[(int64_t)p * f.Rc + bcol[i]] = acc[i][e];
    }
  }
}

// Gp[bchunk][p][q][r] = sum over the chunk's b, ascending, of Mb(b, q) * (sum over the segments, ascending, of V)
__global__ __launch_bounds__(256) void core_fold2_k(CoreFold f, int nseg, double* Gp) {
  const int E = f.Ra * f.Rb * f.Rc;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int r = e % f.Rc, q = (e / f.Rc) % f.Rb, p = e / (f.Rc * f.Rb);
  const int64_t b0 = (int64_t)blockIdx.y * kCoreBChunk;
  const int64_t b1 = b0 + kCoreBChunk < f.Bn ? b0 + kCoreBChunk : f.Bn;
  const int64_t segstride = f.Bn * f.Ra * f.Rc;
  const double* mb = f.Mb + f.ldMb * q;
  double sum = 0.0;
  for (int64_t b = b0; b < b1; ++b) {
    const double* v = f.ws + (b * f.Ra + p) * f.Rc + r;
    double vs = v[0];
    for (int sg = 1; sg < nseg; ++sg) vs += v[sg * segstride];
    sum += mb[b] * vs;
  }
  Gp[(int64_t)blockIdx.y * E + e] = sum;
}

// G(p, q, r) = sum over the chunks of Bn, ascending
__global__ __launch_bounds__(256) void core_fold3_k(CoreFold f, int nbc, const double* Gp) {
  const int E = f.Ra * f.Rb * f.Rc;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int r = e % f.Rc, q = (e / f.Rc) % f.Rb, p = e / (f.Rc * f.Rb);
  double sum = Gp[e];
  for (int bc = 1; bc < nbc; ++bc) sum += Gp[(int64_t)bc * E + e];
  f.G[p * f.sp + q * f.sq + r * f.sr] = sum;
}

// Bn = 1: G(p, (r + shift) mod Rm, r) = sum over the segments, ascending, of V(p, r)
__global__ __launch_bounds__(256) void core_place_k(CoreFold f, int nseg, int shift, int Rm) {
  const int E = f.Ra * f.Rc;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int r = e % f.Rc, p = e / f.Rc;
  const int q = (r + shift) % Rm;
  if (q >= f.Rb) return;
  double vs = f.ws[e];
  for (int sg = 1; sg < nseg; ++sg) vs += f.ws[(int64_t)sg * E + e];
  f.G[p * f.sp + q * f.sq + r * f.sr] = vs;
}

static int64_t core_nseg(int64_t An) { return cdiv(An, (int64_t)kCoreSeg); }
static int64_t core_nbc(int64_t Bn) { return cdiv(Bn, (int64_t)kCoreBChunk); }

size_t core_fold_ws_bytes(int64_t An, int64_t Bn, int Ra, int Rb, int Rc) {
  return (size_t)(core_nseg(An) * Bn * Ra * Rc + core_nbc(Bn) * Ra * Rb * Rc) * sizeof(double);
}

double core_fold_flops(const CoreFold& f) {
  return 2.0 * f.nchunk * (double)f.An * f.Bn * f.Ra * f.Rc + 2.0 * (double)f.Bn * f.Ra * f.Rb * f.Rc;
}

static void core_check(const CoreFold& f) {
  AO_REQUIRE(f.Ra >= 1 && f.Ra <= kMaxRank && f.Rb >= 1 && f.Rb <= kMaxRank && f.Rc >= 1 && f.Rc <= kMaxRank,
             "core fold: ranks %d, %d, %d outside 1..%d", f.Ra, f.Rb, f.Rc, kMaxRank);
  AO_REQUIRE(f.An >= 1 && f.Bn >= 1 && f.Apad >= f.An && f.nchunk >= 1, "core fold: empty T");
  AO_REQUIRE(f.ldMaT == round_up(f.Ra, 16), "core fold: the row-major matrix must be padded to %lld columns",
             (long long)round_up(f.Ra, 16));
  AO_REQUIRE(f.Bn < ((int64_t)1 << 31) && core_nseg(f.An) <= 65535 && core_nbc(f.Bn) <= 65535,
             "core fold: %lld x %lld rows of T are more than one launch holds", (long long)f.An, (long long)f.Bn);
  AO_REQUIRE(f.tprec == AOADMM_PREC_F32 || f.tprec == AOADMM_PREC_F64, "core fold: T in precision %d", f.tprec);
}

static void core_stage1(const CoreFold& f, hipStream_t s) {
  const int ntiles = (int)(cdiv(f.Ra, 16) * cdiv(f.Rc, 16));
  const int nw = ntiles < kCoreMaxWaves ? ntiles : kCoreMaxWaves;
  const int nt = (int)cdiv(ntiles, nw);                // tiles per wave: 1 .. kCoreTilesPerWave
  AO_REQUIRE(nt <= kCoreTilesPerWave, "internal: %d tiles per wave", nt);
  const dim3 grid((unsigned)f.Bn, (unsigned)core_nseg(f.An));
  const unsigned threads = (unsigned)(nw * kCoreWave);
  const bool f32 = f.tprec == AOADMM_PREC_F32;
  switch (nt) {
    case 1: f32 ? core_fold1_k<float, 1><<<grid, threads, 0, s>>>(f) : core_fold1_k<double, 1><<<grid, threads, 0, s>>>(f); break;
    case 2: f32 ? core_fold1_k<float, 2><<<grid, threads, 0, s>>>(f) : core_fold1_k<double, 2><<<grid, threads, 0, s>>>(f); break;
    case 3: f32 ? core_fold1_k<float, 3><<<grid, threads, 0, s>>>(f) : core_fold1_k<double, 3><<<grid, threads, 0, s>>>(f); break;
    default: f32 ? core_fold1_k<float, 4><<<grid, threads, 0, s>>>(f) : core_fold1_k<double, 4><<<grid, threads, 0, s>>>(f); break;
  }
  AO_KERNEL_CHECK();
}

void core_fold(const CoreFold& f, hipStream_t s) {
  core_check(f);
  AO_REQUIRE(f.Mb != nullptr && f.ldMb >= f.Bn, "core fold: second matrix missing or its leading dimension too small");
  core_stage1(f, s);
  const int nseg = (int)core_nseg(f.An), nbc = (int)core_nbc(f.Bn);
  const int E = f.Ra * f.Rb * f.Rc;
  double* Gp = f.ws + (int64_t)nseg * f.Bn * f.Ra * f.Rc;
  core_fold2_k<<<dim3(blocks_for(E), (unsigned)nbc), 256, 0, s>>>(f, nseg, Gp);
  AO_KERNEL_CHECK();
  core_fold3_k<<<blocks_for(E), 256, 0, s>>>(f, nbc, Gp);
  AO_KERNEL_CHECK();
}

void core_fold_rotated(const CoreFold& f, int shift, int Rm, hipStream_t s) {
  core_check(f);
  AO_REQUIRE(f.Bn == 1 && Rm >= f.Rb && Rm >= f.Rc && shift >= 0 && shift < Rm, "core fold: bad rotation %d of %d", shift, Rm);
  core_stage1(f, s);
  core_place_k<<<blocks_for(f.Ra * f.Rc), 256, 0, s>>>(f, (int)core_nseg(f.An), shift, Rm);
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
