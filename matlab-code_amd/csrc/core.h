// Core fold: the reduction over a partial contraction T that keeps ALL (p, r) pairs instead of the Hadamard diagonal,
// which turns a tensor pass into a Tucker projection G = X x_1 Ma' x_2 Mb' x_3 Mc' (DESIGN.md section 9.9).
//   stage 1   V(b, p, r) = sum_chunk sum_a Ma(a, p) * T[chunk][a + Apad * b][r]      (a < An)
//             per b the GEMM Ma' (Ra x An) * T_b (An x Rc) on v_mfma_f64_16x16x4_f64, fp32 T converted on load
//   stage 2   G(p, q, r) = sum_b Mb(b, q) * V(b, p, r)
// 2 An Bn Ra Rc + 2 Bn Ra Rb Rc flops; the Ra Rb Rc outer product per row of T is never formed.  T is read once, rows
// a < An only.  A long An is cut into segments of kCoreSeg rows and a long Bn into chunks of kCoreBChunk; both kinds of
// partial sums are added in ascending order by the next stage.  No float atomics: the bits depend on the inputs only.
#pragma once
#include "common.h"

namespace aoadmm {

constexpr int kCoreSeg = 1024;      // rows of An one workgroup of stage 1 sums; a longer An leaves one partial per segment
constexpr int kCoreBChunk = 128;    // rows of Bn one workgroup of stage 2 sums

struct CoreFold {
  const void* T;            // [chunk][a + Apad * b][r]: element (row, r) of a chunk at row * sRow + r * sCol
  int tprec, nchunk;        // AOADMM_PREC_F32 or AOADMM_PREC_F64
  int64_t chunk_stride;     // elements between chunks
  int64_t sRow, sCol;       // the layout of the tensor pass: sRow = Rc, sCol = 1
  int64_t An, Apad, Bn;
  int Ra, Rb, Rc;           // each in 1 .. kMaxRank
  const double* MaT;        // Ma row-major, An x ldMaT with ldMaT = round_up(Ra, 16) and the columns beyond Ra zero
  int ldMaT;
  const double* Mb;         // Bn x Rb column-major (core_fold alone)
  int64_t ldMb;
  double* ws;               // core_fold_ws_bytes()
  double* G;                // element (p, q, r) at p * sp + q * sq + r * sr
  int64_t sp, sq, sr;
};

size_t core_fold_ws_bytes(int64_t An, int64_t Bn, int Ra, int Rb, int Rc);
// both stages
void core_fold(const CoreFold& f, hipStream_t s);
// Bn = 1 and no second matrix: G(p, (r + shift) mod Rm, r) = V(p, r) wherever that column is below Rb (the sparse
// projection's rotation `shift`; Mb / ldMb are not read)
void core_fold_rotated(const CoreFold& f, int shift, int Rm, hipStream_t s);
double core_fold_flops(const CoreFold& f);

}  // namespace aoadmm
