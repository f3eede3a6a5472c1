// Sparse (COO) CP blocks: Z.object{p} as a Tensor Toolbox sptensor or a MATLAB sparse matrix (cmtf_AOADMM.m:77-79,
// :132; cmtf_fun_AOADMM.m:97, :108, :111).  One copy of the coalesced nonzeros per mode, sorted by that mode's index,
// and an MTTKRP that streams it in fixed chunks of nonzeros with no float atomics.
#pragma once
#include "common.h"

namespace aoadmm {

constexpr int kCooMaxModes = 8;
constexpr int kCooChunk = 256;     // nonzeros per team of the MTTKRP kernel, carries per team of the fix-up passes

// the nonzeros sorted by the index of one mode (stable: inside a row they keep the column-major linear order)
struct CooMode {
  DevBuf row;    // int32 [nnz]: this mode's index
  DevBuf oidx;   // int32 [(N-1) x nnz]: the other modes' indices in mode order, one array per mode
  DevBuf val;    // fp64 [nnz]
};

struct CooBlock {
  int nd = 0;
  int64_t dims[kCooMaxModes] = {0};
  int64_t nnz = 0;               // after coalescing
  CooMode mode[kCooMaxModes];
  DevBuf slot_row[2], slot_val[2];   // carries of the chunks that share a row with a neighbour (ping-pong per level)
  void clear() { *this = CooBlock(); }
  CooBlock() = default;
  CooBlock(CooBlock&&) = default;
  CooBlock& operator=(CooBlock&&) = default;
};

// one factor as the kernel gathers it: element (i, r) at p[i * sI + r * sR] (column-major: sI = 1, sR = ld;
// the row-major copy of the Gram kernel: sI = R, sR = 1)
struct CooFactor {
  const double* p;
  int64_t sI, sR;
};

// Validates (0 <= subs < dims, AOADMM_ERR_INVALID otherwise), sorts on the device, sums duplicate subscripts and
// builds the per-mode copies.  subs: column-major nnz x nd int64 (sptensor.subs layout, 0-based); vals: nnz doubles.
void coo_build(CooBlock& b, int nd, const int64_t* dims, int64_t nnz, const int64_t* subs, const double* vals,
               hipStream_t s);

// out(:, 0:R-1) (column-major, leading dimension ldOut, dims[pos] rows) = scale * mttkrp of the block for mode pos.
// f[k] are the factors of the other modes in mode order.  Bitwise reproducible (no atomics).
void coo_mttkrp(CooBlock& b, int pos, const CooFactor* f, int R, double scale, double* out, int64_t ldOut,
                hipStream_t s);

// algorithmic bytes (nonzeros streamed + factor rows gathered + output written) and flops of one coo_mttkrp
double coo_mttkrp_bytes(const CooBlock& b, int pos, int R);
double coo_mttkrp_flops(const CooBlock& b, int R);

}  // namespace aoadmm
