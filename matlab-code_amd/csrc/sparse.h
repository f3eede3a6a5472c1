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
  int64_t nnz = 0;               // entries of every mode's copy: all coalesced nonzeros, or this rank's share of them
  CooMode mode[kCooMaxModes];
  DevBuf slot_row[2], slot_val[2];   // carries of the chunks that share a row with a neighbour (ping-pong per level)
  // Sharded over the ranks of a communicator (coo_keep_share): every mode's copy holds the entries
  // [coo_share_begin(nnz_full, rank, world), coo_share_begin(nnz_full, rank + 1, world)) of that mode's sorted order,
  // so a rank's part of mode n lies in the rows [span0[n], span1[n]] (span0 = -1: an empty share)
  bool sharded = false;
  int cut_rank = 0, cut_world = 1;
  int64_t nnz_full = 0;          // coalesced nonzeros of the whole tensor
  int64_t span0[kCooMaxModes] = {0}, span1[kCooMaxModes] = {0};
  // send[n]: dims[n] x send_R[n] doubles, the sharded MTTKRP of mode n in front of its all-reduce.  Rows outside the
  // span are zero: cleared when the buffer is made, never written afterwards (the span belongs to the block and a new
  // upload makes a new block, so no buffer outlives its cut)
  DevBuf send[kCooMaxModes];
  int send_R[kCooMaxModes] = {0};
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

// first entry of rank g's share of nnz sorted entries: floor(g * nnz / world) (nnz < 2^31: the product fits)
inline int64_t coo_share_begin(int64_t nnz, int g, int world) { return nnz * g / world; }
// Keeps rank `rank`'s share of every mode's copy in buffers of the share's size (oidx strided by the share's count) and
// frees the full copies, one mode at a time: N (4 N + 8) bytes per kept nonzero stay resident.  The peak is that of
// coo_build.  Call once, on a freshly built block.
void coo_keep_share(CooBlock& b, int rank, int world, hipStream_t s);

// out(:, 0:R-1) (column-major, leading dimension ldOut, dims[pos] rows) = scale * mttkrp of the block for mode pos.
// f[k] are the factors of the other modes in mode order.  Bitwise reproducible (no atomics).
// span_only (sharded blocks): clears and writes the rows [span0[pos], span1[pos]] of `out` alone -- this rank's partial
// sums, complete after the sum over the ranks; an empty share touches nothing.
// vals (optional): nnz values in the order of mode pos's copy, read instead of CooMode::val (the residuals of an
// observed-only block, sparse_em.h)
void coo_mttkrp(CooBlock& b, int pos, const CooFactor* f, int R, double scale, double* out, int64_t ldOut,
                hipStream_t s, bool span_only = false, const double* vals = nullptr);

// A list of n entries sorted by `key` (int32, 0 <= key < rows); entry e carries the index gidx[e] and the value val[e]
struct CooList {
  const int* key;
  const int* gidx;
  const double* val;
  int64_t n, rows;
};
// out(k, 0:R-1) = sum over the entries e with key[e] = k of val[e] * src(gidx[e], 0:R-1), src and out ROW-major with R
// doubles per row (out: l.rows rows, all of them written).  The MTTKRP's team kernel and carry levels with one gathered
// factor: no float atomics, bitwise reproducible.  slot_row / slot_val: two carry buffers each (ping-pong per level).
void coo_list_pass(const CooList& l, const double* src, int R, double* out, DevBuf* slot_row, DevBuf* slot_val,
                   hipStream_t s);

// Pieces of coo_build that the fiber lists of sparse_nvecs.hip use as well.
struct CooSortWork { DevBuf permA, permB, keyA, keyB, tmp, stride; };
// w.permA = the order of the n entries by column-major linear index over the nd index arrays idx[m * n + e]
// (0 <= idx < dims[m]); stable LSD radix sorts over groups of modes whose linear index fits in 64 bits
void coo_sort_linear(CooSortWork& w, const int* idx, int64_t n, int nd, const int64_t* dims, hipStream_t s);
// head[i] = 1 where sorted entry i differs from entry i - 1 in any index, seg = inclusive scan of head (the 1-based run
// of every sorted entry); returns the number of runs (one host read)
int64_t coo_runs_scan(CooSortWork& w, DevBuf& head, DevBuf& seg, const int* idx, int64_t n, int nd, hipStream_t s);

// algorithmic bytes (nonzeros streamed + factor rows gathered + output written: all rows, or the span of a sharded
// block) and flops of one coo_mttkrp, from the entries this rank holds
double coo_mttkrp_bytes(const CooBlock& b, int pos, int R);
double coo_mttkrp_flops(const CooBlock& b, int R);

}  // namespace aoadmm
