// Leading eigenvectors of X_(n) X_(n)' for a sparse block (the SVD start of cmtf_nvecs.m / init_coupled_AOADMM_CMTF.m)
// without the I_n x I_n Gram matrix: block subspace iteration with Rayleigh-Ritz on the operator Y = M (M' V), M the
// I_n x F mode-n unfolding restricted to its F non-empty fibers.  Two passes over the nonzeros per application, both
// by the MTTKRP's team kernel and carry levels (coo_list_pass): no float atomics, bitwise reproducible.  DESIGN.md 9.2.
#pragma once
#include "common.h"
#include "cpblock.h"
#include "sparse.h"

namespace aoadmm {

constexpr int kNvecsOversample = 8;
constexpr int kNvecsMaxIters = 500;
constexpr double kNvecsTol = 1e-10;

// The two lists of one mode.  2-way blocks (and Xcat of a PARAFAC2 block with sparse slabs): views of the block's two
// copies, nothing owned.  Order >= 3: fib and the fiber ids of row are built here (20 bytes per nonzero) and live as
// long as this object.
struct NvecsLists {
  CooList fib;          // sorted by fiber id: gidx = the mode-n subscript; rows = F
  CooList row;          // sorted by the mode-n subscript (the block's own copy): gidx = the fiber id; rows = I_n
  DevBuf fkey, frow, fval, fid;
  float build_ms = 0.f;
};
// Builds the lists of mode `pos` of a block with nonzeros; compares what it allocates with the free device memory
// first (AOADMM_ERR_NOMEM).
void nvecs_build_lists(NvecsLists& l, const CooBlock& b, int pos, hipStream_t s);

// U (host, I_n x r column-major, leading dimension ldU; null: not read back) = the r leading eigenvectors, eig (host,
// optional) their eigenvalues, descending.  `timers` (optional): every pass over the nonzeros is counted in stats[3].
void sparse_nvecs(const NvecsLists& l, int r, const aoadmm_nvecs_options* opt, double* U, int64_t ldU, double* eig,
                  aoadmm_nvecs_info* info, DevBuf* slot_row, DevBuf* slot_val, LaunchTimers* timers, hipStream_t s);

}  // namespace aoadmm
