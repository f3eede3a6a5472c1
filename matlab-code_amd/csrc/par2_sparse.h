// PARAFAC2 blocks whose slabs are sparse (Z.object{p}{k} a MATLAB sparse matrix; cmtf_fun_AOADMM.m:163, :193, :221 only
// ever multiply a slab by a factor).  The block is ONE sparse I x Jtot matrix Xcat = [X_1 ... X_K] (global column
// g = off[k] + j), kept as a 2-way CooBlock: one copy sorted by row i, one by column g (= slab order).  With
// Y = Xcat' * A (Jtot x R) every right-hand side and the objective are one of two passes over the nonzeros
// (coo_mttkrp on the row copy or on the column copy) plus dense work on Jtot x R arrays.
#pragma once
#include "common.h"
#include "par2.h"
#include "sparse.h"

namespace aoadmm {

struct Par2Sparse {
  CooBlock coo;                 // nd = 2, dims = {I, Jtot}; mode[0]: sorted by i, mode[1]: sorted by g
  DevBuf kofg;                  // int32 [Jtot]: slab of global column g
  DevBuf xn;                    // fp64 [K]: ||X_k||_F^2
  DevBuf BC;                    // Jtot x R, row-major: B(g, r) * C(k(g), r), the factor the row pass gathers
  DevBuf Y;                     // Jtot x R, column-major: Xcat' * A
  DevBuf s;                     // K x R, column-major: s(k, r) = sum_{g in slab k} B(g, r) Y(g, r)
  bool y_valid = false;         // Y belongs to version y_version of the A mode's factor
  uint64_t y_version = 0;
  void clear() { *this = Par2Sparse(); }
  Par2Sparse() = default;
  Par2Sparse(Par2Sparse&&) = default;
  Par2Sparse& operator=(Par2Sparse&&) = default;
};

// subs: column-major nnz x 3, 0-based (i, j within the slab, k).  Validates (AOADMM_ERR_INVALID, `sp` untouched),
// coalesces duplicates and builds both sorted copies, the column -> slab map and the slab norms.
void par2s_build(Par2Sparse& sp, const P2Dims& d, int64_t nnz, const int64_t* subs, const double* vals, hipStream_t s);

// BC(g, r) = B_k(j, r) * C(k, r), row-major Jtot x R  (B in the slab layout of par2.h)
void par2s_scale_b(const double* B, const double* Cfac, const P2Dims& d, const int* kofg, double* BC, hipStream_t s);
// Ak (slab layout) = w * C(k, r) * Y(g, r)                                                 (:193)
void par2s_ak(const double* Y, const double* Cfac, double w, const P2Dims& d, const int* kofg, double* Ak, hipStream_t s);
// sv(k, r) = sum_j B_k(j, r) Y(off[k] + j, r); res != null: res[k] = ||X_k - A D_k B_k'||^2 by the expansion
// xn[k] - 2 sum_r C(k,r) sv(k,r) + sum_{r,q} GA(r,q) C(k,r) C(k,q) GB_k(r,q)               (:221, :1262-1264)
void par2s_slab_sums(const double* B, const double* Y, const P2Dims& d, double* sv, const double* xn,
                     const double* Cfac, const double* GA, const double* GB, double* res, hipStream_t s);

}  // namespace aoadmm
