// Fold-in of new slabs into a fitted PARAFAC2 block: the row of C of every new slab X_q
// (I x J_q, column-major, back to back) against the fitted A (I x R) and DeltaB (R x R), with B = P DeltaB imposed exactly:
//   Y = X_q' A,  S = (A'A) .* (DeltaB'DeltaB),  c = c0[q]
//   repeat:  W = Y diag(c) DeltaB',  P = U V' of svd(W, 'econ'),  B = P DeltaB,  b(r) = sum_j Y(j, r) B(j, r),
//            constraint 0: c = (S + ridge I)^-1 b;  constraint 1: the cold-started row loop of foldin.h on (S + ridge I, b)
//   until ||c - c_old|| <= tol ||c|| or max_iter;   res = ||X_q||^2 - 2 c'b + c'S c
// Three kernels, in this order on one stream:
//   par2_fold_system_k  one workgroup: A'A, DeltaB'DeltaB, S, rho = trace(S) / R, L = chol(S + shift I); a failed pivot
//                       sets AdmmCtl::notpd and the alternation returns at once.
//   par2_fold_y_k<T>    one wave per (slab, group of 16 slab columns[, chunk of rows of I]): Y by v_mfma_f64_16x16x4_f64,
//                       T = ceil(R / 16) factor tiles, the rows staged through LDS so that global loads run along i; the
//                       same wave leaves its part of ||X_q||^2.  Chunked (I > kP2FoldChunkRows): par2_fold_ysum_k adds
//                       the chunks' partials in chunk order.
//   par2_fold_alt_k     one wave per slab: the whole alternation with a uniform per-slab exit.
// No float atomics, no dependence between workgroups: a slab's outputs are a function of A, DeltaB, the slab, c0[q] and
// the options.
#pragma once
#include "common.h"
#include "small.h"

namespace aoadmm {

constexpr int kP2FoldTile = 16;            // slab columns per work item, factor columns per MFMA tile
constexpr int kP2FoldStage = 64;           // rows of I staged per step of the Y pass (one per lane)
constexpr int kP2FoldChunkRows = 4096;     // rows of I per chunk of the Y pass; the number of chunks depends on I alone
constexpr size_t kP2FoldLdsBudget = 48 * 1024;   // the budget of par2_b_path()

struct P2FoldinOptions {
  int max_iter = 50;
  double tol = 1e-8, ridge = 0.0;
  int constraint = 0;                      // 0: none, 1: non-negativity
  int max_inner = 5;
  double tol_primal = 0.0, tol_dual = 0.0;
};

// Which kernels a call runs.  Decided from the sizes alone, in one place: the launcher and the `path` output of
// aoadmm_resident_par2_fold_in both read it.  nk does not enter (a slab's bits do not depend on the call it is part of);
// it is an argument so that a later class may depend on it without a change of every caller.
struct P2FoldinPath {
  int tiles;       // T of par2_fold_y_k<T>: 1 .. 4
  int chunks;      // chunks of I in the Y pass: ceil(I / kP2FoldChunkRows); > 1: chunked
  int alt_lds;     // 1: Y_q and W in LDS (R^2 + 2 Jmax R doubles fit kP2FoldLdsBudget), 0: in a workspace
  int y_class() const { return 2 * (tiles - 1) + (chunks > 1 ? 1 : 0); }   // AOADMM_P2FOLD_Y_*: 0 .. 7
  int alt_class() const { return alt_lds ? 0 : 1; }                        // AOADMM_P2FOLD_ALT_LDS / _WS
};
P2FoldinPath par2_foldin_path(int64_t I, int R, int Jmax, int64_t nk);

struct P2FoldinArgs {
  int I = 0, R = 0, Jmax = 0;
  int64_t nk = 0, Jtot = 0;
  const double* A = nullptr;         // device I x R column-major, leading dimension lda
  int64_t lda = 0;
  const double* DeltaB = nullptr;    // device R x R
  const double* X = nullptr;         // device: the slabs back to back
  const int64_t* off = nullptr;      // device [nk + 1]: prefix sums of J_q
  const double* c0 = nullptr;        // device nk x R column-major, or null: ones
  P2FoldinOptions opt;
  // the work items of the Y pass
  int64_t items = 0;
  const int* item_q = nullptr;       // device [items]
  const int* item_g = nullptr;       // device [items]: the group of 16 columns
  const int64_t* item0 = nullptr;    // device [nk + 1]: first item of every slab
  double* ypart = nullptr;           // device [chunks][Jtot R] (chunked only)
  double* xpart = nullptr;           // device [items][chunks]: parts of ||X_q||^2
  double* sys = nullptr;             // device: S (R R), L (R R), rho (1)
  AdmmCtl* ctl = nullptr;            // device: notpd
  double* W = nullptr;               // device [Jtot R]: workspace of the alternation (workspace class only)
  double* Y = nullptr;               // device [Jtot R], slab layout
  double* P = nullptr;               // device [Jtot R], slab layout
  double* B = nullptr;               // device [Jtot R], slab layout
  double* C = nullptr;               // device nk x R column-major
  double* res = nullptr;             // device [nk]
  double* xnorm = nullptr;           // device [nk]
  int* iters = nullptr;              // device [nk]
  int* info = nullptr;               // device [nk]
};
void par2_foldin_enqueue(const P2FoldinArgs& a, hipStream_t s);
size_t par2_foldin_sys_doubles(int R);

// algorithmic bytes (the slabs, A, the outputs) and flops (2 I sum J_q R for Y, and per iteration and slab the J_q R^2
// terms: W, the sweeps counted as one product, P, B); iter_cols = sum over the slabs of iters[q] J_q
double par2_foldin_bytes(int I, int R, int64_t nk, int64_t Jtot);
double par2_foldin_flops(int I, int R, int64_t Jtot, double iter_cols);

}  // namespace aoadmm
