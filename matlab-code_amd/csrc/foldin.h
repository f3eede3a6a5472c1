// Fold-in: the rows of new indices along one mode of a fitted CP block from their entries.
// For query q with observations Omega_q (a subscript for every mode but `mode`, and a value x_e):
//   z_e(r) = prod_{m != mode} F_m(s_{e,m}, r),   G_q = sum_e z_e z_e',   b_q = sum_e x_e z_e
//   constraint 0:  u_q = (G_q + ridge I)^-1 b_q
//   constraint 1:  the row ADMM loop for non-negativity on (G_q + ridge I, b_q), cold-started, rho_q = trace(G_q) / R
// A work item is one query and one chunk of at most kFoldChunk of its observations, handled by one wave: the normal
// equations by v_mfma_f64_16x16x4_f64 (the operand of a step of four observations is A and B at once), the solve by a
// one-wave register Cholesky.  A query of one chunk is solved in the launch that accumulates it (its normal equations
// reach HBM only when they are asked for); a longer one leaves one partial per chunk and a second launch sums them in
// chunk order and solves.  No float atomics, no dependence between workgroups: a query's outputs are a function of the
// factors, its own observations in the caller's order and the options.
//
// Weighted (aoadmm_resident_fold_in_w): with a weight w_e in [0, 1] per observation and alpha in [0, 1] for every cell of
// the new row the list does not name (data 0 there), and H = had_{m != mode} F_m'F_m over all rows of the other factors,
//   G_q = sum_e (w_e - alpha) z_e z_e' + alpha H,   b_q = sum_e (w_e x_e) z_e
// and everything after that is the same solve.  The weighted instantiations of the kernel run for such a call; H is
// computed inside it, once, by fixed-order kernels (skipped at alpha = 0).
#pragma once
#include "common.h"
#include "heldout.h"

namespace aoadmm {

constexpr int kFoldChunk = 256;      // observations per work item; a multiple of 4 (one MFMA step takes four)
constexpr int kFoldTile = 16;        // columns per MFMA tile

struct FoldinOptions {
  double ridge = 0.0;
  int constraint = 0;                // 0: none, 1: non-negativity
  int max_inner = 5;
  double tol_primal = 0.0, tol_dual = 0.0;
};

// The host side of one call: the observations in a stable order by query and the work items.
struct FoldinPlan {
  int64_t nq = 0, nobs = 0;
  std::vector<int64_t> qoff;         // [nq + 1] offsets of the queries into the sorted list
  std::vector<int64_t> order;        // [nobs] sorted position -> position in the caller's list
  std::vector<int> item_q, item_chunk;   // the work items
  std::vector<int64_t> pbase;        // [nq] first partial of a split query (-1: one chunk, solved where it is summed)
  std::vector<int> split_q;          // the split queries
  int64_t partials = 0;
  size_t partial_doubles(int R) const { return (size_t)R * R + R; }
};
// qcol: the query number of every observation, each in [0, nq) (checked by the caller)
FoldinPlan foldin_plan(int64_t nq, int64_t nobs, const int64_t* qcol);

struct FoldinArgs {
  HeldoutFactors hf;                 // the block's factors as Engine::heldout_factors hands them out
  int mode = 0;
  int64_t nq = 0, nobs = 0;
  FoldinOptions opt;
  const int* idx = nullptr;          // device int32 [(nd - 1) x nobs]: the other modes in mode order, sorted list
  const double* val = nullptr;       // device [nobs], sorted list
  const int64_t* qoff = nullptr;     // device [nq + 1]
  const int* item_q = nullptr;       // device, the work items
  const int* item_chunk = nullptr;
  const int64_t* pbase = nullptr;    // device [nq]
  const int* split_q = nullptr;      // device
  int64_t items = 0, splits = 0;
  double* partial = nullptr;         // device, partials x (R R + R)
  double* rows = nullptr;            // device [nq x R] column-major
  int* info = nullptr;               // device [nq]
  int* iters = nullptr;              // device [nq]
  double* gram = nullptr;            // device [nq][R x R] or null
  double* rhs = nullptr;             // device [nq x R] column-major or null
  // the weighted form: the weighted instantiations run, whatever wts and alpha are
  bool weighted = false;
  const double* wts = nullptr;       // device [nobs], sorted list; null: all ones
  double alpha = 0.0;                // the weight of an unlisted cell
  int64_t frows[kCooMaxModes] = {};  // rows of every factor of hf (alpha != 0)
  double* H = nullptr;               // device [R x R]: written by the call when alpha != 0
  double* gram_ws = nullptr;         // device, foldin_gram_ws_doubles (alpha != 0)
};
void foldin_enqueue(const FoldinArgs& a, hipStream_t s);
// H = had_{m != mode} F_m'F_m from the factors as the pass gathers them, in a fixed order that no stride enters
size_t foldin_gram_ws_doubles(const HeldoutFactors& hf, const int64_t* rows, int mode);
void foldin_gram_enqueue(const HeldoutFactors& hf, const int64_t* rows, int mode, double* ws, double* H, hipStream_t s);

// algorithmic bytes (the list streamed, the rows gathered, the outputs) and flops (the normal equations, the solves); a
// weight list adds 8 bytes per observation, alpha != 0 the 8 R other_rows bytes and R R other_rows flops of H, with
// other_rows the rows of the other modes' factors together
double foldin_bytes(int nd, int R, int64_t nq, int64_t nobs, bool normal, bool wts = false, double alpha = 0.0, int64_t other_rows = 0);
double foldin_flops(int nd, int R, int64_t nq, int64_t nobs, double alpha = 0.0, int64_t other_rows = 0);

}  // namespace aoadmm
