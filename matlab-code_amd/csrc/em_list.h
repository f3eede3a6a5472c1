// The missing entries of a masked dense CP block as a list: the EM imputation
// (functions/cmtf_fun_AOADMM.m:410-441) needs the model only there.
//   em_list_build  the list from the block's one-bit-per-entry mask (em.h), on the device, in ascending storage offset:
//                  a count kernel per 64-bit word, one scan, an emit kernel that decodes each offset into subscripts once
//   em_list_pass   per listed entry  m = sum_r prod_n F_n(s_n, r) in fp64 (the team layout of coo_team.h),
//                  num += (m - x_old)^2, den += x_old^2, and with update = 1  x <- m, rounded once to the block's precision
// Observed entries are never touched.  Every sum has a fixed order (the xor butterfly inside a team, a team's entries in
// list order over kEmListUnroll accumulators, the teams' partials in a strided order with an LDS tree): no float atomics,
// two runs return the same bits, and the list's order is a function of the mask alone.
#pragma once
#include "common.h"
#include "heldout.h"

namespace aoadmm {

constexpr int kEmListSums = 2;      // num, den

// The list of one block: 4 N bytes per entry on the device, laid out as HeldoutList::idx.  The storage offsets are not
// kept: the pass forms them from the subscripts it has loaded for the gathers.
struct MissingList {
  bool on = false;                // the block is marked (n = 0: marked, nothing missing)
  int nd = 0;
  int64_t n = 0;
  DevBuf idx;                     // int32 [nd x n]: subscript of mode m of entry e at idx[m * n + e]
  DevBuf part;                    // kEmListSums partial sums per team
  int64_t resident_bytes() const { return on && n > 0 ? n * 4 * (int64_t)nd + heldout_teams(n) * kEmListSums * 8 : 0; }
  void clear() { *this = MissingList(); }
  MissingList() = default;
  MissingList(MissingList&&) = default;
  MissingList& operator=(MissingList&&) = default;
};

// `l` becomes the list of the mask `bits` (em_mask_pack's layout over Ipad x dims[1] x ... entries; a bit past the last
// entry counts as observed).  Synchronises the stream once for the count.  Throws (AOADMM_ERR_NOMEM when the list does
// not fit) with `l` as it was.
void em_list_build(MissingList& l, const uint8_t* bits, int nd, const int64_t* dims, int64_t Ipad, hipStream_t s);

struct EmListArgs {
  const int* idx;                 // MissingList::idx
  int64_t n;
  HeldoutFactors hf;              // what the pass gathers from (off unused)
  void* X;                        // the block's natural array, float / double
  void* Xt;                       // matrices: the transposed copy (second mode contiguous, padded to Jpad); else null
  int64_t stride[kCooMaxModes];   // storage stride of every mode in X: 1, Ipad, Ipad * dims[1], ...
  int64_t Jpad;
  int update;                     // 0: the two sums only; 1: also x <- m in X (and Xt)
  double* part;                   // MissingList::part
};
// num, den (device): the two sums over the list; n = 0 launches nothing and writes two zeros
void em_list_pass(const EmListArgs& a, int prec, double* num, double* den, hipStream_t s);

// algorithmic bytes and flops of one pass: those of a held-out statistics pass (heldout_pass_bytes) with the value read
// from the array in the block's precision instead of the list, plus its write when update = 1
double em_list_pass_bytes(int nd, int R, int64_t n, int prec, bool update);
double em_list_pass_flops(int nd, int R, int64_t n);

}  // namespace aoadmm
