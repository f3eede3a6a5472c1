// Held-out scoring: the model of a CP or PARAFAC2 block evaluated at a list of subscripts.
//   m(s) = sum_r prod_n F_n(s_n, r)                          CP block of any order up to kCooMaxModes
//   m(i, j, k) = sum_r A(i, r) B_k(j, r) C(k, r),  j < J_k   PARAFAC2 block (B_k as par2.h stores it)
// Either the values in the caller's order (heldout_model_at) or three sums against attached values y
// (heldout_stats_enqueue): sum (y - m)^2, sum y^2, sum m^2.  Gathers only: nothing of the block's data is read, so the
// pass serves dense, sparse, sharded and data-less blocks alike.  Every sum has a fixed order (the xor butterfly inside a
// team, a team's entries in list order, the teams' partials in a strided order with an LDS tree): no float atomics, two
// runs return the same bits.
#pragma once
#include "common.h"
#include "sparse.h"

namespace aoadmm {

constexpr int kHeldoutSums = 3;     // sum (y - m)^2, sum y^2, sum m^2

// The attached list of one block: 4 N + 8 bytes per entry on the device, in the caller's order.
struct HeldoutList {
  int nd = 0;
  int64_t n = 0;                  // entries (duplicates included); 0: no list
  DevBuf idx;                     // int32 [nd x n]: subscript of mode m of entry e at idx[m * n + e]
  DevBuf val;                     // fp64 [n]
  DevBuf part;                    // kHeldoutSums partial sums per team
  int64_t resident_bytes() const { return n > 0 ? n * (4 * (int64_t)nd + 8) : 0; }
  void clear() { *this = HeldoutList(); }
  HeldoutList() = default;
  HeldoutList(HeldoutList&&) = default;
  HeldoutList& operator=(HeldoutList&&) = default;
};

// What one pass gathers from.  f[m] addresses factor m as sparse.h's CooFactor does.  off != null: a PARAFAC2 block;
// f[1].p is then the base of the B_k slabs, slab k at off[k] * R, column-major J_k x R with J_k = off[k + 1] - off[k],
// and k is the entry's third subscript (f[1].sI / sR are ignored).
struct HeldoutFactors {
  CooFactor f[kCooMaxModes];
  int nd = 0, R = 0;
  const int64_t* off = nullptr;   // device, K + 1 prefix sums of J_k
};

// out[e] = m(idx[:, e]) for e < n, device buffers, caller's order
void heldout_model_at(const HeldoutFactors& hf, const int* idx, int64_t n, double* out, hipStream_t s);
// sums[0..2] (device) = sum (y - m)^2, sum y^2, sum m^2 over the list; `part` holds kHeldoutSums doubles per team
void heldout_stats_enqueue(const HeldoutFactors& hf, const int* idx, const double* val, int64_t n, double* part, double* sums,
                           hipStream_t s);
inline int64_t heldout_teams(int64_t n) { return cdiv(n, kCooChunk); }

// algorithmic bytes (subscripts and values streamed, factor rows gathered, values written) and flops of one pass
double heldout_pass_bytes(int nd, int R, int64_t n, bool stats);
double heldout_pass_flops(int nd, int R, int64_t n, bool stats);

}  // namespace aoadmm
