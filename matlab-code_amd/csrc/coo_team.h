// The team layout of the sparse (COO) kernels, written once: mttkrp_coo_k and coo_carry_k (sparse.hip), sem_pass_k
// (sparse_em.hip) and model_at_k (heldout.hip) walk a list of entries with it, and their launches pick the team width
// and the compiled-in order with the dispatchers below.  DESIGN.md section 9.
//
// A team is G consecutive lanes of a workgroup of 256 (G = 4 .. 64 divides the wavefront, so a team never straddles
// two).  Team t owns the kCooChunk consecutive entries [t * kCooChunk, min(+ kCooChunk, n)) of the list, lane r owns
// column r of every factor row, G >= R.  Lanes beyond R read column R - 1, so that every address is valid, and
// contribute nothing (they are not live()).  Teams past the end of the list leave as a whole (idle()): a team_sum never
// meets a lane that has returned.  The entries are walked U at a time (the loads of U entries are in flight together);
// the walk's tail reads the range's last entry again (i = i0 + u < end ? i0 + u : end - 1) and drops the value
// (i0 + u < end).
#pragma once
#include <type_traits>

#include "sparse.h"

namespace aoadmm {

// A kernel begins with
//   const CooTeam<G> t(n, R);
//   if (t.idle()) return;
// and takes end(), rr() and live() after that.  They are functions, not members filled before the return, because
// the compiler simplifies a helper's body before it inlines it: what is computed past the early return, with
// start < n known, compiles to the code the kernels had when each spelled the layout out.
template <int G>
struct CooTeam {
  int64_t n;                  // entries of the list
  int R;
  int64_t team, start;        // this team's number and the first entry of its range
  int r;                      // the lane's column
  __device__ __forceinline__ CooTeam(int64_t n_, int R_) : n(n_), R(R_) {
    team = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    r = (int)(threadIdx.x % G);
    start = team * kCooChunk;
  }
  __device__ __forceinline__ bool idle() const { return start >= n; }
  __device__ __forceinline__ int64_t end() const { return start + kCooChunk < n ? start + kCooChunk : n; }
  __device__ __forceinline__ bool live() const { return r < R; }
  __device__ __forceinline__ int rr() const { return r < R ? r : R - 1; }   // the column the lane reads
};

// element (row, rr) of a factor as the kernels gather it (the factor by value: by reference the gathers compile to
// another instruction order than the expression written out)
__device__ __forceinline__ double coo_at(const CooFactor f, int64_t row, int rr) { return f.p[row * f.sI + rr * f.sR]; }

// sum over the G lanes of a team by an xor butterfly: every lane ends with the same bits
template <int G>
__device__ __forceinline__ double team_sum(double v) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}

// Sum over a workgroup of exactly 256 threads in a fixed order, for the one-workgroup finishers of the teams' partials
// (sem_finish_k, heldout_finish_k): every thread's value, then a tree over LDS; sh holds 256 doubles.  The same tree as
// device_utils.h's block_sum_pow2, whose barriers would serve every call sequence of the two finishers as well; its
// loop over blockDim.x at run time costs sem_finish_k one more VGPR than this unrolled form.
__device__ inline double coo_block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

// ---- host side ---------------------------------------------------------------
inline int coo_team_width(int R) { return R <= 4 ? 4 : R <= 8 ? 8 : R <= 16 ? 16 : R <= 32 ? 32 : 64; }

// f(std::integral_constant<int, G>) for the team width of rank R
template <class F>
void for_team_width(int R, F&& f) {
  switch (coo_team_width(R)) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
  }
}

// f(std::integral_constant<int, n>) for the three compiled-in orders n = LO, LO + 1, LO + 2, else f(0): the kernel
// reads the order at run time.  LO = 2 over the modes of a block, LO = 1 over the other modes of an MTTKRP.
template <int LO, class F>
void for_order(int n, F&& f) {
  switch (n - LO) {
    case 0: f(std::integral_constant<int, LO>{}); break;
    case 1: f(std::integral_constant<int, LO + 1>{}); break;
    case 2: f(std::integral_constant<int, LO + 2>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
  }
}

// workgroups of 256 threads for the teams of width G that cover n entries
inline unsigned coo_team_grid(int64_t n, int G) { return blocks_for(cdiv(n, kCooChunk) * G); }

}  // namespace aoadmm
