// Snapshot of the solver state in one launch over a table of segments.  See state_snapshot.h and DESIGN.md section 9.4.
#include "state_snapshot.h"

namespace aoadmm {

constexpr int kSnapThreads = 256;
constexpr int kSnapVecPerLane = (int)(kSnapChunk / (16 * kSnapThreads));   // 16-byte vectors a lane moves per chunk
static_assert(kSnapChunk % (16 * kSnapThreads) == 0, "a chunk is a whole number of 16-byte vectors per lane");

// n > 0 bytes (a multiple of 8, at most kSnapChunk) from src to dst, both 8-byte aligned.  An 8-byte head brings both
// pointers onto a 16-byte boundary, the body moves as 16-byte vectors (all loads of a lane issued before its stores),
// an 8-byte tail finishes an odd count of doubles.
__device__ __forceinline__ void snap_copy_piece(const char* __restrict__ src, char* __restrict__ dst, int64_t n) {
  const int t = (int)threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15) != 0) {
    // not congruent modulo 16 (a table that snapshot_slot_offset did not lay out): 8 bytes at a time
    const uint64_t* s8 = reinterpret_cast<const uint64_t*>(src);
    uint64_t* d8 = reinterpret_cast<uint64_t*>(dst);
    for (int64_t i = t; i < n / 8; i += kSnapThreads) d8[i] = s8[i];
    return;
  }
  const int64_t head = (reinterpret_cast<uintptr_t>(src) & 15) != 0 ? 8 : 0;     // n >= 8: the head fits
  const int64_t nv = (n - head) / 16;                                             // <= kSnapVecPerLane * kSnapThreads
  const int64_t tail = head + 16 * nv;
  const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
  uint4* d4 = reinterpret_cast<uint4*>(dst + head);
  uint4 v[kSnapVecPerLane];
#pragma unroll
  for (int u = 0; u < kSnapVecPerLane; ++u) {
    const int64_t i = t + (int64_t)kSnapThreads * u;
    v[u] = i < nv ? s4[i] : uint4{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int u = 0; u < kSnapVecPerLane; ++u) {
    const int64_t i = t + (int64_t)kSnapThreads * u;
    if (i < nv) d4[i] = v[u];
  }
  if (t == 0 && head != 0) *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(src);
  if (t == 64 && tail < n) *reinterpret_cast<uint64_t*>(dst + tail) = *reinterpret_cast<const uint64_t*>(src + tail);
}

// Workgroup c owns bytes [c * kSnapChunk, (c + 1) * kSnapChunk) of the concatenated range: the segment that holds its
// first byte by bisection over `start`, then every segment that begins inside the chunk.
__global__ __launch_bounds__(kSnapThreads) void state_snapshot_k(const SnapSeg* __restrict__ seg, int nseg, int64_t total) {
  const int64_t c0 = (int64_t)blockIdx.x * kSnapChunk;
  if (c0 >= total) return;
  const int64_t c1 = c0 + kSnapChunk < total ? c0 + kSnapChunk : total;
  int lo = 0, hi = nseg - 1;                          // the last segment with start <= c0 (seg[0].start == 0)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid].start <= c0) lo = mid; else hi = mid - 1;
  }
  for (int i = lo; i < nseg; ++i) {
    const SnapSeg s = seg[i];
    if (s.start >= c1) break;
    const int64_t a = (c0 > s.start ? c0 : s.start) - s.start;                    // [a, b) of the segment, multiples of 8
    const int64_t e = s.start + s.bytes;
    const int64_t b = (c1 < e ? c1 : e) - s.start;
    if (b > a) snap_copy_piece(s.src + a, s.dst + a, b - a);
  }
}

void state_snapshot_copy(const SnapSeg* table, int nseg, int64_t total, hipStream_t s) {
  if (total <= 0 || nseg <= 0) return;
  const int64_t grid = cdiv(total, kSnapChunk);
  AO_REQUIRE(grid < ((int64_t)1 << 31), "internal: state snapshot of %lld bytes", (long long)total);
  state_snapshot_k<<<(unsigned)grid, kSnapThreads, 0, s>>>(table, nseg, total);
  AO_KERNEL_CHECK();
}

}  // namespace aoadmm
