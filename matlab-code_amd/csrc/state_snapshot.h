// Snapshot of the solver state: every array of the struct G copied into one kept buffer by ONE launch, and back by one
// more (aoadmm_heldout_keep_best / aoadmm_heldout_restore_best).  A model of the small
// configurations has 15-20 state arrays of a few kilobytes each; at ~5 us per launch or hipMemcpyAsync a chain of copies
// would cost more than the outer iteration's own kernels, so the arrays are described by a table of segments in device
// memory and workgroups take fixed-size chunks of the concatenated byte range.
// Plain loads and stores, no atomics, no dependence between workgroups: every byte has exactly one writer.
#pragma once
#include "common.h"

namespace aoadmm {

// One array: `bytes` (a multiple of 8: the state is fp64) from src to dst; `start` is the array's offset in the
// concatenated range (the prefix sum of the bytes before it).  src and dst are 8-byte aligned and congruent modulo 16,
// so that one 8-byte head brings both onto a 16-byte boundary (snapshot_slot_offset lays the kept buffer out that way).
struct SnapSeg {
  const char* src;
  char* dst;
  int64_t bytes;
  int64_t start;
};

constexpr int64_t kSnapChunk = 16384;   // bytes of the concatenated range per workgroup: 256 lanes x 4 x 16 bytes

// Offset of an array's slot in the kept buffer, at or after `cursor`: congruent to `src` modulo 16.
inline int64_t snapshot_slot_offset(int64_t cursor, const void* src) {
  const int64_t at = round_up(cursor, 16);
  return at + (int64_t)(reinterpret_cast<uintptr_t>(src) & 15);
}

// Copies the nseg segments of `table` (device memory; `start` ascending, no empty segment, `total` = the sum of their
// bytes) with one launch of cdiv(total, kSnapChunk) workgroups.  Nothing is launched when total == 0.
void state_snapshot_copy(const SnapSeg* table, int nseg, int64_t total, hipStream_t s);

}  // namespace aoadmm
