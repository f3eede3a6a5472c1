// Probe: the state snapshot (matlab-code_amd/csrc/state_snapshot.hip, one launch over a table of segments) against a chain
// of hipMemcpyAsync, one per state array, on the arrays of a small coupled CP + PARAFAC2 model (the shapes of
// example_script1: CP 20 x 30 x 40, PARAFAC2 I = 20, K = 20, J_k = 30, R = 3, 22 state arrays, 64 KB) and on one large
// array list (the factors of a 1e6 x 1e5 x 1e4 model at R = 20, 178 MB).
// Per form: the host time to enqueue, and the wall time from the first enqueue to the end of a stream synchronise, each
// the median (min, max) of `reps` alternating repetitions.  One JSON line per list.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../matlab-code_amd/csrc snapshot_vs_memcpy.hip \
//         ../../matlab-code_amd/csrc/state_snapshot.hip -o snapshot_vs_memcpy
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "state_snapshot.h"

using namespace aoadmm;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s -> %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); return 1; } } while (0)

static double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static void mmm(std::vector<double> v, double out[3]) {
  std::sort(v.begin(), v.end());
  out[0] = v[v.size() / 2]; out[1] = v.front(); out[2] = v.back();
}

static int run(const char* name, const std::vector<int64_t>& doubles, int reps) {
  const int n = (int)doubles.size();
  hipStream_t s;
  CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  std::vector<char*> src(n);
  std::vector<SnapSeg> segs(n);
  int64_t start = 0, cursor = 0;
  std::vector<int64_t> slot(n);
  for (int i = 0; i < n; ++i) {                       // every array its own allocation, as the engine's DevBufs are
    CK(hipMalloc(&src[i], (size_t)doubles[i] * 8));
    CK(hipMemset(src[i], i + 1, (size_t)doubles[i] * 8));
    slot[i] = snapshot_slot_offset(cursor, src[i]);
    cursor = slot[i] + doubles[i] * 8;
  }
  char* store = nullptr;
  CK(hipMalloc(&store, (size_t)cursor));
  for (int i = 0; i < n; ++i) {
    segs[i] = SnapSeg{src[i], store + slot[i], doubles[i] * 8, start};
    start += doubles[i] * 8;
  }
  SnapSeg* table = nullptr;
  CK(hipMalloc(&table, sizeof(SnapSeg) * n));
  CK(hipMemcpy(table, segs.data(), sizeof(SnapSeg) * n, hipMemcpyHostToDevice));
  std::vector<double> enq[2], wall[2];
  for (int rep = -3; rep < reps; ++rep) {             // three warm-up rounds
    for (int form = 0; form < 2; ++form) {
      CK(hipStreamSynchronize(s));
      const double t0 = now_us();
      if (form == 0) {
        state_snapshot_copy(table, n, start, s);
      } else {
        for (int i = 0; i < n; ++i) CK(hipMemcpyAsync(segs[i].dst, segs[i].src, (size_t)segs[i].bytes, hipMemcpyDeviceToDevice, s));
      }
      const double t1 = now_us();
      CK(hipStreamSynchronize(s));
      const double t2 = now_us();
      if (rep >= 0) { enq[form].push_back(t1 - t0); wall[form].push_back(t2 - t0); }
    }
  }
  // the two forms must have written the same bytes: compare the store with the sources once
  std::vector<char> h((size_t)cursor);
  CK(hipMemcpy(h.data(), store, (size_t)cursor, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
    for (int64_t k = 0; k < doubles[i] * 8; k += 4097)
      if (h[slot[i] + k] != (char)(i + 1)) { printf("array %d differs at byte %lld\n", i, (long long)k); return 1; }
  double a[3], b[3], c[3], d[3];
  mmm(enq[0], a); mmm(wall[0], b); mmm(enq[1], c); mmm(wall[1], d);
  printf("{\"what\": \"snapshot_vs_memcpy\", \"list\": \"%s\", \"arrays\": %d, \"state_bytes\": %lld, \"reps\": %d, "
         "\"one_launch_enqueue_us\": [%.2f, %.2f, %.2f], \"one_launch_wall_us\": [%.2f, %.2f, %.2f], "
         "\"memcpy_chain_enqueue_us\": [%.2f, %.2f, %.2f], \"memcpy_chain_wall_us\": [%.2f, %.2f, %.2f]}\n",
         name, n, (long long)start, reps, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], d[0], d[1], d[2]);
  for (int i = 0; i < n; ++i) CK(hipFree(src[i]));
  CK(hipFree(store)); CK(hipFree(table)); CK(hipStreamDestroy(s));
  return 0;
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::max(7, atoi(argv[1])) : 101;
  // example_script1: fac (6), constraint_fac and constraint_dual_fac of modes 1, 2, 3, 4, 6 (10), coupling_fac (1),
  // coupling_dual_fac (2), DeltaB, P, mu_DeltaB (3)
  const std::vector<int64_t> small = {60, 90, 120, 60, 1800, 60, 60, 90, 120, 60, 60, 60, 90, 120, 60, 60,
                                      60, 60, 60, 9, 1800, 1800};
  const std::vector<int64_t> large = {20000000, 2000000, 200000};
  try {
    if (run("script1", small, reps)) return 1;
    if (run("sparse-1e6x1e5x1e4-R20", large, std::min(reps, 21))) return 1;
  } catch (const Error& e) { printf("error: %s\n", e.what()); return 1; }
  return 0;
}
