// Sparse (COO) CP blocks: upload (device radix sort, duplicate coalescing, one sorted copy per mode) and the MTTKRP
// (mttkrp_coo_k + coo_carry_k).  See sparse.h and DESIGN.md section 9.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>

#include "coo_team.h"

namespace aoadmm {

// ---------------------------------------------------------------------------
// upload
// ---------------------------------------------------------------------------
// key[i] = column-major linear index of nonzero perm[i] over modes [m0, m1) (product of their sizes < 2^64)
__global__ void coo_key_k(uint64_t* key, const int* perm, const int* idx, int64_t nnz, int m0, int m1,
                          const int64_t* stride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const int64_t q = perm[i];
  uint64_t k = 0;
  for (int m = m0; m < m1; ++m) k += (uint64_t)idx[m * nnz + q] * (uint64_t)stride[m];
  key[i] = k;
}

__global__ void iota_k(int* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (int)i;
}

// head[i] = 1 where sorted nonzero i starts a new subscript (the first of a run of duplicates)
__global__ void coo_head_k(int* head, const int* perm, const int* idx, int64_t nnz, int nd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  int h = i == 0;
  if (!h) {
    const int64_t q = perm[i], qp = perm[i - 1];
    for (int m = 0; m < nd; ++m) h |= idx[m * nnz + q] != idx[m * nnz + qp];
  }
  head[i] = h;
}

// values in sorted order (vs), the 0-based run of every nonzero (seg, in place: the inclusive scan of the head flags
// minus one) and, for the first nonzero of every run of duplicates, the run's subscript (cidx).  The runs are then
// summed by the carry passes of the MTTKRP (coo_build).
__global__ void coo_runs_k(int* cidx, double* vs, int64_t nc, const int* head, int* seg, const int* perm,
                           const int* idx, const double* val, int64_t nnz, int nd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const int64_t q = perm[i];
  vs[i] = val[q];
  const int s = seg[i] - 1;
  seg[i] = s;
  if (!head[i]) return;
  for (int m = 0; m < nd; ++m) cidx[m * nc + s] = idx[m * nnz + q];
}

static void carry_passes(const int* rin, const double* vin, int64_t n, int R, double scale, double* out, int64_t oI,
                         int64_t oR, DevBuf* srow, DevBuf* sval, int next, hipStream_t s);

// the copy of mode n: other modes' indices and values in the order of perm (row indices are the sort's keys)
__global__ void coo_gather_k(int* oidx, double* oval, const int* perm, const int* cidx, const double* cval, int64_t nc,
                             int nd, int n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const int64_t q = perm[i];
  int k = 0;
  for (int m = 0; m < nd; ++m) {
    if (m == n) continue;
    oidx[k * nc + i] = cidx[m * nc + q];
    ++k;
  }
  oval[i] = cval[q];
}

static int bits_for(uint64_t count) {       // bits of the largest key count - 1
  int b = 0;
  while (b < 64 && (count - 1) >> b) ++b;
  return std::max(b, 1);
}

template <class K>
static void radix_sort(DevBuf& tmp, const K* kin, K* kout, const int* vin, int* vout, int64_t n, int bits,
                       hipStream_t s) {
  size_t need = 0;
  AO_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, kin, kout, vin, vout, (int)n, 0, bits, s));
  tmp.ensure(need);
  AO_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, need, kin, kout, vin, vout, (int)n, 0, bits, s));
}

void coo_sort_linear(CooSortWork& w, const int* idx, int64_t nnz, int nd, const int64_t* dims, hipStream_t s) {
  w.permA.alloc((size_t)nnz * sizeof(int)); w.permB.alloc((size_t)nnz * sizeof(int));
  w.keyA.alloc((size_t)nnz * sizeof(uint64_t)); w.keyB.alloc((size_t)nnz * sizeof(uint64_t));
  iota_k<<<blocks_for(nnz), 256, 0, s>>>(w.permA.as<int>(), nnz);
  AO_KERNEL_CHECK();
  // Column-major linear order by stable LSD radix sorts over groups of consecutive modes whose linear index fits in
  // 64 bits (one group, i.e. one 64-bit sort, unless the product of the sizes reaches 2^64)
  std::vector<int64_t> hstride(nd, 1);
  std::vector<std::pair<int, int>> groups;
  for (int m0 = 0; m0 < nd;) {
    uint64_t prod = 1;
    int m1 = m0;
    while (m1 < nd && prod <= UINT64_MAX / (uint64_t)dims[m1]) { hstride[m1] = (int64_t)prod; prod *= (uint64_t)dims[m1]; ++m1; }
    groups.emplace_back(m0, m1);
    m0 = m1;
  }
  w.stride.alloc(nd * sizeof(int64_t));
  AO_HIP(hipMemcpyAsync(w.stride.p, hstride.data(), nd * sizeof(int64_t), hipMemcpyHostToDevice, s));
  for (const auto& g : groups) {
    uint64_t prod = 1;
    for (int m = g.first; m < g.second; ++m) prod *= (uint64_t)dims[m];
    if (prod <= 1) continue;
    coo_key_k<<<blocks_for(nnz), 256, 0, s>>>(w.keyA.as<uint64_t>(), w.permA.as<int>(), idx, nnz, g.first, g.second,
                                              w.stride.as<int64_t>());
    AO_KERNEL_CHECK();
    radix_sort<uint64_t>(w.tmp, w.keyA.as<uint64_t>(), w.keyB.as<uint64_t>(), w.permA.as<int>(), w.permB.as<int>(), nnz,
                         bits_for(prod), s);
    std::swap(w.permA, w.permB);
  }
  AO_HIP(hipStreamSynchronize(s));                   // hstride is a local
}

int64_t coo_runs_scan(CooSortWork& w, DevBuf& head, DevBuf& seg, const int* idx, int64_t nnz, int nd, hipStream_t s) {
  head.alloc((size_t)nnz * sizeof(int)); seg.alloc((size_t)nnz * sizeof(int));
  coo_head_k<<<blocks_for(nnz), 256, 0, s>>>(head.as<int>(), w.permA.as<int>(), idx, nnz, nd);
  AO_KERNEL_CHECK();
  {
    size_t need = 0;
    AO_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, need, head.as<int>(), seg.as<int>(), (int)nnz, s));
    w.tmp.ensure(need);
    AO_HIP(hipcub::DeviceScan::InclusiveSum(w.tmp.p, need, head.as<int>(), seg.as<int>(), (int)nnz, s));
  }
  int nc32 = 0;
  AO_HIP(hipMemcpyAsync(&nc32, seg.as<int>() + nnz - 1, sizeof(int), hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));
  return nc32;
}

void coo_build(CooBlock& b, int nd, const int64_t* dims, int64_t nnz, const int64_t* subs, const double* vals,
               hipStream_t s) {
  AO_REQUIRE(nd >= 2 && nd <= kCooMaxModes, "sparse block: order %d unsupported (2..%d)", nd, kCooMaxModes);
  AO_REQUIRE(nnz >= 0, "sparse block: nnz = %lld < 0", (long long)nnz);
  AO_REQUIRE(nnz < (int64_t)INT32_MAX, "sparse block: %lld nonzeros, at most 2^31 - 2 per block", (long long)nnz);
  AO_REQUIRE(nnz == 0 || (subs != nullptr && vals != nullptr), "sparse block: null subs / vals");
  for (int m = 0; m < nd; ++m)
    AO_REQUIRE(dims[m] >= 1 && dims[m] < ((int64_t)1 << 31), "sparse block: mode %d has %lld rows (1 .. 2^31 - 1)", m,
               (long long)dims[m]);
  // subscripts: range check and int32 on the host (the column-major nnz x nd array is already one array per mode)
  std::vector<int> hidx((size_t)nd * nnz);
  for (int m = 0; m < nd; ++m) {
    const int64_t* sm = subs + (size_t)m * nnz;
    int* dm = hidx.data() + (size_t)m * nnz;
    const int64_t lim = dims[m];
    for (int64_t i = 0; i < nnz; ++i) {
      const int64_t v = sm[i];
      if (v < 0 || v >= lim)
        throw Error(AOADMM_ERR_INVALID, fmt("sparse block: subscript %lld of nonzero %lld in mode %d is outside [0, %lld)",
                                            (long long)v, (long long)i, m, (long long)lim));
      dm[i] = (int)v;
    }
  }
  CooBlock nb;
  nb.nd = nd;
  for (int m = 0; m < nd; ++m) nb.dims[m] = dims[m];
  if (nnz == 0) {
    nb.nnz = nb.nnz_full = 0;
    b = std::move(nb);
    return;
  }
  DevBuf idx, val, head, seg;
  CooSortWork w;
  DevBuf &permA = w.permA, &permB = w.permB, &keyA = w.keyA, &keyB = w.keyB, &tmp = w.tmp;
  idx.alloc(hidx.size() * sizeof(int));
  val.alloc((size_t)nnz * sizeof(double));
  AO_HIP(hipMemcpyAsync(idx.p, hidx.data(), hidx.size() * sizeof(int), hipMemcpyHostToDevice, s));
  AO_HIP(hipMemcpyAsync(val.p, vals, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, s));
  coo_sort_linear(w, idx.as<int>(), nnz, nd, dims, s);
  // duplicates: runs of equal subscripts in the sorted order
  const int nc32 = (int)coo_runs_scan(w, head, seg, idx.as<int>(), nnz, nd, s);
  const int64_t nc = nc32;
  DevBuf cidx, cval, crow[2], cvals[2];
  cidx.alloc((size_t)nd * nc * sizeof(int));
  cval.alloc((size_t)nc * sizeof(double));
  double* vs = keyB.as<double>();                    // the sort keys are spent: 8 bytes per nonzero for the sorted values
  coo_runs_k<<<blocks_for(nnz), 256, 0, s>>>(cidx.as<int>(), vs, nc, head.as<int>(), seg.as<int>(), permA.as<int>(),
                                             idx.as<int>(), val.d(), nnz, nd);
  AO_KERNEL_CHECK();
  // duplicates summed per run with the MTTKRP's carry passes (a list sorted by run id, one value per entry): chunks of
  // 256 entries per team, chunk-boundary partials added level by level in chunk order -- bitwise reproducible, and no
  // thread walks a long run alone however many copies of one subscript the input holds
  carry_passes(seg.as<int>(), vs, nnz, 1, 1.0, cval.d(), 1, nc, crow, cvals, 0, s);
  idx.release(); val.release(); keyA.release(); keyB.release(); head.release(); seg.release();
  nb.nnz = nb.nnz_full = nc;
  // one copy per mode, stably sorted by that mode's index (32-bit keys)
  iota_k<<<blocks_for(nc), 256, 0, s>>>(permA.as<int>(), nc);
  AO_KERNEL_CHECK();
  for (int n = 0; n < nd; ++n) {
    CooMode& cm = nb.mode[n];
    cm.row.alloc((size_t)nc * sizeof(int));
    cm.oidx.alloc((size_t)(nd - 1) * nc * sizeof(int));
    cm.val.alloc((size_t)nc * sizeof(double));
    radix_sort<unsigned>(tmp, reinterpret_cast<const unsigned*>(cidx.as<int>() + (size_t)n * nc), cm.row.as<unsigned>(),
                         permA.as<int>(), permB.as<int>(), nc, bits_for((uint64_t)dims[n]), s);
    coo_gather_k<<<blocks_for(nc), 256, 0, s>>>(cm.oidx.as<int>(), cm.val.d(), permB.as<int>(), cidx.as<int>(), cval.d(), nc,
                                                nd, n);
    AO_KERNEL_CHECK();
  }
  AO_HIP(hipStreamSynchronize(s));                   // the locals above are freed on return
  b = std::move(nb);
}

void coo_keep_share(CooBlock& b, int rank, int world, hipStream_t s) {
  AO_REQUIRE(world >= 1 && rank >= 0 && rank < world, "sparse block: bad rank/world %d/%d", rank, world);
  AO_REQUIRE(!b.sharded && b.nnz == b.nnz_full, "internal: coo_keep_share on a block that was cut before");
  const int64_t full = b.nnz_full;
  const int64_t lo = coo_share_begin(full, rank, world), hi = coo_share_begin(full, rank + 1, world), cnt = hi - lo;
  const int no = b.nd - 1;
  for (int n = 0; n < b.nd; ++n) {
    CooMode& cm = b.mode[n];
    CooMode keep;                                      // stays without buffers for an empty share
    b.span0[n] = b.span1[n] = -1;
    if (cnt > 0) {
      keep.row.alloc((size_t)cnt * sizeof(int));
      keep.oidx.alloc((size_t)no * cnt * sizeof(int));
      keep.val.alloc((size_t)cnt * sizeof(double));
      AO_HIP(hipMemcpyAsync(keep.row.p, cm.row.as<int>() + lo, (size_t)cnt * sizeof(int), hipMemcpyDeviceToDevice, s));
      for (int k = 0; k < no; ++k)
        AO_HIP(hipMemcpyAsync(keep.oidx.as<int>() + (size_t)k * cnt, cm.oidx.as<int>() + (size_t)k * full + lo,
                              (size_t)cnt * sizeof(int), hipMemcpyDeviceToDevice, s));
      AO_HIP(hipMemcpyAsync(keep.val.p, cm.val.d() + lo, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, s));
      int ends[2] = {-1, -1};
      AO_HIP(hipMemcpyAsync(&ends[0], cm.row.as<int>() + lo, sizeof(int), hipMemcpyDeviceToHost, s));
      AO_HIP(hipMemcpyAsync(&ends[1], cm.row.as<int>() + hi - 1, sizeof(int), hipMemcpyDeviceToHost, s));
      AO_HIP(hipStreamSynchronize(s));                 // the copies are done before the full arrays go
      AO_REQUIRE(ends[0] >= 0 && ends[0] <= ends[1] && ends[1] < b.dims[n], "internal: mode %d of a sparse block is not sorted by row", n);
      b.span0[n] = ends[0]; b.span1[n] = ends[1];
    }
    cm = std::move(keep);                              // frees this mode's full copy
  }
  for (int i = 0; i < 2; ++i) { b.slot_row[i].release(); b.slot_val[i].release(); }   // sized for the full list by the build
  b.nnz = cnt;
  b.sharded = true; b.cut_rank = rank; b.cut_world = world;
}

// ---------------------------------------------------------------------------
// MTTKRP
// ---------------------------------------------------------------------------
// A team (coo_team.h; lane r = column r of the result) walks its range of a list of entries sorted by row and keeps
// the running sum of the current row in a register.  A row that starts and ends inside the team's range is
// complete: one plain store.  A row that continues into the previous or the next range goes to one of the team's two
// carry slots (2 t: its first row, 2 t + 1: its last row); a row that runs through the whole range fills both, the
// second with +0.  Unused slots hold row -1, which only ever sits between two different rows, so the slots of one row
// are consecutive and the next pass (coo_carry_k) sums them in chunk order the same way.
struct SegAcc {
  const int* rows;   // row of every entry of the list (neighbour test at the range ends)
  int64_t n, start, end, team;
  int r, R;
  double scale;
  double* out;
  int64_t oI, oR;    // element (row, r) of the result at out[row * oI + r * oR]
  int* slot_row;
  double* slot_val;
  int cur = -1;
  double acc = 0.0;
  bool first = true, usedL = false, usedR = false;

  __device__ void flush(bool last) {
    const bool cl = first && start > 0 && rows[start - 1] == cur;
    const bool cr = last && end < n && rows[end] == cur;
    if (!cl && !cr) {
      if (r < R) out[cur * oI + oR * r] = scale * acc;
    } else {
      const int64_t sl = 2 * team + (cl ? 0 : 1);
      if (r < R) slot_val[sl * R + r] = acc;
      if (r == 0) slot_row[sl] = cur;
      if (cl) usedL = true; else usedR = true;
      if (cl && cr) {
        if (r < R) slot_val[(sl + 1) * R + r] = 0.0;
        if (r == 0) slot_row[sl + 1] = cur;
        usedR = true;
      }
    }
    first = false;
  }
  __device__ void add(int row, double v) {
    if (row != cur) {
      if (cur >= 0) flush(false);
      cur = row;
      acc = 0.0;
    }
    acc += v;
  }
  __device__ void finish() {
    if (cur >= 0) flush(true);
    if (slot_row && r == 0) {
      if (!usedL) slot_row[2 * team] = -1;
      if (!usedR) slot_row[2 * team + 1] = -1;
    }
  }
};

struct CooArgs {
  const int* row;
  const int* oidx;
  const double* val;
  int64_t nnz;
  CooFactor f[kCooMaxModes - 1];
  int no;
  int R;
  double scale;
  double* out;
  int64_t oI, oR;
  int* slot_row;
  double* slot_val;
};

constexpr int kCooUnroll = 8;    // entries whose loads are in flight together

// NO = number of other modes (1..3 compiled in; 0: a.no at run time, up to 7)
template <int G, int NO>
__global__ __launch_bounds__(256) void mttkrp_coo_k(CooArgs a) {
  const CooTeam<G> t(a.nnz, a.R);
  if (t.idle()) return;
  const int64_t end = t.end();
  const int rr = t.rr();
  const int no = NO > 0 ? NO : a.no;
  SegAcc sa{a.row, a.nnz, t.start, end, t.team, t.r, a.R, a.scale, a.out, a.oI, a.oR, a.slot_row, a.slot_val};
  for (int64_t i0 = t.start; i0 < end; i0 += kCooUnroll) {
    int rowu[kCooUnroll];
    double pu[kCooUnroll];
#pragma unroll
    for (int u = 0; u < kCooUnroll; ++u) {
      const int64_t i = i0 + u < end ? i0 + u : end - 1;
      rowu[u] = a.row[i];
      double p = a.val[i];
      if (NO > 0) {
#pragma unroll
        for (int k = 0; k < (NO > 0 ? NO : 1); ++k)
          p *= coo_at(a.f[k], a.oidx[k * a.nnz + i], rr);
      } else {
        for (int k = 0; k < no; ++k) p *= coo_at(a.f[k], a.oidx[k * a.nnz + i], rr);
      }
      pu[u] = p;
    }
#pragma unroll
    for (int u = 0; u < kCooUnroll; ++u)
      if (i0 + u < end) sa.add(rowu[u], pu[u]);
  }
  sa.finish();
}

// one level of the carry sum: the slots of the level below (rows rin, R-vectors vin, n of them) in chunks of
// kCooChunk per team, same rules; rout / vout receive this level's slots (null when one team covers the list)
template <int G>
__global__ __launch_bounds__(256) void coo_carry_k(const int* rin, const double* vin, int64_t n, int R, double scale,
                                                   double* out, int64_t oI, int64_t oR, int* rout, double* vout) {
  const CooTeam<G> t(n, R);
  if (t.idle()) return;
  const int64_t end = t.end();
  const int rr = t.rr();
  SegAcc sa{rin, n, t.start, end, t.team, t.r, R, scale, out, oI, oR, rout, vout};
  for (int64_t i0 = t.start; i0 < end; i0 += kCooUnroll) {
    int rowu[kCooUnroll];
    double vu[kCooUnroll];
#pragma unroll
    for (int u = 0; u < kCooUnroll; ++u) {
      const int64_t i = i0 + u < end ? i0 + u : end - 1;
      rowu[u] = rin[i];
      vu[u] = vin[i * R + rr];
    }
#pragma unroll
    for (int u = 0; u < kCooUnroll; ++u)
      if (i0 + u < end && rowu[u] >= 0) sa.add(rowu[u], vu[u]);
  }
  sa.finish();
}

// Sums a list sorted by row (rows rin, R-vectors vin, n entries; row -1 = empty) into out, level by level until one team
// covers the list (a level shrinks the list kCooChunk / 2 = 128 times).  Level outputs alternate between srow/sval[next]
// and [next ^ 1], never the buffer the level reads.
static void carry_passes(const int* rin, const double* vin, int64_t n, int R, double scale, double* out, int64_t oI,
                         int64_t oR, DevBuf* srow, DevBuf* sval, int next, hipStream_t s) {
  for (;;) {
    const int64_t teams = cdiv(n, kCooChunk);
    int* rout = nullptr;
    double* vout = nullptr;
    if (teams > 1) {
      srow[next].ensure((size_t)2 * teams * sizeof(int));
      sval[next].ensure((size_t)2 * teams * R * sizeof(double));
      rout = srow[next].as<int>();
      vout = sval[next].d();
    }
    for_team_width(R, [&](auto g) {
      constexpr int G = decltype(g)::value;
      coo_carry_k<G><<<coo_team_grid(n, G), 256, 0, s>>>(rin, vin, n, R, scale, out, oI, oR, rout, vout);
    });
    AO_KERNEL_CHECK();
    if (teams <= 1) break;
    rin = rout; vin = vout; n = 2 * teams;
    next ^= 1;
  }
}

// the team kernel and the carry levels over one list sorted by a.row; `out` has been cleared by the caller
static void run_list(CooArgs a, DevBuf* slot_row, DevBuf* slot_val, hipStream_t s) {
  const int R = a.R;
  const int64_t nteams = cdiv(a.nnz, kCooChunk);
  // level-0 slots: two per team (carry_passes sizes the later levels)
  if (nteams > 1) {
    const size_t n0 = (size_t)2 * nteams;
    slot_row[0].ensure(n0 * sizeof(int)); slot_val[0].ensure(n0 * R * sizeof(double));
  }
  a.slot_row = nteams > 1 ? slot_row[0].as<int>() : nullptr;
  a.slot_val = nteams > 1 ? slot_val[0].d() : nullptr;
  for_team_width(R, [&](auto g) {
    for_order<1>(a.no, [&](auto no) {                // the other modes: 1..3 compiled in
      constexpr int G = decltype(g)::value;
      mttkrp_coo_k<G, decltype(no)::value><<<coo_team_grid(a.nnz, G), 256, 0, s>>>(a);
    });
  });
  AO_KERNEL_CHECK();
  if (nteams > 1)
    carry_passes(slot_row[0].as<int>(), slot_val[0].d(), 2 * nteams, R, a.scale, a.out, a.oI, a.oR, slot_row, slot_val, 1, s);
}

void coo_mttkrp(CooBlock& b, int pos, const CooFactor* f, int R, double scale, double* out, int64_t ldOut,
                hipStream_t s, bool span_only, const double* vals) {
  AO_REQUIRE(pos >= 0 && pos < b.nd, "sparse mttkrp: mode %d out of range", pos);
  AO_REQUIRE(R >= 1 && R <= kMaxRank, "sparse mttkrp: rank %d outside 1..%d", R, kMaxRank);
  const int64_t rows = b.dims[pos];
  AO_REQUIRE(ldOut >= rows, "sparse mttkrp: ldOut %lld < %lld rows", (long long)ldOut, (long long)rows);
  AO_REQUIRE(!span_only || b.sharded, "internal: span form of the sparse mttkrp on a block that is not sharded");
  if (span_only && b.nnz == 0) return;
  // rows without nonzeros are exact zeros; every other row is stored exactly once below (every entry of a share has
  // its row inside the share's span)
  const int64_t r0 = span_only ? b.span0[pos] : 0, nr = span_only ? b.span1[pos] - b.span0[pos] + 1 : rows;
  AO_REQUIRE(r0 >= 0 && nr >= 1 && r0 + nr <= rows, "internal: span [%lld, %lld] of mode %d outside its %lld rows", (long long)r0,
             (long long)(r0 + nr - 1), pos, (long long)rows);
  AO_HIP(hipMemset2DAsync(out + r0, (size_t)ldOut * sizeof(double), 0, (size_t)nr * sizeof(double), (size_t)R, s));
  if (b.nnz == 0) return;
  const CooMode& cm = b.mode[pos];
  CooArgs a;
  a.row = cm.row.as<int>(); a.oidx = cm.oidx.as<int>(); a.val = vals ? vals : cm.val.d(); a.nnz = b.nnz;
  a.no = b.nd - 1;
  for (int k = 0; k < a.no; ++k) a.f[k] = f[k];
  a.R = R; a.scale = scale; a.out = out; a.oI = 1; a.oR = ldOut;
  run_list(a, b.slot_row, b.slot_val, s);
}

void coo_list_pass(const CooList& l, const double* src, int R, double* out, DevBuf* slot_row, DevBuf* slot_val,
                   hipStream_t s) {
  AO_REQUIRE(R >= 1 && R <= kMaxRank, "sparse list pass: width %d outside 1..%d", R, kMaxRank);
  AO_REQUIRE(l.n >= 1 && l.rows >= 1, "sparse list pass: empty list");
  AO_HIP(hipMemsetAsync(out, 0, (size_t)l.rows * R * sizeof(double), s));
  CooArgs a;
  a.row = l.key; a.oidx = l.gidx; a.val = l.val; a.nnz = l.n;
  a.no = 1;
  a.f[0] = CooFactor{src, (int64_t)R, 1};
  a.R = R; a.scale = 1.0; a.out = out; a.oI = R; a.oR = 1;
  run_list(a, slot_row, slot_val, s);
}

double coo_mttkrp_bytes(const CooBlock& b, int pos, int R) {
  const double nz = (double)b.nnz, no = (double)(b.nd - 1);
  const double rows = !b.sharded ? (double)b.dims[pos] : b.nnz == 0 ? 0.0 : (double)(b.span1[pos] - b.span0[pos] + 1);
  return nz * (4.0 + 4.0 * no + 8.0) + nz * no * R * 8.0 + rows * R * 8.0;
}

double coo_mttkrp_flops(const CooBlock& b, int R) { return (double)b.nnz * R * b.nd; }

}  // namespace aoadmm
