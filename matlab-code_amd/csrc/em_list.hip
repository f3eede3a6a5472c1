// The list of a masked dense block's missing entries and the EM pass over it.  See em_list.h and DESIGN.md section 4.5.2.
#include "coo_team.h"
#include "em_list.h"

namespace aoadmm {

// ---------------------------------------------------------------------------
// the list: count per workgroup, scan, emit
// ---------------------------------------------------------------------------
// Thread w of the grid owns the 64-bit word w of the mask: entries [64 w, 64 w + 64) of the padded layout.
struct EmListBuildArgs {
  const uint64_t* bits;           // hipMalloc-aligned; em_mask_bits_bytes leaves room for the last word
  int64_t nbits, nwords;
  int64_t Ipad;
  int64_t dims[kCooMaxModes];
  int nd;
  int64_t* cnt;                   // [workgroups + 1]: zero bits per workgroup, after the scan their exclusive prefix and the total
  int* idx;
  int64_t n;
};

// the missing entries of word w as set bits; what lies past nbits is observed
__device__ __forceinline__ uint64_t em_list_word(const EmListBuildArgs& a, int64_t w) {
  if (w >= a.nwords) return 0;
  uint64_t z = ~a.bits[w];
  const int64_t left = a.nbits - 64 * w;
  if (left < 64) z &= ((uint64_t)1 << left) - 1;
  return z;
}

__global__ __launch_bounds__(256) void em_list_count_k(EmListBuildArgs a) {
  __shared__ int sh[256];
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  sh[threadIdx.x] = __popcll(em_list_word(a, w));
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.cnt[blockIdx.x] = sh[0];
}

// one workgroup: cnt[0 .. nb) -> exclusive prefix sums, cnt[nb] = total
__global__ __launch_bounds__(256) void em_list_scan_k(int64_t* cnt, int64_t nb) {
  __shared__ int64_t sh[256];
  const int64_t per = (nb + 255) / 256;
  const int64_t b0 = per * threadIdx.x, b1 = b0 + per < nb ? b0 + per : nb;
  int64_t s = 0;
  for (int64_t b = b0; b < b1; ++b) s += cnt[b];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int q = 0; q < 256; ++q) { const int64_t v = sh[q]; sh[q] = run; run += v; }
    cnt[nb] = run;
  }
  __syncthreads();
  int64_t run = sh[threadIdx.x];
  for (int64_t b = b0; b < b1; ++b) { const int64_t v = cnt[b]; cnt[b] = run; run += v; }
}

__global__ __launch_bounds__(256) void em_list_emit_k(EmListBuildArgs a) {
  __shared__ int sh[256];
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t z = em_list_word(a, w);
  // exclusive prefix of the words' counts inside the workgroup
  const int c = __popcll(z);
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t pos = a.cnt[blockIdx.x] + (sh[threadIdx.x] - c);
  while (z != 0 && pos < a.n) {
    const int64_t e = 64 * w + (__ffsll((unsigned long long)z) - 1);
    z &= z - 1;
    int64_t col = e / a.Ipad;
    a.idx[pos] = (int)(e - col * a.Ipad);
    for (int m = 1; m < a.nd; ++m) {
      const int64_t q = col / a.dims[m];
      a.idx[(int64_t)m * a.n + pos] = (int)(col - q * a.dims[m]);
      col = q;
    }
    ++pos;
  }
}

void em_list_build(MissingList& l, const uint8_t* bits, int nd, const int64_t* dims, int64_t Ipad, hipStream_t s) {
  AO_REQUIRE(nd >= 2 && nd <= kCooMaxModes && bits != nullptr, "internal: missing-entry list of order %d", nd);
  EmListBuildArgs a;
  a.bits = reinterpret_cast<const uint64_t*>(bits);
  a.nbits = Ipad;
  for (int m = 1; m < nd; ++m) a.nbits *= dims[m];
  a.nwords = cdiv(a.nbits, (int64_t)64);
  a.Ipad = Ipad; a.nd = nd;
  for (int m = 0; m < kCooMaxModes; ++m) {
    a.dims[m] = m < nd ? dims[m] : 1;
    AO_REQUIRE(a.dims[m] < ((int64_t)1 << 31), "mode %d too long for int32 subscripts", m);
  }
  const int64_t nb = cdiv(a.nwords, (int64_t)256);
  AO_REQUIRE(nb >= 1 && nb < ((int64_t)1 << 31), "internal: %lld workgroups for the missing-entry list", (long long)nb);
  DevBuf cnt;
  cnt.alloc((size_t)(nb + 1) * sizeof(int64_t));
  a.cnt = cnt.as<int64_t>(); a.idx = nullptr; a.n = 0;
  em_list_count_k<<<(unsigned)nb, 256, 0, s>>>(a);
  AO_KERNEL_CHECK();
  em_list_scan_k<<<1, 256, 0, s>>>(a.cnt, nb);
  AO_KERNEL_CHECK();
  int64_t n = 0;
  AO_HIP(hipMemcpyAsync(&n, a.cnt + nb, sizeof n, hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));
  AO_REQUIRE(n >= 0 && n <= a.nbits, "internal: %lld missing entries counted", (long long)n);
  MissingList fresh;
  fresh.on = true; fresh.nd = nd; fresh.n = n;
  if (n > 0) {
    fresh.idx.alloc((size_t)n * nd * sizeof(int));               // AOADMM_ERR_NOMEM leaves `l` as it was
    fresh.part.alloc((size_t)heldout_teams(n) * kEmListSums * sizeof(double));
    a.idx = fresh.idx.as<int>(); a.n = n;
    em_list_emit_k<<<(unsigned)nb, 256, 0, s>>>(a);
    AO_KERNEL_CHECK();
    AO_HIP(hipStreamSynchronize(s));                             // cnt is a local
  }
  l = std::move(fresh);
}

// ---------------------------------------------------------------------------
// the pass
// ---------------------------------------------------------------------------
constexpr int kEmListUnroll = 4;    // entries whose gathers are in flight together; one accumulator pair each

// The team layout of coo_team.h over the list.  ND = order (2..4 compiled in; 0: hf.nd at run time, up to kCooMaxModes);
// T = the block's precision.  Every lane of a team holds the same m, x_old and sums; lane 0 stores.
template <int G, int ND, typename T>
__global__ __launch_bounds__(256) void em_list_k(EmListArgs a) {
  const int R = a.hf.R;
  const CooTeam<G> t(a.n, R);
  if (t.idle()) return;
  const int64_t end = t.end();
  const int rr = t.rr();
  const bool live = t.live();
  constexpr int NMAX = ND > 0 ? ND : kCooMaxModes;
  const int nd = ND > 0 ? ND : a.hf.nd;
  T* __restrict__ X = static_cast<T*>(a.X);
  T* __restrict__ Xt = static_cast<T*>(a.Xt);
  double s_num[kEmListUnroll], s_den[kEmListUnroll];
#pragma unroll
  for (int u = 0; u < kEmListUnroll; ++u) s_num[u] = s_den[u] = 0.0;
  for (int64_t i0 = t.start; i0 < end; i0 += kEmListUnroll) {
    double mu[kEmListUnroll], xo[kEmListUnroll];
    int64_t off[kEmListUnroll], offt[kEmListUnroll];
#pragma unroll
    for (int u = 0; u < kEmListUnroll; ++u) {
      const int64_t i = i0 + u < end ? i0 + u : end - 1;   // clamped: every address is valid
      int sub[NMAX];
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < nd) sub[n] = a.idx[(int64_t)n * a.n + i];
      double fv[NMAX];
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < nd) fv[n] = coo_at(a.hf.f[n], sub[n], rr);
      int64_t o = sub[0];
#pragma unroll
      for (int n = 1; n < NMAX; ++n)
        if (n < nd) o += sub[n] * a.stride[n];
      off[u] = o;
      if (ND == 2) offt[u] = sub[1] + a.Jpad * sub[0];
      xo[u] = (double)X[o];
      double m = 1.0;
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < nd) m *= fv[n];
      mu[u] = live ? m : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kEmListUnroll; ++u) mu[u] = team_sum<G>(mu[u]);
#pragma unroll
    for (int u = 0; u < kEmListUnroll; ++u) {
      if (i0 + u < end) {
        const double d = mu[u] - xo[u];
        s_num[u] += d * d; s_den[u] += xo[u] * xo[u];
        if (a.update && t.r == 0) {
          X[off[u]] = (T)mu[u];
          if (ND == 2) Xt[offt[u]] = (T)mu[u];
        }
      }
    }
  }
  if (t.r == 0) {
    a.part[kEmListSums * t.team + 0] = (s_num[0] + s_num[1]) + (s_num[2] + s_num[3]);
    a.part[kEmListSums * t.team + 1] = (s_den[0] + s_den[1]) + (s_den[2] + s_den[3]);
  }
}
static_assert(kEmListUnroll == 4, "em_list_k adds its four accumulators pairwise");

// One workgroup: the teams' partials in a fixed strided order, then the fixed tree of coo_block_sum
__global__ __launch_bounds__(256) void em_list_finish_k(const double* part, int64_t nteams, double* num, double* den) {
  __shared__ double sh[256];
  double p[kEmListSums] = {0.0, 0.0};
  for (int64_t t = threadIdx.x; t < nteams; t += 256)
    for (int k = 0; k < kEmListSums; ++k) p[k] += part[kEmListSums * t + k];
  const double vn = coo_block_sum(p[0], sh);
  const double vd = coo_block_sum(p[1], sh);
  if (threadIdx.x == 0) { *num = vn; *den = vd; }
}

template <typename T>
static void launch(const EmListArgs& a, hipStream_t s) {
  for_team_width(a.hf.R, [&](auto g) {
    constexpr int G = decltype(g)::value;
    const unsigned grid = coo_team_grid(a.n, G);
    for_order<2>(a.hf.nd, [&](auto nd) { em_list_k<G, decltype(nd)::value, T><<<grid, 256, 0, s>>>(a); });
  });
  AO_KERNEL_CHECK();
}

void em_list_pass(const EmListArgs& a, int prec, double* num, double* den, hipStream_t s) {
  const int R = a.hf.R;
  AO_REQUIRE(R >= 1 && R <= kMaxRank && a.hf.nd >= 2 && a.hf.nd <= kCooMaxModes && a.n >= 0 && a.hf.off == nullptr,
             "internal: list pass of rank %d, order %d", R, a.hf.nd);
  AO_REQUIRE(prec == AOADMM_PREC_F32 || prec == AOADMM_PREC_F64, "internal: list pass of precision id %d", prec);
  AO_REQUIRE((a.hf.nd == 2) == (a.Xt != nullptr), "internal: list pass of order %d %s a transposed copy", a.hf.nd, a.Xt ? "with" : "without");
  if (a.n == 0) {                                     // nothing missing: two zeros, no launch
    AO_HIP(hipMemsetAsync(num, 0, sizeof(double), s));
    AO_HIP(hipMemsetAsync(den, 0, sizeof(double), s));
    return;
  }
  if (prec == AOADMM_PREC_F32) launch<float>(a, s);
  else launch<double>(a, s);
  em_list_finish_k<<<1, 256, 0, s>>>(a.part, heldout_teams(a.n), num, den);
  AO_KERNEL_CHECK();
}

double em_list_pass_bytes(int nd, int R, int64_t n, int prec, bool update) {
  const double es = prec == AOADMM_PREC_F32 ? 4.0 : 8.0;
  const double listed = heldout_pass_bytes(nd, R, n, true) - 8.0 * (double)n;   // subscripts streamed, factor rows gathered
  return listed + es * (double)n + (update ? es * (double)n * (nd == 2 ? 2.0 : 1.0) : 0.0);   // x_old read; m written (a matrix: twice)
}

double em_list_pass_flops(int nd, int R, int64_t n) { return heldout_pass_flops(nd, R, n, true); }

}  // namespace aoadmm
