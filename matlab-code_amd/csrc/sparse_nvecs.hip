// nvecs initialisation of sparse blocks by block subspace iteration -- see sparse_nvecs.h and DESIGN.md section 9.2.
// The passes over the nonzeros are coo_list_pass (sparse.hip); the kernels here are the dense pieces on the tall
// row-major n x b matrices (V, Y: I_n x b; W: F x b; b <= 64 doubles per row) and the b x b matrices between them.
#include "sparse_nvecs.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "device_utils.h"
#include "small.h"

namespace aoadmm {

// ---------------------------------------------------------------------------
// fiber lists
// ---------------------------------------------------------------------------
// Sorted position i holds entry q = perm[i] of the block's mode-n copy (perm is a permutation of [0, n)) and fiber
// seg[i] - 1 (inclusive scan of the head flags: 0 <= fiber < F).
__global__ void nv_lists_k(int* fkey, int* frow, double* fval, int* fid, const int* perm, const int* seg, const int* row,
                           const double* val, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t q = perm[i];
  const int f = seg[i] - 1;
  fkey[i] = f;
  frow[i] = row[q];
  fval[i] = val[q];
  fid[q] = f;
}

static void require_free(size_t need, const char* what) {
  size_t free_b = 0, total_b = 0;
  AO_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    throw Error(AOADMM_ERR_NOMEM, fmt("sparse nvecs: %s need %zu bytes of device memory, %zu are free", what, need, free_b));
}

void nvecs_build_lists(NvecsLists& l, const CooBlock& b, int pos, hipStream_t s) {
  AO_REQUIRE(pos >= 0 && pos < b.nd, "sparse nvecs: mode %d out of range", pos);
  AO_REQUIRE(b.nnz >= 1, "sparse nvecs: the block has no nonzeros");
  const int64_t n = b.nnz;
  const CooMode& cm = b.mode[pos];
  l.build_ms = 0.f;
  if (b.nd == 2) {                                     // the fibers are the other mode's indices: its copy is the list
    const CooMode& co = b.mode[1 - pos];
    l.fib = CooList{co.row.as<int>(), co.oidx.as<int>(), co.val.d(), n, b.dims[1 - pos]};
    l.row = CooList{cm.row.as<int>(), cm.oidx.as<int>(), cm.val.d(), n, b.dims[pos]};
    return;
  }
  // 20 bytes per nonzero that stay, 44 of sort keys, permutations, flags and radix-sort scratch that go again
  require_free((size_t)n * 64 + ((size_t)1 << 20), "the fiber lists");
  hipEvent_t e0, e1;
  AO_HIP(hipEventCreate(&e0)); AO_HIP(hipEventCreate(&e1));
  AO_HIP(hipEventRecord(e0, s));
  int64_t odims[kCooMaxModes];
  for (int m = 0, k = 0; m < b.nd; ++m)
    if (m != pos) odims[k++] = b.dims[m];
  CooSortWork w;
  DevBuf head, seg;
  // cm.oidx: one int32[nnz] array per other mode, every value validated by coo_build against that mode's size
  coo_sort_linear(w, cm.oidx.as<int>(), n, b.nd - 1, odims, s);
  const int64_t F = coo_runs_scan(w, head, seg, cm.oidx.as<int>(), n, b.nd - 1, s);
  // the last fiber id is F - 1 by construction of the scan; a count outside 1..nnz means the scan went wrong
  if (F < 1 || F > n) throw Error(AOADMM_ERR_HIP, fmt("sparse nvecs: fiber count %lld outside 1..%lld", (long long)F, (long long)n));
  l.fkey.alloc((size_t)n * sizeof(int)); l.frow.alloc((size_t)n * sizeof(int));
  l.fval.alloc((size_t)n * sizeof(double)); l.fid.alloc((size_t)n * sizeof(int));
  nv_lists_k<<<blocks_for(n), 256, 0, s>>>(l.fkey.as<int>(), l.frow.as<int>(), l.fval.d(), l.fid.as<int>(), w.permA.as<int>(),
                                           seg.as<int>(), cm.row.as<int>(), cm.val.d(), n);
  AO_KERNEL_CHECK();
  AO_HIP(hipEventRecord(e1, s));
  AO_HIP(hipEventSynchronize(e1));                     // the sort's buffers are locals
  (void)hipEventElapsedTime(&l.build_ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  l.fib = CooList{l.fkey.as<int>(), l.frow.as<int>(), l.fval.d(), n, F};
  l.row = CooList{cm.row.as<int>(), l.fid.as<int>(), cm.val.d(), n, b.dims[pos]};
}

// ---------------------------------------------------------------------------
// generator
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t nv_mix(uint64_t z) {          // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// counter-based: a function of (seed, epoch, column, row) only; uniform in (-1, 1)
__device__ __forceinline__ double nv_rand(uint64_t seed, uint64_t epoch, int c, int64_t i) {
  const uint64_t key = nv_mix(seed ^ nv_mix(epoch * 64 + (uint64_t)c + 1));
  const uint64_t z = nv_mix(key + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1));
  return ((double)(z >> 11) + 0.5) * (1.0 / 4503599627370496.0) - 1.0;
}
// columns c with def[c] != 0 (def null: all) of the row-major n x b matrix V <- scale * generator
__global__ void nv_fill_k(double* V, int64_t n, int b, const int* def, uint64_t seed, uint64_t epoch, double scale) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * b) return;
  const int64_t i = e / b;
  const int c = (int)(e - i * b);
  if (def != nullptr && def[c] == 0) return;
  V[e] = scale * nv_rand(seed, epoch, c, i);
}

// ---------------------------------------------------------------------------
// tall row-major matrices
// ---------------------------------------------------------------------------
constexpr int kNvTile = 32;       // rows staged in LDS at a time
constexpr int kNvMaxParts = 512;  // partial b x b sums of one product

// ws[block] (b x b, column-major) = A(r0:r1, :)' * B(r0:r1, :) over the block's rows; thread (tk, tj) of a 16 x 16
// arrangement owns the entries (tk + 16 a, tj + 16 c).  Fixed order; the partials are added by atb_fin.
__global__ __launch_bounds__(256) void nv_atb_k(const double* A, const double* B, int64_t n, int b, int64_t rows_per_block,
                                                double* ws) {
  __shared__ double As[kNvTile * kMaxRank], Bs[kNvTile * kMaxRank];
  const int t = threadIdx.x, tk = t >> 4, tj = t & 15;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
  int ka[4], jc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) { ka[a] = min(tk + 16 * a, b - 1); jc[a] = min(tj + 16 * a, b - 1); }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int64_t base = r0; base < r1; base += kNvTile) {
    const int nrow = r1 - base < kNvTile ? (int)(r1 - base) : kNvTile;
    for (int e = t; e < nrow * b; e += 256) { As[e] = A[base * b + e]; Bs[e] = B[base * b + e]; }
    __syncthreads();
    for (int rr = 0; rr < nrow; ++rr) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) { av[a] = As[rr * b + ka[a]]; bv[a] = Bs[rr * b + jc[a]]; }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] += av[a] * bv[c];
    }
    __syncthreads();
  }
  double* out = ws + (int64_t)blockIdx.x * b * b;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = tk + 16 * a, j = tj + 16 * c;
      if (k < b && j < b) out[k + b * j] = acc[a][c];
    }
}

// out(i, c) at out[i * oI + c * oR] = sum_k A(i, k) * T(k, c);  A row-major n x b, T column-major b x nc in LDS
__global__ __launch_bounds__(256) void nv_gemm_k(const double* A, int64_t n, int b, const double* T, int nc, double* out,
                                                 int64_t oI, int64_t oR) {
  __shared__ double Ts[kMaxRank * kMaxRank];
  for (int e = threadIdx.x; e < b * nc; e += 256) Ts[e] = T[e];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * nc) return;
  const int64_t i = e / nc;
  const int c = (int)(e - i * nc);
  const double* a = A + i * b;
  const double* tc = Ts + b * c;
  double acc = 0.0;
  for (int k = 0; k < b; ++k) acc += a[k] * tc[k];
  out[i * oI + c * oR] = acc;
}

// part[block] = sum over the block's 256 entries (i, c), c < r, of (sum_k (Y(i,k) - theta[c] V(i,k)) T(k,c))^2:
// the squared Frobenius norm of Y Q_r - V Q_r Theta_r
__global__ __launch_bounds__(256) void nv_resid_k(const double* Y, const double* V, int64_t n, int b, const double* T,
                                                  const double* theta, int r, double* part) {
  __shared__ double Ts[kMaxRank * kMaxRank];
  __shared__ double red[256];
  for (int e = threadIdx.x; e < b * r; e += 256) Ts[e] = T[e];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double v = 0.0;
  if (e < n * r) {
    const int64_t i = e / r;
    const int c = (int)(e - i * r);
    const double th = theta[c];
    const double *y = Y + i * b, *x = V + i * b, *tc = Ts + b * c;
    double acc = 0.0;
    for (int k = 0; k < b; ++k) acc += (y[k] - th * x[k]) * tc[k];
    v = acc * acc;
  }
  v = block_sum_pow2(v, red);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}
// out[0] = sum of part[0 .. np) in a fixed order (one block)
__global__ __launch_bounds__(256) void nv_sum_k(const double* part, int64_t np, double* out) {
  __shared__ double red[256];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < np; i += 256) v += part[i];
  v = block_sum_pow2(v, red);
  if (threadIdx.x == 0) out[0] = v;
}

// ---------------------------------------------------------------------------
// b x b matrices
// ---------------------------------------------------------------------------
enum { NV_RITZ = 0, NV_WHITEN = 1, NV_LOWDIN = 2 };
// From the eigendecomposition w, Q (column-major b x b, any order) of a symmetric b x b matrix, with the eigenvalues
// taken in descending order (ties: lower index first):
//   NV_RITZ:   T(:, c) = q_c,               theta[c] = w_c
//   NV_WHITEN: T(:, c) = q_c / sqrt(w_c),   def[c] = 0;  where w_c <= eps * w_max: T(:, c) = 0, def[c] = 1
//   NV_LOWDIN: T = Q diag(w^-1/2) Q' (the symmetric inverse square root; eigenvalues <= 0 count as 1)
__global__ __launch_bounds__(64) void nv_prep_k(int mode, const double* w, const double* Q, int b, double* T, double* theta,
                                                int* def) {
  __shared__ int ord[kMaxRank];
  __shared__ double ws[kMaxRank];
  const int t = threadIdx.x;
  if (t < b) { ws[t] = w[t]; ord[t] = t; }            // (the identity stays where a NaN breaks the order below)
  __syncthreads();
  if (t < b) {                                        // rank of eigenvalue t in the descending order
    int pos = 0;
    for (int j = 0; j < b; ++j) pos += (ws[j] > ws[t]) || (ws[j] == ws[t] && j < t);
    ord[pos] = t;
  }
  __syncthreads();
  if (mode == NV_LOWDIN) {
    for (int e = t; e < b * b; e += 64) {
      const int i = e % b, j = e / b;
      double acc = 0.0;
      for (int k = 0; k < b; ++k) {
        const double lam = ws[k] > 0.0 ? ws[k] : 1.0;
        acc += Q[i + b * k] * Q[j + b * k] / sqrt(lam);
      }
      T[e] = acc;
    }
    return;
  }
  const double wmax = ws[ord[0]];
  for (int e = t; e < b * b; e += 64) {
    const int k = e % b, c = e / b;
    const int src = ord[c];
    const double lam = ws[src];
    double v = Q[k + b * src];
    if (mode == NV_WHITEN) v = (wmax > 0.0 && lam > DBL_EPSILON * wmax) ? v / sqrt(lam) : 0.0;
    T[e] = v;
  }
  if (t < b) {
    const double lam = ws[ord[t]];
    if (mode == NV_RITZ) theta[t] = lam;
    else def[t] = !(wmax > 0.0 && lam > DBL_EPSILON * wmax);
  }
}

// Column c (one block each; c < r <= 64) of the column-major n x r matrix U is negated when its entry of largest
// magnitude (the first one on a tie) is negative.
__global__ __launch_bounds__(256) void nv_sign_k(double* U, int64_t n, int64_t ld) {
  __shared__ double bm[256];
  __shared__ long long bi[256];
  double* u = U + ld * blockIdx.x;
  double m = -1.0;
  long long at = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double a = fabs(u[i]);
    if (a > m) { m = a; at = i; }                     // ascending i: the first of equal magnitudes stays
  }
  bm[threadIdx.x] = m; bi[threadIdx.x] = at;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      const double m2 = bm[threadIdx.x + st];
      const long long i2 = bi[threadIdx.x + st];
      if (m2 > bm[threadIdx.x] || (m2 == bm[threadIdx.x] && i2 < bi[threadIdx.x])) { bm[threadIdx.x] = m2; bi[threadIdx.x] = i2; }
    }
    __syncthreads();
  }
  if (!(u[bi[0]] < 0.0)) return;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < n; i += 256) u[i] = -u[i];
}

// ---------------------------------------------------------------------------
// the iteration
// ---------------------------------------------------------------------------
namespace {

struct NvWork {
  int b = 0;
  uint64_t seed = 0, epoch = 0;
  hipStream_t s = nullptr;
  DevBuf ws, H, Q, w, T, theta, def, part, stat;

  // out (b x b) = A' * B, A and B row-major n x b
  void atb(const double* A, const double* B, int64_t n, int bb, double* out) {
    const int64_t parts = std::min<int64_t>(kNvMaxParts, cdiv(n, 256));
    const int64_t rpb = cdiv(n, parts);
    const int nb = (int)cdiv(n, rpb);
    nv_atb_k<<<nb, 256, 0, s>>>(A, B, n, bb, rpb, nb == 1 ? out : ws.d());
    AO_KERNEL_CHECK();
    if (nb > 1) atb_fin(out, ws.d(), nb, bb * bb, nullptr, s);
  }
  void gemm(const double* A, int64_t n, int bb, const double* Tm, int nc, double* out, int64_t oI, int64_t oR) {
    nv_gemm_k<<<blocks_for(n * nc), 256, 0, s>>>(A, n, bb, Tm, nc, out, oI, oR);
    AO_KERNEL_CHECK();
  }
  void eig(int mode, int bb) {                        // of H
    sym_eig_small(H.d(), bb, w.d(), Q.d(), s);
    nv_prep_k<<<1, 64, 0, s>>>(mode, w.d(), Q.d(), bb, T.d(), theta.d(), def.as<int>());
    AO_KERNEL_CHECK();
  }
  // out = in * Q diag(lambda^-1/2) of in' * in = Q diag(lambda) Q'; directions with lambda <= eps * lambda_max
  // become fresh generator columns (of norm about 1), which the next whitening orthogonalises against the rest
  void whiten(const double* in, double* out, int64_t n) {
    atb(in, in, n, b, H.d());
    eig(NV_WHITEN, b);
    gemm(in, n, b, T.d(), b, out, b, 1);
    nv_fill_k<<<blocks_for(n * b), 256, 0, s>>>(out, n, b, def.as<int>(), seed, ++epoch, std::sqrt(3.0 / (double)n));
    AO_KERNEL_CHECK();
  }
};

}  // namespace

void sparse_nvecs(const NvecsLists& l, int r, const aoadmm_nvecs_options* opt, double* U, int64_t ldU, double* eig,
                  aoadmm_nvecs_info* info, DevBuf* slot_row, DevBuf* slot_val, LaunchTimers* timers, hipStream_t s) {
  const int64_t I = l.row.rows, F = l.fib.rows, nnz = l.row.n;
  AO_REQUIRE(nnz >= 1 && l.fib.n == nnz, "sparse nvecs: the block has no nonzeros");
  AO_REQUIRE(r >= 1 && r <= std::min<int64_t>(I, kMaxRank), "sparse nvecs: r = %d outside 1..%lld", r,
             (long long)std::min<int64_t>(I, kMaxRank));
  AO_REQUIRE(U == nullptr || ldU >= I, "sparse nvecs: ldU %lld < %lld rows", (long long)ldU, (long long)I);
  AO_REQUIRE(F >= 1 && F < ((int64_t)1 << 31), "sparse nvecs: %lld fibers", (long long)F);
  const int over = opt && opt->oversample > 0 ? opt->oversample : kNvecsOversample;
  const int max_iters = opt && opt->max_iters > 0 ? opt->max_iters : kNvecsMaxIters;
  const double tol = opt && opt->tol > 0.0 ? opt->tol : kNvecsTol;
  // block width: r + oversample, cut to the rank the unfolding can have (min(I, F)) and to kMaxRank, never below r
  const int b = (int)std::min<int64_t>(std::min<int64_t>(I, kMaxRank), std::max<int64_t>(r, std::min<int64_t>(F, (int64_t)r + over)));
  // W, the three I x b work matrices, U, the partial sums and the carry slots of the two passes
  const int64_t teams = cdiv(nnz, kCooChunk);
  const size_t need = (size_t)F * b * 8 + (size_t)I * b * 8 * 3 + (size_t)I * r * 8 +
                      (size_t)kNvMaxParts * b * b * 8 + (size_t)cdiv(I * r, 256) * 8 +
                      (size_t)(2 * teams + 2 * cdiv(2 * teams, kCooChunk) + 64) * (4 + 8 * (size_t)b) + ((size_t)1 << 20);
  require_free(need, "the work arrays");
  NvWork k;
  k.b = b; k.s = s; k.seed = opt ? opt->seed : 0;
  DevBuf V, Y, S, W, Ud;
  V.alloc((size_t)I * b * 8); Y.alloc((size_t)I * b * 8); S.alloc((size_t)I * b * 8);
  W.alloc((size_t)F * b * 8); Ud.alloc((size_t)I * r * 8);
  k.ws.alloc((size_t)kNvMaxParts * b * b * 8);
  k.H.alloc((size_t)b * b * 8); k.Q.alloc((size_t)b * b * 8); k.T.alloc((size_t)b * b * 8);
  k.w.alloc((size_t)b * 8); k.def.alloc((size_t)b * sizeof(int));
  k.stat.alloc((size_t)(1 + b) * 8);                   // [0] squared residual, [1 ..] Ritz values, descending
  k.theta.view(k.stat.d() + 1, (size_t)b * 8);
  const int64_t nparts = cdiv(I * r, 256);
  k.part.alloc((size_t)nparts * 8);

  auto pass = [&](const CooList& li, const double* src, double* out) {
    LaunchTimers::Pair pr;
    if (timers) pr = timers->begin(timers->stats[3], timers->profile, s);
    coo_list_pass(li, src, b, out, slot_row, slot_val, s);
    if (timers)
      timers->end(timers->stats[3], pr, s, (double)li.n * (16.0 + 8.0 * b) + (double)li.rows * b * 8.0, 2.0 * (double)li.n * b);
  };

  // start: generator columns, orthonormalised
  nv_fill_k<<<blocks_for(I * b), 256, 0, s>>>(V.d(), I, b, nullptr, k.seed, 0, 1.0);
  AO_KERNEL_CHECK();
  k.whiten(V.d(), S.d(), I);
  k.whiten(S.d(), V.d(), I);

  std::vector<double> stat((size_t)1 + b);
  int it = 0, converged = 0;
  double rho = 0.0;
  for (;;) {
    ++it;
    pass(l.fib, V.d(), W.d());                         // W = M' V
    k.atb(W.d(), W.d(), F, b, k.H.d());                // H = W' W = Q Theta Q'
    k.eig(NV_RITZ, b);
    pass(l.row, W.d(), Y.d());                         // Y = M W
    nv_resid_k<<<(unsigned)nparts, 256, 0, s>>>(Y.d(), V.d(), I, b, k.T.d(), k.theta.d(), r, k.part.d());
    AO_KERNEL_CHECK();
    nv_sum_k<<<1, 256, 0, s>>>(k.part.d(), nparts, k.stat.d());
    AO_KERNEL_CHECK();
    AO_HIP(hipMemcpyAsync(stat.data(), k.stat.p, stat.size() * 8, hipMemcpyDeviceToHost, s));
    AO_HIP(hipStreamSynchronize(s));
    rho = stat[1] > 0.0 ? std::sqrt(stat[0]) / stat[1] : 0.0;
    if (!(rho == rho)) throw Error(AOADMM_ERR_INVALID, "sparse nvecs: the data hold a NaN or an infinity");
    if (rho <= tol) { converged = 1; break; }
    if (it >= max_iters) break;
    k.whiten(Y.d(), S.d(), I);                         // V = orth(Y), whitened twice
    k.whiten(S.d(), V.d(), I);
  }
  // U = V Q_r, polished by the symmetric inverse square root of its own Gram matrix (keeps every column where it is),
  // then the sign rule
  k.gemm(V.d(), I, b, k.T.d(), r, S.d(), r, 1);
  k.atb(S.d(), S.d(), I, r, k.H.d());
  k.eig(NV_LOWDIN, r);
  k.gemm(S.d(), I, r, k.T.d(), r, Ud.d(), 1, I);
  nv_sign_k<<<r, 256, 0, s>>>(Ud.d(), I, I);
  AO_KERNEL_CHECK();
  if (U) AO_HIP(hipMemcpy2DAsync(U, (size_t)ldU * 8, Ud.p, (size_t)I * 8, (size_t)I * 8, (size_t)r, hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));
  if (eig) for (int c = 0; c < r; ++c) eig[c] = stat[(size_t)1 + c];
  if (info) {
    info->iterations = it; info->converged = converged; info->block = b; info->residual = rho; info->fibers = F;
  }
}

}  // namespace aoadmm
