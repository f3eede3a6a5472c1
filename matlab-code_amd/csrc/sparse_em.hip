// Observed-only sparse CP blocks: residual / statistics passes over the per-mode copies of the nonzeros, the R x R
// parts of f_rel_missing and the dense correction of the MTTKRP.  See sparse_em.h and DESIGN.md section 9.3.
#include <algorithm>

#include "coo_team.h"
#include "readback.h"
#include "small.h"
#include "sparse_em.h"

namespace aoadmm {

// ---------------------------------------------------------------------------
// passes over one copy of the nonzeros
// ---------------------------------------------------------------------------
// The team layout of coo_team.h, kSemUnroll entries at a time.  The model value of an entry is the team_sum of the
// lanes' products.
struct SemArgs {
  const int* row;
  const int* oidx;
  const double* val;
  int64_t nnz;
  CooFactor f[kCooMaxModes];    // current factors in the copy's order: [0] the mode the copy is sorted by, then the others
  CooFactor fo[kCooMaxModes];   // the snapshot in the same order (STAT == 2)
  int nd, R;
  double* res;                  // x - m per entry, or null
  double* part;                 // kSemSums (WT: kSemSumsW) sums per team (STAT > 0)
  const double* wt;             // WT: the stored entries' weights in the copy's order, or null (all 1)
  double alpha;                 // WT: the weight of every unstored entry
};

constexpr int kSemUnroll = 4;

// ND = order of the block (2..4 compiled in; 0: a.nd at run time, up to 8)
// STAT 0: residuals only; 1: + sum (x-m)^2 and sum m^2; 2: + sum (m_new - m_old)^2 in the telescoped form
//   m_new - m_old = sum_a prod_{n<a} fo_n * (f_a - fo_a) * prod_{n>a} f_n   per column, then summed over the columns
// WT: the weighted form.  res = w x - (w - alpha) m, the sums are sum w (x-m)^2, sum m^2, sum (1-w)^2 m^2 and, STAT == 2,
//   sum dm^2, sum (1-w)^2 dm^2: no difference of sums is formed here
template <int G, int ND, int STAT, bool WT>
__global__ __launch_bounds__(256) void sem_pass_k(SemArgs a) {
  const CooTeam<G> t(a.nnz, a.R);
  if (t.idle()) return;
  const int64_t end = t.end();
  const int rr = t.rr();
  const bool live = t.live();
  constexpr int NMAX = ND > 0 ? ND : kCooMaxModes;
  const int nd = ND > 0 ? ND : a.nd;
  double s_res = 0.0, s_m2 = 0.0, s_d2 = 0.0, s_cm2 = 0.0, s_cd2 = 0.0;
  for (int64_t i0 = t.start; i0 < end; i0 += kSemUnroll) {
    double mu[kSemUnroll], du[kSemUnroll], xu[kSemUnroll], wu[kSemUnroll];
#pragma unroll
    for (int u = 0; u < kSemUnroll; ++u) {
      const int64_t i = i0 + u < end ? i0 + u : end - 1;
      double fv[NMAX], fov[NMAX];
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        if (n < nd) {
          const int64_t idx = n == 0 ? a.row[i] : a.oidx[(int64_t)(n - 1) * a.nnz + i];
          fv[n] = coo_at(a.f[n], idx, rr);
          if (STAT == 2) fov[n] = coo_at(a.fo[n], idx, rr);
        }
      }
      xu[u] = a.val[i];
      if (WT) wu[u] = a.wt != nullptr ? a.wt[i] : 1.0;
      double m = 1.0;
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < nd) m *= fv[n];
      double d = 0.0;
      if (STAT == 2) {
        double suf[NMAX];                            // suf[n] = prod_{k > n} f_k
        double sprod = 1.0;
#pragma unroll
        for (int n = NMAX - 1; n >= 0; --n)
          if (n < nd) { suf[n] = sprod; sprod *= fv[n]; }
        double pre = 1.0;                            // prod_{k < n} fo_k
#pragma unroll
        for (int n = 0; n < NMAX; ++n)
          if (n < nd) { d += pre * (fv[n] - fov[n]) * suf[n]; pre *= fov[n]; }
      }
      mu[u] = live ? m : 0.0;
      du[u] = live ? d : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kSemUnroll; ++u) {
      mu[u] = team_sum<G>(mu[u]);
      if (STAT == 2) du[u] = team_sum<G>(du[u]);
    }
#pragma unroll
    for (int u = 0; u < kSemUnroll; ++u) {
      if (i0 + u < end) {
        const double e = xu[u] - mu[u];
        if (WT) {
          const double w = wu[u], c2 = (1.0 - w) * (1.0 - w), m2 = mu[u] * mu[u], d2 = du[u] * du[u];
          if (a.res != nullptr && t.r == 0) a.res[i0 + u] = w * xu[u] - (w - a.alpha) * mu[u];
          if (STAT > 0) { s_res += w * (e * e); s_m2 += m2; s_cm2 += c2 * m2; }
          if (STAT == 2) { s_d2 += d2; s_cd2 += c2 * d2; }
        } else {
          if (a.res != nullptr && t.r == 0) a.res[i0 + u] = e;
          if (STAT > 0) { s_res += e * e; s_m2 += mu[u] * mu[u]; }
          if (STAT == 2) s_d2 += du[u] * du[u];
        }
      }
    }
  }
  if (STAT > 0 && t.r == 0) {
    if (WT) {
      double* q = a.part + kSemSumsW * t.team;
      q[0] = s_res; q[1] = s_m2; q[2] = s_cm2; q[3] = s_d2; q[4] = s_cd2;
    } else {
      a.part[3 * t.team + 0] = s_res;
      a.part[3 * t.team + 1] = s_m2;
      a.part[3 * t.team + 2] = s_d2;
    }
  }
}

template <int STAT, bool WT>
static void launch_sem_pass(const SemArgs& a, hipStream_t s) {
  for_team_width(a.R, [&](auto g) {
    for_order<2>(a.nd, [&](auto nd) {                // orders 2..4 compiled in
      constexpr int G = decltype(g)::value;
      sem_pass_k<G, decltype(nd)::value, STAT, WT><<<coo_team_grid(a.nnz, G), 256, 0, s>>>(a);
    });
  });
  AO_KERNEL_CHECK();
}

template <bool WT>
static void launch_sem_stat(const SemArgs& a, int stat, hipStream_t s) {
  switch (stat) {
    case 0: launch_sem_pass<0, WT>(a, s); break;
    case 1: launch_sem_pass<1, WT>(a, s); break;
    default: launch_sem_pass<2, WT>(a, s); break;
  }
}

static void launch_sem(const SemArgs& a, int stat, bool weighted, hipStream_t s) {
  if (weighted) launch_sem_stat<true>(a, stat, s);
  else launch_sem_stat<false>(a, stat, s);
}

// res = w o x, the residual array of the starting point of a weighted block (w absent: res = x)
__global__ void sem_fill_k(double* res, const double* val, const double* wt, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    res[e] = wt != nullptr ? wt[e] * val[e] : val[e];
}

// flag[0] = 1 where two subscript arrays differ (every writer stores the same value)
__global__ void sem_differ_k(int* flag, const int* x, const int* y, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    if (x[e] != y[e]) flag[0] = 1;
}

// ---------------------------------------------------------------------------
// small dense parts
// ---------------------------------------------------------------------------
// snapshot of one factor: column-major with ld = rows, and row-major
__global__ void sem_snapshot_k(double* snapC, double* snapR, const double* F, int64_t ld, int64_t rows, int R) {
  const int64_t n = rows * R;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e % rows;
    const int64_t r = e / rows;
    const double v = F[i + ld * r];
    snapC[e] = v;
    snapR[i * R + r] = v;
  }
}

// D = F - Fo (both column-major, D and Fo with ld = rows)
__global__ void sem_diff_k(double* D, const double* F, int64_t ld, const double* Fo, int64_t rows, int R) {
  const int64_t n = rows * R;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    D[e] = F[e % rows + ld * (e / rows)] - Fo[e];
}

// W = had_{j != skip} M_j, the R x R matrices M_j at M + j * stride
__global__ void sem_had_k(double* W, const double* M, int64_t stride, int nd, int skip, int RR) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= RR) return;
  double w = 1.0;
  for (int j = 0; j < nd; ++j)
    if (j != skip) w *= M[(int64_t)j * stride + e];
  W[e] = w;
}

struct SemFinish {
  const double* part;
  int64_t nteams;
  const double *GFo, *GF, *DtD, *DtFo;   // R x R per mode, modes kCooMaxModes * R * R apart
  int nd, R;
  int form;                              // 0: statistics only; 1: first step (no snapshot); 2: later step
  double* em;                            // the block's EM slots
  double* hold;
  double alpha;                          // WT: the weight of every unstored entry
};

// T_a' T_b of one mode at (r, s), T in {0: Fo, 1: D, 2: F}, from Fo'Fo, D'D, D'Fo and F'F (F = Fo + D)
__device__ __forceinline__ double sem_pair(int ta, int tb, const double* GFo, const double* GF, const double* DtD,
                                           const double* DtFo, int r, int s, int R) {
  const int rs = r + s * R, sr = s + r * R;
  if (ta == tb) return ta == 0 ? GFo[rs] : ta == 1 ? DtD[rs] : GF[rs];
  if (ta == 1 && tb == 0) return DtFo[rs];
  if (ta == 0 && tb == 1) return DtFo[sr];
  if (ta == 0 && tb == 2) return GFo[rs] + DtFo[sr];      // Fo'F = Fo'Fo + Fo'D
  if (ta == 2 && tb == 0) return GFo[rs] + DtFo[rs];      // F'Fo = Fo'Fo + D'Fo
  if (ta == 1 && tb == 2) return DtFo[rs] + DtD[rs];      // D'F = D'Fo + D'D
  return DtFo[sr] + DtD[rs];                              // F'D = Fo'D + D'D
}

// One block.  Sums the teams' partials, then
//   form 1: num = sum(had F'F) - sum_Omega m_new^2, den = 0
//   form 2: num = ||M_new - M_old||^2 - sum_Omega (dm)^2 with the telescoped norm
//             sum_{a,b} sum(had_n T^a_n' T^b_n),  T^a_n = Fo_n (n < a), D_n (n = a), F_n (n > a);  den = hold[0]
//   both leave hold[0] = sum(had F'F) - sum_Omega m_new^2 for the next step
// WT (the weighted form; unst = sum(had F'F) - sum_Omega m^2 is the unstored entries' share of ||M||^2, never below 0):
//   every form: em[kEmObsRes] = sum_Omega w (x - m)^2 + alpha * unst (form 0 needs F'F for that when alpha > 0)
//   form 1: num = (1 - alpha)^2 unst + sum_Omega (1 - w)^2 m_new^2, den = 0
//   form 2: num = (1 - alpha)^2 (||M_new - M_old||^2 - sum_Omega dm^2) + sum_Omega (1 - w)^2 dm^2;  den = hold[0]
//   both leave hold[0] = (1 - alpha)^2 unst + sum_Omega (1 - w)^2 m_new^2
template <bool WT>
__global__ __launch_bounds__(256) void sem_finish_k(SemFinish a) {
  __shared__ double sh[256];
  constexpr int NS = WT ? kSemSumsW : kSemSums;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0, p4 = 0.0;
  for (int64_t t = threadIdx.x; t < a.nteams; t += 256) {
    p0 += a.part[NS * t];
    p1 += a.part[NS * t + 1];
    p2 += a.part[NS * t + 2];
    if (WT) { p3 += a.part[NS * t + 3]; p4 += a.part[NS * t + 4]; }
  }
  const double s_res = coo_block_sum(p0, sh);
  const double s_m2 = coo_block_sum(p1, sh);
  const double s_cm2 = WT ? coo_block_sum(p2, sh) : 0.0;
  const double s_d2 = coo_block_sum(WT ? p3 : p2, sh);
  const double s_cd2 = WT ? coo_block_sum(p4, sh) : 0.0;
  if (a.form == 0 && !(WT && a.alpha > 0.0)) {
    if (threadIdx.x == 0) a.em[kEmObsRes] = s_res;
    return;
  }
  const int R = a.R, RR = R * R;
  const int64_t ms = RR;                             // matrices of consecutive modes are R * R apart
  double full = 0.0, delta = 0.0;
  for (int e = threadIdx.x; e < RR; e += 256) {
    const int r = e % R, s = e / R;
    double h = 1.0;
    for (int n = 0; n < a.nd; ++n) h *= a.GF[n * ms + e];
    full += h;
    if (a.form == 2) {
      for (int ta = 0; ta < a.nd; ++ta)
        for (int tb = 0; tb < a.nd; ++tb) {
          double g = 1.0;
          for (int n = 0; n < a.nd; ++n)
            g *= sem_pair(n < ta ? 0 : n == ta ? 1 : 2, n < tb ? 0 : n == tb ? 1 : 2, a.GFo + n * ms, a.GF + n * ms,
                          a.DtD + n * ms, a.DtFo + n * ms, r, s, R);
          delta += g;
        }
    }
  }
  const double normF = coo_block_sum(full, sh);
  const double normD = coo_block_sum(delta, sh);
  if (WT) {
    if (threadIdx.x == 0) {
      const double unst = normF - s_m2 > 0.0 ? normF - s_m2 : 0.0;
      const double move = normD - s_d2 > 0.0 ? normD - s_d2 : 0.0;
      const double c2 = (1.0 - a.alpha) * (1.0 - a.alpha);
      a.em[kEmObsRes] = s_res + a.alpha * unst;
      if (a.form != 0) {
        const double den = a.form == 2 ? a.hold[0] : 0.0;
        a.em[kEmNum] = a.form == 2 ? c2 * move + s_cd2 : c2 * unst + s_cm2;
        a.em[kEmDen] = den;
        a.hold[0] = c2 * unst + s_cm2;
      }
    }
    return;
  }
  if (threadIdx.x == 0) {
    const double den = a.form == 2 ? a.hold[0] : 0.0;
    const double num = a.form == 2 ? normD - s_d2 : normF - s_m2;
    a.em[kEmObsRes] = s_res;
    a.em[kEmNum] = num > 0.0 ? num : 0.0;            // a sum of squares: rounding may leave -eps where nothing is missing
    a.em[kEmDen] = den > 0.0 ? den : 0.0;
    a.hold[0] = normF - s_m2;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
void sem_enable(SparseEm& e, const CooBlock& b, int R, hipStream_t s) {
  AO_REQUIRE(R >= 1 && R <= kMaxRank, "observed-only block: rank %d outside 1..%d", R, kMaxRank);
  SparseEm n;
  n.on = true; n.nd = b.nd; n.R = R; n.nnz = b.nnz;
  int64_t maxrows = 1;
  for (int m = 0; m < b.nd; ++m) {
    n.dims[m] = b.dims[m];
    maxrows = std::max(maxrows, b.dims[m]);
    n.res[m].alloc((size_t)b.nnz * sizeof(double));
    n.snapC[m].alloc((size_t)b.dims[m] * R * sizeof(double));
    n.snapR[m].alloc((size_t)b.dims[m] * R * sizeof(double));
  }
  n.small.alloc(((size_t)5 * kCooMaxModes + 1) * R * R * sizeof(double));
  n.D.alloc((size_t)maxrows * R * sizeof(double));
  n.part.alloc((size_t)kSemSumsW * cdiv(b.nnz, kCooChunk) * sizeof(double));
  n.ws.alloc(atb_ws_bytes(maxrows, R, R));
  n.hold.alloc(2 * sizeof(double));
  if (e.on && e.weighted && e.nd == b.nd && e.nnz == b.nnz) {     // marked again: the weights stay
    n.weighted = true; n.alpha = e.alpha; n.wnormsq = e.wnormsq;
    for (int m = 0; m < b.nd; ++m) n.wt[m] = std::move(e.wt[m]);
  }
  e = std::move(n);
  sem_reset(e, b, s);
}

void sem_reset(SparseEm& e, const CooBlock& b, hipStream_t s) {
  e.have_snap = false;
  if (!e.weighted) return;                           // the plain MTTKRP reads the block's own values
  AO_REQUIRE(e.on && e.nd == b.nd && e.nnz == b.nnz, "internal: weights of another block");
  for (int m = 0; m < e.nd; ++m) {
    sem_fill_k<<<blocks_for(std::min<int64_t>(e.nnz, (int64_t)1 << 22)), 256, 0, s>>>(e.res[m].d(), b.mode[m].val.d(),
                                                                                     e.wt[m].p ? e.wt[m].d() : nullptr, e.nnz);
    AO_KERNEL_CHECK();
  }
}

void sem_check_weight_list(const CooBlock& b, const CooBlock& wts, hipStream_t s) {
  if (wts.nd != b.nd || wts.nnz != b.nnz)
    throw Error(AOADMM_ERR_INVALID, fmt("entry weights: the list holds %lld distinct subscripts, the block stores %lld entries",
                                        (long long)wts.nnz, (long long)b.nnz));
  DevBuf flag;
  flag.alloc(sizeof(int));
  AO_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
  const unsigned grid = blocks_for(std::min<int64_t>(b.nnz * std::max(1, b.nd - 1), (int64_t)1 << 22));
  for (int m = 0; m < b.nd; ++m) {
    sem_differ_k<<<grid, 256, 0, s>>>(flag.as<int>(), b.mode[m].row.as<int>(), wts.mode[m].row.as<int>(), b.nnz);
    AO_KERNEL_CHECK();
    sem_differ_k<<<grid, 256, 0, s>>>(flag.as<int>(), b.mode[m].oidx.as<int>(), wts.mode[m].oidx.as<int>(), b.nnz * (b.nd - 1));
    AO_KERNEL_CHECK();
  }
  int differ = 0;
  AO_HIP(hipMemcpyAsync(&differ, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));
  if (differ) throw Error(AOADMM_ERR_INVALID, "entry weights: the list names an entry the block does not store");
}

void sem_set_weights(SparseEm& e, const CooBlock& b, CooBlock* wts, double alpha, hipStream_t s) {
  AO_REQUIRE(e.on && e.nd == b.nd && e.nnz == b.nnz && (!wts || (wts->nd == b.nd && wts->nnz == b.nnz)), "internal: weights for a block that is not marked");
  e.weighted = true;
  e.alpha = alpha;
  for (int m = 0; m < e.nd; ++m) {
    if (wts) e.wt[m] = std::move(wts->mode[m].val);
    else e.wt[m].release();
  }
  sem_reset(e, b, s);
  // sum_Omega w x^2 = <w o x, x> over the first copy
  DevBuf ws;
  ws.alloc(((size_t)kReduceBatchMax * kReduceBatchSplit + 1) * sizeof(double));
  ReduceBatch rb;
  ReduceTask k;
  k.kind = RT_DOT; k.slot = ws.d() + (size_t)kReduceBatchMax * kReduceBatchSplit; k.x = e.res[0].d(); k.y = b.mode[0].val.d(); k.n = e.nnz;
  rb.add(k);
  reduce_batch(rb, ws.d(), s);
  AO_HIP(hipMemcpyAsync(&e.wnormsq, k.slot, sizeof(double), hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));
}

int64_t sem_resident_bytes(const SparseEm& e) {
  int64_t n = 0;
  if (!e.on) return 0;
  for (int m = 0; m < e.nd; ++m)
    for (const DevBuf* d : {&e.res[m], &e.wt[m], &e.snapC[m], &e.snapR[m]})
      if (d->p) n += (int64_t)d->bytes;
  return n;
}

// the factors in the order of mode pos's copy: pos first, then the others in mode order
static void copy_order(CooFactor* out, const SemFac* f, int nd, int pos, int R) {
  int k = 1;
  for (int m = 0; m < nd; ++m) {
    const CooFactor cf = f[m].pT ? CooFactor{f[m].pT, (int64_t)R, 1} : CooFactor{f[m].p, 1, f[m].ld};
    if (m == pos) out[0] = cf; else out[k++] = cf;
  }
}

void sem_step_begin(SparseEm& e, const CooBlock& b, const SemFac* f, bool stats_only, hipStream_t s) {
  AO_REQUIRE(e.on && e.nd == b.nd && e.nnz == b.nnz && b.nnz > 0 && !b.sharded, "internal: EM step on a block that is not observed-only");
  const int nd = e.nd, R = e.R;
  if (e.have_snap && !stats_only)
    for (int n = 0; n < nd; ++n) {
      const int64_t rows = e.dims[n];
      sem_diff_k<<<blocks_for(std::min<int64_t>(rows * R, (int64_t)1 << 20)), 256, 0, s>>>(e.D.d(), f[n].p, f[n].ld, e.snapC[n].d(), rows, R);
      AO_KERNEL_CHECK();
      atb_small(e.mat(2, n), e.D.d(), rows, e.D.d(), rows, rows, R, R, e.ws.d(), nullptr, s);
      atb_small(e.mat(3, n), e.D.d(), rows, e.snapC[n].d(), rows, rows, R, R, e.ws.d(), nullptr, s);
    }
}

void sem_step_pass(SparseEm& e, const CooBlock& b, const SemFac* f, int pos, bool stats_only, hipStream_t s) {
  AO_REQUIRE(e.on && e.nd == b.nd && e.nnz == b.nnz && pos >= 0 && pos < e.nd && (!stats_only || pos == 0),
             "internal: EM pass over copy %d", pos);
  const int nd = e.nd, R = e.R;
  const bool snap = e.have_snap && !stats_only;
  SemArgs a;
  a.nnz = e.nnz; a.nd = nd; a.R = R; a.part = e.part.d();
  const CooMode& cm = b.mode[pos];
  a.row = cm.row.as<int>(); a.oidx = cm.oidx.as<int>(); a.val = cm.val.d();
  a.res = stats_only ? nullptr : e.res[pos].d();
  a.wt = e.weighted && e.wt[pos].p ? e.wt[pos].d() : nullptr;
  a.alpha = e.alpha;
  copy_order(a.f, f, nd, pos, R);
  int stat = 0;
  if (pos == 0) {                                    // the statistics ride on the mode-1 copy's pass
    stat = snap ? 2 : 1;
    if (snap) {
      SemFac fo[kCooMaxModes];
      for (int m = 0; m < nd; ++m) fo[m] = SemFac{e.snapC[m].d(), e.dims[m], e.snapR[m].d()};
      copy_order(a.fo, fo, nd, 0, R);
    }
  }
  launch_sem(a, stat, e.weighted, s);
}

void sem_step_finish(SparseEm& e, const SemFac* f, bool stats_only, double* em, hipStream_t s) {
  const int nd = e.nd, R = e.R, RR = R * R;
  const int64_t nteams = cdiv(e.nnz, kCooChunk);
  const bool snap = e.have_snap && !stats_only;
  SemFinish fa;
  fa.part = e.part.d(); fa.nteams = nteams; fa.nd = nd; fa.R = R; fa.em = em; fa.hold = e.hold.d();
  fa.GFo = e.mat(0, 0); fa.GF = e.mat(1, 0); fa.DtD = e.mat(2, 0); fa.DtFo = e.mat(3, 0);
  fa.form = stats_only ? 0 : snap ? 2 : 1;
  fa.alpha = e.alpha;
  if (!stats_only || (e.weighted && e.alpha > 0.0))   // the weighted objective of the starting point needs ||M||^2
    for (int n = 0; n < nd; ++n)
      atb_small(e.mat(1, n), f[n].p, f[n].ld, f[n].p, f[n].ld, e.dims[n], R, R, e.ws.d(), nullptr, s);
  if (e.weighted) sem_finish_k<true><<<1, 256, 0, s>>>(fa);
  else sem_finish_k<false><<<1, 256, 0, s>>>(fa);
  AO_KERNEL_CHECK();
  if (stats_only) return;
  // the snapshot: Fo <- F, Fo'Fo <- F'F
  for (int n = 0; n < nd; ++n) {
    const int64_t rows = e.dims[n];
    sem_snapshot_k<<<blocks_for(std::min<int64_t>(rows * R, (int64_t)1 << 20)), 256, 0, s>>>(e.snapC[n].d(), e.snapR[n].d(), f[n].p, f[n].ld, rows, R);
    AO_KERNEL_CHECK();
  }
  AO_HIP(hipMemcpyAsync(e.mat(0, 0), e.mat(1, 0), (size_t)nd * RR * sizeof(double), hipMemcpyDeviceToDevice, s));
  e.have_snap = true;
}

void sem_mttkrp_correct(SparseEm& e, int pos, const SemFac* f, double scale, double* out, int64_t ldOut, hipStream_t s) {
  AO_REQUIRE(e.on && e.have_snap && pos >= 0 && pos < e.nd, "internal: imputed MTTKRP without a snapshot");
  const int R = e.R, RR = R * R;
  if (e.weighted) scale *= 1.0 - e.alpha;            // the unstored entries keep (1 - alpha) of the snapshot's model
  if (e.weighted && e.alpha == 1.0) return;          // nothing is imputed off the stored set
  for (int j = 0; j < e.nd; ++j)
    if (j != pos) atb_small(e.mat(4, j), e.snapC[j].d(), e.dims[j], f[j].p, f[j].ld, e.dims[j], R, R, e.ws.d(), nullptr, s);
  sem_had_k<<<blocks_for(RR), 256, 0, s>>>(e.W(), e.mat(4, 0), RR, e.nd, pos, RR);
  AO_KERNEL_CHECK();
  gemm_small(out, ldOut, e.snapC[pos].d(), e.dims[pos], e.W(), R, e.dims[pos], R, R, 0, coef(scale), 1.0, nullptr, s);
}

double sem_pass_bytes(const SparseEm& e, bool stats, bool with_snapshot, bool writes) {
  const double nz = (double)e.nnz, nd = (double)e.nd;
  const double wbytes = e.weighted && e.wt[0].p ? nz * 8.0 : 0.0;   // the weights in the copy's order
  return nz * (4.0 * nd + 8.0) + wbytes + nz * nd * e.R * 8.0 * (stats && with_snapshot ? 2.0 : 1.0) + (writes ? nz * 8.0 : 0.0);
}

double sem_pass_flops(const SparseEm& e, bool stats, bool with_snapshot) {
  const double nz = (double)e.nnz;
  return nz * e.R * (e.nd + 1.0) + (stats ? 6.0 * nz : 0.0) + (stats && with_snapshot ? nz * e.R * 4.0 * e.nd : 0.0);
}

}  // namespace aoadmm
