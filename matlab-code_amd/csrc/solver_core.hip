// Engine: Tucker projection of a resident 3-way CP block and the core consistency of its CP model (core.h, DESIGN.md
// section 9.9).
#include "solver.h"
#include "core.h"
#include "hosteig.h"

#include <algorithm>
#include <cmath>

namespace aoadmm {

// the block of tensor p when it can be projected; every refusal happens here, before any device work
CpBlock& Engine::project_block(const char* what, int p) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  if (t.par2) throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s: tensor %d is a PARAFAC2 block", what, p));
  if (t.nmodes != 3) throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s: tensor %d has %d modes; the projection is for 3-way blocks", what, p, t.nmodes));
  if (world_ > 1) throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s is not available on a communicator of %d ranks", what, world_));
  CpBlock& b = t.blk;
  AO_REQUIRE(b.has_data, "tensor %d has no data", p);
  if (b.sparse && b.sem.on)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s: tensor %d is fitted on its stored entries only or under entry weights: its imputed tensor has no array", what, p));
  if (b.sparse && b.coo.sharded)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s: the nonzeros of tensor %d are sharded over the ranks", what, p));
  if (!b.sparse && (b.xp_ksharded || b.full0 != b.dims[0]))
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s: tensor %d is sharded over the ranks", what, p));
  AO_REQUIRE(!(b.has_mask && !b.mask_imputed), "%s: the missing entries of tensor %d were never imputed (run a solve or an EM pass first)", what, p);
  return b;
}

// M row-major with its columns padded by zeros to `ldT`
static std::vector<double> rowmajor_padded(const double* M, int64_t ld, int64_t rows, int r, int ldT) {
  std::vector<double> out((size_t)rows * ldT, 0.0);
  for (int c = 0; c < r; ++c)
    for (int64_t i = 0; i < rows; ++i) out[(size_t)i * ldT + c] = M[(size_t)c * ld + i];
  return out;
}

static void upload(DevBuf& d, const std::vector<double>& h, hipStream_t s) {
  d.alloc(h.size() * sizeof(double));
  AO_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s));
}

// Dense: one tensor pass with M[c] in place of factor c, then the core fold over T with the two other matrices.
void Engine::project_dense(CpBlock& b, const double* const* M, const int64_t* ld, const int* r, double* G) {
  const BlockCtx cx = block_ctx();
  // the matrices as the pass reads a factor: column-major, leading dimension = rows
  DevBuf dM[3];
  std::vector<double> hM[3];
  for (int n = 0; n < 3; ++n) {
    hM[n].resize((size_t)b.dims[n] * r[n]);
    for (int c = 0; c < r[n]; ++c) std::copy(M[n] + (size_t)c * ld[n], M[n] + (size_t)c * ld[n] + b.dims[n], hM[n].begin() + (size_t)c * b.dims[n]);
    upload(dM[n], hM[n], stream_);
  }
  FactorRef facs[3];
  for (int n = 0; n < 3; ++n) facs[n] = FactorRef{dM[n].d(), b.dims[n], ~(uint64_t)0, nullptr};   // a version no factor reaches
  // The contracted mode: the one that leaves the smallest T, dims[c] / r[c] largest (ties: the later mode).  Mode 1 is
  // contracted only where ensure_contraction would: on its pass copy, or by the leading-mode kernel of an fp32 block.
  auto best_mode = [&](int first) {
    int c = first;
    for (int n = first + 1; n < 3; ++n)
      if ((double)b.dims[n] * r[c] >= (double)b.dims[c] * r[n]) c = n;
    return c;
  };
  int c = best_mode(0);
  if (c == 0 && !(b.half || b.X.prec == AOADMM_PREC_F32 || ensure_pass_copy(cx, b, 0))) c = best_mode(1);
  const int pos = (c + 1) % 3, other = (c + 2) % 3;
  const int seq[3] = {pos, other, c};                  // "factor c stays unchanged longest": ensure_contraction contracts it
  b.cached_mode = -1;
  ensure_contraction(cx, b, pos, facs, r[c], true, seq, 3);
  AO_REQUIRE(b.cached_mode == c, "internal: the pass contracted mode %d, not %d", b.cached_mode + 1, c + 1);
  b.cached_mode = -1;                                  // T belongs to no factor of the model
  const ContractPlan& pl = b.plan;
  // rows of T as mttkrp_3way reads them: tensor order on X and on copies 0 and 2, (k, i) on copy 1
  int ia = c == 0 ? 1 : 0, ib = c == 2 ? 1 : 2;
  if (pl.on_copy && c == 1) { ia = 2; ib = 0; }
  const int64_t An = b.dims[ia], Bn = b.dims[ib];
  const int64_t Apad = pl.on_copy ? b.copy[c].pad : (ia == 0 ? b.X.pad0 : b.dims[1]);
  const int ldT = (int)round_up(r[ia], 16);
  DevBuf dMaT, ws;
  const std::vector<double> hMaT = rowmajor_padded(M[ia], ld[ia], An, r[ia], ldT);
  upload(dMaT, hMaT, stream_);
  ws.alloc(core_fold_ws_bytes(An, Bn, r[ia], r[ib], r[c]));
  const int64_t st[3] = {1, r[0], (int64_t)r[0] * r[1]};
  CoreFold f;
  f.T = b.T.p; f.tprec = pl.tprec; f.nchunk = pl.nchunk; f.chunk_stride = pl.trows() * pl.R; f.sRow = pl.R; f.sCol = 1;
  f.An = An; f.Apad = Apad; f.Bn = Bn; f.Ra = r[ia]; f.Rb = r[ib]; f.Rc = r[c];
  f.MaT = dMaT.d(); f.ldMaT = ldT; f.Mb = dM[ib].d(); f.ldMb = b.dims[ib];
  f.ws = ws.d(); f.G = G; f.sp = st[ia]; f.sq = st[ib]; f.sr = st[c];
  LaunchTimers& tm = timers_;
  const LaunchTimers::Pair pr = tm.begin(tm.stats[2], tm.profile && tm.profile_reductions, stream_);
  core_fold(f, stream_);
  tm.end(tm.stats[2], pr, stream_, (double)pl.t_bytes(), core_fold_flops(f));
  AO_HIP(hipStreamSynchronize(stream_));               // the host copies of the matrices go with this frame
}

// Plain sparse (unstored entries are zero): with a the output mode and (m1, m2) the two others, Rm = max(r[m1], r[m2])
// MTTKRPs.  Rotation s pairs column (t + s) mod Rm of M[m1] with column t of M[m2]:
//   Y_s(i, t) = sum_nnz x * M[m1](j, (t + s) mod Rm) * M[m2](k, t),   G(p, (t + s) mod Rm, t) = sum_i M[a](i, p) Y_s(i, t)
void Engine::project_sparse(CpBlock& b, const double* const* M, const int64_t* ld, const int* r, double* G) {
  int a = 0;                                           // the largest rank leaves the fewest rotations
  for (int n = 1; n < 3; ++n)
    if (r[n] > r[a]) a = n;
  const int m1 = a == 0 ? 1 : 0, m2 = a == 2 ? 1 : 2;
  const int Rm = std::max(r[m1], r[m2]);
  const int64_t Ia = b.dims[a], I1 = b.dims[m1], I2 = b.dims[m2];
  // M[m1] row-major with its Rm padded columns written twice, so that a rotation is an offset; M[m2] row-major, padded
  std::vector<double> h1((size_t)I1 * 2 * Rm, 0.0);
  for (int c = 0; c < r[m1]; ++c)
    for (int64_t j = 0; j < I1; ++j) h1[(size_t)j * 2 * Rm + c] = h1[(size_t)j * 2 * Rm + Rm + c] = M[m1][(size_t)c * ld[m1] + j];
  const std::vector<double> h2 = rowmajor_padded(M[m2], ld[m2], I2, r[m2], Rm);
  const int ldT = (int)round_up(r[a], 16);
  const std::vector<double> hMaT = rowmajor_padded(M[a], ld[a], Ia, r[a], ldT);
  DevBuf d1, d2, dMaT, Y, ws;
  upload(d1, h1, stream_); upload(d2, h2, stream_); upload(dMaT, hMaT, stream_);
  Y.alloc((size_t)Ia * Rm * sizeof(double));
  ws.alloc(core_fold_ws_bytes(Ia, 1, r[a], r[m1], r[m2]));
  const int64_t st[3] = {1, r[0], (int64_t)r[0] * r[1]};
  CoreFold f;
  f.T = Y.p; f.tprec = AOADMM_PREC_F64; f.nchunk = 1; f.chunk_stride = 0; f.sRow = 1; f.sCol = Ia;   // Y is column-major
  f.An = Ia; f.Apad = Ia; f.Bn = 1; f.Ra = r[a]; f.Rb = r[m1]; f.Rc = r[m2];
  f.MaT = dMaT.d(); f.ldMaT = ldT; f.Mb = nullptr; f.ldMb = 0;
  f.ws = ws.d(); f.G = G; f.sp = st[a]; f.sq = st[m1]; f.sr = st[m2];
  LaunchTimers& tm = timers_;
  for (int s = 0; s < Rm; ++s) {
    const CooFactor cf[2] = {CooFactor{d1.d() + s, (int64_t)2 * Rm, 1}, CooFactor{d2.d(), (int64_t)Rm, 1}};
    const LaunchTimers::Pair pr = tm.begin(tm.stats[3], tm.profile, stream_);
    coo_mttkrp(b.coo, a, cf, Rm, 1.0, Y.d(), Ia, stream_);
    tm.end(tm.stats[3], pr, stream_, coo_mttkrp_bytes(b.coo, a, Rm), coo_mttkrp_flops(b.coo, Rm));
    core_fold_rotated(f, s, Rm, stream_);
  }
  AO_HIP(hipStreamSynchronize(stream_));
}

void Engine::project(int p, const double* const* M, const int64_t* ld, const int* r, double* core_host) {
  CpBlock& b = project_block("aoadmm_resident_project", p);
  AO_REQUIRE(M != nullptr && ld != nullptr && r != nullptr && core_host != nullptr, "null M / ld / r / core");
  for (int n = 0; n < 3; ++n) {
    AO_REQUIRE(r[n] >= 1 && r[n] <= kMaxRank, "r[%d] = %d outside 1..%d", n, r[n], kMaxRank);
    AO_REQUIRE(M[n] != nullptr, "M[%d] is null", n);
    AO_REQUIRE(ld[n] >= b.dims[n], "ld[%d] = %lld is smaller than the %lld rows of mode %d", n, (long long)ld[n], (long long)b.dims[n], n + 1);
  }
  AO_HIP(hipSetDevice(device_));
  const size_t E = (size_t)r[0] * r[1] * r[2];
  DevBuf G;
  G.alloc(E * sizeof(double));
  if (b.sparse) project_sparse(b, M, ld, r, G.d());
  else project_dense(b, M, ld, r, G.d());
  // (the output is written last: a refusal above leaves it untouched)
  AO_HIP(hipMemcpyAsync(core_host, G.p, E * sizeof(double), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

// M = F (F'F)^+ from the eigendecomposition of the R x R Gram matrix; eigenvalues below R 2^-52 lambda_max count as zero
static bool pinv_t(const std::vector<double>& F, int64_t rows, int R, std::vector<double>& M) {
  std::vector<double> Gm((size_t)R * R, 0.0), w, U;
  for (int a = 0; a < R; ++a)
    for (int c = a; c < R; ++c) {
      double s = 0.0;
      for (int64_t i = 0; i < rows; ++i) s += F[(size_t)a * rows + i] * F[(size_t)c * rows + i];
      Gm[(size_t)a + (size_t)R * c] = Gm[(size_t)c + (size_t)R * a] = s;
    }
  host_sym_eig(R, Gm, w, U);
  double wmax = 0.0;
  for (int k = 0; k < R; ++k) wmax = std::max(wmax, w[(size_t)k]);
  const double cut = R * std::ldexp(1.0, -52) * wmax;
  bool deficient = false;
  std::vector<double> P((size_t)R * R, 0.0);           // (F'F)^+ = U diag(1 / w) U' over the kept eigenvalues
  for (int k = 0; k < R; ++k) {
    if (!(w[(size_t)k] > cut)) { deficient = true; continue; }
    const double inv = 1.0 / w[(size_t)k];
    for (int c = 0; c < R; ++c)
      for (int a = 0; a < R; ++a) P[(size_t)a + (size_t)R * c] += U[(size_t)a + (size_t)R * k] * inv * U[(size_t)c + (size_t)R * k];
  }
  M.assign((size_t)rows * R, 0.0);
  for (int c = 0; c < R; ++c)
    for (int a = 0; a < R; ++a) {
      const double pac = P[(size_t)a + (size_t)R * c];
      for (int64_t i = 0; i < rows; ++i) M[(size_t)c * rows + i] += F[(size_t)a * rows + i] * pac;
    }
  return deficient;
}

void Engine::core_consistency(int p, double* cc, double* core_host, int* rank_deficient) {
  CpBlock& b = project_block("aoadmm_resident_core_consistency", p);
  AO_REQUIRE(cc != nullptr, "null cc");
  const TensorInfo& t = tensors_[p];
  const int R = modes_[t.modes[0]].R;
  AO_REQUIRE(R >= 1 && R <= kMaxRank, "tensor %d: rank %d outside 1..%d", p, R, kMaxRank);
  AO_HIP(hipSetDevice(device_));
  std::vector<double> F[3], Mh[3];
  for (int n = 0; n < 3; ++n) {
    const ModeInfo& mi = modes_[t.modes[n]];
    AO_REQUIRE(mi.has_fac, "G.fac{%d} missing", t.modes[n] + 1);
    AO_REQUIRE(mi.R == R && mi.rows == b.dims[n], "internal: mode %d of tensor %d is %lld x %d", n + 1, p, (long long)mi.rows, mi.R);
    F[n].resize((size_t)mi.rows * R);
    AO_HIP(hipMemcpyAsync(F[n].data(), mi.fac.p, F[n].size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
  }
  AO_HIP(hipStreamSynchronize(stream_));
  bool deficient = false;
  for (int n = 0; n < 3; ++n) deficient = pinv_t(F[n], b.dims[n], R, Mh[n]) || deficient;
  const double* M[3] = {Mh[0].data(), Mh[1].data(), Mh[2].data()};
  const int64_t ld[3] = {b.dims[0], b.dims[1], b.dims[2]};
  const int r[3] = {R, R, R};
  std::vector<double> core((size_t)R * R * R);
  project(p, M, ld, r, core.data());
  double ss = 0.0;
  for (int k = 0; k < R; ++k)
    for (int j = 0; j < R; ++j)
      for (int i = 0; i < R; ++i) {
        const double d = core[(size_t)i + (size_t)R * j + (size_t)R * R * k] - (i == j && j == k ? 1.0 : 0.0);
        ss += d * d;
      }
  *cc = 100.0 * (1.0 - ss / R);
  if (core_host) std::copy(core.begin(), core.end(), core_host);
  if (rank_deficient) *rank_deficient = deficient ? 1 : 0;
}

}  // namespace aoadmm
