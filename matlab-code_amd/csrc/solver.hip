// Engine implementation: see solver.h.  Constructor and destructor, model definition, data upload / synthesis /
// masks / EM pass, state get/set, kernel statistics and the resident_* entries.  This file launches no kernel of its own.
#include "solver.h"
#include "em.h"
#include "hosteig.h"
#include "sparse_nvecs.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace aoadmm {

Engine::Engine(int device) : device_(device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    throw Error(AOADMM_ERR_HIP, "no HIP device available: this library has no CPU fallback");
  if (device < 0 || device >= n) throw Error(AOADMM_ERR_INVALID, fmt("device %d out of range [0,%d)", device, n));
  AO_HIP(hipSetDevice(device));
  AO_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  AO_HIP(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
  AO_HIP(hipEventCreateWithFlags(&side_ev_, hipEventDisableTiming));
  redws_.alloc(4096 * sizeof(double));
  ones_.alloc(sizeof(double));
  const double one = 1.0;
  AO_HIP(hipMemcpy(ones_.p, &one, sizeof one, hipMemcpyHostToDevice));
}

Engine::~Engine() {
  (void)hipSetDevice(device_);
  for (auto& ks : timers_.stats)
    for (auto& pr : ks.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (hipEvent_t e : timers_.pool) (void)hipEventDestroy(e);
  comm_release();
  if (side_ev_) (void)hipEventDestroy(side_ev_);
  if (side_) (void)hipStreamDestroy(side_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

// ---------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------
void Engine::check_mode(int m) const {
  AO_REQUIRE(m >= 0 && m < n_modes_, "mode %d out of range [0,%d)", m, n_modes_);
}

void Engine::model_begin(int n_modes, int n_tensors, int n_couplings) {
  AO_REQUIRE(n_modes > 0 && n_tensors > 0 && n_couplings >= 0, "model_begin: bad counts");
  AO_HIP(hipSetDevice(device_));
  n_modes_ = n_modes; n_tensors_ = n_tensors; n_couplings_ = n_couplings;
  modes_.clear(); tensors_.clear(); couplings_.clear();
  modes_.resize(n_modes); tensors_.resize(n_tensors); couplings_.resize(n_couplings);
  model_done_ = false;
  has_ridge_ = false;
  allow_xp_ = true;                                   // options.hip.no_permuted_copy of an earlier solve does not outlive its model
  best_ = BestKeep();                                 // aoadmm_heldout_keep_best belongs to the model, as the lists do
  track_ = RankTrack();                               // and so does aoadmm_rank_track
  rank_iters_.clear();
  rank_best_iter_ = -1;
}

void Engine::set_mode(int mode, int64_t rows, int rank) {
  check_mode(mode);
  AO_REQUIRE(rows > 0 && rank > 0 && rank <= kMaxRank, "mode %d: rows=%lld rank=%d invalid (rank <= %d)", mode,
             (long long)rows, rank, kMaxRank);
  ModeInfo& mi = modes_[mode];
  mi.defined = true; mi.rows = rows; mi.R = rank; mi.slabs = false;
}

void Engine::set_mode_slabs(int mode, int K, const int64_t* rows_k, int rank) {
  check_mode(mode);
  AO_REQUIRE(K > 0 && rank > 0 && rank <= kMaxRank, "slab mode %d: bad K/rank", mode);
  ModeInfo& mi = modes_[mode];
  mi.defined = true; mi.slabs = true; mi.K = K; mi.R = rank;
  mi.rows_k.assign(rows_k, rows_k + K);
  mi.off_k.assign(K + 1, 0);
  for (int k = 0; k < K; ++k) {
    AO_REQUIRE(rows_k[k] > 0, "slab %d has no rows", k);
    mi.off_k[k + 1] = mi.off_k[k] + rows_k[k];
  }
  mi.rows = mi.off_k[K];
}

void Engine::add_cp(int p, int n, const int* modes, double weight) {
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(n >= 2 && n <= 8, "CP block needs 2..8 modes");
  TensorInfo& t = tensors_[p];
  t.defined = true; t.par2 = false; t.nmodes = n; t.weight = weight;
  for (int i = 0; i < n; ++i) {
    check_mode(modes[i]);
    AO_REQUIRE(modes_[modes[i]].defined && !modes_[modes[i]].slabs, "mode %d undefined or slab-valued", modes[i]);
    AO_REQUIRE(modes_[modes[i]].tensor < 0, "mode %d already belongs to tensor %d", modes[i], modes_[modes[i]].tensor);
    t.modes[i] = modes[i];
    modes_[modes[i]].tensor = p;
    modes_[modes[i]].pos = i;
    AO_REQUIRE(modes_[modes[i]].R == modes_[modes[0]].R, "modes of tensor %d disagree on the rank", p);
  }
}

void Engine::set_constraint(int mode, int type, const double* params, int np, const double* Lmat) {
  check_mode(mode);
  ModeInfo& mi = modes_[mode];
  AO_REQUIRE(type >= AOADMM_C_NONE && type <= AOADMM_C_TPARAFAC2, "unknown constraint id %d", type);
  mi.constrained = type != AOADMM_C_NONE;
  mi.prox = ProxSpec();
  mi.prox.type = type;
  if (np > 0) mi.prox.p0 = params[0];
  if (np > 1) mi.prox.p1 = params[1];
  auto need = [&](int n) { AO_REQUIRE(np >= n, "constraint %d on mode %d needs %d parameter(s)", type, mode, n); };
  switch (type) {
    case AOADMM_C_BOX: need(2); break;
    case AOADMM_C_SIMPLEX_COL: case AOADMM_C_SIMPLEX_ROW: case AOADMM_C_UNIMODAL: case AOADMM_C_L1_BALL:
    case AOADMM_C_L2_BALL: case AOADMM_C_NONNEG_L2_BALL: case AOADMM_C_L1_REG: case AOADMM_C_L0_REG:
    case AOADMM_C_L2_REG: case AOADMM_C_RIDGE: case AOADMM_C_GL_SMOOTH: case AOADMM_C_TV: need(1); break;
    case AOADMM_C_TPARAFAC2: need(1); break;
    case AOADMM_C_QUADRATIC:
      need(1);
      AO_REQUIRE(mi.defined, "quadratic regularization: define the mode before its constraint");
      if (mi.slabs) throw Error(AOADMM_ERR_UNSUPPORTED, "quadratic regularization on the PARAFAC2 B_k mode is not in the device path");
      AO_REQUIRE(Lmat != nullptr, "quadratic regularization on mode %d needs its matrix L (constraints{m}{3})", mode + 1);
      AO_HIP(hipSetDevice(device_));
      mi.quad.build(Lmat, mi.rows, stream_);
      mi.quad.attach(mi.prox);
      break;
    default: break;
  }
}

static void upload_small(DevBuf& b, const double* host, int64_t n, hipStream_t s) {
  b.ensure((size_t)n * sizeof(double));
  AO_HIP(hipMemcpyAsync(b.p, host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
  AO_HIP(hipStreamSynchronize(s));
}

static void upload_with_transpose(DevBuf& b, DevBuf& bt, const double* host, int64_t r, int64_t c, hipStream_t s) {
  std::vector<double> t((size_t)r * c);
  for (int64_t j = 0; j < c; ++j)
    for (int64_t i = 0; i < r; ++i) t[(size_t)j + (size_t)c * i] = host[(size_t)i + (size_t)r * j];
  upload_small(b, host, r * c, s);
  upload_small(bt, t.data(), r * c, s);
}

void Engine::set_coupling(int mode, int coupling, const double* H, int64_t hr, int64_t hc, const double* H2,
                          int64_t h2r, int64_t h2c) {
  check_mode(mode);
  AO_REQUIRE(coupling >= -1 && coupling < n_couplings_, "coupling id %d out of range", coupling);
  ModeInfo& mi = modes_[mode];
  mi.coupling = coupling;
  mi.hr = mi.hc = mi.h2r = mi.h2c = 0;
  mi.H_host.clear();
  if (H && hr > 0 && hc > 0) {
    upload_with_transpose(mi.H, mi.Ht, H, hr, hc, stream_);
    mi.hr = hr; mi.hc = hc;
    mi.H_host.assign(H, H + (size_t)hr * hc);
  }
  if (H2 && h2r > 0 && h2c > 0) { upload_with_transpose(mi.H2, mi.H2t, H2, h2r, h2c, stream_); mi.h2r = h2r; mi.h2c = h2c; }
}

void Engine::set_coupling_type(int coupling, int type) {
  AO_REQUIRE(coupling >= 0 && coupling < n_couplings_, "coupling id %d out of range", coupling);
  AO_REQUIRE(type >= 0 && type <= 5, "coupling type %d invalid", type);
  couplings_[coupling].type = type;
}

void Engine::set_ridge(const double* ridge) {
  has_ridge_ = ridge != nullptr;
  for (int m = 0; m < n_modes_; ++m) modes_[m].ridge = ridge ? ridge[m] : 0.0;
}

void Engine::check_model() const {
  for (int m = 0; m < n_modes_; ++m) {
    AO_REQUIRE(modes_[m].defined, "mode %d has no size", m);
    AO_REQUIRE(modes_[m].tensor >= 0, "mode %d belongs to no tensor (Mismatch between size and modes inputs)", m);
  }
  for (int p = 0; p < n_tensors_; ++p) AO_REQUIRE(tensors_[p].defined, "tensor %d undefined", p);
  for (int m = 0; m < n_modes_; ++m) {
    const ModeInfo& mi = modes_[m];
    if (mi.constrained && mi.prox.type == AOADMM_C_TPARAFAC2)       // cmtf_AOADMM.m:33-41
      AO_REQUIRE(tensors_[mi.tensor].par2 && mi.pos == 1, "The tPARAFAC2 constraint can only be impsed on the second mode of a PARAFAC2 model");
    if (!tensors_[mi.tensor].par2) continue;
    if (mi.pos == 1 && mi.constrained && mi.prox.type == AOADMM_C_TPARAFAC2)
      for (int k = 1; k < mi.K; ++k)
        AO_REQUIRE(mi.rows_k[k] == mi.rows_k[0], "tPARAFAC2 needs slabs of equal size (t_smoothness_prox.m adds B_k matrices)");
    if (mi.pos == 1) {
      // check_data_input.m:33-35
      AO_REQUIRE(mi.coupling < 0, "Coupling in 2. mode (the varying mode) of Parafac2 decomposition not supported.");
    }
  }
}

void Engine::shape_coupling(int c) {
  CouplingInfo& ci = couplings_[c];
  AO_REQUIRE(ci.type >= 0, "coupling %d has no type (Mismatch between number of couplings and coupling types)", c);
  ci.modes.clear();
  for (int m = 0; m < n_modes_; ++m)
    if (modes_[m].coupling == c) ci.modes.push_back(m);
  AO_REQUIRE(!ci.modes.empty(), "coupling %d couples no mode", c);
  AO_REQUIRE(ci.modes.size() <= 8, "more than 8 modes in one coupling");
  for (int m : ci.modes)
    if (tensors_[modes_[m].tensor].par2 && modes_[m].pos == 2 && ci.type == 5)
      AO_REQUIRE(modes_[m].hr <= modes_[m].rows, "coupling type 5 of a PARAFAC2 C mode: Delta has more rows than the mode (cmtf_fun_AOADMM.m:1049-1051 indexes rho by Delta's row)");
  if (ci.type == 4 || ci.type == 5) {       // :945-961, :1034-1052 keep one PARAFAC2 term apart (AAA); two would overwrite each other
    int npc = 0;
    for (int m : ci.modes) npc += (tensors_[modes_[m].tensor].par2 && modes_[m].pos == 2) ? 1 : 0;
    if (npc > 1) throw Error(AOADMM_ERR_UNSUPPORTED, fmt("coupling type %d with more than one PARAFAC2 C mode is not supported", ci.type));
  }
  const ModeInfo& m0 = modes_[ci.modes[0]];
  auto need_H = [&](int m) { AO_REQUIRE(modes_[m].hr > 0, "Coupling matrix for mode %d is missing.", m + 1); };
  switch (ci.type) {
    case 0:                                   // C = Delta  (check_data_input.m:48-61)
      ci.rows = m0.rows; ci.cols = m0.R;
      for (int m : ci.modes) {
        AO_REQUIRE(modes_[m].rows == m0.rows, "Coupled factor matrices of mode %d and mode %d need to have same number of rows.", ci.modes[0] + 1, m + 1);
        AO_REQUIRE(modes_[m].R == m0.R, "Coupled factor matrices of mode %d and mode %d need to have same number of components/columns.", ci.modes[0] + 1, m + 1);
        modes_[m].img_rows = modes_[m].rows; modes_[m].img_cols = modes_[m].R;
      }
      break;
    case 1:                                   // H*C = Delta : H is (rows_Delta x rows_m)  (:62-80)
      need_H(ci.modes[0]);
      ci.rows = m0.hr; ci.cols = m0.R;
      for (int m : ci.modes) {
        need_H(m);
        AO_REQUIRE(modes_[m].hc == modes_[m].rows, "Mismatch between sz and number of columns of coupling matrix for mode %d.", m + 1);
        AO_REQUIRE(modes_[m].hr == ci.rows, "Coupling transformation matrices need to have same number of rows for mode %d and mode %d.", ci.modes[0] + 1, m + 1);
        AO_REQUIRE(modes_[m].R == m0.R, "Coupled factor matrices of mode %d and mode %d need to have same number of components/columns.", ci.modes[0] + 1, m + 1);
        modes_[m].img_rows = ci.rows; modes_[m].img_cols = modes_[m].R;
      }
      break;
    case 2:                                   // C*H = Delta : H is (R_m x cols_Delta)  (:81-98)
      need_H(ci.modes[0]);
      ci.rows = m0.rows; ci.cols = m0.hc;
      for (int m : ci.modes) {
        need_H(m);
        AO_REQUIRE(modes_[m].hr == modes_[m].R, "Mismatch between number of components and number of rows of coupling matrix for mode %d.", m + 1);
        AO_REQUIRE(modes_[m].hc == ci.cols, "Coupling transformation matrices need to have same number of columns for mode %d and mode %d.", ci.modes[0] + 1, m + 1);
        AO_REQUIRE(modes_[m].rows == ci.rows, "Coupled factor matrices of mode %d and mode %d need to have same number of rows.", ci.modes[0] + 1, m + 1);
        modes_[m].img_rows = ci.rows; modes_[m].img_cols = ci.cols;
      }
      AO_REQUIRE(ci.cols <= kMaxRank, "coupling type 2: Delta has more than %d columns", kMaxRank);
      break;
    case 3:                                   // C = H*Delta : H is (rows_m x rows_Delta)  (:99-114)
      need_H(ci.modes[0]);
      ci.rows = m0.hc; ci.cols = m0.R;
      for (int m : ci.modes) {
        need_H(m);
        AO_REQUIRE(modes_[m].hr == modes_[m].rows, "Mismatch between sz and number of rows of coupling matrix for mode %d.", m + 1);
        AO_REQUIRE(modes_[m].hc == ci.rows, "Coupling transformation matrices need to have same number of columns for mode %d and mode %d.", ci.modes[0] + 1, m + 1);
        AO_REQUIRE(modes_[m].R == m0.R, "Coupled factor matrices of mode %d and mode %d need to have same number of components/columns.", ci.modes[0] + 1, m + 1);
        modes_[m].img_rows = modes_[m].rows; modes_[m].img_cols = modes_[m].R;
      }
      break;
    case 4:                                   // C = Delta*H : H is (cols_Delta x R_m)
      need_H(ci.modes[0]);
      ci.rows = m0.rows; ci.cols = m0.hr;
      for (int m : ci.modes) {
        need_H(m);
        AO_REQUIRE(modes_[m].rows == ci.rows && modes_[m].hr == ci.cols && modes_[m].hc == modes_[m].R,
                   "coupling type 4: transformation matrix of mode %d has the wrong shape", m + 1);
        modes_[m].img_rows = modes_[m].rows; modes_[m].img_cols = modes_[m].R;
      }
      AO_REQUIRE(ci.cols <= kMaxRank, "coupling type 4: Delta has more than %d columns", kMaxRank);
      break;
    default:                                  // 5: H*C = Delta*H2 : H (rows_Delta x rows_m), H2 (cols_Delta x R_m)  (:125-140)
      need_H(ci.modes[0]);
      AO_REQUIRE(m0.h2r > 0, "Coupling matrix H2 for mode %d is missing.", ci.modes[0] + 1);
      ci.rows = m0.hr; ci.cols = m0.h2r;
      for (int m : ci.modes) {
        need_H(m);
        AO_REQUIRE(modes_[m].h2r > 0, "Coupling matrix H2 for mode %d is missing.", m + 1);
        AO_REQUIRE(modes_[m].hc == modes_[m].rows && modes_[m].hr == ci.rows && modes_[m].h2r == ci.cols &&
                   modes_[m].h2c == modes_[m].R, "coupling type 5: transformation matrices of mode %d have the wrong shape", m + 1);
        modes_[m].img_rows = ci.rows; modes_[m].img_cols = modes_[m].R;
      }
      AO_REQUIRE(ci.cols <= kMaxRank, "coupling type 5: Delta has more than %d columns", kMaxRank);
      break;
  }
}

void Engine::precompute_coupling(int c) {
  const CouplingInfo& ci = couplings_[c];
  for (int m : ci.modes) {
    ModeInfo& mi = modes_[m];
    if (ci.type == 2) {                       // H*H' (R x R) for the system matrix (:314)
      std::vector<double> hh((size_t)mi.R * mi.R, 0.0);
      for (int a = 0; a < mi.R; ++a)
        for (int b2 = 0; b2 < mi.R; ++b2) {
          double acc = 0.0;
          for (int64_t c2 = 0; c2 < mi.hc; ++c2) acc += mi.H_host[(size_t)a + (size_t)mi.hr * c2] * mi.H_host[(size_t)b2 + (size_t)mi.hr * c2];
          hh[(size_t)a + (size_t)mi.R * b2] = acc;
        }
      upload_small(mi.HHt, hh.data(), (int64_t)mi.R * mi.R, stream_);
    }
    if (ci.type == 1 || ci.type == 5) {       // H'*H = U diag(lam) U' once: the Sylvester solves reuse it (:288, :377)
      const int64_t n = mi.rows;
      if (n > 4096) throw Error(AOADMM_ERR_UNSUPPORTED, "coupling types 1/5: modes beyond 4096 rows are not diagonalised on the host");
      std::vector<double> hth((size_t)n * n, 0.0), lam, U;
      for (int64_t a = 0; a < n; ++a)
        for (int64_t b2 = a; b2 < n; ++b2) {
          double acc = 0.0;
          for (int64_t q = 0; q < mi.hr; ++q) acc += mi.H_host[(size_t)q + (size_t)mi.hr * a] * mi.H_host[(size_t)q + (size_t)mi.hr * b2];
          hth[(size_t)a + (size_t)n * b2] = acc; hth[(size_t)b2 + (size_t)n * a] = acc;
        }
      AO_REQUIRE(host_sym_eig(n, hth, lam, U) >= 0, "eigendecomposition of H'*H (mode %d) did not converge", m + 1);
      std::vector<double> Ut((size_t)n * n);
      for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < n; ++i) Ut[(size_t)j + (size_t)n * i] = U[(size_t)i + (size_t)n * j];
      upload_small(mi.eU, U.data(), n * n, stream_);
      upload_small(mi.eUt, Ut.data(), n * n, stream_);
      upload_small(mi.eLam, lam.data(), n, stream_);
    }
  }
}

// one arena for what the host reads back per outer iteration, so that one copy fetches it
void Engine::alloc_readback() {
  std::vector<int> slabs(n_tensors_, 0);
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].par2) slabs[p] = tensors_[p].p2.K;
  arena_.build(n_modes_, n_tensors_, n_couplings_, slabs);
  for (int p = 0; p < n_tensors_; ++p)            // views of the previous arena go before it does
    if (tensors_[p].par2) { tensors_[p].p2.res.release(); tensors_[p].p2.q.release(); tensors_[p].p2.regv.release(); }
  readback_.alloc(arena_.bytes);
  AO_HIP(hipMemsetAsync(readback_.p, 0, readback_.bytes, stream_));
  dev_ = arena_.at(readback_.p);
  for (int p = 0; p < n_tensors_; ++p) {
    if (!tensors_[p].par2) continue;
    Par2Block& b = tensors_[p].p2;
    b.res.view(dev_.p2_res(p), (size_t)(b.K + 1) * 8);
    b.q.view(dev_.p2_q(p), (size_t)b.K * kSlabSums * 8);
    b.regv.view(dev_.p2_regv(p), (size_t)b.K * 8);
  }
}

void Engine::model_end() {
  check_model();
  for (int c = 0; c < n_couplings_; ++c) {
    shape_coupling(c);
    precompute_coupling(c);
  }
  alloc_readback();
  AO_HIP(hipStreamSynchronize(stream_));
  model_done_ = true;
}

// ---------------------------------------------------------------------------
// data
// ---------------------------------------------------------------------------
// AOADMM_PREC_F16 is for dense 3-way CP blocks given whole, on one engine or on the ranks of a communicator (where the
// upload is a collective: block_make_half).  The verdict depends on the model and on how the context was made only, so
// every rank of a communicator reaches the same one.
void Engine::require_half_ok(const TensorInfo& t, int p, bool row_block) const {
  if (row_block)
    throw Error(AOADMM_ERR_UNSUPPORTED, "AOADMM_PREC_F16 is not available in aoadmm_tensor_upload_rows: the block's scale comes from the whole tensor");
  if (multi_member_)
    throw Error(AOADMM_ERR_UNSUPPORTED, "AOADMM_PREC_F16 is not available on a multi-device context (aoadmm_create_multi): use one context per rank and a communicator");
  if (t.nmodes != 3)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("AOADMM_PREC_F16 is for 3-way CP blocks: tensor %d has %d modes", p, t.nmodes));
}

void Engine::tensor_storage_info(int p, int* precision, double* scale, int64_t* resident_bytes) {
  require_usable();
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  const TensorInfo& t = tensors_[p];
  const CpBlock& b = t.blk;
  const bool dense_cp = !t.par2 && !b.sparse;
  AO_REQUIRE(t.par2 || b.has_data, "tensor %d has no data", p);
  if (precision) *precision = !dense_cp ? AOADMM_PREC_F64 : (b.half ? AOADMM_PREC_F16 : b.X.prec);
  if (scale) *scale = dense_cp && b.half ? b.scale : 1.0;
  if (resident_bytes) {
    int64_t n = 0;
    if (dense_cp) {
      for (const DevBuf* d : {&b.X.data, &b.Xt.data, &b.copy[0].buf, &b.copy[1].buf, &b.copy[2].buf, &b.mask, &b.maskT,
                              &b.X0, &b.Wt, &b.X0t, &b.WtT})
        if (d->p) n += (int64_t)d->bytes;
      n += b.mlist.resident_bytes();       // a marked block: 4 N bytes per missing entry and the teams' partial sums
    } else if (!t.par2) {            // the per-mode copies of the nonzeros this rank holds: N (4 N + 8) bytes each
      for (int m = 0; m < b.coo.nd; ++m)
        for (const DevBuf* d : {&b.coo.mode[m].row, &b.coo.mode[m].oidx, &b.coo.mode[m].val})
          if (d->p) n += (int64_t)d->bytes;
      n += sem_resident_bytes(b.sem);      // observed-only: 8 more bytes per nonzero per copy (16 with entry weights) and the factor snapshots
    }
    *resident_bytes = n;
  }
}

void Engine::tensor_upload(int p, const double* data, int prec, int64_t row0, int64_t local_rows) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(!t.par2, "tensor %d is PARAFAC2: use aoadmm_par2_slab_upload", p);
  AO_REQUIRE(local_rows < 0 || !t.blk.sparse, "tensor %d holds sparse data: a row block cannot replace it (use aoadmm_tensor_upload)", p);
  if (prec == AOADMM_PREC_F16) require_half_ok(t, p, local_rows >= 0);   // refused before anything of the block changes
  if (t.blk.sparse) { t.blk.coo.clear(); t.blk.sem.clear(); t.blk.sparse = false; }   // a dense upload replaces the sparse form
  AO_HIP(hipSetDevice(device_));
  const BlockCtx cx = block_ctx();
  int64_t dims[8];
  for (int i = 0; i < t.nmodes; ++i) dims[i] = modes_[t.modes[i]].rows;
  if (local_rows < 0) {            // full array given: every rank keeps its block of rows
    int64_t I = dims[0];
    int64_t per = cdiv(I, world_);
    row0 = std::min<int64_t>(I, per * rank_);
    local_rows = std::min<int64_t>(I, row0 + per) - row0;
    // the same verdict on every rank (a rank that throws alone leaves the others waiting in the next collective)
    AO_REQUIRE(per * (world_ - 1) < I, "tensor %d: first mode of %lld rows cannot be split over %d ranks (the last rank would own no rows)",
               p, (long long)I, world_);
    if (world_ == 1) {
      t.blk.clear_weights();             // past the last refusal: new data makes a plain block again
      block_upload(cx, t.blk, t.nmodes, dims, data, prec, 0, I);
    } else {
      int64_t ncols = 1;
      for (int i = 1; i < t.nmodes; ++i) ncols *= dims[i];
      std::vector<double> blk((size_t)local_rows * ncols);
      for (int64_t c = 0; c < ncols; ++c)
        std::memcpy(&blk[(size_t)c * local_rows], data + c * I + row0, (size_t)local_rows * sizeof(double));
      t.blk.clear_weights();
      block_upload(cx, t.blk, t.nmodes, dims, blk.data(), prec, row0, local_rows, data);
    }
  } else {
    t.blk.clear_weights();
    block_upload(cx, t.blk, t.nmodes, dims, data, prec, row0, local_rows);
  }
  t.normsq_valid = false;
}

// Z.object{p} as a sptensor / sparse matrix (sparse.h): the block keeps the coalesced nonzeros, one sorted copy per
// mode, and drops whatever dense form it had.  Replicated on every rank of a communicator, or with `shard` cut over the
// ranks (coo_keep_share: the whole list is coalesced first, so the sharded model is the same model; every rank passes
// the whole list and reaches the same verdict on it).  shard without peers is the replicated upload.
void Engine::tensor_upload_coo(int p, int64_t nnz, const int64_t* subs, const double* vals, bool shard) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(!t.par2, "tensor %d is PARAFAC2: sparse slabs go through aoadmm_par2_slab_upload_coo", p);
  AO_REQUIRE(t.nmodes >= 2 && t.nmodes <= kCooMaxModes, "tensor %d: order %d unsupported for sparse data", p, t.nmodes);
  int64_t dims[8];
  for (int i = 0; i < t.nmodes; ++i) dims[i] = modes_[t.modes[i]].rows;
  AO_HIP(hipSetDevice(device_));
  CooBlock coo;
  coo_build(coo, t.nmodes, dims, nnz, subs, vals, stream_);     // validates before anything of the old form is dropped
  if (shard && world_ > 1) coo_keep_share(coo, rank_, world_, stream_);
  CpBlock& b = t.blk;
  drop_pass_copies(b);
  b.X.data.release(); b.Xt.data.release();
  b.emkr.release(); b.emkr2.release(); b.T.release(); b.frag.release(); b.scratch.release(); b.ft.release();
  b.tmpA.release(); b.tmpB.release(); b.mask.release(); b.maskT.release(); b.clear_weights();
  for (int i = 0; i < 2; ++i) { b.own[i].release(); b.own_bytes[i] = 0; b.own_row0[i] = -1; }
  b.coo = std::move(coo);
  b.sem.clear();                                       // a new upload is a plain block again
  b.sparse = true;
  b.nd = t.nmodes;
  for (int i = 0; i < t.nmodes; ++i) b.dims[i] = dims[i];
  b.full0 = dims[0]; b.row0 = 0;
  b.has_mask = false;
  b.reset_derived();
  t.normsq_valid = false;
}

double Engine::tensor_normsq(int p) {
  require_usable();
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  // test hook (tests/test_gpu_sharded.py): AOADMM_FAULT_INJECT=normsq:<rank> makes that rank fail ALONE in front of
  // a collective, the situation MultiCtx::run's abort path exists for (a device error or OOM on one GPU)
  if (const char* fi = getenv("AOADMM_FAULT_INJECT"))
    if (std::strncmp(fi, "normsq:", 7) == 0 && std::atoi(fi + 7) == rank_ && world_ > 1)
      throw Error(AOADMM_ERR_HIP, "injected fault (AOADMM_FAULT_INJECT)");
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(t.blk.has_data, "tensor %d has no data", p);
  if (!t.normsq_valid) {
    AO_HIP(hipSetDevice(device_));
    DevBuf ws;
    ws.alloc(1024 * sizeof(double) + 64);
    double* slot = dev_.scratch();
    if (t.masked()) {
      // ||miss .* X||^2 (cmtf_AOADMM.m:133-148): the observed-entry sum of squares of a statistics-only EM pass
      // (needs factors on the device: solve() calls this after the state checks)
      em_pass_enqueue(p, 0);
      double h4[kEmStats];
      AO_HIP(hipMemcpyAsync(h4, dev_.em(p), sizeof h4, hipMemcpyDeviceToHost, stream_));
      AO_HIP(hipStreamSynchronize(stream_));
      t.normsq = h4[kEmObsX2];
      t.normsq_valid = true;
      return t.normsq;
    }
    if (t.par2 && t.p2.sparse) {   // the coalesced values of all slabs; every rank holds all of them
      tensor_sumsq(slot, t.p2.sp.coo.mode[0].val.p, AOADMM_PREC_F64, t.p2.sp.coo.nnz, ws.d(), stream_);
    } else if (t.par2) {   // sum_k ||X_k||_F^2  (cmtf_AOADMM.m:145-155)
      tensor_sumsq(slot, t.p2.X.p, AOADMM_PREC_F64, (int64_t)t.p2.I * t.p2.Jtot, ws.d(), stream_);
    } else if (t.blk.sparse && t.blk.sem.on && t.blk.sem.weighted) {   // sum_Omega w x^2 (sem_set_weights)
      t.normsq = t.blk.sem.wnormsq;
      t.normsq_valid = true;
      return t.normsq;
    } else if (t.blk.sparse) {     // norm(sptensor)^2 (:132): the coalesced values
      const CooBlock& c = t.blk.coo; // replicated: every rank holds all of them; sharded: the mode-0 shares cover them once
      AO_REQUIRE(!c.sharded || (c.cut_rank == rank_ && c.cut_world == world_),
                 "sparse tensor %d was cut for rank %d of %d, the engine is now rank %d of %d: upload again", p, c.cut_rank,
                 c.cut_world, rank_, world_);
      tensor_sumsq(slot, c.mode[0].val.p, AOADMM_PREC_F64, c.nnz, ws.d(), stream_);
      if (c.sharded) allreduce(slot, 1);
    } else if (t.blk.half) {       // sum of q^2 over a pass copy (its padding is zero); the data is q / s
      const CpBlock& b = t.blk;      // copy[2] holds this rank's rows, and s is the same on every rank
      tensor_sumsq(slot, b.copy[2].buf.p, AOADMM_PREC_F16, half_copy_elems(b.copy[2].pad * b.dims[1], b.dims[2]), ws.d(), stream_);
      allreduce(slot, 1);
    } else {
      AO_REQUIRE(!t.blk.x_released, "internal: ||X||^2 of tensor %d asked for after its natural-layout array was released", p);
      tensor_sumsq(slot, t.blk.X.data.p, t.blk.X.prec, t.blk.X.elems_padded(), ws.d(), stream_);
      allreduce(slot, 1);
    }
    double v = 0;
    AO_HIP(hipMemcpyAsync(&v, slot, sizeof(double), hipMemcpyDeviceToHost, stream_));
    AO_HIP(hipStreamSynchronize(stream_));
    if (!t.par2 && !t.blk.sparse && t.blk.half) v = v / t.blk.scale / t.blk.scale;   // powers of two: exact
    t.normsq = v;
    t.normsq_valid = true;
  }
  return t.normsq;
}

void Engine::tensor_synth(int p, int rank, uint64_t seed, double noise, int prec) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(!t.par2 && t.nmodes == 3, "synthetic generator handles 3-way CP blocks");
  AO_REQUIRE(!t.blk.sparse, "tensor %d holds sparse data: the synthetic generator writes dense blocks (upload dense data first)", p);
  AO_REQUIRE(rank > 0 && rank <= kMaxRank, "bad rank");
  const bool half = prec == AOADMM_PREC_F16;           // generated as for AOADMM_PREC_F32, then rounded like an upload
  if (half) { require_half_ok(t, p, false); prec = AOADMM_PREC_F32; }
  AO_REQUIRE(prec == AOADMM_PREC_F64 || prec == AOADMM_PREC_F32, "bad precision id %d", prec);
  AO_HIP(hipSetDevice(device_));
  const int64_t I = modes_[t.modes[0]].rows, J = modes_[t.modes[1]].rows, K = modes_[t.modes[2]].rows;
  const int64_t per = cdiv(I, world_);
  const int64_t row0 = std::min<int64_t>(I, per * rank_);
  const int64_t loc = std::min<int64_t>(I, row0 + per) - row0;
  AO_REQUIRE(per * (world_ - 1) < I, "tensor %d: first mode of %lld rows cannot be split over %d ranks (the last rank would own no rows)",
             p, (long long)I, world_);           // the same verdict on every rank
  CpBlock& b = t.blk;
  b.nd = 3; b.full0 = I; b.row0 = row0;
  b.dims[0] = loc; b.dims[1] = J; b.dims[2] = K;
  b.X.prec = prec; b.X.nd = 3;
  b.X.dims[0] = loc; b.X.dims[1] = J; b.X.dims[2] = K;
  b.X.pad0 = pad_of(prec, loc);
  b.X.data.alloc((size_t)b.X.elems_padded() * b.X.elem_size());
  DevBuf A, B, C, ws;
  A.alloc((size_t)I * rank * 8); B.alloc((size_t)J * rank * 8); C.alloc((size_t)K * rank * 8);
  ws.alloc(synth_ws_bytes());
  SynthArgs a;
  a.I_loc = loc; a.I_pad = b.X.pad0; a.J = J; a.K = K; a.row0 = row0; a.I_full = I; a.R = rank; a.seed = seed;
  synth_factors(A.d(), B.d(), C.d(), a, stream_);
  double* slot = dev_.scratch();
  synth_norms(slot, A.d(), B.d(), C.d(), a, ws.d(), stream_);
  allreduce(slot, 3);
  double h[3];
  AO_HIP(hipMemcpyAsync(h, slot, 3 * sizeof(double), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  // sigma = noise*||X0||/||N|| (create_coupled_data.m:158-162), then X <- X/||X|| (example_script1:91-92)
  const double sigma = h[1] > 0 ? noise * std::sqrt(h[0]) / std::sqrt(h[1]) : 0.0;
  const double nsq = h[0] + 2.0 * sigma * h[2] + sigma * sigma * h[1];
  synth_write(b.X.data.p, prec, A.d(), B.d(), C.d(), a, sigma, 1.0 / std::sqrt(nsq), stream_);
  AO_HIP(hipStreamSynchronize(stream_));
  b.reset_derived();
  const BlockCtx cx = block_ctx();
  t.normsq_valid = false;
  if (half) {                                          // collective on a sharded engine, like the norms above
    const SlabSource generate = [&](DevBuf& slab, int64_t k0, int64_t kloc) {   // the same tensor's third-mode slab, all rows
      SynthArgs ak = a;
      ak.I_loc = I; ak.I_pad = pad_of(prec, I); ak.row0 = 0; ak.k0 = k0; ak.K_loc = kloc;
      slab.alloc((size_t)ak.I_pad * J * kloc * b.X.elem_size());
      synth_write(slab.p, prec, A.d(), B.d(), C.d(), ak, sigma, 1.0 / std::sqrt(nsq), stream_);
    };
    block_make_half(cx, b, &generate);
    return;
  }
  {
    int64_t k0 = 0, kloc = 0;
    if (want_ksharded_xp(cx, b, K, &k0, &kloc)) {        // this rank's third-mode slab of the SAME tensor, all rows
      SynthArgs ak = a;
      ak.I_loc = I; ak.I_pad = pad_of(prec, I); ak.row0 = 0; ak.k0 = k0; ak.K_loc = kloc;
      DevBuf slab;
      slab.alloc((size_t)ak.I_pad * J * kloc * b.X.elem_size());
      synth_write(slab.p, prec, A.d(), B.d(), C.d(), ak, sigma, 1.0 / std::sqrt(nsq), stream_);
      adopt_ksharded_xp(cx, b, slab.p, k0, kloc);
      AO_HIP(hipStreamSynchronize(stream_));          // slab is a local
    }
  }
  (void)ensure_pass_copy(cx, b, 1); (void)ensure_pass_copy(cx, b, 2);   // set-up cost of the data, like the generation itself
  AO_HIP(hipStreamSynchronize(stream_));
  t.normsq_valid = false;
}

// ---------------------------------------------------------------------------
// missing data (Z.miss, cmtf_AOADMM.m:68-121)
// ---------------------------------------------------------------------------
void Engine::tensor_mask_upload(int p, const uint8_t* mask) {
  require_usable();
  AO_REQUIRE(p >= 0 && p < n_tensors_ && !tensors_[p].par2, "tensor %d is not a CP block", p);
  AO_REQUIRE(mask != nullptr, "null mask");
  TensorInfo& t = tensors_[p];
  CpBlock& b = t.blk;
  AO_REQUIRE(b.has_data, "upload Z.object{%d} before Z.miss{%d}", p + 1, p + 1);
  AO_REQUIRE(!b.sparse, "Missing data (Z.miss) not supported for sptensor objects. Convert to tensor first. (Z.object{%d}, cmtf_AOADMM.m:78-79)", p + 1);
  AO_REQUIRE(!b.x_released, "Z.object{%d} was released after its pass copies were built: upload it again before Z.miss{%d}", p + 1, p + 1);
  AO_HIP(hipSetDevice(device_));
  const int64_t Iloc = b.dims[0], Ip = b.X.pad0, Ifull = b.full0;
  int64_t ncols = 1;
  for (int i = 1; i < b.nd; ++i) ncols *= b.dims[i];
  // the caller's bytes land in a staging buffer in the padded layout and are packed to one bit per entry on the device
  // (the EM pass reads the mask once per outer iteration: 1/8 of the bytes, and 7/8 of a byte per entry of HBM back)
  DevBuf bytes;
  bytes.alloc((size_t)Ip * ncols);
  AO_HIP(hipMemsetAsync(bytes.p, 1, (size_t)Ip * ncols, stream_));
  // rows [row0, row0 + Iloc) of every column of the full column-major mask; the padding rows stay 1
  AO_HIP(hipMemcpy2DAsync(bytes.p, (size_t)Ip, mask + b.row0, (size_t)Ifull, (size_t)Iloc, (size_t)ncols,
                          hipMemcpyHostToDevice, stream_));
  b.mask.alloc(em_mask_bits_bytes(Ip * ncols));
  em_mask_pack(bytes.as<uint8_t>(), b.mask.as<uint8_t>(), Ip * ncols, stream_);
  if (b.nd == 2) {                                   // matrices keep a transposed copy of the data: mask too
    const int64_t J = b.dims[1], Jp = b.Xt.pad0;
    std::vector<uint8_t> mt((size_t)Jp * Iloc, 1);
    for (int64_t i = 0; i < Iloc; ++i)
      for (int64_t j = 0; j < J; ++j) mt[(size_t)j + (size_t)Jp * i] = mask[b.row0 + i + Ifull * j];
    DevBuf bytesT;
    bytesT.alloc(mt.size());
    AO_HIP(hipMemcpyAsync(bytesT.p, mt.data(), mt.size(), hipMemcpyHostToDevice, stream_));
    b.maskT.alloc(em_mask_bits_bytes((int64_t)mt.size()));
    em_mask_pack(bytesT.as<uint8_t>(), b.maskT.as<uint8_t>(), (int64_t)mt.size(), stream_);
    AO_HIP(hipStreamSynchronize(stream_));             // bytesT and mt are locals
  }
  AO_HIP(hipStreamSynchronize(stream_));
  block_drop_weights(block_ctx(), b);                // the later of mask and weights wins: Xhat <- X0 (nothing can refuse any more)
  b.has_mask = true;
  b.mask_imputed = false;
  b.mlist.clear();                                   // the list of the old mask's missing entries, and the mark with it
  drop_pass_copies(b);                               // the imputation would have to update them too
  t.normsq_valid = false;
}

// Per-entry weights on a dense CP block: W in [0, 1] of the block's shape, the FULL array under
// a communicator like the mask.  Everything is checked before the block changes.
void Engine::tensor_weights_upload(int p, const double* W) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  if (t.par2)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("per-entry weights are for CP blocks: tensor %d is PARAFAC2", p));
  CpBlock& b = t.blk;
  AO_REQUIRE(b.has_data, "tensor %d has no data: upload Z.object{%d} before its weights", p, p + 1);
  AO_REQUIRE(!b.sparse, "tensor %d holds sparse data: its weights go through aoadmm_tensor_set_entry_weights", p);
  AO_REQUIRE(!b.half, "tensor %d is stored as fp16: per-entry weights need fp64 or fp32 storage", p);
  AO_REQUIRE(!b.x_released, "Z.object{%d} was released after its pass copies were built: upload it again before its weights", p + 1);
  AO_REQUIRE(!(b.has_mask && b.mask_imputed), "Z.object{%d} holds imputed values at its missing entries (a masked EM pass has run): upload the data again before its weights", p + 1);
  AO_HIP(hipSetDevice(device_));
  const BlockCtx cx = block_ctx();
  if (W == nullptr) {
    if (b.has_weights) { block_drop_weights(cx, b); t.normsq_valid = false; }
    return;
  }
  const int64_t Iloc = b.dims[0], Ifull = b.full0;
  int64_t ncols = 1;
  for (int i = 1; i < b.nd; ++i) ncols *= b.dims[i];
  bool ok;
  if (Iloc == Ifull) {
    ok = block_set_weights(cx, b, W);
  } else {                                             // this rank's rows of every column
    // the same verdict on every rank: each holds the whole W and checks all of it, not only the rows it keeps
    if (!block_weights_in_range(cx, W, Ifull * ncols))
      throw Error(AOADMM_ERR_INVALID, fmt("weights of tensor %d: a value is not a finite number in [0, 1] (divide the weights by their maximum)", p));
    std::vector<double> rows((size_t)Iloc * ncols);
    for (int64_t c = 0; c < ncols; ++c)
      std::memcpy(&rows[(size_t)c * Iloc], W + c * Ifull + b.row0, (size_t)Iloc * sizeof(double));
    ok = block_set_weights(cx, b, rows.data());
  }
  if (!ok)
    throw Error(AOADMM_ERR_INVALID, fmt("weights of tensor %d: a value is not a finite number in [0, 1] (divide the weights by their maximum)", p));
  t.normsq_valid = false;
}

// Observed-only sparse CP block (sparse_em.h): the stored entries are the observations, the others are missing and
// start at 0 (example_script12_CP_PAR2_EM.m:115-147).  Z.miss on sparse data stays refused (tensor_mask_upload).
void Engine::set_observed_only(int p, bool on) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  if (t.par2)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("observed-only is for sparse CP blocks: tensor %d is PARAFAC2 (sparse slabs with missing entries are not supported)", p));
  CpBlock& b = t.blk;
  AO_REQUIRE(b.has_data, "tensor %d has no data: upload it with aoadmm_tensor_upload_coo first", p);
  if (!b.sparse)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("observed-only is for sparse CP blocks: tensor %d holds dense data (use Z.miss / aoadmm_tensor_mask_upload)", p));
  if (b.coo.sharded)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("observed-only is not available for a block uploaded with aoadmm_tensor_upload_coo_sharded (tensor %d): upload it replicated", p));
  AO_REQUIRE(b.coo.nnz > 0, "tensor %d has no stored entry: an observed-only block needs observations", p);
  AO_HIP(hipSetDevice(device_));
  if (b.sem.on && b.sem.weighted) t.normsq_valid = false;   // unmarking drops the weights: ||X||^2 is the plain one again
  if (!on) { b.sem.clear(); return; }
  sem_enable(b.sem, b.coo, modes_[t.modes[0]].R, stream_);   // a weighted block keeps its weights
  AO_HIP(hipStreamSynchronize(stream_));
}

// Weighted least squares on an observed-only block (sparse_em.h): w_e in [0, 1] per stored entry, unstored_weight in
// [0, 1] for every other entry.  The list must name exactly the block's stored entries, once each, in any order; it
// goes through coo_build with the weights as values, which leaves every mode's weights in the order of that copy.
// Everything is checked before the block changes.
void Engine::set_entry_weights(int p, int64_t nnz, const int64_t* subs, const double* wts, double unstored_weight) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  if (t.par2)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("entry weights are for sparse CP blocks: tensor %d is PARAFAC2", p));
  CpBlock& b = t.blk;
  AO_REQUIRE(b.has_data, "tensor %d has no data: upload it with aoadmm_tensor_upload_coo first", p);
  if (!b.sparse)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("aoadmm_tensor_set_entry_weights is for sparse CP blocks: tensor %d holds dense data (use aoadmm_tensor_weights_upload, or Z.miss / aoadmm_tensor_mask_upload)", p));
  if (b.coo.sharded)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("entry weights are not available for a block uploaded with aoadmm_tensor_upload_coo_sharded (tensor %d): upload it replicated", p));
  AO_REQUIRE(b.coo.nnz > 0, "tensor %d has no stored entry: a weighted block needs observations", p);
  AO_REQUIRE(std::isfinite(unstored_weight) && unstored_weight >= 0.0 && unstored_weight <= 1.0,
             "entry weights: the unstored weight %g is outside [0, 1] (divide the weights by their maximum)", unstored_weight);
  AO_REQUIRE(nnz >= 0 && (nnz == 0) == (wts == nullptr) && (nnz == 0 || subs != nullptr),
             "entry weights: give subs and wts for every stored entry, or nnz = 0 and wts = NULL for stored weights 1");
  AO_REQUIRE(nnz == 0 || nnz == b.coo.nnz, "entry weights: %lld weights for a block that stores %lld entries", (long long)nnz, (long long)b.coo.nnz);
  for (int64_t e = 0; e < nnz; ++e)
    AO_REQUIRE(std::isfinite(wts[e]) && wts[e] >= 0.0 && wts[e] <= 1.0,
               "entry weights: weight %g of entry %lld is outside [0, 1] (divide the weights by their maximum)", wts[e], (long long)e);
  AO_HIP(hipSetDevice(device_));
  CooBlock wl;
  if (nnz > 0) {
    coo_build(wl, b.coo.nd, b.coo.dims, nnz, subs, wts, stream_);     // out-of-range subscripts: AOADMM_ERR_INVALID
    if (wl.nnz != nnz)
      throw Error(AOADMM_ERR_INVALID, fmt("entry weights: %lld of the %lld subscripts are duplicates", (long long)(nnz - wl.nnz), (long long)nnz));
    sem_check_weight_list(b.coo, wl, stream_);
  }
  const int R = modes_[t.modes[0]].R;
  if (!b.sem.on || b.sem.R != R) sem_enable(b.sem, b.coo, R, stream_);
  sem_set_weights(b.sem, b.coo, nnz > 0 ? &wl : nullptr, unstored_weight, stream_);
  t.normsq_valid = false;
}

void Engine::sparse_em_enqueue(int p, bool stats_only) {
  TensorInfo& t = tensors_[p];
  CpBlock& b = t.blk;
  SemFac sf[kCooMaxModes];
  for (int i = 0; i < t.nmodes; ++i) {
    const FactorRef fr = factor_ref(modes_[t.modes[i]]);
    sf[i] = SemFac{fr.p, fr.ld, fr.pT};
  }
  const bool snap = b.sem.have_snap && !stats_only;
  // the whole step is one launch of class 3; the pass over mode n's copy is also one of class 4 + n
  const LaunchTimers::Pair pr = timers_.begin(timers_.stats[3], timers_.profile, stream_);
  sem_step_begin(b.sem, b.coo, sf, stats_only, stream_);
  double bytes = 0.0, flops = 0.0;
  for (int pos = 0; pos < (stats_only ? 1 : t.nmodes); ++pos) {
    KernelStats& ks = timers_.stats[kStatsEmPass + pos];
    const LaunchTimers::Pair pp = timers_.begin(ks, timers_.profile, stream_);
    sem_step_pass(b.sem, b.coo, sf, pos, stats_only, stream_);
    const double pb = sem_pass_bytes(b.sem, pos == 0, snap, !stats_only), pf = sem_pass_flops(b.sem, pos == 0, snap);
    timers_.end(ks, pp, stream_, pb, pf);
    bytes += pb; flops += pf;
  }
  sem_step_finish(b.sem, sf, stats_only, dev_.em(p), stream_);
  timers_.end(timers_.stats[3], pr, stream_, bytes, flops);
}

void Engine::resident_em_step(int p, double stats[3]) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(stats != nullptr, "null stats");
  TensorInfo& t = tensors_[p];
  if (!t.observed_only())
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("tensor %d is not an observed-only sparse CP block (aoadmm_tensor_set_observed_only)", p));
  for (int i = 0; i < t.nmodes; ++i) AO_REQUIRE(modes_[t.modes[i]].has_fac, "G.fac{%d} missing", t.modes[i] + 1);
  AO_REQUIRE(t.blk.sem.R == modes_[t.modes[0]].R, "tensor %d was marked observed-only for rank %d", p, t.blk.sem.R);
  AO_HIP(hipSetDevice(device_));
  sparse_em_enqueue(p, false);
  double h4[kEmStats];
  AO_HIP(hipMemcpyAsync(h4, dev_.em(p), sizeof h4, hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  stats[0] = h4[kEmObsRes]; stats[1] = h4[kEmNum]; stats[2] = h4[kEmDen];
}

// natural-layout array on the device (first dimension padded to `pad0`) -> unpadded doubles on the host
void download_unpadded(const DenseTensor& X, int64_t rows, int64_t cols, double* out, hipStream_t s) {
  const size_t es = X.elem_size();
  std::vector<char> h((size_t)X.pad0 * cols * es);
  AO_HIP(hipMemcpyAsync(h.data(), X.data.p, h.size(), hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));
  for (int64_t c = 0; c < cols; ++c)
    for (int64_t i = 0; i < rows; ++i) {
      const size_t e = (size_t)i + (size_t)X.pad0 * c;
      out[i + rows * c] = X.prec == AOADMM_PREC_F32 ? (double)reinterpret_cast<const float*>(h.data())[e]
                                                    : reinterpret_cast<const double*>(h.data())[e];
    }
}

void Engine::resident_em_pass(int p, int update, int fuse, double stats[4], double* data, double* data_t, double* mttkrp,
                              int64_t info[8]) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_REQUIRE(stats != nullptr, "null stats");
  AO_REQUIRE(fuse >= kEmFuseNone && fuse <= kEmFuseSecond, "fuse = %d outside 0..2", fuse);
  if (sharded()) throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_resident_em_pass runs on one engine without a communicator");
  TensorInfo& t = tensors_[p];
  if (t.par2) {
    AO_REQUIRE(!t.p2.sparse, "tensor %d holds sparse slabs: it has no EM pass", p);
    for (int k = 0; k < t.p2.K; ++k) AO_REQUIRE(t.p2.have_slab[k], "slab %d of tensor %d has no data", k, p);
  } else {
    AO_REQUIRE(t.blk.has_data && !t.blk.sparse, "tensor %d holds no dense data (sparse blocks: aoadmm_resident_em_step)", p);
    AO_REQUIRE(!t.blk.half, "tensor %d is stored as fp16: it has no EM pass", p);
  }
  AO_REQUIRE(t.masked(), "tensor %d is neither masked nor weighted (aoadmm_tensor_mask_upload / aoadmm_par2_slab_mask_upload / aoadmm_tensor_weights_upload)", p);
  if (!t.par2 && t.blk.mlist.on && update)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("tensor %d is marked with aoadmm_tensor_set_missing_list: its imputing pass is aoadmm_resident_em_list_pass", p));
  for (int i = 0; i < t.nmodes; ++i) AO_REQUIRE(modes_[t.modes[i]].has_fac, "G.fac{%d} missing", t.modes[i] + 1);
  AO_HIP(hipSetDevice(device_));
  EmPassInfo pi;
  em_pass_enqueue(p, update != 0, fuse, &pi);
  int mpos = -1;
  if (pi.fused >= 0) {
    // the first MTTKRP of the next outer iteration as update_mode runs it: the cached T must serve it
    CpBlock& b = t.blk;
    const std::vector<int> seq = update_sequence(p);
    mpos = seq.empty() ? 0 : seq[0];
    if (mttkrp) {
      FactorRef facs[8];
      factor_refs(t, facs);
      ModeInfo& mi = modes_[t.modes[mpos]];
      ensure_mode_work(mi);
      block_mttkrp(block_ctx(), b, mpos, facs, mi.R, 1.0, mi.A.d(), mi.rows, true, seq.data(), (int)seq.size());
      AO_HIP(hipMemcpyAsync(mttkrp, mi.A.p, (size_t)mi.rows * mi.R * sizeof(double), hipMemcpyDeviceToHost, stream_));
    }
    b.cached_mode = -1;                              // the solver's own factors may differ from what this pass used
  }
  double h4[kEmStats];
  AO_HIP(hipMemcpyAsync(h4, dev_.em(p), sizeof h4, hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
  for (int q = 0; q < kEmStats; ++q) stats[q] = h4[q];
  if (info) {
    info[0] = pi.launch.vec; info[1] = pi.launch.rmax; info[2] = pi.fused; info[3] = pi.walk;
    info[4] = pi.launch.strips; info[5] = pi.launch.jchunks; info[6] = pi.launch.jlen; info[7] = mpos;
  }
  if (t.par2) {
    if (data) {
      AO_HIP(hipMemcpyAsync(data, t.p2.X.p, (size_t)t.p2.I * t.p2.Jtot * sizeof(double), hipMemcpyDeviceToHost, stream_));
      AO_HIP(hipStreamSynchronize(stream_));
    }
    return;
  }
  CpBlock& b = t.blk;
  int64_t cols = 1;
  for (int i = 1; i < b.nd; ++i) cols *= b.dims[i];
  if (data) download_unpadded(b.X, b.dims[0], cols, data, stream_);
  if (data_t && b.nd == 2) download_unpadded(b.Xt, b.dims[1], b.dims[0], data_t, stream_);
}

bool Engine::has_missing() const {
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].missing()) return true;
  return false;
}

// One EM pass over tensor p with the current factors: {num, den, obs_res, obs_x2} -> its EM slots, all-reduced
// over the row shards; update = 1 also overwrites the missing entries with the model (:416-435).
void Engine::em_pass_enqueue(int p, int update, int fuse, EmPassInfo* info) {
  TensorInfo& t = tensors_[p];
  if (info) *info = EmPassInfo();
  if (t.par2) {
    Par2Block& b = t.p2;
    EmPar2Args a;
    a.X = b.X.d(); a.mask = b.mask.as<uint8_t>();
    a.A = modes_[t.modes[0]].fac.d(); a.B = modes_[t.modes[1]].fac.d(); a.C = modes_[t.modes[2]].fac.d();
    a.off = b.off_d.as<int64_t>(); a.K = b.K; a.I = b.I; a.R = b.R; a.update = update;
    emws_.ensure((size_t)b.K * 4 * sizeof(double));
    em_par2_pass(a, emws_.d(), dev_.em(p), stream_);
    return;
  }
  CpBlock& b = t.blk;
  if (update && b.mlist.on) {                         // a marked block imputes from its list; update = 0 stays the dense pass
    em_list_enqueue(p, 1, false);
    return;
  }
  const ModeInfo& m0 = modes_[t.modes[0]];
  const ModeInfo& m1 = modes_[t.modes[1]];
  EmCpArgs a;
  a.X = b.X.data.p; a.mask = b.mask.as<uint8_t>();
  if (b.has_weights) { a.X0 = b.X0.p; a.Wt = b.Wt.p; fuse = kEmFuseNone; }   // no fused form: the plain pass, then the ordinary contraction
  a.A = m0.fac.d() + (sharded() ? b.row0 : 0); a.ldA = m0.rows;
  a.B = m1.fac.d(); a.ldB = m1.rows;
  a.C = nullptr; a.ldC = 0;
  a.I = b.dims[0]; a.Ipad = b.X.pad0; a.J = b.dims[1]; a.K = 1; a.R = m0.R; a.update = update;
  if (b.nd == 3) {
    const ModeInfo& m2 = modes_[t.modes[2]];
    a.C = m2.fac.d(); a.ldC = m2.rows; a.K = b.dims[2];
  } else if (b.nd > 3) {
    // order > 3: modes 3..N are merged into one, its factor is their Khatri-Rao product in storage order
    int64_t Km = 1;
    for (int i = 2; i < b.nd; ++i) Km *= b.dims[i];
    b.emkr.ensure((size_t)Km * a.R * 8); b.emkr2.ensure((size_t)Km * a.R * 8);
    const ModeInfo& m2 = modes_[t.modes[2]];
    const double* cur = m2.fac.d();
    int64_t curK = b.dims[2], ld = m2.rows;
    double* bufs[2] = {b.emkr.d(), b.emkr2.d()};
    for (int i = 3; i < b.nd; ++i) {
      const ModeInfo& mn = modes_[t.modes[i]];
      double* dst = bufs[(i - 3) & 1];
      kr_merge(dst, cur, ld, curK, mn.fac.d(), mn.rows, b.dims[i], a.R, stream_);
      cur = dst; curK *= b.dims[i]; ld = curK;
    }
    a.C = cur; a.ldC = curK; a.K = curK;
  }
  emws_.ensure(em_cp_ws_bytes(a.Ipad, a.J, a.K));
  // The imputation pass reads and rewrites the whole block: it can leave the partial contraction the next outer
  // iteration starts with (the pass that serves the first mode it updates), taken from the values it writes back.
  // Contracted mode: 2 or 3 (the strip kernel vectorises mode 1), the one whose factor stays unchanged longest.
  int fused_c = -1;
  ContractPlan fpl;
  FactorRef facs[8];
  if (fuse != kEmFuseNone && update && b.nd == 3 && em_cp_can_fuse(a, b.X.prec) && b.dims[1] <= 65535 &&
      b.dims[2] <= 65535 && !small_direct(sharded(), b, a.R)) {
    factor_refs(t, facs);
    const std::vector<int> seq = update_sequence(p);
    const int pos0 = seq.empty() ? 0 : seq[0];
    int best = -1;
    for (int cand = 2; cand >= 1; --cand) {
      if (cand == pos0) continue;
      const int dist = next_update_distance(pos0, cand, seq.data(), (int)seq.size());
      if (dist > best) { best = dist; fused_c = cand; }
    }
    // contract the second mode whenever that is allowed, so that the strip's walk along mode 2 with the fused
    // contraction is exercised by models whose update order would never pick it
    if (fuse == kEmFuseSecond && pos0 != 1) fused_c = 1;
    const int64_t J = b.dims[1], K = b.dims[2];
    a.walk = fused_c == 1 ? 1 : 2;
    fpl = fused_c == 2 ? make_plan(1, 0, a.Ipad * J, a.Ipad * J, K, a.R, b.X.prec)
                       : make_plan(K, a.Ipad * J, a.Ipad, a.Ipad, J, a.R, b.X.prec);
    fpl.nchunk = em_cp_fused_chunks(a, b.X.prec);
    b.T.ensure(fpl.t_bytes());
    a.T = b.T.p;
    a.t_chunk_stride = fpl.trows() * a.R;
  }
  if (info) { info->launch = em_cp_launch_of(a, b.X.prec, a.T != nullptr); info->fused = fused_c; info->walk = a.walk; }
  // the op-level call (aoadmm_resident_em_pass) brackets the pass with events of class kStatsEmPass; a solve records none
  const double es = (double)b.X.elem_size(), ne = (double)b.X.elems_padded();
  const LaunchTimers::Pair pr = info ? timers_.begin(timers_.stats[kStatsEmPass], timers_.profile, stream_) : LaunchTimers::Pair();
  em_cp_pass(a, b.X.prec, emws_.d(), dev_.em(p), stream_);
  if (info) timers_.end(timers_.stats[kStatsEmPass], pr, stream_, b.has_weights ? (update ? 4 : 3) * es * ne : (update ? 2 : 1) * es * ne + ne / 8, 0.0);
  if (update && b.has_mask) b.mask_imputed = true;
  if (b.nd == 2 && update) {
    // same imputation on the transposed copy (roles of the two factors swapped); its statistics are discarded
    EmCpArgs at = a;
    at.X = b.Xt.data.p; at.mask = b.maskT.as<uint8_t>();
    if (b.has_weights) { at.X0 = b.X0t.p; at.Wt = b.WtT.p; }
    at.A = m1.fac.d(); at.ldA = m1.rows; at.B = m0.fac.d() + (sharded() ? b.row0 : 0); at.ldB = m0.rows;
    at.I = b.dims[1]; at.Ipad = b.Xt.pad0; at.J = b.dims[0];
    const size_t wsb = em_cp_ws_bytes(at.Ipad, at.J, 1);
    emws_.ensure(wsb + 64);
    em_cp_pass(at, b.Xt.prec, emws_.d(), emws_.d() + wsb / sizeof(double), stream_);   // statistics to a scratch tail
  }
  allreduce(dev_.em(p), kEmStats);
  if (update) b.cached_mode = -1;                    // the data changed: cached partial contractions are stale
  if (fused_c >= 0) { b.cached_mode = fused_c; b.cached_version = facs[fused_c].version; b.plan = fpl; }
}

// ---------------------------------------------------------------------------
// state
// ---------------------------------------------------------------------------
// Resolve a field of the struct G to its device location.  Slab-valued fields (PARAFAC2 B mode and the
// block's P / mu_DeltaB) live back to back; `slab` selects J_k x R block k.
struct StateLoc {
  double* p;
  int64_t rows, cols;
};
static StateLoc slab_loc(DevBuf& buf, const ModeInfo& mB, int slab) {
  buf.ensure((size_t)mB.rows * mB.R * sizeof(double));
  if (slab == AOADMM_ALL_SLABS) return StateLoc{buf.d(), mB.rows, (int64_t)mB.R};   // all K slabs back to back
  AO_REQUIRE(slab >= 0 && slab < mB.K, "slab %d out of range [0,%d)", slab, mB.K);
  return StateLoc{buf.d() + mB.off_k[slab] * mB.R, mB.rows_k[slab], (int64_t)mB.R};
}

void Engine::state_set(int field, int index, int slab, const double* host, int64_t rows, int64_t cols) {
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(host != nullptr && rows > 0 && cols > 0, "state_set: empty array");
  AO_HIP(hipSetDevice(device_));
  best_.iter = -1;                                    // a kept best iterate belongs to the state the last solve started from
  StateLoc loc{nullptr, 0, 0};
  if (field == AOADMM_F_COUPLING_FAC) {
    AO_REQUIRE(index >= 0 && index < n_couplings_, "coupling %d out of range", index);
    CouplingInfo& ci = couplings_[index];
    ci.Delta.ensure((size_t)ci.rows * ci.cols * sizeof(double));
    loc = StateLoc{ci.Delta.d(), ci.rows, ci.cols};
    ci.has_state = true;
  } else if (field == AOADMM_F_DELTAB || field == AOADMM_F_P || field == AOADMM_F_MU_DELTAB) {
    AO_REQUIRE(index >= 0 && index < n_tensors_ && tensors_[index].par2, "tensor %d is not a PARAFAC2 block", index);
    TensorInfo& t = tensors_[index];
    Par2Block& b = t.p2;
    const ModeInfo& mB = modes_[t.modes[1]];
    if (field == AOADMM_F_DELTAB) {
      b.DeltaB.ensure((size_t)b.R * b.R * sizeof(double));
      loc = StateLoc{b.DeltaB.d(), (int64_t)b.R, (int64_t)b.R};
      b.has_DeltaB = true;
    } else if (field == AOADMM_F_P) {
      loc = slab_loc(b.P, mB, slab);
      if (slab == AOADMM_ALL_SLABS) b.have_P.assign(b.K, 1); else b.have_P[slab] = 1;
    } else {
      loc = slab_loc(b.muDB, mB, slab);
      if (slab == AOADMM_ALL_SLABS) b.have_mu.assign(b.K, 1); else b.have_mu[slab] = 1;
    }
  } else {
    check_mode(index);
    ModeInfo& mi = modes_[index];
    auto whole = [&](DevBuf& buf, int64_t r, int64_t c) {
      buf.ensure((size_t)r * c * sizeof(double));
      return StateLoc{buf.d(), r, c};
    };
    switch (field) {
      case AOADMM_F_FAC:
        loc = mi.slabs ? slab_loc(mi.fac, mi, slab) : whole(mi.fac, mi.rows, mi.R);
        mi.has_fac = true; mi.version++;
        break;
      case AOADMM_F_CONSTRAINT_FAC:
        loc = mi.slabs ? slab_loc(mi.Z, mi, slab) : whole(mi.Z, mi.rows, mi.R);
        mi.has_Z = true;
        break;
      case AOADMM_F_CONSTRAINT_DUAL:
        loc = mi.slabs ? slab_loc(mi.mu, mi, slab) : whole(mi.mu, mi.rows, mi.R);
        mi.has_mu = true;
        break;
      case AOADMM_F_COUPLING_DUAL:
        AO_REQUIRE(!mi.slabs, "the PARAFAC2 B_k mode cannot be coupled");
        loc = whole(mi.muD, rows, cols);
        mi.has_muD = true; mi.muD_rows = rows; mi.muD_cols = cols;
        break;
      default: throw Error(AOADMM_ERR_INVALID, fmt("unknown state field %d", field));
    }
  }
  AO_REQUIRE(rows == loc.rows && cols == loc.cols, "state field %d index %d slab %d must be %lld x %lld, got %lld x %lld", field,
             index + 1, slab + 1, (long long)loc.rows, (long long)loc.cols, (long long)rows, (long long)cols);
  AO_HIP(hipMemcpyAsync(loc.p, host, (size_t)rows * cols * sizeof(double), hipMemcpyHostToDevice, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

void Engine::state_get(int field, int index, int slab, double* host, int64_t rows, int64_t cols) {
  AO_REQUIRE(host != nullptr, "state_get: null destination");
  AO_HIP(hipSetDevice(device_));
  StateLoc loc{nullptr, 0, 0};
  if (field == AOADMM_F_COUPLING_FAC) {
    AO_REQUIRE(index >= 0 && index < n_couplings_, "coupling %d out of range", index);
    AO_REQUIRE(couplings_[index].has_state, "coupling_fac{%d} was never set", index + 1);
    loc = StateLoc{couplings_[index].Delta.d(), couplings_[index].rows, couplings_[index].cols};
  } else if (field == AOADMM_F_DELTAB || field == AOADMM_F_P || field == AOADMM_F_MU_DELTAB) {
    AO_REQUIRE(index >= 0 && index < n_tensors_ && tensors_[index].par2, "tensor %d is not a PARAFAC2 block", index);
    TensorInfo& t = tensors_[index];
    Par2Block& b = t.p2;
    const ModeInfo& mB = modes_[t.modes[1]];
    AO_REQUIRE(b.has_DeltaB, "DeltaB{%d} was never set", index + 1);
    if (field == AOADMM_F_DELTAB) loc = StateLoc{b.DeltaB.d(), (int64_t)b.R, (int64_t)b.R};
    else if (field == AOADMM_F_P) loc = slab_loc(b.P, mB, slab);
    else loc = slab_loc(b.muDB, mB, slab);
  } else {
    check_mode(index);
    ModeInfo& mi = modes_[index];
    switch (field) {
      case AOADMM_F_FAC:
        AO_REQUIRE(mi.has_fac, "fac{%d} was never set", index + 1);
        loc = mi.slabs ? slab_loc(mi.fac, mi, slab) : StateLoc{mi.fac.d(), mi.rows, (int64_t)mi.R};
        break;
      case AOADMM_F_CONSTRAINT_FAC:
        AO_REQUIRE(mi.has_Z, "constraint_fac{%d} was never set", index + 1);
        loc = mi.slabs ? slab_loc(mi.Z, mi, slab) : StateLoc{mi.Z.d(), mi.rows, (int64_t)mi.R};
        break;
      case AOADMM_F_CONSTRAINT_DUAL:
        AO_REQUIRE(mi.has_mu, "constraint_dual_fac{%d} was never set", index + 1);
        loc = mi.slabs ? slab_loc(mi.mu, mi, slab) : StateLoc{mi.mu.d(), mi.rows, (int64_t)mi.R};
        break;
      case AOADMM_F_COUPLING_DUAL:
        AO_REQUIRE(mi.has_muD, "coupling_dual_fac{%d} was never set", index + 1);
        loc = StateLoc{mi.muD.d(), mi.muD_rows, mi.muD_cols};
        break;
      default: throw Error(AOADMM_ERR_UNSUPPORTED, fmt("state field %d not available", field));
    }
  }
  AO_REQUIRE(rows == loc.rows && cols == loc.cols, "state_get: destination is %lld x %lld, field is %lld x %lld", (long long)rows,
             (long long)cols, (long long)loc.rows, (long long)loc.cols);
  AO_HIP(hipMemcpyAsync(host, loc.p, (size_t)rows * cols * sizeof(double), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

// ---------------------------------------------------------------------------
// MTTKRP engine
// ---------------------------------------------------------------------------
void Engine::kernel_stats(int which, int reset, double* ms, int64_t* launches, double* bytes, double* flops) {
  static_assert(kStatsEmList == 16, "include/aoadmm_hip.h documents the list pass as class 16");
  static_assert(kStatsPar2Foldin == 17, "include/aoadmm_hip.h documents the fold-in of PARAFAC2 slabs as class 17");
  AO_REQUIRE(which != kStatsFoldin + 1, "kernel_stats: class %d is not assigned", which);
  AO_REQUIRE(which >= 0 && which < kStatsClasses, "kernel_stats: which must be 0 .. %d", kStatsClasses - 1);
  if (which == 2) timers_.profile_reductions = true;
  AO_HIP(hipSetDevice(device_));
  AO_HIP(hipStreamSynchronize(stream_));
  KernelStats& ks = timers_.stats[which];
  for (auto& pr : ks.pending) {
    float t = 0.f;
    AO_HIP(hipEventElapsedTime(&t, pr.first, pr.second));
    ks.ms += t;
    timers_.pool.push_back(pr.first);
    timers_.pool.push_back(pr.second);
  }
  ks.pending.clear();
  // launches that went untimed (event budget exhausted) count at the mean of the timed ones, so ms / launches stays
  // the mean launch duration
  if (ms) *ms = (ks.timed > 0 && ks.timed < ks.launches) ? ks.ms * (double)ks.launches / (double)ks.timed : ks.ms;
  if (launches) *launches = ks.launches;
  if (bytes) *bytes = ks.bytes;
  if (flops) *flops = ks.flops;
  if (reset) { ks.ms = 0; ks.launches = 0; ks.timed = 0; ks.bytes = 0; ks.flops = 0; }
}

// Y = X_(n) X_(n)' of the RESIDENT data of tensor p (cmtf_nvecs.m:31-56, init_coupled_AOADMM_CMTF.m:50-73): the Gram
// matrix whose leading eigenvectors initialise mode `pos` with init_options.nvecs = 1, without another transfer of the
// tensor.  CP blocks (matrices, 3-way): any mode; PARAFAC2 blocks: pos 0 = [X_1 ... X_K] X_k' summed, pos 1 = X_k' X_k
// of slab `slab`.  With a communicator the first mode of a row-sharded block has no local answer (its Gram matrix pairs
// rows of different ranks): AOADMM_ERR_UNSUPPORTED, the caller takes aoadmm_op_unfold_gram with the host array.
void Engine::resident_unfold_gram(int p, int pos, int slab, double* out_host) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);     // out_host may be null: ranks > 0 of a multi-device context
  AO_HIP(hipSetDevice(device_));
  TensorInfo& t = tensors_[p];
  UnfoldGramArgs a;
  int prec = AOADMM_PREC_F64;
  bool reduce = false;
  if (t.par2) {
    const Par2Block& b = t.p2;
    AO_REQUIRE(pos == 0 || pos == 1, "PARAFAC2 block: mode 1 (all slabs) or mode 2 (one slab)");
    for (int k = 0; k < b.K; ++k) AO_REQUIRE(b.have_slab[k], "slab %d of tensor %d has no data", k, p);
    if (b.sparse)
      throw Error(AOADMM_ERR_UNSUPPORTED, fmt("resident unfold_gram: tensor %d holds sparse slabs (their Gram matrices are built on the host)", p));
    if (pos == 0) { a.X = b.X.p; a.n = b.I; a.sa = 1; a.n1 = b.Jtot; a.s1 = b.I; a.n2 = 1; a.s2 = 0; }
    else {
      AO_REQUIRE(slab >= 0 && slab < b.K, "slab %d out of range", slab);
      const int64_t Jk = b.off_h[slab + 1] - b.off_h[slab];
      a.X = b.X.d() + (int64_t)b.I * b.off_h[slab]; a.n = Jk; a.sa = b.I; a.n1 = b.I; a.s1 = 1; a.n2 = 1; a.s2 = 0;
    }
  } else {
    const CpBlock& b = t.blk;
    AO_REQUIRE(b.has_data, "tensor %d has no data", p);
    if (b.sparse)
      throw Error(AOADMM_ERR_UNSUPPORTED, fmt("resident unfold_gram: tensor %d is sparse (the Gram matrix of its unfolding is built on the host)", p));
    AO_REQUIRE((b.nd == 2 || b.nd == 3) && pos >= 0 && pos < b.nd, "unfold_gram handles matrices and 3-way tensors");
    if (sharded() && pos == 0)
      throw Error(AOADMM_ERR_UNSUPPORTED, "resident unfold_gram: the first mode of a row-sharded block pairs rows of different ranks");
    if (b.x_released)
      throw Error(AOADMM_ERR_UNSUPPORTED, "resident unfold_gram: the natural-layout array was released (only the pass copies are resident)");
    const int64_t I = b.dims[0], Ip = b.X.pad0, J = b.dims[1], K = b.nd == 3 ? b.dims[2] : 1;
    prec = b.X.prec;
    a.X = b.X.data.p;
    if (pos == 0) { a.n = I; a.sa = 1; a.n1 = J * K; a.s1 = Ip; a.n2 = 1; a.s2 = 0; }
    else if (pos == 1) { a.n = J; a.sa = Ip; a.n1 = I; a.s1 = 1; a.n2 = K; a.s2 = Ip * J; }
    else { a.n = K; a.sa = Ip * J; a.n1 = Ip * J; a.s1 = 1; a.n2 = 1; a.s2 = 0; }   // padding rows are zeros
    reduce = sharded();                                 // partial sums over this rank's rows
  }
  DevBuf ws, y;
  ws.alloc(unfold_gram_ws_bytes(a));
  y.alloc((size_t)a.n * a.n * sizeof(double));
  unfold_gram(a, prec, ws.d(), y.d(), stream_);
  if (reduce) allreduce(y.d(), a.n * a.n);
  if (out_host) AO_HIP(hipMemcpyAsync(out_host, y.p, (size_t)a.n * a.n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  AO_HIP(hipStreamSynchronize(stream_));
}

// The r leading eigenvectors of X_(n) X_(n)' for the RESIDENT sparse data of tensor p (the nvecs start of
// cmtf_nvecs.m:54-56 without the I_n x I_n Gram matrix): block subspace iteration on the nonzeros, sparse_nvecs.h.
// Sparse CP blocks: any mode; PARAFAC2 blocks with sparse slabs: pos 0 (sum_k X_k X_k' = Xcat Xcat',
// init_coupled_AOADMM_CMTF.m first-mode branch).  Every rank of a communicator holds all nonzeros and computes the
// same bits: no collective.
void Engine::resident_nvecs(int p, int pos, int r, const aoadmm_nvecs_options* opt, double* U_host, int64_t ldU,
                            double* eig_host, aoadmm_nvecs_info* info) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_HIP(hipSetDevice(device_));
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(pos >= 0 && pos < t.nmodes, "tensor mode %d out of range", pos);
  CooBlock* coo = nullptr;
  if (t.par2) {
    Par2Block& b = t.p2;
    for (int k = 0; k < b.K; ++k) AO_REQUIRE(b.have_slab[k], "slab %d of tensor %d has no data", k, p);
    if (!b.sparse)
      throw Error(AOADMM_ERR_UNSUPPORTED, fmt("resident nvecs: tensor %d holds dense slabs (use aoadmm_resident_unfold_gram)", p));
    if (pos != 0)
      throw Error(AOADMM_ERR_UNSUPPORTED, "resident nvecs: only the first mode of a PARAFAC2 block (the B_k and C modes start on the host)");
    coo = &b.sp.coo;
  } else {
    CpBlock& b = t.blk;
    AO_REQUIRE(b.has_data, "tensor %d has no data", p);
    if (!b.sparse)
      throw Error(AOADMM_ERR_UNSUPPORTED, fmt("resident nvecs: tensor %d is dense (use aoadmm_resident_unfold_gram)", p));
    if (b.coo.sharded)
      throw Error(AOADMM_ERR_UNSUPPORTED, fmt("resident nvecs: the nonzeros of tensor %d are sharded over the ranks (the fiber lists need all of them: upload with aoadmm_tensor_upload_coo)", p));
    coo = &b.coo;
  }
  AO_REQUIRE(coo->nnz >= 1, "resident nvecs: tensor %d has no nonzeros", p);
  AO_REQUIRE(r >= 1 && r <= std::min<int64_t>(coo->dims[pos], kMaxRank), "resident nvecs: r = %d outside 1..%lld", r,
             (long long)std::min<int64_t>(coo->dims[pos], kMaxRank));
  AO_REQUIRE(U_host == nullptr || ldU >= coo->dims[pos], "resident nvecs: ldU %lld < %lld rows", (long long)ldU,
             (long long)coo->dims[pos]);
  NvecsLists lists;                                    // freed on return
  nvecs_build_lists(lists, *coo, pos, stream_);
  sparse_nvecs(lists, r, opt, U_host, ldU, eig_host, info, coo->slot_row, coo->slot_val, &timers_, stream_);
}

void Engine::resident_mttkrp(int p, int pos, double* out_host, float* ms) {
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_HIP(hipSetDevice(device_));
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(pos >= 0 && pos < t.nmodes, "tensor mode %d out of range", pos);
  for (int i = 0; i < t.nmodes; ++i) AO_REQUIRE(modes_[t.modes[i]].has_fac, "G.fac{%d} missing", t.modes[i] + 1);
  FactorRef facs[8];
  factor_refs(t, facs);
  ModeInfo& mi = modes_[t.modes[pos]];
  ensure_mode_work(mi);
  hipEvent_t e0, e1;
  AO_HIP(hipEventCreate(&e0)); AO_HIP(hipEventCreate(&e1));
  AO_HIP(hipEventRecord(e0, stream_));
  t.blk.cached_mode = -1;                              // a full MTTKRP: tensor pass + reduction, on the pass's resident copy
  block_mttkrp(block_ctx(), t.blk, pos, facs, mi.R, 1.0, mi.A.d(), mi.rows, true, nullptr, 0, true, true);
  t.blk.cached_mode = -1;                              // the solver's own factors may differ from what this pass used
  AO_HIP(hipEventRecord(e1, stream_));
  AO_HIP(hipEventSynchronize(e1));
  float tms = 0.f;
  AO_HIP(hipEventElapsedTime(&tms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (ms) *ms = tms;
  if (out_host) {
    AO_HIP(hipMemcpyAsync(out_host, mi.A.p, (size_t)mi.rows * mi.R * sizeof(double), hipMemcpyDeviceToHost, stream_));
    AO_HIP(hipStreamSynchronize(stream_));
  }
}

}  // namespace aoadmm
