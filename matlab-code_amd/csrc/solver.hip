// Engine implementation: see solver.h.  Reference control flow:
// functions/cmtf_fun_AOADMM.m:87-476 (outer loop), :1213-1363 (objective),
// functions/evaluate_stopping_conditions.m.  This file launches no kernel of its own.
#include "solver.h"
#include "em.h"
#include "hosteig.h"

#include <rccl/rccl.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <set>

namespace aoadmm {

#define AO_NCCL(expr)                                                                          \
  do {                                                                                         \
    ncclResult_t r__ = (expr);                                                                 \
    if (r__ != ncclSuccess)                                                                    \
      throw Error(AOADMM_ERR_RCCL, fmt("%s failed: %s", #expr, ncclGetErrorString(r__)));      \
  } while (0)

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
  if (comm_) (void)ncclCommDestroy(comm_);
  if (side_ev_) (void)hipEventDestroy(side_ev_);
  if (side_) (void)hipStreamDestroy(side_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

// ---------------------------------------------------------------------------
// communicator
// ---------------------------------------------------------------------------
void Engine::comm_init(const char id[128], int rank, int world, bool share_only) {
  AO_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank/world %d/%d", rank, world);
  AO_REQUIRE(id != nullptr || world == 1, "a communicator of %d ranks needs the id from aoadmm_comm_unique_id", world);
  AO_HIP(hipSetDevice(device_));
  if (comm_) { (void)ncclCommDestroy(comm_); comm_ = nullptr; }
  local_.reset();
  if (id != nullptr) {               // world == 1 with an id: one-rank communicator (exercises the RCCL path on one GPU)
    ncclUniqueId uid;
    static_assert(sizeof(uid) <= 128, "unique id larger than the ABI buffer");
    std::memcpy(&uid, id, sizeof(uid));
    // share_only (aoadmm_comm_init_rank_share): this engine takes rank `rank` of `world` in every sharding decision
    // but its communicator has ONE rank, so the collectives run (ncclAllReduce on the library's stream) without
    // peers: one rank's share of an N-GPU job, timed on a one-GPU box.  The sums are this rank's partial sums only.
    if (share_only) AO_NCCL(ncclCommInitRank(&comm_, 1, uid, 0));
    else AO_NCCL(ncclCommInitRank(&comm_, world, uid, rank));
  }
  rank_ = rank;
  world_ = world;
  share_only_ = share_only;
  aborted_ = false;
}

// Process-local group: engines driven by threads of ONE process (on one device or several) meet at a
// mutex/condvar barrier and add their buffers through host staging, in rank order, so every rank gets the same
// bits.  It exists so the sharded data path (row blocks, own-rows buffers, objective partial sums) can be run with
// world > 1 on a one-GPU box, where RCCL refuses two ranks on one device.  Not a transport for production: the
// data crosses PCIe twice per collective.
struct LocalGroup {
  std::mutex m;
  std::condition_variable cv;
  int world = 0, arrived = 0, joined = 0;
  uint64_t gen = 0;
  bool aborted = false;                       // a rank failed outside the collectives: nobody waits for it any more
  std::vector<std::vector<double>> stage;     // one host buffer per rank
  void barrier() {
    std::unique_lock<std::mutex> lk(m);
    if (aborted) throw Error(AOADMM_ERR_RCCL, "local group: aborted after a failure on another rank");
    const uint64_t g = gen;
    if (++arrived == world) {
      arrived = 0;
      ++gen;
      cv.notify_all();
      return;
    }
    if (!cv.wait_for(lk, std::chrono::seconds(120), [&] { return gen != g || aborted; }))
      throw Error(AOADMM_ERR_RCCL, "local group: a rank did not reach the collective within 120 s");
    if (gen == g) throw Error(AOADMM_ERR_RCCL, "local group: aborted after a failure on another rank");
  }
  void abort() {
    std::lock_guard<std::mutex> lk(m);
    aborted = true;
    cv.notify_all();
  }
};
static std::mutex g_groups_mutex;
static std::map<int, std::shared_ptr<LocalGroup>> g_groups;

void Engine::comm_init_local(int key, int rank, int world) {
  AO_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank/world %d/%d", rank, world);
  if (comm_) { (void)ncclCommDestroy(comm_); comm_ = nullptr; }
  std::lock_guard<std::mutex> lk(g_groups_mutex);
  std::shared_ptr<LocalGroup>& g = g_groups[key];
  if (!g || g->joined == g->world) {           // first rank of a new (or re-used) key
    g = std::make_shared<LocalGroup>();
    g->world = world;
    g->stage.resize(world);
  }
  AO_REQUIRE(g->world == world, "local group %d was created for %d ranks, not %d", key, g->world, world);
  g->joined++;
  local_ = g;
  rank_ = rank;
  world_ = world;
  aborted_ = false;
}

void Engine::comm_abort() {
  aborted_ = true;                              // sticky: every later collective, solve or upload of this engine throws
  if (local_) local_->abort();
  ncclComm_t c = nullptr;
  {
    std::lock_guard<std::mutex> lk(comm_mu_);
    c = comm_;
    comm_ = nullptr;
  }
  // outside the lock: the owner thread may sit inside ncclAllReduce's enqueue with a copy of the handle
  if (c) (void)ncclCommAbort(c);                // the collective kernels of this rank see the flag and exit
}

void Engine::require_usable() const {
  if (aborted_) throw Error(AOADMM_ERR_RCCL, "context unusable: its communicator was aborted after a failure on another rank");
}

void Engine::comm_info(int* nccl_version, int* comm_ranks, char* lib_path, int cap) const {
  if (nccl_version) {
    int v = 0;
    AO_NCCL(ncclGetVersion(&v));
    *nccl_version = v;
  }
  if (comm_ranks) {
    int n = local_ ? world_ : 0;
    std::lock_guard<std::mutex> lk(comm_mu_);
    if (comm_) AO_NCCL(ncclCommCount(comm_, &n));
    *comm_ranks = n;
  }
  if (lib_path && cap > 0) {
    lib_path[0] = 0;
    Dl_info di;
    if (dladdr(reinterpret_cast<const void*>(&ncclGetVersion), &di) && di.dli_fname) {
      std::strncpy(lib_path, di.dli_fname, (size_t)cap - 1);
      lib_path[cap - 1] = 0;
    }
  }
}

void Engine::allreduce(double* buf, int64_t n) { allreduce_from(buf, buf, n); }

// recv = sum over ranks of send (send == recv: in place)
void Engine::allreduce_from(const double* send, double* buf, int64_t n) {
  if (n <= 0) return;
  if (aborted_) throw Error(AOADMM_ERR_RCCL, "communicator aborted after a failure on another rank");
  if (local_) {
    LocalGroup& g = *local_;
    std::vector<double>& mine = g.stage[rank_];
    mine.resize((size_t)n);
    AO_HIP(hipMemcpyAsync(mine.data(), send, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
    AO_HIP(hipStreamSynchronize(stream_));
    g.barrier();                                // every rank has staged its contribution
    std::vector<double> tot((size_t)n, 0.0);
    for (int r = 0; r < g.world; ++r) {
      AO_REQUIRE((int64_t)g.stage[r].size() == n, "local group: rank %d brought %lld values, rank %d brought %lld", r,
                 (long long)g.stage[r].size(), rank_, (long long)n);
      for (int64_t i = 0; i < n; ++i) tot[i] += g.stage[r][i];
    }
    g.barrier();                                // every rank has read all contributions
    AO_HIP(hipMemcpyAsync(buf, tot.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream_));
    AO_HIP(hipStreamSynchronize(stream_));
    return;
  }
  ncclComm_t c = nullptr;
  {
    std::lock_guard<std::mutex> lk(comm_mu_);
    if (aborted_) throw Error(AOADMM_ERR_RCCL, "communicator aborted after a failure on another rank");
    c = comm_;
  }
  if (!c) {
    // a sharded engine without a transport would go on with its partial sums: never silently
    if (world_ > 1) throw Error(AOADMM_ERR_RCCL, fmt("rank %d of %d has no communicator", rank_, world_));
    if (send != buf) AO_HIP(hipMemcpyAsync(buf, send, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    return;
  }
  // enqueued outside the lock so that comm_abort() from the caller's thread never waits behind a stuck enqueue
  AO_NCCL(ncclAllReduce(send, buf, (size_t)n, ncclDouble, ncclSum, c, stream_));
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

void Engine::model_end() {
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
  for (int c = 0; c < n_couplings_; ++c) {
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
  {
    // one arena for what the host reads back per outer iteration, so that one copy fetches it
    const size_t nsl = (size_t)(n_modes_ * (kSlotsPerMode + kResidPerMode) + 2 * n_tensors_ + 16 + 4 * n_tensors_) * sizeof(double);
    const size_t nct = (size_t)(n_modes_ + n_couplings_ + 1) * sizeof(AdmmCtl);
    const size_t off_ctl = (size_t)round_up((int64_t)nsl, 64);
    size_t tot = (size_t)round_up((int64_t)(off_ctl + nct), 64);
    std::vector<size_t> off_p2(n_tensors_, 0);
    for (int p = 0; p < n_tensors_; ++p)
      if (tensors_[p].par2) { off_p2[p] = tot; tot += ((size_t)6 * tensors_[p].p2.K + 1) * sizeof(double); }
    for (int p = 0; p < n_tensors_; ++p)            // views of the previous arena go before it does
      if (tensors_[p].par2) { tensors_[p].p2.res.release(); tensors_[p].p2.q.release(); tensors_[p].p2.regv.release(); }
    ctls_.release(); slots_.release();
    readback_.alloc(tot);
    AO_HIP(hipMemsetAsync(readback_.p, 0, readback_.bytes, stream_));
    char* base = readback_.as<char>();
    slots_.view(base, nsl);
    ctls_.view(base + off_ctl, nct);
    for (int p = 0; p < n_tensors_; ++p) {
      if (!tensors_[p].par2) continue;
      Par2Block& b = tensors_[p].p2;
      char* q = base + off_p2[p];
      b.res.view(q, (size_t)(b.K + 1) * 8);
      b.q.view(q + (size_t)(b.K + 1) * 8, (size_t)b.K * 4 * 8);
      b.regv.view(q + (size_t)(5 * b.K + 1) * 8, (size_t)b.K * 8);
    }
  }
  AO_HIP(hipStreamSynchronize(stream_));
  model_done_ = true;
}

// ---------------------------------------------------------------------------
// data
// ---------------------------------------------------------------------------
void Engine::tensor_upload(int p, const double* data, int prec, int64_t row0, int64_t local_rows) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(!t.par2, "tensor %d is PARAFAC2: use aoadmm_par2_slab_upload", p);
  AO_REQUIRE(local_rows < 0 || !t.blk.sparse, "tensor %d holds sparse data: a row block cannot replace it (use aoadmm_tensor_upload)", p);
  if (t.blk.sparse) { t.blk.coo.clear(); t.blk.sparse = false; }   // a dense upload replaces the sparse form
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
      block_upload(cx, t.blk, t.nmodes, dims, data, prec, 0, I);
    } else {
      int64_t ncols = 1;
      for (int i = 1; i < t.nmodes; ++i) ncols *= dims[i];
      std::vector<double> blk((size_t)local_rows * ncols);
      for (int64_t c = 0; c < ncols; ++c)
        std::memcpy(&blk[(size_t)c * local_rows], data + c * I + row0, (size_t)local_rows * sizeof(double));
      block_upload(cx, t.blk, t.nmodes, dims, blk.data(), prec, row0, local_rows, data);
    }
  } else {
    block_upload(cx, t.blk, t.nmodes, dims, data, prec, row0, local_rows);
  }
  t.normsq_valid = false;
}

// Z.object{p} as a sptensor / sparse matrix (sparse.h): the block keeps the coalesced nonzeros, one sorted copy per
// mode, and drops whatever dense form it had.  Replicated on every rank of a communicator.
void Engine::tensor_upload_coo(int p, int64_t nnz, const int64_t* subs, const double* vals) {
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
  CpBlock& b = t.blk;
  drop_pass_copies(b);
  b.X.data.release(); b.Xt.data.release();
  b.emkr.release(); b.emkr2.release(); b.T.release(); b.frag.release(); b.scratch.release(); b.ft.release();
  b.tmpA.release(); b.tmpB.release(); b.mask.release(); b.maskT.release();
  for (int i = 0; i < 2; ++i) { b.own[i].release(); b.own_bytes[i] = 0; b.own_row0[i] = -1; }
  b.coo = std::move(coo);
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
    double* slot = slots_.d() + n_modes_ * (kSlotsPerMode + kResidPerMode) + 2 * n_tensors_;
    if (t.par2 ? t.p2.has_mask : t.blk.has_mask) {
      // ||miss .* X||^2 (cmtf_AOADMM.m:133-148): the observed-entry sum of squares of a statistics-only EM pass
      // (needs factors on the device: solve() calls this after the state checks)
      em_pass_enqueue(p, 0);
      double h4[4];
      AO_HIP(hipMemcpyAsync(h4, em_slot(p), sizeof h4, hipMemcpyDeviceToHost, stream_));
      AO_HIP(hipStreamSynchronize(stream_));
      t.normsq = h4[3];
      t.normsq_valid = true;
      return t.normsq;
    }
    if (t.par2 && t.p2.sparse) {   // the coalesced values of all slabs; every rank holds all of them
      tensor_sumsq(slot, t.p2.sp.coo.mode[0].val.p, AOADMM_PREC_F64, t.p2.sp.coo.nnz, ws.d(), stream_);
    } else if (t.par2) {   // sum_k ||X_k||_F^2  (cmtf_AOADMM.m:145-155)
      tensor_sumsq(slot, t.p2.X.p, AOADMM_PREC_F64, (int64_t)t.p2.I * t.p2.Jtot, ws.d(), stream_);
    } else if (t.blk.sparse) {     // norm(sptensor)^2 (:132): the coalesced values; every rank holds all of them
      tensor_sumsq(slot, t.blk.coo.mode[0].val.p, AOADMM_PREC_F64, t.blk.coo.nnz, ws.d(), stream_);
    } else {
      AO_REQUIRE(!t.blk.x_released, "internal: ||X||^2 of tensor %d asked for after its natural-layout array was released", p);
      tensor_sumsq(slot, t.blk.X.data.p, t.blk.X.prec, t.blk.X.elems_padded(), ws.d(), stream_);
      allreduce(slot, 1);
    }
    double v = 0;
    AO_HIP(hipMemcpyAsync(&v, slot, sizeof(double), hipMemcpyDeviceToHost, stream_));
    AO_HIP(hipStreamSynchronize(stream_));
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
  double* slot = slots_.d() + n_modes_ * (kSlotsPerMode + kResidPerMode) + 2 * n_tensors_;
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
  b.has_mask = true;
  drop_pass_copies(b);                               // the imputation would have to update them too
  t.normsq_valid = false;
}

bool Engine::has_missing() const {
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].par2 ? tensors_[p].p2.has_mask : tensors_[p].blk.has_mask) return true;
  return false;
}

double* Engine::em_slot(int p) const {
  return slots_.d() + n_modes_ * (kSlotsPerMode + kResidPerMode) + 2 * n_tensors_ + 16 + 4 * p;
}

// One EM pass over tensor p with the current factors: {num, den, obs_res, obs_x2} -> em_slot(p), all-reduced
// over the row shards; update = 1 also overwrites the missing entries with the model (:416-435).
void Engine::em_pass_enqueue(int p, int update, bool fuse_next_pass) {
  TensorInfo& t = tensors_[p];
  if (t.par2) {
    Par2Block& b = t.p2;
    EmPar2Args a;
    a.X = b.X.d(); a.mask = b.mask.as<uint8_t>();
    a.A = modes_[t.modes[0]].fac.d(); a.B = modes_[t.modes[1]].fac.d(); a.C = modes_[t.modes[2]].fac.d();
    a.off = b.off_d.as<int64_t>(); a.K = b.K; a.I = b.I; a.R = b.R; a.update = update;
    emws_.ensure((size_t)b.K * 4 * sizeof(double));
    em_par2_pass(a, emws_.d(), em_slot(p), stream_);
    return;
  }
  CpBlock& b = t.blk;
  const ModeInfo& m0 = modes_[t.modes[0]];
  const ModeInfo& m1 = modes_[t.modes[1]];
  EmCpArgs a;
  a.X = b.X.data.p; a.mask = b.mask.as<uint8_t>();
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
  if (fuse_next_pass && update && b.nd == 3 && em_cp_can_fuse(a, b.X.prec) && b.dims[1] <= 65535 &&
      b.dims[2] <= 65535 && !small_direct(sharded(), b, a.R)) {
    for (int i = 0; i < t.nmodes; ++i) facs[i] = factor_ref(modes_[t.modes[i]]);
    const std::vector<int> seq = update_sequence(p);
    const int pos0 = seq.empty() ? 0 : seq[0];
    int best = -1;
    for (int cand = 2; cand >= 1; --cand) {
      if (cand == pos0) continue;
      const int dist = next_update_distance(pos0, cand, seq.data(), (int)seq.size());
      if (dist > best) { best = dist; fused_c = cand; }
    }
    // test hook (read per call): contract the second mode whenever that is allowed, so that the strip's walk along
    // mode 2 with the fused contraction is exercised by models whose update order would never pick it
    if (getenv("AOADMM_EM_FUSE_SECOND_MODE") != nullptr && pos0 != 1) fused_c = 1;
    const int64_t J = b.dims[1], K = b.dims[2];
    a.walk = fused_c == 1 ? 1 : 2;
    fpl = fused_c == 2 ? make_plan(1, 0, a.Ipad * J, a.Ipad * J, K, a.R, b.X.prec)
                       : make_plan(K, a.Ipad * J, a.Ipad, a.Ipad, J, a.R, b.X.prec);
    fpl.nchunk = em_cp_fused_chunks(a, b.X.prec);
    b.T.ensure(fpl.t_bytes());
    a.T = b.T.p;
    a.t_chunk_stride = fpl.trows() * a.R;
  }
  em_cp_pass(a, b.X.prec, emws_.d(), em_slot(p), stream_);
  if (b.nd == 2 && update) {
    // same imputation on the transposed copy (roles of the two factors swapped); its statistics are discarded
    EmCpArgs at = a;
    at.X = b.Xt.data.p; at.mask = b.maskT.as<uint8_t>();
    at.A = m1.fac.d(); at.ldA = m1.rows; at.B = m0.fac.d() + (sharded() ? b.row0 : 0); at.ldB = m0.rows;
    at.I = b.dims[1]; at.Ipad = b.Xt.pad0; at.J = b.dims[0];
    const size_t wsb = em_cp_ws_bytes(at.Ipad, at.J, 1);
    emws_.ensure(wsb + 64);
    em_cp_pass(at, b.Xt.prec, emws_.d(), emws_.d() + wsb / sizeof(double), stream_);   // statistics to a scratch tail
  }
  allreduce(em_slot(p), 4);
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
  AO_REQUIRE(which >= 0 && which <= 3, "kernel_stats: which must be 0, 1, 2 or 3");
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

// The first tensor pass of the next outer iteration does not depend on the host's stopping decision, so
// it is enqueued before the host waits for the objective values: the round trip hides behind it.
bool Engine::prefetch_next_contraction(const aoadmm_options& opt) {
  if (!opt.use_dimtree) return false;
  for (int cid = -1; cid < n_couplings_; ++cid) {
    for (int p = 0; p < n_tensors_; ++p)
      for (int m = 0; m < n_modes_; ++m) {
        const ModeInfo& mi = modes_[m];
        if (mi.coupling != cid || mi.tensor != p) continue;
        TensorInfo& t = tensors_[p];                      // first mode the next iteration updates
        if (t.par2 || t.blk.sparse || t.blk.nd != 3 || small_direct(sharded(), t.blk, mi.R)) return false;
        FactorRef facs[8];
        for (int i = 0; i < t.nmodes; ++i) {
          const ModeInfo& o = modes_[t.modes[i]];
          facs[i] = factor_ref(o);
        }
        std::vector<int> seq = update_sequence(p);
        const KernelStats* ks = timers_.stats;
        const int64_t before = ks[0].launches + ks[1].launches;
        ensure_contraction(block_ctx(), t.blk, mi.pos, facs, mi.R, true, seq.data(), (int)seq.size());
        return ks[0].launches + ks[1].launches > before;     // false: the cached pass still serves
      }
  }
  return false;
}

std::vector<int> Engine::update_sequence(int p) const {
  // order in which the positions of tensor p are updated inside one outer iteration:
  // uncoupled modes first, then coupling ids ascending (cmtf_fun_AOADMM.m:10,89-93)
  std::vector<int> seq;
  const TensorInfo& t = tensors_[p];
  for (int cid = -1; cid < n_couplings_; ++cid)
    for (int i = 0; i < t.nmodes; ++i)
      if (modes_[t.modes[i]].coupling == cid) seq.push_back(i);
  return seq;
}

// ---------------------------------------------------------------------------
// per-mode pieces of the outer loop
// ---------------------------------------------------------------------------
void Engine::ensure_mode_work(ModeInfo& mi) {
  const size_t nR = (size_t)mi.rows * mi.R * sizeof(double), RR = (size_t)mi.R * mi.R * sizeof(double);
  mi.A.ensure(nR); mi.Ab.ensure(nR);
  mi.gram.ensure(RR); mi.C.ensure(RR); mi.Bsys.ensure(RR); mi.L.ensure(RR); mi.Binv.ensure(RR);
  mi.rho.ensure(64);
  mi.Zold.ensure(nR); mi.V.ensure(nR); mi.Znew.ensure(nR); mi.RHS.ensure(nR); mi.TD.ensure(nR); mi.tmp.ensure(nR);
  mi.part.ensure((size_t)admm_partials(mi.rows) * 4 * sizeof(double));
  if (mi.constrained) mi.proxws.ensure(prox_ws_bytes(mi.prox.type, mi.rows, mi.R));
  atbws_.ensure(atb_ws_bytes(mi.rows, mi.R, mi.R));
}

// Gram of the current factor (:66, :148); the same kernel leaves a row-major copy of the factor for the T
// reductions and closes the ADMM loop that produced the factor.  Call BEFORE bumping mi.version.
void Engine::compute_gram(ModeInfo& mi, const LoopEnd* close) {
  mi.facT.ensure((size_t)mi.rows * mi.R * sizeof(double));
  atb_small(mi.gram.d(), mi.fac.d(), mi.rows, mi.fac.d(), mi.rows, mi.rows, mi.R, mi.R, atbws_.d(), nullptr, stream_,
            mi.facT.d(), close);
  mi.facT_version = mi.version;
}

void Engine::prepare_mode_system(int m, int nrho, const aoadmm_options& opt) {
  ModeInfo& mi = modes_[m];
  TensorInfo& t = tensors_[mi.tensor];
  if (t.par2) {                      // first PARAFAC2 mode: same system, different A and C (:159-178)
    AO_REQUIRE(mi.pos == 0, "internal: only the first PARAFAC2 mode goes through the CP-style system");
    par2_prepare_modeA(m, nrho, opt);
    return;
  }
  FactorRef facs[8];
  for (int i = 0; i < t.nmodes; ++i) {
    const ModeInfo& o = modes_[t.modes[i]];
    facs[i] = factor_ref(o);
  }
  std::vector<int> seq = update_sequence(mi.tensor);
  SysBuild sb;
  sb.ngram = 0;
  for (int i = 0; i < t.nmodes; ++i)
    if (i != mi.pos) sb.grams[sb.ngram++] = modes_[t.modes[i]].gram.d();     // :98-103, :109,:112
  sb.Cpre = nullptr;
  sb.w = t.weight;
  sb.ridge = has_ridge_ ? mi.ridge : 0.0;
  sb.bsum_half = opt.bsum ? opt.bsum_weight / 2 : 0.0;
  sb.rho_scale = 1.0;
  sb.nrho = nrho;
  sb.R = mi.R;
  sb.C = mi.C.d(); sb.rho = mi.rho.d(); sb.Bsys = mi.Bsys.d(); sb.L = mi.L.d();
  sb.Binv = nrho > 0 ? mi.Binv.d() : nullptr;
  sb.ctl = ctl_of_mode(m);
  const int cty = mi.coupling >= 0 ? couplings_[mi.coupling].type : -1;
  if (cty == 2) sb.Madd = mi.HHt.d();
  // The system needs the Gram matrices only: it rides in the launch of the reduction that finishes the MTTKRP (one
  // extra workgroup) when that path is taken, else it gets its own launch behind the MTTKRP.
  bool rode = false;
  block_mttkrp(block_ctx(), t.blk, mi.pos, facs, mi.R, t.weight, mi.A.d(), mi.rows, opt.use_dimtree != 0, seq.data(), (int)seq.size(), true,
               false, &sb, &rode);
  if (!rode) sys_build(sb, stream_);
  if (cty == 1 || cty == 5) {                       // B = V diag(mu) V' for the Sylvester solve of the inner loop
    mi.eV.ensure((size_t)mi.R * mi.R * sizeof(double)); mi.eMu.ensure((size_t)mi.R * sizeof(double));
    sym_eig_small(mi.Bsys.d(), mi.R, mi.eMu.d(), mi.eV.d(), stream_);
  }
  t.last_pos = mi.pos;                                                        // :121-123
  mi.Aeff = mi.A.d();
  if (opt.bsum) {                                                             // :124-127
    Coef c[2] = {coef(1.0), coef(opt.bsum_weight / 2)};
    const double* x[2] = {mi.A.d(), mi.fac.d()};
    ew_lincomb(mi.Ab.d(), mi.rows * mi.R, 2, c, x, nullptr, stream_);
    mi.Aeff = mi.Ab.d();
  }
}

// see the end of the outer loop in solve(): the first uncoupled CP mode of the next iteration, prepared ahead
void Engine::prepare_next_first_mode(const aoadmm_options& opt) {
  for (int p = 0; p < n_tensors_; ++p)
    for (int m = 0; m < n_modes_; ++m) {
      const ModeInfo& mi = modes_[m];
      if (mi.coupling != -1 || mi.tensor != p) continue;
      if (tensors_[p].par2 && mi.pos != 0) return;  // a PARAFAC2 B_k or C mode comes first: nothing ahead
      prepare_mode_system(m, mi.constrained ? 1 : 0, opt);   // (the first PARAFAC2 mode goes through the same call, :159-178)
      prepared_mode_ = m;
      return;
    }
}

void Engine::update_uncoupled_cp_mode(int m, const aoadmm_options& opt) {
  ModeInfo& mi = modes_[m];
  if (prepared_mode_ == m) prepared_mode_ = -1;     // MTTKRP and system were enqueued at the end of the last iteration
  else prepare_mode_system(m, mi.constrained ? 1 : 0, opt);
  AdmmCtl* ctl = ctl_of_mode(m);
  LoopEnd le;
  GramFold gf;
  if (!mi.constrained) {
    // G.fac{m} = A{m}/B{m}  (:134): B is symmetric positive definite -> Cholesky solve
    row_solve(mi.fac.d(), mi.rows, mi.Aeff, mi.rows, mi.L.d(), mi.rows, mi.R, nullptr, stream_);
  } else if (admm_path(mi.rows, mi.R, mi.prox.type, opt.MaxInnerIters, true, mi.proxws.d() != nullptr) == kAdmmPathWg) {
    // short mode: loop, Gram matrix and row-major copy in one launch of one workgroup
    WgLoopU wa;
    wa.A = mi.Aeff; wa.Binv = mi.Binv.d(); wa.L = mi.L.d(); wa.rho = mi.rho.d(); wa.rho_prox = mi.rho.d();
    wa.fac = mi.fac.d(); wa.Z = mi.Z.d(); wa.mu = mi.mu.d();
    wa.rows = mi.rows; wa.R = mi.R; wa.per_row = 0;
    wa.ptype = mi.prox.type; wa.p0 = mi.prox.p0; wa.p1 = mi.prox.p1;
    wa.max_inner = opt.MaxInnerIters; wa.tol_pr = opt.innerRelPrTol_constr; wa.tol_du = opt.innerRelDualTol_constr;
    wa.ctl = ctl;
    mi.facT.ensure((size_t)mi.rows * mi.R * sizeof(double));
    wa.gram = mi.gram.d(); wa.facT = mi.facT.d();
    admm_loop_wg(wa, stream_);
    mi.version++;
    mi.facT_version = mi.version;
    return;
  } else {
    AdmmMode am;
    am.A = mi.Aeff; am.L = mi.L.d(); am.Binv = mi.Binv.d(); am.rho = mi.rho.d();
    am.fac = mi.fac.d(); am.Z = mi.Z.d(); am.mu = mi.mu.d();
    am.rows = mi.rows; am.R = mi.R; am.prox = mi.prox;
    mi.facT.ensure((size_t)mi.rows * mi.R * sizeof(double));
    atbws_.ensure((size_t)cdiv(mi.rows, 16) * mi.R * mi.R * sizeof(double));
    gf.ws = atbws_.d(); gf.At = mi.facT.d();
    admm_constrained_loop(am, mi.part.d(), mi.V.d(), mi.Znew.d(), mi.proxws.d(), ctl, opt.MaxInnerIters,
                          opt.innerRelPrTol_constr, opt.innerRelDualTol_constr, stream_, &le, &gf);
  }
  mi.version++;
  if (gf.nb > 0) {                                                            // :148, partials left by the loop's last launch
    atb_fin(mi.gram.d(), atbws_.d(), gf.nb, mi.R * mi.R, nullptr, stream_);
    mi.facT_version = mi.version;
  } else {
    compute_gram(mi, le.ctl ? &le : nullptr);                                 // :148
  }
}

// ---------------------------------------------------------------------------
// objective (CMTF_AOADMM_func_eval, :1213-1363)
// ---------------------------------------------------------------------------
void Engine::eval_objective_enqueue(bool first) {
  double* S = slots_.d();
  ReduceBatch rb;                                  // every plain reduction of this evaluation in one launch
  auto add = [&](int kind, double* slot, const double* x, const double* y, int64_t n) {
    ReduceTask k;
    k.kind = kind; k.slot = slot; k.x = x; k.y = y; k.n = n;
    rb.add(k);
  };
  for (int p = 0; p < n_tensors_; ++p) {
    TensorInfo& t = tensors_[p];
    const bool masked = t.par2 ? t.p2.has_mask : t.blk.has_mask;
    if (masked && first) em_pass_enqueue(p, 0);  // observed-entry residual (:1224-1226, :1249-1252); later
                                                 // evaluations reuse the statistics of the EM update pass
    if (t.par2) {
      par2_objective_enqueue(t);                 // direct residual (:1262-1264) + internal-coupling gaps (:1355)
      t.eval_shortcut = !masked && !first && t.last_pos == 0;   // remembered for finish_eval: last_pos may move on before
      if (t.eval_shortcut) {                                // shortcut through last_mttkrp / last_had (:1254-1260)
        ModeInfo& lm = modes_[t.modes[0]];
        double* sp = S + n_modes_ * kSlotsPerMode + 2 * p;
        add(RT_DOT, sp + 0, lm.A.d(), lm.fac.d(), lm.rows * lm.R);
        add(RT_DOT, sp + 1, lm.C.d(), lm.gram.d(), (int64_t)lm.R * lm.R);
      }
      continue;
    }
    if (masked) continue;
    if (first) {
      // cp_func.m:47-55 / pca_func.m:29-39: same formula with the first mode's MTTKRP
      ModeInfo& m0 = modes_[t.modes[0]];
      FactorRef facs[8];
      for (int i = 0; i < t.nmodes; ++i) {
        const ModeInfo& o = modes_[t.modes[i]];
        facs[i] = factor_ref(o);
      }
      std::vector<int> seq = update_sequence(p);
      block_mttkrp(block_ctx(), t.blk, 0, facs, m0.R, t.weight, m0.A.d(), m0.rows, true, seq.data(), (int)seq.size());
      SysBuild sb;
      sb.ngram = 0;
      for (int i = 1; i < t.nmodes; ++i) sb.grams[sb.ngram++] = modes_[t.modes[i]].gram.d();
      sb.Cpre = nullptr; sb.w = t.weight; sb.ridge = 0; sb.bsum_half = 0; sb.rho_scale = 1; sb.nrho = 1; sb.R = m0.R;
      sb.C = m0.C.d(); sb.rho = m0.rho.d(); sb.Bsys = m0.Bsys.d(); sb.L = m0.L.d(); sb.ctl = nullptr;
      sys_build(sb, stream_);
      t.last_pos = 0;
    }
    ModeInfo& lm = modes_[t.modes[t.last_pos]];
    double* sp = S + n_modes_ * kSlotsPerMode + 2 * p;
    add(RT_DOT, sp + 0, lm.A.d(), lm.fac.d(), lm.rows * lm.R);                 // f_2 * w
    add(RT_DOT, sp + 1, lm.C.d(), lm.gram.d(), (int64_t)lm.R * lm.R);          // f_3
  }
  for (int m = 0; m < n_modes_; ++m) {
    ModeInfo& mi = modes_[m];
    if (mi.slabs) continue;                      // per-slab ratios come from par2_b_gaps
    double* sm = S + (int64_t)m * kSlotsPerMode;
    const int64_t nm = mi.rows * mi.R;
    add(RT_SUMSQ_DIFF, sm + 0, mi.fac.d(), nullptr, nm);
    if (mi.constrained) {
      add(RT_SUMSQ_DIFF, sm + 1, mi.fac.d(), mi.Z.d(), nm);
      const int ty = mi.prox.type;
      if (ty == AOADMM_C_L2_REG) {
        reg_value(sm + 3, ty, mi.prox.p0, mi.fac.d(), mi.rows, mi.R, redws_.d(), stream_);
      } else if (ty == AOADMM_C_QUADRATIC) {       // eta*trace(x'*L*x) (:67): L*x into the prox workspace, then <x, L*x>
        gemm_small(mi.proxws.d(), mi.rows, mi.prox.Lmat, mi.rows, mi.fac.d(), mi.rows, mi.rows, (int)mi.rows, mi.R, 0,
                   coef(1.0), 0.0, nullptr, stream_);
        ReduceTask k;
        k.kind = RT_DOT; k.slot = sm + 3; k.x = mi.fac.d(); k.y = mi.proxws.d(); k.n = nm; k.scale = mi.prox.p0;
        rb.add(k);
      } else if (ty == AOADMM_C_L1_REG || ty == AOADMM_C_L0_REG || ty == AOADMM_C_RIDGE || ty == AOADMM_C_GL_SMOOTH ||
                 ty == AOADMM_C_TV) {
        ReduceTask k;
        k.kind = RT_REG; k.aux = ty; k.slot = sm + 3; k.x = mi.fac.d(); k.rows = mi.rows; k.R = mi.R; k.scale = mi.prox.p0;
        rb.add(k);
      }
    }
    if (mi.coupling >= 0) {                        // :1303-1329
      CouplingInfo& ci = couplings_[mi.coupling];
      const size_t nimg = (size_t)std::max(nm, mi.img_rows * mi.img_cols) * sizeof(double);
      mi.TD.ensure(nimg); mi.TF.ensure(nimg);
      const double* td = image_d(mi.TD.d(), ci, ci.Delta.d(), mi, nullptr, stream_);
      const double* tf = image_f(mi.TF.d(), ci, mi.fac.d(), mi, nullptr, stream_);
      add(RT_SUMSQ_DIFF, sm + 2, tf, td, mi.img_rows * mi.img_cols);
      if (tf != mi.fac.d()) add(RT_SUMSQ_DIFF, sm + 4, tf, nullptr, mi.img_rows * mi.img_cols);   // ||H*C|| / ||C*H||
    }
    if (rb.n >= kReduceBatchMax - 4) {           // many modes: flush and start the next batch
      reduce_batch(rb, redws_.d(), stream_);
      rb = ReduceBatch();
    }
  }
  reduce_batch(rb, redws_.d(), stream_);
}

static bool stop_one(double f, double fo, const aoadmm_options& o) {
  const double rel = fo > 0 ? std::fabs(fo - f) / fo : std::fabs(fo - f);    // evaluate_stopping_conditions.m:8-15
  return f < o.AbsFuncTol || rel < o.OuterRelTol;
}

void Engine::solve(const aoadmm_options& opt, aoadmm_result* out) {
  require_usable();
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(out != nullptr, "null result");
  AO_REQUIRE(opt.MaxOuterIters >= 0 && opt.MaxInnerIters >= 1, "bad iteration limits");
  AO_HIP(hipSetDevice(device_));
  prepared_mode_ = -1;                                // nothing prepared ahead by an earlier solve is valid for this state
  allow_xp_ = opt.no_permuted_copy == 0;
  if (!allow_xp_)
    for (int p = 0; p < n_tensors_; ++p)
      drop_pass_copies(tensors_[p].blk);
  for (int p = 0; p < n_tensors_; ++p) {
    AO_REQUIRE(tensors_[p].blk.has_data, "tensor %d has no data (Z.object{%d})", p, p + 1);
  }
  for (int m = 0; m < n_modes_; ++m) {
    ModeInfo& mi = modes_[m];
    AO_REQUIRE(mi.has_fac, "G.fac{%d} missing", m + 1);
    if (mi.constrained) AO_REQUIRE(mi.has_Z && mi.has_mu, "G.constraint_fac{%d} / constraint_dual_fac{%d} missing", m + 1, m + 1);
    if (mi.coupling >= 0) {
      AO_REQUIRE(mi.has_muD && mi.muD_rows == mi.img_rows && mi.muD_cols == mi.img_cols, "G.coupling_dual_fac{%d} missing or mis-sized", m + 1);
      AO_REQUIRE(couplings_[mi.coupling].has_state, "G.coupling_fac{%d} missing", mi.coupling + 1);
    }
    ensure_mode_work(mi);
    if (!mi.slabs) compute_gram(mi);                                         // :62-81
  }
  for (int p = 0; p < n_tensors_; ++p) {
    TensorInfo& t = tensors_[p];
    if (t.par2) {
      for (int k = 0; k < t.p2.K; ++k)
        AO_REQUIRE(t.p2.have_P[k] && t.p2.have_mu[k], "G.P{%d}{%d} / G.mu_DeltaB{%d}{%d} missing", p + 1, k + 1, p + 1, k + 1);
    }
    (void)tensor_normsq(p);          // Znorm_const{p}; a masked block needs the factors (statistics-only EM pass)
  }
  const bool has_miss = has_missing();
  for (int p = 0; p < n_tensors_; ++p) {
    TensorInfo& t = tensors_[p];
    if (!t.par2) continue;
    Par2Block& b = t.p2;
    AO_REQUIRE(b.has_DeltaB, "G.DeltaB{%d} missing", p + 1);
    for (int k = 0; k < b.K; ++k) AO_REQUIRE(b.have_P[k] && b.have_mu[k], "G.P{%d}{%d} / G.mu_DeltaB{%d}{%d} missing", p + 1, k + 1, p + 1, k + 1);
    par2_ensure_work(t);
    {
      // slabs over the ranks or every slab on every rank (aoadmm_options.par2_slab_sharding)
      const ModeInfo& mB = modes_[t.modes[1]];
      const bool can = sharded() && world_ > 1 && !b.has_mask && !b.sparse && !(mB.constrained && mB.prox.type == AOADMM_C_TPARAFAC2) &&
                       modes_[t.modes[2]].coupling < 0;     // a coupled C mode needs every row system on every rank
      const bool want = opt.par2_slab_sharding > 0 || (opt.par2_slab_sharding == 0 && b.K / world_ >= 1024);
      const int per = (int)cdiv(b.K, world_);
      // every rank must own a slab, and every rank must reach the same verdict: otherwise repeat the block
      b.slab_sharded = can && want && (int64_t)per * (world_ - 1) < b.K;
      b.k0 = std::min(b.K, per * rank_);
      b.k1 = std::min(b.K, b.k0 + per);
    }
    par2_gram(modes_[t.modes[1]].fac.d(), b.dims(), b.GB.d(), stream_);      // :71-73
    t.last_pos = 2;
  }
  const int nctl = n_modes_ + n_couplings_;
  const int nslots = n_modes_ * kSlotsPerMode + 2 * n_tensors_;
  // pinned landing area + event: the host waits for the objective values only, not for work enqueued
  // behind them (prefetch_next_contraction)
  struct Pinned {
    void* p = nullptr; hipEvent_t ev = nullptr;
    ~Pinned() { if (p) (void)hipHostFree(p); if (ev) (void)hipEventDestroy(ev); }
  } pin;
  // per PARAFAC2 block: K + 1 slab residuals (+ the not-PD flag of sharded slabs), 4 K gap sums, K regulariser values --
  // read back with everything else behind ONE event (three more copies into pageable memory with a stream
  // synchronisation each left the GPU idle for ~60 us per outer iteration of config 4)
  const char* rb_base = readback_.as<char>();
  auto in_arena = [&](const DevBuf& d) {
    return !d.owned && static_cast<const char*>(d.p) >= rb_base && static_cast<const char*>(d.p) + d.bytes <= rb_base + readback_.bytes;
  };
  AO_REQUIRE(in_arena(slots_) && in_arena(ctls_), "read-back arena: slots / loop-control blocks are not views of it");
  AO_HIP(hipHostMalloc(&pin.p, readback_.bytes, hipHostMallocDefault));
  AO_HIP(hipEventCreateWithFlags(&pin.ev, hipEventDisableTiming));
  char* hb = static_cast<char*>(pin.p);
  double* hs = reinterpret_cast<double*>(hb + (slots_.as<char>() - rb_base));
  double* hem = hs + (em_slot(0) - slots_.d());                                // EM statistics, 4 per tensor
  AdmmCtl* hctl = reinterpret_cast<AdmmCtl*>(hb + (ctls_.as<char>() - rb_base));
  std::vector<double*> hp2v(n_tensors_, nullptr);                              // PARAFAC2 per-slab values: res | q | regv
  for (int p = 0; p < n_tensors_; ++p) {
    if (!tensors_[p].par2) continue;
    Par2Block& b = tensors_[p].p2;
    AO_REQUIRE(in_arena(b.res) && in_arena(b.q) && in_arena(b.regv) && b.q.d() == b.res.d() + b.K + 1 &&
               b.regv.d() == b.res.d() + 5 * b.K + 1, "read-back arena: PARAFAC2 block %d keeps its sums elsewhere", p);
    hp2v[p] = reinterpret_cast<double*>(hb + (b.res.as<char>() - rb_base));
  }
  (void)nslots;

  auto enqueue_readback = [&]() {
    AO_HIP(hipMemcpyAsync(hb, readback_.p, readback_.bytes, hipMemcpyDeviceToHost, stream_));
    AO_HIP(hipEventRecord(pin.ev, stream_));
  };
  auto finish_eval = [&](double f[4]) {
    AO_HIP(hipEventSynchronize(pin.ev));
    for (int i = 0; i < nctl; ++i)
      if (hctl[i].notpd)
        throw Error(AOADMM_ERR_NOT_PD, "Cholesky failed: system matrix is not positive definite (chol in cmtf_fun_AOADMM.m:142/273/362)");
    double ft = 0.0, fpar = 0.0, fcon = 0.0;
    int ncon = 0;
    for (int p = 0; p < n_tensors_; ++p) {
      TensorInfo& t = tensors_[p];
      const double* sp = hs + n_modes_ * kSlotsPerMode + 2 * p;
      const bool masked = t.par2 ? t.p2.has_mask : t.blk.has_mask;
      if (t.par2) {
        Par2Block& b = t.p2;
        const double* res = hp2v[p];
        const double* q = res + b.K + 1;
        if (b.slab_sharded && res[b.K] > 0)         // some rank's slabs hit a non-positive-definite system (the slot is only written then)
          throw Error(AOADMM_ERR_NOT_PD, "Cholesky failed in a PARAFAC2 slab system on another rank (chol in cmtf_fun_AOADMM.m:212/240)");
        double fp = 0.0;
        if (masked) fp = hem[4 * p + 2];                                                        // :1249-1252
        else if (t.eval_shortcut) fp = t.normsq - 2.0 * (sp[0] / t.weight) + sp[1];               // :1254-1260
        else for (int k = 0; k < b.K; ++k) fp += res[k];                                        // :1262-1264
        ft += t.weight * fp;                                                                    // :1267
        const ModeInfo& mB = modes_[t.modes[1]];
        double gp = 0.0, gz = 0.0, nb2 = 0.0;
        for (int k = 0; k < b.K; ++k) {
          const double nb = std::sqrt(q[4 * k + 1]);
          gp += std::sqrt(q[4 * k]) / nb;                                                       // :1355
          gz += std::sqrt(q[4 * k + 2]) / nb;                                                   // :1337
          nb2 += q[4 * k + 1];
        }
        fpar += gp;
        if (mB.constrained && mB.prox.type == AOADMM_C_TPARAFAC2) {        // t_smoothness_penalty.m via reg_func (:1276-1277)
          double pen = 0.0;
          for (int k = 1; k < b.K; ++k) pen += q[4 * k + 3];
          ft += mB.prox.p0 * pen;
        }
        if (mB.constrained && prox_has_reg_value(mB.prox.type)) {          // sum_k reg_func(B_k) (:1279-1281)
          const double* rv = res + 5 * b.K + 1;
          for (int k = 0; k < b.K; ++k) ft += rv[k];
        }
        if (mB.constrained) {
          const double g = gz / b.K;                                                            // :1339
          fcon += g;
          if (g != 0.0) ++ncon;
          if (has_ridge_) ft += mB.ridge * nb2;                                                 // :1292-1295 (quirk: only if constrained)
        }
      } else if (masked) {
        ft += t.weight * hem[4 * p + 2];                                       // :1224-1226 = w * ||miss.*(X - M)||^2
      } else {
        const double f2 = sp[0] / t.weight;                                   // last_mttkrp = A*1/w (:121)
        ft += t.weight * (t.normsq - 2.0 * f2 + sp[1]);                        // :1235-1241
      }
    }
    if (fpar > 0) {                                                            // :1360-1362 (quirk: K of the LAST tensor)
      const TensorInfo& tl = tensors_[n_tensors_ - 1];
      fpar /= tl.par2 ? tl.p2.K : 1;
    }
    std::vector<double> cp(n_couplings_, 0.0);
    for (int m = 0; m < n_modes_; ++m) {
      const ModeInfo& mi = modes_[m];
      if (mi.slabs) continue;
      const double* sm = hs + (int64_t)m * kSlotsPerMode;
      const double nf = std::sqrt(sm[0]);
      if (mi.constrained) {
        const int ty = mi.prox.type;
        if (prox_has_reg_value(ty)) ft += sm[3];                               // reg_func (:1272-1288)
        const double g = std::sqrt(sm[1]) / nf;                               // :1341
        fcon += g;
        if (g != 0.0) ++ncon;
      }
      if (has_ridge_) ft += mi.ridge * sm[0];                                  // :1297
      if (mi.coupling >= 0) {                                                  // :1309-1323
        const int cty = couplings_[mi.coupling].type;
        const double den = (cty == 1 || cty == 2 || cty == 5) ? std::sqrt(sm[4]) : nf;
        cp[mi.coupling] += std::sqrt(sm[2]) / den;
      }
    }
    double fc = 0.0; int nc = 0;
    for (double v : cp) { fc += v; if (v != 0.0) ++nc; }
    if (fc > 0) fc /= nc;                                                      // :1327-1329
    if (fcon > 0) fcon /= ncon;                                                // :1346-1348
    f[0] = ft; f[1] = fc; f[2] = fcon; f[3] = fpar;
  };

  double f[4], fo[4];
  eval_objective_enqueue(true);                                                // :32
  enqueue_readback();
  finish_eval(f);
  if (out->func_val_conv) out->func_val_conv[0] = f[0];
  if (out->func_coupl_conv) out->func_coupl_conv[0] = f[1];
  if (out->func_constr_conv) out->func_constr_conv[0] = f[2];
  if (out->func_PAR2_coupl) out->func_PAR2_coupl[0] = f[3];
  if (out->time_at_it) out->time_at_it[0] = 0.0;
  double f_rel_missing = std::nan("");                                          // :30
  if (out->func_rel_missing) out->func_rel_missing[0] = f_rel_missing;
  const bool report = progress_fn_ != nullptr && progress_every_ > 0;
  if (report) progress_fn_(progress_user_, 0, f, f_rel_missing);               // :53-59
  const auto t0 = std::chrono::steady_clock::now();

  int iter = 1;
  bool stop = false;
  while (iter <= opt.MaxOuterIters && !stop) {                                 // :87
    for (ModeInfo& mq : modes_) mq.quad.dirty = true;   // rho moves once per outer iteration ('quadratic regularization', non-symmetric L)
    if (iter == 3)                                      // by now every pass of the schedule has run once: all copies exist
      for (int p = 0; p < n_tensors_; ++p)
        if (!tensors_[p].par2) maybe_release_natural(block_ctx(), tensors_[p].blk, tensors_[p].normsq_valid);
    for (int cid = -1; cid < n_couplings_; ++cid) {                            // :89 (0 = uncoupled first)
      std::vector<int> cm;
      for (int m = 0; m < n_modes_; ++m)
        if (modes_[m].coupling == cid) cm.push_back(m);
      if (cm.empty()) continue;
      std::set<int> ps;
      for (int m : cm) ps.insert(modes_[m].tensor);
      for (int p : ps)                                                         // :91
        for (int m : cm)                                                       // :93
          if (modes_[m].tensor == p) {
            const bool par2 = tensors_[p].par2;
            if (par2 && modes_[m].pos == 1) par2_update_B(m, opt, iter);             // :191-218
            else if (par2 && modes_[m].pos == 2 && cid < 0) par2_update_C(m, opt);   // :219-248
            else if (par2 && modes_[m].pos == 2) par2_prepare_C_coupled(m, couplings_[cid].type, opt);
            else if (cid < 0) update_uncoupled_cp_mode(m, opt);
            else {
              // system of a coupled mode: +rho/2*I (types 0, 3, 4: :269, :336, :358), +rho/2*H*H' (type 2, :314),
              // nothing for the Sylvester types 1, 5 (:288-293, :377-382); +rho/2*I more if constrained
              const int cty = couplings_[cid].type;
              const int con = modes_[m].constrained ? 1 : 0;
              prepare_mode_system(m, (cty == 0 || cty == 3 || cty == 4) ? 1 + con : (cty == 2 ? con : 0), opt);
            }
          }
      if (cid >= 0) {
        coupled_admm(cid, opt);                                                // :277 / :366
        for (int m : cm) { modes_[m].version++; compute_gram(modes_[m]); }      // :393-403
      }
    }
    if (has_miss)                                                              // EM imputation (:408-441)
      for (int p = 0; p < n_tensors_; ++p)
        if (tensors_[p].par2 ? tensors_[p].p2.has_mask : tensors_[p].blk.has_mask)
          em_pass_enqueue(p, 1, opt.use_dimtree != 0 && iter < opt.MaxOuterIters);
    for (int i = 0; i < 4; ++i) fo[i] = f[i];
    if (iter < opt.MaxOuterIters) {
      // The objective needs nothing the first tensor pass of the next iteration writes (frag, T), and that pass does
      // not depend on the stopping decision: the pass goes onto the main stream, the objective kernels and their
      // read-back onto the side stream behind an event, and the main stream takes up its small kernels again only
      // when the objective is through (they overwrite what it reads).  ~50 us per iteration off the critical path.
      // (Only when a pass is actually launched: the cross-stream wait alone costs ~40 us.)
      AO_HIP(hipEventRecord(side_ev_, stream_));
      if (prefetch_next_contraction(opt)) {
        AO_HIP(hipStreamWaitEvent(side_, side_ev_, 0));
        std::swap(stream_, side_);
        try {
          eval_objective_enqueue(false);                                       // :447
          enqueue_readback();
        } catch (...) { std::swap(stream_, side_); throw; }
        std::swap(stream_, side_);
        AO_HIP(hipStreamWaitEvent(stream_, pin.ev, 0));
      } else {
        eval_objective_enqueue(false);                                         // :447
        enqueue_readback();
        // No pass to hide behind: the host now waits ~45 us for the read-back before it can enqueue anything, and the
        // GPU would sit idle.  The MTTKRP (reductions over the cached T) and the system build of the next iteration's
        // first mode depend on no stopping decision and write only that mode's scratch (A, C, rho, B, L, inv, ctl --
        // behind the read-back of this iteration's loop counters in stream order): enqueue them now.
        if (!has_miss) prepare_next_first_mode(opt);
      }
    } else {
      eval_objective_enqueue(false);                                           // :447
      enqueue_readback();
    }
    finish_eval(f);
    if (out->func_val_conv) out->func_val_conv[iter] = f[0];
    if (out->func_coupl_conv) out->func_coupl_conv[iter] = f[1];
    if (out->func_constr_conv) out->func_constr_conv[iter] = f[2];
    if (out->func_PAR2_coupl) out->func_PAR2_coupl[iter] = f[3];
    if (out->time_at_it)
      out->time_at_it[iter] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out->innerIters) {
      for (int m = 0; m < n_modes_; ++m) {
        const ModeInfo& mi = modes_[m];
        double v;
        if (mi.coupling >= 0) v = hctl[n_modes_ + mi.coupling].iters;          // :392
        else if (mi.slabs) v = hctl[m].iters;                                  // :215
        else if (mi.constrained) v = hctl[m].iters;                            // :146
        else v = 1;                                                            // :138
        out->innerIters[(int64_t)(iter - 1) * n_modes_ + m] = v;
      }
    }
    stop = stop_one(f[0], fo[0], opt) && stop_one(f[1], fo[1], opt) && stop_one(f[2], fo[2], opt) &&
           stop_one(f[3], fo[3], opt);                                         // :456
    if (has_miss) {
      double num = 0.0, den = 0.0;
      for (int p = 0; p < n_tensors_; ++p)
        if (tensors_[p].par2 ? tensors_[p].p2.has_mask : tensors_[p].blk.has_mask) { num += hem[4 * p]; den += hem[4 * p + 1]; }
      f_rel_missing = den > 0 ? std::sqrt(num / den) : std::sqrt(num);        // :436-440
      if (out->func_rel_missing) out->func_rel_missing[iter] = f_rel_missing;
      stop = stop && (f_rel_missing < opt.OuterRelTol);                        // :457-459
    }
    if (report && iter % progress_every_ == 0) progress_fn_(progress_user_, iter, f, f_rel_missing);   // :462-468
    ++iter;
  }
  out->f_tensors = f[0]; out->f_couplings = f[1]; out->f_constraints = f[2]; out->f_PAR2_couplings = f[3];
  out->f_rel_missing = f_rel_missing;
  for (int p = 0; p < n_tensors_; ++p)
    if (tensors_[p].par2) par2_gather_slabs(tensors_[p]);
  AO_HIP(hipStreamSynchronize(stream_));
  out->OuterIterations = iter - 1;
  out->exit_code = iter > opt.MaxOuterIters ? 0 : 1;                           // make_exit_flag.m:4-5
  for (int i = 0; i < 4; ++i) out->exit_abs[i] = f[i] < opt.AbsFuncTol ? 1 : 0;
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

void Engine::resident_mttkrp(int p, int pos, double* out_host, float* ms) {
  AO_REQUIRE(model_done_, "call aoadmm_model_end first");
  AO_REQUIRE(p >= 0 && p < n_tensors_, "tensor %d out of range", p);
  AO_HIP(hipSetDevice(device_));
  TensorInfo& t = tensors_[p];
  AO_REQUIRE(pos >= 0 && pos < t.nmodes, "tensor mode %d out of range", pos);
  FactorRef facs[8];
  for (int i = 0; i < t.nmodes; ++i) {
    ModeInfo& o = modes_[t.modes[i]];
    AO_REQUIRE(o.has_fac, "G.fac{%d} missing", t.modes[i] + 1);
    facs[i] = factor_ref(o);
  }
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
