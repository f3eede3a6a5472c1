// Engine: the communicator.  RCCL across processes, a process-local group across the threads of one process; the
// rest of the engine sees allreduce / allreduce_from and the members set here.
#include "solver.h"

#include <rccl/rccl.h>
#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>

namespace aoadmm {

#define AO_NCCL(expr)                                                                          \
  do {                                                                                         \
    ncclResult_t r__ = (expr);                                                                 \
    if (r__ != ncclSuccess)                                                                    \
      throw Error(AOADMM_ERR_RCCL, fmt("%s failed: %s", #expr, ncclGetErrorString(r__)));      \
  } while (0)

void Engine::comm_release() {
  if (comm_) { (void)ncclCommDestroy(comm_); comm_ = nullptr; }
}

void Engine::comm_init(const char id[128], int rank, int world, bool share_only) {
  AO_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank/world %d/%d", rank, world);
  AO_REQUIRE(id != nullptr || world == 1, "a communicator of %d ranks needs the id from aoadmm_comm_unique_id", world);
  AO_HIP(hipSetDevice(device_));
  comm_release();
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
  comm_release();
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

}  // namespace aoadmm
