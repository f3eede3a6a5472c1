// extern "C" boundary of libaoadmm_hip.so (include/aoadmm_hip.h).  No exception
// leaves this file; every entry point returns a status and records the message.
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>

#include "solver.h"
#include "misc.h"
#include "rank_metrics.h"

using namespace aoadmm;

static thread_local std::string g_last_error;

// One process, several GPUs (the shape a MATLAB session needs: SURVEY 8b): the context owns one engine per device
// and one host thread per engine.  Every model/data/state/solve call is handed to all workers at once -- the ranks
// must enter the collectives inside those calls together -- and returns when the last worker is done.
struct MultiCtx {
  std::vector<std::unique_ptr<Engine>> eng;
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv_job, cv_done;
  std::function<void(Engine&, int)> job;
  uint64_t gen = 0;
  int pending = 0;
  bool quit = false;
  bool poisoned = false;                  // set when run() had to abort communicators; never cleared
  std::vector<int> code;
  std::vector<std::string> msg;
  std::vector<char> done;
  // options.Display = 'iter': rank 0's worker queues the rows, the CALLING thread delivers them from inside run()
  // (a MEX callback may only touch MATLAB from the interpreter's thread)
  struct ProgressRow { int iter; double f[4]; double frm; };
  std::deque<ProgressRow> rows;
  aoadmm_progress_fn user_fn = nullptr;
  void* user_arg = nullptr;
  static void queue_row(void* self, int iter, const double f[4], double frm) {
    MultiCtx* mc = static_cast<MultiCtx*>(self);
    ProgressRow r;
    r.iter = iter; r.frm = frm;
    for (int i = 0; i < 4; ++i) r.f[i] = f[i];
    std::lock_guard<std::mutex> lk(mc->m);
    mc->rows.push_back(r);
    mc->cv_done.notify_all();
  }

  void worker(int r, int device) {
    uint64_t seen = 0;
    for (;;) {
      std::function<void(Engine&, int)> f;
      {
        std::unique_lock<std::mutex> lk(m);
        cv_job.wait(lk, [&] { return quit || gen != seen; });
        if (quit) return;
        seen = gen;
        f = job;
      }
      int c = AOADMM_OK;
      std::string w;
      try {
        (void)hipSetDevice(device);
        f(*eng[r], r);
      } catch (const Error& e) { c = e.code; w = e.what(); }
      catch (const std::bad_alloc&) { c = AOADMM_ERR_NOMEM; w = "host allocation failed"; }
      catch (const std::exception& e) { c = AOADMM_ERR_INVALID; w = e.what(); }
      catch (...) { c = AOADMM_ERR_INVALID; w = "unknown failure"; }
      {
        std::lock_guard<std::mutex> lk(m);
        code[r] = c; msg[r] = w; done[r] = 1;
        --pending;
        cv_done.notify_all();             // also on failure: run() starts its grace period for the peers
      }
    }
  }
  // run f on every engine concurrently; progress rows are delivered on this (the caller's) thread while it waits.
  // Throws the failure of the rank that failed by itself: a rank that only reports the abort it received
  // (AOADMM_ERR_RCCL) is passed over when another rank has the cause.
  void run(const std::function<void(Engine&, int)>& f) {
    {
      std::unique_lock<std::mutex> lk(m);
      // sticky: once a peer's communicator had to be aborted the ranks are out of step for good (the aborted ones would
      // skip collectives the failed one still enters), so every later call fails at once instead of computing on
      if (poisoned) throw Error(AOADMM_ERR_RCCL, "multi-device context unusable: a rank failed alone and its peers' communicators were aborted; destroy the context");
      job = f;
      pending = (int)eng.size();
      done.assign(eng.size(), 0);
      code.assign(eng.size(), AOADMM_OK);
      ++gen;
      cv_job.notify_all();
      // A rank that failed alone leaves its peers waiting for it inside a collective.  Failures that every rank
      // detects (bad arguments) finish everywhere within milliseconds; if some rank is still busy kAbortGrace after
      // another one failed, its communicator is aborted so that it returns (the context is unusable afterwards).
      const auto kAbortGrace = std::chrono::seconds(5);
      bool failing = false, aborted = false;
      std::chrono::steady_clock::time_point t_fail;
      for (;;) {
        cv_done.wait_for(lk, std::chrono::milliseconds(500), [&] { return pending == 0 || !rows.empty(); });
        if (!aborted && pending > 0) {
          bool any = false;
          for (size_t r = 0; r < eng.size(); ++r) any = any || (done[r] && code[r] != AOADMM_OK);
          if (any && !failing) { failing = true; t_fail = std::chrono::steady_clock::now(); }
          if (failing && std::chrono::steady_clock::now() - t_fail > kAbortGrace) {
            for (size_t r = 0; r < eng.size(); ++r)
              if (!done[r]) eng[r]->comm_abort();
            aborted = true;
            poisoned = true;
          }
        }
        while (!rows.empty()) {
          const ProgressRow r = rows.front();
          rows.pop_front();
          aoadmm_progress_fn fn = user_fn;
          void* arg = user_arg;
          lk.unlock();
          if (fn) fn(arg, r.iter, r.f, r.frm);
          lk.lock();
        }
        if (pending == 0) break;
      }
    }
    int first = -1;
    for (size_t r = 0; r < eng.size(); ++r)
      if (code[r] != AOADMM_OK && (first < 0 || (code[first] == AOADMM_ERR_RCCL && code[r] != AOADMM_ERR_RCCL))) first = (int)r;
    if (first >= 0) throw Error(code[first], fmt("rank %d: %s", first, msg[first].c_str()));
  }
  ~MultiCtx() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
      cv_job.notify_all();
    }
    for (auto& t : th)
      if (t.joinable()) t.join();
  }
};

struct aoadmm_ctx {
  Engine* eng;          // the engine (single device) or rank 0's engine (multi-device)
  MultiCtx* multi;
};

// f(engine, rank) on the one engine, or on every engine of a multi-device context at once
template <class F>
static void on_engines(aoadmm_ctx* ctx, F&& f) {
  if (ctx->multi) ctx->multi->run(std::function<void(Engine&, int)>(f));
  else f(*ctx->eng, 0);
}

template <class F>
static int guarded(F&& f) {
  try {
    f();
    return AOADMM_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "host allocation failed";
    return AOADMM_ERR_NOMEM;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return AOADMM_ERR_INVALID;
  } catch (...) {
    g_last_error = "unknown failure";
    return AOADMM_ERR_INVALID;
  }
}

#define CTX_OR_FAIL(ctx)                                   \
  if (!(ctx) || !(ctx)->eng) {                             \
    g_last_error = "null context";                         \
    return AOADMM_ERR_INVALID;                             \
  }

extern "C" {

int aoadmm_abi_version(void) { return AOADMM_ABI_VERSION; }
const char* aoadmm_last_error(void) { return g_last_error.c_str(); }

int aoadmm_device_count(int* n) {
  return guarded([&] {
    AO_REQUIRE(n != nullptr, "null pointer");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = (e == hipSuccess) ? c : 0;
  });
}

int aoadmm_create(aoadmm_ctx** ctx, int device) {
  return guarded([&] {
    AO_REQUIRE(ctx != nullptr, "null pointer");
    *ctx = nullptr;
    Engine* e = new Engine(device);
    aoadmm_ctx* c = new aoadmm_ctx;
    c->eng = e;
    c->multi = nullptr;
    *ctx = c;
  });
}

int aoadmm_create_multi(aoadmm_ctx** ctx, int n_devices, const int* devices) {
  return guarded([&] {
    AO_REQUIRE(ctx != nullptr && devices != nullptr && n_devices >= 1 && n_devices <= 64, "bad arguments");
    *ctx = nullptr;
    std::unique_ptr<MultiCtx> mc(new MultiCtx);
    const int n = n_devices;
    mc->eng.resize(n); mc->code.assign(n, AOADMM_OK); mc->msg.resize(n); mc->done.assign(n, 0);
    for (int r = 0; r < n; ++r) mc->eng[r].reset(new Engine(devices[r]));
    for (int r = 0; r < n; ++r) mc->th.emplace_back(&MultiCtx::worker, mc.get(), r, devices[r]);
    bool distinct = true;
    for (int a = 0; a < n; ++a)
      for (int b = a + 1; b < n; ++b) distinct = distinct && devices[a] != devices[b];
    if (n > 1) {
      for (int r = 0; r < n; ++r) mc->eng[r]->set_multi_member();
      if (distinct) {                                 // RCCL over xGMI, one rank per device
        ncclUniqueId uid;
        ncclResult_t r = ncclGetUniqueId(&uid);
        if (r != ncclSuccess) throw Error(AOADMM_ERR_RCCL, fmt("ncclGetUniqueId failed: %s", ncclGetErrorString(r)));
        char id[128];
        std::memset(id, 0, sizeof id);
        std::memcpy(id, &uid, sizeof(uid));
        mc->run([&](Engine& e, int rank) { e.comm_init(id, rank, n); });
      } else {                                        // a device listed twice: bring-up/test transport (see comm_init_local)
        static std::atomic<int> next_key{1 << 20};
        const int key = next_key++;
        mc->run([&](Engine& e, int rank) { e.comm_init_local(key, rank, n); });
      }
    }
    aoadmm_ctx* c = new aoadmm_ctx;
    c->eng = mc->eng[0].get();
    c->multi = mc.release();
    *ctx = c;
  });
}

int aoadmm_destroy(aoadmm_ctx* ctx) {
  return guarded([&] {
    if (!ctx) return;
    if (ctx->multi) delete ctx->multi;                // joins the workers, destroys every engine
    else delete ctx->eng;
    delete ctx;
  });
}

int aoadmm_synchronize(aoadmm_ctx* ctx) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    on_engines(ctx, [&](Engine& e, int) {
      AO_HIP(hipSetDevice(e.device()));
      AO_HIP(hipStreamSynchronize(e.stream()));
    });
  });
}

int aoadmm_set_progress(aoadmm_ctx* ctx, aoadmm_progress_fn fn, void* user, int every) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {                               // rank 0 reports; the caller's thread delivers (MultiCtx::run)
    if (ctx->multi) {
      MultiCtx* mc = ctx->multi;
      { std::lock_guard<std::mutex> lk(mc->m); mc->user_fn = fn; mc->user_arg = user; }
      const bool on = fn != nullptr && every > 0;
      on_engines(ctx, [&](Engine& e, int r) {
        const bool mine = on && r == 0;
        e.set_progress(mine ? &MultiCtx::queue_row : nullptr, mine ? static_cast<void*>(mc) : nullptr, mine ? every : 0);
      });
    } else {
      ctx->eng->set_progress(fn, user, every);
    }
  });
}

int aoadmm_comm_unique_id(char id[128]) {
  return guarded([&] {
    AO_REQUIRE(id != nullptr, "null pointer");
    ncclUniqueId uid;
    ncclResult_t r = ncclGetUniqueId(&uid);
    if (r != ncclSuccess) throw Error(AOADMM_ERR_RCCL, fmt("ncclGetUniqueId failed: %s", ncclGetErrorString(r)));
    std::memset(id, 0, 128);
    std::memcpy(id, &uid, sizeof(uid));
  });
}
int aoadmm_comm_init_rank(aoadmm_ctx* ctx, const char id[128], int rank, int world) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(!ctx->multi, "a multi-device context owns its communicator");
    ctx->eng->comm_init(id, rank, world);
  });
}
int aoadmm_comm_init_rank_share(aoadmm_ctx* ctx, const char id[128], int rank, int world) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(!ctx->multi, "a multi-device context owns its communicator");
    AO_REQUIRE(id != nullptr, "aoadmm_comm_init_rank_share needs the id from aoadmm_comm_unique_id");
    ctx->eng->comm_init(id, rank, world, true);
  });
}
int aoadmm_comm_init_local(aoadmm_ctx* ctx, int key, int rank, int world) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(!ctx->multi, "a multi-device context owns its communicator");
    ctx->eng->comm_init_local(key, rank, world);
  });
}
int aoadmm_comm_rank(aoadmm_ctx* ctx, int* rank, int* world) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    if (rank) *rank = ctx->eng->rank();
    if (world) *world = ctx->eng->world();
  });
}
int aoadmm_comm_info(aoadmm_ctx* ctx, int* nccl_version, int* comm_ranks, char* lib_path, int lib_path_cap) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { ctx->eng->comm_info(nccl_version, comm_ranks, lib_path, lib_path_cap); });
}

int aoadmm_model_begin(aoadmm_ctx* ctx, int n_modes, int n_tensors, int n_couplings) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.model_begin(n_modes, n_tensors, n_couplings); }); });
}
int aoadmm_model_set_mode(aoadmm_ctx* ctx, int mode, int64_t rows, int rank) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.set_mode(mode, rows, rank); }); });
}
int aoadmm_model_set_mode_slabs(aoadmm_ctx* ctx, int mode, int K, const int64_t* rows_k, int rank) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(rows_k != nullptr, "null pointer");
    on_engines(ctx, [&](Engine& e, int) { e.set_mode_slabs(mode, K, rows_k, rank); });
  });
}
int aoadmm_model_add_cp(aoadmm_ctx* ctx, int p, int n, const int* modes, double weight) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(modes != nullptr, "null pointer");
    on_engines(ctx, [&](Engine& e, int) { e.add_cp(p, n, modes, weight); });
  });
}
int aoadmm_model_add_par2(aoadmm_ctx* ctx, int p, const int* modes3, double weight) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(modes3 != nullptr, "null pointer");
    on_engines(ctx, [&](Engine& e, int) { e.add_par2(p, modes3, weight); });
  });
}
int aoadmm_model_set_constraint(aoadmm_ctx* ctx, int mode, int constraint, const double* params, int n_params,
                                const double* Lmat) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(n_params == 0 || params != nullptr, "null parameters");
    on_engines(ctx, [&](Engine& e, int) { e.set_constraint(mode, constraint, params, n_params, Lmat); });
  });
}
int aoadmm_model_set_coupling(aoadmm_ctx* ctx, int mode, int coupling, const double* H, int64_t hr, int64_t hc,
                              const double* H2, int64_t h2r, int64_t h2c) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.set_coupling(mode, coupling, H, hr, hc, H2, h2r, h2c); }); });
}
int aoadmm_model_set_coupling_type(aoadmm_ctx* ctx, int coupling, int type) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.set_coupling_type(coupling, type); }); });
}
int aoadmm_model_set_ridge(aoadmm_ctx* ctx, const double* ridge) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.set_ridge(ridge); }); });
}
int aoadmm_model_end(aoadmm_ctx* ctx) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.model_end(); }); });
}

int aoadmm_tensor_upload(aoadmm_ctx* ctx, int p, const double* data, int precision) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(data != nullptr, "null data");
    on_engines(ctx, [&](Engine& e, int) { e.tensor_upload(p, data, precision, 0, -1); });
  });
}
int aoadmm_tensor_upload_rows(aoadmm_ctx* ctx, int p, const double* block, int64_t row_offset, int64_t local_rows,
                              int precision) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(block != nullptr && local_rows > 0, "null/empty block");
    // one block cannot be every rank's block: a multi-device context shards the FULL array itself
    AO_REQUIRE(!ctx->multi, "aoadmm_tensor_upload_rows is for one-process-per-GPU contexts; give a multi-device context "
                            "the full array through aoadmm_tensor_upload");
    ctx->eng->tensor_upload(p, block, precision, row_offset, local_rows);
  });
}
int aoadmm_par2_slab_upload(aoadmm_ctx* ctx, int p, int k, const double* Xk) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.par2_slab_upload(p, k, Xk); }); });
}
int aoadmm_tensor_synth(aoadmm_ctx* ctx, int p, int rank, uint64_t seed, double noise, int precision) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.tensor_synth(p, rank, seed, noise, precision); }); });
}
int aoadmm_tensor_mask_upload(aoadmm_ctx* ctx, int p, const uint8_t* mask) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.tensor_mask_upload(p, mask); }); });
}
int aoadmm_tensor_weights_upload(aoadmm_ctx* ctx, int p, const double* W) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    if (ctx->multi && ctx->multi->eng.size() > 1)
      throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_tensor_weights_upload is not available on a multi-device context (aoadmm_create_multi with more than one device): use one context per rank and a communicator");
    on_engines(ctx, [&](Engine& e, int) { e.tensor_weights_upload(p, W); });
  });
}
int aoadmm_par2_slab_mask_upload(aoadmm_ctx* ctx, int p, int k, const uint8_t* mask_k) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.par2_slab_mask_upload(p, k, mask_k); }); });
}
int aoadmm_tensor_upload_coo(aoadmm_ctx* ctx, int p, int64_t nnz, const int64_t* subs, const double* vals) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(nnz >= 0, "nnz = %lld < 0", (long long)nnz);
    AO_REQUIRE(nnz == 0 || (subs != nullptr && vals != nullptr), "null subs / vals");
    on_engines(ctx, [&](Engine& e, int) { e.tensor_upload_coo(p, nnz, subs, vals); });   // replicated on every engine
  });
}
int aoadmm_tensor_upload_coo_sharded(aoadmm_ctx* ctx, int p, int64_t nnz, const int64_t* subs, const double* vals) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(nnz >= 0, "nnz = %lld < 0", (long long)nnz);
    AO_REQUIRE(nnz == 0 || (subs != nullptr && vals != nullptr), "null subs / vals");
    on_engines(ctx, [&](Engine& e, int) { e.tensor_upload_coo(p, nnz, subs, vals, true); });   // every engine keeps its share
  });
}
int aoadmm_par2_slab_upload_coo(aoadmm_ctx* ctx, int p, int64_t nnz, const int64_t* subs, const double* vals) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(nnz >= 0, "nnz = %lld < 0", (long long)nnz);
    AO_REQUIRE(nnz == 0 || (subs != nullptr && vals != nullptr), "null subs / vals");
    on_engines(ctx, [&](Engine& e, int) { e.par2_slab_upload_coo(p, nnz, subs, vals); });   // replicated on every engine
  });
}
int aoadmm_tensor_set_observed_only(aoadmm_ctx* ctx, int p, int on) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.set_observed_only(p, on != 0); }); });
}
int aoadmm_tensor_set_entry_weights(aoadmm_ctx* ctx, int p, int64_t nnz, const int64_t* subs, const double* wts,
                                    double unstored_weight) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    if (ctx->multi && ctx->multi->eng.size() > 1)
      throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_tensor_set_entry_weights is not available on a multi-device context (aoadmm_create_multi with more than one device): use one context per rank and a communicator");
    on_engines(ctx, [&](Engine& e, int) { e.set_entry_weights(p, nnz, subs, wts, unstored_weight); });
  });
}
int aoadmm_resident_em_step(aoadmm_ctx* ctx, int p, double stats[3]) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(stats != nullptr, "null stats");
    on_engines(ctx, [&](Engine& e, int r) {          // replicated: every engine takes the same step, rank 0 answers
      double mine[3];
      e.resident_em_step(p, r == 0 ? stats : mine);
    });
  });
}
// One EM pass of a masked or weighted dense block as Engine::outer_updates runs it (Engine::resident_em_pass)
int aoadmm_resident_em_pass(aoadmm_ctx* ctx, int p, int update, int fuse, double stats[4], double* data, double* data_t,
                            double* mttkrp, int64_t info[8]) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    if (ctx->multi) throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_resident_em_pass runs on a single-device context");
    ctx->eng->resident_em_pass(p, update, fuse, stats, data, data_t, mttkrp, info);
  });
}
// The missing entries of a masked dense block as a list (Engine::set_missing_list)
int aoadmm_tensor_set_missing_list(aoadmm_ctx* ctx, int p, int on) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    if (ctx->multi) throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_tensor_set_missing_list is not available on a multi-device context (aoadmm_create_multi)");
    ctx->eng->set_missing_list(p, on != 0);
  });
}
int aoadmm_tensor_missing_list(aoadmm_ctx* ctx, int p, int64_t* n, int64_t* subs_or_null) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { ctx->eng->missing_list(p, n, subs_or_null); });
}
int aoadmm_resident_em_list_pass(aoadmm_ctx* ctx, int p, int update, double stats2[2], double* data, double* data_t) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    if (ctx->multi) throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_resident_em_list_pass runs on a single-device context");
    ctx->eng->resident_em_list_pass(p, update, stats2, data, data_t);
  });
}
// Held-out scoring answers on one engine (which may belong to a communicator); a multi-device context would have to
// keep one list per engine for no gain: it is refused
static void require_single_engine(aoadmm_ctx* ctx, const char* what) {
  if (ctx->multi && ctx->multi->eng.size() > 1)
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s is not available on a multi-device context (aoadmm_create_multi with more than one device): use one context per rank and a communicator", what));
}
int aoadmm_resident_model_at(aoadmm_ctx* ctx, int p, int64_t n, const int64_t* subs, double* out) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_model_at");
    ctx->eng->model_at(p, n, subs, out);
  });
}
int aoadmm_tensor_set_heldout(aoadmm_ctx* ctx, int p, int64_t n, const int64_t* subs, const double* vals) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_tensor_set_heldout");
    ctx->eng->set_heldout(p, n, subs, vals);
  });
}
int aoadmm_resident_heldout_stats(aoadmm_ctx* ctx, int p, double stats[4]) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_heldout_stats");
    ctx->eng->heldout_stats(p, stats);
  });
}
int aoadmm_heldout_info(aoadmm_ctx* ctx, int p, int64_t* n, int64_t* resident_bytes, int* row_major) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { ctx->eng->heldout_info(p, n, resident_bytes, row_major); });   // no device work
}
int aoadmm_heldout_trace(aoadmm_ctx* ctx, int p, double* out, int cap, int* len, int* best_iter) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { ctx->eng->heldout_trace(p, out, cap, len, best_iter); });      // no device work
}
int aoadmm_heldout_keep_best(aoadmm_ctx* ctx, int on) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_heldout_keep_best");
    ctx->eng->heldout_keep_best(on);
  });
}
int aoadmm_heldout_restore_best(aoadmm_ctx* ctx, int* iter) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_heldout_restore_best");
    ctx->eng->heldout_restore_best(iter);
  });
}
int aoadmm_heldout_best_info(aoadmm_ctx* ctx, int* have, int* iter, int64_t* bytes, int64_t* launches) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { ctx->eng->heldout_best_info(have, iter, bytes, launches); });   // no device work
}
int aoadmm_resident_topk(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const int64_t* subs, int k, const int64_t* excl_off,
                         const int64_t* excl_idx, int64_t* idx, double* val) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_topk");
    ctx->eng->topk(p, mode, nq, subs, k, excl_off, excl_idx, idx, val);
  });
}
int aoadmm_resident_topk_w(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const double* W, int k, const int64_t* excl_off,
                           const int64_t* excl_idx, int64_t* idx, double* val) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_topk_w");
    ctx->eng->topk_w(p, mode, nq, W, k, excl_off, excl_idx, idx, val);
  });
}
int aoadmm_resident_rank_of(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off,
                            const int64_t* excl_idx, int64_t* rank, double* score, int64_t* ncand_or_null) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_rank_of");
    ctx->eng->rank_of(p, mode, nq, subs, excl_off, excl_idx, rank, score, ncand_or_null);
  });
}
int aoadmm_resident_rank_of_w(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const double* W, const int64_t* targets,
                              const int64_t* excl_off, const int64_t* excl_idx, int64_t* rank, double* score, int64_t* ncand_or_null) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_rank_of_w");
    ctx->eng->rank_of_w(p, mode, nq, W, targets, excl_off, excl_idx, rank, score, ncand_or_null);
  });
}
int aoadmm_resident_project(aoadmm_ctx* ctx, int p, const double* const* M, const int64_t* ld, const int* r, double* core) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_project");
    ctx->eng->project(p, M, ld, r, core);
  });
}
int aoadmm_resident_core_consistency(aoadmm_ctx* ctx, int p, double* cc, double* core_or_null, int* rank_deficient_or_null) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_core_consistency");
    ctx->eng->core_consistency(p, cc, core_or_null, rank_deficient_or_null);
  });
}
int aoadmm_tensor_set_ranklist(aoadmm_ctx* ctx, int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off,
                               const int64_t* excl_idx) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_tensor_set_ranklist");
    ctx->eng->set_ranklist(p, mode, nq, subs, excl_off, excl_idx);
  });
}
int aoadmm_ranklist_info(aoadmm_ctx* ctx, int p, int64_t* nq, int* mode, int64_t* listed_after_dedup, int64_t* resident_bytes) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { ctx->eng->ranklist_info(p, nq, mode, listed_after_dedup, resident_bytes); });   // no device work
}
int aoadmm_rank_track(aoadmm_ctx* ctx, int metric, int k, int every, int patience, int criterion) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_rank_track");
    ctx->eng->rank_track(metric, k, every, patience, criterion);
  });
}
int aoadmm_rank_trace(aoadmm_ctx* ctx, int p, int what, double* out, int cap, int* len, int* iters_or_null, int* best_iter) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { ctx->eng->rank_trace(p, what, out, cap, len, iters_or_null, best_iter); });     // no device work
}
int aoadmm_ranklist_last(aoadmm_ctx* ctx, int p, int64_t* rank, double* score, int64_t* ncand) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_ranklist_last");
    ctx->eng->ranklist_last(p, rank, score, ncand);
  });
}
int aoadmm_resident_fold_in(aoadmm_ctx* ctx, int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals,
                            const aoadmm_foldin_options* opt_or_null, double* rows, int* info, int* iters_or_null,
                            double* gram_or_null, double* rhs_or_null) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_fold_in");
    ctx->eng->fold_in(p, mode, nq, nobs, subs, vals, opt_or_null, rows, info, iters_or_null, gram_or_null, rhs_or_null);
  });
}
int aoadmm_resident_fold_in_w(aoadmm_ctx* ctx, int p, int mode, int64_t nq, int64_t nobs, const int64_t* subs, const double* vals,
                              const double* wts_or_null, double unstored_weight, const aoadmm_foldin_options* opt_or_null,
                              double* rows, int* info, int* iters_or_null, double* gram_or_null, double* rhs_or_null) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_fold_in_w");
    ctx->eng->fold_in_w(p, mode, nq, nobs, subs, vals, wts_or_null, unstored_weight, opt_or_null, rows, info, iters_or_null, gram_or_null,
                        rhs_or_null);
  });
}
int aoadmm_par2_rows(aoadmm_ctx* ctx, int p, int64_t* rows) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {                                 // no device work; the model is the same on every engine
    AO_REQUIRE(rows != nullptr, "null pointer");
    *rows = ctx->eng->par2_rows(p);
  });
}
int aoadmm_resident_par2_fold_in(aoadmm_ctx* ctx, int p, int64_t nk, const int64_t* cols, const double* X, const double* c0_or_null,
                                 const aoadmm_par2_foldin_options* opt_or_null, double* C, double* B_or_null, double* P_or_null,
                                 double* res, double* xnorm_or_null, int* iters, int* info, double* Y_or_null, double* sys_or_null,
                                 int* path_or_null) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    require_single_engine(ctx, "aoadmm_resident_par2_fold_in");
    ctx->eng->par2_fold_in(p, nk, cols, X, c0_or_null, opt_or_null, C, B_or_null, P_or_null, res, xnorm_or_null, iters, info, Y_or_null,
                           sys_or_null, path_or_null);
  });
}
int aoadmm_tensor_storage_info(aoadmm_ctx* ctx, int p, int* precision, double* scale, int64_t* resident_bytes) {
  CTX_OR_FAIL(ctx);
  // no collective and no device work: rank 0's engine answers for a multi-device context (every rank holds the same
  // form; of a sharded sparse block rank 0's share)
  return guarded([&] { ctx->eng->tensor_storage_info(p, precision, scale, resident_bytes); });
}
int aoadmm_tensor_rank(aoadmm_ctx* ctx, int p, int* rank) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {                                 // no device work; the model is the same on every engine
    AO_REQUIRE(rank != nullptr, "null pointer");
    *rank = ctx->eng->tensor_rank(p);
  });
}
int aoadmm_tensor_normsq(aoadmm_ctx* ctx, int p, double* out) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(out != nullptr, "null pointer");
    on_engines(ctx, [&](Engine& e, int r) {
      const double v = e.tensor_normsq(p);           // collective: every rank computes, rank 0 answers
      if (r == 0) *out = v;
    });
  });
}

int aoadmm_state_set(aoadmm_ctx* ctx, int field, int index, int slab, const double* host, int64_t rows,
                     int64_t cols) {
  CTX_OR_FAIL(ctx);
  return guarded([&] { on_engines(ctx, [&](Engine& e, int) { e.state_set(field, index, slab, host, rows, cols); }); });
}
int aoadmm_state_get(aoadmm_ctx* ctx, int field, int index, int slab, double* host, int64_t rows, int64_t cols) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    ctx->eng->state_get(field, index, slab, host, rows, cols);   // multi-device: the state is replicated, rank 0 answers
  });
}

int aoadmm_solve(aoadmm_ctx* ctx, const aoadmm_options* opt, aoadmm_result* out) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(opt != nullptr && out != nullptr, "null options/result");
    on_engines(ctx, [&](Engine& e, int r) {
      if (r == 0) { e.solve(*opt, out); return; }
      aoadmm_result mine;                             // the other ranks keep their (identical) results to themselves
      std::memset(&mine, 0, sizeof mine);
      e.solve(*opt, &mine);
    });
  });
}
int aoadmm_resident_mttkrp(aoadmm_ctx* ctx, int p, int tensor_mode, double* out_host_or_null, float* elapsed_ms) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    on_engines(ctx, [&](Engine& e, int r) { e.resident_mttkrp(p, tensor_mode, r == 0 ? out_host_or_null : nullptr, r == 0 ? elapsed_ms : nullptr); });
  });
}
int aoadmm_resident_par2_rhs(aoadmm_ctx* ctx, int p, int tensor_mode, double* out_host_or_null, float* elapsed_ms) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    on_engines(ctx, [&](Engine& e, int r) { e.resident_par2_rhs(p, tensor_mode, r == 0 ? out_host_or_null : nullptr, r == 0 ? elapsed_ms : nullptr); });
  });
}
int aoadmm_kernel_stats(aoadmm_ctx* ctx, int which, int reset, double* contract_ms, int64_t* contract_launches,
                        double* contract_bytes, double* contract_flops) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    on_engines(ctx, [&](Engine& e, int r) {
      if (r == 0) e.kernel_stats(which, reset, contract_ms, contract_launches, contract_bytes, contract_flops);
      else e.kernel_stats(which, reset, nullptr, nullptr, nullptr, nullptr);
    });
  });
}

// ---------------------------------------------------------------------------
// op level
// ---------------------------------------------------------------------------
static void h2d(DevBuf& b, const double* h, int64_t n, hipStream_t s) {
  b.alloc((size_t)n * sizeof(double));
  AO_HIP(hipMemcpyAsync(b.p, h, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
}
static void d2h(double* h, const DevBuf& b, int64_t n, hipStream_t s) {
  AO_HIP(hipMemcpyAsync(h, b.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));
}
// a zeroed loop-control record on the device; and what the kernels left in it, once the stream has drained
static AdmmCtl* ctl_new(DevBuf& b, hipStream_t s) {
  b.alloc(sizeof(AdmmCtl));
  AO_HIP(hipMemsetAsync(b.p, 0, sizeof(AdmmCtl), s));
  return b.as<AdmmCtl>();
}
static AdmmCtl ctl_fetch(const DevBuf& b, hipStream_t s) {
  AdmmCtl h;
  AO_HIP(hipMemcpyAsync(&h, b.p, sizeof h, hipMemcpyDeviceToHost, s));
  AO_HIP(hipStreamSynchronize(s));
  if (h.notpd) throw Error(AOADMM_ERR_NOT_PD, "Matrix must be positive definite.");
  return h;
}

int aoadmm_op_mttkrp(aoadmm_ctx* ctx, const double* X, int ndims, const int64_t* dims, const double* const* U, int R,
                     int n, int precision, double* out) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(X && dims && U && out, "null pointer");
    AO_REQUIRE(ndims >= 2 && ndims <= 8 && n >= 0 && n < ndims, "bad order/mode");
    if (precision == AOADMM_PREC_F16)
      throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_op_mttkrp runs on a natural-layout array: AOADMM_PREC_F16 exists for resident blocks only (aoadmm_tensor_upload)");
    Engine& e = *ctx->eng;
    AO_HIP(hipSetDevice(e.device()));
    CpBlock blk;
    block_upload(e.block_ctx(), blk, ndims, dims, X, precision, 0, dims[0]);
    std::vector<DevBuf> fac(ndims);
    FactorRef refs[8];
    for (int m = 0; m < ndims; ++m) {
      AO_REQUIRE(U[m] != nullptr, "null factor");
      h2d(fac[m], U[m], dims[m] * R, e.stream());
      refs[m] = FactorRef{fac[m].d(), dims[m], 1};
    }
    DevBuf o;
    o.alloc((size_t)dims[n] * R * sizeof(double));
    // host in / host out on ONE engine with the whole tensor: no collective, whatever communicator the engine is in
    block_mttkrp(e.block_ctx(), blk, n, refs, R, 1.0, o.d(), dims[n], false, nullptr, 0, false, true);
    d2h(out, o, dims[n] * R, e.stream());
  });
}

int aoadmm_op_unfold_gram(aoadmm_ctx* ctx, const double* X, int ndims, const int64_t* dims, int n, int precision,
                          double* out) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(X && dims && out, "null pointer");
    AO_REQUIRE((ndims == 2 || ndims == 3) && n >= 0 && n < ndims, "unfold_gram handles matrices and 3-way tensors");
    if (precision == AOADMM_PREC_F16)
      throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_op_unfold_gram runs on a natural-layout array: AOADMM_PREC_F16 exists for resident blocks only (aoadmm_tensor_upload)");
    Engine& e = *ctx->eng;
    AO_HIP(hipSetDevice(e.device()));
    CpBlock blk;
    block_upload(e.block_ctx(), blk, ndims, dims, X, precision, 0, dims[0]);
    const int64_t I = dims[0], Ip = blk.X.pad0, J = dims[1], K = ndims == 3 ? dims[2] : 1;
    UnfoldGramArgs a;
    a.X = blk.X.data.p;
    if (n == 0) { a.n = I; a.sa = 1; a.n1 = J * K; a.s1 = Ip; a.n2 = 1; a.s2 = 0; }
    else if (n == 1) { a.n = J; a.sa = Ip; a.n1 = I; a.s1 = 1; a.n2 = K; a.s2 = Ip * J; }
    else { a.n = K; a.sa = Ip * J; a.n1 = Ip * J; a.s1 = 1; a.n2 = 1; a.s2 = 0; }   // padding rows are zeros
    DevBuf ws, y;
    ws.alloc(unfold_gram_ws_bytes(a));
    y.alloc((size_t)a.n * a.n * sizeof(double));
    unfold_gram(a, precision, ws.d(), y.d(), e.stream());
    d2h(out, y, a.n * a.n, e.stream());
  });
}

int aoadmm_resident_unfold_gram(aoadmm_ctx* ctx, int p, int tensor_mode, int slab, double* out) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(out != nullptr, "null pointer");
    // every engine of a multi-device context enters (the Gram matrix of a sharded block is all-reduced); rank 0 reports
    on_engines(ctx, [&](Engine& e, int r) { e.resident_unfold_gram(p, tensor_mode, slab, r == 0 ? out : nullptr); });
  });
}

int aoadmm_resident_nvecs(aoadmm_ctx* ctx, int p, int tensor_mode, int r, const aoadmm_nvecs_options* opt, double* U,
                          int64_t ldU, double* eigvals, aoadmm_nvecs_info* info) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(U != nullptr, "null pointer");
    // the block is replicated: every engine of a multi-device context computes the same bits, rank 0 reports
    on_engines(ctx, [&](Engine& e, int rk) {
      e.resident_nvecs(p, tensor_mode, r, opt, rk == 0 ? U : nullptr, ldU, rk == 0 ? eigvals : nullptr, rk == 0 ? info : nullptr);
    });
  });
}

int aoadmm_op_gram(aoadmm_ctx* ctx, const double* F, int64_t rows, int R, double* out) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(F && out && rows > 0 && R > 0 && R <= kMaxRank, "bad arguments");
    Engine& e = *ctx->eng;
    AO_HIP(hipSetDevice(e.device()));
    DevBuf f, g, ws;
    h2d(f, F, rows * R, e.stream());
    g.alloc((size_t)R * R * 8);
    ws.alloc(atb_ws_bytes(rows, R, R));
    atb_small(g.d(), f.d(), rows, f.d(), rows, rows, R, R, ws.d(), nullptr, e.stream());
    d2h(out, g, (int64_t)R * R, e.stream());
  });
}

// The metric reduction of a ranking list (rank_metrics.h) on host arrays
int aoadmm_op_rank_metrics(aoadmm_ctx* ctx, int64_t n, const int64_t* rank, const int64_t* ncand, int64_t k, double out[8]) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(rank && ncand && out && n >= 1 && k >= 1, "bad arguments");
    Engine& e = *ctx->eng;
    AO_HIP(hipSetDevice(e.device()));
    DevBuf r, c, part, slots;
    r.alloc((size_t)n * sizeof(int64_t));
    c.alloc((size_t)n * sizeof(int64_t));
    part.alloc(rank_metrics_part_bytes(n));
    slots.alloc(kRankSlots * sizeof(double));
    AO_HIP(hipMemcpyAsync(r.p, rank, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, e.stream()));
    AO_HIP(hipMemcpyAsync(c.p, ncand, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, e.stream()));
    rank_metrics_enqueue(r.as<int64_t>(), c.as<int64_t>(), n, k, part.d(), slots.d(), e.stream());
    d2h(out, slots, kRankSlots, e.stream());
  });
}

int aoadmm_op_chol(aoadmm_ctx* ctx, const double* B, int R, double* L) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(B && L && R > 0 && R <= kMaxRank, "bad arguments");
    Engine& e = *ctx->eng;
    AO_HIP(hipSetDevice(e.device()));
    DevBuf b, l, c;
    h2d(b, B, (int64_t)R * R, e.stream());
    l.alloc((size_t)R * R * 8);
    ctl_new(c, e.stream());
    AO_HIP(hipMemsetAsync(l.p, 0, (size_t)R * R * 8, e.stream()));
    chol_only(l.d(), b.d(), R, c.as<AdmmCtl>(), e.stream());
    (void)ctl_fetch(c, e.stream());
    d2h(L, l, (int64_t)R * R, e.stream());
  });
}

static ProxSpec make_spec(int constraint, const double* params, int np) {
  ProxSpec ps;
  ps.type = constraint;
  if (np > 0) ps.p0 = params[0];
  if (np > 1) ps.p1 = params[1];
  return ps;
}

int aoadmm_op_prox(aoadmm_ctx* ctx, int constraint, const double* params, int n_params, const double* Lmat,
                   const double* X, int64_t rows, int R, double rho, double* out) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(X && out && rows > 0 && R > 0 && R <= kMaxRank, "bad arguments");
    Engine& e = *ctx->eng;
    AO_HIP(hipSetDevice(e.device()));
    DevBuf x, z, r, ws;
    h2d(x, X, rows * R, e.stream());
    z.alloc((size_t)rows * R * 8);
    h2d(r, &rho, 1, e.stream());
    ws.alloc(prox_ws_bytes(constraint, rows, R));
    ProxSpec ps = make_spec(constraint, params, n_params);
    QuadPrep qp;
    if (constraint == AOADMM_C_QUADRATIC) { qp.build(Lmat, rows, e.stream()); qp.attach(ps); }
    prox_apply(ps, x.d(), rows, z.d(), rows, rows, R, r.d(), 1.0, ws.d(), nullptr, e.stream());
    d2h(out, z, rows * R, e.stream());
  });
}

int aoadmm_op_admm_constrained(aoadmm_ctx* ctx, const double* A, const double* Bsys, double rho, int constraint,
                               const double* params, int n_params, const double* Lmat, int64_t rows, int R,
                               int max_inner, double tol_pr, double tol_du, double* fac, double* Z, double* mu,
                               int* inner_iters) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(A && Bsys && fac && Z && mu && rows > 0 && R > 0 && R <= kMaxRank && max_inner >= 1, "bad arguments");
    Engine& e = *ctx->eng;
    hipStream_t s = e.stream();
    AO_HIP(hipSetDevice(e.device()));
    DevBuf a, b, l, rh, f, z, m, part, V, Zn, ws, ctl, Cd;
    h2d(a, A, rows * R, s); h2d(b, Bsys, (int64_t)R * R, s);
    h2d(f, fac, rows * R, s); h2d(z, Z, rows * R, s); h2d(m, mu, rows * R, s);
    l.alloc((size_t)R * R * 8); rh.alloc(64); Cd.alloc((size_t)R * R * 8);
    part.alloc((size_t)admm_partials(rows) * 4 * 8 + 2048);
    V.alloc((size_t)rows * R * 8); Zn.alloc((size_t)rows * R * 8);
    ws.alloc(prox_ws_bytes(constraint, rows, R));
    ctl_new(ctl, s);
    // B + rho/2*I and its Cholesky (cmtf_fun_AOADMM.m:141-142): feed sys_build with C = Bsys, w = 1
    // but keep the caller's rho: do it by hand
    std::vector<double> Bh(Bsys, Bsys + (size_t)R * R);
    for (int i = 0; i < R; ++i) Bh[i + (size_t)R * i] += rho / 2;
    DevBuf bb;
    h2d(bb, Bh.data(), (int64_t)R * R, s);
    h2d(rh, &rho, 1, s);
    AO_HIP(hipStreamSynchronize(s));
    chol_only(l.d(), bb.d(), R, ctl.as<AdmmCtl>(), s);
    ctl_reset(ctl.as<AdmmCtl>(), s);
    AdmmMode am;
    am.A = a.d(); am.L = l.d(); am.rho = rh.d(); am.fac = f.d(); am.Z = z.d(); am.mu = m.d();
    am.rows = rows; am.R = R; am.prox = make_spec(constraint, params, n_params);
    QuadPrep qp;
    if (constraint == AOADMM_C_QUADRATIC) { qp.build(Lmat, rows, s); qp.attach(am.prox); }
    admm_constrained_loop(am, part.d(), V.d(), Zn.d(), ws.d(), ctl.as<AdmmCtl>(), max_inner, tol_pr, tol_du, s);
    const AdmmCtl h = ctl_fetch(ctl, s);
    if (inner_iters) *inner_iters = h.iters;
    d2h(fac, f, rows * R, s); d2h(Z, z, rows * R, s); d2h(mu, m, rows * R, s);
  });
}

// One mode's ADMM update as Engine::update_uncoupled_cp_mode runs it for a constrained mode: the system from sys_build
// (rho, L, inv(L*L')), then the solver's own step (admm_mode_update): the loop on the path admm_path() names, the Gram
// matrix and the row-major copy.
int aoadmm_op_admm_mode(aoadmm_ctx* ctx, const double* A, const double* Cmat, int constraint, const double* params,
                        int n_params, const double* Lmat, int64_t rows, int R, int max_inner, double tol_pr,
                        double tol_du, double* fac, double* Z, double* mu, int* inner_iters, double* res,
                        double* gram, double* fac_rowmajor, int* path) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(A && Cmat && fac && Z && mu && rows > 0 && R > 0 && R <= kMaxRank && max_inner >= 1, "bad arguments");
    AO_REQUIRE(constraint != AOADMM_C_QUADRATIC || Lmat != nullptr, "quadratic regularization needs its matrix");
    Engine& e = *ctx->eng;
    hipStream_t s = e.stream();
    AO_HIP(hipSetDevice(e.device()));
    const int64_t nR = rows * R, RR = (int64_t)R * R;
    DevBuf a, cpre, cd, bs, l, bi, rh, f, z, m, part, V, Zn, ws, ctl, g, ft, aws;
    h2d(a, A, nR, s); h2d(cpre, Cmat, RR, s);
    h2d(f, fac, nR, s); h2d(z, Z, nR, s); h2d(m, mu, nR, s);
    cd.alloc((size_t)RR * 8); bs.alloc((size_t)RR * 8); l.alloc((size_t)RR * 8); bi.alloc((size_t)RR * 8); rh.alloc(64);
    part.alloc((size_t)admm_partials(rows) * 4 * 8);
    V.alloc((size_t)nR * 8); Zn.alloc((size_t)nR * 8);
    ws.alloc(prox_ws_bytes(constraint, rows, R));
    g.alloc((size_t)RR * 8); ft.alloc((size_t)nR * 8);
    aws.alloc(admm_mode_ws_bytes(rows, R));
    AdmmCtl* c = ctl_new(ctl, s);
    SysBuild sb;                                     // prepare_mode_system with the Hadamard product given
    sb.ngram = 0; sb.Cpre = cpre.d(); sb.w = 1.0; sb.ridge = 0.0; sb.bsum_half = 0.0; sb.rho_scale = 1.0;
    sb.nrho = 1; sb.R = R;
    sb.C = cd.d(); sb.rho = rh.d(); sb.Bsys = bs.d(); sb.L = l.d(); sb.Binv = bi.d(); sb.ctl = c;
    sys_build(sb, s);
    ProxSpec ps = make_spec(constraint, params, n_params);
    QuadPrep qp;
    if (constraint == AOADMM_C_QUADRATIC) { qp.build(Lmat, rows, s); qp.attach(ps); }
    AdmmMode am;
    am.A = a.d(); am.L = l.d(); am.Binv = bi.d(); am.rho = rh.d();
    am.fac = f.d(); am.Z = z.d(); am.mu = m.d();
    am.rows = rows; am.R = R; am.prox = ps;
    const AdmmPath ap = admm_mode_update(am, part.d(), V.d(), Zn.d(), ws.d(), g.d(), ft.d(), aws.d(), c, max_inner,
                                         tol_pr, tol_du, s);
    const AdmmCtl h = ctl_fetch(ctl, s);
    if (inner_iters) *inner_iters = h.iters;
    if (res) { res[0] = h.res[1]; res[1] = h.res[3]; }
    if (path) *path = (int)ap;
    d2h(fac, f, nR, s); d2h(Z, z, nR, s); d2h(mu, m, nR, s);
    if (gram) d2h(gram, g, RR, s);
    if (fac_rowmajor) d2h(fac_rowmajor, ft, nR, s);
  });
}

// Mode B of a PARAFAC2 block from the right-hand side on, as Engine::par2_update_B runs it: par2_b_loop (slab systems,
// ADMM_B_Parafac2 on the path par2_b_path() names, Gram matrices) on uploaded buffers, no model.
int aoadmm_op_par2_b_loop(aoadmm_ctx* ctx, int K, const int64_t* rows_k, int R, const double* Ak, const double* GA,
                          const double* Cmat, double weight, double rho_scale, int constraint, const double* params,
                          int n_params, int max_inner, const double* tol, double* P, double* mu_DeltaB, double* DeltaB,
                          double* Z, double* muZ, double* B, double* rho, double* L, double* GB, int* inner_iters,
                          double* res, int* path) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(K >= 1 && rows_k && R > 0 && R <= kMaxRank && max_inner >= 1 && tol, "bad arguments");
    AO_REQUIRE(Ak && GA && Cmat && P && mu_DeltaB && DeltaB && B, "bad arguments");
    AO_REQUIRE(constraint >= AOADMM_C_NONE && constraint <= AOADMM_C_TPARAFAC2 && constraint != AOADMM_C_QUADRATIC,
               "constraint id %d is not available here", constraint);
    const bool constr = constraint != AOADMM_C_NONE;
    AO_REQUIRE(!constr || (Z && muZ), "a constrained B_k loop needs Z and muZ");
    std::vector<int64_t> off((size_t)K + 1, 0);
    int64_t jmax = 0;
    for (int k = 0; k < K; ++k) {
      AO_REQUIRE(rows_k[k] >= 1 && rows_k[k] < ((int64_t)1 << 31) / R, "slab %d: bad row count", k);
      off[k + 1] = off[k] + rows_k[k];
      jmax = std::max(jmax, rows_k[k]);
    }
    if (constraint == AOADMM_C_TPARAFAC2) {
      AO_REQUIRE(K <= kTsmoothMaxK, "tPARAFAC2 on the device supports up to %d slabs", kTsmoothMaxK);
      for (int k = 1; k < K; ++k)
        AO_REQUIRE(rows_k[k] == rows_k[0], "tPARAFAC2 needs slabs of equal size (t_smoothness_prox.m adds B_k matrices)");
    }
    Engine& e = *ctx->eng;
    hipStream_t s = e.stream();
    AO_HIP(hipSetDevice(e.device()));
    const int64_t RR = (int64_t)R * R, n = off[K] * R;
    DevBuf offd, ak, ga, cf, rh, l, b, p, pold, mu, w, db, dbo, part, norms, jrot, z, mz, zold, v, ws, gb, ctl;
    offd.alloc((size_t)(K + 1) * sizeof(int64_t));
    AO_HIP(hipMemcpyAsync(offd.p, off.data(), (size_t)(K + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    h2d(ak, Ak, n, s); h2d(ga, GA, RR, s); h2d(cf, Cmat, (int64_t)K * R, s);
    h2d(p, P, n, s); h2d(mu, mu_DeltaB, n, s); h2d(db, DeltaB, RR, s);
    rh.alloc((size_t)K * 8); l.alloc((size_t)K * RR * 8); gb.alloc((size_t)K * RR * 8);
    b.alloc((size_t)n * 8); pold.alloc((size_t)n * 8); w.alloc((size_t)n * 8);
    dbo.alloc((size_t)RR * 8); part.alloc((size_t)K * RR * 8); norms.alloc((size_t)K * 8 * 8); jrot.alloc((size_t)K * RR * 8);
    AO_HIP(hipMemsetAsync(b.p, 0, (size_t)n * 8, s));
    AO_HIP(hipMemsetAsync(l.p, 0, (size_t)K * RR * 8, s));
    if (constr) {
      h2d(z, Z, n, s); h2d(mz, muZ, n, s);
      zold.alloc((size_t)n * 8); v.alloc((size_t)n * 8);
      ws.alloc(prox_ws_bytes(constraint, jmax, R));
    }
    ctl_new(ctl, s);
    P2Dims d;
    d.K = K; d.I = 0; d.R = R; d.off = offd.as<int64_t>(); d.off_h = off.data();
    d.Jtot = off[K]; d.Jmax = (int)jmax; d.k0 = 0; d.k1 = K;
    P2BLoop g;
    g.GA = ga.d(); g.Cfac = cf.d();
    g.w = weight; g.ridge = 0.0; g.bsum = false; g.bsum_half = 0.0; g.rho_scale = rho_scale;
    g.Ak = ak.d(); g.rho = rh.d(); g.L = l.d();
    g.a.B = b.d(); g.a.P = p.d(); g.a.Pold = pold.d(); g.a.mu = mu.d(); g.a.W = w.d();
    g.a.DeltaB = db.d(); g.a.DeltaBold = dbo.d(); g.a.part = part.d(); g.a.norms = norms.d(); g.a.Jrot = jrot.d();
    g.constrained = constr;
    g.prox = make_spec(constraint, params, n_params);
    g.Z = z.d(); g.muZ = mz.d(); g.Zold = zold.d(); g.V = v.d(); g.prox_ws = ws.d();
    g.max_inner = max_inner;
    g.tol_pr_coupl = tol[0]; g.tol_pr_constr = tol[1]; g.tol_du_coupl = tol[2]; g.tol_du_constr = tol[3];
    g.GB = gb.d();
    const P2BPath bp = par2_b_path(d, constr, false);
    par2_b_loop(g, d, ctl.as<AdmmCtl>(), s);
    const AdmmCtl h = ctl_fetch(ctl, s);
    if (inner_iters) *inner_iters = h.iters;
    if (res) for (int i = 0; i < 4; ++i) res[i] = h.res[i];
    if (path) { path[0] = bp.folded; path[1] = bp.slab; path[2] = bp.in_lds; path[3] = bp.dual_fold; }
    d2h(B, b, n, s); d2h(P, p, n, s); d2h(mu_DeltaB, mu, n, s); d2h(DeltaB, db, RR, s);
    if (constr) { d2h(Z, z, n, s); d2h(muZ, mz, n, s); }
    if (rho) d2h(rho, rh, K, s);
    if (L) d2h(L, l, (int64_t)K * RR, s);
    if (GB) d2h(GB, gb, (int64_t)K * RR, s);
  });
}

// Slab layout of the op-level PARAFAC2 entries below: K dense slabs of rows_k[k] columns (par2.h)
struct OpSlabs {
  std::vector<int64_t> off;
  DevBuf offd;
  P2Dims d;
};
static void op_slabs(OpSlabs& o, aoadmm_ctx* ctx, const char* who, int K, const int64_t* rows_k, int I, int R, hipStream_t s) {
  if (ctx->multi || ctx->eng->sharded())
    throw Error(AOADMM_ERR_UNSUPPORTED, fmt("%s runs on one engine without a communicator", who));
  AO_REQUIRE(K >= 1 && rows_k && R > 0 && R <= kMaxRank && I >= 1, "bad arguments");
  AO_REQUIRE((int64_t)I * R + (int64_t)R * R < ((int64_t)1 << 31) / K, "block too large");
  o.off.assign((size_t)K + 1, 0);
  int64_t jmax = 0;
  for (int k = 0; k < K; ++k) {
    AO_REQUIRE(rows_k[k] >= 1 && rows_k[k] < ((int64_t)1 << 31) / std::max(R, I), "slab %d: bad column count", k);
    o.off[k + 1] = o.off[k] + rows_k[k];
    jmax = std::max(jmax, rows_k[k]);
  }
  o.offd.alloc((size_t)(K + 1) * sizeof(int64_t));
  AO_HIP(hipMemcpyAsync(o.offd.p, o.off.data(), (size_t)(K + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  o.d.K = K; o.d.I = I; o.d.R = R; o.d.off = o.offd.as<int64_t>(); o.d.off_h = o.off.data();
  o.d.Jtot = o.off[K]; o.d.Jmax = (int)jmax; o.d.k0 = 0; o.d.k1 = K;
}

// Mode A of a dense PARAFAC2 block as Engine::par2_prepare_modeA runs it in front of the common system build: the Gram
// matrices the B_k update leaves (par2_gram), par2_mode_a, and the Csys-only launch of a block with sparse slabs.
int aoadmm_op_par2_mode_a(aoadmm_ctx* ctx, int K, const int64_t* rows_k, int I, int R, const double* X, const double* B,
                          const double* Cmat, double* T1, double* GB, double* Amt, double* Csys, double* Csys_only,
                          int* path) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(X && B && Cmat, "bad arguments");
    Engine& e = *ctx->eng;
    hipStream_t s = e.stream();
    AO_HIP(hipSetDevice(e.device()));
    OpSlabs o;
    op_slabs(o, ctx, "aoadmm_op_par2_mode_a", K, rows_k, I, R, s);
    const P2Dims& d = o.d;
    const int64_t RR = (int64_t)R * R, nA = (int64_t)I * R;
    DevBuf x, b, c, t1, gb, am, cs, co;
    h2d(x, X, (int64_t)I * d.Jtot, s); h2d(b, B, d.Jtot * R, s); h2d(c, Cmat, (int64_t)K * R, s);
    t1.alloc((size_t)K * nA * 8); gb.alloc((size_t)K * RR * 8); am.alloc((size_t)nA * 8); cs.alloc((size_t)RR * 8);
    co.alloc((size_t)RR * 8);
    par2_gram(b.d(), d, gb.d(), s);
    par2_mode_a(x.d(), b.d(), c.d(), gb.d(), d, t1.d(), am.d(), cs.d(), s);
    par2_modeA_csys(c.d(), gb.d(), d, co.d(), s);
    if (path) { path[0] = par2_modeA_tile_width(d); path[1] = par2_modeA_csys_tile_width(d); }
    AO_HIP(hipStreamSynchronize(s));
    if (T1) d2h(T1, t1, (int64_t)K * nA, s);
    if (GB) d2h(GB, gb, (int64_t)K * RR, s);
    if (Amt) d2h(Amt, am, nA, s);
    if (Csys) d2h(Csys, cs, RR, s);
    if (Csys_only) d2h(Csys_only, co, RR, s);
  });
}

// Mode C of a dense PARAFAC2 block: system 0 = the uncoupled update as Engine::par2_update_C runs it (par2_c_systems,
// par2_c_solve on the path par2_c_path() names); systems 1..4 = the builders of Engine::par2_prepare_C_coupled
// (par2_c_coupled_kind, par2_c_systems, par2_rho_max, par2_c_coupled_big).
int aoadmm_op_par2_mode_c(aoadmm_ctx* ctx, int system, int K, const int64_t* rows_k, int I, int R, const double* X,
                          const double* A, const double* B, double weight, double ridge, double bsum_half, int constraint,
                          const double* params, int n_params, int max_inner, const double* tol, const double* sysmat,
                          double* Cmat, double* Z, double* mu, double* a, double* rho, double* L, double* rho_stats,
                          double* M, int* inner_iters, double* res, int* path) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(X && A && B && Cmat, "bad arguments");
    AO_REQUIRE(system >= AOADMM_P2CSYS_UNCOUPLED && system <= AOADMM_P2CSYS_DENSE, "system selector %d out of range", system);
    AO_REQUIRE(constraint >= AOADMM_C_NONE && constraint < AOADMM_C_TPARAFAC2 && constraint != AOADMM_C_QUADRATIC,
               "constraint id %d is not available here", constraint);
    const bool constr = constraint != AOADMM_C_NONE;
    const bool uncoupled = system == AOADMM_P2CSYS_UNCOUPLED;
    AO_REQUIRE(!uncoupled || !constr || (Z && mu && tol && max_inner >= 1), "a constrained C update needs Z, mu, tol and max_inner >= 1");
    AO_REQUIRE(system < AOADMM_P2CSYS_HHT || sysmat, "systems 2, 3 and 4 need their matrix (H*H', the diagonal of H'*H, H'*H)");
    Engine& e = *ctx->eng;
    hipStream_t s = e.stream();
    AO_HIP(hipSetDevice(e.device()));
    OpSlabs o;
    op_slabs(o, ctx, "aoadmm_op_par2_mode_c", K, rows_k, I, R, s);
    const P2Dims& d = o.d;
    const int64_t RR = (int64_t)R * R, KR = (int64_t)K * R, n = KR;
    if (system == AOADMM_P2CSYS_DENSE) AO_REQUIRE(n <= kDenseMaxN, "K*R = %lld exceeds the dense-system limit %d", (long long)n, kDenseMaxN);
    DevBuf x, af, bf, cf, ga, gb, t1, ac, rh, l, sm, rst, mbig, z, m, zold, v, ws, slots, red, ctl, aws;
    h2d(x, X, (int64_t)I * d.Jtot, s); h2d(af, A, (int64_t)I * R, s); h2d(bf, B, d.Jtot * R, s); h2d(cf, Cmat, KR, s);
    ga.alloc((size_t)RR * 8); gb.alloc((size_t)K * RR * 8); t1.alloc((size_t)K * I * R * 8);
    ac.alloc((size_t)KR * 8); rh.alloc((size_t)K * 8); l.alloc((size_t)K * RR * 8); rst.alloc(64);
    AO_HIP(hipMemsetAsync(l.p, 0, (size_t)K * RR * 8, s));
    aws.alloc(atb_ws_bytes(I, R, R));
    AdmmCtl* c = ctl_new(ctl, s);
    atb_small(ga.d(), af.d(), I, af.d(), I, I, R, R, aws.d(), nullptr, s);     // A'A as the A update leaves it (:148)
    par2_gram(bf.d(), d, gb.d(), s);                                           // B_k'B_k as the B_k update leaves them
    P2CSys cs;
    cs.X = x.d(); cs.A = af.d(); cs.B = bf.d(); cs.GA = ga.d(); cs.GB = gb.d(); cs.Cfac = cf.d();
    cs.w = weight; cs.ridge = ridge; cs.bsum_half = bsum_half;
    cs.T1 = t1.d(); cs.a = ac.d(); cs.rho = rh.d(); cs.L = l.d();
    int pth = -1;
    if (uncoupled) {
      cs.nrho = constr ? 1 : 0; cs.raw = 0;
      par2_c_systems(cs, d, c, s);
      P2CSolve g;
      g.a = ac.d(); g.rho = rh.d(); g.L = l.d(); g.fac = cf.d();
      g.constrained = constr; g.prox = make_spec(constraint, params, n_params);
      g.max_inner = constr ? max_inner : 0; g.tol_pr = constr ? tol[0] : 0.0; g.tol_du = constr ? tol[1] : 0.0;
      g.rhomax = rst.d();
      if (constr) {
        h2d(z, Z, KR, s); h2d(m, mu, KR, s);
        zold.alloc((size_t)KR * 8); v.alloc((size_t)KR * 8); ws.alloc(prox_ws_bytes(constraint, K, R));
        slots.alloc(8 * 8); red.alloc(4096 * sizeof(double));
        AO_HIP(hipMemsetAsync(slots.p, 0, 8 * 8, s));
        g.Z = z.d(); g.mu = m.d(); g.Zold = zold.d(); g.V = v.d(); g.prox_ws = ws.d(); g.slots = slots.d(); g.red_ws = red.d();
      }
      pth = (int)par2_c_solve(g, d, c, s);
    } else {
      // the coupling types that lead to each builder: 0 (also 3, 4) | 2 | 1 (also 5) with a diagonal / a dense H'H
      const int ctype = system == AOADMM_P2CSYS_ROWS ? 0 : (system == AOADMM_P2CSYS_HHT ? 2 : 1);
      const P2CCoupledKind ck = par2_c_coupled_kind(ctype, constr ? 1 : 0);
      if (sysmat) h2d(sm, sysmat, system == AOADMM_P2CSYS_HHT ? RR : (system == AOADMM_P2CSYS_DIAG ? (int64_t)K : (int64_t)K * K), s);
      cs.nrho = ck.nrho; cs.raw = ck.raw; cs.Madd = ck.madd ? sm.d() : nullptr;
      par2_c_systems(cs, d, c, s);
      par2_rho_max(rh.d(), K, rst.d(), s, rst.d() + 1, rst.d() + 2);
      if (ck.raw) {
        const bool diag = system == AOADMM_P2CSYS_DIAG;
        if (!diag) mbig.alloc((size_t)n * n * 8);
        par2_c_coupled_big(l.d(), sm.d(), diag, rst.d() + 1, constr ? 1 : 0, K, R, diag ? nullptr : mbig.d(), c, s);
      }
    }
    const AdmmCtl h = ctl_fetch(ctl, s);
    if (inner_iters) *inner_iters = h.iters;
    if (res) { res[0] = h.res[1]; res[1] = h.res[3]; }
    if (path) { path[0] = pth; path[1] = par2_c_rowsolve_class(R); }
    if (a) d2h(a, ac, KR, s);
    if (rho) d2h(rho, rh, K, s);
    if (L) d2h(L, l, (int64_t)K * RR, s);
    if (rho_stats && !(uncoupled && pth == (int)kP2CWgLoop)) d2h(rho_stats, rst, uncoupled ? 1 : 3, s);
    if (M && system == AOADMM_P2CSYS_DENSE) d2h(M, mbig, n * n, s);
    if (uncoupled) {
      d2h(Cmat, cf, KR, s);
      if (constr) { d2h(Z, z, KR, s); d2h(mu, m, KR, s); }
    }
  });
}

// Objective pieces of a dense PARAFAC2 block as Engine::par2_objective_enqueue runs them (par2_objective).
int aoadmm_op_par2_objective(aoadmm_ctx* ctx, int K, const int64_t* rows_k, int I, int R, const double* X, const double* A,
                             const double* B, const double* Cmat, const double* P, const double* DeltaB, const double* Z,
                             int reg_type, double eta, double* res, double* q, double* regv) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    AO_REQUIRE(X && A && B && Cmat && P && DeltaB && res && q, "bad arguments");
    AO_REQUIRE(reg_type == AOADMM_C_NONE || (prox_has_reg_value(reg_type) && reg_type != AOADMM_C_QUADRATIC && regv),
               "regularisation type %d has no value here", reg_type);
    Engine& e = *ctx->eng;
    hipStream_t s = e.stream();
    AO_HIP(hipSetDevice(e.device()));
    OpSlabs o;
    op_slabs(o, ctx, "aoadmm_op_par2_objective", K, rows_k, I, R, s);
    const P2Dims& d = o.d;
    const int64_t nB = d.Jtot * R;
    DevBuf x, af, bf, cf, pf, db, zf, rs, qq, rv;
    h2d(x, X, (int64_t)I * d.Jtot, s); h2d(af, A, (int64_t)I * R, s); h2d(bf, B, nB, s); h2d(cf, Cmat, (int64_t)K * R, s);
    h2d(pf, P, nB, s); h2d(db, DeltaB, (int64_t)R * R, s);
    if (Z) h2d(zf, Z, nB, s);
    rs.alloc((size_t)K * 8); qq.alloc((size_t)K * 4 * 8); rv.alloc((size_t)K * 8);
    P2Objective g;
    g.X = x.d(); g.A = af.d(); g.B = bf.d(); g.Cfac = cf.d(); g.P = pf.d(); g.DeltaB = db.d(); g.Z = Z ? zf.d() : nullptr;
    g.reg_type = reg_type; g.eta = eta;
    g.res = rs.d(); g.q = qq.d(); g.regv = rv.d();
    par2_objective(g, d, s);
    d2h(res, rs, K, s); d2h(q, qq, (int64_t)K * 4, s);
    if (reg_type != AOADMM_C_NONE) d2h(regv, rv, K, s);
  });
}

// The coupled loop of one coupling of the declared model as Engine::outer_updates runs it behind the MTTKRPs
// (Engine::coupled_loop_op: the solver's own system build, coupled_admm and Gram matrices).
int aoadmm_op_coupled_loop(aoadmm_ctx* ctx, int coupling, const double* const* A, const double* const* C, int max_inner,
                           const double* tol, int* inner_iters, double* res, double* rho, double* const* L,
                           double* const* gram, double* slots, int* path) {
  CTX_OR_FAIL(ctx);
  return guarded([&] {
    if (ctx->multi) throw Error(AOADMM_ERR_UNSUPPORTED, "aoadmm_op_coupled_loop runs on a single-device context");
    ctx->eng->coupled_loop_op(coupling, A, C, max_inner, tol, inner_iters, res, rho, L, gram, slots, path);
  });
}

}  // extern "C"
