/*
 * fake_aoadmm.cpp -- a recording fake of the part of the C ABI (include/aoadmm_hip.h) that the MEX gateway calls: the 36
 * aoadmm_* functions aoadmm_mex.cpp references.  No device, no arithmetic.  Every call appends one JSON line to a log --
 * {"fn": name, then the scalar arguments and a copy of the array arguments} -- that tests/mex_harness.py reads back, so
 * that what the gateway marshals can be asserted exactly on a machine without a GPU.  Doubles are written with 17
 * significant digits (they read back bit for bit), null pointers as null.
 *
 *   outputs     aoadmm_state_get fills host[e] = 1e6 * field + 1e3 * index + e; the traces, innerIters and the result
 *               scalars of aoadmm_solve, the held-out and ranking traces are fixed patterns (see each function)
 *   script      fake_script_solve sets exit_code / exit_abs and the iteration cap of the next solves;
 *               fake_fail(fn, status) makes the next call of `fn` return `status` (once)
 */
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "aoadmm_hip.h"

struct aoadmm_ctx { int id; };

namespace {

std::string g_log;
std::string g_error;
std::string g_fail_fn;
int g_fail_status = 0;
int g_created = 0, g_destroyed = 0;
int g_exit_code = 0, g_exit_abs[4] = {0, 0, 0, 0}, g_iter_cap = 3, g_nvecs_converged = 1;

// the model as described so far: what the sizes of the array arguments follow from
int g_n_modes = 0;
std::vector<int64_t> g_rows;                       // rows of a mode (a slab mode: the sum)
std::vector<std::vector<int64_t>> g_slab_rows;
std::vector<std::vector<int>> g_block_modes;
aoadmm_progress_fn g_progress = nullptr;
void* g_progress_user = nullptr;
int g_progress_every = 0;
int g_last_iters = 0;

void put(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_log += buf;
}
void num(double v) {
  if (v != v) g_log += "NaN";
  else put("%.17g", v);
}
struct Call {
  explicit Call(const char* fn) { put("{\"fn\": \"%s\"", fn); }
  ~Call() { g_log += "}\n"; }
  Call& i(const char* k, long long v) { put(", \"%s\": %lld", k, v); return *this; }
  Call& d(const char* k, double v) { put(", \"%s\": ", k); num(v); return *this; }
  template <class T> Call& arr(const char* k, const T* p, int64_t n, bool integer) {
    put(", \"%s\": ", k);
    if (!p) { g_log += "null"; return *this; }
    g_log += "[";
    for (int64_t e = 0; e < n; ++e) {
      if (e) g_log += ", ";
      if (integer) put("%lld", (long long)p[e]); else num((double)p[e]);
    }
    g_log += "]";
    return *this;
  }
  Call& ints(const char* k, const int64_t* p, int64_t n) { return arr(k, p, n, true); }
  Call& ints(const char* k, const int* p, int64_t n) { return arr(k, p, n, true); }
  Call& bytes(const char* k, const uint8_t* p, int64_t n) { return arr(k, p, n, true); }
  Call& dbl(const char* k, const double* p, int64_t n) { return arr(k, p, n, false); }
};

int status_of(const char* fn) {
  if (g_fail_fn == fn) {
    g_fail_fn.clear();
    g_error = std::string("fake: ") + fn + " was told to fail";
    return g_fail_status;
  }
  return AOADMM_OK;
}

// an index the model does not have is answered as the library answers it, not by running off an array
int invalid(const char* what) {
  g_error = std::string("fake: ") + what + " outside the model";
  return AOADMM_ERR_INVALID;
}
bool mode_ok(int m) { return m >= 0 && m < g_n_modes; }
bool block_ok(int p) { return p >= 0 && p < (int)g_block_modes.size(); }
int64_t block_size(int p) {
  int64_t n = 1;
  for (int m : g_block_modes.at((size_t)p)) n *= g_rows.at((size_t)m);
  return n;
}
int block_order(int p) { return (int)g_block_modes.at((size_t)p).size(); }

}  // namespace

extern "C" {

/* ---- the fake's own entry points -------------------------------------------------------------------------------- */
const char* fake_log(void) { return g_log.c_str(); }
void fake_clear_log(void) { g_log.clear(); }
void fake_fail(const char* fn, int status) { g_fail_fn = fn; g_fail_status = status; }
void fake_script_solve(int exit_code, const int exit_abs[4], int iter_cap) {
  g_exit_code = exit_code;
  for (int i = 0; i < 4; ++i) g_exit_abs[i] = exit_abs ? exit_abs[i] : 0;
  g_iter_cap = iter_cap;
}
void fake_script_nvecs(int converged) { g_nvecs_converged = converged; }
int fake_contexts_created(void) { return g_created; }
int fake_contexts_destroyed(void) { return g_destroyed; }

/* ---- the C ABI -------------------------------------------------------------------------------------------------- */
const char* aoadmm_last_error(void) { return g_error.c_str(); }
int aoadmm_create(aoadmm_ctx** ctx, int device) {
  Call("aoadmm_create").i("device", device);
  const int st = status_of("aoadmm_create");
  if (st) return st;
  *ctx = new aoadmm_ctx{++g_created};
  return AOADMM_OK;
}
int aoadmm_create_multi(aoadmm_ctx** ctx, int n, const int* devices) {
  Call("aoadmm_create_multi").i("n_devices", n).ints("devices", devices, n);
  const int st = status_of("aoadmm_create_multi");
  if (st) return st;
  *ctx = new aoadmm_ctx{++g_created};
  return AOADMM_OK;
}
int aoadmm_destroy(aoadmm_ctx* ctx) {
  Call("aoadmm_destroy").i("ctx", ctx ? ctx->id : 0);
  ++g_destroyed;
  delete ctx;
  return AOADMM_OK;
}
int aoadmm_set_progress(aoadmm_ctx*, aoadmm_progress_fn fn, void* user, int every) {
  Call("aoadmm_set_progress").i("set", fn != nullptr).i("every", every);
  g_progress = fn; g_progress_user = user; g_progress_every = every;
  return status_of("aoadmm_set_progress");
}
int aoadmm_model_begin(aoadmm_ctx* ctx, int n_modes, int n_tensors, int n_couplings) {
  Call("aoadmm_model_begin").i("ctx", ctx ? ctx->id : 0).i("n_modes", n_modes).i("n_tensors", n_tensors).i("n_couplings", n_couplings);
  g_n_modes = n_modes;
  g_rows.assign((size_t)n_modes, 0);
  g_slab_rows.assign((size_t)n_modes, {});
  g_block_modes.assign((size_t)n_tensors, {});
  return status_of("aoadmm_model_begin");
}
int aoadmm_model_set_mode(aoadmm_ctx*, int mode, int64_t rows, int rank) {
  if (!(mode_ok(mode))) { Call("aoadmm_model_set_mode").i("refused", 1); return invalid("mode"); }
  Call("aoadmm_model_set_mode").i("mode", mode).i("rows", rows).i("rank", rank);
  g_rows.at((size_t)mode) = rows;
  return status_of("aoadmm_model_set_mode");
}
int aoadmm_model_set_mode_slabs(aoadmm_ctx*, int mode, int K, const int64_t* rows_k, int rank) {
  if (!(mode_ok(mode))) { Call("aoadmm_model_set_mode_slabs").i("refused", 1); return invalid("mode"); }
  Call("aoadmm_model_set_mode_slabs").i("mode", mode).i("K", K).ints("rows_k", rows_k, K).i("rank", rank);
  g_slab_rows.at((size_t)mode).assign(rows_k, rows_k + K);
  g_rows.at((size_t)mode) = 0;
  for (int k = 0; k < K; ++k) g_rows[(size_t)mode] += rows_k[k];
  return status_of("aoadmm_model_set_mode_slabs");
}
int aoadmm_model_add_cp(aoadmm_ctx*, int p, int n, const int* modes, double weight) {
  Call("aoadmm_model_add_cp").i("p", p).i("n_tensor_modes", n).ints("modes", modes, n).d("weight", weight);
  if (!block_ok(p)) return invalid("block");
  for (int i = 0; i < n; ++i)
    if (!mode_ok(modes[i])) return invalid("mode");
  g_block_modes[(size_t)p].assign(modes, modes + n);
  return status_of("aoadmm_model_add_cp");
}
int aoadmm_model_add_par2(aoadmm_ctx*, int p, const int* modes3, double weight) {
  Call("aoadmm_model_add_par2").i("p", p).ints("modes", modes3, 3).d("weight", weight);
  if (!block_ok(p)) return invalid("block");
  for (int i = 0; i < 3; ++i)
    if (!mode_ok(modes3[i])) return invalid("mode");
  g_block_modes[(size_t)p].assign(modes3, modes3 + 2);              // data: I x sum J_k
  return status_of("aoadmm_model_add_par2");
}
int aoadmm_model_set_constraint(aoadmm_ctx*, int mode, int constraint, const double* params, int n_params, const double* Lmat) {
  if (!(mode_ok(mode))) { Call("aoadmm_model_set_constraint").i("refused", 1); return invalid("mode"); }
  const int64_t r = g_rows.at((size_t)mode);
  Call("aoadmm_model_set_constraint").i("mode", mode).i("constraint", constraint).dbl("params", params, n_params)
      .i("n_params", n_params).dbl("Lmat", Lmat, r * r);
  return status_of("aoadmm_model_set_constraint");
}
int aoadmm_model_set_coupling(aoadmm_ctx*, int mode, int coupling, const double* H, int64_t hr, int64_t hc, const double* H2,
                              int64_t h2r, int64_t h2c) {
  Call("aoadmm_model_set_coupling").i("mode", mode).i("coupling", coupling).dbl("H", H, hr * hc).i("hr", hr).i("hc", hc)
      .dbl("H2", H2, h2r * h2c).i("h2r", h2r).i("h2c", h2c);
  return status_of("aoadmm_model_set_coupling");
}
int aoadmm_model_set_coupling_type(aoadmm_ctx*, int coupling, int type) {
  Call("aoadmm_model_set_coupling_type").i("coupling", coupling).i("type", type);
  return status_of("aoadmm_model_set_coupling_type");
}
int aoadmm_model_set_ridge(aoadmm_ctx*, const double* ridge) {
  Call("aoadmm_model_set_ridge").dbl("ridge", ridge, g_n_modes);
  return status_of("aoadmm_model_set_ridge");
}
int aoadmm_model_end(aoadmm_ctx*) {
  Call("aoadmm_model_end");
  return status_of("aoadmm_model_end");
}
int aoadmm_tensor_upload(aoadmm_ctx*, int p, const double* data, int precision) {
  if (!(block_ok(p))) { Call("aoadmm_tensor_upload").i("refused", 1); return invalid("block"); }
  Call("aoadmm_tensor_upload").i("p", p).dbl("data", data, block_size(p)).i("precision", precision);
  return status_of("aoadmm_tensor_upload");
}
int aoadmm_par2_slab_upload(aoadmm_ctx*, int p, int k, const double* Xk) {
  if (!(block_ok(p))) { Call("aoadmm_par2_slab_upload").i("refused", 1); return invalid("block"); }
  const std::vector<int>& md = g_block_modes.at((size_t)p);
  const int64_t I = g_rows.at((size_t)md[0]);
  const int64_t J = k == AOADMM_ALL_SLABS ? g_rows.at((size_t)md[1]) : g_slab_rows.at((size_t)md[1]).at((size_t)k);
  Call("aoadmm_par2_slab_upload").i("p", p).i("k", k).dbl("data", Xk, I * J);
  return status_of("aoadmm_par2_slab_upload");
}
int aoadmm_tensor_mask_upload(aoadmm_ctx*, int p, const uint8_t* mask) {
  if (!(block_ok(p))) { Call("aoadmm_tensor_mask_upload").i("refused", 1); return invalid("block"); }
  Call("aoadmm_tensor_mask_upload").i("p", p).bytes("mask", mask, block_size(p));
  return status_of("aoadmm_tensor_mask_upload");
}
int aoadmm_par2_slab_mask_upload(aoadmm_ctx*, int p, int k, const uint8_t* mask_k) {
  if (!(block_ok(p))) { Call("aoadmm_par2_slab_mask_upload").i("refused", 1); return invalid("block"); }
  const std::vector<int>& md = g_block_modes.at((size_t)p);
  const int64_t n = g_rows.at((size_t)md[0]) * g_slab_rows.at((size_t)md[1]).at((size_t)k);
  Call("aoadmm_par2_slab_mask_upload").i("p", p).i("k", k).bytes("mask", mask_k, n);
  return status_of("aoadmm_par2_slab_mask_upload");
}
int aoadmm_tensor_upload_coo(aoadmm_ctx*, int p, int64_t nnz, const int64_t* subs, const double* vals) {
  if (!(block_ok(p))) { Call("aoadmm_tensor_upload_coo").i("refused", 1); return invalid("block"); }
  Call("aoadmm_tensor_upload_coo").i("p", p).i("nnz", nnz).ints("subs", subs, nnz * block_order(p)).dbl("vals", vals, nnz);
  return status_of("aoadmm_tensor_upload_coo");
}
int aoadmm_tensor_upload_coo_sharded(aoadmm_ctx*, int p, int64_t nnz, const int64_t* subs, const double* vals) {
  if (!(block_ok(p))) { Call("aoadmm_tensor_upload_coo_sharded").i("refused", 1); return invalid("block"); }
  Call("aoadmm_tensor_upload_coo_sharded").i("p", p).i("nnz", nnz).ints("subs", subs, nnz * block_order(p)).dbl("vals", vals, nnz);
  return status_of("aoadmm_tensor_upload_coo_sharded");
}
int aoadmm_par2_slab_upload_coo(aoadmm_ctx*, int p, int64_t nnz, const int64_t* subs, const double* vals) {
  Call("aoadmm_par2_slab_upload_coo").i("p", p).i("nnz", nnz).ints("subs", subs, nnz * 3).dbl("vals", vals, nnz);
  return status_of("aoadmm_par2_slab_upload_coo");
}
int aoadmm_tensor_set_observed_only(aoadmm_ctx*, int p, int on) {
  Call("aoadmm_tensor_set_observed_only").i("p", p).i("on", on);
  return status_of("aoadmm_tensor_set_observed_only");
}
int aoadmm_tensor_set_entry_weights(aoadmm_ctx*, int p, int64_t nnz, const int64_t* subs, const double* wts, double alpha) {
  if (!(block_ok(p))) { Call("aoadmm_tensor_set_entry_weights").i("refused", 1); return invalid("block"); }
  Call("aoadmm_tensor_set_entry_weights").i("p", p).i("nnz", nnz).ints("subs", subs, nnz * block_order(p)).dbl("wts", wts, nnz)
      .d("unstored_weight", alpha);
  return status_of("aoadmm_tensor_set_entry_weights");
}
int aoadmm_tensor_set_heldout(aoadmm_ctx*, int p, int64_t n, const int64_t* subs, const double* vals) {
  if (!(block_ok(p))) { Call("aoadmm_tensor_set_heldout").i("refused", 1); return invalid("block"); }
  const int N = block_order(p) == 2 && g_slab_rows.at((size_t)g_block_modes[(size_t)p][1]).size() ? 3 : block_order(p);
  Call("aoadmm_tensor_set_heldout").i("p", p).i("n", n).ints("subs", subs, n * N).dbl("vals", vals, n);
  return status_of("aoadmm_tensor_set_heldout");
}
int aoadmm_tensor_set_ranklist(aoadmm_ctx*, int p, int mode, int64_t nq, const int64_t* subs, const int64_t* excl_off,
                               const int64_t* excl_idx) {
  if (!(block_ok(p))) { Call("aoadmm_tensor_set_ranklist").i("refused", 1); return invalid("block"); }
  const int64_t n_ex = excl_off ? excl_off[nq] : 0;
  Call("aoadmm_tensor_set_ranklist").i("p", p).i("mode", mode).i("nq", nq).ints("subs", subs, nq * block_order(p))
      .ints("excl_off", excl_off, nq + 1).ints("excl_idx", excl_idx, n_ex).i("excl_idx_set", excl_idx != nullptr);
  return status_of("aoadmm_tensor_set_ranklist");
}
int aoadmm_rank_track(aoadmm_ctx*, int metric, int k, int every, int patience, int criterion) {
  Call("aoadmm_rank_track").i("metric", metric).i("k", k).i("every", every).i("patience", patience).i("criterion", criterion);
  return status_of("aoadmm_rank_track");
}
int aoadmm_heldout_keep_best(aoadmm_ctx*, int on) {
  Call("aoadmm_heldout_keep_best").i("on", on);
  return status_of("aoadmm_heldout_keep_best");
}
int aoadmm_heldout_restore_best(aoadmm_ctx*, int* iter) {
  Call("aoadmm_heldout_restore_best");
  if (iter) *iter = 1;
  return status_of("aoadmm_heldout_restore_best");
}
/* out[i] = 700 + 10 p + i for i = 0 .. iterations of the last solve; best_iter = 1 */
int aoadmm_heldout_trace(aoadmm_ctx*, int p, double* out, int cap, int* len, int* best_iter) {
  Call("aoadmm_heldout_trace").i("p", p).i("cap", cap);
  for (int i = 0; out && i < cap && i <= g_last_iters; ++i) out[i] = 700.0 + 10.0 * p + i;
  if (len) *len = g_last_iters + 1;
  if (best_iter) *best_iter = 1;
  return status_of("aoadmm_heldout_trace");
}
/* one evaluation per iteration: out[e] = 100 (what + 1) + 10 p + e, but N_AUC of evaluation 0 is 0 (its AUC mean is NaN);
 * iters[e] = 2 e; best_iter = 2 */
int aoadmm_rank_trace(aoadmm_ctx*, int p, int what, double* out, int cap, int* len, int* iters, int* best_iter) {
  Call("aoadmm_rank_trace").i("p", p).i("what", what).i("cap", cap);
  for (int e = 0; e < cap && e <= g_last_iters; ++e) {
    if (out) out[e] = what == AOADMM_RANKSUM_N_AUC && e == 0 ? 0.0 : 100.0 * (what + 1) + 10.0 * p + e;
    if (iters) iters[e] = 2 * e;
  }
  if (len) *len = g_last_iters + 1;
  if (best_iter) *best_iter = 2;
  return status_of("aoadmm_rank_trace");
}
int aoadmm_state_set(aoadmm_ctx*, int field, int index, int slab, const double* host, int64_t rows, int64_t cols) {
  Call("aoadmm_state_set").i("field", field).i("index", index).i("slab", slab).dbl("host", host, rows * cols).i("rows", rows)
      .i("cols", cols);
  return status_of("aoadmm_state_set");
}
int aoadmm_state_get(aoadmm_ctx*, int field, int index, int slab, double* host, int64_t rows, int64_t cols) {
  Call("aoadmm_state_get").i("field", field).i("index", index).i("slab", slab).i("rows", rows).i("cols", cols);
  for (int64_t e = 0; e < rows * cols; ++e) host[e] = 1e6 * field + 1e3 * index + (double)e;
  return status_of("aoadmm_state_get");
}
/* OuterIterations = min(iteration cap, MaxOuterIters); trace t has t[i] = 100 (t + 1) + i in the order func_val_conv,
 * func_coupl_conv, func_constr_conv, func_PAR2_coupl, time_at_it, func_rel_missing; innerIters[m + n_modes i] = 10 m + i + 1;
 * the result scalars are 1.5, 2.5, 3.5, 4.5 and f_rel_missing = 0.125.  A progress callback gets its rows on this thread. */
int aoadmm_solve(aoadmm_ctx*, const aoadmm_options* o, aoadmm_result* r) {
  Call("aoadmm_solve").i("MaxOuterIters", o->MaxOuterIters).i("MaxInnerIters", o->MaxInnerIters).d("AbsFuncTol", o->AbsFuncTol)
      .d("OuterRelTol", o->OuterRelTol).d("innerRelPrTol_coupl", o->innerRelPrTol_coupl).d("innerRelPrTol_constr", o->innerRelPrTol_constr)
      .d("innerRelDualTol_coupl", o->innerRelDualTol_coupl).d("innerRelDualTol_constr", o->innerRelDualTol_constr).i("bsum", o->bsum)
      .d("bsum_weight", o->bsum_weight).i("iter_start_PAR2Bkconstraint", o->iter_start_PAR2Bkconstraint)
      .i("has_increase_factor_rhoBk", o->has_increase_factor_rhoBk).d("increase_factor_rhoBk", o->increase_factor_rhoBk)
      .i("use_dimtree", o->use_dimtree).i("no_permuted_copy", o->no_permuted_copy).i("par2_slab_sharding", o->par2_slab_sharding)
      .i("heldout_patience", o->heldout_patience).ints("reserved", o->reserved, 4);
  const int st = status_of("aoadmm_solve");
  if (st) return st;
  const int it = o->MaxOuterIters < g_iter_cap ? o->MaxOuterIters : g_iter_cap;
  g_last_iters = it;
  double* tr[6] = {r->func_val_conv, r->func_coupl_conv, r->func_constr_conv, r->func_PAR2_coupl, r->time_at_it, r->func_rel_missing};
  for (int t = 0; t < 6; ++t)
    for (int i = 0; tr[t] && i <= it; ++i) tr[t][i] = 100.0 * (t + 1) + i;
  if (r->func_rel_missing) r->func_rel_missing[0] = std::numeric_limits<double>::quiet_NaN();
  for (int i = 0; i < (it > 0 ? it : 1); ++i)
    for (int m = 0; m < g_n_modes; ++m) r->innerIters[m + (size_t)g_n_modes * i] = 10.0 * m + i + 1;
  r->f_tensors = 1.5; r->f_couplings = 2.5; r->f_constraints = 3.5; r->f_PAR2_couplings = 4.5; r->f_rel_missing = 0.125;
  r->OuterIterations = it;
  r->exit_code = g_exit_code;
  for (int i = 0; i < 4; ++i) r->exit_abs[i] = g_exit_abs[i];
  if (g_progress && g_progress_every > 0)
    for (int i = 0; i <= it; i += g_progress_every) {
      const double f[4] = {1.0 + i, 0.25, 0.5, 0.125};
      g_progress(g_progress_user, i, f, 0.0625 * i);
    }
  return AOADMM_OK;
}
/* out[e] = 5e6 + e */
int aoadmm_op_unfold_gram(aoadmm_ctx*, const double* X, int ndims, const int64_t* dims, int n, int precision, double* out) {
  int64_t total = 1;
  for (int i = 0; i < ndims; ++i) total *= dims[i];
  Call("aoadmm_op_unfold_gram").dbl("X", X, total).i("ndims", ndims).ints("dims", dims, ndims).i("n", n).i("precision", precision);
  for (int64_t e = 0; e < dims[n] * dims[n]; ++e) out[e] = 5e6 + (double)e;
  return status_of("aoadmm_op_unfold_gram");
}
/* U(i, j) = 6e6 + i + ldU j */
int aoadmm_resident_nvecs(aoadmm_ctx*, int p, int tensor_mode, int r, const aoadmm_nvecs_options* opt, double* U, int64_t ldU,
                          double* eigvals, aoadmm_nvecs_info* info) {
  Call("aoadmm_resident_nvecs").i("p", p).i("tensor_mode", tensor_mode).i("r", r).i("opt_set", opt != nullptr).i("ldU", ldU)
      .i("eigvals_set", eigvals != nullptr);
  for (int64_t e = 0; e < ldU * r; ++e) U[e] = 6e6 + (double)e;
  if (info) { info->iterations = 7; info->converged = g_nvecs_converged; info->block = r; info->residual = 0.5; info->fibers = 1; }
  return status_of("aoadmm_resident_nvecs");
}

}  // extern "C"
