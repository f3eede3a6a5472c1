/*
 * aoadmm_mex.cpp -- MEX gateway: MATLAB <-> libaoadmm_hip.so (C ABI in include/aoadmm_hip.h).
 *
 * Marshalling only.  It replaces the call
 *     [Fac,out] = cmtf_fun_AOADMM(Z,Znorm_const,G,fh,gh,lscalar,uscalar,options)
 * at functions/cmtf_AOADMM.m:193 of the reference: the MATLAB wrapper
 * cmtf_fun_AOADMM_hip.m (same directory) passes the structs Z, G and options; this
 * file walks them with the mx* API, feeds the engine through the C ABI and builds
 * `Fac` (same fields as G) and `out` (cmtf_fun_AOADMM.m:480-494).
 *
 * Build (on a machine that has MATLAB):
 *     mex -R2018a -largeArrayDims aoadmm_mex.cpp -I../../include -L.. -laoadmm_hip
 * Neither mex.h nor libmx exist where the project is developed and tested.  There this file is compiled against
 * mex_stub/mex.h and linked with a functional mock of the C Matrix API (tests/mxmock/mxmock.cpp), and its logic is
 * executed: on the CPU against a recording fake of the C ABI (tests/test_mex_gateway_host.py: every marshalled value,
 * every field of Fac / out and every error id below is asserted) and on the GPU against libaoadmm_hip.so, bit for bit
 * beside driver.py (tests/test_gpu_mex_gateway.py).  Real MATLAB has still never run it.
 *
 * Errors: every non-zero status becomes mexErrMsgIdAndTxt with an id in the
 * `cmtf:` namespace; AOADMM_ERR_UNSUPPORTED maps to
 * `cmtf:hip:unsupported`, which the wrapper catches to fall back to the original
 * MATLAB implementation.
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "mex.h"
#include "aoadmm_hip.h"

namespace {

aoadmm_ctx* g_ctx = nullptr;
std::vector<int> g_devices;      // the device list g_ctx was created for
bool g_at_exit = false;

void at_exit() {
  if (g_ctx) {
    aoadmm_destroy(g_ctx);
    g_ctx = nullptr;
  }
}

void check(int status) {
  if (status == AOADMM_OK) return;
  const char* msg = aoadmm_last_error();
  switch (status) {
    case AOADMM_ERR_NOT_PD: mexErrMsgIdAndTxt("cmtf:hip:notPositiveDefinite", "%s", msg); break;
    case AOADMM_ERR_UNSUPPORTED: mexErrMsgIdAndTxt("cmtf:hip:unsupported", "%s", msg); break;
    case AOADMM_ERR_HIP: mexErrMsgIdAndTxt("cmtf:hip:device", "%s", msg); break;
    case AOADMM_ERR_RCCL: mexErrMsgIdAndTxt("cmtf:hip:rccl", "%s", msg); break;
    case AOADMM_ERR_NOMEM: mexErrMsgIdAndTxt("cmtf:hip:outOfMemory", "%s", msg); break;
    default: mexErrMsgIdAndTxt("cmtf:hip:invalid", "%s", msg); break;
  }
}

const mxArray* field(const mxArray* s, const char* name, bool required = true) {
  const mxArray* f = mxIsStruct(s) ? mxGetField(s, 0, name) : nullptr;
  if (!f && required) mexErrMsgIdAndTxt("cmtf:hip:missingField", "Reference to non-existent field '%s'.", name);
  return f;
}

double scalar(const mxArray* s, const char* name) { return mxGetScalar(field(s, name)); }

std::string str(const mxArray* a) {
  char* c = mxArrayToString(a);
  std::string r = c ? c : "";
  mxFree(c);
  return r;
}

// constraint names of "List of constraints and regularizations.txt" -> AOADMM_C_* ids
int constraint_id(const std::string& n) {
  static const struct { const char* name; int id; } tab[] = {
      {"non-negativity", AOADMM_C_NONNEG}, {"box", AOADMM_C_BOX}, {"simplex column-wise", AOADMM_C_SIMPLEX_COL},
      {"simplex row-wise", AOADMM_C_SIMPLEX_ROW}, {"non-decreasing", AOADMM_C_NONDECREASING},
      {"non-increasing", AOADMM_C_NONINCREASING}, {"unimodality", AOADMM_C_UNIMODAL}, {"l1-ball", AOADMM_C_L1_BALL},
      {"l2-ball", AOADMM_C_L2_BALL}, {"non-negative l2-ball", AOADMM_C_NONNEG_L2_BALL},
      {"non-negative l2-sphere", AOADMM_C_NONNEG_L2_SPHERE}, {"orthonormal", AOADMM_C_ORTHONORMAL},
      {"l1 regularization", AOADMM_C_L1_REG}, {"l0 regularization", AOADMM_C_L0_REG},
      {"l2 regularization", AOADMM_C_L2_REG}, {"ridge", AOADMM_C_RIDGE},
      {"quadratic regularization", AOADMM_C_QUADRATIC}, {"GL smoothness", AOADMM_C_GL_SMOOTH},
      {"TV regularization", AOADMM_C_TV}, {"tPARAFAC2", AOADMM_C_TPARAFAC2}};
  for (const auto& e : tab)
    if (n == e.name) return e.id;
  if (n == "custom")
    mexErrMsgIdAndTxt("cmtf:hip:unsupported", "'custom' prox handles cannot cross to the device (constraints_to_prox.m:86-90)");
  mexErrMsgIdAndTxt("cmtf:hip:invalid", "unknown constraint '%s'", n.c_str());
  return 0;
}

// dense numeric data of a Tensor Toolbox `tensor` (field .data) or a plain array.  Anything else (single, logical,
// integer, complex sparse, a sparse logical matrix, an sptensor with non-double or complex values) is routed back to
// the MATLAB path (cmtf:hip:unsupported, caught by cmtf_fun_AOADMM_hip.m).
const mxArray* dense_data(const mxArray* obj) {
  if (mxIsDouble(obj) && !mxIsSparse(obj)) return obj;
  const mxArray* d = mxIsClass(obj, "tensor") ? mxGetProperty(obj, 0, "data") : nullptr;
  if (!d || !mxIsDouble(d))
    mexErrMsgIdAndTxt("cmtf:hip:unsupported", "Z.object is not a double array, a dense tensor, a real double sptensor or a "
                                              "real sparse double matrix: it stays on the MATLAB path");
  return d;
}

// an sptensor, or a real sparse double matrix (a complex or logical sparse matrix goes through dense_data's fallback)
bool is_sparse_object(const mxArray* obj) {
  return mxIsClass(obj, "sptensor") || (mxIsDouble(obj) && mxIsSparse(obj) && !mxIsComplex(obj));
}

// Z.object{p} as an sptensor (subs 1-based doubles nnz x N, vals nnz x 1, size) or a MATLAB sparse double matrix
// (compressed columns: ir / jc / values) -> 0-based int64 COO, column-major nnz x N, through aoadmm_tensor_upload_coo.
// The sizes must be those of Z.size for the block's modes (`md`).
// the conversion alone; N < 0: whatever order the sptensor has
void read_sparse(int p, const mxArray* obj, int N, std::vector<int64_t>& subs, std::vector<double>& vals,
                 std::vector<double>& shape) {
  if (mxIsClass(obj, "sptensor")) {
    mxArray* s = mxGetProperty(obj, 0, "subs");
    mxArray* v = mxGetProperty(obj, 0, "vals");
    mxArray* z = mxGetProperty(obj, 0, "size");
    if (!s || !v || !z || !mxIsDouble(s) || !mxIsDouble(z))
      mexErrMsgIdAndTxt("cmtf:hip:invalid", "Z.object{%d}: sptensor without double subs / size", p + 1);
    if (!mxIsDouble(v) || mxIsComplex(v))
      mexErrMsgIdAndTxt("cmtf:hip:unsupported", "Z.object{%d}: sptensor values are not real doubles: it stays on the MATLAB path", p + 1);
    shape.assign(mxGetDoubles(z), mxGetDoubles(z) + mxGetNumberOfElements(z));
    if (N < 0) N = (int)shape.size();
    const size_t nnz = mxGetNumberOfElements(v);
    if (nnz > 0 && (mxGetM(s) != nnz || (int)mxGetN(s) != N))
      mexErrMsgIdAndTxt("cmtf:hip:invalid", "Z.object{%d}: sptensor subs is not nnz x %d", p + 1, N);
    subs.resize(nnz * N);
    const double* sd = nnz ? mxGetDoubles(s) : nullptr;
    for (size_t i = 0; i < nnz * N; ++i) subs[i] = (int64_t)sd[i] - 1;
    vals.assign(mxGetDoubles(v), mxGetDoubles(v) + nnz);
    mxDestroyArray(s);                                    // the property copies: no second copy of subs held further on
    mxDestroyArray(v);
    mxDestroyArray(z);
  } else {
    const size_t M = mxGetM(obj), C = mxGetN(obj);
    const mwIndex* jc = mxGetJc(obj);
    const mwIndex* ir = mxGetIr(obj);
    const size_t nnz = jc[C];
    shape = {(double)M, (double)C};
    subs.resize(nnz * 2);
    for (size_t j = 0; j < C; ++j)
      for (mwIndex k = jc[j]; k < jc[j + 1]; ++k) { subs[k] = (int64_t)ir[k]; subs[nnz + k] = (int64_t)j; }
    vals.assign(mxGetDoubles(obj), mxGetDoubles(obj) + nnz);
  }
}

// wts (weighted): options.hip.sparse_entry_weights{p}, aligned with the entries of the object as read_sparse returns them
// (an sptensor's subs / vals, a sparse matrix's stored entries column by column), or null / empty for stored weights 1;
// alpha: the block's unstored weight (aoadmm_tensor_set_entry_weights, which marks the block observed-only)
void upload_sparse(int p, const mxArray* obj, const mxArray* sz, const std::vector<int>& md, bool sharded,
                   bool weighted = false, const mxArray* wts = nullptr, double alpha = 0.0) {
  const int N = (int)md.size();
  std::vector<int64_t> subs;
  std::vector<double> vals;
  std::vector<double> shape;
  read_sparse(p, obj, N, subs, vals, shape);
  bool same = (int)shape.size() == N;
  for (int i = 0; same && i < N; ++i) same = shape[i] == mxGetScalar(mxGetCell(sz, md[i]));
  if (!same) mexErrMsgIdAndTxt("cmtf:hip:invalid", "Z.object{%d}: size does not match Z.size of its modes", p + 1);
  // options.hip.sparse_sharding: the engines of a multi-device context (options.hip.devices) keep one share each
  check((sharded ? aoadmm_tensor_upload_coo_sharded : aoadmm_tensor_upload_coo)(g_ctx, p, (int64_t)vals.size(), subs.data(),
                                                                                vals.data()));
  if (!weighted) return;
  if (wts && !mxIsEmpty(wts)) {
    if (!mxIsDouble(wts) || mxIsComplex(wts) || mxGetNumberOfElements(wts) != vals.size())
      mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.sparse_entry_weights{%d} must hold one real double per stored entry of Z.object{%d} (%d)",
                        p + 1, p + 1, (int)vals.size());
    check(aoadmm_tensor_set_entry_weights(g_ctx, p, (int64_t)vals.size(), subs.data(), mxGetDoubles(wts), alpha));
  } else {
    check(aoadmm_tensor_set_entry_weights(g_ctx, p, 0, nullptr, nullptr, alpha));
  }
}

void put_state(int field_id, int index, int slab, const mxArray* a) {
  if (!a || mxIsEmpty(a)) return;
  check(aoadmm_state_set(g_ctx, field_id, index, slab, mxGetDoubles(a), (int64_t)mxGetM(a), (int64_t)mxGetN(a)));
}

void put_state_maybe_cell(int field_id, int index, const mxArray* a) {
  if (!a || mxIsEmpty(a)) return;
  if (mxIsCell(a)) {
    // all cells in one transfer: J_k x R blocks back to back (AOADMM_ALL_SLABS)
    std::vector<double> packed;
    int64_t rows = 0, cols = 0;
    for (mwSize k = 0; k < mxGetNumberOfElements(a); ++k) {
      const mxArray* ak = mxGetCell(a, k);
      if (!ak || mxIsEmpty(ak)) mexErrMsgIdAndTxt("cmtf:hip:state", "empty cell %d in a cell-valued state field", (int)k + 1);
      const double* d = mxGetDoubles(ak);
      packed.insert(packed.end(), d, d + mxGetNumberOfElements(ak));
      rows += (int64_t)mxGetM(ak);
      cols = (int64_t)mxGetN(ak);
    }
    check(aoadmm_state_set(g_ctx, field_id, index, AOADMM_ALL_SLABS, packed.data(), rows, cols));
  } else {
    put_state(field_id, index, 0, a);
  }
}

struct ProgressState { bool has_missing = false; };
void print_progress(void* user, int iter, const double f[4], double f_rel_missing) {
  const ProgressState* ps = static_cast<const ProgressState*>(user);
  if (ps->has_missing)
    mexPrintf("%6d %12f %12f %12f %17f %12f %12f\n", iter, f[0] + f[1] + f[2] + f[3], f[0], f[1], f[2], f[3], f_rel_missing);
  else
    mexPrintf("%6d %12f %12f %12f %17f %12f\n", iter, f[0] + f[1] + f[2] + f[3], f[0], f[1], f[2], f[3]);
  mexEvalString("drawnow;");                          // flush the command window while the solve is running
}

// mxSetCell does not free the element it replaces (the copy of G's, here): destroy it, or every call leaks it
void replace_cell(mxArray* c, mwIndex i, mxArray* v) {
  mxArray* old = mxGetCell(c, i);
  mxSetCell(c, i, v);
  mxDestroyArray(old);
}

mxArray* get_like(int field_id, int index, const mxArray* ref) {
  if (!ref || mxIsEmpty(ref)) return mxCreateDoubleMatrix(0, 0, mxREAL);
  if (mxIsCell(ref)) {
    mxArray* c = mxCreateCellMatrix(mxGetM(ref), mxGetN(ref));
    int64_t rows = 0, cols = 0;
    for (mwSize k = 0; k < mxGetNumberOfElements(ref); ++k) {
      rows += (int64_t)mxGetM(mxGetCell(ref, k));
      cols = (int64_t)mxGetN(mxGetCell(ref, k));
    }
    std::vector<double> packed((size_t)(rows * cols));
    check(aoadmm_state_get(g_ctx, field_id, index, AOADMM_ALL_SLABS, packed.data(), rows, cols));
    size_t o0 = 0;
    for (mwSize k = 0; k < mxGetNumberOfElements(ref); ++k) {
      const mxArray* rk = mxGetCell(ref, k);
      mxArray* o = mxCreateDoubleMatrix(mxGetM(rk), mxGetN(rk), mxREAL);
      std::copy(packed.begin() + o0, packed.begin() + o0 + mxGetNumberOfElements(rk), mxGetDoubles(o));
      o0 += mxGetNumberOfElements(rk);
      mxSetCell(c, k, o);
    }
    return c;
  }
  mxArray* o = mxCreateDoubleMatrix(mxGetM(ref), mxGetN(ref), mxREAL);
  check(aoadmm_state_get(g_ctx, field_id, index, 0, mxGetDoubles(o), (int64_t)mxGetM(ref), (int64_t)mxGetN(ref)));
  return o;
}

}  // namespace

/* [Fac, out] = aoadmm_mex(Z, G, options)      (options.hip.device / .precision are optional) */
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  // Y = aoadmm_mex('unfold_gram', X, n): Gram matrix of the mode-n unfolding (cmtf_nvecs.m:40-56), n 1-based
  if (nrhs == 3 && mxIsChar(prhs[0])) {
    if (str(prhs[0]) != "unfold_gram") mexErrMsgIdAndTxt("cmtf:hip:usage", "unknown operation '%s'", str(prhs[0]).c_str());
    if (!g_ctx) {
      check(aoadmm_create(&g_ctx, 0));
      g_devices.assign(1, 0);
      if (!g_at_exit) { mexAtExit(at_exit); g_at_exit = true; }
    }
    const mxArray* X = prhs[1];
    const int nd = (int)mxGetNumberOfDimensions(X);
    const mwSize* d = mxGetDimensions(X);
    int64_t dims[8];
    for (int i = 0; i < nd && i < 8; ++i) dims[i] = (int64_t)d[i];
    const int n = (int)mxGetScalar(prhs[2]) - 1;
    if (nd < 2 || nd > 3 || n < 0 || n >= nd) mexErrMsgIdAndTxt("cmtf:hip:unsupported", "unfold_gram handles matrices and 3-way tensors");
    plhs[0] = mxCreateDoubleMatrix((mwSize)dims[n], (mwSize)dims[n], mxREAL);
    check(aoadmm_op_unfold_gram(g_ctx, mxGetDoubles(X), nd, dims, n, AOADMM_PREC_F64, mxGetDoubles(plhs[0])));
    return;
  }
  // U = aoadmm_mex('nvecs', X, n, r): the r leading left singular vectors of the mode-n unfolding (n 1-based) of an
  // sptensor or a sparse double matrix by subspace iteration on the device (aoadmm_resident_nvecs): no I_n x I_n
  // Gram matrix.  X goes up as a scratch one-block model, which replaces whatever model the context held.
  if (nrhs == 4 && mxIsChar(prhs[0])) {
    if (str(prhs[0]) != "nvecs") mexErrMsgIdAndTxt("cmtf:hip:usage", "unknown operation '%s'", str(prhs[0]).c_str());
    if (!is_sparse_object(prhs[1])) mexErrMsgIdAndTxt("cmtf:hip:unsupported", "nvecs handles sptensors and sparse double matrices (dense data: 'unfold_gram')");
    if (!g_ctx) {
      check(aoadmm_create(&g_ctx, 0));
      g_devices.assign(1, 0);
      if (!g_at_exit) { mexAtExit(at_exit); g_at_exit = true; }
    }
    std::vector<int64_t> subs;
    std::vector<double> vals, shape;
    read_sparse(0, prhs[1], -1, subs, vals, shape);
    const int N = (int)shape.size();
    const int n = (int)mxGetScalar(prhs[2]) - 1, r = (int)mxGetScalar(prhs[3]);
    if (N < 2 || N > 8 || n < 0 || n >= N) mexErrMsgIdAndTxt("cmtf:hip:invalid", "nvecs: mode %d of an order-%d object", n + 1, N);
    check(aoadmm_model_begin(g_ctx, N, 1, 0));
    std::vector<int> md(N);
    for (int m = 0; m < N; ++m) {
      md[m] = m;
      check(aoadmm_model_set_mode(g_ctx, m, (int64_t)shape[m], r));
    }
    check(aoadmm_model_add_cp(g_ctx, 0, N, md.data(), 1.0));
    for (int m = 0; m < N; ++m) check(aoadmm_model_set_coupling(g_ctx, m, -1, nullptr, 0, 0, nullptr, 0, 0));
    check(aoadmm_model_end(g_ctx));
    check(aoadmm_tensor_upload_coo(g_ctx, 0, (int64_t)vals.size(), subs.data(), vals.data()));
    const int64_t In = (int64_t)shape[n];
    plhs[0] = mxCreateDoubleMatrix((mwSize)In, (mwSize)r, mxREAL);
    aoadmm_nvecs_info info;
    check(aoadmm_resident_nvecs(g_ctx, 0, n, r, nullptr, mxGetDoubles(plhs[0]), In, nullptr, &info));
    if (!info.converged)
      mexWarnMsgIdAndTxt("cmtf:hip:nvecs", "nvecs of mode %d: subspace iteration stopped after %d iterations with residual %.3e",
                         n + 1, info.iterations, info.residual);
    return;
  }
  if (nrhs != 3 || nlhs > 2) mexErrMsgIdAndTxt("cmtf:hip:usage", "usage: [Fac,out] = aoadmm_mex(Z, G, options)");
  const mxArray *Z = prhs[0], *G = prhs[1], *opt = prhs[2];
  // options.hip.device = d (one GPU) or options.hip.devices = [d0 d1 ...] (several GPUs from this one MATLAB process:
  // aoadmm_create_multi, one engine + host thread per device inside the library, RCCL between them)
  std::vector<int> devices(1, 0);
  int precision = AOADMM_PREC_F64;
  bool sparse_sharding = false;                      // options.hip.sparse_sharding (default 0: sparse CP blocks replicated)
  // options.hip.sparse_observed_only: 0 (default), 1 = every sparse CP block, or a list of 1-based block numbers: the
  // unstored entries of those blocks are missing, not zero (aoadmm_tensor_set_observed_only)
  bool observed_all = false;
  std::vector<int> observed_list;
  const mxArray *entry_weights = nullptr, *unstored_weight = nullptr;
  if (const mxArray* hip = field(opt, "hip", false)) {
    if (const mxArray* f = field(hip, "sparse_sharding", false)) sparse_sharding = mxGetScalar(f) != 0;
    if (const mxArray* f = field(hip, "sparse_observed_only", false)) {
      if (mxIsCell(f) || mxIsEmpty(f))
        mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.sparse_observed_only must be 0, 1 or a list of block numbers");
      const mwSize ne = mxGetNumberOfElements(f);
      if (ne == 1 && mxGetScalar(f) <= 1) {           // the scalars 0 and 1; any other value names blocks
        observed_all = mxGetScalar(f) == 1;
      } else {
        if (!mxIsDouble(f)) mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.sparse_observed_only: a list of block numbers must be double");
        for (mwSize i = 0; i < ne; ++i) observed_list.push_back((int)mxGetDoubles(f)[i] - 1);
      }
    }
    // options.hip.sparse_entry_weights: a cell over the blocks, {p} = one weight in [0, 1] per stored entry of the sparse
    // CP block p or []; options.hip.sparse_unstored_weight: one number for all named blocks (those with weights and
    // those sparse_observed_only names), or a cell over the blocks of numbers or [].  A named block is observed-only.
    entry_weights = field(hip, "sparse_entry_weights", false);
    unstored_weight = field(hip, "sparse_unstored_weight", false);
    if (entry_weights && !mxIsCell(entry_weights))
      mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.sparse_entry_weights must be a cell over the blocks of Z.object");
    if (unstored_weight && !mxIsCell(unstored_weight) && !(mxIsDouble(unstored_weight) && mxGetNumberOfElements(unstored_weight) == 1))
      mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.sparse_unstored_weight must be one number or a cell over the blocks of Z.object");
    if ((entry_weights || unstored_weight) && sparse_sharding)
      mexErrMsgIdAndTxt("cmtf:hip:unsupported", "options.hip.sparse_entry_weights is not available together with options.hip.sparse_sharding");
    if ((observed_all || !observed_list.empty()) && sparse_sharding)
      mexErrMsgIdAndTxt("cmtf:hip:unsupported", "options.hip.sparse_observed_only is not available together with options.hip.sparse_sharding");
    if (const mxArray* d = field(hip, "device", false)) devices.assign(1, (int)mxGetScalar(d));
    if (const mxArray* d = field(hip, "devices", false)) {
      devices.clear();
      for (mwSize i = 0; i < mxGetNumberOfElements(d); ++i) devices.push_back((int)mxGetDoubles(d)[i]);
      if (devices.empty()) devices.assign(1, 0);
    }
    if (const mxArray* p = field(hip, "precision", false)) {
      const std::string ps = str(p);
      if (ps == "f64") precision = AOADMM_PREC_F64;
      else if (ps == "f32") precision = AOADMM_PREC_F32;
      else if (ps == "f16") precision = AOADMM_PREC_F16;
      else mexErrMsgIdAndTxt("aoadmm:precision", "options.hip.precision must be 'f64', 'f32' or 'f16', got '%s'", ps.c_str());
    }
  }
  if (g_ctx && devices != g_devices) {               // another device list: start over
    aoadmm_destroy(g_ctx);
    g_ctx = nullptr;
  }
  if (!g_ctx) {
    if (devices.size() == 1) check(aoadmm_create(&g_ctx, devices[0]));
    else check(aoadmm_create_multi(&g_ctx, (int)devices.size(), devices.data()));
    g_devices = devices;
    if (!g_at_exit) { mexAtExit(at_exit); g_at_exit = true; }
  }

  // ---- model: Z.size, Z.modes, Z.model, Z.weights, Z.coupling, Z.constraints (example_script1:74-89)
  const mxArray* sz = field(Z, "size");
  const mxArray* modes = field(Z, "modes");
  const mxArray* model = field(Z, "model");
  const mxArray* weights = field(Z, "weights");
  const mxArray* coupling = field(Z, "coupling");
  const mxArray* lin = field(coupling, "lin_coupled_modes");
  const mxArray* ctype = field(coupling, "coupling_type");
  const mxArray* trafo = field(coupling, "coupl_trafo_matrices");
  const mxArray* trafo2 = field(coupling, "coupl_trafo_matrices2", false);
  const mxArray* cmodes = field(Z, "constrained_modes");
  const mxArray* constraints = field(Z, "constraints");
  const mxArray* object = field(Z, "object");
  const mxArray* fac = field(G, "fac");
  const int n_modes = (int)mxGetNumberOfElements(sz);
  const int P = (int)mxGetNumberOfElements(object);
  const double* linv = mxGetDoubles(lin);
  int n_couplings = 0;
  for (int m = 0; m < n_modes; ++m) n_couplings = linv[m] > n_couplings ? (int)linv[m] : n_couplings;
  for (int p = 0; p < P; ++p)
    if (str(mxGetCell(field(Z, "loss_function"), p)) != "Frobenius")
      mexErrMsgIdAndTxt("cmtf:hip:unsupported", "non-Frobenius losses need the L-BFGS-B path of the MATLAB code");
  const mxArray* miss = field(Z, "miss", false);        // cmtf_fun_AOADMM_hip.m passes dense uint8 masks (1 = observed)
  bool has_missing = false;

  check(aoadmm_model_begin(g_ctx, n_modes, P, n_couplings));
  for (int m = 0; m < n_modes; ++m) {
    const mxArray* s = mxGetCell(sz, m);
    const mxArray* f = mxGetCell(fac, m);
    const int R = (int)mxGetN(mxIsCell(f) ? mxGetCell(f, 0) : f);
    if (mxGetNumberOfElements(s) > 1) {
      std::vector<int64_t> rows(mxGetNumberOfElements(s));
      for (size_t k = 0; k < rows.size(); ++k) rows[k] = (int64_t)mxGetDoubles(s)[k];
      check(aoadmm_model_set_mode_slabs(g_ctx, m, (int)rows.size(), rows.data(), R));
    } else {
      check(aoadmm_model_set_mode(g_ctx, m, (int64_t)mxGetScalar(s), R));
    }
  }
  for (int p = 0; p < P; ++p) {
    const mxArray* mp = mxGetCell(modes, p);
    std::vector<int> md(mxGetNumberOfElements(mp));
    for (size_t i = 0; i < md.size(); ++i) md[i] = (int)mxGetDoubles(mp)[i] - 1;
    const double w = mxGetDoubles(weights)[p];
    if (str(mxGetCell(model, p)) == "CP") check(aoadmm_model_add_cp(g_ctx, p, (int)md.size(), md.data(), w));
    else check(aoadmm_model_add_par2(g_ctx, p, md.data(), w));
  }
  for (int m = 0; m < n_modes; ++m) {
    if (mxGetDoubles(cmodes)[m] != 0) {
      const mxArray* c = mxGetCell(constraints, m);
      if (!c || mxIsEmpty(c)) mexErrMsgIdAndTxt("cmtf:hip:invalid", "No constraint provided for mode %d.", m + 1);
      const int id = constraint_id(str(mxGetCell(c, 0)));
      std::vector<double> par;
      const double* Lmat = nullptr;
      for (mwSize q = 1; q < mxGetNumberOfElements(c); ++q) {
        const mxArray* v = mxGetCell(c, q);
        if (id == AOADMM_C_QUADRATIC && q == 2) Lmat = mxGetDoubles(v);
        else par.push_back(mxGetScalar(v));
      }
      check(aoadmm_model_set_constraint(g_ctx, m, id, par.data(), (int)par.size(), Lmat));
    }
    const mxArray* H = mxGetCell(trafo, m);
    const mxArray* H2 = trafo2 ? mxGetCell(trafo2, m) : nullptr;
    const bool coupled = linv[m] > 0;
    check(aoadmm_model_set_coupling(g_ctx, m, (int)linv[m] - 1,
                                    coupled && H && !mxIsEmpty(H) ? mxGetDoubles(H) : nullptr, H ? (int64_t)mxGetM(H) : 0,
                                    H ? (int64_t)mxGetN(H) : 0,
                                    coupled && H2 && !mxIsEmpty(H2) ? mxGetDoubles(H2) : nullptr,
                                    H2 ? (int64_t)mxGetM(H2) : 0, H2 ? (int64_t)mxGetN(H2) : 0));
  }
  for (int c = 0; c < n_couplings; ++c) check(aoadmm_model_set_coupling_type(g_ctx, c, (int)mxGetDoubles(ctype)[c]));
  if (const mxArray* ridge = field(Z, "ridge", false)) check(aoadmm_model_set_ridge(g_ctx, mxGetDoubles(ridge)));
  check(aoadmm_model_end(g_ctx));

  // ---- data: Z.object{p}
  for (int p = 0; p < P; ++p) {
    const mxArray* obj = mxGetCell(object, p);
    bool sparse_slabs = false;
    if (mxIsCell(obj)) {                                  // PARAFAC2 slabs: all sparse matrices or all full ones
      mwSize nsp = 0;
      for (mwSize k = 0; k < mxGetNumberOfElements(obj); ++k) nsp += mxIsSparse(mxGetCell(obj, k)) ? 1 : 0;
      if (nsp != 0 && nsp != mxGetNumberOfElements(obj))
        mexErrMsgIdAndTxt("aoadmm:mixedSlabs", "Z.object{%d}: the slabs of a PARAFAC2 block must be all sparse or all full.", p + 1);
      sparse_slabs = nsp != 0;
    }
    if (sparse_slabs) {
      // compressed columns (ir / jc / values) of every slab -> 0-based (i, j, k), column-major nnz x 3, one transfer;
      // values stay fp64 whatever options.hip.precision says
      std::vector<int64_t> si, sj, sk;
      std::vector<double> vals;
      // shapes against Z.size, as the Python layer does: a slab with fewer rows or columns, or a surplus cell, would
      // otherwise go up silently as a differently shaped model
      const mxArray* mp = mxGetCell(modes, p);
      const int mA = (int)mxGetDoubles(mp)[0] - 1, mB = (int)mxGetDoubles(mp)[1] - 1;
      const mxArray* szB = mxGetCell(sz, mB);
      if (mxGetNumberOfElements(obj) != mxGetNumberOfElements(szB))
        mexErrMsgIdAndTxt("aoadmm:slabCount", "Z.object{%d} has %d slabs, Z.size says %d.", p + 1,
                          (int)mxGetNumberOfElements(obj), (int)mxGetNumberOfElements(szB));
      const double rowsA = mxGetScalar(mxGetCell(sz, mA));
      for (mwSize k = 0; k < mxGetNumberOfElements(obj); ++k) {
        const mxArray* xk = mxGetCell(obj, k);
        if (!mxIsDouble(xk) || mxIsComplex(xk))
          mexErrMsgIdAndTxt("aoadmm:sparseSlabType", "Z.object{%d}{%d} must be a real sparse double matrix.", p + 1, (int)k + 1);
        if ((double)mxGetM(xk) != rowsA || (double)mxGetN(xk) != mxGetDoubles(szB)[k])
          mexErrMsgIdAndTxt("aoadmm:slabSize", "Z.object{%d}{%d} has size [%d %d], Z.size says [%d %d].", p + 1, (int)k + 1,
                            (int)mxGetM(xk), (int)mxGetN(xk), (int)rowsA, (int)mxGetDoubles(szB)[k]);
        const mwIndex* jc = mxGetJc(xk);
        const mwIndex* ir = mxGetIr(xk);
        const double* v = mxGetDoubles(xk);
        for (mwSize j = 0; j < mxGetN(xk); ++j)
          for (mwIndex q = jc[j]; q < jc[j + 1]; ++q) {
            si.push_back((int64_t)ir[q]); sj.push_back((int64_t)j); sk.push_back((int64_t)k);
            vals.push_back(v[q]);
          }
      }
      std::vector<int64_t> subs;
      subs.reserve(3 * vals.size());
      subs.insert(subs.end(), si.begin(), si.end());
      subs.insert(subs.end(), sj.begin(), sj.end());
      subs.insert(subs.end(), sk.begin(), sk.end());
      check(aoadmm_par2_slab_upload_coo(g_ctx, p, (int64_t)vals.size(), subs.data(), vals.data()));
    } else if (mxIsCell(obj)) {
      if (std::find(observed_list.begin(), observed_list.end(), p) != observed_list.end())
        mexErrMsgIdAndTxt("cmtf:hip:unsupported", "options.hip.sparse_observed_only: Z.object{%d} is a PARAFAC2 block", p + 1);
      // shapes against Z.size, as for sparse slabs and as the Python layer does: the library reads I x sum(J_k) doubles
      // whatever the cells hold, so a short slab or a missing cell would be read past its end
      const mxArray* mp = mxGetCell(modes, p);
      const int mA = (int)mxGetDoubles(mp)[0] - 1, mB = (int)mxGetDoubles(mp)[1] - 1;
      const mxArray* szB = mxGetCell(sz, mB);
      if (mxGetNumberOfElements(obj) != mxGetNumberOfElements(szB))
        mexErrMsgIdAndTxt("aoadmm:slabCount", "Z.object{%d} has %d slabs, Z.size says %d.", p + 1,
                          (int)mxGetNumberOfElements(obj), (int)mxGetNumberOfElements(szB));
      const double rowsA = mxGetScalar(mxGetCell(sz, mA));
      std::vector<double> packed;                         // the slabs back to back, one transfer
      for (mwSize k = 0; k < mxGetNumberOfElements(obj); ++k) {
        const mxArray* xk = mxGetCell(obj, k);
        if (!xk || !mxIsDouble(xk) || mxIsComplex(xk))
          mexErrMsgIdAndTxt("cmtf:hip:unsupported", "Z.object{%d}{%d} is not a real double matrix: it stays on the MATLAB path", p + 1, (int)k + 1);
        if ((double)mxGetM(xk) != rowsA || (double)mxGetN(xk) != mxGetDoubles(szB)[k])
          mexErrMsgIdAndTxt("aoadmm:slabSize", "Z.object{%d}{%d} has size [%d %d], Z.size says [%d %d].", p + 1, (int)k + 1,
                            (int)mxGetM(xk), (int)mxGetN(xk), (int)rowsA, (int)mxGetDoubles(szB)[k]);
        packed.insert(packed.end(), mxGetDoubles(xk), mxGetDoubles(xk) + mxGetNumberOfElements(xk));
      }
      check(aoadmm_par2_slab_upload(g_ctx, p, AOADMM_ALL_SLABS, packed.data()));
    } else if (is_sparse_object(obj)) {
      const mxArray* mp = mxGetCell(modes, p);
      std::vector<int> md(mxGetNumberOfElements(mp));
      for (size_t i = 0; i < md.size(); ++i) md[i] = (int)mxGetDoubles(mp)[i] - 1;
      const bool marked = observed_all || std::find(observed_list.begin(), observed_list.end(), p) != observed_list.end();
      const mxArray* wp = entry_weights && (mwSize)p < mxGetNumberOfElements(entry_weights) ? mxGetCell(entry_weights, p) : nullptr;
      const mxArray* ap = unstored_weight && mxIsCell(unstored_weight)
                              ? ((mwSize)p < mxGetNumberOfElements(unstored_weight) ? mxGetCell(unstored_weight, p) : nullptr)
                              : nullptr;
      const bool has_w = wp && !mxIsEmpty(wp), has_a = ap && !mxIsEmpty(ap);
      const bool scalar_a = unstored_weight && !mxIsCell(unstored_weight);
      const bool weighted = has_w || has_a || (scalar_a && marked);
      const double alpha = has_a ? mxGetScalar(ap) : (scalar_a && weighted ? mxGetScalar(unstored_weight) : 0.0);
      upload_sparse(p, obj, sz, md, sparse_sharding, weighted, wp, alpha);    // values stay fp64 whatever options.hip.precision says
      if (marked || weighted) {
        check(aoadmm_tensor_set_observed_only(g_ctx, p, 1));
        has_missing = true;                               // out.func_rel_missing and the display column as for Z.miss
      }
    } else {
      if (std::find(observed_list.begin(), observed_list.end(), p) != observed_list.end())
        mexErrMsgIdAndTxt("cmtf:hip:unsupported", "options.hip.sparse_observed_only: Z.object{%d} is dense (use Z.miss)", p + 1);
      // 'f16': dense 3-way blocks without Z.miss are stored fp16 (AOADMM_PREC_F16), every other dense block fp32
      int prec_p = precision;
      if (precision == AOADMM_PREC_F16) {
        const mxArray* mkp = (miss && !mxIsEmpty(miss) && (mwSize)p < mxGetNumberOfElements(miss)) ? mxGetCell(miss, p) : nullptr;
        if (mxGetNumberOfElements(mxGetCell(modes, p)) != 3 || (mkp && !mxIsEmpty(mkp))) prec_p = AOADMM_PREC_F32;
      }
      // the shape against Z.size, as for a sparse block and as the Python layer does: the library reads prod(Z.size of
      // the block's modes) doubles whatever the array holds
      const mxArray* data = dense_data(obj);
      const mxArray* mp = mxGetCell(modes, p);
      const mwSize N = mxGetNumberOfElements(mp), nd = mxGetNumberOfDimensions(data);
      bool same = !mxIsComplex(data);
      for (mwSize i = 0; same && i < (N > nd ? N : nd); ++i) {   // trailing singleton dimensions are not stored
        const double want = i < N ? mxGetScalar(mxGetCell(sz, (mwIndex)mxGetDoubles(mp)[i] - 1)) : 1.0;
        same = (i < nd ? (double)mxGetDimensions(data)[i] : 1.0) == want;
      }
      if (!same) mexErrMsgIdAndTxt("cmtf:hip:invalid", "Z.object{%d}: size does not match Z.size of its modes", p + 1);
      check(aoadmm_tensor_upload(g_ctx, p, mxGetDoubles(data), prec_p));
    }
    // Z.miss{p} (cmtf_AOADMM.m:68-121): same shape as the data, uint8
    const mxArray* mk = (miss && !mxIsEmpty(miss) && (mwSize)p < mxGetNumberOfElements(miss)) ? mxGetCell(miss, p) : nullptr;
    if (mk && !mxIsEmpty(mk)) {
      has_missing = true;
      if (is_sparse_object(obj))                          // cmtf_AOADMM.m:77-79
        mexErrMsgIdAndTxt("cmtf:missingData:sptensor", "Missing data (Z.miss) not supported for sptensor objects. Convert to tensor first.");
      if (sparse_slabs)
        mexErrMsgIdAndTxt("cmtf:missingData:sparseSlabs", "Missing data (Z.miss) not supported for sparse PARAFAC2 slabs. Convert to full slabs first.");
      if (mxIsCell(obj)) {
        if (!mxIsCell(mk) || mxGetNumberOfElements(mk) != mxGetNumberOfElements(obj))
          mexErrMsgIdAndTxt("cmtf:missingData:PAR2maskNotCell", "Z.miss{%d} must be a cell array of length %d for PAR2.", p + 1,
                            (int)mxGetNumberOfElements(obj));
        for (mwSize k = 0; k < mxGetNumberOfElements(obj); ++k) {
          const mxArray* mkk = mxGetCell(mk, k);
          if (!mxIsUint8(mkk) || mxGetNumberOfElements(mkk) != mxGetNumberOfElements(mxGetCell(obj, k)))
            mexErrMsgIdAndTxt("cmtf:missingData:PAR2maskSliceSizeMismatch", "Z.miss{%d}{%d} size does not match Z.object{%d}{%d}.",
                              p + 1, (int)k + 1, p + 1, (int)k + 1);
          check(aoadmm_par2_slab_mask_upload(g_ctx, p, (int)k, static_cast<const uint8_t*>(mxGetData(mkk))));
        }
      } else {
        if (!mxIsUint8(mk) || mxGetNumberOfElements(mk) != mxGetNumberOfElements(dense_data(obj)))
          mexErrMsgIdAndTxt("cmtf:missingData:maskSizeMismatch", "Z.miss{%d} size does not match Z.object{%d}.", p + 1, p + 1);
        check(aoadmm_tensor_mask_upload(g_ctx, p, static_cast<const uint8_t*>(mxGetData(mk))));
      }
    }
  }

  // ---- options.hip.heldout: a cell per block of a struct with `subs` (n x N, 1-based as MATLAB has them; a PARAFAC2
  // block: i, j within slab k, k) and `vals` (n): entries kept out of the fit, scored on the device with every
  // evaluation of the objective (aoadmm_tensor_set_heldout).  Empty cells and blocks beyond the cell have no list.
  std::vector<char> has_list(P, 0);
  if (const mxArray* hip = field(opt, "hip", false))
    if (const mxArray* ho = field(hip, "heldout", false)) {
      if (!mxIsCell(ho) || mxGetNumberOfElements(ho) > (mwSize)P)
        mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.heldout must be a cell with at most one entry per block of Z.object");
      for (mwSize p = 0; p < mxGetNumberOfElements(ho); ++p) {
        const mxArray* e = mxGetCell(ho, p);
        if (!e || mxIsEmpty(e)) continue;
        if (!mxIsStruct(e)) mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.heldout{%d} must be a struct with subs and vals", (int)p + 1);
        const mxArray* hs = field(e, "subs");
        const mxArray* hv = field(e, "vals");
        const mwSize N = mxGetNumberOfElements(mxGetCell(modes, p));
        const mwSize n = mxGetNumberOfElements(hv);
        if (!mxIsDouble(hs) || !mxIsDouble(hv) || mxIsComplex(hv) || mxGetM(hs) != n || mxGetN(hs) != N)
          mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.heldout{%d}: subs must be a double n x %d array and vals n real doubles",
                            (int)p + 1, (int)N);
        if (n == 0) continue;
        std::vector<int64_t> s0((size_t)n * N);              // column-major n x N as subs is; 1-based -> 0-based
        const double* sd = mxGetDoubles(hs);
        for (size_t i = 0; i < s0.size(); ++i) {
          if (sd[i] != std::floor(sd[i]))
            mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.heldout{%d}: subscripts must be integers", (int)p + 1);
          s0[i] = (int64_t)sd[i] - 1;
        }
        check(aoadmm_tensor_set_heldout(g_ctx, (int)p, (int64_t)n, s0.data(), mxGetDoubles(hv)));   // range and NaN: the library
        has_list[p] = 1;
      }
    }

  // ---- options.hip.rank_lists: a cell per block of a struct with `mode` (1-based position in the block), `subs` (nq x N,
  // 1-based; column `mode` holds the target row) and optionally `excl_off` (nq + 1 offsets from 0) with `excl_idx` (1-based
  // rows): ranking metrics of held-out rows, evaluated on the device beside the objective (aoadmm_tensor_set_ranklist).
  // options.hip.rank_metric ('ndcg@10', 'hit@5', 'mrr', 'auc'), rank_every, rank_patience, rank_criterion: aoadmm_rank_track.
  std::vector<char> has_rank(P, 0);
  int rank_criterion = 0;
  if (const mxArray* hip = field(opt, "hip", false)) {
    if (const mxArray* rl = field(hip, "rank_lists", false)) {
      if (!mxIsCell(rl) || mxGetNumberOfElements(rl) > (mwSize)P)
        mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_lists must be a cell with at most one entry per block of Z.object");
      for (mwSize p = 0; p < mxGetNumberOfElements(rl); ++p) {
        const mxArray* e = mxGetCell(rl, p);
        if (!e || mxIsEmpty(e)) continue;
        if (!mxIsStruct(e)) mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_lists{%d} must be a struct with mode and subs", (int)p + 1);
        const mxArray* rs = field(e, "subs");
        const mwSize N = mxGetNumberOfElements(mxGetCell(modes, p));
        const mwSize nq = mxGetM(rs);
        if (!mxIsDouble(rs) || mxGetN(rs) != N)
          mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_lists{%d}: subs must be a double nq x %d array", (int)p + 1, (int)N);
        if (nq == 0) continue;
        auto ints = [&](const mxArray* a, double shift, const char* what) {
          std::vector<int64_t> v(mxGetNumberOfElements(a));
          const double* d = mxGetDoubles(a);
          for (size_t i = 0; i < v.size(); ++i) {
            if (d[i] != std::floor(d[i]))
              mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_lists{%d}: %s must hold integers", (int)p + 1, what);
            v[i] = (int64_t)d[i] - (int64_t)shift;
          }
          return v;
        };
        const std::vector<int64_t> s0 = ints(rs, 1.0, "subs");   // column-major nq x N as subs is; 1-based -> 0-based
        std::vector<int64_t> eo, ei;
        const mxArray* xo = field(e, "excl_off", false);
        const mxArray* xi = field(e, "excl_idx", false);
        if (xo && !mxIsEmpty(xo)) {
          if (!mxIsDouble(xo) || mxGetNumberOfElements(xo) != nq + 1 || (xi && !mxIsDouble(xi)))
            mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_lists{%d}: excl_off must hold nq + 1 offsets and excl_idx doubles", (int)p + 1);
          eo = ints(xo, 0.0, "excl_off");
          if (xi) ei = ints(xi, 1.0, "excl_idx");
          if (eo.back() != (int64_t)ei.size())
            mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_lists{%d}: excl_off ends at %lld, excl_idx holds %lld rows", (int)p + 1,
                              (long long)eo.back(), (long long)ei.size());
          if (ei.empty()) ei.push_back(0);                     // a valid address for an empty list
        }
        check(aoadmm_tensor_set_ranklist(g_ctx, (int)p, (int)scalar(e, "mode") - 1, (int64_t)nq, s0.data(), eo.empty() ? nullptr : eo.data(),
                                         eo.empty() ? nullptr : ei.data()));   // ranges: the library
        has_rank[p] = 1;
      }
    }
    int metric = AOADMM_RANK_NDCG, rk = 10, every = 1, patience = 0;
    bool given = false;
    if (const mxArray* f = field(hip, "rank_metric", false)) {
      if (!mxIsChar(f)) mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_metric must be a string such as 'ndcg@10', 'hit@5', 'mrr' or 'auc'");
      const std::string spec = str(f);
      const size_t at = spec.find('@');
      const std::string name = spec.substr(0, at);
      if (name == "hit") metric = AOADMM_RANK_HIT;
      else if (name == "ndcg") metric = AOADMM_RANK_NDCG;
      else if (name == "mrr") metric = AOADMM_RANK_MRR;
      else if (name == "auc") metric = AOADMM_RANK_AUC;
      else mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_metric '%s': the metric must be hit, ndcg, mrr or auc", spec.c_str());
      if (at != std::string::npos) {
        const std::string ktxt = spec.substr(at + 1);
        if ((metric != AOADMM_RANK_HIT && metric != AOADMM_RANK_NDCG) || ktxt.empty() || ktxt.size() > 10 ||
            ktxt.find_first_not_of("0123456789") != std::string::npos || std::stoll(ktxt) < 1 || std::stoll(ktxt) >= (1LL << 31))
          mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.rank_metric '%s': the cut-off must be an integer in [1, 2^31) after hit or ndcg", spec.c_str());
        rk = (int)std::stoll(ktxt);
      }
      given = true;
    }
    if (const mxArray* f = field(hip, "rank_every", false)) { every = (int)mxGetScalar(f); given = true; }
    if (const mxArray* f = field(hip, "rank_patience", false)) { patience = (int)mxGetScalar(f); given = true; }
    if (const mxArray* f = field(hip, "rank_criterion", false)) { rank_criterion = (int)mxGetScalar(f); given = true; }
    const bool any_rank = std::find(has_rank.begin(), has_rank.end(), 1) != has_rank.end();
    if (given || any_rank) check(aoadmm_rank_track(g_ctx, metric, rk, every, patience, rank_criterion));   // ranges and combinations: the library
  }

  // ---- state: the struct G (init_coupled_AOADMM_CMTF.m:41-45)
  for (int m = 0; m < n_modes; ++m) {
    put_state_maybe_cell(AOADMM_F_FAC, m, mxGetCell(fac, m));
    if (const mxArray* f = field(G, "constraint_fac", false)) put_state_maybe_cell(AOADMM_F_CONSTRAINT_FAC, m, mxGetCell(f, m));
    if (const mxArray* f = field(G, "constraint_dual_fac", false)) put_state_maybe_cell(AOADMM_F_CONSTRAINT_DUAL, m, mxGetCell(f, m));
    if (const mxArray* f = field(G, "coupling_dual_fac", false)) put_state_maybe_cell(AOADMM_F_COUPLING_DUAL, m, mxGetCell(f, m));
  }
  if (const mxArray* f = field(G, "coupling_fac", false))
    for (int c = 0; c < n_couplings; ++c) put_state(AOADMM_F_COUPLING_FAC, c, 0, mxGetCell(f, c));
  for (int p = 0; p < P; ++p) {
    if (const mxArray* f = field(G, "DeltaB", false))
      if ((mwSize)p < mxGetNumberOfElements(f)) put_state(AOADMM_F_DELTAB, p, 0, mxGetCell(f, p));
    if (const mxArray* f = field(G, "P", false))
      if ((mwSize)p < mxGetNumberOfElements(f)) put_state_maybe_cell(AOADMM_F_P, p, mxGetCell(f, p));
    if (const mxArray* f = field(G, "mu_DeltaB", false))
      if ((mwSize)p < mxGetNumberOfElements(f)) put_state_maybe_cell(AOADMM_F_MU_DELTAB, p, mxGetCell(f, p));
  }

  // ---- options (example_script1_CP_PAR2_nonneg.m:110-123; missing fields error like MATLAB)
  aoadmm_options o;
  std::memset(&o, 0, sizeof o);
  o.MaxOuterIters = (int)scalar(opt, "MaxOuterIters");
  o.MaxInnerIters = (int)scalar(opt, "MaxInnerIters");
  o.AbsFuncTol = scalar(opt, "AbsFuncTol");
  o.OuterRelTol = scalar(opt, "OuterRelTol");
  o.innerRelPrTol_coupl = scalar(opt, "innerRelPrTol_coupl");
  o.innerRelPrTol_constr = scalar(opt, "innerRelPrTol_constr");
  o.innerRelDualTol_coupl = scalar(opt, "innerRelDualTol_coupl");
  o.innerRelDualTol_constr = scalar(opt, "innerRelDualTol_constr");
  o.bsum = scalar(opt, "bsum") != 0;
  if (o.bsum) o.bsum_weight = scalar(opt, "bsum_weight");
  if (const mxArray* f = field(opt, "iter_start_PAR2Bkconstraint", false)) o.iter_start_PAR2Bkconstraint = (int)mxGetScalar(f);
  if (const mxArray* f = field(opt, "increase_factor_rhoBk", false)) {
    o.has_increase_factor_rhoBk = 1;
    o.increase_factor_rhoBk = mxGetScalar(f);
  }
  o.use_dimtree = 1;
  if (const mxArray* hip = field(opt, "hip", false)) {
    if (const mxArray* f = field(hip, "no_permuted_copy", false)) o.no_permuted_copy = (int)mxGetScalar(f);
    if (const mxArray* f = field(hip, "par2_slab_sharding", false)) o.par2_slab_sharding = (int)mxGetScalar(f);
    if (const mxArray* f = field(hip, "heldout_patience", false)) o.heldout_patience = (int)mxGetScalar(f);
  }
  // ---- options.hip.heldout_keep_best = 1: Fac is the iterate with the smallest weighted held-out sum, not the last one
  // (aoadmm_heldout_keep_best / aoadmm_heldout_restore_best).  The switch belongs to the model, which was just built.
  bool keep_best = false;
  if (const mxArray* hip = field(opt, "hip", false))
    if (const mxArray* f = field(hip, "heldout_keep_best", false)) {
      const double v = mxIsChar(f) || mxIsEmpty(f) ? -1.0 : mxGetScalar(f);
      if (mxGetNumberOfElements(f) != 1 || (v != 0.0 && v != 1.0))
        mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.heldout_keep_best must be 0 or 1");
      keep_best = v == 1.0;
      const std::vector<char>& serves = rank_criterion == 1 ? has_rank : has_list;   // rank_criterion = 1: the best ranking score is kept
      if (keep_best && std::find(serves.begin(), serves.end(), 1) == serves.end())
        mexErrMsgIdAndTxt("cmtf:hip:invalid", "options.hip.heldout_keep_best = 1 needs a held-out list (options.hip.heldout)");
    }
  if (keep_best) check(aoadmm_heldout_keep_best(g_ctx, 1));

  // ---- solve
  const int n = o.MaxOuterIters + 1;
  std::vector<double> fv(n), fc(n), fz(n), fp(n), tt(n), frm(n), inner((size_t)n_modes * (o.MaxOuterIters > 0 ? o.MaxOuterIters : 1));
  aoadmm_result res;
  std::memset(&res, 0, sizeof res);
  res.func_val_conv = fv.data(); res.func_coupl_conv = fc.data(); res.func_constr_conv = fz.data();
  res.func_PAR2_coupl = fp.data(); res.time_at_it = tt.data(); res.innerIters = inner.data();
  res.func_rel_missing = frm.data();
  // options.Display = 'iter': one table row every DisplayIters iterations, live (cmtf_fun_AOADMM.m:53-59, :462-468)
  ProgressState ps;
  ps.has_missing = has_missing;
  const mxArray* disp = field(opt, "Display", false);
  const bool live = disp && mxIsChar(disp) && str(disp) == "iter";
  if (live) {
    const mxArray* di = field(opt, "DisplayIters", false);
    check(aoadmm_set_progress(g_ctx, &print_progress, &ps, di ? (int)mxGetScalar(di) : 10));
  }
  const int rc = aoadmm_solve(g_ctx, &o, &res);
  if (live) (void)aoadmm_set_progress(g_ctx, nullptr, nullptr, 0);
  check(rc);
  int restored_iter = -1;
  if (keep_best) check(aoadmm_heldout_restore_best(g_ctx, &restored_iter));   // before the state is read: Fac is the best iterate

  // ---- Fac: same fields as G (cmtf_AOADMM.m:193,197-206)
  plhs[0] = mxDuplicateArray(G);
  mxArray* Fac = plhs[0];
  for (int m = 0; m < n_modes; ++m) {
    replace_cell(mxGetField(Fac, 0, "fac"), m, get_like(AOADMM_F_FAC, m, mxGetCell(fac, m)));
    const char* names[3] = {"constraint_fac", "constraint_dual_fac", "coupling_dual_fac"};
    const int ids[3] = {AOADMM_F_CONSTRAINT_FAC, AOADMM_F_CONSTRAINT_DUAL, AOADMM_F_COUPLING_DUAL};
    for (int q = 0; q < 3; ++q)
      if (mxArray* f = mxGetField(Fac, 0, names[q])) {
        const mxArray* ref = mxGetCell(f, m);
        if (ref && !mxIsEmpty(ref)) replace_cell(f, m, get_like(ids[q], m, ref));
      }
  }
  if (mxArray* f = mxGetField(Fac, 0, "coupling_fac"))
    for (int c = 0; c < n_couplings; ++c) replace_cell(f, c, get_like(AOADMM_F_COUPLING_FAC, c, mxGetCell(f, c)));
  for (int p = 0; p < P; ++p) {
    const char* names[3] = {"DeltaB", "P", "mu_DeltaB"};
    const int ids[3] = {AOADMM_F_DELTAB, AOADMM_F_P, AOADMM_F_MU_DELTAB};
    for (int q = 0; q < 3; ++q)
      if (mxArray* f = mxGetField(Fac, 0, names[q]))
        if ((mwSize)p < mxGetNumberOfElements(f)) {
          const mxArray* ref = mxGetCell(f, p);
          if (ref && !mxIsEmpty(ref)) replace_cell(f, p, get_like(ids[q], p, ref));
        }
  }

  // ---- out (cmtf_fun_AOADMM.m:480-494)
  if (nlhs > 1) {
    std::vector<const char*> fn = {"f_tensors", "f_couplings", "f_constraints", "f_PAR2_couplings", "f_rel_missing", "exit_flag",
                                   "OuterIterations", "func_val_conv", "func_coupl_conv", "func_constr_conv", "func_PAR2_coupl",
                                   "time_at_it", "innerIters"};
    if (has_missing) fn.push_back("func_rel_missing");                     /* only with Z.miss (:490-492) */
    const bool any_list = std::find(has_list.begin(), has_list.end(), 1) != has_list.end();
    if (any_list) { fn.push_back("func_heldout"); fn.push_back("heldout_best_iter"); }   /* only with options.hip.heldout */
    if (keep_best) fn.push_back("heldout_restored_iter");                  /* only with options.hip.heldout_keep_best */
    const bool any_rank = std::find(has_rank.begin(), has_rank.end(), 1) != has_rank.end();
    if (any_rank) { fn.push_back("rank_trace"); fn.push_back("rank_best_iter"); }        /* only with options.hip.rank_lists */
    mxArray* out = mxCreateStructMatrix(1, 1, (int)fn.size(), fn.data());
    const int it = res.OuterIterations;
    auto vec = [&](const std::vector<double>& v, int len) {
      mxArray* a = mxCreateDoubleMatrix(1, len, mxREAL);
      std::memcpy(mxGetDoubles(a), v.data(), sizeof(double) * len);
      return a;
    };
    mxSetField(out, 0, "f_tensors", mxCreateDoubleScalar(res.f_tensors));
    mxSetField(out, 0, "f_couplings", mxCreateDoubleScalar(res.f_couplings));
    mxSetField(out, 0, "f_constraints", mxCreateDoubleScalar(res.f_constraints));
    mxSetField(out, 0, "f_PAR2_couplings", mxCreateDoubleScalar(res.f_PAR2_couplings));
    mxSetField(out, 0, "f_rel_missing", mxCreateDoubleScalar(has_missing ? res.f_rel_missing : mxGetNaN()));
    if (has_missing) mxSetField(out, 0, "func_rel_missing", vec(frm, it + 1));
    if (any_list) {
      // out.func_heldout{p}: sum (y - m)^2 of block p's list at iteration 0 .. OuterIterations; out.heldout_best_iter: the
      // iteration of the smallest weighted sum.  Fac holds the LAST iteration unless options.hip.heldout_keep_best = 1
      mxArray* fh = mxCreateCellMatrix(1, P);
      int best = -1;
      for (int p = 0; p < P; ++p) {
        if (!has_list[p]) continue;
        std::vector<double> tr(it + 1);
        int len = 0;
        check(aoadmm_heldout_trace(g_ctx, p, tr.data(), it + 1, &len, &best));
        mxSetCell(fh, p, vec(tr, len < it + 1 ? len : it + 1));
      }
      mxSetField(out, 0, "func_heldout", fh);
      mxSetField(out, 0, "heldout_best_iter", mxCreateDoubleScalar(best));
    }
    if (keep_best) mxSetField(out, 0, "heldout_restored_iter", mxCreateDoubleScalar(restored_iter));
    if (any_rank) {
      // out.rank_trace{p}: per evaluation of block p's ranking list the iteration, the counts n and n_auc, the means hit,
      // ndcg, mrr (over n) and auc (over n_auc; NaN over nothing) and the raw sums; out.rank_best_iter: the iteration of
      // the best pooled score
      const char* rf[] = {"iters", "n", "n_auc", "hit", "ndcg", "mrr", "auc", "hits", "ndcg_sum", "mrr_sum", "auc_sum"};
      mxArray* rt = mxCreateCellMatrix(1, P);
      int best = -1;
      for (int p = 0; p < P; ++p) {
        if (!has_rank[p]) continue;
        int len = 0;
        check(aoadmm_rank_trace(g_ctx, p, AOADMM_RANKSUM_N, nullptr, 0, &len, nullptr, &best));
        std::vector<int> iters((size_t)len + 1);
        std::vector<std::vector<double>> sums(AOADMM_RANKSUM_COUNT, std::vector<double>((size_t)len + 1));
        for (int w = 0; w < AOADMM_RANKSUM_COUNT; ++w) check(aoadmm_rank_trace(g_ctx, p, w, sums[w].data(), len, nullptr, iters.data(), nullptr));
        mxArray* st = mxCreateStructMatrix(1, 1, 11, rf);
        std::vector<double> itd(iters.begin(), iters.end());
        mxSetField(st, 0, "iters", vec(itd, len));
        mxSetField(st, 0, "n", vec(sums[AOADMM_RANKSUM_N], len));
        mxSetField(st, 0, "n_auc", vec(sums[AOADMM_RANKSUM_N_AUC], len));
        auto mean = [&](int num, int den) {
          std::vector<double> m((size_t)len + 1);
          for (int e = 0; e < len; ++e) m[e] = sums[den][e] > 0 ? sums[num][e] / sums[den][e] : mxGetNaN();
          return vec(m, len);
        };
        mxSetField(st, 0, "hit", mean(AOADMM_RANKSUM_HITS, AOADMM_RANKSUM_N));
        mxSetField(st, 0, "ndcg", mean(AOADMM_RANKSUM_NDCG, AOADMM_RANKSUM_N));
        mxSetField(st, 0, "mrr", mean(AOADMM_RANKSUM_MRR, AOADMM_RANKSUM_N));
        mxSetField(st, 0, "auc", mean(AOADMM_RANKSUM_AUC, AOADMM_RANKSUM_N_AUC));
        mxSetField(st, 0, "hits", vec(sums[AOADMM_RANKSUM_HITS], len));
        mxSetField(st, 0, "ndcg_sum", vec(sums[AOADMM_RANKSUM_NDCG], len));
        mxSetField(st, 0, "mrr_sum", vec(sums[AOADMM_RANKSUM_MRR], len));
        mxSetField(st, 0, "auc_sum", vec(sums[AOADMM_RANKSUM_AUC], len));
        mxSetCell(rt, p, st);
      }
      mxSetField(out, 0, "rank_trace", rt);
      mxSetField(out, 0, "rank_best_iter", mxCreateDoubleScalar(best));
    }
    if (res.exit_code == 0) {
      mxSetField(out, 0, "exit_flag", mxCreateString("maxIterations"));      /* make_exit_flag.m:4-5 */
    } else if (res.exit_code == 2) {
      mxSetField(out, 0, "exit_flag", mxCreateString("heldoutPatience"));    /* options.hip.heldout_patience */
    } else if (res.exit_code == 3) {
      mxSetField(out, 0, "exit_flag", mxCreateString("rankPatience"));       /* options.hip.rank_patience */
    } else {
      const char* q[] = {"f_tensors", "f_couplings", "f_constraints", "f_PAR2_couplings"};
      mxArray* ef = mxCreateStructMatrix(1, 1, 4, q);
      for (int i = 0; i < 4; ++i) mxSetField(ef, 0, q[i], mxCreateString(res.exit_abs[i] ? "AbsFuncTol" : "RelFuncTol"));
      mxSetField(out, 0, "exit_flag", ef);
    }
    mxSetField(out, 0, "OuterIterations", mxCreateDoubleScalar(it));
    mxSetField(out, 0, "func_val_conv", vec(fv, it + 1));
    mxSetField(out, 0, "func_coupl_conv", vec(fc, it + 1));
    mxSetField(out, 0, "func_constr_conv", vec(fz, it + 1));
    mxSetField(out, 0, "func_PAR2_coupl", vec(fp, it + 1));
    mxSetField(out, 0, "time_at_it", vec(tt, it + 1));
    mxArray* ii = mxCreateDoubleMatrix(n_modes, it > 0 ? it : 1, mxREAL);
    std::memcpy(mxGetDoubles(ii), inner.data(), sizeof(double) * n_modes * (it > 0 ? it : 1));
    mxSetField(out, 0, "innerIters", ii);
    plhs[1] = out;
  }
}
