/*
 * mxmock.cpp -- a functional mock of the part of MATLAB's C Matrix API that the MEX gateway uses: every function
 * declared in matlab-code_amd/mex/mex_stub/mex.h, written from the documented behaviour of the API, plus the test-only
 * entry points of mxmock.h.  It lets the gateway's logic run without MATLAB: linked with aoadmm_mex.cpp and either
 * libaoadmm_hip.so or the recording fake (fake_aoadmm.cpp).
 *
 * Where MATLAB's behaviour is undefined (a crash, garbage) the mock is strict: it throws Misuse, which mxmock_call
 * reports as "mxmock:misuse" with a text of its own per case, so that a test fails instead of reading something
 * plausible.  Destroyed arrays keep their header until mxmock_free_all so that a use after mxDestroyArray is seen.
 */
#include "mxmock.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <pthread.h>
#include <string>
#include <vector>

struct mxArray_tag {
  int kind = MXMOCK_DOUBLE;
  bool sparse = false, cplx = false, alive = true;
  std::vector<mwSize> dims;
  std::vector<double> d;             // double values (full: all elements; sparse: the stored ones)
  std::vector<uint8_t> b;            // uint8 / logical
  std::vector<float> f;              // single
  std::string chars;                 // char
  std::vector<mxArray*> kids;        // cell elements, struct field values, object property values (may be null)
  std::vector<std::string> names;    // struct fields / object properties, in order
  std::string cls;                   // object class
  std::vector<mwIndex> ir, jc;
  mxArray* parent = nullptr;
  bool displaced = false;            // mxSetCell / mxSetField put another value in its place
};

namespace {

struct Misuse { std::string text; };
struct MexError { std::string id, text; };

std::vector<mxArray*> g_all;
std::vector<mxArray*> g_call_created;
bool g_in_call = false;
std::vector<void (*)(void)> g_at_exit;
int g_at_exit_calls = 0;
int64_t g_orphans = 0;
std::mutex g_out_mutex;
struct Printed { std::string text; uint64_t thread; };
std::vector<Printed> g_printed;
std::vector<std::string> g_evals;
std::vector<std::pair<std::string, std::string>> g_warns;
uint64_t g_call_thread = 0;
std::string g_err_id, g_err_msg;

uint64_t this_thread() { return (uint64_t)pthread_self(); }

[[noreturn]] void misuse(const std::string& t) { throw Misuse{t}; }

const mxArray* chk(const mxArray* a, const char* fn) {
  if (!a) misuse(std::string(fn) + ": null mxArray");
  if (!a->alive) misuse(std::string(fn) + ": use after mxDestroyArray");
  return a;
}

mxArray* make(int kind, std::vector<mwSize> dims) {
  mxArray* a = new mxArray_tag;
  a->kind = kind;
  a->dims = std::move(dims);
  g_all.push_back(a);
  if (g_in_call) g_call_created.push_back(a);
  return a;
}

size_t numel(const mxArray* a) {
  size_t n = 1;
  for (mwSize v : a->dims) n *= v;
  return n;
}

void kill(mxArray* a) {
  if (!a || !a->alive) return;
  a->alive = false;
  for (mxArray* k : a->kids) kill(k);
}

mxArray* dup(const mxArray* a) {
  if (!a) return nullptr;
  mxArray* c = make(a->kind, a->dims);
  c->sparse = a->sparse; c->cplx = a->cplx; c->d = a->d; c->b = a->b; c->f = a->f; c->chars = a->chars;
  c->names = a->names; c->cls = a->cls; c->ir = a->ir; c->jc = a->jc;
  for (const mxArray* k : a->kids) {
    mxArray* kc = dup(k);
    if (kc) kc->parent = c;
    c->kids.push_back(kc);
  }
  return c;
}

void adopt(mxArray* owner, mxArray*& slot, mxArray* value, const char* fn) {
  if (value) {
    chk(value, fn);
    if (value->parent) misuse(std::string(fn) + ": the value already belongs to another array");
    if (value == owner) misuse(std::string(fn) + ": an array cannot hold itself");
    value->parent = owner;
  }
  if (slot) {                                // MATLAB does not free the element it replaces: it is an orphan now,
    slot->parent = nullptr;                  // the caller's to destroy (mxmock_orphans counts those it did not)
    slot->displaced = true;
  }
  slot = value;
}

std::string vformat(const char* fmt, va_list ap) {
  va_list ap2;
  va_copy(ap2, ap);
  const int n = vsnprintf(nullptr, 0, fmt, ap2);
  va_end(ap2);
  std::string s(n > 0 ? (size_t)n : 0, '\0');
  if (n > 0) vsnprintf(&s[0], (size_t)n + 1, fmt, ap);
  return s;
}

}  // namespace

extern "C" {

/* ---- type queries ----------------------------------------------------------------------------------------------- */
bool mxIsStruct(const mxArray* a) { return chk(a, "mxIsStruct")->kind == MXMOCK_STRUCT; }
bool mxIsCell(const mxArray* a) { return chk(a, "mxIsCell")->kind == MXMOCK_CELL; }
bool mxIsDouble(const mxArray* a) { return chk(a, "mxIsDouble")->kind == MXMOCK_DOUBLE; }
bool mxIsChar(const mxArray* a) { return chk(a, "mxIsChar")->kind == MXMOCK_CHAR; }
bool mxIsUint8(const mxArray* a) { return chk(a, "mxIsUint8")->kind == MXMOCK_UINT8; }
bool mxIsSparse(const mxArray* a) { return chk(a, "mxIsSparse")->sparse; }
bool mxIsComplex(const mxArray* a) { return chk(a, "mxIsComplex")->cplx; }
bool mxIsEmpty(const mxArray* a) { return numel(chk(a, "mxIsEmpty")) == 0; }
bool mxIsClass(const mxArray* a, const char* name) {
  chk(a, "mxIsClass");
  static const char* builtin[] = {"double", "uint8", "char", "logical", "single", "cell", "struct"};
  if (a->kind == MXMOCK_OBJECT) return a->cls == name;
  return std::strcmp(builtin[a->kind], name) == 0;
}

/* ---- shape ------------------------------------------------------------------------------------------------------ */
size_t mxGetM(const mxArray* a) { return chk(a, "mxGetM")->dims[0]; }
size_t mxGetN(const mxArray* a) {
  chk(a, "mxGetN");
  size_t n = 1;
  for (size_t i = 1; i < a->dims.size(); ++i) n *= a->dims[i];
  return n;
}
size_t mxGetNumberOfElements(const mxArray* a) { return numel(chk(a, "mxGetNumberOfElements")); }
const mwSize* mxGetDimensions(const mxArray* a) { return chk(a, "mxGetDimensions")->dims.data(); }
mwSize mxGetNumberOfDimensions(const mxArray* a) { return chk(a, "mxGetNumberOfDimensions")->dims.size(); }

/* ---- data ------------------------------------------------------------------------------------------------------- */
double* mxGetDoubles(const mxArray* a) {
  if (chk(a, "mxGetDoubles")->kind != MXMOCK_DOUBLE) misuse("mxGetDoubles: the array is not double");
  if (a->cplx) misuse("mxGetDoubles: the array is complex");
  return const_cast<double*>(a->d.data());
}
void* mxGetData(const mxArray* a) {
  chk(a, "mxGetData");
  switch (a->kind) {
    case MXMOCK_DOUBLE: return const_cast<double*>(a->d.data());
    case MXMOCK_UINT8: case MXMOCK_LOGICAL: return const_cast<uint8_t*>(a->b.data());
    case MXMOCK_SINGLE: return const_cast<float*>(a->f.data());
    default: misuse("mxGetData: the array is not numeric");
  }
}
double mxGetScalar(const mxArray* a) {
  chk(a, "mxGetScalar");
  if (a->kind == MXMOCK_CELL || a->kind == MXMOCK_STRUCT || a->kind == MXMOCK_OBJECT)
    misuse("mxGetScalar: the array is a cell, a struct or an object");
  if (numel(a) == 0 || (a->sparse && a->d.empty())) misuse("mxGetScalar: the array is empty");
  switch (a->kind) {
    case MXMOCK_DOUBLE: return a->d[0];
    case MXMOCK_UINT8: case MXMOCK_LOGICAL: return (double)a->b[0];
    case MXMOCK_SINGLE: return (double)a->f[0];
    default: return (double)(unsigned char)a->chars[0];
  }
}
mwIndex* mxGetIr(const mxArray* a) {
  if (!chk(a, "mxGetIr")->sparse) misuse("mxGetIr: the array is full");
  return const_cast<mwIndex*>(a->ir.data());
}
mwIndex* mxGetJc(const mxArray* a) {
  if (!chk(a, "mxGetJc")->sparse) misuse("mxGetJc: the array is full");
  return const_cast<mwIndex*>(a->jc.data());
}
char* mxArrayToString(const mxArray* a) {
  if (chk(a, "mxArrayToString")->kind != MXMOCK_CHAR) return nullptr;       // documented: NULL for a non-char array
  char* s = static_cast<char*>(std::malloc(a->chars.size() + 1));
  std::memcpy(s, a->chars.c_str(), a->chars.size() + 1);
  return s;
}
void mxFree(void* p) { std::free(p); }
double mxGetNaN(void) { return std::numeric_limits<double>::quiet_NaN(); }

/* ---- containers ------------------------------------------------------------------------------------------------- */
mxArray* mxGetCell(const mxArray* a, mwIndex i) {
  if (chk(a, "mxGetCell")->kind != MXMOCK_CELL) misuse("mxGetCell: the array is not a cell");
  if (i >= a->kids.size()) misuse("mxGetCell: index out of range");
  return a->kids[i];
}
void mxSetCell(mxArray* a, mwIndex i, mxArray* v) {
  if (chk(a, "mxSetCell")->kind != MXMOCK_CELL) misuse("mxSetCell: the array is not a cell");
  if (i >= a->kids.size()) misuse("mxSetCell: index out of range");
  adopt(a, a->kids[i], v, "mxSetCell");
}
mxArray* mxGetField(const mxArray* a, mwIndex i, const char* name) {
  if (chk(a, "mxGetField")->kind != MXMOCK_STRUCT) misuse("mxGetField: the array is not a struct");
  if (i != 0) misuse("mxGetField: index out of range");
  for (size_t q = 0; q < a->names.size(); ++q)
    if (a->names[q] == name) return a->kids[q];
  return nullptr;                                                            // documented: NULL for a field it lacks
}
void mxSetField(mxArray* a, mwIndex i, const char* name, mxArray* v) {
  if (chk(a, "mxSetField")->kind != MXMOCK_STRUCT) misuse("mxSetField: the array is not a struct");
  if (i != 0) misuse("mxSetField: index out of range");
  for (size_t q = 0; q < a->names.size(); ++q)
    if (a->names[q] == name) { adopt(a, a->kids[q], v, "mxSetField"); return; }
  misuse(std::string("mxSetField: undeclared field '") + name + "'");
}
mxArray* mxGetProperty(const mxArray* a, mwIndex i, const char* name) {
  if (chk(a, "mxGetProperty")->kind != MXMOCK_OBJECT || i != 0) return nullptr;
  for (size_t q = 0; q < a->names.size(); ++q)
    if (a->names[q] == name) return dup(a->kids[q]);                         // a copy the caller must destroy
  return nullptr;
}

/* ---- creation and destruction ----------------------------------------------------------------------------------- */
mxArray* mxCreateDoubleMatrix(mwSize m, mwSize n, mxComplexity c) {
  mxArray* a = make(MXMOCK_DOUBLE, {m, n});
  a->d.assign(m * n, 0.0);
  a->cplx = c == mxCOMPLEX;
  return a;
}
mxArray* mxCreateDoubleScalar(double v) {
  mxArray* a = mxCreateDoubleMatrix(1, 1, mxREAL);
  a->d[0] = v;
  return a;
}
mxArray* mxCreateCellMatrix(mwSize m, mwSize n) {
  mxArray* a = make(MXMOCK_CELL, {m, n});
  a->kids.assign(m * n, nullptr);
  return a;
}
mxArray* mxCreateStructMatrix(mwSize m, mwSize n, int nf, const char** names) {
  if (m != 1 || n != 1) misuse("mxCreateStructMatrix: the mock has 1 x 1 structs only");
  mxArray* a = make(MXMOCK_STRUCT, {1, 1});
  for (int i = 0; i < nf; ++i) {
    for (const std::string& s : a->names)
      if (s == names[i]) misuse(std::string("mxCreateStructMatrix: duplicate field '") + names[i] + "'");
    a->names.push_back(names[i]);
  }
  a->kids.assign((size_t)nf, nullptr);
  return a;
}
mxArray* mxCreateString(const char* s) {
  mxArray* a = make(MXMOCK_CHAR, {(mwSize)(*s ? 1 : 0), (mwSize)std::strlen(s)});
  a->chars = s;
  return a;
}
mxArray* mxDuplicateArray(const mxArray* a) { return dup(chk(a, "mxDuplicateArray")); }
void mxDestroyArray(mxArray* a) {
  if (!a) return;                                                            // documented: a null pointer is ignored
  if (!a->alive) misuse("mxDestroyArray: the array was destroyed before");
  if (a->parent) misuse("mxDestroyArray: the array belongs to a cell, a struct or an object");
  kill(a);
}

/* ---- mex* ------------------------------------------------------------------------------------------------------- */
void mexErrMsgIdAndTxt(const char* id, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::string text = vformat(fmt, ap);
  va_end(ap);
  throw MexError{id, text};                                                   // never returns, as in MATLAB
}
void mexWarnMsgIdAndTxt(const char* id, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::string text = vformat(fmt, ap);
  va_end(ap);
  std::lock_guard<std::mutex> lock(g_out_mutex);
  g_warns.emplace_back(id, text);
}
int mexAtExit(void (*fn)(void)) {
  ++g_at_exit_calls;
  g_at_exit.assign(1, fn);                                                   // one hook per MEX file: the last one set
  return 0;
}
int mexPrintf(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::string text = vformat(fmt, ap);
  va_end(ap);
  std::lock_guard<std::mutex> lock(g_out_mutex);
  g_printed.push_back({text, this_thread()});
  return (int)text.size();
}
int mexEvalString(const char* s) {
  std::lock_guard<std::mutex> lock(g_out_mutex);
  g_evals.emplace_back(s);
  return 0;
}

/* ---- mxmock.h --------------------------------------------------------------------------------------------------- */
mxArray* mxmock_create_double_nd(int ndim, const mwSize* dims, const double* data) {
  mxArray* a = make(MXMOCK_DOUBLE, std::vector<mwSize>(dims, dims + ndim));
  while (a->dims.size() < 2) a->dims.push_back(1);
  a->d.assign(numel(a), 0.0);
  if (data) std::memcpy(a->d.data(), data, sizeof(double) * a->d.size());
  return a;
}
mxArray* mxmock_create_uint8_nd(int ndim, const mwSize* dims, const uint8_t* data) {
  mxArray* a = make(MXMOCK_UINT8, std::vector<mwSize>(dims, dims + ndim));
  while (a->dims.size() < 2) a->dims.push_back(1);
  a->b.assign(numel(a), 0);
  if (data) std::memcpy(a->b.data(), data, a->b.size());
  return a;
}
mxArray* mxmock_create_logical(mwSize m, mwSize n, const uint8_t* data) {
  mxArray* a = make(MXMOCK_LOGICAL, {m, n});
  a->b.assign(m * n, 0);
  if (data) std::memcpy(a->b.data(), data, a->b.size());
  return a;
}
mxArray* mxmock_create_single(mwSize m, mwSize n, const float* data) {
  mxArray* a = make(MXMOCK_SINGLE, {m, n});
  a->f.assign(m * n, 0.0f);
  if (data) std::memcpy(a->f.data(), data, sizeof(float) * a->f.size());
  return a;
}
mxArray* mxmock_create_sparse(mwSize m, mwSize n, const mwIndex* ir, const mwIndex* jc, const double* vals, int is_complex) {
  mxArray* a = make(MXMOCK_DOUBLE, {m, n});
  a->sparse = true;
  a->cplx = is_complex != 0;
  a->jc.assign(jc, jc + n + 1);
  const size_t nnz = a->jc[n];
  a->ir.assign(ir, ir + nnz);
  a->d.assign(vals, vals + nnz);
  a->ir.reserve(nnz + 1);                                                    // nzmax >= 1 in MATLAB: a valid address
  a->d.reserve(nnz + 1);
  return a;
}
mxArray* mxmock_create_object(const char* cls) {
  mxArray* a = make(MXMOCK_OBJECT, {1, 1});
  a->cls = cls;
  return a;
}
void mxmock_set_property(mxArray* obj, const char* name, mxArray* value) {
  obj->names.push_back(name);
  obj->kids.push_back(nullptr);
  adopt(obj, obj->kids.back(), value, "mxmock_set_property");
}
void mxmock_set_complex(mxArray* a, int is_complex) { a->cplx = is_complex != 0; }

int mxmock_kind(const mxArray* a) { return chk(a, "mxmock_kind")->kind; }
int mxmock_num_fields(const mxArray* a) { return (int)chk(a, "mxmock_num_fields")->names.size(); }
const char* mxmock_field_name(const mxArray* a, int i) { return chk(a, "mxmock_field_name")->names.at((size_t)i).c_str(); }
const char* mxmock_chars(const mxArray* a) { return chk(a, "mxmock_chars")->chars.c_str(); }

int mxmock_call(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[], const char** err_id, const char** err_msg) {
  int status = 0;
  g_call_thread = this_thread();
  g_call_created.clear();
  g_in_call = true;
  try {
    mexFunction(nlhs, plhs, nrhs, prhs);
  } catch (const MexError& e) {
    status = 1; g_err_id = e.id; g_err_msg = e.text;
  } catch (const Misuse& e) {
    status = 2; g_err_id = "mxmock:misuse"; g_err_msg = e.text;
  }
  g_in_call = false;
  // what the call created and did not hand back goes, as MATLAB's memory manager does it; after an error all of it
  const int nout = nlhs > 1 ? nlhs : 1;
  for (mxArray* a : g_call_created) {
    if (!a->alive || a->parent) continue;
    if (a->displaced && status == 0) ++g_orphans;      // real MATLAB would leak it: it was part of another array
    bool returned = false;
    for (int i = 0; status == 0 && i < nout; ++i) returned = returned || plhs[i] == a;
    if (!returned) kill(a);
  }
  if (status != 0)
    for (int i = 0; i < nout; ++i) plhs[i] = nullptr;
  g_call_created.clear();
  if (err_id) *err_id = status ? g_err_id.c_str() : "";
  if (err_msg) *err_msg = status ? g_err_msg.c_str() : "";
  return status;
}
int mxmock_run_at_exit(void) {
  const std::vector<void (*)(void)> hooks = g_at_exit;       // the hook stays set: the MEX file is not unloaded here
  for (auto fn : hooks) fn();
  return (int)hooks.size();
}
int mxmock_at_exit_registered(void) { return g_at_exit_calls; }
void mxmock_free_all(void) {
  for (mxArray* a : g_all) delete a;
  g_all.clear();
  g_call_created.clear();
}
int64_t mxmock_orphans(void) { return g_orphans; }
int64_t mxmock_live_arrays(void) {
  int64_t n = 0;
  for (const mxArray* a : g_all) n += a->alive ? 1 : 0;
  return n;
}

int mxmock_printf_count(void) { return (int)g_printed.size(); }
const char* mxmock_printf_text(int i) { return g_printed.at((size_t)i).text.c_str(); }
uint64_t mxmock_printf_thread(int i) { return g_printed.at((size_t)i).thread; }
uint64_t mxmock_call_thread(void) { return g_call_thread; }
int mxmock_eval_count(void) { return (int)g_evals.size(); }
const char* mxmock_eval_text(int i) { return g_evals.at((size_t)i).c_str(); }
int mxmock_warn_count(void) { return (int)g_warns.size(); }
const char* mxmock_warn_id(int i) { return g_warns.at((size_t)i).first.c_str(); }
const char* mxmock_warn_text(int i) { return g_warns.at((size_t)i).second.c_str(); }
void mxmock_clear_output(void) {
  g_printed.clear();
  g_evals.clear();
  g_warns.clear();
}

}  // extern "C"
