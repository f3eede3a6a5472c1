/*
 * host_check.cpp -- a stand-alone program (its own main) that runs the MEX gateway on the CPU: it hand-builds four
 * inputs with the mock's constructors (mxmock.h), calls mexFunction against the recording fake of the C ABI
 * (fake_aoadmm.cpp) and prints "RESULT ok".  Inputs: a dense CP block; a PARAFAC2 block with cell-valued state and
 * masks; a weighted sparse block with held-out and ranking lists; one error path.  It also checks that the mock refuses
 * the uses MATLAB leaves undefined.  tests/test_mex_gateway_host.py builds and runs it as it is; the `host_check_asan`
 * target of matlab-code_amd/mex/Makefile builds it with -fsanitize=address,undefined for a run on the CPU.
 */
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "mxmock.h"

extern "C" {
const char* fake_log(void);
void fake_clear_log(void);
int fake_contexts_created(void);
int fake_contexts_destroyed(void);
}

namespace {

int g_failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } \
  } while (0)

mxArray* mat(mwSize m, mwSize n, double first = 0.25) {          // m x n with the values first, first + 1, ...
  mxArray* a = mxCreateDoubleMatrix(m, n, mxREAL);
  for (mwSize i = 0; i < m * n; ++i) mxGetDoubles(a)[i] = first + (double)i;
  return a;
}
mxArray* row(std::initializer_list<double> v) {
  mxArray* a = mxCreateDoubleMatrix(v.size() ? 1 : 0, v.size(), mxREAL);
  size_t i = 0;
  for (double x : v) mxGetDoubles(a)[i++] = x;
  return a;
}
mxArray* empty() { return mxCreateDoubleMatrix(0, 0, mxREAL); }
mxArray* cell(std::vector<mxArray*> v) {
  mxArray* c = mxCreateCellMatrix(v.empty() ? 0 : 1, v.size());
  for (size_t i = 0; i < v.size(); ++i) mxSetCell(c, i, v[i]);
  return c;
}
mxArray* strct(std::vector<std::pair<const char*, mxArray*>> f) {
  std::vector<const char*> names;
  for (auto& e : f) names.push_back(e.first);
  mxArray* s = mxCreateStructMatrix(1, 1, (int)names.size(), names.data());
  for (auto& e : f) mxSetField(s, 0, e.first, e.second);
  return s;
}
mxArray* strs(std::initializer_list<const char*> v) {
  std::vector<mxArray*> c;
  for (const char* s : v) c.push_back(mxCreateString(s));
  return cell(c);
}
mxArray* options(double max_outer, mxArray* hip) {
  std::vector<std::pair<const char*, mxArray*>> f = {
      {"MaxOuterIters", mxCreateDoubleScalar(max_outer)}, {"MaxInnerIters", mxCreateDoubleScalar(5)},
      {"AbsFuncTol", mxCreateDoubleScalar(0)}, {"OuterRelTol", mxCreateDoubleScalar(0)},
      {"innerRelPrTol_coupl", mxCreateDoubleScalar(0)}, {"innerRelPrTol_constr", mxCreateDoubleScalar(0)},
      {"innerRelDualTol_coupl", mxCreateDoubleScalar(0)}, {"innerRelDualTol_constr", mxCreateDoubleScalar(0)},
      {"bsum", mxCreateDoubleScalar(0)}, {"Display", mxCreateString("iter")}, {"DisplayIters", mxCreateDoubleScalar(2)}};
  if (hip) f.push_back({"hip", hip});
  return strct(f);
}
mxArray* coupling(int n_modes) {
  std::vector<mxArray*> none;
  for (int i = 0; i < n_modes; ++i) none.push_back(empty());
  mxArray* lin = mxCreateDoubleMatrix(1, n_modes, mxREAL);
  return strct({{"lin_coupled_modes", lin}, {"coupling_type", empty()}, {"coupl_trafo_matrices", cell(none)}});
}
// Z of one 3-way CP block 4 x 3 x 2 with `object` as its data; non-negativity on mode 1, a box on mode 2
mxArray* cp_Z(mxArray* object, const char* loss = "Frobenius") {
  return strct({{"size", cell({mxCreateDoubleScalar(4), mxCreateDoubleScalar(3), mxCreateDoubleScalar(2)})},
                {"modes", cell({row({1, 2, 3})})}, {"model", strs({"CP"})}, {"loss_function", strs({loss})},
                {"weights", row({1.0})}, {"coupling", coupling(3)}, {"constrained_modes", row({1, 1, 0})},
                {"constraints", cell({strs({"non-negativity"}), cell({mxCreateString("box"), mxCreateDoubleScalar(0), mxCreateDoubleScalar(2)}), empty()})},
                {"object", cell({object})}});
}
mxArray* cp_G() {
  return strct({{"fac", cell({mat(4, 2), mat(3, 2), mat(2, 2)})}, {"constraint_fac", cell({mat(4, 2), mat(3, 2), empty()})},
                {"constraint_dual_fac", cell({mat(4, 2), mat(3, 2), empty()})}, {"coupling_fac", cell({})},
                {"coupling_dual_fac", cell({empty(), empty(), empty()})}});
}

int call(int nlhs, mxArray** plhs, std::vector<const mxArray*> prhs, std::string* id = nullptr, std::string* msg = nullptr) {
  const char *eid = "", *emsg = "";
  const int st = mxmock_call(nlhs, plhs, (int)prhs.size(), prhs.data(), &eid, &emsg);
  if (id) *id = eid;
  if (msg) *msg = emsg;
  if (st == 2) std::printf("mock misuse: %s\n", emsg);
  return st;
}
bool logged(const char* what) { return std::strstr(fake_log(), what) != nullptr; }

void dense_cp() {
  const mwSize dims[3] = {4, 3, 2};
  std::vector<double> X(24);
  for (int i = 0; i < 24; ++i) X[i] = 0.5 * i;
  mxArray* plhs[2] = {nullptr, nullptr};
  fake_clear_log();
  EXPECT(call(2, plhs, {cp_Z(mxmock_create_double_nd(3, dims, X.data())), cp_G(), options(5, nullptr)}) == 0);
  EXPECT(logged("\"fn\": \"aoadmm_tensor_upload\", \"p\": 0, \"data\": [0, 0.5, 1, "));
  EXPECT(logged("\"fn\": \"aoadmm_model_add_cp\", \"p\": 0, \"n_tensor_modes\": 3, \"modes\": [0, 1, 2], \"weight\": 1}"));
  EXPECT(logged("\"constraint\": 2, \"params\": [0, 2], \"n_params\": 2"));
  EXPECT(plhs[0] && plhs[1]);
  if (plhs[0] && plhs[1]) {
    const mxArray* f1 = mxGetCell(mxGetField(plhs[0], 0, "fac"), 1);
    EXPECT(mxGetM(f1) == 3 && mxGetN(f1) == 2 && mxGetDoubles(f1)[5] == 1e3 + 5);
    EXPECT(mxGetScalar(mxGetField(plhs[1], 0, "OuterIterations")) == 3);
    EXPECT(mxGetNumberOfElements(mxGetField(plhs[1], 0, "func_val_conv")) == 4);
    const mxArray* ii = mxGetField(plhs[1], 0, "innerIters");
    EXPECT(mxGetM(ii) == 3 && mxGetN(ii) == 3 && mxGetDoubles(ii)[8] == 23);
    EXPECT(mxGetField(plhs[1], 0, "func_rel_missing") == nullptr);
  }
  EXPECT(mxmock_printf_count() == 2 && mxmock_eval_count() == 2 && mxmock_printf_thread(0) == mxmock_call_thread());
  mxmock_free_all();
  mxmock_clear_output();
}

void par2_with_cells_and_masks() {
  // I = 3, J_k = (2, 3), K = 2, R = 2
  auto cells = [] { return cell({mat(2, 2, 1.0), mat(3, 2, 5.0)}); };
  const mwSize d0[2] = {3, 2}, d1[2] = {3, 3};
  const uint8_t m0[6] = {1, 0, 1, 1, 1, 0}, m1[9] = {1, 1, 1, 0, 1, 1, 1, 1, 0};
  mxArray* Z = strct({{"size", cell({mxCreateDoubleScalar(3), row({2, 3}), mxCreateDoubleScalar(2)})},
                      {"modes", cell({row({1, 2, 3})})}, {"model", strs({"PAR2"})}, {"loss_function", strs({"Frobenius"})},
                      {"weights", row({0.5})}, {"coupling", coupling(3)}, {"constrained_modes", row({0, 0, 1})},
                      {"constraints", cell({empty(), empty(), strs({"non-negativity"})})},
                      {"object", cell({cell({mat(3, 2), mat(3, 3, 6.25)})})},
                      {"miss", cell({cell({mxmock_create_uint8_nd(2, d0, m0), mxmock_create_uint8_nd(2, d1, m1)})})}});
  mxArray* G = strct({{"fac", cell({mat(3, 2), cells(), mat(2, 2)})}, {"constraint_fac", cell({empty(), empty(), mat(2, 2)})},
                      {"constraint_dual_fac", cell({empty(), empty(), mat(2, 2)})}, {"coupling_fac", cell({})},
                      {"coupling_dual_fac", cell({empty(), empty(), empty()})}, {"DeltaB", cell({mat(2, 2)})},
                      {"P", cell({cells()})}, {"mu_DeltaB", cell({cells()})}});
  mxArray* plhs[2] = {nullptr, nullptr};
  fake_clear_log();
  EXPECT(call(2, plhs, {Z, G, options(0, nullptr)}) == 0);
  EXPECT(logged("\"fn\": \"aoadmm_model_set_mode_slabs\", \"mode\": 1, \"K\": 2, \"rows_k\": [2, 3], \"rank\": 2}"));
  EXPECT(logged("\"fn\": \"aoadmm_par2_slab_upload\", \"p\": 0, \"k\": -1, \"data\": [0.25, 1.25, 2.25, 3.25, 4.25, 5.25, 6.25, "));
  EXPECT(logged("\"fn\": \"aoadmm_par2_slab_mask_upload\", \"p\": 0, \"k\": 1, \"mask\": [1, 1, 1, 0, 1, 1, 1, 1, 0]}"));
  EXPECT(logged("\"fn\": \"aoadmm_state_set\", \"field\": 0, \"index\": 1, \"slab\": -1, \"host\": [1, 2, 3, 4, 5, 6, 7, 8, 9, 10], \"rows\": 5, \"cols\": 2}"));
  EXPECT(logged("\"fn\": \"aoadmm_state_get\", \"field\": 7, \"index\": 0, \"slab\": -1, \"rows\": 5, \"cols\": 2}"));
  if (plhs[0] && plhs[1]) {
    const mxArray* P1 = mxGetCell(mxGetCell(mxGetField(plhs[0], 0, "P"), 0), 1);
    EXPECT(mxGetM(P1) == 3 && mxGetN(P1) == 2 && mxGetDoubles(P1)[0] == 6e6 + 4 && mxGetDoubles(P1)[5] == 6e6 + 9);
    const mxArray* ii = mxGetField(plhs[1], 0, "innerIters");
    EXPECT(mxGetM(ii) == 3 && mxGetN(ii) == 1);                   // MaxOuterIters = 0: one column
    EXPECT(mxGetNumberOfElements(mxGetField(plhs[1], 0, "func_rel_missing")) == 1);
  }
  mxmock_free_all();
  mxmock_clear_output();
}

void weighted_sparse_with_lists() {
  // an sptensor 4 x 3 x 2 with three stored entries, 1-based subs nnz x N
  mxArray* X = mxmock_create_object("sptensor");
  const mwSize ds[2] = {3, 3};
  const double subs[9] = {1, 3, 4, 1, 2, 3, 1, 1, 2};
  mxmock_set_property(X, "subs", mxmock_create_double_nd(2, ds, subs));
  mxArray* vals = mxCreateDoubleMatrix(3, 1, mxREAL);
  mxGetDoubles(vals)[0] = 1.5; mxGetDoubles(vals)[1] = -2; mxGetDoubles(vals)[2] = 3;
  mxmock_set_property(X, "vals", vals);
  mxmock_set_property(X, "size", row({4, 3, 2}));
  mxArray* w = mxCreateDoubleMatrix(3, 1, mxREAL);
  mxGetDoubles(w)[0] = 0.5; mxGetDoubles(w)[1] = 1; mxGetDoubles(w)[2] = 0.25;
  const mwSize dh[2] = {2, 3};
  const double hs[6] = {4, 1, 3, 1, 2, 1}, rs[6] = {2, 3, 1, 3, 1, 2};
  mxArray* hv = mxCreateDoubleMatrix(2, 1, mxREAL);
  mxGetDoubles(hv)[0] = 0.75; mxGetDoubles(hv)[1] = -0.5;
  mxArray* hip = strct({{"sparse_entry_weights", cell({w})}, {"sparse_unstored_weight", mxCreateDoubleScalar(0.125)},
                        {"heldout", cell({strct({{"subs", mxmock_create_double_nd(2, dh, hs)}, {"vals", hv}})})},
                        {"heldout_keep_best", mxCreateDoubleScalar(1)},
                        {"rank_lists", cell({strct({{"mode", mxCreateDoubleScalar(2)}, {"subs", mxmock_create_double_nd(2, dh, rs)},
                                                    {"excl_off", row({0, 1, 3})}, {"excl_idx", row({3, 1, 2})}})})},
                        {"rank_metric", mxCreateString("hit@5")}});
  mxArray* plhs[2] = {nullptr, nullptr};
  fake_clear_log();
  EXPECT(call(2, plhs, {cp_Z(X), cp_G(), options(4, hip)}) == 0);
  EXPECT(logged("\"fn\": \"aoadmm_tensor_upload_coo\", \"p\": 0, \"nnz\": 3, \"subs\": [0, 2, 3, 0, 1, 2, 0, 0, 1], \"vals\": [1.5, -2, 3]}"));
  EXPECT(logged("\"fn\": \"aoadmm_tensor_set_entry_weights\", \"p\": 0, \"nnz\": 3, \"subs\": [0, 2, 3, 0, 1, 2, 0, 0, 1], \"wts\": [0.5, 1, 0.25], \"unstored_weight\": 0.125}"));
  EXPECT(logged("\"fn\": \"aoadmm_tensor_set_heldout\", \"p\": 0, \"n\": 2, \"subs\": [3, 0, 2, 0, 1, 0], \"vals\": [0.75, -0.5]}"));
  EXPECT(logged("\"fn\": \"aoadmm_tensor_set_ranklist\", \"p\": 0, \"mode\": 1, \"nq\": 2, \"subs\": [1, 2, 0, 2, 0, 1], \"excl_off\": [0, 1, 3], \"excl_idx\": [2, 0, 1]"));
  EXPECT(logged("\"fn\": \"aoadmm_rank_track\", \"metric\": 0, \"k\": 5, \"every\": 1, \"patience\": 0, \"criterion\": 0}"));
  if (plhs[1]) {
    EXPECT(mxGetScalar(mxGetField(plhs[1], 0, "heldout_restored_iter")) == 1);
    EXPECT(mxGetNumberOfElements(mxGetCell(mxGetField(plhs[1], 0, "func_heldout"), 0)) == 4);
    const mxArray* tr = mxGetCell(mxGetField(plhs[1], 0, "rank_trace"), 0);
    EXPECT(mxmock_num_fields(tr) == 11 && mxGetDoubles(mxGetField(tr, 0, "auc"))[0] != mxGetDoubles(mxGetField(tr, 0, "auc"))[0]);
    EXPECT(mxGetNumberOfElements(mxGetField(plhs[1], 0, "func_rel_missing")) == 4);
  }
  mxmock_free_all();
  mxmock_clear_output();
}

void error_path() {
  const mwSize dims[3] = {4, 3, 2};
  mxArray* plhs[2] = {nullptr, nullptr};
  std::string id, msg;
  EXPECT(call(2, plhs, {cp_Z(mxmock_create_double_nd(3, dims, nullptr), "KL"), cp_G(), options(5, nullptr)}, &id, &msg) == 1);
  EXPECT(id == "cmtf:hip:unsupported" && msg == "non-Frobenius losses need the L-BFGS-B path of the MATLAB code");
  EXPECT(plhs[0] == nullptr);
  // an error in the middle of the model description; the next good call runs
  mxArray* Z = cp_Z(mxmock_create_double_nd(3, dims, nullptr));
  mxSetCell(mxGetField(Z, 0, "constraints"), 1, strs({"custom"}));
  EXPECT(call(2, plhs, {Z, cp_G(), options(5, nullptr)}, &id, &msg) == 1 && id == "cmtf:hip:unsupported");
  EXPECT(call(2, plhs, {cp_Z(mxmock_create_double_nd(3, dims, nullptr)), cp_G(), options(5, nullptr)}) == 0 && plhs[0] && plhs[1]);
  mxmock_free_all();
  mxmock_clear_output();
}

template <class Fn> bool refused(Fn fn) {
  try { fn(); } catch (...) { return true; }
  return false;
}
void mock_is_strict() {
  mxArray* d = mat(2, 2);
  mxArray* c = cell({mat(1, 1)});
  const mwSize one[2] = {1, 1};
  mxArray* u = mxmock_create_uint8_nd(2, one, nullptr);
  const char* names[1] = {"a"};
  mxArray* s = mxCreateStructMatrix(1, 1, 1, names);
  EXPECT(refused([&] { mxGetDoubles(u); }));
  EXPECT(refused([&] { mxGetScalar(empty()); }));
  EXPECT(refused([&] { mxGetCell(c, 1); }) && refused([&] { mxGetCell(d, 0); }));
  EXPECT(refused([&] { mxGetField(d, 0, "a"); }) && refused([&] { mxGetField(s, 1, "a"); }));
  EXPECT(refused([&] { mxGetIr(d); }) && refused([&] { mxGetJc(d); }));
  EXPECT(refused([&] { mxSetField(s, 0, "b", mat(1, 1)); }));
  EXPECT(mxGetField(s, 0, "b") == nullptr && mxArrayToString(d) == nullptr);         // documented, not misuse
  mxDestroyArray(d);
  EXPECT(refused([&] { mxGetM(d); }) && refused([&] { mxDestroyArray(d); }));
  EXPECT(refused([&] { mxDestroyArray(mxGetCell(c, 0)); }));                         // it belongs to the cell
  mxArray* X = mxmock_create_object("tensor");
  mxmock_set_property(X, "data", mat(2, 3));
  mxArray* copy = mxGetProperty(X, 0, "data");
  EXPECT(copy && copy != nullptr && mxGetN(copy) == 3);
  mxDestroyArray(copy);                                                              // a copy: the caller's to destroy
  EXPECT(mxGetProperty(X, 0, "nothing") == nullptr && mxIsClass(X, "tensor") && !mxIsClass(X, "sptensor"));
  mxmock_free_all();
}

}  // namespace

int main() {
  dense_cp();
  par2_with_cells_and_masks();
  weighted_sparse_with_lists();
  error_path();
  mock_is_strict();
  EXPECT(mxmock_at_exit_registered() == 1 && fake_contexts_created() == 1 && mxmock_orphans() == 0);
  mxmock_run_at_exit();
  mxmock_run_at_exit();
  EXPECT(fake_contexts_destroyed() == 1);
  if (g_failures) {
    std::printf("RESULT failed (%d)\n", g_failures);
    return 1;
  }
  std::printf("RESULT ok\n");
  return 0;
}
