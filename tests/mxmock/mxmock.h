/*
 * mxmock.h -- test-only entry points of the functional mock of the C Matrix API (mxmock.cpp).
 *
 * The gateway (matlab-code_amd/mex/aoadmm_mex.cpp) is compiled against mex_stub/mex.h and linked with mxmock.cpp, which
 * defines every function that header declares.  What mex.h cannot do -- build inputs of the kinds only MATLAB creates,
 * read results back, call mexFunction the way MATLAB does -- is declared here, as plain C so that ctypes can use it.
 */
#ifndef AOADMM_MXMOCK_H
#define AOADMM_MXMOCK_H
#include <stdint.h>
#include "mex.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MXMOCK_DOUBLE = 0, MXMOCK_UINT8 = 1, MXMOCK_CHAR = 2, MXMOCK_LOGICAL = 3, MXMOCK_SINGLE = 4, MXMOCK_CELL = 5,
       MXMOCK_STRUCT = 6, MXMOCK_OBJECT = 7 };

/* ---- constructors for what mex.h cannot create.  Data is copied; a null `data` leaves zeros. */
mxArray* mxmock_create_double_nd(int ndim, const mwSize* dims, const double* data);
mxArray* mxmock_create_uint8_nd(int ndim, const mwSize* dims, const uint8_t* data);
mxArray* mxmock_create_logical(mwSize m, mwSize n, const uint8_t* data);
mxArray* mxmock_create_single(mwSize m, mwSize n, const float* data);
/* sparse double m x n in compressed columns: jc has n + 1 entries, ir and vals jc[n]; is_complex only sets the flag */
mxArray* mxmock_create_sparse(mwSize m, mwSize n, const mwIndex* ir, const mwIndex* jc, const double* vals, int is_complex);
/* a 1 x 1 object of class `cls` (`tensor`, `sptensor`); the object takes the property value over */
mxArray* mxmock_create_object(const char* cls);
void mxmock_set_property(mxArray* obj, const char* name, mxArray* value);
void mxmock_set_complex(mxArray* a, int is_complex);          /* flags a full double array complex */

/* ---- read accessors */
int mxmock_kind(const mxArray* a);
int mxmock_num_fields(const mxArray* a);                       /* struct fields / object properties, in order */
const char* mxmock_field_name(const mxArray* a, int i);
const char* mxmock_chars(const mxArray* a);                    /* the text of a char array */

/* ---- the call.  Runs mexFunction inside try.  0: returned; 1: mexErrMsgIdAndTxt (id / message in *err_id / *err_msg,
 * valid until the next call); 2: the mock refused a use MATLAB leaves undefined (id "mxmock:misuse").  Arrays created
 * during the call that are neither returned nor owned by a returned array are released when it ends, as MATLAB does;
 * after an error that includes plhs. */
int mxmock_call(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[], const char** err_id, const char** err_msg);
int mxmock_run_at_exit(void);                                  /* runs the mexAtExit hook; returns how many ran */
int mxmock_at_exit_registered(void);                           /* how many times mexAtExit was called */
void mxmock_free_all(void);                                    /* releases every array the mock still holds */
int64_t mxmock_live_arrays(void);
/* arrays that mxSetCell / mxSetField displaced from a cell or struct during successful calls and that the gateway did not
 * destroy: MATLAB does not free what these functions replace, so each is a leak there */
int64_t mxmock_orphans(void);

/* ---- what the gateway said */
int mxmock_printf_count(void);
const char* mxmock_printf_text(int i);
uint64_t mxmock_printf_thread(int i);
uint64_t mxmock_call_thread(void);                             /* the thread of the last mxmock_call */
int mxmock_eval_count(void);
const char* mxmock_eval_text(int i);
int mxmock_warn_count(void);
const char* mxmock_warn_id(int i);
const char* mxmock_warn_text(int i);
void mxmock_clear_output(void);

#ifdef __cplusplus
}
#endif
#endif
