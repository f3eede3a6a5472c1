"""Runs the MEX gateway (matlab-code_amd/mex/aoadmm_mex.cpp) without MATLAB.

The gateway is compiled with tests/mxmock/mxmock.cpp, a functional mock of the C Matrix API, into one shared object that
is linked either against libaoadmm_hip.so (the real library: `build(outdir, fake=False)`) or against
tests/mxmock/fake_aoadmm.cpp, a fake of the C ABI that records every call (`fake=True`, no GPU needed).

`to_mx` lays the dicts the tests use (tests/helpers.py models, the G of `init_coupled_AOADMM_CMTF`, `helpers.options`
with an `options['hip']` dict) out as MATLAB has them and as the gateway documents them: cell arrays, column-major
doubles, 1-based `Z.modes`, subscripts and block numbers, uint8 masks with 1 = observed.  `driver.build_model` /
`driver.upload_state` are the statement of what each field means.  `from_mx` turns `Fac` and `out` back into the shapes
`pkg.cmtf_AOADMM` returns.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEX_DIR = os.path.join(ROOT, 'matlab-code_amd', 'mex')
MOCK_DIR = os.path.join(ROOT, 'tests', 'mxmock')
LIB_DIR = os.path.join(ROOT, 'matlab-code_amd')
INCLUDES = ['-I', os.path.join(MEX_DIR, 'mex_stub'), '-I', os.path.join(ROOT, 'include'), '-I', MOCK_DIR]

K_DOUBLE, K_UINT8, K_CHAR, K_LOGICAL, K_SINGLE, K_CELL, K_STRUCT, K_OBJECT = range(8)


class MexError(Exception):
    """mexErrMsgIdAndTxt(id, msg) inside the gateway."""

    def __init__(self, id, msg):
        super().__init__('%s: %s' % (id, msg))
        self.id, self.msg = id, msg


class MockMisuse(AssertionError):
    """The gateway used the C Matrix API in a way MATLAB leaves undefined (mxmock:misuse)."""


class Raw:
    """A value `to_mx` passes through: `make(harness)` returns the mxArray pointer (for the kinds no dict maps to)."""

    def __init__(self, make):
        self.make = make


class TensorObject:
    """A Tensor Toolbox `tensor`: an object of that class with the property `data`."""

    def __init__(self, data):
        self.data = data


def gateway_source(src=None):
    return src or os.path.join(MEX_DIR, 'aoadmm_mex.cpp')


def build(outdir, fake, src=None, name=None):
    """g++ -std=c++17: gateway + mock (+ fake, or -laoadmm_hip) -> one shared object in `outdir`; returns its path."""
    so = os.path.join(str(outdir), name or ('mexgw_fake.so' if fake else 'mexgw_real.so'))
    # -Bsymbolic: the object's own mx* and (fake) aoadmm_* definitions serve its own calls, whatever else the process has loaded
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-shared', '-fPIC', '-Wl,-Bsymbolic'] + INCLUDES + \
          [gateway_source(src), os.path.join(MOCK_DIR, 'mxmock.cpp')]
    if fake:
        cmd += [os.path.join(MOCK_DIR, 'fake_aoadmm.cpp')]
    else:
        cmd += ['-L', LIB_DIR, '-laoadmm_hip', '-Wl,-rpath,' + LIB_DIR]
    subprocess.run(cmd + ['-o', so, '-lpthread'], check=True)
    return so


def build_host_check(outdir, extra_flags=()):
    """tests/mxmock/host_check.cpp + gateway + mock + fake -> a stand-alone program; returns its path."""
    exe = os.path.join(str(outdir), 'host_check')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall'] + list(extra_flags) + INCLUDES +
                   [os.path.join(MOCK_DIR, 'host_check.cpp'), gateway_source(), os.path.join(MOCK_DIR, 'mxmock.cpp'),
                    os.path.join(MOCK_DIR, 'fake_aoadmm.cpp'), '-o', exe, '-lpthread'], check=True)
    return exe


class Harness:
    def __init__(self, so, fake):
        self.fake = fake
        self.lib = lib = C.CDLL(so)
        P, Z, I = C.c_void_p, C.c_size_t, C.c_int
        sig = {
            'mxCreateDoubleMatrix': (P, [Z, Z, I]), 'mxCreateDoubleScalar': (P, [C.c_double]), 'mxCreateCellMatrix': (P, [Z, Z]),
            'mxCreateStructMatrix': (P, [Z, Z, I, C.POINTER(C.c_char_p)]), 'mxCreateString': (P, [C.c_char_p]),
            'mxSetCell': (None, [P, Z, P]), 'mxSetField': (None, [P, Z, C.c_char_p, P]), 'mxGetCell': (P, [P, Z]),
            'mxGetField': (P, [P, Z, C.c_char_p]), 'mxGetNumberOfElements': (Z, [P]), 'mxGetNumberOfDimensions': (Z, [P]),
            'mxGetDimensions': (C.POINTER(Z), [P]), 'mxGetData': (P, [P]),
            'mxmock_create_double_nd': (P, [I, C.POINTER(Z), P]), 'mxmock_create_uint8_nd': (P, [I, C.POINTER(Z), P]),
            'mxmock_create_logical': (P, [Z, Z, P]), 'mxmock_create_single': (P, [Z, Z, P]),
            'mxmock_create_sparse': (P, [Z, Z, P, P, P, I]), 'mxmock_create_object': (P, [C.c_char_p]),
            'mxmock_set_property': (None, [P, C.c_char_p, P]), 'mxmock_set_complex': (None, [P, I]),
            'mxmock_kind': (I, [P]), 'mxmock_num_fields': (I, [P]), 'mxmock_field_name': (C.c_char_p, [P, I]),
            'mxmock_chars': (C.c_char_p, [P]),
            'mxmock_call': (I, [I, C.POINTER(P), I, C.POINTER(P), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]),
            'mxmock_run_at_exit': (I, []), 'mxmock_at_exit_registered': (I, []), 'mxmock_free_all': (None, []),
            'mxmock_live_arrays': (C.c_int64, []), 'mxmock_orphans': (C.c_int64, []), 'mxmock_printf_count': (I, []), 'mxmock_printf_text': (C.c_char_p, [I]),
            'mxmock_printf_thread': (C.c_uint64, [I]), 'mxmock_call_thread': (C.c_uint64, []), 'mxmock_eval_count': (I, []),
            'mxmock_eval_text': (C.c_char_p, [I]), 'mxmock_warn_count': (I, []), 'mxmock_warn_id': (C.c_char_p, [I]),
            'mxmock_warn_text': (C.c_char_p, [I]), 'mxmock_clear_output': (None, []),
        }
        if fake:
            sig.update({'fake_log': (C.c_char_p, []), 'fake_clear_log': (None, []), 'fake_fail': (None, [C.c_char_p, I]),
                        'fake_script_solve': (None, [I, C.POINTER(I), I]), 'fake_script_nvecs': (None, [I]),
                        'fake_contexts_created': (I, []), 'fake_contexts_destroyed': (I, [])})
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        self.printed, self.print_threads, self.call_thread, self.evals, self.warns = [], [], 0, [], []
        self.live_before = self.live_after = self.nodes_read = 0       # arrays alive around the last call, arrays it returned

    # ---- python -> mxArray ------------------------------------------------------------------------------------------
    def _dims(self, shape):
        shape = tuple(int(s) for s in shape)
        return len(shape), (C.c_size_t * max(len(shape), 1))(*shape)

    def double(self, a, shape=None):
        """A full double array; 1-D input becomes a row vector unless `shape` says otherwise."""
        a = np.asarray(a, dtype=np.float64)
        if shape is None:
            shape = (1, a.shape[0]) if a.ndim == 1 else ((1, 1) if a.ndim == 0 else a.shape)
        a = np.asfortranarray(a.reshape(shape, order='F'))
        nd, dims = self._dims(shape)
        return self.lib.mxmock_create_double_nd(nd, dims, a.ctypes.data)

    def uint8(self, a):
        a = np.asfortranarray(np.asarray(a, dtype=np.uint8))
        nd, dims = self._dims(a.shape if a.ndim > 1 else (1, a.size))
        return self.lib.mxmock_create_uint8_nd(nd, dims, a.ctypes.data)

    def logical(self, a):
        a = np.asfortranarray(np.atleast_2d(np.asarray(a, dtype=np.uint8)))
        return self.lib.mxmock_create_logical(a.shape[0], a.shape[1], a.ctypes.data)

    def single(self, a):
        a = np.asfortranarray(np.atleast_2d(np.asarray(a, dtype=np.float32)))
        return self.lib.mxmock_create_single(a.shape[0], a.shape[1], a.ctypes.data)

    def sparse(self, m, is_complex=False):
        """A scipy.sparse matrix as MATLAB's compressed columns (row indices ascending within a column)."""
        m = m.tocsc()
        m.sort_indices()
        ir = np.ascontiguousarray(m.indices, dtype=np.uint64)
        jc = np.ascontiguousarray(m.indptr, dtype=np.uint64)
        v = np.ascontiguousarray(m.data, dtype=np.float64)
        return self.lib.mxmock_create_sparse(m.shape[0], m.shape[1], ir.ctypes.data, jc.ctypes.data, v.ctypes.data, int(is_complex))

    def cell(self, items, shape=None):
        items = list(items)
        m, n = shape if shape is not None else (1 if items else 0, len(items))
        c = self.lib.mxCreateCellMatrix(m, n)
        for i, it in enumerate(items):
            self.lib.mxSetCell(c, i, self.to_mx(it))
        return c

    def struct(self, d):
        names = [k.encode() for k in d]
        s = self.lib.mxCreateStructMatrix(1, 1, len(names), (C.c_char_p * max(len(names), 1))(*names))
        for k, v in d.items():
            self.lib.mxSetField(s, 0, k.encode(), self.to_mx(v))
        return s

    def obj(self, cls, props):
        o = self.lib.mxmock_create_object(cls.encode())
        for k, v in props.items():
            self.lib.mxmock_set_property(o, k.encode(), self.to_mx(v))
        return o

    def sptensor(self, X):
        """`pkg.sptensor` (0-based subs) -> an object of class sptensor: subs nnz x N doubles 1-based, vals nnz x 1, size 1 x N."""
        subs = np.asarray(X.subs, dtype=np.float64) + 1.0
        v = np.asarray(X.vals, dtype=np.float64)
        return self.obj('sptensor', dict(subs=Raw(lambda h: h.double(subs, subs.shape)), vals=Raw(lambda h: h.double(v, (v.shape[0], 1))),
                                         size=np.asarray(X.shape, dtype=np.float64)))

    def to_mx(self, v):
        if isinstance(v, Raw):
            return v.make(self)
        if v is None:
            return self.lib.mxCreateDoubleMatrix(0, 0, 0)
        if isinstance(v, str):
            return self.lib.mxCreateString(v.encode())
        if isinstance(v, (bool, int, float, np.integer, np.floating, np.bool_)):
            return self.lib.mxCreateDoubleScalar(float(v))
        if isinstance(v, TensorObject):
            return self.obj('tensor', dict(data=np.asarray(v.data, dtype=np.float64)))
        if type(v).__name__ == 'sptensor':
            return self.sptensor(v)
        if hasattr(v, 'tocsc') and not isinstance(v, np.ndarray):
            return self.sparse(v)
        if isinstance(v, np.ndarray):
            if v.dtype == np.uint8:
                return self.uint8(v)
            if v.dtype == np.bool_:
                return self.logical(v)
            if v.dtype == np.float32:
                return self.single(v)
            return self.double(v)
        if isinstance(v, (list, tuple)):
            return self.cell(v)
        if isinstance(v, dict):
            return self.struct(v)
        raise TypeError('to_mx: no MATLAB layout for %r' % type(v))

    # ---- the three arguments ----------------------------------------------------------------------------------------
    @staticmethod
    def _vec(v):
        return np.asarray(v, dtype=np.float64).reshape(-1)

    def Z_layout(self, Z):
        """The struct Z of cmtf_AOADMM.m as a dict `to_mx` maps field by field."""
        vec = self._vec
        out = {}
        for k, v in Z.items():
            if k.startswith('_'):
                continue
            if isinstance(v, Raw):
                out[k] = v
            elif k == 'size':
                out[k] = [vec(s) if isinstance(s, (list, tuple, np.ndarray)) else float(s) for s in v]
            elif k == 'modes':
                out[k] = [vec(ms) for ms in v]
            elif k in ('weights', 'constrained_modes', 'ridge'):
                out[k] = v if isinstance(v, Raw) else vec(v)
            elif k == 'coupling':
                out[k] = {kk: (vec(vv) if kk in ('lin_coupled_modes', 'coupling_type') else
                               [None if H is None else np.asarray(H, dtype=np.float64) for H in vv]) for kk, vv in v.items()}
            elif k == 'constraints':
                out[k] = [None if c is None else [np.asarray(x, dtype=np.float64) if isinstance(x, np.ndarray) else x for x in c]
                          for c in v]
            elif k == 'object':
                out[k] = [[xk if hasattr(xk, 'tocsc') or isinstance(xk, Raw) else np.asarray(xk, dtype=np.float64) for xk in X]
                          if isinstance(X, (list, tuple)) else
                          (np.asarray(X, dtype=np.float64) if isinstance(X, np.ndarray) else X) for X in v]
            elif k == 'miss':
                def mask(m):
                    if m is None or isinstance(m, Raw):
                        return m
                    if isinstance(m, (list, tuple)):
                        return [mask(mk) for mk in m]
                    return (np.asarray(m) != 0).astype(np.uint8)          # uint8, 1 = observed
                out[k] = None if v is None else [mask(m) for m in v]
            else:
                out[k] = v
        return out

    def G_layout(self, G, P):
        """The struct G of init_coupled_AOADMM_CMTF.m: cells over the modes / couplings / blocks, [] where nothing is."""
        def item(v):
            if v is None or (isinstance(v, (list, tuple)) and len(v) == 0):
                return None
            if isinstance(v, (list, tuple)):
                return [None if x is None else np.asarray(x, dtype=np.float64) for x in v]
            a = np.asarray(v, dtype=np.float64)
            return a.reshape(-1, 1) if a.ndim == 1 else a
        out = {}
        for k, v in G.items():
            if isinstance(v, dict):                                          # DeltaB, P, mu_DeltaB: keyed by 0-based block
                out[k] = [item(v.get(p)) for p in range(P)] if v else []
            else:
                out[k] = [item(x) for x in v]
        return out

    def options_layout(self, opt, Z, precision=None):
        """options as cmtf_fun_AOADMM_hip.m passes them; options.hip in MATLAB's conventions (1-based subscripts, rows and
        block numbers; cells over the blocks)."""
        P = len(Z['object'])
        out = {k: v for k, v in opt.items() if k != 'hip'}
        hip = dict(opt.get('hip', {}))
        if precision is not None:
            hip['precision'] = precision
        lay = {}
        for k, v in hip.items():
            if isinstance(v, Raw):
                lay[k] = v
            elif k == 'devices':
                lay[k] = self._vec(v)
            elif k == 'sparse_observed_only':
                lay[k] = self._vec(v) if isinstance(v, (list, tuple, np.ndarray)) else float(v)
            elif k == 'sparse_entry_weights':
                lay[k] = [None if w is None else np.asarray(w, dtype=np.float64).reshape(-1, 1) for w in v]
            elif k == 'sparse_unstored_weight':
                lay[k] = [None if a is None else float(a) for a in v] if isinstance(v, (list, tuple)) else float(v)
            elif k == 'heldout':
                cells = [None] * P
                for q, item in v.items():
                    subs, vals = (item.subs, item.vals) if type(item).__name__ == 'sptensor' else item
                    subs = np.asarray(subs, dtype=np.float64) + 1.0
                    vals = np.asarray(vals, dtype=np.float64).reshape(-1, 1)
                    cells[q - 1] = dict(subs=Raw(lambda h, s=subs: h.double(s, s.shape)), vals=Raw(lambda h, x=vals: h.double(x, x.shape)))
                lay[k] = cells
            elif k == 'rank_lists':
                cells = [None] * P
                for q, item in v.items():
                    subs = np.asarray(item['subs'], dtype=np.float64) + 1.0
                    e = dict(mode=float(item['mode']), subs=Raw(lambda h, s=subs: h.double(s, s.shape)))
                    if item.get('exclude') is not None:
                        off, idx = item['exclude']
                        e['excl_off'] = self._vec(off)
                        e['excl_idx'] = self._vec(idx) + 1.0
                    cells[q - 1] = e
                lay[k] = cells
            else:
                lay[k] = v
        if lay:
            out['hip'] = lay
        return out

    # ---- mxArray -> python ------------------------------------------------------------------------------------------
    def from_mx(self, a):
        """double -> float64 array of the array's shape (0 x 0 -> None), char -> str, cell -> list, struct -> dict."""
        if not a:
            return None
        self.nodes_read += 1
        lib = self.lib
        kind = lib.mxmock_kind(a)
        nd = lib.mxGetNumberOfDimensions(a)
        dims = tuple(lib.mxGetDimensions(a)[i] for i in range(nd))
        if kind == K_CHAR:
            return lib.mxmock_chars(a).decode()
        if kind == K_CELL:
            return [self.from_mx(lib.mxGetCell(a, i)) for i in range(lib.mxGetNumberOfElements(a))]
        if kind == K_STRUCT:
            return {lib.mxmock_field_name(a, i).decode(): self.from_mx(lib.mxGetField(a, 0, lib.mxmock_field_name(a, i)))
                    for i in range(lib.mxmock_num_fields(a))}
        if kind == K_DOUBLE:
            n = int(np.prod(dims))
            if n == 0:
                return None if dims == (0, 0) else np.zeros(dims, order='F')
            buf = (C.c_double * n).from_address(lib.mxGetData(a))
            return np.array(np.frombuffer(buf, dtype=np.float64).reshape(dims, order='F'), order='F')
        raise TypeError('from_mx: kind %d' % kind)

    @staticmethod
    def Fac_shape(Fac):
        """`Fac` as `pkg.cmtf_AOADMM` returns it: DeltaB / P / mu_DeltaB keyed by 0-based block."""
        out = dict(Fac)
        for k in ('DeltaB', 'P', 'mu_DeltaB'):
            if k in out:
                out[k] = {p: v for p, v in enumerate(out[k] or []) if v is not None}
        return out

    @staticmethod
    def out_shape(out):
        """`out` as `driver.run_solver` returns it: scalars as numbers, traces 1-D, per-block cells keyed by 1-based block."""
        o = {}
        for k, v in out.items():
            if k in ('func_heldout', 'rank_trace'):
                o[k] = {p + 1: ({kk: vv.reshape(-1) for kk, vv in x.items()} if isinstance(x, dict) else x.reshape(-1))
                        for p, x in enumerate(v) if x is not None}
            elif k in ('OuterIterations', 'heldout_best_iter', 'heldout_restored_iter', 'rank_best_iter'):
                o[k] = int(v[0, 0])
            elif k == 'innerIters' or not isinstance(v, np.ndarray):
                o[k] = v
            elif v.size == 1 and k.startswith('f_'):
                o[k] = float(v[0, 0])
            else:
                o[k] = v.reshape(-1)
        return o

    # ---- calls --------------------------------------------------------------------------------------------------------
    def call(self, args, nlhs=1):
        """mexFunction(nlhs, plhs, len(args), args) with `args` laid out by `to_mx`; returns the converted outputs.  Raises
        MexError for mexErrMsgIdAndTxt and MockMisuse for a use of the API that MATLAB leaves undefined."""
        lib = self.lib
        lib.mxmock_clear_output()
        try:
            prhs = (C.c_void_p * max(len(args), 1))(*[self.to_mx(a) for a in args])
            plhs = (C.c_void_p * max(nlhs, 1))()
            eid, emsg = C.c_char_p(), C.c_char_p()
            self.live_before = lib.mxmock_live_arrays()
            st = lib.mxmock_call(nlhs, plhs, len(args), prhs, C.byref(eid), C.byref(emsg))
            self.live_after = lib.mxmock_live_arrays()
            self.printed = [lib.mxmock_printf_text(i).decode() for i in range(lib.mxmock_printf_count())]
            self.print_threads = [lib.mxmock_printf_thread(i) for i in range(lib.mxmock_printf_count())]
            self.call_thread = lib.mxmock_call_thread()
            self.evals = [lib.mxmock_eval_text(i).decode() for i in range(lib.mxmock_eval_count())]
            self.warns = [(lib.mxmock_warn_id(i).decode(), lib.mxmock_warn_text(i).decode()) for i in range(lib.mxmock_warn_count())]
            if st == 1:
                raise MexError(eid.value.decode(), emsg.value.decode())
            if st == 2:
                raise MockMisuse(emsg.value.decode())
            self.nodes_read = 0
            return [self.from_mx(plhs[i]) for i in range(max(nlhs, 1))]
        finally:
            lib.mxmock_free_all()

    def gateway(self, Z, G, options, nlhs=2, precision=None):
        """[Fac, out] = aoadmm_mex(Z, G, options) -> (Fac, out, printed) in the shapes `pkg.cmtf_AOADMM` returns."""
        P = len(Z['object'])
        res = self.call([self.Z_layout(Z), self.G_layout(G, P) if isinstance(G, dict) else G,
                         self.options_layout(options, Z, precision) if isinstance(options, dict) else options], nlhs)
        Fac = self.Fac_shape(res[0]) if res[0] is not None else None
        out = self.out_shape(res[1]) if nlhs > 1 else None
        return Fac, out, ''.join(self.printed)

    # ---- the fake's log ---------------------------------------------------------------------------------------------
    def log(self, clear=True):
        """The calls the fake recorded since the last clear: a list of dicts, `fn` first."""
        text = self.lib.fake_log().decode()
        if clear:
            self.lib.fake_clear_log()
        return [json.loads(line) for line in text.splitlines()]

    def calls(self, fn, log):
        return [c for c in log if c['fn'] == fn]
