"""GPU: half-precision storage of dense 3-way CP blocks (AOADMM_PREC_F16: fp16 entries with one power-of-two scale per
block, three half pass copies that ARE the data, contract16_f16 on the matrix cores with an fp32 T).

The reference everywhere is the fp64 oracle on the DEQUANTISED data D = q / s, with q and s computed here from the rule
of include/aoadmm_hip.h in numpy (float32, frexp, astype(float16)): what is bounded is the kernel, not the quantisation.
Every test asserts that no nonzero |q| is below 2^-14, so no stored entry is subnormal and every entry is exact in
either rounding mode of the convert.

Every MTTKRP case proves its path from the launch accounting of `aoadmm_kernel_stats` (one pass, on a half copy: 2 bytes
per entry of a copy in whole 512-row blocks, T in fp32)."""
import copy
import functools
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from oracle.tensor_ops import mttkrp as o_mttkrp
from helpers import cp_model, options, rel_fro, script3_model

pytestmark = pytest.mark.gpu

TOL_F32 = 2e-6                              # the project's fp32 op-level bar (test_gpu_tensor_pass.TOL['f32'])
ROW_BLOCK = 512                             # misc.h kRowBlockElems
GROUP = 32                                  # misc.h kHalfGroupCols: columns per MFMA / per column group of a half copy

RANKS_ALL = [1, 16, 17, 20, 32, 33, 48, 49, 63, 64]   # both ends of every NT = ceil(R / 16) class
RANKS_CLASS = [20, 32, 48, 64]                        # one rank per class

CASES = ([(d, R) for d in ((6, 10, 2565), (10, 2565, 6), (150, 70, 66)) for R in RANKS_CLASS] +
         [(d, R) for d in ((12, 9, 245), (131, 37, 29)) for R in RANKS_ALL])


@pytest.fixture(scope='module')
def capi():
    return importlib.import_module('matlab-code_amd._capi')


def _round_up(a, b):
    return (a + b - 1) // b * b


def quantize(X):
    """(q as float16, s) by the storage rule; the block's data is q / s."""
    x = np.asarray(X, dtype=np.float64).astype(np.float32)
    a = float(np.abs(x).max())
    s = 1.0
    if a > 0:
        _, E = np.frexp(a)
        s = float(2.0 ** min(127, max(-126, 15 - int(E))))
    q = (x * np.float32(s)).astype(np.float16)
    nz = np.abs(q[q != 0]).astype(np.float64)
    assert nz.size == 0 or nz.min() >= 2.0 ** -14, nz.min()      # no subnormal: exact in either rounding mode
    return q, s


def dequantize(X):
    q, s = quantize(X)
    D = np.asfortranarray(q.astype(np.float64) / s)
    return D, s


def _copy_rows(dims, c):
    """Rows of the half pass copy of contracted mode c: the two other modes in cyclic order after c, the first of them
    padded to a multiple of 4 (as the fp32 copies), in whole 512-row blocks."""
    return _round_up(_round_up(dims[(c + 1) % 3], 4) * dims[(c + 2) % 3], ROW_BLOCK)


def _cp_block(dims, R, X):
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[[1, 2, 3]], size=list(dims),
                coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
                constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[X], _ranks=[R] * 3)


@functools.lru_cache(maxsize=None)
def _tensor(dims):
    """(X, D = dequantised X, s), read-only."""
    X = np.asfortranarray(np.random.default_rng(sum(dims)).standard_normal(dims))
    D, s = dequantize(X)
    X.setflags(write=False)
    D.setflags(write=False)
    return X, D, s


@functools.lru_cache(maxsize=None)
def _reference(dims, R):
    """(U, [mttkrp(D, U, n) for n]) in fp64 on the CPU, once per (dims, R)."""
    rng = np.random.default_rng(1000 * sum(dims) + R)
    U = [rng.standard_normal((n, R)) for n in dims]
    D = _tensor(dims)[1]
    ref = [o_mttkrp(D, U, n) for n in range(3)]
    for a in U + ref:
        a.setflags(write=False)
    return U, ref


def _resident_mttkrp_checked(eng, dims, R, n):
    """eng.resident_mttkrp of mode n plus the proof that it was ONE pass on a half copy; returns (result, chunks)."""
    eng.kernel_stats(0, reset=True)
    eng.kernel_stats(1, reset=True)
    got = eng.resident_mttkrp(0, n, dims[n], R)
    _, launches, nbytes, flops = eng.kernel_stats(0)
    assert launches == 1, launches
    assert eng.kernel_stats(1)[1] == 0
    c = 2 if n != 2 else 1                                       # no update sequence: the last mode that is not n
    C = dims[c]
    rows = _copy_rows(dims, c)
    assert flops == 2.0 * rows * C * R, (flops, rows, C, R)
    t_bytes = nbytes - 2.0 * rows * C                            # bytes = 2 rows C + 4 nchunk rows R
    assert t_bytes > 0 and t_bytes % (4 * rows * R) == 0, (nbytes, rows, C, R)
    nchunk = int(t_bytes // (4 * rows * R))
    assert nchunk >= -(-C // 2048), (nchunk, C)                  # at most 2048 fp32-accumulated terms per chunk
    return got, nchunk


# ---- 1. storage ---------------------------------------------------------------------------------------------------------
def test_storage_info_scale_and_norm(pkg, eng, capi):
    dims, R = (150, 70, 66), 4
    X, D, s = _tensor(dims)
    pkg.build_model(eng, _cp_block(dims, R, X), 'f16')
    prec, scale, nbytes = eng.tensor_storage_info(0)
    assert prec == capi.PREC_F16
    assert scale == s
    # three half copies, rows in whole 512-row blocks, columns in whole groups of 32: nothing else is resident
    padded = [_copy_rows(dims, c) * _round_up(dims[c], GROUP) for c in range(3)]
    assert nbytes == 2 * sum(padded), (nbytes, padded)
    # 6 bytes per padded entry (an entry of the copies' common padded size); the slack of this shape: rows to whole
    # 512-row blocks (<= 5 %), columns to whole groups of 32 (150 -> 160, 70 -> 96, 66 -> 96)
    assert 0 < nbytes < 6.6 * (sum(padded) / 3.0)
    nsq = np.zeros(1)
    capi.check(eng.lib.aoadmm_tensor_normsq(eng.h, 0, capi.dptr(nsq)))
    ref = float(np.sum(D * D))
    print('f16 ||X||^2: %.17g against %.17g, resident %d bytes = %.3f per entry' % (nsq[0], ref, nbytes, nbytes / X.size))
    assert abs(nsq[0] - ref) <= 1e-13 * ref


def test_all_zero_tensor(pkg, eng, capi):
    dims = (9, 8, 7)
    pkg.build_model(eng, _cp_block(dims, 3, np.zeros(dims)), 'f16')
    prec, scale, nbytes = eng.tensor_storage_info(0)
    assert (prec, scale) == (capi.PREC_F16, 1.0) and nbytes > 0
    nsq = np.ones(1)
    capi.check(eng.lib.aoadmm_tensor_normsq(eng.h, 0, capi.dptr(nsq)))
    assert nsq[0] == 0.0


def _f32_model_still_works(pkg, eng, capi):
    """An fp32 model on the same engine: resident_mttkrp at the fp32 bar, storage info F32 / scale 1."""
    dims, R = (12, 9, 245), 20
    X = _tensor(dims)[0]
    rng = np.random.default_rng(5)
    U = [rng.standard_normal((n, R)) for n in dims]
    Z = _cp_block(dims, R, X)
    pkg.build_model(eng, Z, 'f32')
    pkg.upload_state(eng, Z, dict(fac=U))
    prec, scale, _ = eng.tensor_storage_info(0)
    assert (prec, scale) == (capi.PREC_F32, 1.0)
    for n in range(3):
        assert rel_fro(eng.resident_mttkrp(0, n, dims[n], R), o_mttkrp(X, U, n)) < TOL_F32


def test_non_finite_entry_is_refused(pkg, eng, capi):
    dims = (9, 8, 7)
    X = np.random.default_rng(3).standard_normal(dims)
    X[4, 3, 2] = np.inf
    with pytest.raises(pkg.AoadmmError) as ei:
        pkg.build_model(eng, _cp_block(dims, 3, X), 'f16')
    assert ei.value.code == capi.ERR_INVALID
    _f32_model_still_works(pkg, eng, capi)


# ---- 2. resident MTTKRP, every mode --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims,R', CASES, ids=['%dx%dx%d-R%d' % (*d, R) for d, R in CASES])
def test_resident_mttkrp_matches_oracle_on_dequantised_data(pkg, eng, dims, R):
    """aoadmm_resident_mttkrp on a half block against oracle.tensor_ops.mttkrp on D = q / s, every mode, at the project's
    fp32 bar 2e-6.  A numpy emulation of the kernel's arithmetic (factor split into two fp16 fragments, fp64 sums) sits
    at 3.5e-8 to 7.3e-8 on these shapes; a one-fragment factor would leave 2e-4.  Measured: 4.9e-8 to 1.5e-7 (the largest
    where C = 2565 is summed in fp32 runs of up to 160 terms per chunk)."""
    X, D, s = _tensor(dims)
    U, ref = _reference(dims, R)
    Z = _cp_block(dims, R, X)
    pkg.build_model(eng, Z, 'f16')
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    assert eng.tensor_storage_info(0)[1] == s
    for n in range(3):
        got, nchunk = _resident_mttkrp_checked(eng, dims, R, n)
        err = rel_fro(got, ref[n])
        print('f16 resident mttkrp %s R=%d mode %d: %d chunk(s), error %.3g' % (dims, R, n + 1, nchunk, err))
        assert err < TOL_F32, (n, err)


# ---- 3. exact integers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [7, 37, 64])
@pytest.mark.parametrize('dims', [(131, 6, 5), (10, 70, 6)])
def test_resident_mttkrp_exact_integers(pkg, eng, dims, R):
    """Integer tensor and integer factors: the tensor scale and the column scales are powers of two, the low factor
    fragment is zero, every product and partial sum is an integer below 2^24 times a power of two, so the result must
    EQUAL the oracle's.  A wrong lane map, a transposed copy index or an inexact descale gives a wrong integer."""
    I, J, K = dims
    X = np.arange(I * J * K, dtype=np.float64).reshape(dims, order='F') % 17 - 8
    U = [np.arange(n * R, dtype=np.float64).reshape((n, R), order='F') % 5 - 2 for n in dims]
    D, s = dequantize(X)
    assert np.array_equal(D, X)
    ref = [o_mttkrp(X, U, n) for n in range(3)]
    assert max(np.abs(o_mttkrp(np.abs(X), [np.abs(u) for u in U], n)).max() for n in range(3)) < 2 ** 24
    assert max(np.abs(r).max() for r in ref) < 2 ** 24
    Z = _cp_block(dims, R, X)
    pkg.build_model(eng, Z, 'f16')
    pkg.upload_state(eng, Z, dict(fac=U))
    for n in range(3):
        got, _ = _resident_mttkrp_checked(eng, dims, R, n)
        assert np.array_equal(got, ref[n]), (n, np.abs(got - ref[n]).max())


def test_subnormal_low_fragment_is_kept(pkg, eng):
    """One tensor entry (1.0: s = 2^14) against a factor entry v = (1 + 2^-20) 2^-14 in a column whose largest entry is 1
    (t_r = 2^14): hi = 1, lo = 2^-20, a subnormal fp16.  16384 (1 + 2^-20) fits an fp32 accumulator and both descales are
    exact, so the MTTKRP returns v exactly if and only if the MFMA keeps subnormal fp16 inputs (flushed: 2^-14)."""
    dims, R = (4, 4, 4), 2
    X = np.zeros(dims)
    X[0, 0, 0] = 1.0
    v = (1.0 + 2.0 ** -20) * 2.0 ** -14
    U = [np.ones((4, R)), np.ones((4, R)), np.zeros((4, R))]
    U[2][0, :] = v
    U[2][1, :] = 1.0
    assert np.array_equal(dequantize(X)[0], X)
    Z = _cp_block(dims, R, X)
    pkg.build_model(eng, Z, 'f16')
    pkg.upload_state(eng, Z, dict(fac=U))
    got = eng.resident_mttkrp(0, 0, 4, R)
    assert np.array_equal(got, o_mttkrp(X, U, 0)) and got[0, 0] == v, (got[0, 0], v)


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------------
def test_two_runs_return_the_same_bits(pkg, eng):
    dims, R = (131, 37, 29), 20
    X = _tensor(dims)[0]
    U, _ = _reference(dims, R)
    Z = _cp_block(dims, R, X)
    pkg.build_model(eng, Z, 'f16')
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    for n in range(3):
        a = eng.resident_mttkrp(0, n, dims[n], R)
        b = eng.resident_mttkrp(0, n, dims[n], R)
        assert np.array_equal(a, b), n


# ---- 5. the mode-1 pass, which only a solve reaches -------------------------------------------------------------------------------
SOLVE_ITERS = 3
SOLVE_CASES = [((2565, 6, 10), 5), ((2565, 6, 10), 20), ((70, 64, 66), 40), ((70, 64, 66), 52), ((70, 64, 66), 64)]


@functools.lru_cache(maxsize=None)
def _solve_reference(dims, R):
    """As test_gpu_tensor_pass._solve_reference, with the dequantised tensor as the data of the oracle's model."""
    rng = np.random.default_rng(sum(dims) + R)
    Z, io, _ = cp_model(dims, R, rng, [('non-negativity',)] * 3)
    Zd = dict(Z)
    Zd['object'] = [dequantize(Z['object'][0])[0]]
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, Fo, _, oo = OA.cmtf_AOADMM(Zd, alg_options=options(MaxOuterIters=SOLVE_ITERS), init=copy.deepcopy(G))
    return Z, G, Fo, oo


@pytest.mark.parametrize('dims,R', SOLVE_CASES, ids=['%dx%dx%d-R%d' % (*d, R) for d, R in SOLVE_CASES])
def test_solve_reaches_the_mode1_pass(pkg, eng, dims, R):
    """Three outer iterations, non-negativity on every mode: five passes (see test_gpu_tensor_pass), exactly one of them
    the mode-1 pass on copy[0], all on half copies whatever the size of the block (no one-launch kernel, no pass on X).
    Factors within 1e-4 of the oracle on the dequantised tensor, the bar of every fp32 solver test here."""
    Z, G, Fo, oo = _solve_reference(dims, R)
    eng.kernel_stats(0, reset=True)
    eng.kernel_stats(1, reset=True)
    _, Fg, _, og = pkg.cmtf_AOADMM(dict(Z), alg_options=options(MaxOuterIters=SOLVE_ITERS), init=copy.deepcopy(G),
                                   engine=eng, precision='f16')
    _, launches, _, flops = eng.kernel_stats(0)
    assert (launches, eng.kernel_stats(1)[1]) == (5, 0), (launches, eng.kernel_stats(1)[1])
    I, J, K = dims
    rows = [_copy_rows(dims, c) for c in range(3)]
    assert flops == 2.0 * R * (rows[0] * I + 2 * rows[1] * J + 2 * rows[2] * K), flops
    err = max(rel_fro(b, a) for a, b in zip(Fo['fac'], Fg['fac']))
    print('f16 solve %s R=%d: max factor error %.3g' % (dims, R, err))
    assert og['OuterIterations'] == oo['OuterIterations']
    assert err < 1e-4, err


# ---- 6. refusals and hygiene ---------------------------------------------------------------------------------------------------
def _upload_f16(eng, capi, X):
    X = capi.as_f(X)
    capi.check(eng.lib.aoadmm_tensor_upload(eng.h, 0, capi.dptr(X), capi.PREC_F16))


@pytest.mark.parametrize('dims', [(9, 8), (5, 4, 3, 6)])
def test_f16_refused_for_blocks_that_are_not_3way(pkg, eng, capi, dims):
    """Through the C ABI (build_model sends such blocks up as fp32): refused, and the fp32 data of the block stays."""
    n = len(dims)
    rng = np.random.default_rng(11)
    X = rng.standard_normal(dims)
    Z = dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(dims),
             coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
             constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[X], _ranks=[3] * n)
    pkg.build_model(eng, Z, 'f16')                               # not 3-way: stored as fp32
    assert eng.tensor_storage_info(0)[:2] == (capi.PREC_F32, 1.0)
    with pytest.raises(pkg.UnsupportedOnDevice):
        _upload_f16(eng, capi, X)
    assert eng.tensor_storage_info(0)[:2] == (capi.PREC_F32, 1.0)   # left as it was
    U = [rng.standard_normal((d, 3)) for d in dims]
    pkg.upload_state(eng, Z, dict(fac=U))
    assert rel_fro(eng.resident_mttkrp(0, 0, dims[0], 3), o_mttkrp(X, U, 0)) < TOL_F32
    _f32_model_still_works(pkg, eng, capi)


def test_f16_refused_on_a_multi_device_context(pkg, eng, capi):
    dims = (12, 9, 11)
    X = np.random.default_rng(12).standard_normal(dims)
    with pkg.Engine([0, 0]) as e2:
        with pytest.raises(pkg.UnsupportedOnDevice):
            pkg.build_model(e2, _cp_block(dims, 3, X), 'f16')
        pkg.build_model(e2, _cp_block(dims, 3, X), 'f32')        # the context works on
    _f32_model_still_works(pkg, eng, capi)


def test_f16_refused_at_op_level_and_for_row_blocks(pkg, eng, capi):
    dims = (12, 9, 11)
    rng = np.random.default_rng(13)
    X = rng.standard_normal(dims)
    U = [rng.standard_normal((n, 4)) for n in dims]
    with pytest.raises(pkg.UnsupportedOnDevice):
        eng.mttkrp(X, U, 0, precision='f16')
    with pytest.raises(pkg.UnsupportedOnDevice):
        eng.unfold_gram(X, 0, precision='f16')
    pkg.build_model(eng, _cp_block(dims, 4, X), 'f32')
    Xf = capi.as_f(X)
    with pytest.raises(pkg.UnsupportedOnDevice):
        capi.check(eng.lib.aoadmm_tensor_upload_rows(eng.h, 0, capi.dptr(Xf), 0, dims[0], capi.PREC_F16))
    assert eng.tensor_storage_info(0)[:2] == (capi.PREC_F32, 1.0)
    _f32_model_still_works(pkg, eng, capi)


def test_mask_and_no_permuted_copy_are_refused_on_a_half_block(pkg, eng, capi):
    import ctypes as C
    dims, R = (20, 14, 12), 3
    rng = np.random.default_rng(14)
    Z, io, _ = cp_model(dims, R, rng, [('non-negativity',)] * 3)
    Zr = dict(Z, _ranks=[R] * 3)
    pkg.build_model(eng, Zr, 'f16')
    assert eng.tensor_storage_info(0)[0] == capi.PREC_F16
    mk = np.asfortranarray(np.ones(dims, dtype=np.uint8))
    with pytest.raises(pkg.AoadmmError) as ei:
        capi.check(eng.lib.aoadmm_tensor_mask_upload(eng.h, 0, mk.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert ei.value.code == capi.ERR_INVALID
    with pytest.raises(pkg.UnsupportedOnDevice):                 # as for any released natural-layout array
        eng.resident_unfold_gram(0, 1, dims[1])
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    with pytest.raises(pkg.AoadmmError) as ei:
        pkg.cmtf_AOADMM(dict(Z), alg_options=options(MaxOuterIters=2, hip=dict(no_permuted_copy=1)), init=copy.deepcopy(G),
                        engine=eng, precision='f16')
    assert ei.value.code == capi.ERR_INVALID
    _f32_model_still_works(pkg, eng, capi)
    # a masked block asked for in 'f16' is stored as fp32 by build_model
    Zm = dict(Zr, miss=[np.ones(dims)])
    pkg.build_model(eng, Zm, 'f16')
    assert eng.tensor_storage_info(0)[:2] == (capi.PREC_F32, 1.0)


def test_coupled_tensor_and_matrix_model(pkg, eng, capi):
    """script3 family (CP tensor + matrix, first modes coupled): 'f16' stores the tensor as F16 and the matrix as F32, and
    the solve stays within 1e-4 of the oracle on the dequantised tensor."""
    rng = np.random.default_rng(3)
    Z, io = script3_model(rng)
    Zd = dict(Z)
    D, s = dequantize(Z['object'][0])
    Zd['object'] = [D, Z['object'][1]]
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    opt = options(MaxOuterIters=10)
    _, Fo, _, oo = OA.cmtf_AOADMM(Zd, alg_options=opt, init=copy.deepcopy(G))
    _, Fg, _, og = pkg.cmtf_AOADMM(dict(Z), alg_options=opt, init=copy.deepcopy(G), engine=eng, precision='f16')
    assert eng.tensor_storage_info(0)[:2] == (capi.PREC_F16, s)
    assert eng.tensor_storage_info(1)[:2] == (capi.PREC_F32, 1.0)
    err = max(rel_fro(b, a) for a, b in zip(Fo['fac'], Fg['fac']))
    print('f16 coupled tensor + matrix: max factor error %.3g' % err)
    assert og['OuterIterations'] == oo['OuterIterations']
    assert err < 1e-4, err


def test_f32_model_after_a_half_model(pkg, eng, capi):
    dims = (12, 9, 245)
    pkg.build_model(eng, _cp_block(dims, 20, _tensor(dims)[0]), 'f16')
    assert eng.tensor_storage_info(0)[0] == capi.PREC_F16
    _f32_model_still_works(pkg, eng, capi)
