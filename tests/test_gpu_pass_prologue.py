"""GPU: the tensor-pass kernels at the branch point between their two ways into the column loop.

contract16_f32, contract_f64 and contract16_f16 split a wave's work on the number of full column groups of its chunk,
ng: with ng >= 5 (ng >= 4 in the two-stage fp64 form with leftover columns) an ordered, unconditional prologue feeds
the steady loop, then the drained round and the leftover stages; with fewer groups a short path runs that never passes
the loop header.  test_gpu_tensor_pass.py covers rank classes and chunk edges, not ng = 0..8; this file does.

Contracted lengths (fp32 / fp64, groups of 8 columns): C = 5 .. 65 gives 0..8 full groups with and without a ragged
group --
   C      5  8  12 16 17 24 32 39 40 41 47 48 56 64 65
   full   0  1  1  2  2  3  4  4  5  5  5  6  7  8  8
   ragged y  -  y  -  y  -  -  y  -  y  y  -  -  -  y
so 39 is the last chunk on the short path, 40 the first that enters the steady loop (one revolution, then the two
leftover stages), 64 the first with a drained round behind the loop.  fp16 storage has groups of 32 columns, padded with
zeros to whole groups: C = 31 .. 224 gives 1..7 groups in one chunk; at C = 256 make_plan, which keeps at least 128 columns
per chunk when it splits the reduction of a short mode, makes two chunks of four groups.

Shapes: (12, 9, C) contracts C on copy[2] for the MTTKRPs of modes 1 and 2; (C, 12, 9) is the same tensor length with C
as the row mode of the permuted copies (many row blocks, short reductions of 9 and 12 columns); (9, C, 12) contracts C
on the permuted copy[1] for the MTTKRP of mode 3.  AOADMM_NO_SMALL_MTTKRP sends these tiny blocks through the passes, and
every case proves that from the launch accounting of `aoadmm_kernel_stats`, as test_gpu_tensor_pass.py does.

Every case passes before and after the restructuring of the prologue: these tests pin behaviour, they do not define it."""
import functools

import numpy as np
import pytest

from oracle.tensor_ops import mttkrp as o_mttkrp
from helpers import rel_fro
from test_gpu_tensor_pass import TOL, _cp_block, _resident_mttkrp_checked
from test_gpu_f16_storage import TOL_F32 as TOL_F16, dequantize
from test_gpu_f16_storage import _resident_mttkrp_checked as _resident_mttkrp_checked_f16

pytestmark = pytest.mark.gpu

LENGTHS = [5, 8, 12, 16, 17, 24, 32, 39, 40, 41, 47, 48, 56, 64, 65]
LENGTHS_F16 = [31, 32, 64, 96, 128, 159, 160, 161, 192, 224, 256]
RANKS = {'f32': [16, 20, 17, 36, 64], 'f64': [16, 20, 36]}
RANKS_F16 = [20, 36]


def _shapes(C):
    return [(12, 9, C), (C, 12, 9), (9, C, 12)]


@functools.lru_cache(maxsize=None)
def _tensor(dims):
    X = np.asfortranarray(np.random.default_rng(7 * sum(dims) + dims[0]).standard_normal(dims))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _factors(dims, R):
    rng = np.random.default_rng(1000 * sum(dims) + R)
    U = tuple(rng.standard_normal((n, R)) for n in dims)
    for a in U:
        a.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def _reference(dims, R):
    """[mttkrp(X, U, n) for n] in fp64 on the CPU, once per (dims, R) for both precisions."""
    ref = tuple(o_mttkrp(_tensor(dims), list(_factors(dims, R)), n) for n in range(3))
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _reference_f16(dims, R):
    """The same on the dequantised data D = q / s (test_gpu_f16_storage.py: the kernel is bounded, not the rounding)."""
    D, _ = dequantize(_tensor(dims))
    ref = tuple(o_mttkrp(D, list(_factors(dims, R)), n) for n in range(3))
    for a in ref:
        a.setflags(write=False)
    return ref


CASES = [(p, R, C) for p in ('f32', 'f64') for R in RANKS[p] for C in LENGTHS]


@pytest.mark.parametrize('prec,R,C', CASES, ids=['%s-R%d-C%d' % c for c in CASES])
def test_full_groups_0_to_8(pkg, eng, tensor_passes, prec, R, C):
    """All three MTTKRPs of the three shapes against the fp64 oracle: 1e-12 in fp64, 2e-6 in fp32."""
    for dims in _shapes(C):
        U, ref = _factors(dims, R), _reference(dims, R)
        Z = _cp_block(dims, R, _tensor(dims))
        pkg.build_model(eng, Z, prec)
        pkg.upload_state(eng, Z, dict(fac=list(U)))
        for n in range(3):
            got, nchunk, c = _resident_mttkrp_checked(eng, dims, R, prec, n)
            assert nchunk == 1, (dims, n, nchunk)
            err = rel_fro(got, ref[n])
            print('pass prologue %s R=%d %s mode %d (contracts %d columns): %.3g' % (dims, R, prec, n + 1, dims[c], err))
            assert err < TOL[prec], (dims, n, err)


CASES_F16 = [(R, C) for R in RANKS_F16 for C in LENGTHS_F16]


@pytest.mark.parametrize('R,C', CASES_F16, ids=['R%d-C%d' % c for c in CASES_F16])
def test_full_groups_1_to_8_half_storage(pkg, eng, tensor_passes, R, C):
    """fp16 storage: 1..8 groups of 32 columns, on the dequantised data at the fp32 bar 2e-6."""
    def chunks(length):                                          # make_plan on a short mode: >= 4 groups per chunk
        return max(1, -(-length // 32) // 4)

    for dims in _shapes(C):
        U, ref = _factors(dims, R), _reference_f16(dims, R)
        Z = _cp_block(dims, R, _tensor(dims))
        pkg.build_model(eng, Z, 'f16')
        pkg.upload_state(eng, Z, dict(fac=list(U)))
        for n in range(3):
            got, nchunk = _resident_mttkrp_checked_f16(eng, dims, R, n)
            assert nchunk == chunks(dims[2 if n != 2 else 1]), (dims, n, nchunk)
            err = rel_fro(got, ref[n])
            print('pass prologue %s R=%d f16 mode %d: %.3g' % (dims, R, n + 1, err))
            assert err < TOL_F16, (dims, n, err)


@pytest.mark.parametrize('R', [20, 36])
def test_split_reduction_mixes_both_paths(pkg, eng, tensor_passes, R):
    """A short mode (108 rows: one row block, four wave tiles), so make_plan splits the reduction over the column groups:
    C = 1909 is 239 groups, the last ragged (5 columns); make_plan keeps at least 16 groups per chunk, so 239 // 16 = 14
    chunks of ceil(239 / 14) = 18 groups.  Chunks 0..12 run the steady loop (18 groups: five revolutions, one in-loop
    flush at R = 20, a drained round), chunk 13 holds the last 5 groups -- four full ones and the ragged one -- and takes
    the short path, in the same launch.  (make_plan never makes every chunk that short: 16 groups is its floor.)"""
    dims = (12, 9, 1909)
    U, ref = _factors(dims, R), _reference(dims, R)
    Z = _cp_block(dims, R, _tensor(dims))
    pkg.build_model(eng, Z, 'f32')
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    for n in (0, 1):
        got, nchunk, c = _resident_mttkrp_checked(eng, dims, R, 'f32', n)
        assert (c, nchunk) == (2, 14), (n, c, nchunk)
        err = rel_fro(got, ref[n])
        print('pass prologue %s R=%d f32 mode %d, %d chunks: %.3g' % (dims, R, n + 1, nchunk, err))
        assert err < TOL['f32'], (n, err)


def _integer_case(dims, R):
    I, J, K = dims
    X = np.arange(I * J * K, dtype=np.float64).reshape(dims, order='F') % 17 - 8
    U = [np.arange(n * R, dtype=np.float64).reshape((n, R), order='F') % 5 - 2 for n in dims]
    ref = [o_mttkrp(X, U, n) for n in range(3)]
    # no partial sum, in any order, exceeds the sum of the absolute values of its terms
    assert max(np.abs(o_mttkrp(np.abs(X), [np.abs(u) for u in U], n)).max() for n in range(3)) < 2 ** 24
    return X, U, ref


@pytest.mark.parametrize('prec,C', [('f32', 41), ('f32', 65), ('f64', 41), ('f64', 65), ('f16', 161), ('f16', 192)])
def test_exact_integers_across_the_branch_point(pkg, eng, tensor_passes, prec, C):
    """Small integer tensor and factors: every product and partial sum is an integer below 2^24 (times a power of two in
    fp16 storage), so each precision must EQUAL the oracle.  A stage consumed before its loads have landed gives a wrong
    integer, which no tolerance hides.  C = 41 / 161: one revolution of the steady loop, two leftover stages and (fp32,
    fp64) the ragged group; C = 65 / 192: the drained round as well."""
    for dims in ((12, 9, C), (9, C, 12)):
        for R in (20, 36):
            X, U, ref = _integer_case(dims, R)
            if prec == 'f16':
                assert np.array_equal(dequantize(X)[0], X)
            Z = _cp_block(dims, R, X)
            pkg.build_model(eng, Z, prec)
            pkg.upload_state(eng, Z, dict(fac=U))
            for n in range(3):
                if prec == 'f16':
                    got = _resident_mttkrp_checked_f16(eng, dims, R, n)[0]
                else:
                    got = _resident_mttkrp_checked(eng, dims, R, prec, n)[0]
                assert np.array_equal(got, ref[n]), (dims, R, n, np.abs(got - ref[n]).max())
