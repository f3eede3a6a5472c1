"""GPU: the dense MTTKRP of blocks of order above 3 (`mttkrp_nway`, cpblock.hip) against the fp64 oracle, at both ends of
every kernel class of its fold chain.  The path: ONE matrix-core contraction (of the last mode; of the one before it when
the last mode is the wanted one, then with one batch per index of the last mode), after which every other mode is folded
over T, one per launch: the modes behind the wanted one with `launch_reduce_outer`, last mode first, then the modes in
front of it with `launch_reduce_inner`, first mode first.  Every fold but the last leaves a smaller fp64 T in [row][r]
layout (`rowmajor_out = 1`, no leading dimension) in `tmpA` / `tmpB` by turns; the last writes the column-major result.
The 3-way tests reach none of this: their reductions read T straight from the contraction, write column-major output and
never fold twice.  The entry is `Engine.mttkrp` (`aoadmm_op_mttkrp`: block_upload + block_mttkrp, what a resident block
runs); the same path from a resident block and inside a solve is at the end of the file.

Every case proves its contraction from the exact launch accounting of `aoadmm_kernel_stats` (ContractPlan::flops /
algorithmic_bytes): one launch, 2 nbatch M C R flops, and the chunk count in SHAPES.  The folds are not in that
accounting; their classes follow from the conditions below, restated from contract.hip.  If `make_plan`,
`outer_geometry` or `launch_inner_t` is retuned, the chunk identities fail or the conditions no longer hold for the
shape named: pick a new shape then.

Conditions (Ip: the first extent padded to 2 in fp64, to 4 in fp32; c: the contracted mode; M: Ip times the extents
between the first mode and c; Cg = ceil(C / 8)):
  make_plan        ntiles = nbatch * ceil(M / 64) (fp32: 128) < 2048: nchunk = min(ceil(2048 / ntiles), max(Cg // 16, 1)),
                   in fp32 at least ceil(Cg / 256); ceil(Cg / nchunk) groups per chunk, so a last chunk can be empty
  VEC of a fold    T in fp32 (first fold of an fp32 block): float4 if R % 4 == 0, else scalar; T in fp64 (every fold of
                   an fp64 block, every later fold of an fp32 one): double2 if R % 2 == 0, else scalar
  launch_inner_t   fold of a leading mode of extent A into B output rows: R / VEC threads per row of T, 256 // rq * rq per
                   workgroup; reduce_inner2_k (two slabs per workgroup) iff B >= 1024 and 2 R <= threads (any R <= 64),
                   else reduce_inner_k; B odd: the last workgroup of reduce_inner2_k holds one slab
  outer_geometry   fold of a trailing mode of extent B over A rows: TA = 256 // ceil(R / VEC) rows per workgroup,
                   nblkA = ceil(A / TA), SB = min(ceil(2048 / nblkA), 64, B) slices of bper = ceil(B / SB); a slice past
                   ceil(B / bper) is empty, the last non-empty one is ragged when bper does not divide B
  reduce_outer_fin SB // 8 eight-slice steps, then pairs, then one odd slice

Class table (`rm`: a fold that writes [row][r] output, `fin`: the fold that writes the column-major result):
  (9,7,6,5), (7,4,6,3,5)   R in RANKS_VEC: R % 4 == 0 (4, 16, 20, 36, 64), R % 4 == 2 (2, 6), odd (1, 3, 17, 33, 37, 63), at
                 both ends of each: all four TT, VEC pairs of reduce_outer_k and reduce_inner_k (fp32 T in rm form, fp64 T
                 in rm and fin form); rq = R / VEC from 1 to 63 threads per row, i.e. TA from 256 down to 4 rows per
                 workgroup with padding threads where TA * rq is no multiple of 64, and 192 to 256 threads in the inner
                 folds; an fp32 first fold followed by fp64 folds; I = 9, 7 odd, so Ip != I in both precisions: the padded
                 rows of T sit in every fold's stride (Apad = Ip * ...) and the fold of mode 1 sums I of Ip rows
  (5,35,6,31)    mode 4 contracts mode 3 (31 batches); the fold of mode 1 has B = 35 * 31 = 1085 output rows, >= 1024 and
                 odd: reduce_inner2_k in rm form with a one-slab last workgroup, at R = 1, 20, 37, 64 (all four TT, VEC)
  (6,5,4,1085)   mode 4: reduce_inner2_k twice, rm at B = 5 * 1085 = 5425 (fp32 or fp64 T) and fin at B = 1085 (fp64 T).
                 Modes 1-3 contract C = 1085: Cg = 136, ntiles <= 2, 8 chunks of 17 groups, none empty
  (6,5,4,2565)   modes 1-3 contract C = 2565: Cg = 321, 20 chunks of 17 groups, the last EMPTY, the 321st group ragged;
                 the 20-chunk T feeds reduce_outer_k (modes 1, 2) and reduce_inner_k (mode 3), in fp32 and in fp64
  (6,5,2565,4)   mode 4: the same 20 chunks on the batched plan (nbatch = 4, M = 5 Ip).  Modes 1, 2: first fold over
                 B = 2565 with A = 5 Ip rows, nblkA <= 4: SB = 64, bper = 41, slice 62 ragged (23), slice 63 empty
  (6,5,65,3)     modes 1, 2: first fold over B = 65, SB = 64, bper = 2: slice 32 holds one b, slices 33-63 are empty
  (32,32,35,9)   modes 1, 2 at R = 64: first fold A = 1024; fp64: TA = 8, nblkA = 128, SB = 16 < B = 35, bper = 3, slice 11
                 ragged, 12-15 empty; fp32: TA = 16, nblkA = 64, SB = 32, bper = 2, slice 17 ragged, 18-31 empty
  (32,32,16,6,3) mode 1 at R = 64: first fold A = 16384; fp64: nblkA = 2048, SB = 1 (one slice, the odd-tail branch of
                 reduce_outer_fin alone); fp32: nblkA = 1024, SB = 2.  Three folds: tmpA, tmpB, result
  (6,5,B,3)      B in 1, 2, 7, 8, 9, 17, R = 5: first fold of modes 1, 2 has SB = B (nblkA = 1, B < 64): reduce_outer_fin
                 in rm form through odd tail only; one pair; pairs + tail; one eight-step; eight-step + tail; two + tail
  (4,3,2,3,2,5), (3,2,4,2,3,2,2,3)   four and six folds before the last (tmpA is reused from the third on); order 8 is
                 the API's limit.  Every mode: every split of the chain between outer and inner folds
  (1,6,5,7), (5,4,1,6)   a first mode of extent 1 (Ip = 2 or 4, T is mostly padding; an inner fold with A = 1) and a
                 singleton middle mode (an outer fold with B = 1, SB = 1; a one-row result; contracted with C = 1 for mode 4)

Shapes listed for something else reach reduce_inner2_k as well (mode 4 of (6,5,4,2565): B = 5 * 2565; mode 3 of
(32,32,35,9): B = 32 * 35; modes 4 and 5 of (32,32,16,6,3)), so it runs at all four TT, VEC pairs in rm form and at both
fp64 ones in fin form.

TOL = {'f64': 1e-12, 'f32': 2e-6} is the project's op-level bar (test_gpu_tensor_pass).  Largest errors seen on an MI355X
over the 518 mode results of the op-level and resident parity tests: fp64 1.11e-14 ((6,5,4,2565), R = 3, mode 2); fp32
2.13e-7 ((6,5,4,1085), R = 37, mode 1: 136 columns per chunk summed in fp32 inside the MFMA; the input-rounding floor of
that case -- tensor and factors rounded to fp32, sums in fp64 -- is 5.0e-8)."""
import functools

import numpy as np
import pytest

from oracle.tensor_ops import mttkrp as o_mttkrp
from helpers import cp_model, options, rel_fro
from test_gpu_tensor_pass import TOL

pytestmark = pytest.mark.gpu

RANKS_VEC = [1, 2, 3, 4, 6, 16, 17, 20, 33, 36, 37, 63, 64]

# dims -> (ranks, {contracted mode (0-based): chunks of its pass}); the last mode is contracted for every wanted mode but
# the last, the one before it for the last.  The chunk counts are the same in both precisions at these shapes.
SHAPES = {
    (9, 7, 6, 5): (RANKS_VEC, {3: 1, 2: 1}),
    (7, 4, 6, 3, 5): (RANKS_VEC, {4: 1, 3: 1}),
    (5, 35, 6, 31): ([1, 20, 37, 64], {3: 1, 2: 1}),
    (6, 5, 4, 1085): ([20, 37], {3: 8, 2: 1}),
    (6, 5, 4, 2565): ([3, 20, 64], {3: 20, 2: 1}),
    (6, 5, 2565, 4): ([3, 20, 64], {3: 1, 2: 20}),
    (6, 5, 65, 3): ([4, 37], {3: 1, 2: 1}),
    (32, 32, 35, 9): ([64], {3: 1, 2: 1}),
    (32, 32, 16, 6, 3): ([64], {4: 1, 3: 1}),
    (6, 5, 1, 3): ([5], {3: 1, 2: 1}),
    (6, 5, 2, 3): ([5], {3: 1, 2: 1}),
    (6, 5, 7, 3): ([5], {3: 1, 2: 1}),
    (6, 5, 8, 3): ([5], {3: 1, 2: 1}),
    (6, 5, 9, 3): ([5], {3: 1, 2: 1}),
    (6, 5, 17, 3): ([5], {3: 1, 2: 1}),
    (4, 3, 2, 3, 2, 5): ([4, 37], {5: 1, 4: 1}),
    (3, 2, 4, 2, 3, 2, 2, 3): ([4, 37], {7: 1, 6: 1}),
    (1, 6, 5, 7): ([3, 20], {3: 1, 2: 1}),
    (5, 4, 1, 6): ([3, 20], {3: 1, 2: 1}),
}
CASES = [(d, R) for d, (ranks, _) in SHAPES.items() for R in ranks]
EXACT_RANKS = [7, 20, 64]


def _id(dims, R):
    return 'x'.join(map(str, dims)) + '-R%d' % R


def _round_up(a, b):
    return (a + b - 1) // b * b


@functools.lru_cache(maxsize=None)
def _tensor(dims):
    X = np.asfortranarray(np.random.default_rng(sum(dims) + 100 * len(dims)).standard_normal(dims))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _reference(dims, R):
    """(U, [mttkrp(X, U, n) for n]) in fp64 on the CPU, once per (dims, R) for both precisions and both entries."""
    rng = np.random.default_rng(1000 * sum(dims) + 10 * len(dims) + R)
    U = [rng.standard_normal((n, R)) for n in dims]
    ref = [o_mttkrp(_tensor(dims), U, n) for n in range(len(dims))]
    for a in U + ref:
        a.setflags(write=False)
    return U, ref


def _int_factors(dims, R, hi):
    rng = np.random.default_rng(7000 * sum(dims) + 70 * len(dims) + R)
    return [rng.integers(-hi, hi + 1, size=(n, R)).astype(np.float64) for n in dims]


@functools.lru_cache(maxsize=None)
def _int_tensor(dims):
    X = np.asfortranarray(np.random.default_rng(5 * sum(dims) + len(dims)).integers(-8, 9, size=dims).astype(np.float64))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _int_case(dims, R):
    """Integer tensor in [-8, 8] and integer factors in [-2, 2] ([-1, 1] where the sums of absolute values would reach
    2^24), with the oracle's MTTKRPs: once per (dims, R) for both precisions."""
    X = _int_tensor(dims)
    N = len(dims)
    for hi in (2, 1):
        U = _int_factors(dims, R, hi)
        cap = max(o_mttkrp(np.abs(X), [np.abs(u) for u in U], n).max() for n in range(N))
        if cap < 2 ** 24:
            break
    # no partial sum, in any order, exceeds the sum of the absolute values of its terms
    assert cap < 2 ** 24, (dims, R, cap)
    for a in range(N):                                           # asymmetric: a swapped pair of factors is a wrong integer
        for b in range(a + 1, N):
            assert dims[a] != dims[b] or not np.array_equal(U[a], U[b]), (a, b)
    ref = [o_mttkrp(X, U, n) for n in range(N)]
    assert all(np.any(r) for r in ref)
    for a in U + ref:
        a.setflags(write=False)
    return X, U, ref


def _contraction(dims, prec, n):
    """(contracted mode, nbatch, M, C) of the pass `mttkrp_nway` runs for wanted mode n."""
    N = len(dims)
    c = N - 2 if n == N - 1 else N - 1
    M = _round_up(dims[0], 2 if prec == 'f64' else 4)
    for m in range(1, c):
        M *= dims[m]
    return c, (1 if c == N - 1 else dims[N - 1]), M, dims[c]


def _checked(eng, call, dims, R, prec, n):
    """call() plus the proof that it ran ONE contraction of the plan `mttkrp_nway` makes, on the natural array: returns
    (result, chunks of the pass, contracted mode)."""
    es = 8 if prec == 'f64' else 4
    c, nbatch, M, C = _contraction(dims, prec, n)
    eng.kernel_stats(0, reset=True)
    eng.kernel_stats(1, reset=True)
    got = call()
    _, launches, nbytes, flops = eng.kernel_stats(0)
    assert launches == 1, launches
    assert eng.kernel_stats(1)[1] == 0                           # never the leading-mode kernel
    assert flops == 2.0 * nbatch * M * C * R, (flops, nbatch, M, C, R)
    t_elems = nbytes / es - nbatch * M * C                       # bytes = nbatch M C es + nchunk nbatch M R es
    assert t_elems % (nbatch * M * R) == 0, (nbytes, nbatch, M, C, R)
    return got, int(t_elems // (nbatch * M * R)), c


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('dims,R', CASES, ids=[_id(d, R) for d, R in CASES])
def test_nway_mttkrp_matches_oracle(pkg, eng, dims, R, prec):
    """Every mode of every shape of the class table against oracle.tensor_ops.mttkrp: 1e-12 in fp64 (summation order
    only), 2e-6 in fp32 (the project's op-level bound)."""
    X = _tensor(dims)
    U, ref = _reference(dims, R)
    for n in range(len(dims)):
        got, nchunk, c = _checked(eng, lambda: eng.mttkrp(X, U, n, precision=prec), dims, R, prec, n)
        assert nchunk == SHAPES[dims][1][c], (n, c, nchunk)
        err = rel_fro(got, ref[n])
        print('nway mttkrp %s R=%d %s mode %d: %.3g' % (dims, R, prec, n + 1, err))
        assert err < TOL[prec], (n, err)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('R', EXACT_RANKS)
@pytest.mark.parametrize('dims', list(SHAPES), ids=['x'.join(map(str, d)) for d in SHAPES])
def test_nway_mttkrp_exact_integers(pkg, eng, dims, R, prec):
    """Integer-valued tensor and integer factors: every product and every partial sum is an integer below 2^24, so fp32
    is exact too and the result must EQUAL the oracle's.  A rel-Frobenius bar cannot see a few wrong entries among many
    (one lost slab, one slice read twice, one row of a [row][r] buffer in the wrong place); this can."""
    X, U, ref = _int_case(dims, R)
    for n in range(len(dims)):
        got, _, _ = _checked(eng, lambda: eng.mttkrp(X, U, n, precision=prec), dims, R, prec, n)
        assert np.array_equal(got, ref[n]), (n, np.abs(got - ref[n]).max())


# ---- the same path from a resident block and inside a solve ----------------------------------------------------------
def _cp_block(dims, R, X):
    """One dense CP block of any order, no constraints."""
    N = len(dims)
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, N + 1))], size=list(dims),
                coupling=dict(lin_coupled_modes=[0] * N, coupling_type=[], coupl_trafo_matrices=[None] * N),
                constrained_modes=[0] * N, constraints=[None] * N, weights=[1.0], object=[X], _ranks=[R] * N)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('dims', [(6, 5, 4, 2565), (7, 4, 6, 3, 5)], ids=['6x5x4x2565', '7x4x6x3x5'])
def test_resident_nway_mttkrp_matches_oracle(pkg, eng, dims, prec):
    """`aoadmm_resident_mttkrp` of a resident block of order 4 and 5 at R = 20: the same bars, the same launch accounting.
    A resident N-way block keeps no pass copies, so the pass reads the natural array (M is not rounded to row blocks)."""
    R = 20
    X = _tensor(dims)
    U, ref = _reference(dims, R)
    Z = _cp_block(dims, R, X)
    pkg.build_model(eng, Z, prec)
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    for n in range(len(dims)):
        got, nchunk, c = _checked(eng, lambda: eng.resident_mttkrp(0, n, dims[n], R), dims, R, prec, n)
        assert nchunk == SHAPES[dims][1][c], (n, c, nchunk)
        err = rel_fro(got, ref[n])
        print('resident nway mttkrp %s R=%d %s mode %d: %.3g' % (dims, R, prec, n + 1, err))
        assert err < TOL[prec], (n, err)


def test_solve_five_way(pkg, eng):
    """The first dense block of order 5 through the solver: (9,7,6,5,4), R = 4, non-negativity on modes 1 and 4, eight
    outer iterations, against the oracle with the bars of test_gpu_solver.compare (1e-8 on every factor)."""
    from test_gpu_solver import compare, run_both
    rng = np.random.default_rng(95)
    Z, io, _ = cp_model((9, 7, 6, 5, 4), 4, rng, [('non-negativity',), None, None, ('non-negativity',), None])
    compare(*run_both(pkg, eng, Z, io, options(MaxOuterIters=8)))


SOLVE4_OPT = dict(MaxOuterIters=3, MaxInnerIters=5)


@functools.lru_cache(maxsize=None)
def _solve4_reference():
    """Model, initial state and the oracle's result for the 4-way solve, once for both precisions."""
    import copy
    from oracle import aoadmm as OA
    rng = np.random.default_rng(94)
    Z, io, _ = cp_model((35, 6, 5, 1085), 20, rng, [('non-negativity',), None, None, ('non-negativity',)])
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, Fo, _, oo = OA.cmtf_AOADMM(Z, alg_options=options(**SOLVE4_OPT), init=copy.deepcopy(G))
    return Z, G, Fo, oo


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_solve_four_way_long_last_mode(pkg, eng, prec):
    """(35,6,5,1085) at R = 20 inside a solve (non-negativity on modes 1 and 4, 3 outer and 5 inner iterations): the
    MTTKRPs of modes 1-3 contract C = 1085 in 8 chunks (M = 36 * 30 rows in fp64: 17 tiles) and fold an 8-chunk T; mode 4
    contracts mode 3 in 1085 batches and folds mode 1 with reduce_inner2_k in [row][r] form (A = 35 of Ip = 36 rows,
    B = 6 * 1085 = 6510), then mode 2 with it into the result (B = 1085).  fp64: test_gpu_solver.compare.  fp32: 1e-4 on
    the factors, as every fp32 solver test here."""
    import copy
    from test_gpu_solver import compare
    Z, G, Fo, oo = _solve4_reference()
    _, Fg, _, og = pkg.cmtf_AOADMM(dict(Z), alg_options=options(**SOLVE4_OPT), init=copy.deepcopy(G), engine=eng,
                                   precision=prec)
    if prec == 'f64':
        compare(Fo, oo, Fg, og)
        return
    err = max(rel_fro(b, a) for a, b in zip(Fo['fac'], Fg['fac']))
    print('solve (35, 6, 5, 1085) R=20 f32: max factor error %.3g' % err)
    assert og['OuterIterations'] == oo['OuterIterations']
    assert err < 1e-4, err
