"""GPU: the dense MTTKRP in the form the solver runs it -- every tensor pass on the row-blocked resident copies
(`CpBlock::copy[0..2]`, cpblock.hip ensure_contraction with use_cache) -- against the fp64 oracle at kernel level, at
both ends of every rank class of the contraction kernels (nt16 in 1..4, with and without the 1..4 leftover columns on
the vector pipe) and of the reductions over T, and at the chunking edges of `make_plan` (an empty last chunk, a ragged
8-column group, the in-loop flush of the two-level fp32 sums).  The op-level entry `aoadmm_op_mttkrp`
(test_gpu_ops.py) runs its passes on the natural array X and reaches none of this.

Every case proves the path it is there for from the exact launch accounting of `aoadmm_kernel_stats`
(ContractPlan::flops / algorithmic_bytes): one launch, on a copy (rows rounded up to whole 512-row blocks), with the
expected number of chunks.  If `make_plan` is retuned these identities fail and say so: pick new shapes then."""
import copy
import functools

import numpy as np
import pytest

from oracle import aoadmm as OA
from oracle.tensor_ops import mttkrp as o_mttkrp
from helpers import cp_model, options, rel_fro

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-12, 'f32': 2e-6}          # test_mttkrp_matches_oracle / README 8a
ROW_BLOCK = 512                            # misc.h kRowBlockElems

# both ends of every nt16 x EX class of contract16_f32 / contract_f64 (R = 16nt, 16nt + 1, 16nt + 4, 16nt + 5) and of
# the VEC classes of the reductions (R % 4, R % 2)
RANKS_ALL = [1, 16, 17, 20, 21, 32, 33, 36, 37, 48, 49, 52, 53, 63, 64]
# one rank per contraction class plus two odd ones
RANKS_CLASS = [20, 32, 36, 48, 52, 64, 37, 63]

# dims -> {contracted mode: chunks of its pass}.  What each shape is there for:
#  (6, 10, 2565)  copy[2]: 60 (80 in fp32) rows in one 512-row block that is mostly padding; C = 2565 -> 321 groups in 20
#                 chunks of 17, the last chunk empty, the 321st group ragged (5 columns).  Mode 3 runs on copy[1]: 31 row
#                 blocks with a ragged last one, C = 10: one full group and a 2-column one.
#  (10, 2565, 6)  copy[1] (mode 3): the permuted copy with C = 2565 and the same empty chunk.  Mode 2: reduce_inner2_k
#                 (B = 2565 >= 1024, odd).  copy[2]: 51 row blocks (61 in fp32), C = 6: only a ragged group.
#  (12, 9, 245)   31 groups in ONE chunk: nine steady-state rounds, i.e. three in-loop flushes of the two-level fp32 sums
#                 at R <= 20, then the drained round and the ragged 5-column group.
#  (131, 37, 29)  ragged everywhere (all odd: the padded extents differ between fp64 and fp32), several row blocks.
#  (150, 70, 66)  pass copies of 21 / 20 row blocks with more than one full group.
NCHUNK = {
    (6, 10, 2565): {2: 20, 1: 1},
    (10, 2565, 6): {2: 1, 1: 20},
    (12, 9, 245): {2: 1, 1: 1},
    (131, 37, 29): {2: 1, 1: 1},
    (150, 70, 66): {2: 1, 1: 1},
}

CASES = ([(d, R) for d in ((6, 10, 2565), (10, 2565, 6)) for R in RANKS_CLASS] +
         [(d, R) for d in ((12, 9, 245), (131, 37, 29)) for R in RANKS_ALL] +
         [((150, 70, 66), R) for R in (20, 37, 64)])


def _round_up(a, b):
    return (a + b - 1) // b * b


def _copy_rows(dims, c, prec):
    """Rows of the pass copy of contracted mode c: the two other modes in cyclic order after c, the first of them padded
    (cpblock.h pad_of), in whole 512-row blocks."""
    pad = _round_up(dims[(c + 1) % 3], 2 if prec == 'f64' else 4)
    return _round_up(pad * dims[(c + 2) % 3], ROW_BLOCK)


def _cp_block(dims, R, X):
    """One dense CP block, no constraints (as test_config5_2000cube_mttkrp_inner_product_identity builds it)."""
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[[1, 2, 3]], size=list(dims),
                coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
                constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[X], _ranks=[R] * 3)


@functools.lru_cache(maxsize=None)
def _tensor(dims):
    X = np.asfortranarray(np.random.default_rng(sum(dims)).standard_normal(dims))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _reference(dims, R):
    """(U, [mttkrp(X, U, n) for n]) in fp64 on the CPU, once per (dims, R) for both precisions."""
    rng = np.random.default_rng(1000 * sum(dims) + R)
    U = [rng.standard_normal((n, R)) for n in dims]
    ref = [o_mttkrp(_tensor(dims), U, n) for n in range(3)]
    for a in U + ref:
        a.setflags(write=False)
    return U, ref


def _resident_mttkrp_checked(eng, dims, R, prec, n):
    """eng.resident_mttkrp of mode n plus the proof that it was ONE pass on a resident copy: returns (result, chunks of
    the pass, contracted mode)."""
    es = 8 if prec == 'f64' else 4
    eng.kernel_stats(0, reset=True)
    eng.kernel_stats(1, reset=True)
    got = eng.resident_mttkrp(0, n, dims[n], R)
    _, launches, nbytes, flops = eng.kernel_stats(0)
    assert launches == 1, launches
    assert eng.kernel_stats(1)[1] == 0                          # never the leading-mode kernel: the copies exist
    # with no update sequence the pass contracts the last mode that is not n (next_update_distance)
    c = 2 if n != 2 else 1
    C = dims[c]
    # rows of the copy: the two other modes in cyclic order after c, the first padded, in whole 512-row blocks;
    # on X itself the same pass would have pad(I) * J (c = 2) or K * pad(I) (c = 1) rows, no multiple of 512 here
    rows = _copy_rows(dims, c, prec)
    assert flops == 2.0 * rows * C * R, (flops, rows, C, R)     # flops = 2 nbatch M C R
    t_elems = nbytes / es - rows * C                            # bytes = nbatch M C es + nchunk nbatch M R es
    assert t_elems % (rows * R) == 0, (nbytes, rows, C, R)
    return got, int(t_elems // (rows * R)), c


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('dims,R', CASES, ids=['%dx%dx%d-R%d' % (*d, R) for d, R in CASES])
def test_resident_mttkrp_matches_oracle(pkg, eng, dims, R, prec):
    """aoadmm_resident_mttkrp (the solver's path: passes on the row-blocked copies, T in (k, i) order on copy[1],
    row-major factor copies) against oracle.tensor_ops.mttkrp for every mode: 1e-12 in fp64 (summation order only),
    2e-6 in fp32 (the project's op-level bound; the input-rounding floor of these shapes -- tensor and factors rounded
    to fp32, sums in fp64 -- is 3.6e-8 to 5.0e-8)."""
    X = _tensor(dims)
    U, ref = _reference(dims, R)
    Z = _cp_block(dims, R, X)
    pkg.build_model(eng, Z, prec)
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    for n in range(3):
        got, nchunk, c = _resident_mttkrp_checked(eng, dims, R, prec, n)
        assert nchunk == NCHUNK[dims][c], (n, c, nchunk)
        err = rel_fro(got, ref[n])
        print('resident mttkrp %s R=%d %s mode %d: %.3g' % (dims, R, prec, n + 1, err))
        assert err < TOL[prec], (n, err)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('R', [7, 37, 64])
@pytest.mark.parametrize('dims', [(131, 6, 5), (10, 70, 6)])
def test_resident_mttkrp_exact_integers(pkg, eng, dims, R, prec):
    """Integer-valued tensor and asymmetric integer factors on the resident path: every product and every partial sum is
    an integer below 2^24, so fp32 is exact too and the result must EQUAL the oracle's.  A swapped fragment map or a
    transposed index in a copy kernel gives a wrong integer, not a small error."""
    I, J, K = dims
    X = np.arange(I * J * K, dtype=np.float64).reshape(dims, order='F') % 17 - 8
    U = [np.arange(n * R, dtype=np.float64).reshape((n, R), order='F') % 5 - 2 for n in dims]
    ref = [o_mttkrp(X, U, n) for n in range(3)]
    # no partial sum, in any order, exceeds the sum of the absolute values of its terms
    assert max(np.abs(o_mttkrp(np.abs(X), [np.abs(u) for u in U], n)).max() for n in range(3)) < 2 ** 24
    assert max(np.abs(r).max() for r in ref) < 2 ** 24
    Z = _cp_block(dims, R, X)
    pkg.build_model(eng, Z, prec)
    pkg.upload_state(eng, Z, dict(fac=U))
    for n in range(3):
        got, _, _ = _resident_mttkrp_checked(eng, dims, R, prec, n)
        assert np.array_equal(got, ref[n]), (n, np.abs(got - ref[n]).max())


def test_rank_limit(pkg, eng):
    """kMaxRank = 64: rank 65 is refused by the host-side argument checks (launch_contract, aoadmm_model_set_mode), and
    the engine works on afterwards."""
    rng = np.random.default_rng(65)
    dims = (9, 8, 7)
    X = rng.standard_normal(dims)
    U65 = [rng.standard_normal((n, 65)) for n in dims]
    U4 = [rng.standard_normal((n, 4)) for n in dims]

    def still_works():
        for prec in ('f64', 'f32'):
            for n in range(3):
                assert rel_fro(eng.mttkrp(X, U4, n, precision=prec), o_mttkrp(X, U4, n)) < TOL[prec]

    for prec in ('f64', 'f32'):
        with pytest.raises(pkg.AoadmmError):
            eng.mttkrp(X, U65, 0, precision=prec)
    still_works()
    with pytest.raises(pkg.AoadmmError):
        pkg.build_model(eng, _cp_block(dims, 65, X), 'f64')
    still_works()
    Z = _cp_block(dims, 4, X)                                    # and the model interface as well
    pkg.build_model(eng, Z, 'f64')
    pkg.upload_state(eng, Z, dict(fac=U4))
    assert rel_fro(eng.resident_mttkrp(0, 0, dims[0], 4), o_mttkrp(X, U4, 0)) < TOL['f64']


# ---- the mode-1 pass, which only a solve reaches ----------------------------------------------------------------------
# resident_mttkrp never contracts mode 1 (no update sequence: the last mode is preferred).  In a solve with update order
# 1-2-3 the mode-1 contraction first runs in the second outer iteration: on copy[0] in either precision, or with
# contract_lead16_f32 in fp32 when options.hip.no_permuted_copy = 1.
SOLVE_ITERS = 3
SOLVE_CASES = ([((2565, 6, 10), R, v) for R in (5, 20) for v in ('f64', 'f32')] + [((2565, 6, 10), 20, 'f32-lead')] +
               [((70, 64, 66), R, v) for R in (40, 52, 64) for v in ('f64', 'f32', 'f32-lead')])


@functools.lru_cache(maxsize=None)
def _solve_reference(dims, R):
    """Model, initial state and the oracle's factors after SOLVE_ITERS outer iterations, once per (dims, R)."""
    rng = np.random.default_rng(sum(dims) + R)
    Z, io, _ = cp_model(dims, R, rng, [('non-negativity',)] * 3)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, Fo, _, oo = OA.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=SOLVE_ITERS), init=copy.deepcopy(G))
    return Z, G, Fo, oo


def _solve_case(dims, R):
    """The cached case with a model dict and an initial state of the caller's own."""
    Z, G, Fo, oo = _solve_reference(dims, R)
    return dict(Z), copy.deepcopy(G), Fo, oo


@pytest.mark.parametrize('dims,R,variant', SOLVE_CASES, ids=['%dx%dx%d-R%d-%s' % (*d, R, v) for d, R, v in SOLVE_CASES])
def test_solve_reaches_the_mode1_pass(pkg, eng, tensor_passes, dims, R, variant):
    """Three outer iterations (non-negativity on every mode) against the oracle.
    (2565, 6, 10): copy[0] with C = I = 2565 (20 chunks, the last empty, a ragged group) and the reductions over a T
    of 20 chunks; with no_permuted_copy the lead kernel in two reduction slices (41 chunks of 64 columns, the last with
    2565 % 64 = 5).  (70, 64, 66) at R = 40, 52, 64: NT = 3, 3 + leftover columns and 4 of all three contraction kernels
    inside a solve, and the R > 32 classes of the system build, the row solve and the row loop.
    The passes of such a solve with update order 1-2-3 and the partial-contraction cache (ensure_contraction): mode 3
    contracted for the initial objective (its T serves modes 1 and 2 of the first iteration), mode 2 in the first
    iteration, mode 1 in the second (its T also serves mode 3), modes 3 and 2 again for the third -- five launches,
    exactly one of them the mode-1 pass, which the flop count of the launches pins: on copy[0] (rows in whole 512-row
    blocks) or, with no_permuted_copy, the one launch of the lead kernel beside four passes on X.
    fp64: 1e-8 on every factor and the trace checks of test_gpu_solver.compare.  fp32: 1e-4 on the factors, as every
    fp32 solver test here (the largest error of the three factors is printed per case)."""
    from test_gpu_solver import compare
    Z, G, Fo, oo = _solve_case(dims, R)
    prec = 'f64' if variant == 'f64' else 'f32'
    lead = variant == 'f32-lead'
    opt = options(MaxOuterIters=SOLVE_ITERS, hip=dict(no_permuted_copy=int(lead)))
    eng.kernel_stats(0, reset=True)
    eng.kernel_stats(1, reset=True)
    _, Fg, _, og = pkg.cmtf_AOADMM(Z, alg_options=opt, init=G, engine=eng, precision=prec)
    _, launches, _, flops = eng.kernel_stats(0)
    _, lead_launches, _, lead_flops = eng.kernel_stats(1)
    I, J, K = dims
    if lead:                                                     # on X: pad(I) * J rows by K, K batches of pad(I) rows by J
        Ip = _round_up(I, 4)
        assert (launches, lead_launches) == (4, 1), (launches, lead_launches)
        assert flops == 2.0 * R * (2 * Ip * J * K + 2 * K * Ip * J), flops
        assert lead_flops == 2.0 * R * (J * K) * I, lead_flops
    else:
        rows = [_copy_rows(dims, c, prec) for c in range(3)]
        assert (launches, lead_launches) == (5, 0), (launches, lead_launches)
        assert flops == 2.0 * R * (rows[0] * I + 2 * rows[1] * J + 2 * rows[2] * K), flops
    if prec == 'f64':
        compare(Fo, oo, Fg, og)
        return
    err = max(rel_fro(b, a) for a, b in zip(Fo['fac'], Fg['fac']))
    print('solve %s R=%d %s: max factor error %.3g' % (dims, R, variant, err))
    assert og['OuterIterations'] == oo['OuterIterations']
    assert err < 1e-4, err


def test_no_permuted_copy_does_not_outlive_its_model(pkg, eng):
    """options.hip.no_permuted_copy = 1 does not outlive the model it was solved on: the next model built on the same
    engine has its pass copies again (they are made at upload), so aoadmm_resident_mttkrp runs on them."""
    Z, G, _, _ = _solve_case((70, 64, 66), 40)
    opt = options(MaxOuterIters=1, hip=dict(no_permuted_copy=1))
    pkg.cmtf_AOADMM(Z, alg_options=opt, init=G, engine=eng, precision='f32')
    dims, R = (12, 9, 245), 20
    U, ref = _reference(dims, R)
    Zb = _cp_block(dims, R, _tensor(dims))
    pkg.build_model(eng, Zb, 'f32')
    pkg.upload_state(eng, Zb, dict(fac=list(U)))
    got, nchunk, _ = _resident_mttkrp_checked(eng, dims, R, 'f32', 0)
    assert nchunk == 1 and rel_fro(got, ref[0]) < TOL['f32']
