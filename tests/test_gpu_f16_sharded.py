"""GPU: half-precision storage (AOADMM_PREC_F16) of ROW-SHARDED dense 3-way CP blocks under a communicator.

Ranks are threads of this process, each with its own `Engine(0)`, joined by the library's process-local group
(`comm_init_local`, as in test_gpu_sharded.py).  On such engines the upload of a half block is a collective: every rank
takes the largest magnitude of what it holds (its rows and its mode-3 slab), one all-reduce makes the scale the same
everywhere, the mode-1 pass streams a half copy of the rank's slab X(:, :, K_g) and the other two passes stream half
copies of its rows.

The reference everywhere is the fp64 oracle on the DEQUANTISED tensor D = q / s, q and s computed here in numpy from the
WHOLE tensor by the rule of include/aoadmm_hip.h.  Bars, all the project's own: 1e-4 on factors (every fp32 / fp16 solver
test), 2e-6 at op level, 1e-6 sharded against unsharded, 1e-13 relative on ||X||^2, ranks bit-identical.  Measured on an
MI355X: MTTKRP 5.3e-8 - 8.2e-8, solver factors 2.7e-7 - 8.7e-6 against the oracle and 1.2e-11 - 4.5e-7 against one engine,
coupled model 2.8e-5, ||X||^2 equal to the last bit, one-rank communicator against none 0."""
import copy
import ctypes as C
import functools
import importlib
import itertools
import threading

import numpy as np
import pytest

from oracle import aoadmm as OA
from oracle.tensor_ops import mttkrp as o_mttkrp
from helpers import cp_model, options, rel_fro, script3_model

pytestmark = pytest.mark.gpu

TOL_F32 = 2e-6                              # the project's fp32 op-level bar
ROW_BLOCK = 512                             # misc.h kRowBlockElems
GROUP = 32                                  # misc.h kHalfGroupCols
JOIN_S = 120.0
_keys = itertools.count(5000)
NONNEG = (('non-negativity',),) * 3
TV_NONNEG = (('TV regularization', 0.01), ('non-negativity',), ('non-negativity',))


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


# ---- what a rank holds ---------------------------------------------------------------------------------------------------
def _share(n, world, r):
    """(first, count) of rank r's block of n items: blocks of ceil(n / world)."""
    per = -(-n // world)
    lo = min(n, per * r)
    return lo, min(n, lo + per) - lo


def _slab(K, world, r):
    """Rank r's mode-3 slab (first, count), or None where some rank would own none (cpblock.hip want_ksharded_xp)."""
    per = -(-K // world)
    if world <= 1 or per * (world - 1) >= K:
        return None
    return _share(K, world, r)


def _rank_copies(dims, world, r):
    """[(rows, C)] of rank r's three half pass copies: rows in whole 512-row blocks, C the contracted extent.  Copy 0 is
    the slab X(:, :, K_g) with all of mode 1 where the ranks own slabs, else the rank's rows like the other two."""
    I, J, K = dims
    Iloc = _share(I, world, r)[1]
    ks = _slab(K, world, r)
    c0 = (_round_up(_round_up(J, 4) * ks[1], ROW_BLOCK), I) if ks else (_round_up(_round_up(J, 4) * K, ROW_BLOCK), Iloc)
    return [c0, (_round_up(_round_up(K, 4) * Iloc, ROW_BLOCK), J), (_round_up(_round_up(Iloc, 4) * J, ROW_BLOCK), K)]


def _cp_block(dims, R, X):
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[[1, 2, 3]], size=list(dims),
                coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
                constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[X], _ranks=[R] * 3)


# ---- ranks as threads ------------------------------------------------------------------------------------------------------
def run_ranks(pkg, world, body):
    """body(engine, rank) on `world` engines joined by a process-local group, one daemon thread each, all at once.
    Returns the list of results; a rank that raised, or that has not finished after 120 s, fails the test."""
    key = next(_keys)
    res, err = [None] * world, [None] * world

    def rank_main(r):
        try:
            with pkg.Engine(0) as e:
                e.comm_init_local(key, r, world)
                res[r] = body(e, r)
        except BaseException as ex:   # noqa: BLE001 -- reported by the main thread
            err[r] = ex

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(JOIN_S)
    for r, t in enumerate(th):
        assert not t.is_alive(), 'rank %d has not finished after %g s' % (r, JOIN_S)
    for r, ex in enumerate(err):
        assert ex is None, 'rank %d: %r' % (r, ex)
    return res


def _assert_ranks_identical(res):
    """res[r] = (Fac, out): replicated state and objective history must be the same bits on every rank."""
    F0, o0 = res[0]
    for r in range(1, len(res)):
        Fr, orr = res[r]
        for key_ in ('fac', 'constraint_fac', 'constraint_dual_fac'):
            for a, b in zip(F0[key_], Fr[key_]):
                if a is None:
                    continue
                assert np.array_equal(a, b), (key_, r)
        assert np.array_equal(o0['func_val_conv'], orr['func_val_conv']), r


def _solve_on_ranks(pkg, Z, G, opt, world, precision='f16', probe=None):
    """The same solve on every rank; returns [(Fac, out, probe(engine, rank))]."""
    def body(e, r):
        e.kernel_stats(0, reset=True)
        e.kernel_stats(1, reset=True)
        _, Fg, _, og = pkg.cmtf_AOADMM(dict(Z), alg_options=opt, init=copy.deepcopy(G), engine=e, precision=precision)
        return Fg, og, probe(e, r) if probe else None
    return run_ranks(pkg, world, body)


# ---- 1. the scale and the norm are those of the whole tensor ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _outlier_tensor():
    dims = (37, 14, 13)
    X = np.asfortranarray(np.random.default_rng(101).standard_normal(dims))
    X[36, 0, 12] = 40.0                      # the last rank's rows and the last rank's slab only
    D, s = dequantize(X)
    X.setflags(write=False)
    D.setflags(write=False)
    return dims, X, D, s


@pytest.mark.parametrize('world', [2, 3])
def test_scale_and_norm_are_global(pkg, capi, world):
    """One entry of 40.0 among standard-normal data, in the last rank's rows and slab: a scale taken from a rank's own
    data would be 8 x too large on rank 0.  Every rank reports the global scale, ||X||^2 of the WHOLE dequantised tensor
    and 2 bytes per padded entry of its own three copies."""
    dims, X, D, s = _outlier_tensor()
    assert quantize(X[:_share(37, world, 0)[1]])[1] >= 8 * s      # what rank 0 would choose from its own rows alone
    ref = float(np.sum(D * D))

    def body(e, r):
        pkg.build_model(e, _cp_block(dims, 3, X), 'f16')
        nsq = np.zeros(1)
        capi.check(e.lib.aoadmm_tensor_normsq(e.h, 0, capi.dptr(nsq)))
        return e.tensor_storage_info(0), float(nsq[0])

    for r, ((prec, scale, nbytes), nsq) in enumerate(run_ranks(pkg, world, body)):
        copies = _rank_copies(dims, world, r)
        if world == 2:
            assert copies[0] == (_round_up(16 * (7, 6)[r], ROW_BLOCK), 37)
        print('f16 sharded storage, rank %d of %d: scale %g (global %g), ||X||^2 %.17g against %.17g, %d bytes resident'
              % (r, world, scale, s, nsq, ref, nbytes))
        assert (prec, scale) == (capi.PREC_F16, s)
        assert abs(nsq - ref) <= 1e-13 * ref, (nsq, ref)
        assert nbytes == 2 * sum(rows * _round_up(Cc, GROUP) for rows, Cc in copies), (nbytes, copies)


# ---- 2. MTTKRP through the row-sharded passes --------------------------------------------------------------------------------
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


MTTKRP_CASES = ([((37, 14, 13), R, 3) for R in (20, 32, 48, 64)] + [((131, 37, 29), R, 3) for R in (20, 32, 48, 64)] +
                [((2565, 6, 10), 20, 2)])


@pytest.mark.parametrize('dims,R,world', MTTKRP_CASES, ids=['%dx%dx%d-R%d-w%d' % (*d, R, w) for d, R, w in MTTKRP_CASES])
def test_resident_mttkrp_on_row_sharded_half_copies(pkg, dims, R, world):
    """aoadmm_resident_mttkrp (collective: the full result on every rank) against the oracle on D, every mode, at 2e-6; the
    same bits on every rank; per rank ONE pass on its own half copy (2 bytes per entry in whole 512-row blocks, T in fp32,
    at most 2048 terms per chunk)."""
    X, D, s = _tensor(dims)
    U, ref = _reference(dims, R)

    def body(e, r):
        Z = _cp_block(dims, R, X)
        pkg.build_model(e, Z, 'f16')
        pkg.upload_state(e, Z, dict(fac=list(U)))
        assert e.tensor_storage_info(0)[1] == s
        got, stats = [], []
        for n in range(3):
            e.kernel_stats(0, reset=True)
            e.kernel_stats(1, reset=True)
            got.append(e.resident_mttkrp(0, n, dims[n], R))
            stats.append((e.kernel_stats(0)[1:], e.kernel_stats(1)[1]))
        return got, stats

    res = run_ranks(pkg, world, body)
    for r, (got, stats) in enumerate(res):
        copies = _rank_copies(dims, world, r)
        for n in range(3):
            (launches, nbytes, flops), lead = stats[n]
            assert (launches, lead) == (1, 0), (r, n, launches, lead)
            rows, Cc = copies[2 if n != 2 else 1]                # no update sequence: the last mode that is not n
            assert flops == 2.0 * rows * Cc * R, (r, n, flops, rows, Cc)
            t_bytes = nbytes - 2.0 * rows * Cc                   # bytes = 2 rows C + 4 nchunk rows R
            assert t_bytes > 0 and t_bytes % (4 * rows * R) == 0, (r, n, nbytes, rows, Cc)
            assert t_bytes // (4 * rows * R) >= -(-Cc // 2048)
            assert np.array_equal(got[n], res[0][0][n]), (r, n)
    for n in range(3):
        err = rel_fro(res[0][0][n], ref[n])
        print('f16 sharded resident mttkrp %s R=%d world %d mode %d: error %.3g' % (dims, R, world, n + 1, err))
        assert err < TOL_F32, (n, err)


# ---- 3. solves, which alone reach the mode-1 pass on the slab copy -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solve_reference(dims, R, constraints, iters, seed):
    """(Z, G, oracle factors, oracle out) with the dequantised tensor as the data of the oracle's model."""
    rng = np.random.default_rng(seed)
    Z, io, _ = cp_model(dims, R, rng, list(constraints))
    Zd = dict(Z)
    Zd['object'] = [dequantize(Z['object'][0])[0]]
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, Fo, _, oo = OA.cmtf_AOADMM(Zd, alg_options=options(MaxOuterIters=iters), init=copy.deepcopy(G))
    return Z, G, Fo, oo


def _check_sharded_solve(pkg, eng, capi, dims, R, world, constraints=NONNEG, iters=3, seed=None):
    Z, G, Fo, oo = _solve_reference(dims, R, constraints, iters, sum(dims) + R if seed is None else seed)
    opt = options(MaxOuterIters=iters)
    s = quantize(Z['object'][0])[1]
    res = _solve_on_ranks(pkg, Z, G, opt, world,
                          probe=lambda e, r: (e.tensor_storage_info(0), e.kernel_stats(0)[1:], e.kernel_stats(1)[1]))
    _assert_ranks_identical([(F, o) for F, o, _ in res])
    Fg, og, _ = res[0]
    _, F1, _, o1 = pkg.cmtf_AOADMM(dict(Z), alg_options=opt, init=copy.deepcopy(G), engine=eng, precision='f16')
    err = max(rel_fro(b, a) for a, b in zip(Fo['fac'], Fg['fac']))
    gap = max(rel_fro(b, a) for a, b in zip(F1['fac'], Fg['fac']))
    print('f16 sharded solve %s R=%d world %d: max factor error %.3g against the oracle, %.3g against one engine'
          % (dims, R, world, err, gap))
    I, J, K = dims
    for r, (_, _, (info, (launches, _, flops), lead)) in enumerate(res):
        assert info[:2] == (capi.PREC_F16, s), (r, info)
        assert lead == 0, (r, lead)
        if iters == 3:
            # five passes (test_gpu_tensor_pass), exactly one of them the mode-1 pass: on the slab copy with C = I where
            # the ranks own slabs, on the row-sharded copy with C = the rank's rows where they do not
            (r0, C0), (r1, C1), (r2, C2) = _rank_copies(dims, world, r)
            assert (C1, C2) == (J, K)
            assert launches == 5, (r, launches)
            assert flops == 2.0 * R * (r0 * C0 + 2 * r1 * J + 2 * r2 * K), (r, flops, r0, C0, r1, r2)
    assert og['OuterIterations'] == oo['OuterIterations'] == o1['OuterIterations']
    assert err < 1e-4, err
    assert gap < 1e-6, gap


SOLVE_CASES = [((2565, 6, 10), 5, 2), ((2565, 6, 10), 20, 2), ((70, 64, 66), 40, 3), ((70, 64, 66), 64, 3)]


@pytest.mark.parametrize('dims,R,world', SOLVE_CASES, ids=['%dx%dx%d-R%d-w%d' % (*d, R, w) for d, R, w in SOLVE_CASES])
def test_sharded_solve_reaches_the_mode1_pass_on_the_slab_copy(pkg, eng, capi, dims, R, world):
    """Three outer iterations, non-negativity on every mode.  (2565, 6, 10) over two ranks: the slab copy contracts
    C = 2565 in two chunks; (70, 64, 66) over three: rows 24 + 24 + 22, slabs of 22."""
    assert _slab(dims[2], world, 0) is not None
    _check_sharded_solve(pkg, eng, capi, dims, R, world)


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_cp_tv_nonneg_f16(pkg, eng, capi, world):
    """The model of test_gpu_sharded.test_sharded_cp_tv_nonneg at (37, 14, 13): ragged rows (19+18, 13+13+11) and ragged
    slabs (7+6, 5+5+3), TV on mode 1, 8 iterations."""
    _check_sharded_solve(pkg, eng, capi, (37, 14, 13), 3, world, constraints=TV_NONNEG, iters=8, seed=21)


# ---- 4. no slab to own -------------------------------------------------------------------------------------------------------------
def test_no_slab_to_own(pkg, eng, capi):
    """K = 2 over three ranks: some rank would own no slab, so copy 0 is built from the rank's rows like the others and the
    mode-1 pass contracts the rank's rows (partial sums meet in the all-reduce, as in fp32)."""
    dims, world = (37, 14, 2), 3
    assert _slab(dims[2], world, 0) is None
    assert [_rank_copies(dims, world, r)[0][1] for r in range(3)] == [13, 13, 11]
    _check_sharded_solve(pkg, eng, capi, dims, 3, world)


# ---- 5. coupled model ------------------------------------------------------------------------------------------------------------
def test_coupled_tensor_and_matrix_model_sharded(pkg, capi):
    """script3 family (matrix + CP tensor, first modes coupled, both row-sharded): the tensor is stored F16 with the global
    scale, the matrix F32 with scale 1."""
    rng = np.random.default_rng(3)
    Z, io = script3_model(rng)
    Zd = dict(Z)
    D, s = dequantize(Z['object'][0])
    Zd['object'] = [D, Z['object'][1]]
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    opt = options(MaxOuterIters=10)
    _, Fo, _, oo = OA.cmtf_AOADMM(Zd, alg_options=opt, init=copy.deepcopy(G))
    res = _solve_on_ranks(pkg, Z, G, opt, 2, probe=lambda e, r: (e.tensor_storage_info(0)[:2], e.tensor_storage_info(1)[:2]))
    for r, (_, _, (t0, t1)) in enumerate(res):
        assert t0 == (capi.PREC_F16, s), (r, t0)
        assert t1 == (capi.PREC_F32, 1.0), (r, t1)
    _assert_ranks_identical([(F, o) for F, o, _ in res])
    Fg, og, _ = res[0]
    err = max(rel_fro(b, a) for a, b in zip(Fo['fac'], Fg['fac']))
    print('f16 sharded coupled tensor + matrix: max factor error %.3g' % err)
    assert og['OuterIterations'] == oo['OuterIterations']
    assert err < 1e-4, err


# ---- 6. reproducible -------------------------------------------------------------------------------------------------------------
def test_two_sharded_runs_return_the_same_bits(pkg):
    Z, G, _, _ = _solve_reference((37, 14, 13), 3, TV_NONNEG, 8, 21)
    opt = options(MaxOuterIters=8)
    a = _solve_on_ranks(pkg, Z, G, opt, 3)
    b = _solve_on_ranks(pkg, Z, G, opt, 3)
    _assert_ranks_identical([(a[0][0], a[0][1]), (b[0][0], b[0][1])])
    print('f16 sharded: two runs over 3 ranks, identical bits: yes')


# ---- 7. one-rank communicator ---------------------------------------------------------------------------------------------------
def test_one_rank_communicator_changes_nothing(pkg, eng):
    dims, R = (70, 64, 66), 20
    Z, G, _, _ = _solve_reference(dims, R, NONNEG, 3, sum(dims) + R)
    opt = options(MaxOuterIters=3)
    _, F1, _, o1 = pkg.cmtf_AOADMM(dict(Z), alg_options=opt, init=copy.deepcopy(G), engine=eng, precision='f16')
    with pkg.Engine(0) as e:
        e.comm_init_local(next(_keys), 0, 1)
        _, Fc, _, oc = pkg.cmtf_AOADMM(dict(Z), alg_options=opt, init=copy.deepcopy(G), engine=e, precision='f16')
        assert e.tensor_storage_info(0) == eng.tensor_storage_info(0)
    gap = max(rel_fro(b, a) for a, b in zip(F1['fac'], Fc['fac']))
    print('f16 with a one-rank communicator against none: max factor gap %.3g' % gap)
    assert oc['OuterIterations'] == o1['OuterIterations']
    assert gap < 1e-12, gap


# ---- 8. a non-finite entry on one rank only ----------------------------------------------------------------------------------------
def test_non_finite_entry_on_one_rank_fails_every_rank(pkg, capi):
    """X[0, 3, 0] = nan lies in rank 0's rows and rank 0's slab only.  The verdict is taken after the exchange, so every
    rank raises AOADMM_ERR_INVALID and none is left alone in a collective; the same engines then solve the finite model."""
    dims, R, world = (37, 14, 13), 3, 3
    Z, G, _, _ = _solve_reference(dims, R, NONNEG, 3, sum(dims) + R)
    Xbad = np.array(Z['object'][0], order='F')
    Xbad[0, 3, 0] = np.nan
    opt = options(MaxOuterIters=3)
    _, Fo, _, _ = OA.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G))

    def body(e, r):
        code = None
        try:
            pkg.build_model(e, _cp_block(dims, R, Xbad), 'f16')
        except pkg.AoadmmError as ex:
            code = ex.code
        _, Fg, _, og = pkg.cmtf_AOADMM(dict(Z), alg_options=opt, init=copy.deepcopy(G), engine=e, precision='f32')
        return code, Fg

    res = run_ranks(pkg, world, body)
    print('f16 sharded, nan on rank 0: codes', [code for code, _ in res])
    assert [code for code, _ in res] == [capi.ERR_INVALID] * world
    err = max(rel_fro(b, a) for a, b in zip(Fo['fac'], res[0][1]['fac']))
    print('f32 solve on the same engines afterwards: max factor error %.3g' % err)
    assert err < 1e-4, err


# ---- 9. what stays refused -------------------------------------------------------------------------------------------------------
def test_row_blocks_and_masks_stay_refused_on_a_communicator_engine(pkg, capi):
    dims, R = (20, 14, 12), 3
    X = capi.as_f(np.random.default_rng(14).standard_normal(dims))
    with pkg.Engine(0) as e:
        e.comm_init_local(next(_keys), 0, 1)
        pkg.build_model(e, _cp_block(dims, R, X), 'f32')
        before = e.tensor_storage_info(0)
        with pytest.raises(pkg.UnsupportedOnDevice):
            capi.check(e.lib.aoadmm_tensor_upload_rows(e.h, 0, capi.dptr(X), 0, dims[0], capi.PREC_F16))
        assert e.tensor_storage_info(0) == before and before[:2] == (capi.PREC_F32, 1.0)
        pkg.build_model(e, _cp_block(dims, R, X), 'f16')
        assert e.tensor_storage_info(0)[0] == capi.PREC_F16
        mk = np.asfortranarray(np.ones(dims, dtype=np.uint8))
        with pytest.raises(pkg.AoadmmError) as ei:
            capi.check(e.lib.aoadmm_tensor_mask_upload(e.h, 0, mk.ctypes.data_as(C.POINTER(C.c_uint8))))
        assert ei.value.code == capi.ERR_INVALID
