"""GPU: a sparse (COO) CP block with its nonzeros sharded over the ranks of a communicator
(aoadmm_tensor_upload_coo_sharded; csrc/sparse.hip coo_keep_share, csrc/cpblock.hip sparse_mttkrp_sharded).  Ranks are
threads of this process with one engine each, joined by the process-local group, as in test_gpu_sharded.py.  MTTKRP
parity of every mode on every rank, the edges of the cut, resident bytes, solver equivalence with the oracle and with
the single-engine sparse solve, the multi-device context, and the refusals."""
import copy
import ctypes as C
import importlib
import itertools
import threading

import numpy as np
import pytest

from oracle import aoadmm as OA
from oracle.tensor_ops import mttkrp as dense_mttkrp
from helpers import cp_cp_exact_model, cp_model, options, script3_model
from test_gpu_solver import compare
from test_gpu_sparse import SHAPES, assert_close, assert_same_solve, random_coo, ref_mttkrp, sparsify, to_sptensor

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')
_keys = itertools.count(9000)


def on_ranks(pkg, world, fn):
    """fn(engine, rank) on `world` engines of device 0, one thread each, joined by a process-local group."""
    key = next(_keys)
    res, err = [None] * world, [None] * world

    def rank_main(r):
        try:
            with pkg.Engine(0) as e:
                e.comm_init_local(key, r, world)
                res[r] = fn(e, r)
        except BaseException as ex:   # noqa: BLE001 -- reported by the main thread
            err[r] = ex

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r, ex in enumerate(err):
        assert ex is None, 'rank %d: %r' % (r, ex)
    return res


def cp_Z(shape, R, obj):
    n = len(shape)
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(shape),
                coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
                constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[obj], _ranks=[R] * n)


def empty(pkg, shape):
    return pkg.sptensor(np.zeros((0, len(shape)), dtype=np.int64), np.zeros(0), shape)


def raw_model(pkg, e, shape, U, subs, vals, sharded=True):
    """One uncoupled CP block with the factors U; the raw list goes up as given (the device sorts and coalesces)."""
    Z = cp_Z(shape, U[0].shape[1], empty(pkg, shape))
    pkg.build_model(e, Z)
    e.upload_coo(0, subs, vals, sharded=sharded)
    pkg.upload_state(e, Z, {'fac': U})


def all_modes(e, shape, R):
    return [e.resident_mttkrp(0, n, shape[n], R) for n in range(len(shape))]


def normsq(e):
    v = C.c_double(0)
    capi.check(e.lib.aoadmm_tensor_normsq(e.h, 0, C.byref(v)))
    return v.value


def distinct_coo(rng, shape, nnz, row0=None, row0_count=0):
    """nnz DISTINCT subscripts (so the coalesced count is nnz); row0_count of them in row `row0` of the first mode."""
    rest = int(np.prod(shape[1:]))
    if row0 is None:
        lin = rng.choice(shape[0] * rest, nnz, replace=False)
    else:
        hot = row0 + shape[0] * rng.choice(rest, row0_count, replace=False)
        other = np.setdiff1d(np.arange(shape[0] * rest), row0 + shape[0] * np.arange(rest))
        lin = np.concatenate([hot, rng.choice(other, nnz - row0_count, replace=False)])
        lin = lin[rng.permutation(nnz)]
    subs = np.stack(np.unravel_index(lin, shape, order='F'), axis=1).astype(np.int64)
    return subs, rng.random(nnz) + 0.1


def bytes_per_nonzero(N):
    return N * (4 * N + 8)


def check_mttkrps(pkg, world, shape, R, subs, vals, rng):
    """Every mode on every rank against numpy; all ranks and a second run the same bits.  Returns rank 0's results."""
    U = [rng.random((s, R)) for s in shape]

    def rank_fn(e, r):
        raw_model(pkg, e, shape, U, subs, vals)
        return all_modes(e, shape, R), all_modes(e, shape, R)

    res = on_ranks(pkg, world, rank_fn)
    for n in range(len(shape)):
        ref = ref_mttkrp(subs, vals, shape, U, n)
        for first, second in res:
            if len(vals):
                assert_close(first[n], ref)
            else:
                assert not first[n].any()
            assert np.array_equal(first[n], res[0][0][n]) and np.array_equal(second[n], first[n])
    return res[0][0], U


# ---- 1. MTTKRP of every mode on every rank -----------------------------------------------------------------------------
@pytest.mark.parametrize('world', [2, 3, 4])
@pytest.mark.parametrize('N', [2, 3, 4])
@pytest.mark.parametrize('R', [1, 5, 20, 64])
def test_mttkrp_parity_on_every_rank(pkg, world, N, R):
    """build_model(sparse_sharding=True) on every rank: duplicates, explicit zeros, empty rows, an nnz that no rank
    count divides (fp64, rtol 1e-12 against numpy); all ranks and a second run bit-identical."""
    rng = np.random.default_rng(1000 * world + 100 * N + R)
    shape = SHAPES[N]
    subs, vals = random_coo(rng, shape, 3001, dup=37, zeros=11)
    S = pkg.sptensor(subs, vals, shape)
    U = [rng.random((s, R)) for s in shape]

    def rank_fn(e, r):
        Z = cp_Z(shape, R, S)
        pkg.build_model(e, Z, sparse_sharding=True)
        pkg.upload_state(e, Z, {'fac': U})
        return all_modes(e, shape, R), all_modes(e, shape, R)

    res = on_ranks(pkg, world, rank_fn)
    for n in range(N):
        ref = ref_mttkrp(subs, vals, shape, U, n)
        for first, second in res:
            assert_close(first[n], ref)
            assert np.array_equal(first[n], res[0][0][n]) and np.array_equal(second[n], first[n])
        if n == 0:
            assert not res[0][0][0][0].any() and not res[0][0][0][-1].any()   # rows without nonzeros: exact zeros


# ---- 2. edges of the cut -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nnz', [0, 1, 2])
def test_empty_shares(pkg, nnz):
    """Fewer nonzeros than ranks: the ranks with an empty share still join every collective."""
    rng = np.random.default_rng(nnz)
    shape = (12, 10, 8)
    subs, vals = distinct_coo(rng, shape, nnz)
    check_mttkrps(pkg, 3, shape, 5, subs, vals, rng)


@pytest.mark.parametrize('world', [2, 3, 4])
@pytest.mark.parametrize('extra', [0, 1])
def test_share_of_one_chunk(pkg, world, extra):
    """nnz = world * 256: each share is exactly one chunk of the kernel (no carry pass); + 1: one share starts a second."""
    rng = np.random.default_rng(10 * world + extra)
    shape = (40, 30, 20)
    subs, vals = distinct_coo(rng, shape, world * 256 + extra)
    check_mttkrps(pkg, world, shape, 20, subs, vals, rng)


@pytest.mark.parametrize('world', [2, 3, 4])
def test_every_cut_inside_a_row(pkg, world):
    """A first mode of 3 rows with 1500 nonzeros: every rank's span shares its boundary rows with its neighbours."""
    rng = np.random.default_rng(20 + world)
    shape = (3, 40, 30)
    subs, vals = distinct_coo(rng, shape, 1500)
    check_mttkrps(pkg, world, shape, 5, subs, vals, rng)


@pytest.mark.parametrize('world', [2, 3, 4])
def test_one_row_with_most_nonzeros(pkg, world):
    """Row 5 of the first mode holds 90 % of 2000 nonzeros: it is spread over several ranks."""
    rng = np.random.default_rng(30 + world)
    shape = (20, 60, 50)
    subs, vals = distinct_coo(rng, shape, 2000, row0=5, row0_count=1800)
    check_mttkrps(pkg, world, shape, 20, subs, vals, rng)


@pytest.mark.parametrize('world', [2, 3])
def test_duplicates_are_summed_before_the_cut(pkg, eng, world):
    """Every subscript `world` times, shuffled: coalesced over the whole list first, so the shares add up to the distinct
    count and the block is the one a single engine holds (MTTKRPs at the 1e-12 bar, normsq to 1e-14)."""
    rng = np.random.default_rng(40 + world)
    shape, R, nd = (25, 20, 15), 5, 700
    s1, _ = distinct_coo(rng, shape, nd)
    perm = rng.permutation(nd * world)
    subs = np.tile(s1, (world, 1))[perm]
    vals = rng.random(nd * world) + 0.1
    U = [rng.random((s, R)) for s in shape]
    raw_model(pkg, eng, shape, U, subs, vals, sharded=False)
    single, single_normsq = all_modes(eng, shape, R), normsq(eng)

    def rank_fn(e, r):
        raw_model(pkg, e, shape, U, subs, vals)
        return all_modes(e, shape, R), normsq(e), e.tensor_storage_info(0)[2]

    res = on_ranks(pkg, world, rank_fn)
    assert sum(b for _, _, b in res) == bytes_per_nonzero(3) * nd
    for got, nsq, _ in res:
        for n in range(3):
            assert_close(got[n], single[n])
            assert_close(got[n], ref_mttkrp(subs, vals, shape, U, n))
            assert np.array_equal(got[n], res[0][0][n])
        assert nsq == res[0][1]
        assert abs(nsq - single_normsq) <= 1e-14 * single_normsq


# ---- 3. storage --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world,N', [(2, 3), (3, 4), (4, 2)])
def test_resident_bytes_and_kernel_stats_follow_the_share(pkg, world, N):
    rng = np.random.default_rng(50 + world)
    shape, R = SHAPES[N], 20
    nnz = 3001
    subs, vals = distinct_coo(rng, shape, nnz)
    U = [rng.random((s, R)) for s in shape]

    def rank_fn(e, r):
        raw_model(pkg, e, shape, U, subs, vals)
        info = e.tensor_storage_info(0)
        stats = []
        for n in range(N):
            e.kernel_stats(3, reset=True)
            e.resident_mttkrp(0, n, shape[n], R)
            stats.append(e.kernel_stats(3))
        e.upload_coo(0, subs, vals)                      # plain upload on the same communicator: replicated again
        return info, stats, e.tensor_storage_info(0), all_modes(e, shape, R)

    res = on_ranks(pkg, world, rank_fn)
    per = bytes_per_nonzero(N)
    for r, (info, stats, info_plain, plain) in enumerate(res):
        lo, hi = capi.coo_share(nnz, r, world)
        assert info == (capi.PREC_F64, 1.0, per * (hi - lo))
        assert info_plain == (capi.PREC_F64, 1.0, per * nnz)
        for n in range(N):
            rows = np.sort(subs[:, n])[lo:hi]            # the share of mode n in that mode's own order
            span = int(rows[-1] - rows[0] + 1)
            ms, launches, by, fl = stats[n]
            assert launches == 1
            assert by == (hi - lo) * (4 + 4 * (N - 1) + 8) + (hi - lo) * (N - 1) * R * 8 + span * R * 8
            assert fl == (hi - lo) * R * N
            assert_close(plain[n], ref_mttkrp(subs, vals, shape, U, n))
    assert sum(info[2] for info, _, _, _ in res) == per * nnz


# ---- 4. solves ---------------------------------------------------------------------------------------------------------
def solve_sharded(pkg, eng, Z, io, opt, p, make_sparse, world, seed=7):
    """Z.object{p} sparsified; the oracle on the densified data, one engine on the sparse data, and `world` ranks with
    sparse_sharding = 1 from the same initial state.  Bars: compare (1e-8) against the oracle, assert_same_solve (1e-10:
    another summation order of the MTTKRP, nothing else) against the single engine, ranks bit-identical."""
    rng = np.random.default_rng(seed + 1)
    Zd = dict(Z, object=list(Z['object']))
    Zd['object'][p] = sparsify(Z['object'][p], rng)
    Zs = dict(Zd, object=list(Zd['object']))
    Zs['object'][p] = make_sparse(Zd['object'][p])
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=np.random.default_rng(seed))
    _, Fo, _, oo = OA.cmtf_AOADMM(Zd, alg_options=opt, init=copy.deepcopy(G))
    _, F1, _, o1 = pkg.cmtf_AOADMM(Zs, alg_options=opt, init=copy.deepcopy(G), engine=eng)
    opt_sh = dict(opt, hip=dict(sparse_sharding=1))

    def rank_fn(e, r):
        _, Fg, _, og = pkg.cmtf_AOADMM(Zs, alg_options=opt_sh, init=copy.deepcopy(G), engine=e)
        return Fg, og, e.tensor_storage_info(p)[2]

    res = on_ranks(pkg, world, rank_fn)
    F0, o0, _ = res[0]
    nnz = Zs['object'][p].nnz
    nd = len(Z['modes'][p])
    assert [b for _, _, b in res] == [bytes_per_nonzero(nd) * (hi - lo) for lo, hi in
                                      (capi.coo_share(nnz, r, world) for r in range(world))]   # the solve ran on shares
    for Fr, orr, _ in res[1:]:
        for key in ('fac', 'constraint_fac', 'constraint_dual_fac', 'coupling_fac', 'coupling_dual_fac'):
            for a, b in zip(F0[key], Fr[key]):
                if a is not None:
                    assert np.array_equal(a, b), key
        assert np.array_equal(o0['func_val_conv'], orr['func_val_conv'])
    compare(Fo, oo, F0, o0)
    assert_same_solve(F1, o1, F0, o0)
    return Zs, G, F1, o1


@pytest.mark.parametrize('world', [2, 3])
def test_solve_cp_nonneg(pkg, eng, world):
    rng = np.random.default_rng(11)
    Z, io, _ = cp_model((40, 50, 60), 3, rng, [('non-negativity',)] * 3)
    solve_sharded(pkg, eng, Z, io, options(MaxOuterIters=8), 0, lambda X: to_sptensor(pkg, X), world)


def test_solve_script3_sptensor_coupled_to_row_sharded_dense_matrix(pkg, eng):
    rng = np.random.default_rng(13)
    Z, io = script3_model(rng)
    solve_sharded(pkg, eng, Z, io, options(MaxOuterIters=8), 0, lambda X: to_sptensor(pkg, X), 2)


def test_solve_scipy_matrix_block_coupled_to_dense_tensor(pkg, eng):
    sps = pytest.importorskip('scipy.sparse')
    rng = np.random.default_rng(14)
    Z, io = script3_model(rng)
    solve_sharded(pkg, eng, Z, io, options(MaxOuterIters=8), 1, lambda X: sps.csc_matrix(X), 2)


def test_solve_rank20_tv_long_mode(pkg, eng):
    rng = np.random.default_rng(15)
    Z, io, _ = cp_model((300, 40, 30), 20, rng, [('TV regularization', 0.01), ('non-negativity',), ('non-negativity',)])
    solve_sharded(pkg, eng, Z, io, options(MaxOuterIters=6), 0, lambda X: to_sptensor(pkg, X), 2)


def test_multi_device_context_shards_over_its_engines(pkg, eng):
    """Engine([0, 0]) with sparse_sharding = 1: both engines keep a share (rank 0 reports its own bytes); the dense tensor
    coupled to the sparse block is row-sharded.  Equal to the single engine at the assert_same_solve bar."""
    rng = np.random.default_rng(18)
    Z, io = cp_cp_exact_model(rng)
    S = to_sptensor(pkg, sparsify(Z['object'][0], rng))
    Z = dict(Z, object=[S, Z['object'][1]])
    Zd = dict(Z, object=[S.full(), Z['object'][1]])
    G = OA.init_coupled_AOADMM_CMTF({**Zd, 'prox_operators': None}, io, rng=rng)
    opt = options(MaxOuterIters=8)
    _, F1, _, o1 = pkg.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G), engine=eng)
    with pkg.Engine([0, 0]) as e2:
        _, F2, _, o2 = pkg.cmtf_AOADMM(Z, alg_options=dict(opt, hip=dict(sparse_sharding=1)), init=copy.deepcopy(G), engine=e2)
        lo, hi = capi.coo_share(S.nnz, 0, 2)
        assert e2.tensor_storage_info(0)[2] == bytes_per_nonzero(3) * (hi - lo)
    assert_same_solve(F1, o1, F2, o2)


# ---- 5. hygiene --------------------------------------------------------------------------------------------------------
def test_refusals_and_replacement(pkg):
    rng = np.random.default_rng(60)
    shape, R = (12, 10, 8), 3
    subs, vals = distinct_coo(rng, shape, 200)
    U = [rng.random((s, R)) for s in shape]
    Xd = rng.random(shape)
    mask = np.ones(shape, dtype=np.uint8, order='F')

    def rank_fn(e, r):
        raw_model(pkg, e, shape, U, subs, vals)
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.resident_nvecs(0, 0, shape[0], 2)
        with pytest.raises(pkg.AoadmmError) as ei:
            capi.check(e.lib.aoadmm_tensor_mask_upload(e.h, 0, mask.ctypes.data_as(C.POINTER(C.c_uint8))))
        assert ei.value.code == capi.ERR_INVALID and 'sptensor' in str(ei.value)
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.resident_unfold_gram(0, 0, shape[0])
        after = e.resident_mttkrp(0, 1, shape[1], R)     # the block still answers
        capi.check(e.lib.aoadmm_tensor_upload(e.h, 0, capi.dptr(np.asfortranarray(Xd)), 0))   # dense, row-sharded
        dense = e.resident_mttkrp(0, 1, shape[1], R)
        e.upload_coo(0, subs, vals, sharded=True)        # and sharded again over the dense form
        again = e.resident_mttkrp(0, 2, shape[2], R)
        e.upload_coo(0, subs, vals)                      # plain: replicated, no collective
        plain = e.resident_mttkrp(0, 0, shape[0], R)
        return after, dense, again, plain, e.tensor_storage_info(0)[2]

    for after, dense, again, plain, nbytes in on_ranks(pkg, 2, rank_fn):
        assert_close(after, ref_mttkrp(subs, vals, shape, U, 1))
        assert np.allclose(dense, dense_mttkrp(Xd, U, 1), rtol=1e-12, atol=0)
        assert_close(again, ref_mttkrp(subs, vals, shape, U, 2))
        assert_close(plain, ref_mttkrp(subs, vals, shape, U, 0))
        assert nbytes == bytes_per_nonzero(3) * 200


def test_share_of_another_cut_is_refused(pkg):
    """The engine leaves its 2-rank group for a communicator of its own: the share it holds was cut for (r, 2), and the
    block says so instead of returning the sum of half the nonzeros."""
    rng = np.random.default_rng(61)
    shape, R = (12, 10, 8), 3
    subs, vals = distinct_coo(rng, shape, 200)
    U = [rng.random((s, R)) for s in shape]
    solo = [next(_keys), next(_keys)]

    def rank_fn(e, r):
        raw_model(pkg, e, shape, U, subs, vals)
        e.comm_init_local(solo[r], 0, 1)
        codes = []
        for call in (lambda: e.resident_mttkrp(0, 0, shape[0], R), lambda: normsq(e)):
            with pytest.raises(pkg.AoadmmError) as ei:
                call()
            codes.append((ei.value.code, 'upload again' in str(ei.value)))
        e.upload_coo(0, subs, vals, sharded=True)        # world 1 now: the plain upload
        return codes, e.resident_mttkrp(0, 0, shape[0], R)

    for codes, got in on_ranks(pkg, 2, rank_fn):
        assert codes == [(capi.ERR_INVALID, True)] * 2
        assert_close(got, ref_mttkrp(subs, vals, shape, U, 0))


def test_without_a_communicator_it_is_the_plain_upload(pkg, eng):
    rng = np.random.default_rng(62)
    shape, R = SHAPES[3], 20
    subs, vals = random_coo(rng, shape, 3001, dup=37, zeros=11)
    U = [rng.random((s, R)) for s in shape]
    raw_model(pkg, eng, shape, U, subs, vals, sharded=False)
    plain, plain_info, plain_nsq = all_modes(eng, shape, R), eng.tensor_storage_info(0), normsq(eng)
    raw_model(pkg, eng, shape, U, subs, vals, sharded=True)
    assert eng.tensor_storage_info(0) == plain_info and normsq(eng) == plain_nsq
    for a, b in zip(all_modes(eng, shape, R), plain):
        assert np.array_equal(a, b)
    eng.resident_nvecs(0, 0, shape[0], 2, max_iters=2)   # not sharded: the nvecs start is still there
