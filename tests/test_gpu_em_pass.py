"""GPU: ONE dense EM pass (csrc/em.hip) as a solve runs it -- `Engine.resident_em_pass` -> aoadmm_resident_em_pass ->
Engine::em_pass_enqueue -- against the longdouble reference and the derived bounds of tests/em_ref.py, per kernel class:
every RMAX instantiation of the strip kernel in both precisions with and without the fused contraction, the walk along
either mode, the kernel for R > 32, the moving mask bit, the line write-back at every lane / slot position, the column
chunking, and matrix, 4-way and PARAFAC2 blocks.

Every update case checks: observed entries bitwise the input; missing entries within beta of the longdouble model; the
four statistics within their bounds (exactly 0 where the reference sum is empty); a second pass on re-uploaded data
returns the same bits; `info` is what the shape is there for (`_expected_info` restates em_chunking / em_vec as they
are today: if they are retuned the assertion fails and says so -- pick new shapes then).  Fused cases also check the
MTTKRP finished from the T the pass left, at the op-level bars of test_gpu_tensor_pass.py, with no contraction launch.

Observed error-to-bound ratios on an MI355X (largest over all cases of this file; every case prints its own):
             imputed value / beta    num     den      obs_res   obs_x2      MTTKRP from the fused T (relative)
    fp64     0.377                   0.083   0.024    0.022     0.045       1.5e-15  (bar 1e-12)
    fp32     0.441                   0.045   0.011    0.0070    0.014       2.9e-7   (bar 2e-6)
"""
import functools

import numpy as np
import pytest

import em_ref
from helpers import rel_fro

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-12, 'f32': 2e-6}          # test_gpu_tensor_pass.py / README 8a
PRECS = ['f64', 'f32']


def _cdiv(a, b):
    return -(-a // b)


def _pad(prec, n):
    q = 2 if prec == 'f64' else 4
    return _cdiv(n, q) * q


def _expected_info(dims, R, prec, fused):
    """em.hip em_vec / em_chunking / em_cp_launch as of this writing; dims merged to (I, J, K) as the pass sees them."""
    I, J = dims[0], dims[1]
    K = int(np.prod(dims[2:])) if len(dims) > 2 else 1
    vec = 1 if R > 32 else (2 if prec == 'f64' else 4)
    rmax = 64 if R > 32 else _cdiv(R, 4) * 4
    strips = _cdiv(_pad(prec, I), 256 * vec)
    walk = 2 if fused == 2 else 1
    NW, NF = (J, K) if walk == 1 else (K, J)
    tiles = _cdiv(NW, 64)
    want = _cdiv(768 if fused >= 0 else 6144, strips * NF)
    if fused >= 0:
        want = max(want, _cdiv(NW, 2048))
    want = max(1, min(want, tiles))
    jlen = _cdiv(tiles, want) * 64
    return dict(vec=vec, rmax=rmax, fused=fused, walk=walk, strips=strips, jchunks=_cdiv(NW, jlen), jlen=jlen)


def _block(dims, R, X, obs):
    n = len(dims)
    return dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(dims),
                coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
                constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[X],
                miss=[obs.astype(np.uint8)], _ranks=[R] * n)


@functools.lru_cache(maxsize=4)
def _data(dims, R):
    """(X, U, M): data, factors and the longdouble model, once per (dims, R) for every mask and both precisions."""
    X, U = em_ref.make_data(dims, R, np.random.default_rng(1000 * sum(dims) + 7 * len(dims) + R))
    M = em_ref.model(U)
    for a in [X, M] + U:
        a.setflags(write=False)
    return X, U, M


def _mask(dims, spec):
    """Boolean 'observed' array.  ('frac', f): each entry missing with probability f, at least one when f > 0;
    ('slab', k): the whole slab k of the last mode missing, nothing else; ('single', index): exactly that entry."""
    obs = np.ones(dims, dtype=bool)
    if spec[0] == 'frac':
        if spec[1] > 0:
            rng = np.random.default_rng(int(spec[1] * 1e6) + sum(dims))
            obs = rng.random(dims) >= spec[1]
            if obs.all():
                obs.flat[rng.integers(obs.size)] = False
    elif spec[0] == 'slab':
        obs[..., spec[1]] = False
    else:
        obs[tuple(spec[1])] = False
    return obs


@functools.lru_cache(maxsize=2)
def _ref(dims, R, mask, fill):
    X, U, M = _data(dims, R)
    obs = _mask(dims, mask)
    if fill == 'zero':
        X = np.where(obs, X, 0.0)
    return em_ref.EmRef(X, obs, U, M=M)


WORST = {}                                  # prec -> [entry, num, den, obs_res, obs_x2] largest ratio seen (printed per case)


def _note(prec, re, rs):
    w = WORST.setdefault(prec, np.zeros(5))
    w[:] = np.maximum(w, np.concatenate([[re], np.where(np.isfinite(rs), rs, 0)]))
    return 'worst so far %s: entry %.3g sums %s' % (prec, w[0], ' '.join('%.3g' % v for v in w[1:]))


def _run(pkg, eng, dims, R, prec, mask=('frac', 0.01), fuse=0, update=1, fill='nonzero', fused=-1):
    """One case: the pass twice on freshly uploaded data, every check of the module docstring.  Returns the first
    call's result."""
    ref = _ref(dims, R, mask, fill)
    X, obs, U = ref.X, ref.obs, ref.U
    Z = _block(dims, R, np.asfortranarray(X), obs)

    def once():
        pkg.build_model(eng, Z, prec)
        pkg.upload_state(eng, Z, dict(fac=list(U)))
        eng.kernel_stats(0, reset=True)
        eng.kernel_stats(1, reset=True)
        out = eng.resident_em_pass(0, dims, R, update=update, fuse=fuse)
        out['contractions'] = (eng.kernel_stats(0)[1], eng.kernel_stats(1)[1])
        return out

    out = once()
    assert out['info'] == _expected_info(dims, R, prec, fused), (out['info'], _expected_info(dims, R, prec, fused))
    rs = ref.stat_ratios(out['stats'], prec)
    re = ref.entry_ratio(out['data'], prec) if update else 0.0
    print('em pass %s R=%d %s mask=%s fuse=%d update=%d: entry %.3g of beta, sums %s of their bounds | %s'
          % (dims, R, prec, mask, fuse, update, re, ' '.join('%.3g' % v for v in rs), _note(prec, re, rs)))
    if update:
        assert np.array_equal(out['data'][obs], X[obs])                  # bitwise: X holds fp32 values
        assert re <= 1.0, re
    else:
        assert np.array_equal(out['data'], X)
    for q, name in enumerate(em_ref.STAT_NAMES):
        if ref.stats[q] == 0:
            assert out['stats'][q] == 0, (name, out['stats'][q])
        assert rs[q] <= 1.0, (name, rs[q], out['stats'][q], ref.stats[q])
    if fused >= 0:
        assert out['mttkrp_mode'] == 0 and out['mttkrp'] is not None
        assert out['contractions'] == (0, 0), out['contractions']       # finished from the cached T alone
        err = rel_fro(out['mttkrp'], ref.mttkrp(0))
        print('   mttkrp from the fused T: %.3g' % err)
        assert err < TOL[prec], err
    else:
        assert out['mttkrp'] is None and out['mttkrp_mode'] == -1
    again = once()
    assert again['stats'].tobytes() == out['stats'].tobytes()            # fixed summation order
    assert np.array_equal(again['data'], out['data'])
    if fused >= 0:
        assert np.array_equal(again['mttkrp'], out['mttkrp'])
    return out


# ---- rank classes ---------------------------------------------------------------------------------------------------------
# (37, 70, 9): one strip that is mostly padding, walks of 70 (64 + 6) and 9 columns; small enough for the one-launch
# MTTKRP, so the fused cases need `tensor_passes`.  (131, 67, 70): walks of 67 (64 + 3) and 70 (64 + 6), I odd in both
# paddings, too large for the one-launch MTTKRP.
RANK_SHAPES = [(37, 70, 9), (131, 67, 70)]
R_FUSED = [1, 4, 5, 8, 12, 13, 16, 20, 21, 24]       # both ends of every fused RMAX class; R == RMAX: vector stores of T
R_UNFUSED = [25, 28, 29, 32]                         # RMAX = 28 and 32: no fused form
R_SCALAR = [33, 64]                                  # em_cp_k
R_SECOND = [4, 13, 20, 24]                           # fused walk along mode 2


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R', R_FUSED)
@pytest.mark.parametrize('dims', RANK_SHAPES, ids=str)
def test_fused_rank_classes(pkg, eng, tensor_passes, dims, R, prec):
    """fuse = 1, update order 1-2-3: the pass contracts mode 3 (walk = 2) and the T it leaves serves mode 1."""
    out = _run(pkg, eng, dims, R, prec, fuse=1, fused=2)
    assert out['info']['walk'] == 2 and out['info']['vec'] == (2 if prec == 'f64' else 4)
    assert out['info']['rmax'] in (4, 8, 12, 16, 20, 24) and 0 <= out['info']['rmax'] - R < 4


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R', R_SECOND)
@pytest.mark.parametrize('dims', RANK_SHAPES, ids=str)
def test_fused_second_mode_rank_classes(pkg, eng, tensor_passes, dims, R, prec):
    """fuse = 2 (what AOADMM_EM_FUSE_SECOND_MODE forces in a solve): the strips walk mode 2 and contract it."""
    out = _run(pkg, eng, dims, R, prec, fuse=2, fused=1)
    assert out['info']['walk'] == 1


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R', R_UNFUSED + R_SCALAR)
@pytest.mark.parametrize('dims', RANK_SHAPES, ids=str)
def test_unfused_rank_classes(pkg, eng, tensor_passes, dims, R, prec):
    """R > 24 has no fused form even when asked for one: RMAX = 28 and 32 of the strip kernel, one row per thread
    above 32."""
    out = _run(pkg, eng, dims, R, prec, fuse=1, fused=-1)
    want = (1, 64) if R > 32 else (2 if prec == 'f64' else 4, 28 if R <= 28 else 32)
    assert (out['info']['vec'], out['info']['rmax']) == want


def test_small_block_is_not_fused_without_the_fixture(pkg, eng):
    """Without AOADMM_NO_SMALL_MTTKRP the one-launch MTTKRP serves (37, 70, 9) at R = 5: a solve fuses nothing there."""
    for prec in PRECS:
        _run(pkg, eng, (37, 70, 9), 5, prec, fuse=1, fused=-1)


# ---- rows -----------------------------------------------------------------------------------------------------------------
# I = 1, 3, 9: far below one wave, mostly padding.  Padded rows mod 8 (the mask bit moves with the walk when it is not 0):
# fp64 9 -> 10 (2), 13 -> 14 (6), 523 -> 524 (4), 525 -> 526 (6), 513 -> 514 (2); fp32 1100 (4), 9 -> 12 (4).  One row past a
# strip: 513 and 523 in fp64 (512 rows per strip), 1025 and 1029 in fp32 (1024 rows per strip).  (9, 7, 3): 210 / 252
# padded entries, no multiple of 8: the mask's tail byte.
ROWS = [1, 3, 9, 13, 513, 523, 525, 1025, 1029, 1100]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('fuse', [0, 1])
@pytest.mark.parametrize('I', ROWS)
def test_rows(pkg, eng, tensor_passes, I, fuse, prec):
    dims = (I, 7, 3)
    out = _run(pkg, eng, dims, 5, prec, mask=('frac', 0.05), fuse=fuse, fused=2 if fuse else -1)
    per_strip = 512 if prec == 'f64' else 1024
    assert out['info']['strips'] == _cdiv(_pad(prec, I), per_strip)
    if I == 9:
        assert (_pad(prec, I) * 7 * 3) % 8 != 0
    if (prec, I) in (('f64', 513), ('f64', 523), ('f64', 525), ('f32', 1025), ('f32', 1029), ('f32', 1100)):
        assert out['info']['strips'] == 2
    if (prec, I) in (('f64', 9), ('f64', 13), ('f64', 513), ('f64', 523), ('f64', 525), ('f32', 9), ('f32', 1100)):
        assert _pad(prec, I) % 8 != 0


# ---- walked mode ----------------------------------------------------------------------------------------------------------
WALK = [1, 3, 64, 65, 130]                           # 1 and 3: fewer columns than the prefetch ring holds; tile edges


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('L', WALK)
def test_walk_lengths_second_mode(pkg, eng, L, prec):
    _run(pkg, eng, (37, L, 9), 6, prec, mask=('frac', 0.05), fuse=0, fused=-1)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('L', WALK)
def test_walk_lengths_third_mode_fused(pkg, eng, tensor_passes, L, prec):
    _run(pkg, eng, (37, 7, L), 6, prec, mask=('frac', 0.05), fuse=1, fused=2)


# ---- chunking -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_unfused_pieces_of_several_tiles(pkg, eng, prec):
    """(8, 130, 3100): one strip, 3100 fixed indices -> 2 pieces of the 130 columns: two whole tiles, then a ragged
    piece of 2 columns."""
    out = _run(pkg, eng, (8, 130, 3100), 5, prec, mask=('frac', 0.003), fuse=0, fused=-1)
    assert (out['info']['jchunks'], out['info']['jlen']) == (2, 128)


@pytest.mark.parametrize('prec', PRECS)
def test_fused_pieces(pkg, eng, prec):
    """(9, 400, 500) at R = 20: the fused pass walks mode 3 in 2 pieces of 256 and 244 positions, one chunk of T each."""
    out = _run(pkg, eng, (9, 400, 500), 20, prec, mask=('frac', 0.003), fuse=1, fused=2)
    assert (out['info']['jchunks'], out['info']['jlen'], out['info']['walk']) == (2, 256, 2)


# ---- masks ----------------------------------------------------------------------------------------------------------------
MASKS = [('frac', 0.0), ('frac', 0.003), ('frac', 0.01), ('frac', 0.2), ('slab', 4)]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('R,fuse', [(5, 0), (20, 1)], ids=['R5', 'R20-fused'])
@pytest.mark.parametrize('mask', MASKS, ids=lambda m: '%s%s' % m)
def test_masks(pkg, eng, mask, R, fuse, prec):
    """Missing fractions 0 (nothing written, num = den = 0 exactly), 0.003, 0.01 (few lines go back), 0.2 (all do) and
    one whole slab.  R = 20 is fused without the fixture (the one-launch MTTKRP stops at R = 16)."""
    out = _run(pkg, eng, (37, 70, 9), R, prec, mask=mask, fuse=fuse, fused=2 if fuse else -1)
    if mask == ('frac', 0.0):
        assert out['stats'][0] == 0 and out['stats'][1] == 0


@pytest.mark.parametrize('prec', PRECS)
def test_zero_initialised_missing_entries(pkg, eng, prec):
    """What every solver test uploads: zeros at the missing positions, den = 0 exactly."""
    out = _run(pkg, eng, (37, 70, 9), 5, prec, mask=('frac', 0.05), fill='zero')
    assert out['stats'][1] == 0 and out['stats'][0] > 0


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('fuse', [0, 1])
def test_statistics_only_pass_leaves_the_data_alone(pkg, eng, tensor_passes, fuse, prec):
    """update = 0 (the start objective and Znorm_const): the same statistics, the data bitwise unchanged everywhere, and
    no fused contraction whatever was asked for."""
    _run(pkg, eng, (37, 70, 9), 5, prec, mask=('frac', 0.2), fuse=fuse, update=0, fused=-1)


# One missing entry in a full block: num is a single (m - x)^2, den a single x^2, and one 128-byte line goes back.
# I = 260 (fp32: 65 vectors of 16 bytes per column) / 130 (fp64: the same): lane 0 of the strip sits at 16-byte slot
# (65 w) mod 8 = w mod 8 of its line in column w, and lanes 0, 7, 8, 63, 64 are rows 0, 7, 8, 63, 64 times the vector.
SINGLE_I = {'f64': 130, 'f32': 260}
LANES = [0, 7, 8, 63, 64]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('lane', LANES)
def test_single_missing_entry_at_every_slot(pkg, eng, lane, prec):
    I, vec, es = SINGLE_I[prec], (2 if prec == 'f64' else 4), (8 if prec == 'f64' else 4)
    dims = (I, 8, 2)
    assert _pad(prec, I) == I and I // vec == 65
    slots = {((I * 8 * 1 + I * w) * es // 16) % 8 for w in range(8)}     # lane 0's slot in column w of slab 1
    assert slots == set(range(8))
    for w in range(8):
        for v in (0, vec - 1):                                           # first and last entry of the lane's vector
            out = _run(pkg, eng, dims, 5, prec, mask=('single', (lane * vec + v, w, 1)), fuse=0, fused=-1)
            assert out['stats'][0] > 0 and out['stats'][1] > 0


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('where', ['first', 'last'])
def test_single_missing_entry_at_the_ends_of_the_block(pkg, eng, where, prec):
    dims = (37, 70, 9)
    idx = (0, 0, 0) if where == 'first' else (36, 69, 8)
    _run(pkg, eng, dims, 5, prec, mask=('single', idx), fuse=0, fused=-1)


# ---- block kinds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_matrix_block(pkg, eng, prec):
    """(130, 300): the natural array and the transposed copy are both imputed.  The transposed pass multiplies the same
    rounded factors in the same order with the operands of each multiply-add swapped, so the two agree bitwise."""
    dims, R = (130, 300), 5
    out = _run(pkg, eng, dims, R, prec, mask=('frac', 0.05))
    ref = _ref(dims, R, ('frac', 0.05), 'nonzero')
    assert out['data_t'].shape == (300, 130)
    assert np.array_equal(out['data_t'].T[ref.obs], ref.X[ref.obs])
    assert ref.entry_ratio(out['data_t'].T, prec) <= 1.0
    assert np.array_equal(out['data_t'].T, out['data'])


@pytest.mark.parametrize('prec', PRECS)
def test_four_way_block(pkg, eng, prec):
    """(7, 5, 4, 3): modes 3 and 4 merged, their factor the Khatri-Rao product built on the device."""
    out = _run(pkg, eng, (7, 5, 4, 3), 3, prec, mask=('frac', 0.1))
    assert out['info']['rmax'] == 4


def test_parafac2_block(pkg, eng):
    """Ragged slabs (em_par2_k, fp64 only): the statistics at fp64 rounding, the slabs like a CP block's entries."""
    I, Jk, R = 21, [5, 9, 14, 4, 30], 4
    K = len(Jk)
    rng = np.random.default_rng(212)
    A, C = rng.standard_normal((I, R)), rng.standard_normal((K, R))
    Bk = [rng.standard_normal((j, R)) for j in Jk]
    X, obs, refs = [], [], []
    for k in range(K):
        Xk = rng.standard_normal((I, Jk[k])).astype(np.float32).astype(np.float64) * 2
        ok = rng.random((I, Jk[k])) >= 0.15
        X.append(Xk); obs.append(ok)
        # slab k is the I x J_k x 1 block of the factors A, B_k and row k of C
        refs.append(em_ref.EmRef(Xk[:, :, None], ok[:, :, None], [A, Bk[k], C[k:k + 1]]))
    assert not all(o.all() for o in obs)
    want = np.sum([r.stats for r in refs], axis=0)
    Z = dict(loss_function=['Frobenius'], model=['PAR2'], modes=[[1, 2, 3]], size=[I, Jk, K],
             coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
             constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[X],
             miss=[[o.astype(np.uint8) for o in obs]], _ranks=[R] * 3)

    def once(update):
        pkg.build_model(eng, Z, 'f64')
        pkg.upload_state(eng, Z, dict(fac=[A, Bk, C]))
        return eng.resident_em_pass(0, (I, Jk, K), R, update=update, fuse=1)

    for update in (0, 1):
        out = once(update)
        assert out['info']['fused'] == -1 and out['mttkrp'] is None
        # sums: every slab's terms are within (2 rho + rho^2 + 80 u) of their own, so is the total of positive terms
        bnd = np.max([r.stat_bounds('f64') for r in refs], axis=0)
        rel = np.abs(out['stats'] - want) / want
        print('parafac2 em pass update=%d: sums %s of their bounds' % (update, ' '.join('%.3g' % v for v in rel / bnd)))
        assert np.all(rel <= bnd), (rel, bnd)
        for k in range(K):
            if update:
                assert np.array_equal(out['data'][k][obs[k]], X[k][obs[k]])
                assert refs[k].entry_ratio(out['data'][k][:, :, None], 'f64') <= 1.0
            else:
                assert np.array_equal(out['data'][k], X[k])
        assert once(update)['stats'].tobytes() == out['stats'].tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, eng):
    """Unmasked and sparse blocks are AOADMM_ERR_INVALID, a bad fuse value too; the engine works on afterwards."""
    capi = __import__('importlib').import_module('matlab-code_amd._capi')
    dims, R = (9, 7, 3), 2
    X, U, _ = _data(dims, R)
    Z = _block(dims, R, np.asfortranarray(X), np.ones(dims, dtype=bool))
    Z['miss'] = None
    pkg.build_model(eng, Z, 'f64')
    pkg.upload_state(eng, Z, dict(fac=list(U)))
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.resident_em_pass(0, dims, R)
    assert ei.value.code == capi.ERR_INVALID
    subs = np.argwhere(np.abs(X) > 1.0)
    eng.upload_coo(0, subs, X[tuple(subs.T)])
    with pytest.raises(pkg.AoadmmError) as ei:
        eng.resident_em_pass(0, dims, R)
    assert ei.value.code == capi.ERR_INVALID
    with pytest.raises(pkg.AoadmmError) as ei:
        _run(pkg, eng, dims, R, 'f64', fuse=3)
    assert ei.value.code == capi.ERR_INVALID
    _run(pkg, eng, dims, R, 'f64', mask=('frac', 0.1))
