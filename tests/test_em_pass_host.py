"""CPU: the reference and the bounds of tests/em_ref.py, which tests/test_gpu_em_pass.py holds the device EM pass to.
The reference is pinned to the oracle's tensor operations; the bounds are checked against a numpy emulation of the strip
kernel's fp32 arithmetic (em_ref.emulate_f32_pass): correct arithmetic must stay inside all of them, with room."""
import numpy as np
import pytest

import em_ref
from oracle.tensor_ops import full_ktensor, mttkrp as o_mttkrp

SHAPES = [((37, 70, 9), 5), ((9, 130, 11), 20), ((64, 65, 5), 24), ((130, 3, 20), 32)]


def _case(dims, R, frac=0.05):
    rng = np.random.default_rng(1000 * sum(dims) + R)
    X, U = em_ref.make_data(dims, R, rng)
    obs = rng.random(dims) >= frac
    return X, obs, U


def test_model_matches_the_oracle():
    """em_ref.model (3-way and the merged Khatri-Rao order of a 4-way block) is the oracle's full_ktensor."""
    rng = np.random.default_rng(3)
    for dims in ((7, 5, 4), (7, 5, 4, 3), (6, 9)):
        U = em_ref.random_factors(dims, 3, rng)
        M = em_ref.model(U)
        assert M.shape == dims
        assert np.abs(M.astype(np.float64) - full_ktensor(U)).max() < 1e-13
        assert np.abs(em_ref.model(U, np.float64) - full_ktensor(U)).max() < 1e-13


def test_reference_pass():
    """The four sums against a direct fp64 restatement, X_new against its definition, and the data generator's
    promises: values exact in fp32, non-zero at every position, residuals of the size of the data."""
    dims, R = (11, 13, 6), 4
    X, obs, U = _case(dims, R, 0.2)
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64)) and np.all(X != 0)
    ref = em_ref.EmRef(X, obs, U)
    M = full_ktensor(U)
    want = [((M - X)[~obs] ** 2).sum(), (X[~obs] ** 2).sum(), ((X - M)[obs] ** 2).sum(), (X[obs] ** 2).sum()]
    assert np.allclose(ref.stats, want, rtol=1e-13, atol=0)
    assert np.array_equal(ref.X_new[obs], X[obs]) and np.abs(ref.X_new[~obs] - M[~obs]).max() < 1e-13
    assert 0.1 < ref.stats[2] / ref.stats[3] < 10                     # residuals are O(|X|)
    for n in range(3):
        assert np.allclose(ref.mttkrp(n), o_mttkrp(np.where(obs, X, M), U, n), rtol=1e-12, atol=1e-12)


def test_bounds_of_an_empty_sum_are_zero():
    dims, R = (5, 6, 3), 2
    X, _, U = _case(dims, R)
    ref = em_ref.EmRef(X, np.ones(dims, dtype=bool), U)
    assert ref.stats[0] == 0 and ref.stats[1] == 0
    b = ref.stat_bounds('f32')
    assert b[0] == 0 and b[1] == 0 and b[2] > 0 and b[3] == em_ref.SUM_TERMS * 2.0 ** -24
    assert np.array_equal(ref.stat_ratios(ref.stats, 'f32'), np.zeros(4))
    assert ref.stat_ratios([1e-30, 0, ref.stats[2], ref.stats[3]], 'f32')[0] == np.inf
    assert ref.entry_ratio(X, 'f32') == 0.0


@pytest.mark.parametrize('dims,R', SHAPES, ids=['%dx%dx%d-R%d' % (*d, R) for d, R in SHAPES])
def test_fp32_emulation_stays_inside_the_bounds(dims, R):
    """The kernel's arithmetic, emulated: every imputed value within beta, every statistic within its bound.  The
    ratios printed here were at most 0.40 (entries) and 0.01 (sums) when the bounds were written."""
    X, obs, U = _case(dims, R)
    ref = em_ref.EmRef(X, obs, U)
    m, stats = em_ref.emulate_f32_pass(X, obs, U)
    x_new = np.where(obs, X, m.astype(np.float64))
    re = ref.entry_ratio(x_new, 'f32')
    rs = ref.stat_ratios(stats, 'f32')
    print('emulated fp32 pass %s R=%d: entry %.3f of beta, sums %s of their bounds' % (dims, R, re, np.round(rs, 4)))
    assert 0 < re <= 1.0
    assert np.all(rs <= 1.0), rs
    # the bounds are not vacuous: a value one beta-sized step further off is caught, and so is a lost entry
    worst = np.unravel_index(np.argmax(np.where(obs, 0, ref.beta('f32'))), dims)
    bad = x_new.copy()
    bad[worst] = float(ref.M[worst]) + 1.5 * ref.beta('f32')[worst]
    assert ref.entry_ratio(bad, 'f32') > 1.0
    lost = x_new.copy()
    lost[worst] = X[worst]
    assert ref.entry_ratio(lost, 'f32') > 1e3
    # dropping one missing entry's term from num is caught whenever it is a visible share of the sum
    d2 = float(ref.d[worst] ** 2)
    if d2 / ref.stats[0] > 2 * ref.stat_bounds('f32')[0]:
        assert ref.stat_ratios([stats[0] - d2, stats[1], stats[2], stats[3]], 'f32')[0] > 1.0


def test_fp64_bound_holds_for_plain_fp64_arithmetic():
    """The same chain in fp64 (numpy's own products and sums) stays inside the fp64 beta against the longdouble model."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps      # the reference needs a wider type than fp64
    dims, R = (9, 130, 11), 20
    X, obs, U = _case(dims, R)
    ref = em_ref.EmRef(X, obs, U)
    A, B, C = U
    m = np.zeros(dims)
    for r in range(R):
        m = m + (A[:, None, None, r] * C[None, None, :, r]) * B[None, :, None, r]
    assert 0 < ref.entry_ratio(np.where(obs, X, m), 'f64') <= 1.0
