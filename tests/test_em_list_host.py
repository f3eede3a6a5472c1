"""CPU: the objective arithmetic of a masked block marked with `Engine.set_missing_list`.

Such a block's imputing pass visits the missing entries only, so the observed-entry residual is not summed directly but
combined on the host from what an unmasked block's objective uses and the two sums of the list pass:

    obs_res = (obs_x2 + den) - 2 dot + had - num

with Xhat the array the iteration's last MTTKRP ran on (observed data, previous imputation at the missing entries),
dot = <Xhat, M> = <mttkrp(Xhat, last mode), F_last>, had = ||M||^2 = sum of the Hadamard product of the Gram matrices,
num = sum_missing (m - xhat)^2 and den = sum_missing xhat^2.  The identity is exact; in fp64 the three large terms
cancel, so the bar is the one tests/test_gpu_objective.py uses for cancelled terms: 1e-12 (||Xhat||^2 + 2 |dot| + ||M||^2).
The reference is em_ref's longdouble direct sum over the observed entries.

The EM loop here is plain alternating least squares in fp64 numpy: the arithmetic of the combination is what is under
test, not the solver.  Noisy data only: a noise-free fit drives the direct sum far below the floor of the combined form
(1e-24 ||X||^2 against 1e-16 ||Xhat||^2), which is why the option is opt-in and documented so."""
import numpy as np
import pytest

import em_ref
from oracle.tensor_ops import mttkrp

BAR = 1e-12


def _noisy(dims, R, noise, rng):
    A = [rng.random((n, R)) for n in dims]
    X = em_ref.model(A, np.float64)
    N = rng.standard_normal(dims)
    X = X + noise * np.linalg.norm(X) / np.linalg.norm(N) * N
    return np.asfortranarray(X / np.linalg.norm(X))


def _combined(Xhat, obs, U, last):
    """(combined obs_res, scale of the bar) as objective_from_host forms them, fp64 throughout."""
    M = em_ref.model(U, np.float64)
    miss = ~obs
    num = float(((M[miss] - Xhat[miss]) ** 2).sum())
    den = float((Xhat[miss] ** 2).sum())
    obs_x2 = float((Xhat[obs] ** 2).sum())
    dot = float((mttkrp(Xhat, U, last) * U[last]).sum())
    had = np.ones((U[0].shape[1],) * 2)
    for F in U:
        had = had * (F.T @ F)
    had = float(had.sum())
    scale = float((Xhat ** 2).sum()) + 2 * abs(dot) + had
    return (obs_x2 + den) - 2.0 * dot + had - num, scale


def _direct(X, obs, U):
    return em_ref.EmRef(X, obs, U).stats[2]              # longdouble sum over the observed entries


@pytest.mark.parametrize('frac', [0.2, 0.01])
def test_combination_matches_the_direct_sum_over_an_em_run(frac):
    dims, R, iters = (37, 22, 19), 3, 12
    rng = np.random.default_rng(5)
    X = _noisy(dims, R, 0.05, rng)
    obs = np.ones(dims, dtype=bool)
    obs.flat[rng.choice(obs.size, int(frac * obs.size), replace=False)] = False
    Xhat = np.asfortranarray(np.where(obs, X, 0.0))
    U = [rng.random((n, R)) for n in dims]
    worst = 0.0
    for _ in range(iters):
        for n in range(len(dims)):
            G = np.ones((R, R))
            for m, F in enumerate(U):
                if m != n:
                    G = G * (F.T @ F)
            U[n] = np.linalg.solve(G, mttkrp(Xhat, U, n).T).T
        got, scale = _combined(Xhat, obs, U, len(dims) - 1)
        want = _direct(Xhat, obs, U)
        worst = max(worst, abs(got - want) / scale)
        assert abs(got - want) <= BAR * scale, (got, want, scale)
        assert want > 1e-6 * scale                        # noisy data: the residual sits far above the floor
        Xhat = np.asfortranarray(np.where(obs, Xhat, em_ref.model(U, np.float64)))
    print('combined form, %g missing: worst |difference| / scale = %.3g (bar %g)' % (frac, worst, BAR))


def test_combination_at_the_fused_pass_shape():
    """45 x 150 x 21, R = 6, 10 % noise, 20 % missing: one evaluation with arbitrary values under the mask."""
    dims, R = (45, 150, 21), 6
    rng = np.random.default_rng(6)
    X = _noisy(dims, R, 0.10, rng)
    obs = rng.random(dims) >= 0.2
    U = [rng.random((n, R)) / np.sqrt(n) for n in dims]
    for last in range(3):
        got, scale = _combined(X, obs, U, last)
        want = _direct(X, obs, U)
        assert abs(got - want) <= BAR * scale, (last, got, want, scale)


def test_empty_list_is_the_unmasked_formula():
    dims, R = (9, 7, 5), 2
    rng = np.random.default_rng(7)
    X = _noisy(dims, R, 0.05, rng)
    obs = np.ones(dims, dtype=bool)
    U = [rng.random((n, R)) for n in dims]
    got, scale = _combined(X, obs, U, 2)
    assert abs(got - float(((X - em_ref.model(U, np.float64)) ** 2).sum())) <= BAR * scale
