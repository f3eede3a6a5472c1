"""numpy references of the Tucker projection and of core consistency, and the planted case the
host and GPU tests share."""
import copy
import functools

import numpy as np

from helpers import options


def ref_core(X, M):
    """G = X x_1 M[0]' x_2 M[1]' x_3 M[2]'"""
    return np.einsum('ijk,ip,jq,kr->pqr', np.asarray(X, dtype=np.float64), M[0], M[1], M[2], optimize=True)


def ref_bound(X, M):
    """The same contraction on absolute values: what every rounding error of a projection is measured against."""
    return ref_core(np.abs(X), [np.abs(m) for m in M])


def ref_cc(core):
    R = core.shape[0]
    T = np.zeros((R, R, R))
    for r in range(R):
        T[r, r, r] = 1.0
    return 100.0 * (1.0 - np.sum((np.asarray(core) - T) ** 2) / R)


def pinv_t(F, how='svd'):
    """F (F'F)^+ = pinv(F)': by numpy's SVD pseudo-inverse, or as F inv(F'F) in longdouble."""
    if how == 'svd':
        return np.linalg.pinv(F).T.copy()
    Fl = np.asarray(F, dtype=np.longdouble)
    G = Fl.T @ Fl
    R = G.shape[0]
    A = np.concatenate([G, np.eye(R, dtype=np.longdouble)], axis=1)      # Gauss-Jordan with partial pivoting
    for c in range(R):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, piv]] = A[[piv, c]]
        A[c] = A[c] / A[c, c]
        for i in range(R):
            if i != c:
                A[i] = A[i] - A[i, c] * A[c]
    return np.asarray(Fl @ A[:, R:], dtype=np.float64)


def pinv_floor(X, F):
    """Largest entrywise |ref_core(X, pinv_t svd) - ref_core(X, pinv_t longdouble)| / ref_bound: the disagreement of two
    host formulations of the same core, below which no device result can be judged."""
    Ms, Ml = [pinv_t(f) for f in F], [pinv_t(f, 'longdouble') for f in F]
    return float(np.max(np.abs(ref_core(X, Ms) - ref_core(X, Ml)) / ref_bound(X, Ms)))


# ---- the planted case: 12 x 10 x 8, rank 3, uniform factors + 0.1, noise 5 % of the mean magnitude --------------------
PLANTED_DIMS, PLANTED_SEED, PLANTED_ITERS = (12, 10, 8), 1, 500
# The oracle's fit (oracle.aoadmm, unconstrained, PLANTED_ITERS outer iterations) has cc = 97.31 at R = 3 and -21.72 at
# R = 4.  Room is measured on 100 - cc = 100 sum (core - T)^2 / R, the quantity that grows with the misfit: 2.69 and
# 121.7.  "Good" is 100 - cc < 10 (3.7 times the oracle's), "bad" is 100 - cc > 50 (2.4 times below the oracle's).
# (Of seeds 0..5 this one has the mildest two-factor degeneracy at R = 4; the others reach -185 to -1.4e8.)
CC_OK_ABOVE, CC_BAD_BELOW = 90.0, 50.0


def planted_data():
    rng = np.random.default_rng(PLANTED_SEED)
    A = [rng.random((n, 3)) + 0.1 for n in PLANTED_DIMS]
    X = np.einsum('ir,jr,kr->ijk', *A)
    X = X + 0.05 * np.mean(np.abs(X)) * rng.standard_normal(X.shape)
    return np.asfortranarray(X)


def planted_model(R):
    """(Z, G, alg_options): the unconstrained CP block of the planted data at rank R with a fixed random start."""
    from oracle import aoadmm as OA
    X = planted_data()
    rng = np.random.default_rng(100 + R)
    Z = dict(loss_function=['Frobenius'], model=['CP'], modes=[[1, 2, 3]], size=list(PLANTED_DIMS),
             coupling=dict(lin_coupled_modes=[0, 0, 0], coupling_type=[], coupl_trafo_matrices=[None] * 3),
             constrained_modes=[0, 0, 0], constraints=[None] * 3, weights=[1.0], object=[X])
    io = dict(lambdas_init=[[1] * R], nvecs=0, distr=[lambda a, b: rng.random((a, b))] * 3, normalize=1)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=rng)
    return Z, G, options(MaxOuterIters=PLANTED_ITERS)


@functools.lru_cache(maxsize=None)
def planted_oracle_cc(R):
    """Core consistency of the oracle's fit at rank R, in numpy."""
    from oracle import aoadmm as OA
    Z, G, opt = planted_model(R)
    _, Fo, _, _ = OA.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G))
    return float(ref_cc(ref_core(Z['object'][0], [pinv_t(f) for f in Fo['fac']])))
