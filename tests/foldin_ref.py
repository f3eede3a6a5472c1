"""The fold-in of DESIGN.md section 9.6 restated in numpy, in fp64 and in longdouble: the normal equations of every
query, the Cholesky solve, and the row ADMM loop for non-negativity (ADMM_constrained_only of the reference on one row,
cold-started).  numpy.linalg has no longdouble, so the factorisation and the substitutions are written out."""
import numpy as np

LD = np.longdouble


def zrows(U, mode, subs, dtype=np.float64):
    """z_e = prod_{m != mode} F_m(s_{e,m}, :) multiplied in mode order from 1: nobs x R."""
    z = np.ones((subs.shape[0], U[0].shape[1]), dtype=dtype)
    for m in range(len(U)):
        if m != mode:
            z = z * U[m].astype(dtype)[subs[:, m]]
    return z


def normal(U, mode, subs, vals, nq, dtype=np.float64):
    """(G nq x R x R, b nq x R): per query, over its observations in the caller's order, before any ridge."""
    R = U[0].shape[1]
    z = zrows(U, mode, subs, dtype)
    x = np.asarray(vals).astype(dtype)
    G = np.zeros((nq, R, R), dtype=dtype)
    b = np.zeros((nq, R), dtype=dtype)
    for q in range(nq):
        sel = np.flatnonzero(subs[:, mode] == q)
        G[q] = z[sel].T @ z[sel]
        b[q] = z[sel].T @ x[sel]
    return G, b


def cholesky(A):
    """Lower L with A = L L', or None when a pivot is not positive (the rule of the device: !(d > 0))."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def chol_solve(L, b):
    n = L.shape[0]
    y = np.zeros_like(b)
    for j in range(n):
        y[j] = (b[j] - L[j, :j] @ y[:j]) / L[j, j]
    u = np.zeros_like(b)
    for j in range(n - 1, -1, -1):
        u[j] = (y[j] - L[j + 1:, j] @ u[j + 1:]) / L[j, j]
    return u


def solve_row(G, b, ridge):
    """(u, info) of (G + ridge I) u = b; info 1 and a NaN row when the system is not positive definite."""
    R = G.shape[0]
    L = cholesky(G + G.dtype.type(ridge) * np.eye(R, dtype=G.dtype))
    if L is None:
        return np.full(R, np.nan, dtype=G.dtype), 1
    return chol_solve(L, b), 0


def _norm(v):
    return np.sqrt(v @ v)


def admm_row(G, b, ridge, max_inner, tol=(0.0, 0.0), trace=False):
    """The row loop: rho = trace(G) / R, L = chol(G + (ridge + rho / 2) I), z = mu = 0, then u = (b + rho / 2 (z - mu)) / B,
    z_old = z, z = max(u + mu, 0), mu += u - z, at least once and while iter < max_inner and a residual exceeds its
    tolerance.  Returns (z, info, iters[, the z of every iteration])."""
    R = G.shape[0]
    ty = G.dtype.type
    rho = np.trace(G) / ty(R)
    L = cholesky(G + (ty(ridge) + rho / ty(2)) * np.eye(R, dtype=G.dtype))
    if L is None:
        out = (np.full(R, np.nan, dtype=G.dtype), 1, 0)
        return out + ([],) if trace else out
    z = np.zeros(R, dtype=G.dtype)
    mu = np.zeros(R, dtype=G.dtype)
    it, zs = 0, []
    while True:
        u = chol_solve(L, b + rho / ty(2) * (z - mu))
        z_old = z
        z = np.maximum(u + mu, ty(0))
        mu = mu + u - z
        it += 1
        zs.append(z)
        with np.errstate(invalid='ignore', divide='ignore'):
            rp = _norm(u - z) / _norm(u)
            nmu = _norm(mu)
            rd = _norm(z - z_old) / nmu if nmu > 0 else _norm(z - z_old)
        if not (it < max_inner and (rp > tol[0] or rd > tol[1])):
            break
    return (z, 0, it, zs) if trace else (z, 0, it)


def fold_in(U, mode, subs, vals, nq, ridge=0.0, nonneg=False, max_inner=5, tol=(0.0, 0.0), dtype=np.float64):
    """(rows nq x R, info, iters) as Engine.fold_in returns them, in `dtype`."""
    G, b = normal(U, mode, subs, vals, nq, dtype)
    R = U[0].shape[1]
    rows = np.zeros((nq, R), dtype=dtype)
    info = np.zeros(nq, dtype=np.int32)
    iters = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        if nonneg:
            rows[q], info[q], iters[q] = admm_row(G[q], b[q], ridge, max_inner, tol)
        else:
            rows[q], info[q] = solve_row(G[q], b[q], ridge)
    return rows, info, iters


def make_list(rng, shape, mode, counts, values='normal', shuffle=True):
    """A list for `fold_in`: counts[q] observations of query q at random subscripts of the other modes.  values:
    'normal', or 'int' for integers in [-5, 5]."""
    nobs = int(np.sum(counts))
    subs = np.stack([rng.integers(0, s, nobs) for s in shape], axis=1).astype(np.int64)
    subs[:, mode] = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    vals = rng.integers(-5, 6, nobs).astype(np.float64) if values == 'int' else rng.standard_normal(nobs)
    if shuffle:
        perm = rng.permutation(nobs)
        subs, vals = subs[perm], vals[perm]
    return np.ascontiguousarray(subs), vals
