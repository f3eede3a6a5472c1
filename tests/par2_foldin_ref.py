"""The fold-in of new slabs into a fitted PARAFAC2 block restated in numpy, generic over fp64 and
longdouble: per slab Y = X'A, then W = Y diag(c) DeltaB', P = the polar factor of W, B = P DeltaB, b = diag(Y'B), the c step,
until c stops moving.  numpy.linalg has no longdouble, so the polar factor is a one-sided (Hestenes) Jacobi written out,
the Cholesky factorisation and its substitutions come from tests/foldin_ref.py, and so does the row loop for
non-negativity."""
import numpy as np

from foldin_ref import LD, admm_row, chol_solve, cholesky   # noqa: F401  (LD is re-exported)


def jacobi_polar(W, max_sweeps=60):
    """(P, sigma, lost): P = U V' of svd(W, 'econ') by one-sided Jacobi in W's dtype, cyclic over the pairs (p, q), p < q.
    A column whose norm after the sweeps is exactly 0 is lost: U keeps a zero column there (the device's convention)."""
    ty = W.dtype.type
    thr = ty(1e-15) if W.dtype == np.float64 else ty(1e-18)
    U = W.copy()
    n, R = U.shape
    V = np.eye(R, dtype=W.dtype)
    for _ in range(max_sweeps):
        rotated = False
        for p in range(R - 1):
            for q in range(p + 1, R):
                al, be, ga = U[:, p] @ U[:, p], U[:, q] @ U[:, q], U[:, p] @ U[:, q]
                if ga != 0 and abs(ga) > thr * np.sqrt(al * be):
                    zeta = (be - al) / (ty(2) * ga)
                    t = (ty(1) if zeta >= 0 else ty(-1)) / (abs(zeta) + np.sqrt(ty(1) + zeta * zeta))
                    c = ty(1) / np.sqrt(ty(1) + t * t)
                    s = c * t
                    up, uq = U[:, p].copy(), U[:, q].copy()
                    U[:, p], U[:, q] = c * up - s * uq, s * up + c * uq
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
                    rotated = True
        if not rotated:
            break
    sigma = np.sqrt(np.sum(U * U, axis=0))
    lost = bool(np.any(sigma == 0))
    with np.errstate(invalid='ignore', divide='ignore'):
        Un = np.where(sigma > 0, U / np.where(sigma > 0, sigma, ty(1)), ty(0))
    return Un @ V.T, sigma, lost


def system(A, DB, dtype=np.float64):
    """S = (A'A) .* (DeltaB'DeltaB) before any ridge."""
    A, DB = A.astype(dtype), DB.astype(dtype)
    return (A.T @ A) * (DB.T @ DB)


def _norm(v):
    return np.sqrt(v @ v)


def fold_in_slab(A, DB, X, c0=None, max_iter=50, tol=1e-8, ridge=0.0, nonneg=False, max_inner=5, inner_tol=(0.0, 0.0),
                 dtype=np.float64, trace=False):
    """One slab.  Returns a dict: c, B, P, res, xnorm, iters, info, Y, and with trace=True also cs (c after every
    iteration), ress (res after every iteration) and conds (sigma_min / sigma_max of W at every iteration).  Raises
    numpy.linalg.LinAlgError when the shared system is not positive definite."""
    ty = np.dtype(dtype).type
    A, DB, X = A.astype(dtype), DB.astype(dtype), np.asarray(X).astype(dtype)
    R = A.shape[1]
    Y = X.T @ A
    S = (A.T @ A) * (DB.T @ DB)
    xnorm = np.sum(X * X)
    L = None
    if not nonneg:
        L = cholesky(S + ty(ridge) * np.eye(R, dtype=dtype))
        if L is None:
            raise np.linalg.LinAlgError('S + ridge I is not positive definite')
    elif cholesky(S + (ty(ridge) + np.trace(S) / ty(R) / ty(2)) * np.eye(R, dtype=dtype)) is None:
        raise np.linalg.LinAlgError('S + (ridge + rho / 2) I is not positive definite')
    c = np.ones(R, dtype=dtype) if c0 is None else np.asarray(c0).astype(dtype)
    it, info = 0, 0
    cs, ress, conds = [], [], []
    while True:
        W = (Y * c) @ DB.T
        P, sigma, lost = jacobi_polar(W)
        info |= int(lost)
        B = P @ DB
        b = np.sum(Y * B, axis=0)
        c_old = c
        if nonneg:
            c = admm_row(S, b, ridge, max_inner, inner_tol)[0]
        else:
            c = chol_solve(L, b)
        it += 1
        if trace:
            cs.append(c)
            ress.append(xnorm - ty(2) * (c @ b) + c @ S @ c)
            with np.errstate(invalid='ignore', divide='ignore'):
                conds.append(float(sigma.min() / sigma.max()) if sigma.max() > 0 else 0.0)
        with np.errstate(invalid='ignore'):
            if it >= max_iter or _norm(c - c_old) <= ty(tol) * _norm(c):
                break
    res = xnorm - ty(2) * (c @ b) + c @ S @ c
    out = dict(c=c, B=B, P=P, res=res, xnorm=xnorm, iters=it, info=info, Y=Y)
    if trace:
        out.update(cs=cs, ress=ress, conds=conds)
    return out


def fold_in(A, DB, slabs, c0=None, **kw):
    """Every slab of a call: a dict of lists / arrays as Engine.par2_fold_in returns them (C nk x R, B, P, Y lists)."""
    outs = [fold_in_slab(A, DB, X, None if c0 is None else c0[q], **kw) for q, X in enumerate(slabs)]
    dt = kw.get('dtype', np.float64)
    return dict(C=np.array([o['c'] for o in outs], dtype=dt).reshape(len(outs), A.shape[1]), B=[o['B'] for o in outs],
                P=[o['P'] for o in outs], Y=[o['Y'] for o in outs], res=np.array([o['res'] for o in outs], dtype=dt),
                xnorm=np.array([o['xnorm'] for o in outs], dtype=dt), iters=np.array([o['iters'] for o in outs], dtype=np.int32),
                info=np.array([o['info'] for o in outs], dtype=np.int32), outs=outs)


def make_model(rng, R, I):
    """The recipe of the tests: A standard normal, DeltaB = Q + 0.1 N with Q orthogonal."""
    A = rng.standard_normal((I, R))
    Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    return A, Q + 0.1 * rng.standard_normal((R, R))


def make_slab(rng, A, DB, J, noise=0.05):
    """X = A diag(c) (P DeltaB)' with c in [0.75, 1.25] and P orthonormal J x R, plus `noise` of its norm.  Returns (X, c, P)."""
    R = A.shape[1]
    c = 0.75 + 0.5 * rng.random(R)
    P, _ = np.linalg.qr(rng.standard_normal((J, R)))
    X = (A * c) @ (P @ DB).T
    if noise > 0:
        N = rng.standard_normal(X.shape)
        X = X + noise * np.linalg.norm(X) / np.linalg.norm(N) * N
    return X, c, P
