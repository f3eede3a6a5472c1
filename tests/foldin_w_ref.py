"""The weighted fold-in of DESIGN.md section 9.6 restated in numpy, in fp64 and in longdouble, and the definition it is
pinned to.  With w_e in [0, 1] per listed observation and alpha in [0, 1] for every cell of the new row that the list
does not name (data 0 there):

    G_q = sum_e (w_e - alpha) z_e z_e' + alpha H,   b_q = sum_e (w_e x_e) z_e,   H = had_{m != mode} F_m'F_m

The solve and the row ADMM loop are those of tests/foldin_ref.py.  `dense_problem` builds the definition itself: the
weight row W over all cells of the other modes, Z over all cells, x with zeros at the unlisted cells."""
import numpy as np

import foldin_ref as FR

LD = FR.LD


def hadamard_gram(U, mode, dtype=np.float64):
    """H = had_{m != mode} F_m'F_m over all rows, multiplied in mode order."""
    R = U[0].shape[1]
    H = np.ones((R, R), dtype=dtype)
    for m in range(len(U)):
        if m != mode:
            F = U[m].astype(dtype)
            H = H * (F.T @ F)
    return H


def normal(U, mode, subs, vals, wts, alpha, nq, dtype=np.float64):
    """(G nq x R x R with alpha H included, b nq x R), before any ridge.  wts None: all ones."""
    R = U[0].shape[1]
    z = FR.zrows(U, mode, subs, dtype)
    x = np.asarray(vals).astype(dtype)
    w = np.ones(len(x), dtype=dtype) if wts is None else np.asarray(wts).astype(dtype)
    a = dtype(alpha)
    aH = a * hadamard_gram(U, mode, dtype) if alpha != 0 else np.zeros((R, R), dtype=dtype)
    G = np.zeros((nq, R, R), dtype=dtype)
    b = np.zeros((nq, R), dtype=dtype)
    for q in range(nq):
        sel = np.flatnonzero(subs[:, mode] == q)
        G[q] = ((w[sel] - a)[:, None] * z[sel]).T @ z[sel] + aH
        b[q] = z[sel].T @ (w[sel] * x[sel])
    return G, b


def fold_in(U, mode, subs, vals, wts, alpha, nq, ridge=0.0, nonneg=False, max_inner=5, tol=(0.0, 0.0), dtype=np.float64):
    """(rows nq x R, info, iters) as Engine.fold_in(..., weights=wts, unstored_weight=alpha) returns them, in `dtype`."""
    G, b = normal(U, mode, subs, vals, wts, alpha, nq, dtype)
    R = U[0].shape[1]
    rows = np.zeros((nq, R), dtype=dtype)
    info = np.zeros(nq, dtype=np.int32)
    iters = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        if nonneg:
            rows[q], info[q], iters[q] = FR.admm_row(G[q], b[q], ridge, max_inner, tol)
        else:
            rows[q], info[q] = FR.solve_row(G[q], b[q], ridge)
    return rows, info, iters


def all_cells(shape, mode):
    """Every cell of the other modes as rows of subscripts (column `mode` zero): prod(other) x N, first other mode fastest."""
    other = [m for m in range(len(shape)) if m != mode]
    grids = np.meshgrid(*[np.arange(shape[m]) for m in other], indexing='ij')
    cells = np.zeros((grids[0].size, len(shape)), dtype=np.int64)
    for m, g in zip(other, grids):
        cells[:, m] = g.reshape(-1, order='F')
    return cells


def dense_problem(U, mode, subs, vals, wts, alpha):
    """One query (column `mode` of subs is ignored), each cell listed at most once: (Z over all cells, the weight row W,
    the data row x) of  min_u sum_cells W (x - Z u)^2."""
    shape = [u.shape[0] for u in U]
    other = [m for m in range(len(shape)) if m != mode]
    cells = all_cells(shape, mode)
    Z = FR.zrows(U, mode, cells)
    dims = [shape[m] for m in other]
    lin = np.ravel_multi_index(tuple(subs[:, m] for m in other), dims, order='F')
    assert len(np.unique(lin)) == len(lin)
    W = np.full(len(cells), float(alpha))
    x = np.zeros(len(cells))
    W[lin] = np.ones(len(lin)) if wts is None else wts
    x[lin] = vals
    return Z, W, x


def make_cells(rng, shape, mode, nq, frac, values='normal'):
    """A list in which every query names a random `frac` of the cells of the other modes, each once; shuffled."""
    cells = all_cells(shape, mode)
    parts = []
    for q in range(nq):
        pick = cells[rng.random(len(cells)) < frac].copy()
        pick[:, mode] = q
        parts.append(pick)
    subs = np.concatenate(parts)
    subs = subs[rng.permutation(len(subs))]
    vals = rng.integers(-5, 6, len(subs)).astype(np.float64) if values == 'int' else rng.standard_normal(len(subs))
    return np.ascontiguousarray(subs), vals
