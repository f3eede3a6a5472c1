"""Host side of the per-kernel-class prox tests (numpy only; imported by test_prox_ref_host.py on the CPU and by
test_gpu_prox_classes.py, test_gpu_ops.py and test_gpu_admm.py on the GPU).

  * make_input(case): one generator per input *kind*, seeded from zlib.crc32 of the case id (hash() of a str changes
    from process to process).  Every column of a case holds different data, so an indexing error between columns shows.
  * reference(c, X, rho): oracle.prox.constraints_to_prox; GL smoothness above 1000 rows by the banded solve gl_banded
    (the oracle builds the dense matrix), which test_prox_ref_host.py pins to the oracle.
  * prox_class(c, rows, R): pure-Python mirror of the dispatch of prox_apply / tv_fast_launch (csrc/prox.hip) and
    prox_iso / prox_gl_pcr (csrc/iso.hip).  test_prox_ref_host.py reads the constants below back from the sources, so a
    retuned dispatch fails there ("pick a new shape") instead of silently moving a case to another kernel.
  * CASES: every case names, as a literal, the class it is meant to hit.
  * POLAR_FLOOR: distance of numpy's SVD polar factor from a 40-digit one for the ill-conditioned orthonormal cases,
    measured on the host (test_prox_ref_host.py re-measures it with mpmath); the device never enters it.
"""
import collections
import zlib

import numpy as np

from oracle import prox as OP

RHO = 1.7

# ---------------------------------------------------------------------------------------------------------------------
# dispatch mirror.  The constants are compared with the sources in test_prox_ref_host.py.
ROWS_STEPS = (8, 16, 32)                 # prox_apply: prox_rows_k<8|16|32|64>
TV_PAR_MAX = 6400                        # kTvParMax: all working arrays of a column in LDS
TV_HYBRID_MAX = 12000                    # kTvHybridMax: Pc / start / J in LDS, the rest in the workspace
TV_SHORT_ROWS = 1024                     # tv_fast_launch: 256 threads up to here, 1024 above
TV_STAGE_STEPS = (1, 2, 4)               # prox_tv_fast_k: entries staged per thread (8 beyond 4 x threads)
ISO_ONE_KERNEL_ROWS = 512                # kIsoOneKernelRows: prox_iso_k does the comparisons itself
ISO_SMALL_ROWS = 256                     # prox_iso: prox_iso_k<256, true>
ISO_LDS_ROWS = 2048                      # kIsoLdsRows: prox_iso_k<1024, true>
ISO_PREV_LDS_ROWS = 6000                 # kIsoPrevLdsRows: iso_prev_k<256, true>
ISO_SHARE_BUDGET, ISO_SHARE_MAX = 512, 64
GL_STEPS = (256, 1024, 4096)             # prox_gl_pcr: <256,1>, <1024,1>, <1024,4>, prox_gl_pcr_long_k

ROW_WISE = ('non-negativity', 'box', 'l1 regularization', 'l0 regularization', 'ridge', 'simplex row-wise')
COL_NORM = ('l2-ball', 'non-negative l2-ball', 'non-negative l2-sphere', 'l2 regularization')
SIMPLEX_COL = ('simplex column-wise', 'l1-ball')
ISOTONIC = ('non-decreasing', 'non-increasing', 'unimodality')


def iso_shares(R, ndir):
    return max(1, min(ISO_SHARE_MAX, ISO_SHARE_BUDGET // (R * ndir)))


def prox_class(c, rows, R):
    """Name of the kernel class `eng.prox(c, X, rho)` runs for a rows x R input (op entry: workspace present,
    leading dimension = rows)."""
    name = c[0]
    if name in ROW_WISE:
        for s in ROWS_STEPS:
            if R <= s:
                return 'rows<%d>' % s
        return 'rows<64>'
    if name in COL_NORM:
        return 'colnorm'
    if name in SIMPLEX_COL:
        return 'simplexcol'
    if name == 'TV regularization':
        if rows > TV_HYBRID_MAX:
            return 'tv-1024thr-workspace'
        if rows > TV_PAR_MAX:
            return 'tv-1024thr-hybrid'
        thr = 1024 if rows > TV_SHORT_ROWS else 256
        for k in TV_STAGE_STEPS:
            if rows <= k * thr:
                return 'tv-%dthr-x%d' % (thr, k)
        return 'tv-%dthr-x8' % thr
    if name in ISOTONIC:
        ndir = 2 if name == 'unimodality' else 1
        main = 'iso256' if rows <= ISO_SMALL_ROWS else ('isolds' if rows <= ISO_LDS_ROWS else 'isoglobal')
        if rows <= ISO_ONE_KERNEL_ROWS:
            return 'iso-prevself-%s' % main
        prev = 'prevlds' if rows <= ISO_PREV_LDS_ROWS else 'prevglobal'
        return 'iso-%s-%s-shares%d' % (prev, main, iso_shares(R, ndir))
    if name == 'GL smoothness':
        if rows <= GL_STEPS[0]:
            return 'gl-256thr-x1'
        if rows <= GL_STEPS[1]:
            return 'gl-1024thr-x1'
        if rows <= GL_STEPS[2]:
            return 'gl-1024thr-x4'
        return 'gl-long'
    if name == 'orthonormal':
        return 'ortho'
    raise ValueError('no device class for %r' % (name,))


# ---------------------------------------------------------------------------------------------------------------------
# references
def gl_banded(x, rho, eta):
    """(2*eta/rho*L + I) \\ x with the path-graph Laplacian L (constraints_to_prox.m:68-76) by a banded solve: the
    oracle builds the dense matrix (3 GB at 20 000 rows), so long columns are checked against this and this against
    the oracle."""
    from scipy.linalg import solveh_banded
    n = x.shape[0]
    g = 2.0 * eta / rho
    if n == 1:
        return x / (g + 1.0)
    ab = np.zeros((2, n))
    ab[0, 1:] = -g                                   # upper diagonal of g*L + I, L = gl_laplacian(n)
    ab[1, :] = 2.0 * g + 1.0
    ab[1, 0] = ab[1, -1] = g + 1.0
    return solveh_banded(ab, x)


def reference(c, X, rho=RHO):
    if c[0] == 'GL smoothness' and X.shape[0] > 1000:
        return gl_banded(X, rho, c[1])
    return OP.constraints_to_prox([1], [c], [X.shape[0]])[0][0](X, rho)


def unimodal_tied_check(got, ref, X, nonneg):
    """Tied unimodal splits.  Integer data: many splits have exactly the same criterion value and the projection is
    not unique.  The reference's pick among them is decided by the rounding of its error sums
    (project_unimodal_vector.m:67-72 accumulates them pool by pool); the device takes the first split within a few ulp
    of the minimum.  Every column must then be feasible and exactly as close to the input as the oracle's."""
    for r in range(X.shape[1]):
        g = got[:, r]
        pk = int(np.argmax(g))
        assert np.all(np.diff(g[:pk + 1]) >= 0) and np.all(np.diff(g[pk:]) <= 0)
        assert not nonneg or g.min() >= 0
        eg, er = np.sum((g - X[:, r]) ** 2), np.sum((ref[:, r] - X[:, r]) ** 2)
        assert abs(eg - er) <= 1e-12 * er, (r, eg, er)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def _feasible(rng, c, rows, R):
    """A point of the constraint's set (for 'l2 regularization': a column the prox sends to zero)."""
    name = c[0]
    col = 0.3 + 0.6 * (np.arange(R) + 1.0) / R          # a different fraction of the bound per column
    if name in ('l2-ball', 'l2 regularization'):
        X = rng.standard_normal((rows, R))
        bound = c[1] if name == 'l2-ball' else c[1] / RHO
        return X / np.linalg.norm(X, axis=0) * (bound * col)
    if name in ('non-negative l2-ball', 'non-negative l2-sphere'):
        X = np.abs(rng.standard_normal((rows, R)))
        return X / np.linalg.norm(X, axis=0) * (c[1] * col if name == 'non-negative l2-ball' else 1.0)
    if name == 'simplex column-wise':
        X = rng.random((rows, R))
        return X / X.sum(axis=0) * c[1]
    if name == 'l1-ball':
        X = rng.standard_normal((rows, R))
        return X / np.abs(X).sum(axis=0) * (c[1] * col)
    if name == 'simplex row-wise':
        X = rng.random((rows, R))
        return X / X.sum(axis=1, keepdims=True) * c[1]
    raise ValueError(name)


def boundary_eta(rows):
    """l1 norm of every column of the 'on-boundary' input."""
    return float(np.sum(np.arange(rows) % 4))


def make_input(case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    rows, R, kind, c = case.rows, case.R, case.kind, case.c
    if kind == 'noise':
        return rng.standard_normal((rows, R))
    if kind == 'smooth':                                # a random walk under noise (GL smoothness)
        return np.cumsum(rng.standard_normal((rows, R)), axis=0) * 0.05 + rng.standard_normal((rows, R))
    if kind == 'ties':
        return rng.integers(-2, 3, size=(rows, R)).astype(float)
    if kind == 'constant':
        return np.tile(0.25 * (np.arange(R) + 1.0) - 1.0, (rows, 1))
    if kind == 'feasible':
        return _feasible(rng, c, rows, R)
    if kind == 'zero-col':
        X = rng.standard_normal((rows, R))
        X[:, R // 2] = 0.0
        return X
    if kind == 'one-dominant':
        X = 0.01 * rng.standard_normal((rows, R))
        r = np.arange(R)
        X[(7 * r + 3) % rows, r] = 5.0 + r
        return X
    if kind == 'allneg':
        return -np.abs(rng.standard_normal((rows, R))) - 0.1
    if kind == 'on-boundary':                           # integers, every column's l1 norm == boundary_eta(rows)
        X = np.stack([rng.permutation(np.arange(rows) % 4) for _ in range(R)], axis=1).astype(float)
        if c[0] == 'l1-ball':
            X *= rng.choice([-1.0, 1.0], size=(rows, R))
        return X
    if kind == 'steps':
        lv = rng.standard_normal((rows // 50 + 1, R))
        return np.repeat(lv, 50, axis=0)[:rows] + 0.05 * rng.standard_normal((rows, R))
    if kind == 'sphere-tie':                            # no positive entry; the maximum is tied within each column
        X = -np.abs(rng.standard_normal((rows, R))) - 0.5
        for r, (i, j) in enumerate(SPHERE_TIES):
            X[i, r] = X[j, r] = -0.125 * r              # column 0: tied zeros
        return X
    if kind.startswith('illcond'):
        cond = float(kind[len('illcond'):])
        U, _ = np.linalg.qr(rng.standard_normal((rows, R)))
        V, _ = np.linalg.qr(rng.standard_normal((R, R)))
        return U @ np.diag(np.logspace(0.0, -np.log10(cond), R)) @ V.T
    raise ValueError(kind)


# tied maxima of the sphere's one-hot fallback (256 threads, thread t reads rows t, t + 256, ...): rows 3 and 259 are
# two strides of one thread, rows 5 and 200 two threads, rows 2 and 258 the last stride of a 260-row column
SPHERE_TIES = ((3, 259), (5, 200), (2, 258))

# ---------------------------------------------------------------------------------------------------------------------
# cases
Case = collections.namedtuple('Case', 'id family c rows R kind cls')


def _case(family, c, rows, R, kind, cls, tag=''):
    par = ''.join('-%g' % p for p in c[1:] if not isinstance(p, bool)) + ''.join('-nn' for p in c[1:] if p is True)
    return Case('%s%s%s-%s-%dx%d' % (c[0], par, tag, kind, rows, R), family, c, rows, R, kind, cls)


def _build_cases():
    out = []
    # --- rows kernel.  l1 / l0: about half of the N(0,1) entries on each side of the threshold
    # (|x| > eta/rho at 0.6745 / x^2 > 2 eta/rho at 0.455)
    rows_cls = {8: 'rows<8>', 9: 'rows<16>', 16: 'rows<16>', 17: 'rows<32>', 32: 'rows<32>', 33: 'rows<64>', 64: 'rows<64>'}
    shapes = [(129, R) for R in (8, 9, 16, 17, 32, 33, 64)] + [(1, 64)]
    for rows, R in shapes:
        for c in (('non-negativity',), ('box', -0.3, 0.4), ('l1 regularization', 0.6745 * RHO),
                  ('l0 regularization', 0.5 * 0.455 * RHO), ('ridge', 0.3), ('simplex row-wise', 2.0)):
            out.append(_case('rows', c, rows, R, 'noise', rows_cls[R]))
        for kind in ('ties', 'feasible'):
            out.append(_case('rows', ('simplex row-wise', 2.0), rows, R, kind, rows_cls[R]))
    # --- column-norm family
    col_shapes = [(255, 3), (256, 3), (257, 3), (257, 64)]
    for c in (('l2-ball', 1.0), ('non-negative l2-ball', 1.0), ('non-negative l2-sphere', 1.0), ('l2 regularization', 0.5)):
        for rows, R in col_shapes:
            for kind in ('noise', 'zero-col', 'feasible', 'allneg'):
                out.append(_case('colnorm', c, rows, R, kind, 'colnorm'))
    out.append(_case('colnorm', ('non-negative l2-sphere', 1.0), 260, 3, 'sphere-tie', 'colnorm'))
    # --- simplex column-wise / l1-ball
    for name in SIMPLEX_COL:
        for rows, R in col_shapes:
            for kind in ('noise', 'ties', 'feasible', 'one-dominant'):
                out.append(_case('simplexcol', (name, 3.0), rows, R, kind, 'simplexcol'))
            out.append(_case('simplexcol', (name, boundary_eta(rows)), rows, R, 'on-boundary', 'simplexcol'))
            out.append(_case('simplexcol', (name, 1e3), rows, R, 'noise', 'simplexcol'))      # every entry active
    # --- TV
    tv_cls = {2: 'tv-256thr-x1', 3: 'tv-256thr-x1', 256: 'tv-256thr-x1', 257: 'tv-256thr-x2', 512: 'tv-256thr-x2',
              513: 'tv-256thr-x4', 1000: 'tv-256thr-x4', 1024: 'tv-256thr-x4', 1025: 'tv-1024thr-x2',
              2048: 'tv-1024thr-x2', 2049: 'tv-1024thr-x4', 4096: 'tv-1024thr-x4', 12000: 'tv-1024thr-hybrid',
              12001: 'tv-1024thr-workspace'}
    tv_eta = {'noise': 0.4, 'steps': 0.3, 'ties': 0.8, 'constant': 0.4}     # several segments survive (but 'constant')
    for rows in (2, 3, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 12000, 12001):
        for kind in ('noise', 'steps', 'ties'):
            out.append(_case('tv', ('TV regularization', tv_eta[kind]), rows, 2, kind, tv_cls[rows]))
    for kind in ('noise', 'steps', 'ties'):
        out.append(_case('tv', ('TV regularization', tv_eta[kind]), 1000, 64, kind, tv_cls[1000]))
    out.append(_case('tv', ('TV regularization', 0.4), 513, 2, 'constant', tv_cls[513]))
    # --- isotonic / unimodal: class by rows and by the share count of (R, directions)
    iso_cls = {255: 'iso-prevself-iso256', 256: 'iso-prevself-iso256', 257: 'iso-prevself-isolds',
               512: 'iso-prevself-isolds', 513: 'iso-prevlds-isolds', 2048: 'iso-prevlds-isolds',
               2049: 'iso-prevlds-isoglobal', 6000: 'iso-prevlds-isoglobal', 6001: 'iso-prevglobal-isoglobal'}
    shares = {(3, 1): 64, (3, 2): 64, (64, 1): 8, (64, 2): 4, (5, 1): 64, (5, 2): 51, (20, 1): 25, (20, 2): 12}
    iso_shapes = [(rows, 3) for rows in (255, 256, 257, 512, 513, 2048, 2049, 6000, 6001)] + [(513, 64), (6001, 5), (6001, 20)]
    for c in (('non-decreasing',), ('non-increasing',), ('unimodality', True), ('unimodality', False)):
        ndir = 2 if c[0] == 'unimodality' else 1
        for rows, R in iso_shapes:
            cls = iso_cls[rows] + ('-shares%d' % shares[(R, ndir)] if rows > 512 else '')
            for kind in ('noise', 'ties'):
                out.append(_case('iso', c, rows, R, kind, cls))
        out.append(_case('iso', c, 257, 3, 'constant', iso_cls[257]))
    # --- GL smoothness
    gl_cls = {2: 'gl-256thr-x1', 3: 'gl-256thr-x1', 256: 'gl-256thr-x1', 257: 'gl-1024thr-x1', 1024: 'gl-1024thr-x1',
              1025: 'gl-1024thr-x4', 4096: 'gl-1024thr-x4'}
    for rows, R in [(rows, 3) for rows in (2, 3, 256, 257, 1024, 1025, 4096)] + [(257, 64)]:
        for eta in (1e-3, 0.7, 40.0):
            out.append(_case('gl', ('GL smoothness', eta), rows, R, 'smooth', gl_cls[rows]))
    # --- orthonormal
    for R in (1, 2, 33, 64):
        for rows in (R, R + 1, 129):
            out.append(_case('ortho', ('orthonormal',), rows, R, 'noise', 'ortho'))
    for rows, R, cond in ILLCOND_SHAPES:
        out.append(_case('ortho-illcond', ('orthonormal',), rows, R, 'illcond%s' % cond, 'ortho'))
    assert len({c.id for c in out}) == len(out)
    return out


ILLCOND_SHAPES = ((40, 12, '1e3'), (40, 12, '1e5'), (40, 12, '1e6'), (40, 33, '1e6'))

# ||U V'(numpy SVD) - P||_F / ||P||_F with P the 40-digit polar factor (mpmath.svd_r) of the case's input, measured on
# the host and rounded up (test_prox_ref_host.py: measured <= floor <= 2 x measured).  The device bar of a case is
# max(1e-10, 10 x floor).
POLAR_FLOOR = {
    'orthonormal-illcond1e3-40x12': 1.9e-14,          # measured 1.32e-14
    'orthonormal-illcond1e5-40x12': 1.1e-12,          # measured 7.79e-13
    'orthonormal-illcond1e6-40x12': 1.8e-11,          # measured 1.27e-11
    'orthonormal-illcond1e6-40x33': 4.7e-12,          # measured 3.34e-12
}

CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
