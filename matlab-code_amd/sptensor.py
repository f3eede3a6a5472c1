"""A small Tensor Toolbox `sptensor` (cmtf_AOADMM.m:77-79, :132): coordinate storage of a sparse CP block.

    X = sptensor(subs, vals, shape)

`subs` is nnz x N with 0-based subscripts (MATLAB's `X.subs` minus 1), `vals` has nnz entries.  Duplicate
subscripts are summed on construction (sptensor's constructor rule) and the nonzeros are kept in column-major
linear order.  `build_model` uploads it through `aoadmm_tensor_upload_coo`; the values stay fp64 on the device.
"""
from __future__ import annotations

import numpy as np


class sptensor:
    def __init__(self, subs, vals, shape):
        shape = tuple(int(s) for s in shape)
        if len(shape) < 2:
            raise ValueError('sptensor: at least 2 modes, got shape %s' % (shape,))
        if any(s < 1 for s in shape):
            raise ValueError('sptensor: every size must be positive, got %s' % (shape,))
        subs = np.asarray(subs)
        vals = np.asarray(vals, dtype=np.float64).reshape(-1)
        if subs.size == 0:
            subs = np.zeros((0, len(shape)), dtype=np.int64)
        if subs.ndim != 2 or subs.shape[1] != len(shape):
            raise ValueError('sptensor: subs must be nnz x %d, got %s' % (len(shape), subs.shape))
        if subs.shape[0] != vals.shape[0]:
            raise ValueError('sptensor: %d subscripts but %d values' % (subs.shape[0], vals.shape[0]))
        if not np.issubdtype(subs.dtype, np.integer):
            if not np.all(np.asarray(subs) == np.floor(subs)):
                raise ValueError('sptensor: subscripts must be integers')
        subs = subs.astype(np.int64)
        if subs.size and (subs.min() < 0 or np.any(subs.max(axis=0) >= np.asarray(shape))):
            bad = np.argwhere((subs < 0) | (subs >= np.asarray(shape)[None, :]))[0]
            raise ValueError('sptensor: subscript %d of nonzero %d in mode %d is outside [0, %d)'
                             % (subs[bad[0], bad[1]], bad[0], bad[1], shape[bad[1]]))
        # column-major linear order; duplicates summed in the order given
        order = np.lexsort(subs.T) if subs.shape[0] else np.zeros(0, dtype=np.int64)
        subs, vals = subs[order], vals[order]
        if subs.shape[0]:
            new = np.ones(subs.shape[0], dtype=bool)
            new[1:] = np.any(subs[1:] != subs[:-1], axis=1)
            starts = np.flatnonzero(new)
            vals = np.add.reduceat(vals, starts)
            subs = subs[starts]
        self.subs = np.ascontiguousarray(subs)
        self.vals = np.ascontiguousarray(vals)
        self.shape = shape

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def nnz(self):
        return int(self.vals.shape[0])

    def full(self):
        """Dense numpy array (column-major), for tests and small blocks."""
        X = np.zeros(self.shape, order='F')
        if self.nnz:
            np.add.at(X, tuple(self.subs.T), self.vals)
        return X

    def norm(self):
        return float(np.sqrt(np.sum(self.vals * self.vals)))

    def split(self, frac, rng=None):
        """(train, heldout): two sptensors of this shape.  `heldout` gets round(frac * nnz) of the stored entries,
        drawn without replacement by `rng` (a numpy Generator or a seed), `train` the rest.  The cut is made after
        coalescing, so the parts are disjoint and their union is this tensor; the same rng state gives the same cut."""
        frac = float(frac)
        if not 0.0 <= frac <= 1.0:
            raise ValueError('sptensor.split: frac must lie in [0, 1], got %r' % (frac,))
        rng = np.random.default_rng(rng)
        k = int(round(frac * self.nnz))
        held = np.zeros(self.nnz, dtype=bool)
        held[rng.permutation(self.nnz)[:k]] = True
        return (sptensor(self.subs[~held], self.vals[~held], self.shape),
                sptensor(self.subs[held], self.vals[held], self.shape))

    def fiber_lists(self, mode, subs):
        """(off, idx) for `Engine.topk(..., exclude=...)`: query q (row q of `subs`, nq x N, 0-based, column `mode`
        ignored) names the fibre along `mode` through its other subscripts; idx[off[q]:off[q + 1]] are the indices
        along `mode` of the entries stored in that fibre, ascending.  An empty fibre gives an empty list."""
        mode = int(mode)
        if not 0 <= mode < self.ndim:
            raise ValueError('sptensor.fiber_lists: mode %d outside [0, %d)' % (mode, self.ndim))
        subs = np.asarray(subs, dtype=np.int64)
        if subs.ndim != 2 or subs.shape[1] != self.ndim:
            raise ValueError('sptensor.fiber_lists: subs must be nq x %d, got %s' % (self.ndim, subs.shape))
        others = [m for m in range(self.ndim) if m != mode]
        dims = np.asarray([self.shape[m] for m in others], dtype=np.int64)
        qs = subs[:, others]
        if qs.size and (qs.min() < 0 or np.any(qs >= dims[None, :])):
            raise ValueError('sptensor.fiber_lists: a query subscript is outside the tensor')
        if float(np.prod(dims.astype(np.float64))) >= 2.0 ** 63:
            raise ValueError('sptensor.fiber_lists: the fibres of mode %d have too many positions for 64-bit keys' % mode)

        def key(s):                                # linear position of the fibre among the other modes
            out = np.zeros(s.shape[0], dtype=np.int64)
            stride = 1
            for j in range(len(others)):
                out += s[:, j] * stride
                stride *= int(dims[j])
            return out

        fk = key(self.subs[:, others])
        order = np.lexsort((self.subs[:, mode], fk))
        fk, rows = fk[order], self.subs[order, mode]
        qk = key(qs)
        lo, hi = np.searchsorted(fk, qk, side='left'), np.searchsorted(fk, qk, side='right')
        off = np.zeros(subs.shape[0] + 1, dtype=np.int64)
        np.cumsum(hi - lo, out=off[1:])
        take = np.repeat(lo - off[:-1], hi - lo) + np.arange(off[-1], dtype=np.int64)
        return off, np.ascontiguousarray(rows[take].astype(np.int64))

    def take_rows(self, mode, rows, return_index=False):
        """(subs, vals) of the stored entries whose subscript along `mode` is in `rows` (distinct indices), in stored
        order, with column `mode` renumbered to the position in `rows`: the list `Engine.fold_in` takes for the queries
        rows[0], rows[1], ...  A row without stored entries contributes nothing.  return_index=True: (subs, vals, index)
        with index the positions of the taken entries in the stored list, so that an array kept beside `vals` (the entry
        weights of a fit) is cut the same way: `w[index]`."""
        mode = int(mode)
        if not 0 <= mode < self.ndim:
            raise ValueError('sptensor.take_rows: mode %d outside [0, %d)' % (mode, self.ndim))
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= self.shape[mode]):
            raise ValueError('sptensor.take_rows: a row is outside [0, %d)' % self.shape[mode])
        if len(np.unique(rows)) != len(rows):
            raise ValueError('sptensor.take_rows: rows must be distinct')
        pos = np.full(self.shape[mode], -1, dtype=np.int64)
        pos[rows] = np.arange(len(rows), dtype=np.int64)
        q = pos[self.subs[:, mode]]
        keep = q >= 0
        subs = self.subs[keep].copy()
        subs[:, mode] = q[keep]
        if return_index:
            return np.ascontiguousarray(subs), np.ascontiguousarray(self.vals[keep]), np.flatnonzero(keep).astype(np.int64)
        return np.ascontiguousarray(subs), np.ascontiguousarray(self.vals[keep])

    def __repr__(self):
        return 'sptensor(shape=%s, nnz=%d)' % (self.shape, self.nnz)


def coo_of(obj):
    """(subs int64 nnz x N, vals float64, shape) of an sptensor or of any object with .tocoo() (a scipy.sparse
    matrix); None for anything else."""
    if isinstance(obj, sptensor):
        return obj.subs, obj.vals, obj.shape
    if hasattr(obj, 'tocoo') and not isinstance(obj, np.ndarray):
        c = obj.tocoo()
        subs = np.stack([np.asarray(c.row, dtype=np.int64), np.asarray(c.col, dtype=np.int64)], axis=1)
        return subs, np.asarray(c.data, dtype=np.float64), tuple(int(s) for s in c.shape)
    return None


def pack_par2_slabs(slabs, I, Jk, p=0):
    """The sparse slabs of a PARAFAC2 block -> one COO list for `aoadmm_par2_slab_upload_coo`: subs nnz x 3, 0-based
    (i, j within the slab, k), vals.  Every slab is an sptensor or has .tocoo(); its shape must be I x Jk[k].
    Duplicates and explicit zeros are passed on as they are (the device sums duplicates)."""
    subs, vals = [], []
    for k, Xk in enumerate(slabs):
        c = coo_of(Xk)
        if c is None:
            raise ValueError('Z.object{%d}: slab %d is dense, the others sparse: all slabs must be sparse or all dense' % (p + 1, k + 1))
        sk, vk, shape = c
        if tuple(shape) != (int(I), int(Jk[k])):
            raise ValueError('Z.object{%d}{%d} has size %s, Z.size says %s' % (p + 1, k + 1, tuple(shape), [int(I), int(Jk[k])]))
        sk = np.asarray(sk, dtype=np.int64).reshape(-1, 2)
        subs.append(np.column_stack([sk, np.full(sk.shape[0], k, dtype=np.int64)]))
        vals.append(np.asarray(vk, dtype=np.float64).reshape(-1))
    if not subs:
        return np.zeros((0, 3), dtype=np.int64), np.zeros(0)
    return np.ascontiguousarray(np.vstack(subs)), np.concatenate(vals)


def slab_gram(obj, n):
    """Gram matrix of a sparse slab for init_options.nvecs = 1 without densifying it: X X' (n = 0) or X' X (n = 1)."""
    subs, vals, shape = coo_of(obj)
    return unfold_gram(subs, vals, shape, n)


def unfold_gram(subs, vals, shape, n):
    """Y = X_(n) X_(n)' of a sparse tensor (cmtf_nvecs.m:41-42, `double(sptenmat(X, n))`) without densifying the
    tensor: the unfolding is a scipy.sparse matrix (columns = linear index of the other modes, column-major)."""
    import scipy.sparse as sps            # only on this path
    subs = np.asarray(subs, dtype=np.int64)
    others = [m for m in range(len(shape)) if m != n]
    col = np.zeros(subs.shape[0], dtype=np.int64)
    stride = 1
    for m in others:
        col += subs[:, m] * stride
        stride *= int(shape[m])
    if stride >= 2 ** 63:
        raise ValueError('sptensor: the mode-%d unfolding has too many columns for 64-bit indices' % (n + 1))
    # column ids compressed to the ones that occur (same product A*A')
    ucol, cidx = np.unique(col, return_inverse=True)
    A = sps.csr_matrix((np.asarray(vals, dtype=np.float64), (subs[:, n], cidx)), shape=(int(shape[n]), max(len(ucol), 1)))
    return np.asfortranarray((A @ A.T).toarray())
