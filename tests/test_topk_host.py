"""CPU: the host layer of the top-k completions.  The header declares `aoadmm_resident_topk`, the
binding lists it and the library exports it; `Engine.topk` exists; `sptensor.fiber_lists` against a brute-force loop."""
import importlib
import os
import re

import numpy as np
import pytest

capi = importlib.import_module('matlab-code_amd._capi')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'aoadmm_resident_topk'


def test_entry_is_declared_bound_and_exported(pkg):
    with open(os.path.join(ROOT, 'include', 'aoadmm_hip.h')) as f:
        text = f.read()
    decl = re.search(r'^int %s\(([^;]*)\);' % ENTRY, text, flags=re.M | re.S)
    assert decl, 'the header does not declare %s' % ENTRY
    args = ' '.join(decl.group(1).split())
    assert args == ('aoadmm_ctx* ctx, int p, int mode, int64_t nq, const int64_t* subs, int k, const int64_t* excl_off, '
                    'const int64_t* excl_idx, int64_t* idx, double* val')
    assert ENTRY in pkg.SYMBOLS and ENTRY in capi.SYMBOLS
    assert re.search(r'int aoadmm_abi_version\(void\)', text)
    assert hasattr(pkg.load_library(), ENTRY)


def test_engine_has_topk(pkg):
    assert callable(getattr(pkg.Engine, 'topk', None))
    assert callable(getattr(pkg.sptensor, 'fiber_lists', None))


def brute_fiber_lists(X, mode, subs):
    off, idx = [0], []
    others = [m for m in range(X.ndim) if m != mode]
    for q in range(subs.shape[0]):
        rows = sorted(int(s[mode]) for s in X.subs if all(s[m] == subs[q, m] for m in others))
        idx.extend(rows)
        off.append(len(idx))
    return np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int64)


@pytest.mark.parametrize('shape', [(9, 7), (7, 6, 5), (5, 4, 3, 4)])
def test_fiber_lists_against_a_brute_force_loop(pkg, shape):
    rng = np.random.default_rng(len(shape))
    keep = rng.random(shape) < 0.3
    keep[(0,) * len(shape)] = True
    X = pkg.sptensor(np.argwhere(keep), rng.standard_normal(int(keep.sum())), shape)
    for mode in range(len(shape)):
        subs = np.stack([rng.integers(0, s, 40) for s in shape], axis=1).astype(np.int64)
        subs[5] = subs[3]                                      # a duplicate query
        subs[7] = subs[3]
        # a query whose fibre is empty: clear one fibre of the tensor
        others = [m for m in range(len(shape)) if m != mode]
        gone = subs[11]
        sel = np.all(X.subs[:, others] == gone[others][None, :], axis=1)
        Y = pkg.sptensor(X.subs[~sel], X.vals[~sel], shape)
        off, idx = Y.fiber_lists(mode, subs)
        roff, ridx = brute_fiber_lists(Y, mode, subs)
        assert off.dtype == np.int64 and idx.dtype == np.int64
        assert np.array_equal(off, roff) and np.array_equal(idx, ridx)
        assert off[12] == off[11]                              # the emptied fibre
        assert np.array_equal(idx[off[5]:off[6]], idx[off[3]:off[4]]) and np.array_equal(idx[off[7]:off[8]], idx[off[3]:off[4]])
        subs2 = subs.copy()
        subs2[:, mode] = -7                                    # the free mode's column is ignored
        off2, idx2 = Y.fiber_lists(mode, subs2)
        assert np.array_equal(off2, off) and np.array_equal(idx2, idx)


def test_fiber_lists_edges(pkg):
    X = pkg.sptensor(np.zeros((0, 3), dtype=np.int64), np.zeros(0), (4, 3, 2))
    off, idx = X.fiber_lists(0, np.array([[0, 1, 1], [0, 2, 0]]))
    assert np.array_equal(off, [0, 0, 0]) and idx.shape == (0,)
    off, idx = X.fiber_lists(2, np.zeros((0, 3), dtype=np.int64))
    assert np.array_equal(off, [0]) and idx.shape == (0,)
    for bad_mode in (-1, 3):
        with pytest.raises(ValueError):
            X.fiber_lists(bad_mode, np.zeros((1, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        X.fiber_lists(0, np.zeros((1, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        X.fiber_lists(0, np.array([[0, 3, 0]]))
