"""GPU: every kernel class of the stand-alone proximal operator catalogue (csrc/prox.hip, csrc/iso.hip and the
sym_eig_small / atb_small / gemm_small pieces of the orthonormal prox), through `eng.prox` (aoadmm_op_prox), against
oracle.prox in fp64 at the shapes where the dispatch changes kernel and on the degenerate inputs of each kernel.

Inputs, references, the dispatch mirror and the case table live in tests/prox_ref.py; test_prox_ref_host.py checks on
the CPU that every case lands in the class it names and that the mirror's thresholds are the sources' constants.

Bar (all but the ill-conditioned orthonormal cases): that of test_prox_matches_oracle, relative Frobenius < 1e-10 or
max abs < 1e-12 -- these are exact algorithms that differ from the oracle in summation order only.  Unimodal projections
of integer data whose split is tied: feasibility plus equal distance (prox_ref.unimodal_tied_check).  Ill-conditioned
orthonormal cases: max(1e-10, 10 x POLAR_FLOOR) against numpy's SVD, POLAR_FLOOR being numpy's own distance from a
40-digit polar factor (10 for a different but equally stable algorithm, as in test_gpu_admm.py), and
||Q'Q - I||_F < 1e-10.  No bar comes from the device.

Class -> case (rows x R; ids as pytest prints them: <constraint>-<parameters>-<kind>-<rows>x<R>):
  prox_rows_k<8>       129x8                        non-negativity, box, l1 / l0 regularization (half the entries on each
  prox_rows_k<16>      129x9, 129x16                side of the threshold), ridge, simplex row-wise on noise; simplex
  prox_rows_k<32>      129x17, 129x32               row-wise also on ties (small integers) and feasible rows
  prox_rows_k<64>      129x33, 129x64, 1x64         (simplex_regs<64> included)
  prox_colnorm_k       255x3, 256x3, 257x3, 257x64  l2-ball, non-negative l2-ball, non-negative l2-sphere, l2
                                                    regularization on noise / zero-col / feasible / allneg;
                       260x3 sphere-tie             maxima tied at rows (3, 259), (5, 200), (2, 258): one-hot at the first
  prox_simplex_col_k   255x3, 256x3, 257x3, 257x64  simplex column-wise and l1-ball on noise / ties / feasible /
                                                    one-dominant / on-boundary (integers, ||x||_1 == eta: the input bit
                                                    for bit) and with eta = 1e3 (every entry active)
  prox_tv_fast_k<256>  x1: 2, 3, 256   x2: 257, 512   x4: 513, 1024, 1000x64                  (x2 columns; noise / steps /
  prox_tv_fast_k<1024> x2: 1025, 2048  x4: 2049, 4096  hybrid: 12000  workspace: 12001          ties; constant at 513)
                       (x8, 4097-6400, and the 6400 / 6401 edge: test_tv_prox_long_columns)
  prox_iso_k<256,lds>      no iso_prev_k   255x3, 256x3               non-decreasing, non-increasing, unimodality with and
  prox_iso_k<1024,lds>     no iso_prev_k   257x3, 512x3               without non-negativity, on noise and ties; constant
                           iso_prev_k lds  513x3, 2048x3 (64 shares), 513x64 (8 shares, unimodal 4)           at 257x3
  prox_iso_k<1024,global>  iso_prev_k lds  2049x3, 6000x3 (64 shares)
                           iso_prev_k global   6001x3 (64), 6001x5 (64, unimodal 51), 6001x20 (25, unimodal 12): several
                                               columns, directions and shares in the global prefix-sum form
  prox_gl_pcr_k<256,1>     2x3 (both rows are end rows), 3x3, 256x3   eta 1e-3, 0.7, 40
  prox_gl_pcr_k<1024,1>    257x3, 1024x3, 257x64
  prox_gl_pcr_k<1024,4>    1025x3, 4096x3                             (4097 and beyond: test_gl_prox_long_columns)
  prox_ortho               (R, R), (R + 1, R), (129, R) for R 1, 2, 33, 64 on Gaussian matrices: 1e-10 and
                           ||Q'Q - I||_F < 1e-12;  40x12 at cond 1e3, 1e5, 1e6 and 40x33 at cond 1e6 (U diag(logspace) V')

Measured on an MI355X (largest error per family; relative Frobenius unless stated): see LARGEST_SEEN below.
"""
import numpy as np
import pytest

import prox_ref as PR
from helpers import rel_fro

pytestmark = pytest.mark.gpu

# family -> largest relative Frobenius error seen on an MI355X over the family's cases (a record, not a bar)
LARGEST_SEEN = {
    'rows': 8.3e-16, 'colnorm': 3.6e-16, 'simplexcol': 9.5e-16, 'tv': 8.1e-15, 'gl': 2.8e-15,
    'iso': 3.8e-15,                        # one case (unimodality-ties-513x64) took another split of a tied criterion
    'ortho': 5.7e-15,                      # ||Q'Q - I||_F at most 8.1e-14 (129x64)
    # ill-conditioned, cond 1e3 / 1e5 / 1e6 at 40x12 and 1e6 at 40x33 (||Q'Q - I||_F at most 3.6e-14):
    'ortho-illcond': (1.6e-14, 9.3e-13, 1.4e-11, 4.0e-12),
    # the same four under the norm-wise stopping rule sym_eig_small_k had for every caller before this test existed
    # (||Q'Q - I||_F 2.4e-11, 1.8e-8, 1.7e-5, 3.9e-10): three of the four failed
    'ortho-illcond, norm-wise rule': (3.7e-12, 3.1e-9, 3.1e-6, 3.9e-11),
}


def _cases(*families):
    return [pytest.param(c, id=c.id) for c in PR.CASES if c.family in families]


def _run(eng, case):
    X = PR.make_input(case)
    ref = PR.reference(case.c, X)
    got = eng.prox(case.c, X, PR.RHO)
    err, mx = rel_fro(got, ref), float(np.max(np.abs(got - ref)))
    print('%s [%s]: rel fro %.3e, max abs %.3e' % (case.id, case.cls, err, mx))
    return X, ref, got, err, mx


@pytest.mark.parametrize('case', _cases('rows', 'colnorm', 'simplexcol', 'tv', 'gl'))
def test_prox_class_matches_oracle(eng, case):
    X, ref, got, err, mx = _run(eng, case)
    assert err < 1e-10 or mx < 1e-12, err
    if case.kind == 'on-boundary':                      # ||x||_1 == eta exactly: the projection is the input
        assert np.array_equal(got, X)
    if case.kind == 'sphere-tie':
        for r, (i, _) in enumerate(PR.SPHERE_TIES):
            want = np.zeros(case.rows)
            want[i] = 1.0
            assert np.array_equal(got[:, r], want), (r, int(np.argmax(got[:, r])))
    if case.kind == 'feasible' and case.c[0] == 'l1-ball':
        assert np.array_equal(got, X)                   # strictly inside the ball: copied


@pytest.mark.parametrize('case', _cases('iso'))
def test_isotonic_class_matches_oracle(eng, case):
    X, ref, got, err, mx = _run(eng, case)
    if case.kind == 'ties' and case.c[0] == 'unimodality' and not (err < 1e-10):
        PR.unimodal_tied_check(got, ref, X, case.c[1])
        return
    assert err < 1e-10 or mx < 1e-12, err


@pytest.mark.parametrize('case', _cases('ortho'))
def test_orthonormal_well_conditioned(eng, case):
    _, _, got, err, _ = _run(eng, case)
    orth = float(np.linalg.norm(got.T @ got - np.eye(case.R)))
    print('%s: ||Q\'Q - I||_F %.3e' % (case.id, orth))
    assert err < 1e-10, err
    assert orth < 1e-12, orth


@pytest.mark.parametrize('case', _cases('ortho-illcond'))
def test_orthonormal_ill_conditioned(eng, case):
    _, _, got, err, _ = _run(eng, case)
    orth = float(np.linalg.norm(got.T @ got - np.eye(case.R)))
    bar = max(1e-10, 10.0 * PR.POLAR_FLOOR[case.id])
    print('%s: ||Q\'Q - I||_F %.3e, bar %.1e' % (case.id, orth, bar))
    assert err < bar, (err, bar)
    assert orth < 1e-10, orth
