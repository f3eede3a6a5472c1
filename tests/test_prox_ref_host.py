"""CPU: the host side of the per-kernel-class prox tests (tests/prox_ref.py) is itself right.

  * every case of the table lands in the kernel class it names (prox_class, the pure-Python mirror of the dispatch);
  * the thresholds of that mirror equal the constants of csrc/prox.hip and csrc/iso.hip, read from the sources (the
    precedent is test_pass_loop_waits.py, which reads the compiled code): a retuned dispatch fails here with "pick a new
    shape" instead of silently moving a case of test_gpu_prox_classes.py to another kernel;
  * the banded GL solve equals the oracle's dense one;
  * the tie-tolerant unimodal comparison accepts a different split of a tied criterion and rejects a worse one;
  * POLAR_FLOOR, the bar of the ill-conditioned orthonormal cases, is the measured distance of numpy's SVD polar factor
    from a 40-digit one (mpmath) -- no device is involved in setting it.
"""
import os
import re

import numpy as np
import pytest

import prox_ref as PR
from helpers import rel_fro
from oracle import prox as OP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'matlab-code_amd', 'csrc')
RETUNED = 'the dispatch of %s was retuned: update prox_ref.py and pick a new shape for the cases at the old threshold'


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, head):
    """Text of the function whose definition starts with `head`, up to the closing brace in column 0."""
    at = src.index(head)
    return src[at:src.index('\n}\n', at)]


def _const(src, name):
    m = re.search(r'static constexpr int(?:64_t)? %s = (\d+);' % name, src)
    assert m, name
    return int(m.group(1))


@pytest.mark.parametrize('case', PR.CASES, ids=[c.id for c in PR.CASES])
def test_case_lands_in_the_class_it_names(case):
    assert PR.prox_class(case.c, case.rows, case.R) == case.cls, 'pick a new shape for %s' % case.id


def test_both_sides_of_every_threshold_have_a_case():
    seen = {c.cls for c in PR.CASES}
    want = ({'rows<8>', 'rows<16>', 'rows<32>', 'rows<64>', 'colnorm', 'simplexcol', 'ortho'} |
            {'tv-256thr-x1', 'tv-256thr-x2', 'tv-256thr-x4', 'tv-1024thr-x2', 'tv-1024thr-x4', 'tv-1024thr-hybrid',
             'tv-1024thr-workspace'} |
            {'iso-prevself-iso256', 'iso-prevself-isolds', 'iso-prevglobal-isoglobal-shares64',
             'iso-prevlds-isolds-shares64', 'iso-prevlds-isolds-shares8', 'iso-prevlds-isolds-shares4',
             'iso-prevlds-isoglobal-shares64', 'iso-prevglobal-isoglobal-shares51', 'iso-prevglobal-isoglobal-shares25',
             'iso-prevglobal-isoglobal-shares12'} |
            {'gl-256thr-x1', 'gl-1024thr-x1', 'gl-1024thr-x4'})
    assert seen == want, seen ^ want
    edges = {'rows': [(c, 129, R) for c in [('ridge', 0.3)] for R in (8, 9, 16, 17, 32, 33)],
             'tv': [(('TV regularization', 0.4), rows, 2) for rows in (256, 257, 512, 513, 1024, 1025, 2048, 2049, 12000, 12001)],
             'iso': [(('non-decreasing',), rows, 3) for rows in (256, 257, 512, 513, 2048, 2049, 6000, 6001)],
             'gl': [(('GL smoothness', 0.7), rows, 3) for rows in (256, 257, 1024, 1025)]}
    have = {(c.c[0], c.rows, c.R) for c in PR.CASES}
    for fam, lst in edges.items():
        for lo, hi in zip(lst[::2], lst[1::2]):
            assert (lo[0][0],) + lo[1:] in have and (hi[0][0],) + hi[1:] in have
            assert PR.prox_class(*lo) != PR.prox_class(*hi), (fam, lo, hi)


def test_mirror_thresholds_equal_the_source_constants():
    prox, iso = _src('prox.hip'), _src('iso.hip')
    # prox_rows_k<8|16|32|64>
    apply_ = _body(prox, 'void prox_apply(')
    steps = re.findall(r'if \(R <= (\d+)\) prox_rows_k<(\d+)><<<', apply_)
    assert [tuple(map(int, s)) for s in steps] == [(s, s) for s in PR.ROWS_STEPS], RETUNED % 'prox_rows_k'
    assert 'else prox_rows_k<64><<<' in apply_, RETUNED % 'prox_rows_k'
    for fam, kern in (('colnorm', 'prox_colnorm_k'), ('simplexcol', 'prox_simplex_col_k')):
        assert '%s<<<R, 256, 0, s>>>' % kern in apply_, RETUNED % kern
    # TV: LDS / hybrid / workspace, 256 / 1024 threads, 1 / 2 / 4 / 8 entries staged per thread
    assert _const(prox, 'kTvParMax') == PR.TV_PAR_MAX, RETUNED % 'prox_tv_fast_k'
    assert _const(prox, 'kTvHybridMax') == PR.TV_HYBRID_MAX, RETUNED % 'prox_tv_fast_k'
    launch = _body(prox, 'static void tv_fast_launch(')
    assert re.search(r'if \(a\.rows > kTvParMax\) \{', launch) and re.search(r'if \(a\.rows <= kTvHybridMax\) \{', launch)
    m = re.search(r'\} else if \(a\.rows > (\d+)\) \{\s*ensure_dynamic_lds\([^;]*prox_tv_fast_k<1024>', launch)
    assert m and int(m.group(1)) == PR.TV_SHORT_ROWS, RETUNED % 'tv_fast_launch'
    assert 'prox_tv_fast_k<256><<<a.R, 256,' in launch and 'prox_tv_fast_k<1024><<<a.R, 1024,' in launch
    kern = _body(prox, '__global__ __launch_bounds__(kTvThreads) void prox_tv_fast_k(')
    for phase in ('stage', 'dual'):
        got = re.findall(r'if \(n <= (?:(\d+) \* )?kTvThreads\) %s\(std::integral_constant<int, (\d+)>\(\)\);' % phase, kern)
        assert [(int(a or 1), int(b)) for a, b in got] == [(k, k) for k in PR.TV_STAGE_STEPS], RETUNED % 'prox_tv_fast_k'
        assert 'else %s(std::integral_constant<int, 8>());' % phase in kern, RETUNED % 'prox_tv_fast_k'
    # the 8x-threads rule: the largest LDS-resident column fits eight entries per thread
    assert PR.TV_PAR_MAX <= 8 * 1024 and PR.TV_SHORT_ROWS <= 8 * 256
    # isotonic / unimodal
    assert _const(iso, 'kIsoOneKernelRows') == PR.ISO_ONE_KERNEL_ROWS, RETUNED % 'prox_iso'
    assert _const(iso, 'kIsoLdsRows') == PR.ISO_LDS_ROWS, RETUNED % 'prox_iso'
    assert _const(iso, 'kIsoPrevLdsRows') == PR.ISO_PREV_LDS_ROWS, RETUNED % 'prox_iso'
    piso = _body(iso, 'void prox_iso(')
    assert re.search(r'if \(rows <= %d\) \{\s*prox_iso_k<256, true><<<' % PR.ISO_SMALL_ROWS, piso), RETUNED % 'prox_iso'
    assert re.search(r'\} else if \(rows <= kIsoLdsRows\) \{', piso) and 'if (rows > kIsoOneKernelRows) {' in piso
    assert 'if (rows <= kIsoPrevLdsRows) {' in piso and 'const int shares = iso_shares(R, ndir);' in piso
    sh = _body(iso, 'static int iso_shares(')
    m = re.search(r'int shares = (\d+) / \(R \* ndir\);\s*return shares < 1 \? 1 : \(shares > (\d+) \? (\d+) : shares\);', sh)
    assert m and tuple(map(int, m.groups())) == (PR.ISO_SHARE_BUDGET, PR.ISO_SHARE_MAX, PR.ISO_SHARE_MAX), RETUNED % 'iso_shares'
    for R, ndir, want in ((3, 1, 64), (64, 1, 8), (64, 2, 4), (20, 1, 25), (20, 2, 12), (5, 2, 51), (64, 16, 1)):
        assert PR.iso_shares(R, ndir) == want
    # GL smoothness
    gl = _body(iso, 'bool prox_gl_pcr(')
    assert re.search(r'if \(rows > %d\) \{' % PR.GL_STEPS[2], gl), RETUNED % 'prox_gl_pcr'
    assert re.search(r'if \(rows <= %d\) \{\s*prox_gl_pcr_k<256, 1><<<' % PR.GL_STEPS[0], gl), RETUNED % 'prox_gl_pcr'
    assert re.search(r'\} else if \(rows <= %d\) \{\s*prox_gl_pcr_k<1024, 1><<<' % PR.GL_STEPS[1], gl), RETUNED % 'prox_gl_pcr'
    assert 'prox_gl_pcr_k<1024, 4><<<' in gl, RETUNED % 'prox_gl_pcr'


@pytest.mark.parametrize('rows', [1, 2, 3, 257, 1001])
@pytest.mark.parametrize('eta', [1e-3, 0.7, 40.0])
def test_banded_gl_solve_is_the_oracle_prox(rows, eta):
    x = np.random.default_rng(rows).standard_normal((rows, 4))
    dense = OP.constraints_to_prox([1], [('GL smoothness', eta)], [rows])[0][0](x, PR.RHO)
    assert rel_fro(PR.gl_banded(x, PR.RHO, eta), dense) < 1e-13


def test_inputs_are_reproducible_and_differ_between_columns():
    for case in PR.CASES:
        if case.rows * case.R > 20000:
            continue
        X = PR.make_input(case)
        assert X.shape == (case.rows, case.R) and X.dtype == np.float64
        assert np.array_equal(X, PR.make_input(case))
        if case.rows >= 40 and case.R > 1:
            assert len({X[:, r].tobytes() for r in range(case.R)}) == case.R, case.id
    onb = PR.BY_ID['l1-ball-%g-on-boundary-257x3' % PR.boundary_eta(257)]
    assert np.all(np.abs(PR.make_input(onb)).sum(axis=0) == onb.c[1])
    tie = PR.make_input(next(c for c in PR.CASES if c.kind == 'sphere-tie'))
    for r, (i, j) in enumerate(PR.SPHERE_TIES):
        assert tie[i, r] == tie[j, r] == tie[:, r].max() <= 0.0 and np.argmax(tie[:, r]) == i


def test_tied_unimodal_split_comparison():
    """[2, 0, 2]: rising to the last entry ([1, 1, 2]) and falling from the first ([2, 1, 1]) are both projections, at
    distance 2.  The comparison accepts either against the other and rejects an infeasible or a farther point."""
    X = np.array([[2.0], [0.0], [2.0]])
    ref = OP.project_unimodal(X, False)
    a, b = np.array([[1.0], [1.0], [2.0]]), np.array([[2.0], [1.0], [1.0]])
    assert np.array_equal(ref, a) or np.array_equal(ref, b)
    for g in (a, b):
        PR.unimodal_tied_check(g, ref, X, False)
    with pytest.raises(AssertionError):
        PR.unimodal_tied_check(X, ref, X, False)                        # not unimodal
    with pytest.raises(AssertionError):
        PR.unimodal_tied_check(np.full((3, 1), 4.0 / 3.0), ref, X, False)   # feasible, but farther (8/3 > 2)
    with pytest.raises(AssertionError):
        PR.unimodal_tied_check(-a, OP.project_unimodal(-X, True), -X, True)  # negative under non-negativity


def mp_polar(X, digits=40):
    import mpmath
    with mpmath.workdps(digits):
        U, _, V = mpmath.svd_r(mpmath.matrix(X.tolist()), full_matrices=False)
        P = U * V
        return np.array([[float(P[i, j]) for j in range(P.cols)] for i in range(P.rows)])


def measured_polar_floor(case):
    X = PR.make_input(case)
    P = mp_polar(X)
    return rel_fro(OP.project_ortho(X), P)


@pytest.mark.parametrize('case', [c for c in PR.CASES if c.family == 'ortho-illcond'], ids=lambda c: c.id)
def test_polar_floor_is_the_measured_svd_error(case):
    pytest.importorskip('mpmath')
    X = PR.make_input(case)
    s = np.linalg.svd(X, compute_uv=False)
    assert abs(s[0] / s[-1] / float(case.kind[len('illcond'):]) - 1.0) < 1e-6
    floor = measured_polar_floor(case)
    print('%s: numpy SVD polar factor against 40 digits: %.3e (POLAR_FLOOR %.3e)' % (case.id, floor, PR.POLAR_FLOOR[case.id]))
    assert floor <= PR.POLAR_FLOOR[case.id] <= 2.0 * floor
