"""GPU: every kernel class a dense PARAFAC2 block runs outside the B_k loop (cmtf_fun_AOADMM.m:160-178 mode A, :219-248
mode C with ADMM_constrained_only :600-606, :260-312 the coupled C systems, :1262-1264 / :1355 / :1337 / :1279-1281 the
objective pieces; csrc/par2.hip, admm_loop_wg_k<RM, 256, 2> of csrc/admm.hip), run as the solver runs them
(`Engine.par2_mode_a` / `par2_mode_c` / `par2_objective` -> aoadmm_op_par2_* -> par2_mode_a, par2_c_systems,
par2_c_solve, par2_c_coupled_big, par2_objective: the functions the engine calls), against tests/par2_modes_ref.py.

Every case asserts its path against LITERALS of the case table (a moved threshold turns the case red: pick a new shape),
the iteration count, and every returned array.

Data (`make_block`): A with orthogonal columns of norm 0.8..1.25, B_k = s_k Q_k DeltaB with Q_k orthonormal (Gaussian where
J_k < R) and DeltaB with singular values in [0.7, 1.6], C in [0.5, 1.5], X_k = A D_k B_k' + 5 % noise.  s_k^2 is spread over
12 x, so rho_k = trace(A'A .* B_k'B_k) / R spread over 12 x; the largest sits at `peak` (never the last row unless the case
says so).  Exact cases: small integers with asymmetric factors, compared with array_equal.

Bars.  Arrays (T1-free quantities: C, Z, mu, a, rho, L, M, Amt, Csys against the reference): each case's floor is the
largest relative Frobenius distance between two host evaluations (fp64 restatement / longdouble sums; Cholesky solve /
explicit inverse), the bar is max(1e-11, 10 x floor), never taken from the device.  Largest floor over the cases of this
file: LARGEST_FLOOR below; every case must stay below MAX_FLOOR (tests/test_par2_modes_host.py checks that on the CPU).
Sums in fixed order, bounds stated beside each assertion, eps = 2^-52, first order:
  T1, GB        four partial sums of J_k / 4 products: (J_k / 4 + 3) eps sum |terms|           (the GB bound of the B-loop file)
  Amt, Csys     256 / ew slab groups add ceil(K / ng) terms in order, then log2(ng) tree levels; the products cost 1 (2)
                roundings: (ceil(K / ng) + log2(ng) + 2 (3)) eps sum |terms|, against the longdouble sum of the DEVICE's
                T1 and GB
  a             I terms in order on T1: (I + J_k / 4 + 5) eps w sum_i |A| (|X_k| |B_k|)
  res           256 threads add ceil(n / 256) squares in order, 8 tree levels, the model entry is a sum of R products:
                (ceil(n / 256) + 11) eps res + 2 (R + 2) eps sum |x - m| sum_r |a c b|
  q             64 threads, ceil(J_k R / 64) terms, 6 tree levels: (ceil(n / 64) + 9) eps q (+ the R-term product P_k DeltaB
                for q0, as for res)
  regv          (ceil(n / 64) + 9) eps eta sum |terms|; l2: per column (ceil(J_k / 64) + 8) eps / 2 + 1 for the root,
                R columns in order: (ceil(J_k / 64) / 2 + R + 6) eps value
Residuals of the loops: ratios ||x - y|| / ||z|| with an error of bar on each, bound bar x (scale + residual) as in the
B-loop file.

Class -> case (ids as pytest prints them):
  par2_modeA_combine_k ew 4              A-ew4-I37-R3 (nA % 4 = 3), A-ew4-below2048, A-K{1,63,64,65,300} (64 slab groups)
  par2_modeA_combine_k ew 16             A-ew16-at2048, A-ew16-ragged (nA % 16 = 13), A-ew16-below16384
  par2_modeA_combine_k ew 64             A-ew64-at16384, A-ew64-ragged (nA % 64 = 55), A-ew64-K3, A-ew64-K5 (4 slab groups);
                                         Csys-only launch at ew 16: the three ew64 cases (R*R >= 2048)
  par2_xkb_k / par2_gram_k remainders    A-remJ (J_k = 1, R, and J_k % 4 = 0..3), A-remI{1..7}
  par2_c_rowsolve_k<4|8|16|64>, single   C1-R{1,4|5,8|9,16|17,64}; more than one workgroup: C1-K{1,64,65,300}
  admm_loop_wg_k<4|8|16, 256, 2>         Cwg-R{1,3,4|5,8|9,16}, Cwg-K{1,63,64,65,255,256}; max(rho) butterfly over padding
                                         threads: Cwg-peak-{first,lastwave,lastrow}; prox: Cwg-{nonneg,box,l1,l0,ridge,
                                         simplex,l2ball,nnl2ball,l2reg,nnsphere}, Cwg-nnsphere-zerocol; Cwg-*|inner{1,6}
  launched loop (use_admm = 1)           Cl-K257-R3, Cl-ridge-K257 (five workgroups), Cl-R17-K5 (<64>), Cl-nondecr-K40, Cl-tv-K40;
                                         CTL_GUARD under a closed ctl: exit-{pr,du} on Cl-ridge-K257 (and on Cwg-ridge)
  terms, refusals                        C-ridge-bsum-{single,wg}, zero slab of B (not PD), test_refusals (multi-device context,
                                         communicator)
  par2_c_system_k nrho / Madd / raw,
  par2_c_rowsys_diag_k, par2_c_big_system_k   Csys{1,2,3,4}-R{3,9,17}-con{0,1} (K = 6; K R = 102 at R = 17)
  par2_residual_k four-at-a-time loop    O-n{200,1023,1024,1025,5000}; ranks O-R1, O-R64; prev term: equal and unequal
                                         neighbours and J_k = 1 in every case; O-noZ; par2_reg_k: O-reg-{l1,l0,l2,ridge,gl,tv}
  exact (array_equal)                    test_mode_a_exact_small_integers (ew 4, 16, 64), test_mode_c_dense_system_exact_small_integers,
                                         test_objective_exact_small_integers
"""
import functools
import math
import zlib

import numpy as np
import pytest

import par2_modes_ref as REF

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble

# Largest distance between the two host evaluations over every case of this file (host only, no device involved):
# 7.2e-15 (Cl-tv-K40).  Every case is required to stay below MAX_FLOOR, so every case runs at the 1e-11 bar.
LARGEST_FLOOR = 7.2e-15
MAX_FLOOR = 1e-12

SINGLE, WG, LAUNCHED = 0, 1, 2                  # AOADMM_P2C_* (include/aoadmm_hip.h)
WEIGHT = 0.7
EXIT_INNER = 10
INF = float('inf')

NONNEG = ('non-negativity',)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _params(cases):
    return [pytest.param(c, id=c['id']) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_block(cid, I, R, J, peak=None, noise=0.05):
    """A dense block with a known truth (see the module docstring).  Arrays are read-only."""
    rng = np.random.default_rng(zlib.crc32(cid.split('|')[0].encode()))
    K = len(J)
    if I >= R:
        A = np.linalg.qr(rng.standard_normal((I, R)))[0] * (np.linspace(0.8, 1.25, R) if R > 1 else 1.1)
    else:
        A = rng.standard_normal((I, R))
    U, _ = np.linalg.qr(rng.standard_normal((R, R)))
    V, _ = np.linalg.qr(rng.standard_normal((R, R)))
    DeltaB = (U * (np.linspace(0.7, 1.6, R) if R > 1 else np.array([1.1]))) @ V.T
    # s_k^2 over 10 x, shuffled, the largest at `peak`
    u = rng.permutation(np.linspace(0.0, 1.0, K)) if K > 1 else np.array([0.5])
    peak = (K // 3) if peak is None else peak
    at = int(np.argmax(u))
    u[at], u[peak] = u[peak], u[at]
    if K > 1:
        u[peak] += 0.1                                # the largest rho_k stands 26 % clear of the next
    s = 10.0 ** (0.5 * u)
    Cm = rng.random((K, R)) + 0.5
    X, B, P, Zb = [], [], [], []
    for k, j in enumerate(J):
        Q = np.linalg.qr(rng.standard_normal((j, R)))[0] if j >= R else rng.standard_normal((j, R)) / np.sqrt(j)
        Bk = s[k] * Q @ DeltaB
        M = A @ np.diag(Cm[k]) @ Bk.T
        N = rng.standard_normal(M.shape)
        X.append(M + noise * np.linalg.norm(M) / np.linalg.norm(N) * N)
        B.append(Bk)
        P.append(s[k] * (Q + 0.1 / np.sqrt(j) * rng.standard_normal((j, R))))
        Zb.append(Bk + 0.05 * s[k] * rng.standard_normal((j, R)) / np.sqrt(j))
    blk = dict(I=I, R=R, J=tuple(J), K=K, peak=peak, X=X, A=A, B=B, C=Cm, P=P, DeltaB=DeltaB, Zb=Zb,
               Zc=Cm + 0.05 * rng.standard_normal((K, R)), muc=0.05 * rng.standard_normal((K, R)))
    for v in blk.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return blk


def seq_tree(nseq, levels, extra):
    """First-order rounding count of `nseq` terms added in order, `levels` pairwise levels and `extra` roundings per term."""
    return (nseq + levels + extra) * EPS


# ---------------------------------------------------------------------------------------------------------------------
# mode A
# ---------------------------------------------------------------------------------------------------------------------
def acase(cid, I, R, J, ew):
    return dict(id=cid, I=I, R=R, J=tuple(J), ew=ew)


def _cyc(K, lo, n):
    return [lo + (5 * k) % n for k in range(K)]


A_CASES = [
    # (tile width of the Amt + Csys launch over I R + R R outputs, of the Csys-only launch over R R)
    acase('A-ew4-I37-R3', 37, 3, [5, 6, 7], (4, 4)),                       # 120 outputs, nA % 4 = 3
    acase('A-ew4-below2048', 66, 23, [5, 6, 7], (4, 4)),                   # 2047
    acase('A-ew16-at2048', 32, 32, [5, 6, 7], (16, 4)),                    # 2048
    acase('A-ew16-ragged', 67, 31, [5, 6, 7], (16, 4)),                    # 3038, nA % 16 = 13
    acase('A-ew16-below16384', 338, 43, [5, 6, 7], (16, 4)),               # 16383
    acase('A-ew64-at16384', 192, 64, [5, 6, 7], (64, 16)),                 # 16384; R R = 4096 >= 2048
    acase('A-ew64-ragged', 259, 61, [5, 6, 7], (64, 16)),                  # 19520, nA % 64 = 55
    acase('A-ew64-K3', 259, 61, [4, 5, 6], (64, 16)),                      # 4 slab groups: one idle
    acase('A-ew64-K5', 259, 61, [4, 5, 6, 7, 4], (64, 16)),                # 4 slab groups: one takes two slabs
] + [acase('A-K%d' % K, 37, 3, _cyc(K, 3, 4), (4, 4)) for K in (1, 63, 64, 65, 300)] + [
    acase('A-remJ', 37, 3, [1, 3, 4, 5, 6, 7, 8], (4, 4)),                 # J_k = 1, J_k = R, J_k % 4 = 0, 1, 2, 3
] + [acase('A-remI%d' % I, I, 3, [4, 5, 7], (4, 4)) for I in (1, 2, 3, 4, 5, 6, 7)]


@functools.lru_cache(maxsize=None)
def a_reference(cid, I, R, J):
    blk = make_block(cid, I, R, J)
    ref = REF.mode_a(blk['X'], blk['B'], blk['C'])
    alt = REF.mode_a(blk['X'], blk['B'], blk['C'], ld=True)
    floor = max(rel(alt[k], ref[k]) for k in ('T1', 'GB', 'Amt', 'Csys'))
    return blk, ref, alt, floor


def a_floor(c):
    return a_reference(c['id'], c['I'], c['R'], c['J'])[3]


@pytest.mark.parametrize('c', _params(A_CASES))
def test_mode_a(eng, c):
    blk, ref, alt, floor = a_reference(c['id'], c['I'], c['R'], c['J'])
    assert floor < MAX_FLOOR
    bar = max(1e-11, 10 * floor)
    out = eng.par2_mode_a(blk['X'], blk['B'], blk['C'])
    K, I, R, Cm = blk['K'], blk['I'], blk['R'], blk['C']
    print('%s I %d R %d K %d: path %s floor %.2e Amt %.2e Csys %.2e Csys_only %.2e'
          % (c['id'], I, R, K, out['path'], floor, rel(out['Amt'], ref['Amt']), rel(out['Csys'], ref['Csys']),
             rel(out['Csys_only'], ref['Csys'])))
    assert out['path'] == c['ew'], 'tile widths %s here, the case is meant for %s: pick a new shape' % (out['path'], c['ew'])
    for k, j in enumerate(blk['J']):
        # four partial sums of J_k / 4 products: (J_k / 4 + 3) eps sum |terms|
        assert (np.abs(out['T1'][k] - alt['T1'][k]) <= (j / 4 + 3) * EPS * (np.abs(blk['X'][k]) @ np.abs(blk['B'][k]))).all(), k
        assert (np.abs(out['GB'][k] - alt['GB'][k]) <= (j / 4 + 3) * EPS * (np.abs(blk['B'][k]).T @ np.abs(blk['B'][k]))).all(), k
    # ksum_tile on the device's own T1 / GB: ceil(K / ng) terms in order per group, log2(ng) tree levels, 1 (2) products
    dev = REF.mode_a_sums(list(out['T1']), list(out['GB']), Cm, ld=True)
    absA = sum(np.abs(out['T1'][k]) * np.abs(Cm[k])[None, :] for k in range(K))
    absC = sum(np.abs(Cm[k])[:, None] * np.abs(out['GB'][k]) * np.abs(Cm[k])[None, :] for k in range(K))
    for name, ew, tot, extra in (('Amt', c['ew'][0], absA, 2), ('Csys', c['ew'][0], absC, 3), ('Csys_only', c['ew'][1], absC, 3)):
        ng = 256 // ew
        bound = seq_tree(math.ceil(K / ng), int(math.log2(ng)), extra) * tot
        want = dev['Amt' if name == 'Amt' else 'Csys'].astype(np.float64)
        assert (np.abs(out[name] - want) <= bound).all(), (name, float(np.max(np.abs(out[name] - want) / bound)))
    assert rel(out['Amt'], ref['Amt']) < bar and rel(out['Csys'], ref['Csys']) < bar and rel(out['Csys_only'], ref['Csys']) < bar


def test_mode_a_exact_small_integers(eng):
    """Integer slabs, B_k and C without any symmetry: T1, GB, Amt, Csys are sums of small integers, exact in any order.  A
    swapped i / r, r / q or slab index changes them at the first digit."""
    rng = np.random.default_rng(11)
    I, R, J = 37, 3, [5, 6, 7, 4, 9]
    X = [rng.integers(-3, 4, size=(I, j)).astype(np.float64) for j in J]
    B = [rng.integers(-3, 4, size=(j, R)).astype(np.float64) for j in J]
    Cm = rng.integers(1, 5, size=(len(J), R)).astype(np.float64)
    ref = REF.mode_a(X, B, Cm)
    out = eng.par2_mode_a(X, B, Cm)
    assert out['path'] == (4, 4)
    for name in ('T1', 'GB', 'Amt', 'Csys'):
        assert np.array_equal(out[name], ref[name]), name
    assert np.array_equal(out['Csys_only'], ref['Csys'])
    # ew 16 and 64: the same with the Csys half behind a ragged A half
    for I, R, ew in ((67, 31, (16, 4)), (259, 61, (64, 16))):
        X = [rng.integers(-2, 3, size=(I, j)).astype(np.float64) for j in J]
        B = [rng.integers(-2, 3, size=(j, R)).astype(np.float64) for j in J]
        Cm = rng.integers(1, 4, size=(len(J), R)).astype(np.float64)
        ref = REF.mode_a(X, B, Cm)
        out = eng.par2_mode_a(X, B, Cm)
        assert out['path'] == ew
        for name in ('T1', 'GB', 'Amt', 'Csys'):
            assert np.array_equal(out[name], ref[name]), (I, R, name)
        assert np.array_equal(out['Csys_only'], ref['Csys'])


# ---------------------------------------------------------------------------------------------------------------------
# mode C, uncoupled
# ---------------------------------------------------------------------------------------------------------------------
def ccase(cid, R, K, path, con=None, inner=5, peak=None, ridge=0.0, bsum_half=0.0, special=None):
    I = max(R, 6) + 1
    J = tuple(R + 1 + (3 * k) % 4 for k in range(K))
    return dict(id=cid, I=I, R=R, J=J, K=K, path=path, con=con, inner=inner, peak=peak, ridge=ridge, bsum_half=bsum_half,
                special=special)


def rank_class(R):
    return 4 if R <= 4 else (8 if R <= 8 else (16 if R <= 16 else 64))


C_SINGLE = [ccase('C1-R%d' % R, R, 5, (SINGLE, cls)) for R, cls in
            ((1, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 64), (64, 64))] + \
           [ccase('C1-K%d' % K, 3, K, (SINGLE, 4)) for K in (1, 64, 65, 300)]

C_WG = [ccase('Cwg-R%d' % R, R, 20, (WG, cls), NONNEG) for R, cls in
        ((1, 4), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16))] + \
       [ccase('Cwg-K%d' % K, 3, K, (WG, 4), NONNEG) for K in (1, 63, 64, 65, 255, 256)] + [
    # the butterfly max(rho): 200 rows = three full waves, 8 rows in the fourth, 56 padding threads on the last row's value
    ccase('Cwg-peak-first', 3, 200, (WG, 4), ('l1 regularization', 0.05), peak=5),
    ccase('Cwg-peak-lastwave', 3, 200, (WG, 4), ('l1 regularization', 0.05), peak=195),
    ccase('Cwg-peak-lastrow', 3, 200, (WG, 4), ('l1 regularization', 0.05), peak=199),
    ccase('Cwg-nonneg', 3, 70, (WG, 4), NONNEG),
    ccase('Cwg-box', 3, 70, (WG, 4), ('box', 0.6, 1.2)),
    ccase('Cwg-l1', 3, 70, (WG, 4), ('l1 regularization', 0.05)),
    ccase('Cwg-l0', 3, 70, (WG, 4), ('l0 regularization', 0.3)),
    ccase('Cwg-ridge', 3, 70, (WG, 4), ('ridge', 0.2)),
    ccase('Cwg-simplex', 5, 70, (WG, 8), ('simplex row-wise', 2.0)),
    ccase('Cwg-l2ball', 3, 70, (WG, 4), ('l2-ball', 5.0)),
    ccase('Cwg-nnl2ball', 3, 70, (WG, 4), ('non-negative l2-ball', 5.0)),
    ccase('Cwg-l2reg', 3, 70, (WG, 4), ('l2 regularization', 0.5)),
    ccase('Cwg-nnsphere', 3, 70, (WG, 4), ('non-negative l2-sphere', 1)),
    ccase('Cwg-nnsphere-zerocol', 3, 200, (WG, 4), ('non-negative l2-sphere', 1), special='zerocol'),
]

C_LAUNCHED = [
    ccase('Cl-K257-R3', 3, 257, (LAUNCHED, 4), NONNEG),                    # five workgroups of par2_c_rowsolve_k
    ccase('Cl-ridge-K257', 3, 257, (LAUNCHED, 4), ('ridge', 0.2)),          # both residuals fall steadily: the exit cases
    ccase('Cl-R17-K5', 17, 5, (LAUNCHED, 64), NONNEG),
    ccase('Cl-nondecr-K40', 3, 40, (LAUNCHED, 4), ('non-decreasing',)),
    ccase('Cl-tv-K40', 3, 40, (LAUNCHED, 4), ('TV regularization', 0.05)),
]

C_TERMS = [
    ccase('C-ridge-bsum-single', 5, 9, (SINGLE, 8), None, ridge=0.3, bsum_half=0.15),
    ccase('C-ridge-bsum-wg', 5, 9, (WG, 8), NONNEG, ridge=0.3, bsum_half=0.15),
]

ZEROCOL_ROW = 150


def _ckey(c):
    return (c['id'].split('|')[0], c['I'], c['R'], c['J'], c['con'], c['peak'], c['ridge'], c['bsum_half'], c['special'])


@functools.lru_cache(maxsize=None)
def _c_reference(key):
    cid, I, R, J, con, peak, ridge, bsum_half, special = key
    blk = make_block(cid, I, R, J, peak)
    Cm, Zc, muc = blk['C'], blk['Zc'], blk['muc']
    X = blk['X']
    if special == 'zerocol':
        # column 1 negative in every row of C, Z and mu, and so of fac + mu: the clamped column is all zero and the prox
        # puts the unit vector at the first maximum of the input, row ZEROCOL_ROW (fourth wave... third: rows 128..191)
        Cm, Zc, muc = Cm.copy(), Zc.copy(), muc.copy()
        Cm[:, 1] = -Cm[:, 1]
        Cm[ZEROCOL_ROW, 1] = -0.02
        Zc[:, 1] = Cm[:, 1]
        muc[:, 1] = -0.01
        X = [blk['A'] @ np.diag(Cm[k]) @ blk['B'][k].T for k in range(len(J))]
    sysd = REF.c_systems(X, blk['A'], blk['B'], Cm, WEIGHT, ridge, bsum_half)
    sysl = REF.c_systems(X, blk['A'], blk['B'], Cm, WEIGHT, ridge, bsum_half, ld=True)
    loop = REF.CLoop(sysd, con, Cm, Zc, muc, 'cho')
    alt = REF.CLoop(sysd, con, Cm, Zc, muc, 'inv')
    inp = dict(blk, X=X, C=Cm, Zc=Zc, muc=muc)
    return inp, sysd, sysl['a'], loop, alt


def c_reference(c):
    return _c_reference(_ckey(c))


def c_host(c, tol=(0.0, 0.0)):
    """(reference result, floor) of a case: the Cholesky-solve loop against the explicit-inverse loop, a against its
    longdouble sum."""
    inp, sysd, ald, loop, alt = c_reference(c)
    fa = rel(ald, sysd['a'])
    if c['con'] is None:
        ref = dict(C=loop.single(), Z=None, mu=None, inner_iters=0, res=(0.0, 0.0), scale=None)
        return ref, max(fa, rel(alt.single(), ref['C']))
    ref, other = loop.run(c['inner'], tol), alt.run(c['inner'], tol)
    assert other['inner_iters'] == ref['inner_iters'], 'the two host formulations stop at different iterations'
    d = [fa] + [rel(other[k], ref[k]) for k in ('C', 'Z', 'mu')]
    for q in range(2):
        if np.isfinite(ref['res'][q]) and ref['scale'][q] > 0:
            d.append(abs(other['res'][q] - ref['res'][q]) / (ref['scale'][q] + ref['res'][q]))
    return ref, max(d)


def c_floor(c):
    return c_host(c)[1]


def check_c(eng, c, tol=(0.0, 0.0), expect_iters=None):
    inp, sysd, ald, loop, _ = c_reference(c)
    ref, floor = c_host(c, tol)
    assert floor < MAX_FLOOR, ('the two host evaluations differ by %.2e: the input sits on a tie of a discontinuous prox; '
                               'pick another input' % floor)
    bar = max(1e-11, 10 * floor)
    if expect_iters is not None:
        assert ref['inner_iters'] == expect_iters
    con = c['con']
    out = eng.par2_mode_c(inp['X'], inp['A'], inp['B'], inp['C'], WEIGHT, c['ridge'], c['bsum_half'], con,
                          inp['Zc'] if con else None, inp['muc'] if con else None, c['inner'], tol)
    K, R, I = inp['K'], inp['R'], inp['I']
    L = np.stack(loop.L)
    d = dict(C=rel(out['C'], ref['C']), a=rel(out['a'], sysd['a']), rho=rel(out['rho'], sysd['rho']), L=rel(out['L'], L))
    if con:
        d.update(Z=rel(out['Z'], ref['Z']), mu=rel(out['mu'], ref['mu']))
    print('%s R %d K %d I %d inner %d: path %s its %d/%d floor %.2e bar %.2e %s res dev %s ref %s'
          % (c['id'], R, K, I, c['inner'], out['path'], out['inner_iters'], ref['inner_iters'], floor, bar,
             ' '.join('%s %.2e' % kv for kv in d.items()), ' '.join('%.15e' % v for v in out['res']),
             ' '.join('%.15e' % v for v in ref['res'])))
    assert out['path'] == c['path'], 'dispatch runs %s here, the case is meant for %s: pick a new shape' % (out['path'], c['path'])
    assert out['inner_iters'] == ref['inner_iters']
    for k, v in d.items():
        assert v < bar, (k, v, bar)
    # a(k,r): I terms in order on T1 entries of four partial sums: (I + J_k / 4 + 5) eps w sum_i |A| (|X_k| |B_k|)
    for k, j in enumerate(inp['J']):
        tot = WEIGHT * np.sum(np.abs(inp['A']) * (np.abs(inp['X'][k]) @ np.abs(inp['B'][k])), axis=0) \
            + c['bsum_half'] * np.abs(inp['C'][k])
        assert (np.abs(out['a'][k] - ald[k]) <= (I + j / 4 + 5) * EPS * tot).all(), k
    if out['path'][0] != WG:
        assert out['rho_max'] == np.max(out['rho'])                  # par2_max_k: a maximum has no rounding
    else:
        assert np.isnan(out['rho_max'])                              # the one-workgroup loop takes it itself
    if con:
        for q, name in enumerate(('pr_constr', 'du_constr')):
            bound = bar * (ref['scale'][q] + ref['res'][q])
            assert abs(out['res'][q] - ref['res'][q]) <= bound, (name, out['res'][q], ref['res'][q], bound)
    return out, ref


@pytest.mark.parametrize('c', _params(C_SINGLE + C_TERMS[:1]))
def test_mode_c_single_solve(eng, c):
    check_c(eng, c, expect_iters=0)


@pytest.mark.parametrize('c', _params(C_WG + C_TERMS[1:]))
def test_mode_c_one_workgroup_loop(eng, c):
    inp, sysd, _, loop, _ = c_reference(c)
    if c['peak'] is not None:
        assert int(np.argmax(sysd['rho'])) == c['peak'] and sysd['rho'].max() > 1.2 * np.sort(sysd['rho'])[-2]
    assert sysd['rho'].max() > 5 * sysd['rho'].min() or c['K'] < 3
    out, ref = check_c(eng, c, expect_iters=5)
    if c['special'] == 'zerocol':
        first = loop.run(1)
        e = np.zeros(c['K'])
        e[ZEROCOL_ROW] = 1.0
        assert ZEROCOL_ROW > 64 and np.array_equal(first['Z'][:, 1], e)      # the all-zero-column branch ran (reference)
        one, _ = check_c(eng, dict(c, id=c['id'] + '|inner1', inner=1), expect_iters=1)
        assert np.array_equal(one['Z'][:, 1], e)


def _with(c, suffix, **kw):
    d = dict(c)
    d.update(kw)
    d['id'] = c['id'] + '|' + suffix
    return d


_BY_ID = {c['id']: c for c in C_SINGLE + C_WG + C_LAUNCHED + C_TERMS}
INNER_BASES = ['Cwg-R3', 'Cwg-R9', 'Cwg-K65', 'Cwg-l2reg', 'Cl-K257-R3']
INNER_CASES = [_with(_BY_ID[b], 'inner%d' % n, inner=n) for b in INNER_BASES for n in (1, 6)]


@pytest.mark.parametrize('c', _params(INNER_CASES))
def test_mode_c_runs_to_max_inner(eng, c):
    check_c(eng, c, expect_iters=c['inner'])


@pytest.mark.parametrize('c', _params(C_LAUNCHED))
def test_mode_c_launched_loop(eng, c):
    check_c(eng, c, expect_iters=5)


def pick_exit(series):
    """Iterations k in 2..9 (1-based) whose residual is below 0.8 x the smallest earlier one -> [(k, tolerance)]; the
    tolerance is the geometric mean of the two, > 10 % away from both."""
    out = []
    for k in range(2, EXIT_INNER):
        lo = min(series[:k - 1])
        if 0 < series[k - 1] < 0.8 * lo:
            out.append((k, float(np.sqrt(series[k - 1] * lo))))
    return out


def exit_plan(c, which):
    """(case, k*, tolerances) from the reference history alone; asserts the 10 % margin up to k*."""
    c = _with(c, 'exit%d' % which, inner=EXIT_INNER)
    loop = c_reference(c)[3]
    hist = loop.history(EXIT_INNER)
    picks = pick_exit(hist[which])
    assert picks, '%s no longer has such an exit iteration in 2..9 with the 0.8 gap: pick another input' % c['id']
    kstar, t = picks[len(picks) // 2]
    tol = tuple(t if q == which else INF for q in range(2))
    assert 1 < kstar < EXIT_INNER
    for k in range(1, kstar + 1):
        assert abs(hist[which][k - 1] / t - 1.0) > 0.1
        assert (hist[which][k - 1] > t) == (k < kstar)
    return c, kstar, tol


EXIT_BASES = ['Cl-ridge-K257', 'Cwg-ridge']


@pytest.mark.parametrize('base', EXIT_BASES)
@pytest.mark.parametrize('which', [0, 1], ids=['pr', 'du'])
def test_mode_c_early_exit(eng, base, which):
    """Each tolerance alone ends the loop at k*; the launched form then runs its remaining launches under a closed ctl
    (CTL_GUARD), which must leave the state of iteration k* untouched."""
    c, kstar, tol = exit_plan(_BY_ID[base], which)
    out, _ = check_c(eng, c, tol, expect_iters=kstar)
    last = c_reference(c)[3].run(EXIT_INNER)
    assert rel(out['mu'], last['mu']) > 1e-6


def test_mode_c_zero_slab_is_not_positive_definite(eng, pkg):
    """B_k = 0: GB_k = 0, C_k = 0 and rho_k = 0, so the row's system is the zero matrix and chol fails: a return code."""
    c = _BY_ID['C1-R4']
    inp = c_reference(c)[0]
    B = [b.copy() for b in inp['B']]
    B[2][:] = 0.0
    for con in (None, NONNEG):
        with pytest.raises(pkg.NotPositiveDefinite):
            eng.par2_mode_c(inp['X'], inp['A'], B, inp['C'], WEIGHT, 0.0, 0.0, con, inp['Zc'] if con else None,
                            inp['muc'] if con else None, 2, (0.0, 0.0))


# ---------------------------------------------------------------------------------------------------------------------
# mode C, the systems of a coupled C mode
# ---------------------------------------------------------------------------------------------------------------------
def scase(system, R, con):
    return dict(id='Csys%d-R%d-con%d' % (system, R, con), system=system, R=R, con=con, K=6, I=max(R, 6) + 1,
                J=tuple(R + 1 + (3 * k) % 4 for k in range(6)))


S_CASES = [scase(s, R, con) for s in (1, 2, 3, 4) for R in (3, 9, 17) for con in (0, 1)]


@functools.lru_cache(maxsize=None)
def s_reference(cid, system, R, con, I, J):
    blk = make_block(cid, I, R, J)
    rng = np.random.default_rng(zlib.crc32(cid.encode()) + 1)
    K = len(J)
    sysmat = None
    if system == 2:
        H = rng.standard_normal((R, R + 2))
        sysmat = H @ H.T
    elif system == 3:
        sysmat = rng.random(K) + 0.2
    elif system == 4:
        H = rng.standard_normal((K + 1, K))
        sysmat = H.T @ H                                                      # off-diagonal entries
    sysd = REF.c_systems(blk['X'], blk['A'], blk['B'], blk['C'], WEIGHT, 0.2, 0.1)
    sysl = REF.c_systems(blk['X'], blk['A'], blk['B'], blk['C'], WEIGHT, 0.2, 0.1, ld=True)
    ref = REF.c_coupled(sysd, system, con, sysmat)
    # the second host evaluation: GA and GB_k from longdouble products, rounded
    GA = (blk['A'].astype(LD).T @ blk['A'].astype(LD)).astype(np.float64)
    GB = [(b.astype(LD).T @ b.astype(LD)).astype(np.float64) for b in blk['B']]
    alt = REF.c_coupled(REF.c_systems(blk['X'], blk['A'], blk['B'], blk['C'], WEIGHT, 0.2, 0.1, GA=GA, GB=GB), system, con, sysmat)
    d = [rel(sysl['a'], sysd['a']), rel(np.stack(alt['L']), np.stack(ref['L']))]
    if system == 4:
        d.append(rel(alt['M'], ref['M']))
    return blk, sysmat, sysd, ref, max(d)


def s_floor(c):
    return s_reference(c['id'], c['system'], c['R'], c['con'], c['I'], c['J'])[4]


@pytest.mark.parametrize('c', _params(S_CASES))
def test_mode_c_coupled_systems(eng, c):
    blk, sysmat, sysd, ref, floor = s_reference(c['id'], c['system'], c['R'], c['con'], c['I'], c['J'])
    assert floor < MAX_FLOOR
    bar = max(1e-11, 10 * floor)
    out = eng.par2_mode_c(blk['X'], blk['A'], blk['B'], blk['C'], WEIGHT, 0.2, 0.1, NONNEG if c['con'] else None,
                          system=c['system'], sysmat=sysmat)
    d = dict(a=rel(out['a'], sysd['a']), rho=rel(out['rho'], sysd['rho']), L=rel(out['L'], np.stack(ref['L'])))
    if c['system'] == 4:
        d['M'] = rel(out['M'], ref['M'])
    print('%s: path %s floor %.2e bar %.2e %s' % (c['id'], out['path'], floor, bar, ' '.join('%s %.2e' % kv for kv in d.items())))
    assert out['path'] == (-1, rank_class(c['R'])) and out['inner_iters'] == 0
    assert np.array_equal(out['C'], blk['C'])
    for k, v in d.items():
        assert v < bar, (k, v, bar)
    assert out['rho_max'] == np.max(out['rho'])
    # par2_max_k: 64 lanes add ceil(K / 64) values in order, 6 butterfly levels: (ceil(K / 64) + 6) eps sum(rho)
    bound = seq_tree(math.ceil(c['K'] / 64), 6, 0) * float(np.sum(out['rho']))
    assert abs(out['rho_sum'] - float(np.sum(out['rho'].astype(LD)))) <= bound
    assert abs(out['rho_mean'] - out['rho_sum'] / c['K']) <= EPS * out['rho_mean']


def test_mode_c_dense_system_exact_small_integers(eng):
    """system 4 on integers, R = K = 4, w = 1: a, rho = trace / 4, the raw B_k and M = blkdiag(B_k) + mean(rho)/2 kron(HtH, I)
    are exact.  HtH is given WITHOUT symmetry: a swapped k / k2 or r / q in par2_c_big_system_k changes M."""
    rng = np.random.default_rng(12)
    I, R, K = 6, 4, 4
    J = [4, 5, 6, 7]
    X = [rng.integers(-2, 3, size=(I, j)).astype(np.float64) for j in J]
    A = rng.integers(-2, 3, size=(I, R)).astype(np.float64)
    B = [rng.integers(-2, 3, size=(j, R)).astype(np.float64) for j in J]
    Cm = rng.integers(1, 4, size=(K, R)).astype(np.float64)
    HtH = rng.integers(0, 5, size=(K, K)).astype(np.float64) * 8.0          # mean(rho) / 2 = t / 32: multiples of 8 keep M integer
    assert not np.array_equal(HtH, HtH.T)
    sysd = REF.c_systems(X, A, B, Cm, 1.0, 2.0, 0.0)
    ref = REF.c_coupled(sysd, 4, False, HtH)
    out = eng.par2_mode_c(X, A, B, Cm, 1.0, 2.0, 0.0, None, system=4, sysmat=HtH)
    assert np.array_equal(out['a'], sysd['a']) and np.array_equal(out['rho'], sysd['rho'])
    assert np.array_equal(out['L'], np.stack(sysd['Bk']))
    assert np.array_equal(out['M'], ref['M'])
    assert (out['rho_max'], out['rho_mean'], out['rho_sum']) == (ref['rho_max'], ref['rho_mean'], ref['rho_sum'])


# ---------------------------------------------------------------------------------------------------------------------
# objective pieces
# ---------------------------------------------------------------------------------------------------------------------
def ocase(cid, I, R, J0, reg=None, withZ=True, last=1):
    # neighbours of equal size (slabs 0, 1 and 2, 3), of unequal size (1 -> 2, 3 -> 4) and J_k = 1
    return dict(id=cid, I=I, R=R, J=(J0, J0, J0 - 1, J0 - 1, last), reg=reg, withZ=withZ)


# O-reg-gl ends in a slab of two rows, not one: constraints_to_prox.m:71-73 builds the path Laplacian as 2 I - shifts and
# then overwrites its corners with 1, which for a single row leaves L = 1 (reg_func = eta x^2) where a path of one node
# has no edge (par2_reg_k: 0).  The reference defines the GL term on B_k only for slabs of one common size, so a single-row
# slab beside longer ones has no reference value at all.
O_CASES = [
    ocase('O-n200', 8, 3, 25), ocase('O-n1023', 33, 3, 31), ocase('O-n1024', 32, 3, 32), ocase('O-n1025', 25, 3, 41),
    ocase('O-n5000', 50, 3, 100), ocase('O-R1', 32, 1, 32), ocase('O-R64', 32, 64, 32), ocase('O-noZ', 32, 3, 32, withZ=False),
    ocase('O-reg-l1', 8, 3, 70, ('l1 regularization', 0.3)), ocase('O-reg-l0', 8, 3, 70, ('l0 regularization', 0.3)),
    ocase('O-reg-l2', 8, 3, 70, ('l2 regularization', 0.3)), ocase('O-reg-ridge', 8, 3, 70, ('ridge', 0.3)),
    ocase('O-reg-gl', 8, 3, 70, ('GL smoothness', 0.3), last=2), ocase('O-reg-tv', 8, 3, 70, ('TV regularization', 0.3)),
]


@functools.lru_cache(maxsize=None)
def o_reference(cid, I, R, J, reg, withZ):
    blk = make_block(cid, I, R, J)
    if reg is not None and reg[0] == 'l0 regularization':
        blk = dict(blk, B=[np.where(np.abs(b) < 0.1 * np.abs(b).max(), 0.0, b) for b in blk['B']])
    args = (blk['X'], blk['A'], blk['B'], blk['C'], blk['P'], blk['DeltaB'], blk['Zb'] if withZ else None, reg)
    ref, alt = REF.objective(*args), REF.objective(*args, ld=True)
    d = [rel(alt['res'], ref['res']), rel(alt['q'], ref['q'])]
    if reg is not None and reg[0] != 'TV regularization':                     # the TV quirk is a telescoping sum: see its bound
        d.append(rel(alt['regv'], ref['regv']))
    return blk, ref, alt, max(d)


def o_floor(c):
    return o_reference(c['id'], c['I'], c['R'], c['J'], c['reg'], c['withZ'])[3]


@pytest.mark.parametrize('c', _params(O_CASES))
def test_objective(eng, c):
    blk, ref, alt, floor = o_reference(c['id'], c['I'], c['R'], c['J'], c['reg'], c['withZ'])
    assert floor < MAX_FLOOR
    I, R, reg = c['I'], c['R'], c['reg']
    Zb = blk['Zb'] if c['withZ'] else None
    out = eng.par2_objective(blk['X'], blk['A'], blk['B'], blk['C'], blk['P'], blk['DeltaB'], Zb, reg)
    print('%s: floor %.2e res %.2e q %.2e' % (c['id'], floor, rel(out['res'], alt['res']), rel(out['q'], alt['q'])))
    absA, absD = np.abs(blk['A']), np.abs(blk['DeltaB'])
    for k, j in enumerate(c['J']):
        Bk, Xk = blk['B'][k], blk['X'][k]
        n = I * j
        M = blk['A'] @ np.diag(blk['C'][k]) @ Bk.T
        Mabs = absA @ np.diag(np.abs(blk['C'][k])) @ np.abs(Bk).T
        # 256 threads, ceil(n / 256) squares in order, 8 tree levels, 3 roundings per square; the model entry carries
        # (R + 2) eps sum_r |a c b|
        bound = seq_tree(math.ceil(n / 256), 8, 3) * float(alt['res'][k]) + 2 * (R + 2) * EPS * float(np.sum(np.abs(Xk - M) * Mabs))
        assert abs(out['res'][k] - float(alt['res'][k])) <= bound, ('res', k, out['res'][k], float(alt['res'][k]), bound)
        # 64 threads, ceil(J_k R / 64) terms in order, 6 tree levels, 3 roundings per term
        cnt = seq_tree(math.ceil(j * R / 64), 6, 3)
        PD = blk['P'][k] @ blk['DeltaB']
        b0 = cnt * float(alt['q'][k, 0]) + 2 * (R + 2) * EPS * float(np.sum(np.abs(Bk - PD) * (np.abs(blk['P'][k]) @ absD)))
        for col, bnd in ((0, b0), (1, cnt * float(alt['q'][k, 1])), (2, cnt * float(alt['q'][k, 2])), (3, cnt * float(alt['q'][k, 3]))):
            assert abs(out['q'][k, col] - float(alt['q'][k, col])) <= bnd, ('q', k, col)
        if not c['withZ']:
            assert out['q'][k, 2] == 0.0
        if k == 0 or c['J'][k] != c['J'][k - 1]:
            assert out['q'][k, 3] == 0.0
        else:
            assert out['q'][k, 3] > 0.0
        if reg is not None:
            eta, name = reg[1], reg[0]
            if name == 'l2 regularization':
                # per column (ceil(J_k / 64) + 8) eps on the sum of squares, halved by the root, + 1; R columns in order
                bnd = (math.ceil(j / 64) / 2 + R + 6) * EPS * float(alt['regv'][k])
            else:
                terms = {'l1 regularization': np.abs(Bk), 'l0 regularization': (Bk != 0).astype(float), 'ridge': Bk * Bk,
                         'GL smoothness': np.diff(Bk, axis=0) ** 2, 'TV regularization': np.abs(np.diff(Bk, axis=0))}[name]
                bnd = cnt * eta * float(np.sum(terms))
            assert abs(out['regv'][k] - float(alt['regv'][k])) <= bnd, ('regv', k, out['regv'][k], float(alt['regv'][k]), bnd)
    if reg is None:
        assert out['regv'] is None


def test_objective_exact_small_integers(eng):
    """Integers without symmetry: every residual, gap and regularisation value is an exact integer (eta = 0.5: a
    half-integer) in any order."""
    rng = np.random.default_rng(13)
    I, R = 7, 3
    A = rng.integers(-2, 3, size=(I, R)).astype(np.float64)
    DeltaB = rng.integers(-2, 3, size=(R, R)).astype(np.float64)
    assert not np.array_equal(DeltaB, DeltaB.T)
    for reg in (None, ('l1 regularization', 0.5), ('l0 regularization', 0.5), ('ridge', 0.5), ('GL smoothness', 0.5),
                ('TV regularization', 0.5)):
        J = [5, 5, 6, 2 if reg and reg[0] == 'GL smoothness' else 1, 9]      # GL on a single row: see O_CASES
        X = [rng.integers(-3, 4, size=(I, j)).astype(np.float64) for j in J]
        B = [rng.integers(-2, 3, size=(j, R)).astype(np.float64) for j in J]
        P = [rng.integers(-1, 2, size=(j, R)).astype(np.float64) for j in J]
        Zb = [rng.integers(-2, 3, size=(j, R)).astype(np.float64) for j in J]
        Cm = rng.integers(1, 4, size=(len(J), R)).astype(np.float64)
        ref = REF.objective(X, A, B, Cm, P, DeltaB, Zb, reg)
        out = eng.par2_objective(X, A, B, Cm, P, DeltaB, Zb, reg)
        assert np.array_equal(out['res'], np.rint(ref['res'])) and np.array_equal(out['q'], np.rint(ref['q'])), reg
        if reg is not None:
            assert np.array_equal(out['regv'], np.rint(2 * ref['regv']) / 2), reg


def test_refusals(pkg):
    """A context that drives several devices, and one that belongs to a communicator (here of one rank): the three
    entries answer AOADMM_ERR_UNSUPPORTED before anything is uploaded."""
    blk = make_block('refused', 7, 3, (4, 5, 6))

    def all_three(e):
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.par2_mode_a(blk['X'], blk['B'], blk['C'])
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.par2_mode_c(blk['X'], blk['A'], blk['B'], blk['C'], WEIGHT)
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.par2_objective(blk['X'], blk['A'], blk['B'], blk['C'], blk['P'], blk['DeltaB'])

    with pkg.Engine([0]) as e:
        all_three(e)
    with pkg.Engine(0) as e:
        e.comm_init_rank(e.comm_unique_id(), 0, 1)
        all_three(e)


# every case that has a host floor, for the CPU check of MAX_FLOOR and LARGEST_FLOOR (tests/test_par2_modes_host.py)
def all_floors():
    out = {c['id']: a_floor(c) for c in A_CASES}
    out.update({c['id']: c_floor(c) for c in C_SINGLE + C_WG + C_LAUNCHED + C_TERMS + INNER_CASES})
    for base in EXIT_BASES:
        for which in (0, 1):
            c, _, tol = exit_plan(_BY_ID[base], which)
            out[c['id']] = c_host(c, tol)[1]
    out.update({c['id']: s_floor(c) for c in S_CASES})
    out.update({c['id']: o_floor(c) for c in O_CASES})
    return out
