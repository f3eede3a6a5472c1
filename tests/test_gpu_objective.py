"""GPU: the objective evaluation (CMTF_AOADMM_func_eval; csrc/solver_objective.hip, reduce_batch in csrc/small.hip,
reg_value in csrc/misc.hip, the coupling images of csrc/solver_coupled.hip) per reduction class, against the longdouble
reference of tests/objective_ref.py (pinned to the oracle by tests/test_objective_ref_host.py).

The solver's own path is driven: build_model, upload_state of a state in which no term is zero, run_solver with
MaxOuterIters = 0.  Element 0 of func_val_conv / func_coupl_conv / func_constr_conv is then the first evaluation of
exactly that state; the later-evaluation tests run two outer iterations and evaluate the downloaded state instead.

reduce_batch cuts every task of a batch into nsplit = min(64, cdiv(largest task, 2048)) pieces of per = cdiv(n, nsplit)
elements (RT_REG: of cdiv(rows, nsplit) rows, flattened with the columns), so the tensors stay tiny and the LONG mode of
a block picks the class: one split, two, an interior count, the cap of 64, beyond the cap, piece lengths on both sides of
the unrolled loop's 1024, and the empty pieces the short modes get in the same batch.

Tolerances (derived, not tuned).  A device sum and its reference differ by summation order only, so every comparison is
bounded by REL64 = 1e-12 (the project's bound for fp64 summation order, test_mttkrp_matches_oracle) of the magnitude S
the term was cancelled from: w (||X||^2 + 2 |<X, M>| + ||M||^2) for a tensor term, the sum of the absolute summands for a
regulariser value, numerator and denominator separately for a ratio (objective_ref.ObjectiveRef.bounds).  With fp32
storage the tensor term alone gets REL32 = 2e-6, the project's fp32 MTTKRP bound; everything else is computed from the
fp64 factors whatever the storage.  Every case prints its error as a fraction of its bound; on an MI355X the largest
fraction over all cases was 0.0012 (the fp32 case's f_tensors; 0.0002 for a ratio), so nothing here needed more."""

import numpy as np
import pytest

import objective_ref
from helpers import options
from oracle.tensor_ops import full_ktensor

pytestmark = pytest.mark.gpu

REL64 = 1e-12
REL32 = 2e-6
NN = ('non-negativity',)
SPLIT_CAP = 64                      # kReduceBatchSplit
SPLIT_UNIT = 2048


def cdiv(a, b):
    return -(-a // b)


def nsplit_of(n):
    return max(1, min(SPLIT_CAP, cdiv(n, SPLIT_UNIT)))


# ---- models -----------------------------------------------------------------------------------------------------------
def make_Z(shapes, ranks, objects, constraints, weights=None, lin=None, ctype=(), H=None, H2=None, ridge=None):
    modes, size, mode_ranks = [], [], []
    for shp, R in zip(shapes, ranks):
        modes.append(list(range(len(size) + 1, len(size) + len(shp) + 1)))
        size += [int(s) for s in shp]
        mode_ranks += [R] * len(shp)
    nm, P = len(size), len(shapes)
    coupling = dict(lin_coupled_modes=list(lin) if lin else [0] * nm, coupling_type=list(ctype),
                    coupl_trafo_matrices=list(H) if H else [None] * nm)
    if H2 is not None:
        coupling['coupl_trafo_matrices2'] = list(H2)
    Z = dict(loss_function=['Frobenius'] * P, model=['CP'] * P, modes=modes, size=size, coupling=coupling,
             constrained_modes=[0 if c is None else 1 for c in constraints], constraints=list(constraints),
             weights=list(weights) if weights else [1.0] * P, object=list(objects), _ranks=mode_ranks)
    if ridge is not None:
        Z['ridge'] = list(ridge)
    return Z


def block_data(rng, dims, R, noise=0.05):
    """(X, A): X = [[A]] + noise, A signed"""
    A = [rng.standard_normal((n, R)) for n in dims]
    X = full_ktensor(A)
    X = X + noise * np.sqrt(np.mean(X * X)) * rng.standard_normal(X.shape)
    return X, A


def off(A, rng, s=0.2):
    return [a + s * rng.standard_normal(a.shape) for a in A]


def dual_shapes(Z, fac, Delta):
    """shape of coupling_dual_fac per mode (init_coupled_AOADMM_CMTF.m:133-169): Delta's for types 0, 1, 2, the factor's
    for types 3, 4, and (rows of Delta, columns of the factor) for type 5; None for an uncoupled mode"""
    out = []
    for m, c in enumerate(Z['coupling']['lin_coupled_modes']):
        if not c:
            out.append(None)
            continue
        ct, D = Z['coupling']['coupling_type'][c - 1], Delta[c - 1]
        out.append(D.shape if ct <= 2 else fac[m].shape if ct <= 4 else (D.shape[0], fac[m].shape[1]))
    return out


def noisy_state(Z, fac, rng, Delta=(), s=0.1):
    """constraint_fac = fac + s * noise on the constrained modes, so no constraint term is zero; the duals, which the
    evaluation does not read but the solver wants present, are noise as well"""
    noise = lambda shape: s * rng.standard_normal(shape)
    con = Z['constrained_modes']
    return dict(fac=list(fac), coupling_fac=list(Delta),
                constraint_fac=[F + noise(F.shape) if c else None for F, c in zip(fac, con)],
                constraint_dual_fac=[noise(F.shape) if c else None for F, c in zip(fac, con)],
                coupling_dual_fac=[None if shp is None else noise(shp) for shp in dual_shapes(Z, fac, Delta)])


def long_block(rng, rows, R, long_constraint=NN, ridge=(0.5, 0.0, 0.25), rest=(3, 2)):
    """one block (rows, 3, 2): long mode constrained as asked, second mode non-negative, third free"""
    dims = (rows,) + tuple(rest)
    X, A = block_data(rng, dims, R)
    Z = make_Z([dims], [R], [X], [long_constraint, NN, None], ridge=ridge)
    fac = off(A, rng)
    if rows > 1:                                   # exact zeros of both signs: l0 counts neither
        fac[0][::5, 0] = 0.0
        fac[0][1::7, -1] = -0.0
    return Z, noisy_state(Z, fac, rng)


# ---- device and comparison --------------------------------------------------------------------------------------------
def device_eval(pkg, eng, Z, G, prec='f64'):
    pkg.build_model(eng, Z, prec)
    pkg.upload_state(eng, Z, G)
    out = pkg.run_solver(eng, options(MaxOuterIters=0), len(Z['size']))
    assert out['OuterIterations'] == 0
    return out['func_val_conv'][0], out['func_coupl_conv'][0], out['func_constr_conv'][0]


def compare(dev, ref, bounds, what):
    """all three pieces, each within its bound; prints the error as a fraction of the bound"""
    frac = [abs(d - r) / b if b > 0 else (0.0 if d == r else np.inf) for d, r, b in zip(dev, ref.f, bounds)]
    print('%s: device %s reference %s error/bound %s' % (what, tuple(dev), ref.f, np.round(frac, 4)))
    for name, d, r, b in zip(('f_tensors', 'f_couplings', 'f_constraints'), dev, ref.f, bounds):
        assert np.isfinite(d) and abs(d - r) <= b, (what, name, d, r, abs(d - r), b)
    return frac


def check(pkg, eng, Z, G, what, prec='f64'):
    ref = objective_ref.evaluate(Z, G)
    assert ref.f_tensors != 0 and ref.f_constraints != 0
    bounds = ref.bounds(REL64)
    if prec == 'f32':                              # the tensor terms come from fp32 data through fp32 passes
        st = float(sum(t[2] for t in ref.terms if t[0].startswith('tensor')))
        bounds = (REL32 * st + REL64 * (ref.mag_tensors - st),) + tuple(bounds[1:])
    return compare(device_eval(pkg, eng, Z, G, prec), ref, bounds, what), ref


# ---- 1. split classes of reduce_batch ---------------------------------------------------------------------------------
# rows x R of the long mode -> n = rows * R -> nsplit: 2048 -> 1;  683 * 3 = 2049 -> 2;  4097 * 20 = 81940 -> 41 with
# per = cdiv(81940, 41) = 1999, which does not divide n (the last piece has 1980);  4099 * 64 = 262336 -> cdiv = 129,
# capped at 64, per = 4099;  131073 -> capped at 64, per = 2049, last piece 1986: the unrolled loop runs two trips in
# every piece.  Ranks 1, 3, 20 and 64: all modes of a block share R.
SPLIT_SHAPES = [(2048, 1), (683, 3), (4097, 20), (4099, 64), (131073, 1)]
EDGE_SHAPES = [(1, 3), (2, 3), (33, 64)]           # no differences; one; 33 * 64 = 2112 -> 2 pieces of 17 and 16 rows


def test_split_rule_of_the_shapes():
    assert [nsplit_of(r * R) for r, R in SPLIT_SHAPES] == [1, 2, 41, 64, 64]
    assert cdiv(81940, 41) == 1999 and 81940 % 1999 != 0 and cdiv(131073, 64) == 2049
    assert nsplit_of(33 * 64) == 2 and cdiv(33, 2) == 17


@pytest.mark.parametrize('rows,R', SPLIT_SHAPES, ids=['%dx%d' % s for s in SPLIT_SHAPES])
def test_split_classes(pkg, eng, rows, R):
    """Tensor dots, ||fac||^2, ||fac - Z||^2 and the ridge term of a long mode in every split class; the modes of 3 and 2
    rows get empty pieces in the same batch."""
    Z, G = long_block(np.random.default_rng(rows + R), rows, R)
    check(pkg, eng, Z, G, 'split %dx%d' % (rows, R))


def test_split_class_fp32_storage(pkg, eng):
    """prec = 'f32': the reference takes X rounded to fp32, which is what the device stores."""
    Z, G = long_block(np.random.default_rng(32), 4097, 20)
    Z['object'] = [Z['object'][0].astype(np.float32).astype(np.float64)]
    check(pkg, eng, Z, G, 'split 4097x20 f32', prec='f32')


# Piece lengths around the unrolled loop (`e + 768 < e1`, four loads 256 apart, then a tail): 1023, 1024, 1025.
# The largest task of the batch sets nsplit = 2 (2048 < n <= 4096), and per = cdiv(n', 2) for EVERY task n' of the batch:
#   R = 3, block (683, 682, 2): n = 2049 -> pieces 1025, 1024;   n' = 682 * 3 = 2046 -> pieces 1023, 1023
#   R = 2, block (1025, 1024, 2): n = 2050 -> pieces 1025, 1025;  n' = 2048 -> pieces 1024, 1024
#   R = 1, matrix (2049, 2047):  n = 2049 -> pieces 1025, 1024;  n' = 2047 -> pieces 1024, 1023
# (a piece of 1023 cannot be the largest task's: two pieces of at most 1024 are one split).  RT_REG flattens
# cdiv(rows, 2) rows with the R columns: 342 * 3 = 1026 and 341 * 3 = 1023;  513 * 2 = 1026, 512 * 2 = 1024;  1025, 1024, 1023.
LENGTH_MODELS = {3: (683, 682, 2), 2: (1025, 1024, 2), 1: (2049, 2047)}
LENGTH_REGS = [(NN, NN), (('TV regularization', 0.4), ('GL smoothness', 0.9)), (('GL smoothness', 0.9), ('TV regularization', 0.4)),
               (('l1 regularization', 0.3), ('ridge', 1.3)), (('l0 regularization', 0.02), ('l1 regularization', 0.3))]


@pytest.mark.parametrize('regs', LENGTH_REGS, ids=['%s+%s' % (a[0].split()[0], b[0].split()[0]) for a, b in LENGTH_REGS])
@pytest.mark.parametrize('R', [3, 2, 1])
def test_piece_lengths_around_the_unrolled_loop(pkg, eng, R, regs):
    dims = LENGTH_MODELS[R]
    assert nsplit_of(dims[0] * R) == 2 and nsplit_of(dims[1] * R) <= 2
    rng = np.random.default_rng(100 + R)
    X, A = block_data(rng, dims, R)
    Z = make_Z([dims], [R], [X], list(regs) + [None] * (len(dims) - 2), ridge=[0.5, 0.25] + [0.0] * (len(dims) - 2))
    fac = off(A, rng)
    fac[1][::5, 0] = 0.0
    check(pkg, eng, Z, noisy_state(Z, fac, rng), 'lengths R=%d %s' % (R, [r[0] for r in regs]))


# ---- 2. regulariser values ----------------------------------------------------------------------------------------------
REGS = [('l1 regularization', 0.3), ('l0 regularization', 0.02), ('l2 regularization', 0.7), ('ridge', 1.3),
        ('GL smoothness', 0.9), ('TV regularization', 0.4)]


@pytest.mark.parametrize('rows,R', SPLIT_SHAPES + EDGE_SHAPES, ids=['%dx%d' % s for s in SPLIT_SHAPES + EDGE_SHAPES])
@pytest.mark.parametrize('reg', REGS, ids=[r[0].split()[0] for r in REGS])
def test_regulariser_values(pkg, eng, reg, rows, R):
    """Each value-carrying regulariser on the long mode: RT_REG split over rows (differences across a split boundary but
    not across a column end), reg_value_k for l2.  The eta are O(1) and the data O(1), so the value is a visible share
    of f_tensors and of its magnitude; one wrong summand is many orders above the bound."""
    Z, G = long_block(np.random.default_rng(7 * rows + R), rows, R, reg)
    _, ref = check(pkg, eng, Z, G, '%s %dx%d' % (reg[0], rows, R))
    (_, value, mag), = ref.term('reg 0')
    if rows == 1 and reg[0] in ('GL smoothness', 'TV regularization'):
        assert value == 0 and mag == 0                # one row: no differences
    else:
        assert mag > 0


@pytest.mark.parametrize('rows,R', [(1024, 3), (1025, 3), (2500, 3), (2500, 20)], ids=lambda v: str(v))
def test_l2_value_beyond_one_workgroup(pkg, eng, rows, R):
    """reg_value_k: one workgroup of 1024 threads per launch, a strided loop over the rows of a column and block_reduce_n
    per column: a column of exactly 1024 rows, one more, and several trips; 3 and 20 columns."""
    Z, G = long_block(np.random.default_rng(rows + R), rows, R, ('l2 regularization', 0.7))
    check(pkg, eng, Z, G, 'l2 %dx%d' % (rows, R))


# ---- 3. quadratic regularisation value ---------------------------------------------------------------------------------
def quad_L(rng, n, kind):
    """sym: dense symmetric (300 rows); the library diagonalises a symmetric L on the host with a cyclic Jacobi method
    when the constraint is set, O(n^3) per sweep for a dense matrix, so the symmetric L of 1100 rows is a randomly
    permuted block-diagonal matrix (blocks of 8): its non-zeros lie all over the 1100 x 1100 array the device's
    `gemm_small` multiplies, and the rotations stay inside the blocks.  nonsym: dense at both sizes."""
    if kind == 'nonsym':
        return rng.standard_normal((n, n)) / np.sqrt(n) + np.eye(n)
    if n <= 300:
        B = rng.standard_normal((n, n))
        return (B + B.T) / np.sqrt(n)
    L = np.zeros((n, n))
    for s in range(0, n, 8):
        b = min(8, n - s)
        B = rng.standard_normal((b, b))
        L[s:s + b, s:s + b] = B + B.T
    p = rng.permutation(n)
    return np.ascontiguousarray(L[np.ix_(p, p)])


@pytest.mark.parametrize('R', [3, 20])
@pytest.mark.parametrize('rows', [300, 1100])
@pytest.mark.parametrize('kind', ['sym', 'nonsym'])
def test_quadratic_value(pkg, eng, kind, rows, R):
    """eta trace(x' L x): L x by gemm_small (rows x rows), then RT_DOT with the factor; 1100 * 3 and both sizes at R = 20
    split."""
    rng = np.random.default_rng(rows + R)
    L = quad_L(rng, rows, kind)
    assert (np.abs(L - L.T).max() == 0) == (kind == 'sym')
    Z, G = long_block(rng, rows, R, ('quadratic regularization', 0.6, L))
    _, ref = check(pkg, eng, Z, G, 'quadratic %s %dx%d' % (kind, rows, R))
    assert ref.term('reg 0')[0][2] > 0


# ---- 4. couplings, types 0 to 5 -------------------------------------------------------------------------------------------
def coupled_model(rng, ctype):
    """Two blocks coupled in their long modes, the relations of helpers.transformed_coupling_model scaled up: every-second
    -row sampling on the row side (types 1, 3, 5), shared-column selectors on the column side (types 2, 4, 5).  Images
    (rows x columns): type 1: 650 x 3 twice (1950 < 2048) next to factors of 1950 and 3900;  type 3: 650 x 3 and
    1300 x 3 = 3900;  type 4: 650 x 4 = 2600 and 650 x 3 = 1950;  type 5: 650 x 4 = 2600 and 650 x 3;  types 0 and 2 give
    both members the same image, 1100 x 3 = 3300.  Unequal block weights: f_2 = <w * mttkrp, fac> / w."""
    n1, n4 = 650, 1300
    sub = np.zeros((n1, n4))
    sub[np.arange(n1), 2 * np.arange(n1)] = 1.0
    sel = np.vstack([np.eye(3), np.zeros((1, 3))])                 # 4 x 3: the first three of four columns
    H, H2 = [None] * 6, None
    if ctype == 0:
        D = rng.random((1100, 3)); F1, F4, Delta = D, D, D
    elif ctype == 1:                                               # H*C = Delta
        D = rng.random((n4, 3)); F1, F4, Delta = sub @ D, D, sub @ D
        H[0], H[3] = np.eye(n1), sub
    elif ctype == 2:                                               # C*H = Delta
        D = rng.random((1100, 4)); F1, F4, Delta = D, D[:, :3], D[:, :3]
        H[0], H[3] = sel, np.eye(3)
    elif ctype == 3:                                               # C = H*Delta
        D = rng.random((n4, 3)); F1, F4, Delta = sub @ D, D, D
        H[0], H[3] = sub, np.eye(n4)
    elif ctype == 4:                                               # C = Delta*H
        D = rng.random((n1, 4)); F1, F4, Delta = D, D[:, :3], D
        H[0], H[3] = np.eye(4), sel
    else:                                                          # H*C = Delta*H2
        D = rng.random((n4, 4)); F1, F4, Delta = sub @ D, D[:, :3], sub @ D
        H[0], H[3] = np.eye(n1), sub
        H2 = [None] * 6
        H2[0], H2[3] = np.eye(4), sel
    R1, R4 = F1.shape[1], F4.shape[1]
    A = [F1, rng.standard_normal((3, R1)), rng.random((2, R1))]
    B = [F4, rng.random((3, R4)), rng.standard_normal((2, R4))]
    X1, X2 = full_ktensor(A), full_ktensor(B)
    X1 = X1 + 0.05 * rng.standard_normal(X1.shape)
    X2 = X2 + 0.05 * rng.standard_normal(X2.shape)
    Z = make_Z([X1.shape, X2.shape], [R1, R4], [X1, X2], [NN, None, NN, NN, ('box', 0.0, 2.0), None], weights=[0.3, 1.7],
               lin=[1, 0, 0, 1, 0, 0], ctype=[ctype], H=H, H2=H2, ridge=[0.4, 0.0, 0.1, 0.0, 0.7, 0.0])
    G = noisy_state(Z, off(A + B, rng, 0.05), rng, [Delta + 0.05 * rng.standard_normal(Delta.shape)])
    return Z, G


@pytest.mark.parametrize('ctype', [0, 1, 2, 3, 4, 5])
def test_coupling_terms(pkg, eng, ctype):
    """Gaps through image_f (types 1, 2, 5) and image_d (types 3, 4, 5), kObjImageSq as the denominator of types 1, 2, 5,
    at image sizes on both sides of one split.  The transformation matrices hold 0 and 1 only, so an image is exact and a
    gap sum has no cancellation beyond its own differences."""
    Z, G = coupled_model(np.random.default_rng(50 + ctype), ctype)
    frac, ref = check(pkg, eng, Z, G, 'coupling type %d' % ctype)
    assert ref.f_couplings > 0 and len(ref.coupling_ratios[0]) == 2


# ---- 5. batch flush and overflow ------------------------------------------------------------------------------------------
def test_mid_loop_flush_twelve_constrained_modes(pkg, eng):
    """Three 4-way blocks, every mode with a value-carrying regulariser: 6 tensor tasks and 3 per mode (2 where the value
    is l2's, which has its own kernel) pass kReduceBatchMax - 4 = 36 inside the mode loop, which flushes and goes on."""
    rng = np.random.default_rng(60)
    shapes = [(2500, 3, 2, 2), (7, 5, 4, 3), (6, 700, 3, 2)]
    regs = [('l1 regularization', 0.3), ('ridge', 1.3), ('GL smoothness', 0.9), ('TV regularization', 0.4),
            ('l0 regularization', 0.02), ('l2 regularization', 0.7)]
    data = [block_data(rng, s, 2) for s in shapes]
    Z = make_Z(shapes, [2] * 3, [d[0] for d in data], [regs[i % 6] for i in range(12)], weights=[0.5, 1.0, 2.0],
               ridge=[0.1 * (i % 3) for i in range(12)])
    G = noisy_state(Z, off([a for d in data for a in d[1]], rng), rng)
    check(pkg, eng, Z, G, 'twelve constrained modes')


def twenty_matrices(rng, groups):
    """20 matrices (6, 5) of rank 2 whose first modes hold one factor; `groups`: sizes of the type-0 couplings they share
    it through, in block order"""
    D = rng.random((6, 2))
    facs, objs, lin = [], [], []
    for c, g in enumerate(groups):
        lin += [c + 1, 0] * g
    for p in range(20):
        A = [D, rng.standard_normal((5, 2))]
        objs.append(full_ktensor(A) + 0.05 * rng.standard_normal((6, 5)))
        facs += A
    cons = [NN if m % 2 == 0 else (('l1 regularization', 0.3) if m % 6 == 1 else None) for m in range(40)]
    Z = make_Z([(6, 5)] * 20, [2] * 20, objs, cons, weights=[0.5 + 0.1 * p for p in range(20)], lin=lin,
               ctype=[0] * len(groups), ridge=[0.05 * (m % 4) for m in range(40)])
    G = noisy_state(Z, off(facs, rng, 0.05), rng, [D + 0.05 * rng.standard_normal(D.shape) for _ in groups])
    return Z, G


def test_twenty_coupled_matrices(pkg, eng):
    """20 matrices (6, 5) of rank 2 sharing their first mode through type-0 couplings: 40 tensor tasks fill a batch
    before the first mode adds its own.  (Before a full batch was launched from inside the tensor loop this evaluation
    could not be enqueued: reduce_batch refused it with "too many tasks".)  The library takes at most 8 modes in one
    coupling (test_one_coupling_takes_eight_modes), so the 20 first modes share the factor through three couplings of
    8, 8 and 4 members: 20 gap ratios, and the mean over three couplings."""
    Z, G = twenty_matrices(np.random.default_rng(61), (8, 8, 4))
    _, ref = check(pkg, eng, Z, G, 'twenty coupled matrices')
    assert [len(g) for g in ref.coupling_ratios] == [8, 8, 4] and ref.f_couplings > 0


def test_one_coupling_takes_eight_modes(pkg, eng):
    """The same 20 matrices in ONE coupling are refused when the model is described (a stated limit of the coupled
    kernels' argument records), before anything is evaluated."""
    Z, G = twenty_matrices(np.random.default_rng(61), (20,))
    with pytest.raises(pkg.AoadmmError, match='more than 8 modes in one coupling'):
        pkg.build_model(eng, Z, 'f64')


# ---- 6. later evaluations (first == false) --------------------------------------------------------------------------------
def later_model(rng, kind):
    """Noise-free rank-2 data, long mode 4097 (2 * 4097 = 8194: 5 pieces), the state the generating factors plus 1e-3:
    f_tensors is small next to ||X||^2, so the shortcut ||X||^2 - 2 <mttkrp, fac> + <had, gram> cancels for real.
    Under coupling type 1 the library takes modes of at most 4096 rows and forms H'H of such a mode on the host in
    rows(H) * rows^2 / 2 steps when the model is described (8 s at 4095 rows), so there the long mode has 2501 rows
    (5002 elements: 3 pieces of 1668, the last one short) and its partner every second row of it, 1251.  A non-negative
    or l1 mode whose iterates stay positive ends with Z = fac exactly (the dual settles at the shift), so one mode of
    every model carries GL smoothness, whose prox keeps moving it."""
    R = 2
    pos = lambda *s: rng.random(s) + 0.1
    H = None
    if kind == 'regularised':
        A = [pos(4097, R), pos(5, R), pos(4, R)]
        shapes, cons, lin, ctype, Delta = [(4097, 5, 4)], [('GL smoothness', 1e-3), NN, None], None, [], []
    else:
        n4 = 4097 if kind == 'type0' else 2501
        D = pos(n4, R)
        if kind == 'type0':
            F1 = D; Delta = [D.copy()]
        else:                                                      # type 1: H*C = Delta, every second row of the longer mode
            n1 = 1251
            sub = np.zeros((n1, n4))
            sub[np.arange(n1), 2 * np.arange(n1)] = 1.0
            F1 = sub @ D; Delta = [F1.copy()]
            H = [np.eye(n1), None, None, sub, None, None]
        A = [F1, pos(5, R), pos(4, R), D, pos(4, R), pos(3, R)]
        shapes = [(F1.shape[0], 5, 4), (n4, 4, 3)]
        cons, lin, ctype = [NN, None, ('GL smoothness', 1e-3), NN, None, None], [1, 0, 0, 1, 0, 0], [0 if kind == 'type0' else 1]
    objs = [full_ktensor(A[:3])] + ([full_ktensor(A[3:])] if len(A) > 3 else [])
    Z = make_Z(shapes, [R] * len(shapes), objs, cons, weights=[1.0] if len(shapes) == 1 else [0.3, 1.7], lin=lin,
               ctype=ctype, H=H)
    small = lambda shape: 1e-3 * rng.standard_normal(shape)
    G = noisy_state(Z, [a + small(a.shape) for a in A], rng, [d + small(d.shape) for d in Delta], s=1e-3)
    return Z, G


@pytest.mark.parametrize('kind', ['regularised', 'type0', 'type1'])
def test_later_evaluations(pkg, eng, kind):
    """After MaxOuterIters = 2, MaxInnerIters = 3 the last element of each trace is the evaluation (through last_mttkrp /
    last_had of the mode updated last) of the state download_state returns; the reference takes the direct residual."""
    Z, G = later_model(np.random.default_rng(70), kind)
    pkg.build_model(eng, Z, 'f64')
    pkg.upload_state(eng, Z, G)
    out = pkg.run_solver(eng, options(MaxOuterIters=2, MaxInnerIters=3), len(Z['size']))
    assert out['OuterIterations'] == 2 and len(out['func_val_conv']) == 3
    G2 = pkg.download_state(eng, Z, G)
    ref = objective_ref.evaluate(Z, G2)
    tensors = sum(float(t[1]) for t in ref.terms if t[0].startswith('tensor'))
    normsq = sum(w * float(np.sum(X * X)) for w, X in zip(Z['weights'], Z['object']))
    assert 0 < tensors < 1e-3 * normsq                          # the cancellation is real
    assert ref.f_constraints > 0 and (ref.f_couplings > 0) == (kind != 'regularised')
    dev = (out['func_val_conv'][-1], out['func_coupl_conv'][-1], out['func_constr_conv'][-1])
    compare(dev, ref, ref.bounds(REL64), 'later evaluation, %s' % kind)


# ---- 7. exact integers --------------------------------------------------------------------------------------------------------
EXACT = ([(('TV regularization', 0.5), r, R) for r, R in [(1, 3), (2, 3), (33, 64), (683, 3), (2500, 3), (4097, 20), (131073, 1)]] +
         [((name, 0.25), 2500, 3) for name in ('l1 regularization', 'l0 regularization', 'ridge', 'GL smoothness')] +
         [(('quadratic regularization', 0.5), 1100, 3)])


@pytest.mark.parametrize('reg,rows,R', EXACT, ids=['%s-%dx%d' % (c[0].split()[0], r, R) for c, r, R in EXACT])
def test_exact_integers(pkg, eng, reg, rows, R):
    """Factors, data, Z and Delta are integers in -2..2, weights, eta and ridge powers of two: every product and every sum
    is an integer multiple of 1/4 far below 2^53 (the largest, ||M||^2 of 131073 x 3 x 2 entries of at most 8 R, stays
    under 2^41), so f_tensors with its regulariser and ridge parts is exact in any summation order and must EQUAL the
    reference.  TV is also held to eta sum_r (x[-1, r] - x[0, r]), which the telescoping sum equals exactly: a dropped or
    doubled boundary difference changes it.  The model has one constrained mode and one coupling whose two members hold
    the same factor, so f_constraints is one ratio and f_couplings twice one ratio: within 2 ulp of the reference (two
    square roots and a division, each rounded once, and the reference's own rounding to fp64)."""
    rng = np.random.default_rng(rows + R)
    ints = lambda *s: rng.integers(-2, 3, s).astype(np.float64)
    F = ints(rows, R)
    F[0, 0] = 2.0
    A = [F, ints(3, R), ints(2, R), F.copy(), ints(3, R)]
    cz, Delta = ints(rows, R), ints(rows, R)
    cz[0, 0], Delta[0, 0] = -1.0, 1.0                              # neither gap is zero
    if reg[0] == 'quadratic regularization':
        reg = reg + (ints(rows, rows),)
    Z = make_Z([(rows, 3, 2), (rows, 3)], [R, R], [ints(rows, 3, 2), ints(rows, 3)], [reg, None, None, None, None],
               weights=[1.0, 0.5], lin=[1, 0, 0, 1, 0], ctype=[0], ridge=[0.5, 0.0, 2.0, 0.25, 0.0])
    G = dict(fac=A, constraint_fac=[cz, None, None, None, None], coupling_fac=[Delta],
             constraint_dual_fac=[ints(rows, R), None, None, None, None],
             coupling_dual_fac=[ints(rows, R), None, None, ints(rows, R), None])
    ref = objective_ref.evaluate(Z, G)
    dev = device_eval(pkg, eng, Z, G)
    print('exact %s %dx%d: device %s reference %s' % (reg[0], rows, R, dev, ref.f))
    assert dev[0] == ref.f_tensors
    if reg[0] == 'TV regularization':
        tel = reg[1] * float(np.sum(F[-1] - F[0]))
        assert float(ref.term('reg 0')[0][1]) == tel
        rest = sum(float(t[1]) for t in ref.terms if t[0] != 'reg 0')
        assert dev[0] == rest + tel
    assert ref.f_couplings > 0 and ref.f_constraints > 0
    assert abs(dev[1] - ref.f_couplings) <= 2 * np.spacing(ref.f_couplings)
    assert abs(dev[2] - ref.f_constraints) <= 2 * np.spacing(ref.f_constraints)
