"""CPU: tests/objective_ref.py, the reference tests/test_gpu_objective.py holds the device's objective evaluation to, is
the oracle's func_eval.  The oracle evaluates the state it is given once before its first iteration
(`MaxOuterIters=0`: element 0 of the three traces); both compute in at least fp64 from the same numbers, so they agree to
rtol 1e-11 whatever the summation order."""
import copy

import numpy as np
import pytest

import objective_ref
from helpers import cp_cp_exact_model, cp_model, options, script3_model, transformed_coupling_model
from oracle import aoadmm as OA

RTOL = 1e-11
NN = ('non-negativity',)


def init(Z, io, seed, Delta=None):
    return OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, Delta=Delta, rng=np.random.default_rng(seed))


def oracle_eval(Z, G):
    out = OA.cmtf_AOADMM(Z, alg_options=options(MaxOuterIters=0), init=copy.deepcopy(G))[3]
    return out['func_val_conv'][0], out['func_coupl_conv'][0], out['func_constr_conv'][0]


def check(Z, G, nonzero=(True, True, True)):
    ref = objective_ref.evaluate(Z, G)
    want = oracle_eval(Z, G)
    print('objective_ref %s  oracle %s' % (ref.f, want))
    for got, w, nz in zip(ref.f, want, nonzero):
        assert (w != 0) == nz
        assert abs(got - w) <= RTOL * abs(w), (ref.f, want)
    return ref


def _quad_L(n, rng, symmetric):
    B = rng.standard_normal((n, n))
    return B @ B.T / n if symmetric else B / np.sqrt(n) + np.eye(n)


def test_script3_partial_coupling_type4():
    Z, io = script3_model(np.random.default_rng(1))
    check(Z, init(Z, io, 2))


def test_exact_coupling_type0_with_ridge():
    Z, io = cp_cp_exact_model(np.random.default_rng(3))
    G = init(Z, io, 4)
    check(Z, G)
    Z['ridge'] = [0.3, 0.0, 0.05, 0.0, 1.5, 0.2]
    ref = check(Z, G)
    assert len(ref.term('ridge 4')) == 1 and ref.term('ridge 1')[0][1] == 0


@pytest.mark.parametrize('ctype', [1, 2, 3, 5])
def test_transformed_couplings(ctype):
    Z, io = transformed_coupling_model(np.random.default_rng(10 + ctype), ctype)
    check(Z, init(Z, io, 20 + ctype, Delta=[np.zeros((25, 4))] if ctype == 5 else None))


REGS = [('l1 regularization', 0.3), ('l0 regularization', 0.02), ('l2 regularization', 0.7), ('ridge', 1.3),
        ('GL smoothness', 0.9), ('TV regularization', 0.4), ('quadratic regularization', 0.6, 'sym'),
        ('quadratic regularization', 0.6, 'nonsym')]


@pytest.mark.parametrize('reg', REGS, ids=[' '.join(str(v) for v in r) for r in REGS])
def test_regulariser_values(reg):
    rng = np.random.default_rng(40)
    dims, R = (23, 7, 5), 3
    if reg[0] == 'quadratic regularization':
        reg = (reg[0], reg[1], _quad_L(dims[0], rng, reg[2] == 'sym'))
    Z, io, _ = cp_model(dims, R, rng, [reg, NN, None])
    G = init(Z, io, 41)
    G['fac'][0] = rng.standard_normal((dims[0], R))                 # signed, so TV and l1 differ; some exact zeros for l0
    G['fac'][0][::4, 1] = 0.0
    G['fac'][0][3, 2] = -0.0
    ref = check(Z, G, nonzero=(True, False, True))
    (name, value, mag), = ref.term('reg 0')
    assert mag >= abs(value) > 0
    if reg[0] == 'l0 regularization':
        assert float(value) == reg[1] * (dims[0] * R - 6 - 1)
    if reg[0] == 'TV regularization':                             # the telescoping sum
        assert abs(float(value) - reg[1] * float(np.sum(G['fac'][0][-1] - G['fac'][0][0]))) < 1e-13 * float(mag)


def test_bounds_scale_with_the_magnitudes():
    """bounds(rel): rel * S on f_tensors; a ratio moved by rel in numerator and denominator stays inside its bound and one
    moved by 3 rel does not."""
    Z, io = cp_cp_exact_model(np.random.default_rng(5))
    G = init(Z, io, 6)
    ref = objective_ref.evaluate(Z, G)
    rel = 1e-9
    bt, bc, bz = ref.bounds(rel)
    assert bt == rel * ref.mag_tensors and ref.mag_tensors > ref.f_tensors > 0
    for groups, f, b in ((ref.coupling_ratios, ref.f_couplings, bc), ([[ab] for ab in ref.constraint_ratios], ref.f_constraints, bz)):
        moved = [[(a * (1 + rel), c * (1 - rel)) for a, c in g] for g in groups]
        assert 0 < abs(float(ref._mean_of_ratio_sums(moved)) - f) <= b
        moved = [[(a * (1 + 3 * rel), c * (1 - 3 * rel)) for a, c in g] for g in groups]
        assert abs(float(ref._mean_of_ratio_sums(moved)) - f) > b
