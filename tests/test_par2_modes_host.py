"""CPU: tests/par2_modes_ref.py is the oracle's mode A, mode C and objective of a PARAFAC2 block.

From an oracle state G1 (one outer iteration behind a random start) the oracle runs one more outer iteration to G2; the
restatement, fed with G1 and with the A and B_k factors of G2 where the oracle has already updated them, must give the
oracle's own numbers at 1e-12 relative: the A-mode MTTKRP and system (the arguments the oracle hands to its solver,
recorded through its module-level helpers), the C factor with constraint_fac and constraint_dual_fac, and the terms of
func_val of that iteration.  On the coupled model the C mode is updated by ADMM_coupled; with MaxInnerIters = 1 that is
one row solve against the systems of c_coupled with the coupling target in the bracket (:640-643), then update_constraint.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import helpers
import par2_modes_ref as REF
from oracle import aoadmm as OA

TOL = 1e-12


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) <= TOL * np.linalg.norm(b)


class Recorder:
    """Arguments of the oracle's _mrdivide / _chol_lower / _solve_llt_right, in call order."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ('_mrdivide', '_chol_lower', '_solve_llt_right'):
            orig = getattr(OA, name)

            def wrapped(*a, _orig=orig, _name=name):
                self.calls.append((_name, [np.array(x, copy=True) for x in a]))
                return _orig(*a)
            monkeypatch.setattr(OA, name, wrapped)

    def of(self, name):
        return [a for n, a in self.calls if n == name]


def two_states(Z, io, opt, monkeypatch):
    G0 = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
    _, G1, _, _ = OA.cmtf_AOADMM(Z, opt, init=G0)
    rec = Recorder(monkeypatch)
    _, G2, _, out = OA.cmtf_AOADMM(Z, opt, init=G1)
    return G1, G2, out, rec


def check_objective(Z, p, md, G2, out, extra=0.0):
    """f_tensors of the PARAFAC2 block (:1262-1264 with the weight) and f_PAR2_couplings (:1355) from the pieces."""
    X = Z['object'][p]
    A, B, C = (G2['fac'][m] for m in md)
    Zb = G2['constraint_fac'][md[1]] if Z['constrained_modes'][md[1]] else None
    for ld in (False, True):
        o = REF.objective(X, A, B, C, G2['P'][p], G2['DeltaB'][p], Zb, ld=ld)
        f_t = Z['weights'][p] * float(np.sum(o['res'])) + extra
        assert abs(f_t - out['f_tensors']) <= TOL * abs(out['f_tensors']), (ld, f_t, out['f_tensors'])
        K = len(X)
        f_p = float(np.sum(np.sqrt(o['q'][:, 0].astype(np.float64)) / np.sqrt(o['q'][:, 1].astype(np.float64)))) / K
        assert abs(f_p - out['f_PAR2_couplings']) <= TOL * abs(out['f_PAR2_couplings']), (ld, f_p)
    return o


def test_script4_model_one_outer_iteration(monkeypatch):
    rng = np.random.default_rng(3)
    Z, io = helpers.script4_model(rng, K=7, constraints_B=('non-negativity',))
    opt = helpers.options(MaxOuterIters=1)
    G1, G2, out, rec = two_states(Z, io, opt, monkeypatch)
    X, w = Z['object'][0], Z['weights'][0]
    # mode A (:160-178): unconstrained, the oracle solves A / B with A = w * MTTKRP, B = w * C
    ma = REF.mode_a(X, G1['fac'][1], G1['fac'][2])
    sysA = REF.mode_a_system(ma['Amt'], ma['Csys'], w)
    Aor, Bor = rec.of('_mrdivide')[0]
    assert Aor.shape == ma['Amt'].shape
    assert close(sysA['A'], Aor) and close(sysA['B'], Bor)
    mld = REF.mode_a_sums(ma['T1'], ma['GB'], G1['fac'][2], ld=True)
    assert close(mld['Amt'], ma['Amt']) and close(mld['Csys'], ma['Csys'])
    assert close(OA._mrdivide(sysA['A'], sysA['B']), G2['fac'][0])
    # mode C (:219-248) with the new A and B_k, from C / Z / mu of G1
    A2, B2 = G2['fac'][0], G2['fac'][1]
    cs = REF.c_systems(X, A2, B2, G1['fac'][2], w)
    assert close(REF.c_systems(X, A2, B2, G1['fac'][2], w, ld=True)['a'], cs['a'])
    for solve in ('cho', 'inv'):
        loop = REF.CLoop(cs, Z['constraints'][2], G1['fac'][2], G1['constraint_fac'][2], G1['constraint_dual_fac'][2], solve)
        r = loop.run(opt['MaxInnerIters'], (opt['innerRelPrTol_constr'], opt['innerRelDualTol_constr']))
        assert r['inner_iters'] == out['innerIters'][2, 0]
        tol = TOL if solve == 'cho' else 1e-10
        for got, name in ((r['C'], 'fac'), (r['Z'], 'constraint_fac'), (r['mu'], 'constraint_dual_fac')):
            want = G2[name][2]
            assert np.linalg.norm(got - want) <= tol * np.linalg.norm(want), (solve, name)
    # the K factors the oracle took for the row systems
    Lor = rec.of('_chol_lower')[-len(X):]
    for k in range(len(X)):
        assert close(loop.Bsys[k], Lor[k][0])
    o = check_objective(Z, 0, [0, 1, 2], G2, out)
    fc = np.mean(np.sqrt(o['q'][:, 2].astype(np.float64)) / np.sqrt(o['q'][:, 1].astype(np.float64)))   # :1337 for B_k
    C2 = G2['fac'][2]
    fcC = np.linalg.norm(C2 - G2['constraint_fac'][2]) / np.linalg.norm(C2)
    terms = np.array([fc, fcC])
    assert abs(terms.sum() / np.count_nonzero(terms) - out['f_constraints']) <= TOL * out['f_constraints']   # :1346-1348


def test_script4_model_unconstrained_C_and_reg_values(monkeypatch):
    """C unconstrained: the single solve (:236); B_k under ridge regularisation: its reg_func value enters f_tensors."""
    rng = np.random.default_rng(4)
    Z, io = helpers.script4_model(rng, K=5, constraints_B=('ridge', 0.01))
    Z['constrained_modes'][2] = 0
    Z['constraints'][2] = None
    opt = helpers.options(MaxOuterIters=1, bsum=1, bsum_weight=0.3)
    G1, G2, out, rec = two_states(Z, io, opt, monkeypatch)
    X, w = Z['object'][0], Z['weights'][0]
    cs = REF.c_systems(X, G2['fac'][0], G2['fac'][1], G1['fac'][2], w, bsum_half=opt['bsum_weight'] / 2)
    assert close(REF.CLoop(cs, None, G1['fac'][2], None, None).single(), G2['fac'][2])
    regs = REF.objective(X, G2['fac'][0], G2['fac'][1], G2['fac'][2], G2['P'][0], G2['DeltaB'][0],
                         G2['constraint_fac'][1], reg=Z['constraints'][1])
    regl = REF.objective(X, G2['fac'][0], G2['fac'][1], G2['fac'][2], G2['P'][0], G2['DeltaB'][0],
                         G2['constraint_fac'][1], reg=Z['constraints'][1], ld=True)
    assert close(regl['regv'], regs['regv'])
    check_objective(Z, 0, [0, 1, 2], G2, out, extra=float(np.sum(regs['regv'])))


@pytest.mark.parametrize('ctype,average', [(0, False), (1, False), (1, True)])
def test_par2_C_coupled_model_one_outer_iteration(monkeypatch, ctype, average):
    rng = np.random.default_rng(5)
    Z, io = helpers.par2_C_coupled_model(rng, ctype, noise=0.05, K=8, average=average)
    opt = helpers.options(MaxOuterIters=1, MaxInnerIters=1)
    G1, G2, out, rec = two_states(Z, io, opt, monkeypatch)
    X, w = Z['object'][1], Z['weights'][1]
    K, R = G1['fac'][5].shape
    # mode A of the block (mode 4, constrained): B = w C + rho/2 I goes to _chol_lower, A_inner to _solve_llt_right
    ma = REF.mode_a(X, G1['fac'][4], G1['fac'][5])
    sysA = REF.mode_a_system(ma['Amt'], ma['Csys'], w)
    Bsys = sysA['B'] + sysA['rho'] / 2 * np.eye(R)
    assert any(a[0].shape == Bsys.shape and close(Bsys, a[0]) for a in rec.of('_chol_lower'))
    inner = [a[0] for a in rec.of('_solve_llt_right') if a[0].shape == ma['Amt'].shape]
    want = inner[0] - sysA['rho'] / 2 * (G1['constraint_fac'][3] - G1['constraint_dual_fac'][3])
    assert close(sysA['A'], want)
    # mode C inside the coupling: systems, then the first row step of ADMM_coupled and update_constraint
    A2, B2 = G2['fac'][3], G2['fac'][4]
    cs = REF.c_systems(X, A2, B2, G1['fac'][5], w)
    H = Z['coupling']['coupl_trafo_matrices'][5]
    D, muD = G1['coupling_fac'][0], G1['coupling_dual_fac'][5]
    Zc, muc = G1['constraint_fac'][5], G1['constraint_dual_fac'][5]
    if ctype == 0:
        cc = REF.c_coupled(cs, 1, True)
        Lor = rec.of('_chol_lower')[-K:]
        fac = np.zeros((K, R))
        for k in range(K):
            assert close(cc['L'][k], np.linalg.cholesky(Lor[k][0]))
            rhs = cs['a'][k] + cs['rho'][k] / 2 * (D[k] - muD[k]) + cs['rho'][k] / 2 * (Zc[k] - muc[k])   # :640-643
            fac[k] = sla.cho_solve((cc['L'][k], True), rhs)
    else:
        HtH = H.T @ H
        diag = np.count_nonzero(HtH - np.diag(np.diag(HtH))) == 0
        assert diag == (not average)
        cc = REF.c_coupled(cs, 3 if diag else 4, True, np.diag(HtH).copy() if diag else HtH)
        rc = cc['rho_mean']
        rhs = cs['a'] + rc / 2 * (H.T @ (D - muD)) + rc / 2 * (Zc - muc)                                  # :714-719
        if diag:
            fac = np.stack([sla.cho_solve((cc['L'][k], True), rhs[k]) for k in range(K)])
        else:
            fac = sla.cho_solve((np.linalg.cholesky(cc['M']), True), rhs.ravel()).reshape(K, R)
    assert close(fac, G2['fac'][5])
    prox = Z_prox(Z, 5)
    Znew = prox(fac + muc, cc['rho_max'])
    assert close(Znew, G2['constraint_fac'][5]) and close(muc + fac - Znew, G2['constraint_dual_fac'][5])
    # func_val: the PARAFAC2 block's term next to the CP block's (:1228-1241, through the oracle's own cp_func)
    f_cp = OA.cp_func(Z['object'][0], [G2['fac'][m] for m in (0, 1, 2)], OA.compute_Znorm_const(Z)[0], Z['weights'][0])
    o = REF.objective(X, A2, B2, G2['fac'][5], G2['P'][1], G2['DeltaB'][1])
    f_t = w * float(np.sum(o['res'])) + f_cp
    assert abs(f_t - out['f_tensors']) <= TOL * abs(out['f_tensors'])
    f_p = float(np.sum(np.sqrt(o['q'][:, 0]) / np.sqrt(o['q'][:, 1]))) / K
    assert abs(f_p - out['f_PAR2_couplings']) <= TOL * abs(out['f_PAR2_couplings'])


def Z_prox(Z, m):
    from oracle import prox as OP
    return OP.constraints_to_prox(Z['constrained_modes'], Z['constraints'], Z['size'])[0][m]


def test_floors_of_the_gpu_cases():
    """tests/test_gpu_par2_modes.py takes its bars from the distance of two host evaluations per case: every case stays
    below the cap, and the literal in that file's docstring is the largest of them."""
    import test_gpu_par2_modes as G
    floors = G.all_floors()
    worst = max(floors, key=floors.get)
    print('largest floor %.2e at %s' % (floors[worst], worst))
    assert floors[worst] < G.MAX_FLOOR, worst
    assert floors[worst] <= 1.5 * G.LARGEST_FLOOR and G.LARGEST_FLOOR <= 10 * floors[worst], (worst, floors[worst])
