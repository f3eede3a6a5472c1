"""CPU: the numpy coupled loop the GPU tests compare against (coupled_ref.RefCoupled, 'reference' solve mode) reproduces
oracle.aoadmm's ADMM_coupled for every coupling type.

One outer iteration of the oracle on a two-block CP model from helpers: the uncoupled modes are updated before the
coupling (cmtf_fun_AOADMM.m:89-93), so their final factors give the coupled modes' MTTKRP A_j and Hadamard product C_j
on the host.  From the same initial state RefCoupled must then leave the oracle's coupled factors, Z, duals and Delta
(1e-12) and, with non-zero tolerances, stop at the oracle's inner iteration.
"""
import copy

import numpy as np
import pytest

from coupled_ref import RefCoupled
from helpers import cp_cp_exact_model, options, rel_fro, script3_model, transformed_coupling_model
from oracle import aoadmm as OA
from oracle import prox as OP
from oracle.tensor_ops import mttkrp


def model_of(ctype, rng):
    if ctype == 0:
        return cp_cp_exact_model(rng) + (None,)
    if ctype == 4:
        return script3_model(rng) + (None,)
    Z, io = transformed_coupling_model(rng, ctype)
    return Z, io, ([np.zeros((25, 4))] if ctype == 5 else None)      # init_coupled_AOADMM_CMTF.m:160-164


def oracle_and_ref(ctype, opt, solve='reference'):
    rng = np.random.default_rng(90 + ctype)
    Z, io, Delta = model_of(ctype, rng)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, Delta=Delta, rng=rng)
    _, Fo, _, oo = OA.cmtf_AOADMM(Z, alg_options=opt, init=copy.deepcopy(G))
    lin = Z['coupling']['lin_coupled_modes']
    cmodes = [m for m, v in enumerate(lin) if v == 1]
    prox_ops, _ = OP.constraints_to_prox(Z['constrained_modes'], Z['constraints'], Z['size'])
    ctm = Z['coupling'].get('coupl_trafo_matrices', [None] * len(lin))
    ctm2 = Z['coupling'].get('coupl_trafo_matrices2', [None] * len(lin))
    modes = []
    for m in cmodes:
        p = next(q for q, md in enumerate(Z['modes']) if m + 1 in md)
        md = [q - 1 for q in Z['modes'][p]]
        U = [Fo['fac'][q] for q in md]                    # the other modes of the block: their final = updated factors
        pos = md.index(m)
        C = np.ones((U[0].shape[1],) * 2)
        for i, u in enumerate(U):
            if i != pos:
                C = C * (u.T @ u)                                                  # :98-103
        w = Z['weights'][p]
        con = bool(Z['constrained_modes'][m])
        modes.append(dict(A=w * mttkrp(Z['object'][p], U, pos), C=C, w=w, fac=G['fac'][m], muD=G['coupling_dual_fac'][m],
                          Z=G['constraint_fac'][m] if con else None, mu=G['constraint_dual_fac'][m] if con else None,
                          prox=prox_ops[m] if con else None, H=ctm[m], H2=ctm2[m]))
    ref = RefCoupled(ctype, modes, G['coupling_fac'][0], solve)
    return Fo, oo, cmodes, ref


@pytest.mark.parametrize('ctype', range(6))
def test_numpy_loop_reproduces_the_oracle(ctype):
    opt = options(MaxOuterIters=1, MaxInnerIters=5)
    Fo, oo, cmodes, ref = oracle_and_ref(ctype, opt)
    out = ref.run(5)
    assert out['inner_iters'] == 5 and all(oo['innerIters'][m][0] == 5 for m in cmodes)
    assert rel_fro(out['Delta'], Fo['coupling_fac'][0]) < 1e-12
    for j, m in enumerate(cmodes):
        assert rel_fro(out['fac'][j], Fo['fac'][m]) < 1e-12, (m, 'fac')
        assert rel_fro(out['muD'][j], Fo['coupling_dual_fac'][m]) < 1e-12, (m, 'coupling_dual_fac')
        if out['Z'][j] is not None:
            assert rel_fro(out['Z'][j], Fo['constraint_fac'][m]) < 1e-12, (m, 'constraint_fac')
            assert rel_fro(out['mu'][j], Fo['constraint_dual_fac'][m]) < 1e-12, (m, 'constraint_dual_fac')


@pytest.mark.parametrize('ctype', range(6))
def test_device_formulation_stays_close_on_these_models(ctype):
    """The second host formulation (explicit inverses, Sylvester solve in the eigenbases) is the same loop."""
    opt = options(MaxOuterIters=1, MaxInnerIters=5)
    Fo, _, cmodes, ref = oracle_and_ref(ctype, opt, 'device')
    out = ref.run(5)
    assert rel_fro(out['Delta'], Fo['coupling_fac'][0]) < 1e-10
    for j, m in enumerate(cmodes):
        assert rel_fro(out['fac'][j], Fo['fac'][m]) < 1e-10


def test_numpy_loop_stops_where_the_oracle_stops():
    """Non-zero tolerances (those of test_coupled_loop_early_exit_matches): the same inner iteration count, and the
    state of that iteration."""
    tol = dict(innerRelPrTol_coupl=1e-2, innerRelDualTol_coupl=1e-2, innerRelPrTol_constr=1e-2, innerRelDualTol_constr=1e-2)
    seen = set()
    for ctype in (0, 4, 1):
        opt = options(MaxOuterIters=1, MaxInnerIters=40, **tol)
        Fo, oo, cmodes, ref = oracle_and_ref(ctype, opt)
        out = ref.run(40, (1e-2,) * 4)
        assert out['inner_iters'] == oo['innerIters'][cmodes[0]][0], ctype
        assert rel_fro(out['fac'][0], Fo['fac'][cmodes[0]]) < 1e-12
        seen.add(out['inner_iters'])
    assert any(1 < k < 40 for k in seen), 'no model left its loop early: the case checks nothing'
