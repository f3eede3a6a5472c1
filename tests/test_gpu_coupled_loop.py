"""GPU: every form of the coupled ADMM inner loop (cmtf_fun_AOADMM.m:625-1075), run as the solver runs it
(`Engine.coupled_loop` -> aoadmm_op_coupled_loop: the solver's own system build, couple_path(), coupled_admm and Gram
matrices on a model declared through aoadmm_model_*), against the numpy fp64 loop coupled_ref.RefCoupled, which
tests/test_coupled_ref_host.py pins to the oracle on the CPU.

The model of a case: one two-mode CP block per coupled mode (the coupled mode and a one-row filler mode of the same
rank), one coupling; no tensor data.  Inputs: A standard normal; fac, Z, mu, mu_Delta, Delta uniform; C = F'F with F
uniform 400 x R (rho ~ 133); transformation matrices with singular values in [0.5, 2].  Where Delta has more columns than
a mode has components (type 4 with q > R_j), AA = sum rho_j H_j H_j' is positive definite only if the ranks add up to
q, and mu_Delta is more than rounding noise only if they add up to more (else C_j = Delta*H_j is solved exactly in every
iteration): q = 7 runs with three modes of rank 3, q = 16 with modes of rank 3 and 16.  One coupled mode of type 0
(regs-t0-n1-*) is that degenerate case by nature, Delta = fac + mu_Delta, so fac - Delta and the new mu_Delta are
rounding noise: there mu_Delta and the primal coupling residual must come back below 1e-13, and the noise itself (slots 4
and 5, the two coupling residuals) is not compared.

Every case asserts: path[0] (the form) and path[1] (rank class of the row kernels), so that a retuned dispatch says
"pick a new shape"; inner_iters; fac, Z, mu, mu_Delta of every mode and Delta against the bar below; the four residual
means and every residual slot (rtol 1e-9); rho_j (1e-14); gram_j against the host fac'fac of the returned fac (1e-13);
Z and mu of an unconstrained mode come back bitwise as they went in.  Slots not compared: 0, 2 and 3 of an
unconstrained mode on the RowSteps and Generic forms (nothing writes them there; the one-workgroup kernels write zeros,
which are compared).  Zold, DeltaOld and dDelta are not readable through aoadmm_state_get; they are checked through
what is computed from them in the last iteration: slots 3 and 6 and the two dual residuals.

Bar: the device multiplies by explicit inverses / works in eigenbases where the reference solves with triangular
factors, `sylvester` and mrdivide.  RefCoupled has both formulations; per case floor = the largest relative Frobenius
distance between the two host results, bar = max(1e-11, 10 x floor) -- 10 for a different summation order over at most
64 terms -- and floor <= 1e-10 is asserted (a condition on the inputs).  The bar is never taken from the device.
LARGEST_FLOOR below is the largest floor over the file.

Early exit: k* comes from the reference history at tolerance 0: an iteration in 2..9 whose deciding residual lies below
0.8 x every earlier value; the tolerance is the geometric mean of the two, so the decision sits >= 10 % from the
threshold at every iteration (asserted, never skipped).  The other three tolerances are inf (exit-<residual>-*) or all
four are finite (exit-all-*).  The device must stop at exactly k* and leave the state of k*.

Class -> case (ids as pytest prints them):
  couple_loop_wg_regs_k<4,NM,T4>   regs-t0-n1-*, regs-t0-n2-64x1 / 65x3 / 255x4 / 256x4, regs-t0-n3-63x3, regs-t4-n2-64x3q4,
                                   regs-t4-n3-65x3q2 (q < R), regs-t4-n1-1x4q3
  couple_loop_wg_regs_k<8,NM,T4>   regs-t0-n2-256x5 / 1x8, regs-t0-n3-255x8, regs-t4-n3-64x3q7 (class set by q),
                                   regs-t4-n2-63x(5,8)q6 (unequal ranks), regs-t4-n1-65x8q5
  fusable proxes (regs)            regs-prox-<constraint>; mixed / no constraints: regs-mixed-*, regs-nocon-* (nz = 0)
  couple_loop_wg_k<4|8|16>         wg-t0-n2-257x4 / 257x8 (rows 256|257), wg-t0-n2-64x9 (rmax 8|9), wg-t0-n4-64x3 (n 3|4),
                                   wg-t0-n2-511x3 / 512x5 / 513x9 / 2048x3, wg-t4-n3-300x16q16, wg-t4-n2-64x(3,16)q16,
                                   wg-t4-n4-300x(2,5,9,3)q6 (unequal ranks), wg-mixed-*, wg-nocon-*
  RowSteps                         rows-t0-n2-2049x3 / 2500x7 / 2500x12 (classes 4, 8, 16), rows-t4-n2-2049x(4,3)q4,
                                   rows-<non-fusable prox>-65 (l2-ball, unimodality, TV, GL smoothness, orthonormal),
                                   rows-t0-n5-64x3, rows-t4-n8-64x2q5, rows-t0-n2-70001x3 (grid stride, block partials)
  Generic                          gen-t1 / t2 / t3 / t5 (+ -nocon, -mixed), gen-t5-n3 (stale rho of :1032 is the third
                                   mode's), gen-t0-n2-64x17 (rmax 16|17: wg-t0-n2-64x16) / 130x17 (image > 2048) / 64x32,
                                   gen-t4-n2-64x(17,9)q17, gen-t4-n2-40x(32,20)q32
  thresholds                       the other side of each threshold runs beside it with the form it must take: wg-t0-n2-256x8,
                                   wg-t0-n2-64x8, wg-t0-n3-64x3 (registers), rows-t0-n2-2048x3b, rows-t0-n4-64x3b (LDS),
                                   wg-t0-n2-64x16 and gen-t4-n2-64x(16,9)q16 (LDS, rmax 16|17)
  early exit                       exit-<prc|prz|duc|duz|all>-<case>
  degenerate                       zero-*, ident-* (mu_Delta = 0 throughout), inner1-*, notpd-*, exact-* (bitwise)
  re-entry                         twice-*
"""
import collections
import functools
import importlib
import itertools
import zlib

import numpy as np
import pytest

from coupled_ref import RefCoupled
from helpers import rel_fro
from oracle import prox as OP

pytestmark = pytest.mark.gpu

REGS, WG, ROWSTEPS, GENERIC = range(4)                # AOADMM_CPATH_* (include/aoadmm_hip.h)
PATH_NAME = ['registers one-workgroup', 'LDS one-workgroup', 'row kernels per step', 'generic']

# Largest distance between the two host formulations over every case of this file (host only, no device involved):
# coupling type 5, whose Sylvester solve the reference does by Schur forms and the device in two eigenbases.  Every case
# therefore runs at the 1e-11 bar.
LARGEST_FLOOR = (1.1e-14, 'gen-t5-nocon')

CONSTRAINTS = {
    'non-negativity': ('non-negativity',),
    'box': ('box', 0.1, 0.6),
    'l1 regularization': ('l1 regularization', 20.0),
    'l0 regularization': ('l0 regularization', 5.0),
    'ridge': ('ridge', 30.0),
    'simplex row-wise': ('simplex row-wise', 1.0),
    'l2-ball': ('l2-ball', 1.0),
    'unimodality': ('unimodality', True),
    'TV regularization': ('TV regularization', 5.0),
    'GL smoothness': ('GL smoothness', 50.0),
    'orthonormal': ('orthonormal',),
    'wide box': ('box', -1e6, 1e6),
}
FUSABLE = ['non-negativity', 'box', 'l1 regularization', 'l0 regularization', 'ridge', 'simplex row-wise']
NON_FUSABLE = ['l2-ball', 'unimodality', 'TV regularization', 'GL smoothness', 'orthonormal']
# Seed changes: l0, simplex and unimodality are discontinuous; a seed changes only when the two host runs disagree
# (floor assertion).  id -> bump.
SEED_BUMP = {}

NN = 'non-negativity'
Spec = collections.namedtuple('Spec', 'id ctype rows ranks cons q drows kind')
SPECS = {}


def spec(id, ctype, rows, ranks, cons=None, q=None, drows=None, kind='random'):
    """rows: one row count (types 0, 2, 4: shared) or one per mode (types 1, 3, 5, with drows = rows of Delta); ranks:
    one rank or one per mode; cons: constraint names per mode (None = unconstrained), default non-negativity on all."""
    n = len(ranks) if isinstance(ranks, tuple) else len(rows) if isinstance(rows, tuple) else len(cons)
    ranks = ranks if isinstance(ranks, tuple) else (ranks,) * n
    rows = rows if isinstance(rows, tuple) else (rows,) * n
    cons = tuple(cons) if cons is not None else (NN,) * n
    assert len(ranks) == len(rows) == len(cons) == n and id not in SPECS
    SPECS[id] = Spec(id, ctype, rows, ranks, cons, q, drows, kind)
    return id


def _orth(rng, r, k):
    return np.linalg.qr(rng.standard_normal((r, k)))[0]


def _trafo(rng, r, c):
    """r x c with singular values in [0.5, 2]"""
    k = min(r, c)
    return (_orth(rng, r, k) * rng.uniform(0.5, 2.0, k)) @ _orth(rng, c, k).T


@functools.lru_cache(maxsize=None)
def inputs(sid):
    """-> (modes for RefCoupled, Delta); computed once, shared, never modified."""
    s = SPECS[sid]
    rng = np.random.default_rng(zlib.crc32(sid.encode()) + SEED_BUMP.get(sid, 0))
    n, t = len(s.ranks), s.ctype
    drows = s.drows if t in (1, 3, 5) else s.rows[0]
    dcols = s.q if t in (2, 4, 5) else s.ranks[0]
    modes = []
    for j in range(n):
        rows, R = s.rows[j], s.ranks[j]
        md = dict(H=None, H2=None)
        if t in (1, 5):
            md['H'] = _trafo(rng, drows, rows)
        elif t == 2:
            md['H'] = _trafo(rng, R, dcols)
        elif t == 3:
            md['H'] = _trafo(rng, rows, drows)
        elif t == 4:
            md['H'] = _trafo(rng, dcols, R)
        if t == 5:
            md['H2'] = _trafo(rng, dcols, R)
        img = (drows, R) if t in (1, 5) else (rows, dcols) if t == 2 else (rows, R)
        F = rng.random((400, R))
        md.update(C=F.T @ F, A=rng.standard_normal((rows, R)), fac=rng.random((rows, R)), muD=rng.random(img),
                  Z=rng.random((rows, R)), mu=rng.random((rows, R)), name=s.cons[j], prox=None)
        if s.cons[j] is not None:
            md['prox'] = OP.constraints_to_prox([1], [CONSTRAINTS[s.cons[j]]], [rows])[0][0]
        modes.append(md)
    Delta = rng.random((drows, dcols))
    if s.kind == 'zero':                              # everything 0: fac = Delta = 0, the primal residuals are 0/0
        for md in modes:
            for k in ('A', 'fac', 'muD', 'Z', 'mu'):
                md[k] = np.zeros_like(md[k])
        Delta = np.zeros_like(Delta)
    elif s.kind == 'ident':                           # identical modes, mu_Delta = 0, rho = 128 exactly: Delta = fac bitwise
        for md in modes:
            R = md['C'].shape[0]
            md.update({k: modes[0][k] for k in ('A', 'fac', 'Z', 'mu')})
            md['C'] = 127.0 * np.eye(R) + np.ones((R, R))
            md['muD'] = np.zeros_like(md['muD'])
    elif s.kind == 'exact':                           # small integers, C = 2 I: rho = 2, B = 4 I, L = 2 I, coef = 1/2
        for md in modes:
            R = md['C'].shape[0]
            md['C'] = 2.0 * np.eye(R)
            for k in ('A', 'fac', 'muD', 'Z', 'mu'):
                md[k] = rng.integers(-3, 4, md[k].shape).astype(np.float64)
        Delta = rng.integers(-3, 4, Delta.shape).astype(np.float64)
    elif s.kind == 'notpd':
        modes[-1]['C'] = -modes[-1]['C']
    for md in modes:
        for v in md.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    Delta.setflags(write=False)
    return modes, Delta


@functools.lru_cache(maxsize=None)
def reference(sid):
    """(reference-formulation loop, device-formulation loop) of a case; iterates are kept inside and shared."""
    modes, Delta = inputs(sid)
    return RefCoupled(SPECS[sid].ctype, modes, Delta, 'reference'), RefCoupled(SPECS[sid].ctype, modes, Delta, 'device')


STATE_KEYS = ('fac', 'muD', 'Z', 'mu')


def floor_of(ref, alt, keys=STATE_KEYS):
    f = rel_fro(alt['Delta'], ref['Delta'])
    for k in keys:
        for a, b in zip(alt[k], ref[k]):
            if b is not None:
                f = max(f, rel_fro(a, b))
    return f


def host_pair(sid, max_inner, tol=(0.0,) * 4, start=None):
    loop, loop_dev = reference(sid)
    ref, alt = loop.run(max_inner, tol), loop_dev.run(max_inner, tol)
    assert alt['inner_iters'] == ref['inner_iters'], 'the two host formulations stop at different iterations'
    with np.errstate(invalid='ignore'):
        floor = floor_of(ref, alt, ('fac', 'Z', 'mu') if SPECS[sid].kind == 'single0' else STATE_KEYS)
    if SPECS[sid].kind == 'zero':
        floor = 0.0                                   # 0/0 distances of all-zero states
    assert floor <= 1e-10, ('%s: the two host formulations differ by %.2e: ill-conditioned input or a tie of a '
                            'discontinuous prox; choose other inputs (SEED_BUMP), not a wider bar' % (sid, floor))
    return ref, floor


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
def _mods():
    return importlib.import_module('matlab-code_amd._capi'), importlib.import_module('matlab-code_amd.driver')


def declare(eng, sid):
    """The model of the case on the engine: block j = (coupled mode j, filler mode n + j), coupling 0."""
    import ctypes as C
    capi, _ = _mods()
    pkg = importlib.import_module('matlab-code_amd')
    s = SPECS[sid]
    modes, _ = inputs(sid)
    n, lib = len(s.ranks), eng.lib
    eng._resident_model = None
    capi.check(lib.aoadmm_model_begin(eng.h, 2 * n, n, 1))
    for j in range(n):
        capi.check(lib.aoadmm_model_set_mode(eng.h, j, s.rows[j], s.ranks[j]))
        capi.check(lib.aoadmm_model_set_mode(eng.h, n + j, 1, s.ranks[j]))
    for j in range(n):
        capi.check(lib.aoadmm_model_add_cp(eng.h, j, 2, (C.c_int * 2)(j, n + j), 1.0))
    keep = []
    for j, md in enumerate(modes):
        if md['name'] is not None:
            cid, params, Lmat = pkg.constraint_descriptor(CONSTRAINTS[md['name']])
            capi.check(lib.aoadmm_model_set_constraint(eng.h, j, cid, capi.dptr(params) if params.size else None,
                                                       params.size, None))
        H = capi.as_f(md['H']) if md['H'] is not None else None
        H2 = capi.as_f(md['H2']) if md['H2'] is not None else None
        keep += [H, H2]
        capi.check(lib.aoadmm_model_set_coupling(eng.h, j, 0, capi.dptr(H), H.shape[0] if H is not None else 0,
                                                 H.shape[1] if H is not None else 0, capi.dptr(H2),
                                                 H2.shape[0] if H2 is not None else 0, H2.shape[1] if H2 is not None else 0))
        capi.check(lib.aoadmm_model_set_coupling(eng.h, n + j, -1, None, 0, 0, None, 0, 0))
    capi.check(lib.aoadmm_model_set_coupling_type(eng.h, 0, s.ctype))
    capi.check(lib.aoadmm_model_end(eng.h))


def put_state(eng, state):
    capi, drv = _mods()
    for j in range(len(state['fac'])):
        drv._put(eng, capi.F_FAC, j, 0, state['fac'][j])
        drv._put(eng, capi.F_COUPLING_DUAL, j, 0, state['muD'][j])
        drv._put(eng, capi.F_CONSTRAINT_FAC, j, 0, state['Z'][j])
        drv._put(eng, capi.F_CONSTRAINT_DUAL, j, 0, state['mu'][j])
    drv._put(eng, capi.F_COUPLING_FAC, 0, 0, state['Delta'])


def get_state(eng, like):
    capi, drv = _mods()
    out = dict(fac=[], muD=[], Z=[], mu=[])
    for j in range(len(like['fac'])):
        out['fac'].append(drv._get(eng, capi.F_FAC, j, 0, like['fac'][j].shape))
        out['muD'].append(drv._get(eng, capi.F_COUPLING_DUAL, j, 0, like['muD'][j].shape))
        out['Z'].append(drv._get(eng, capi.F_CONSTRAINT_FAC, j, 0, like['Z'][j].shape))
        out['mu'].append(drv._get(eng, capi.F_CONSTRAINT_DUAL, j, 0, like['mu'][j].shape))
    out['Delta'] = drv._get(eng, capi.F_COUPLING_FAC, 0, 0, like['Delta'].shape)
    return out


def start_state(sid):
    modes, Delta = inputs(sid)
    return dict(fac=[m['fac'] for m in modes], muD=[m['muD'] for m in modes], Z=[m['Z'] for m in modes],
                mu=[m['mu'] for m in modes], Delta=Delta)


def _close(dev, ref, rtol=1e-9):
    if np.isnan(ref):
        return bool(np.isnan(dev))
    return abs(dev - ref) <= rtol * abs(ref)


WORST = dict(err=0.0, bar=1.0, case='')               # largest device error / bar seen in this session (printed per case)


def compare(sid, out, dev, ref, floor, path, start):
    s = SPECS[sid]
    modes, _ = inputs(sid)
    loop, _ = reference(sid)
    bar = max(1e-11, 10 * floor)
    n = len(modes)
    errs = {}
    noise = s.kind == 'single0'                       # mu_Delta is rounding noise: see the module docstring
    if noise:
        assert np.abs(dev['muD'][0]).max() < 1e-13 and np.abs(ref['muD'][0]).max() < 1e-13
        assert out['res'][0] < 1e-13 and ref['res'][0] < 1e-13
    for k in STATE_KEYS:
        for j in range(n):
            if ref[k][j] is not None and not (noise and k == 'muD'):
                errs['%s%d' % (k, j)] = rel_fro(dev[k][j], ref[k][j]) if np.any(ref[k][j]) else float(np.abs(dev[k][j]).max())
    errs['Delta'] = rel_fro(dev['Delta'], ref['Delta']) if np.any(ref['Delta']) else float(np.abs(dev['Delta']).max())
    worst = max(errs, key=errs.get)
    print('%s: path %s its %d/%d floor %.2e bar %.2e worst %s %.2e res %s / %s'
          % (sid, out['path'], out['inner_iters'], ref['inner_iters'], floor, bar, worst, errs[worst],
             ' '.join('%.12e' % v for v in out['res']), ' '.join('%.12e' % v for v in ref['res'])))
    if errs[worst] / bar > WORST['err'] / WORST['bar']:
        WORST.update(err=errs[worst], bar=bar, case=sid)
    assert out['path'][0] == path[0], ('dispatch runs the %s form here, the case is meant for the %s form: pick a new shape'
                                       % (PATH_NAME[out['path'][0]], PATH_NAME[path[0]]))
    assert out['path'][1] == path[1], 'rank class %d, the case is meant for %d: pick a new shape' % (out['path'][1], path[1])
    assert out['inner_iters'] == ref['inner_iters']
    for k, e in errs.items():
        assert e < bar or e == 0.0, (k, e, bar)
    for i in range(4):
        if not (noise and i in (0, 2)):
            assert _close(out['res'][i], ref['res'][i]), ('res', i, out['res'][i], ref['res'][i])
    for j in range(n):
        con = modes[j]['prox'] is not None
        for k in range(8):
            if (not con and k in (0, 2, 3) and path[0] in (ROWSTEPS, GENERIC)) or (noise and k in (4, 5)):
                continue
            assert _close(out['slots'][j, k], ref['slots'][j, k]), ('slot', j, k, out['slots'][j, k], ref['slots'][j, k])
        assert abs(out['rho'][j] - loop.rho[j]) <= 1e-14 * loop.rho[j], ('rho', j)
        G = dev['fac'][j].T @ dev['fac'][j]
        assert np.linalg.norm(out['gram'][j] - G) <= 1e-13 * np.linalg.norm(G) or not G.any(), ('gram', j)
        if not con:
            assert np.array_equal(dev['Z'][j], start['Z'][j]) and np.array_equal(dev['mu'][j], start['mu'][j]), \
                'Z / mu of unconstrained mode %d were written' % j


def run_device(eng, sid, max_inner, tol=(0.0,) * 4):
    modes, _ = inputs(sid)
    return eng.coupled_loop(0, [m['A'] for m in modes], [m['C'] for m in modes], max_inner, tol)


def check_case(eng, sid, path, max_inner=5, tol=(0.0,) * 4, expect_iters=None):
    ref, floor = host_pair(sid, max_inner, tol)
    if expect_iters is not None:
        assert ref['inner_iters'] == expect_iters
    start = start_state(sid)
    declare(eng, sid)
    put_state(eng, start)
    out = run_device(eng, sid, max_inner, tol)
    dev = get_state(eng, start)
    compare(sid, out, dev, ref, floor, path, start)
    return out, dev


# ---------------------------------------------------------------------------------------------------------------------
# the forms, tolerances 0
# ---------------------------------------------------------------------------------------------------------------------
def _params(cases):
    return [pytest.param(sid, path, id=sid) for sid, path in cases]


REGS_CASES = [
    (spec('regs-t0-n1-63x3', 0, 63, (3,), kind='single0'), (REGS, 4)),
    (spec('regs-t0-n1-64x7', 0, 64, (7,), cons=(None,), kind='single0'), (REGS, 8)),
    (spec('regs-t0-n2-64x1', 0, 64, (1, 1)), (REGS, 4)),
    (spec('regs-t0-n2-65x3', 0, 65, (3, 3)), (REGS, 4)),
    (spec('regs-t0-n2-255x4', 0, 255, (4, 4)), (REGS, 4)),
    (spec('regs-t0-n2-256x4', 0, 256, (4, 4)), (REGS, 4)),
    (spec('regs-t0-n3-63x3', 0, 63, (3, 3, 3)), (REGS, 4)),
    (spec('regs-t4-n2-64x3q4', 4, 64, (3, 3), q=4), (REGS, 4)),
    (spec('regs-t4-n3-65x3q2', 4, 65, (3, 3, 3), q=2), (REGS, 4)),
    (spec('regs-t4-n1-1x4q3', 4, 1, (4,), q=3), (REGS, 4)),
    (spec('regs-t0-n2-256x5', 0, 256, (5, 5)), (REGS, 8)),
    (spec('regs-t0-n2-1x8', 0, 1, (8, 8)), (REGS, 8)),
    (spec('regs-t0-n3-255x8', 0, 255, (8, 8, 8)), (REGS, 8)),
    (spec('regs-t4-n3-64x3q7', 4, 64, (3, 3, 3), q=7), (REGS, 8)),
    (spec('regs-t4-n2-63x(5,8)q6', 4, 63, (5, 8), q=6), (REGS, 8)),
    (spec('regs-t4-n1-65x8q5', 4, 65, (8,), q=5), (REGS, 8)),
] + [
    # every fusable prox, types 0 and 4 in turn, both rank classes in turn (no simplex at one column)
    (spec('regs-prox-%s' % c, (0, 4)[i % 2], 65, (4, 4) if i % 2 == 0 else (5, 3), cons=(c, c), q=None if i % 2 == 0 else 5),
     (REGS, 4 if i % 2 == 0 else 8)) for i, c in enumerate(FUSABLE)
] + [
    (spec('regs-mixed-t0-n3-65x3', 0, 65, (3, 3, 3), cons=(NN, None, 'box')), (REGS, 4)),
    (spec('regs-mixed-t4-n2-65x(5,3)q5', 4, 65, (5, 3), cons=(None, 'simplex row-wise'), q=5), (REGS, 8)),
    (spec('regs-nocon-t0-n2-65x3', 0, 65, (3, 3), cons=(None, None)), (REGS, 4)),
    (spec('regs-nocon-t4-n3-65x3q7', 4, 65, (3, 3, 3), cons=(None, None, None), q=7), (REGS, 8)),
]

WG_CASES = [
    (spec('wg-t0-n2-257x4', 0, 257, (4, 4)), (WG, 4)),
    (spec('wg-t0-n2-257x8', 0, 257, (8, 8)), (WG, 8)),
    (spec('wg-t0-n2-256x8', 0, 256, (8, 8)), (REGS, 8)),
    (spec('wg-t0-n2-64x9', 0, 64, (9, 9)), (WG, 16)),
    (spec('wg-t0-n2-64x8', 0, 64, (8, 8)), (REGS, 8)),
    (spec('wg-t0-n4-64x3', 0, 64, (3, 3, 3, 3)), (WG, 4)),
    (spec('wg-t0-n3-64x3', 0, 64, (3, 3, 3)), (REGS, 4)),
    (spec('wg-t0-n2-511x3', 0, 511, (3, 3)), (WG, 4)),
    (spec('wg-t0-n2-512x5', 0, 512, (5, 5), cons=('l1 regularization', 'box')), (WG, 8)),
    (spec('wg-t0-n2-513x9', 0, 513, (9, 9), cons=('simplex row-wise', NN)), (WG, 16)),
    (spec('wg-t0-n2-2048x3', 0, 2048, (3, 3)), (WG, 4)),
    (spec('wg-t0-n2-64x16', 0, 64, (16, 16), cons=('ridge', 'l0 regularization')), (WG, 16)),
    (spec('wg-t4-n3-300x16q16', 4, 300, (16, 16, 16), q=16), (WG, 16)),
    (spec('wg-t4-n2-64x(3,16)q16', 4, 64, (3, 16), q=16), (WG, 16)),
    (spec('wg-t4-n4-300x(2,5,9,3)q6', 4, 300, (2, 5, 9, 3), cons=(NN, 'box', 'simplex row-wise', None), q=6), (WG, 16)),
    (spec('wg-mixed-t4-n2-300x(4,3)q4', 4, 300, (4, 3), cons=(None, NN), q=4), (WG, 4)),
    (spec('wg-nocon-t0-n2-300x7', 0, 300, (7, 7), cons=(None, None)), (WG, 8)),
    (spec('wg-nocon-t4-n2-300x(4,3)q4', 4, 300, (4, 3), cons=(None, None), q=4), (WG, 4)),
]

ROWSTEPS_CASES = [
    (spec('rows-t0-n2-2049x3', 0, 2049, (3, 3)), (ROWSTEPS, 4)),
    (spec('rows-t0-n2-2048x3b', 0, 2048, (3, 3), cons=(NN, 'box')), (WG, 4)),
    (spec('rows-t0-n2-2500x7', 0, 2500, (7, 7), cons=('box', 'l0 regularization')), (ROWSTEPS, 8)),
    (spec('rows-t0-n2-2500x12', 0, 2500, (12, 12), cons=('l1 regularization', None)), (ROWSTEPS, 16)),
    (spec('rows-t4-n2-2049x(4,3)q4', 4, 2049, (4, 3), q=4), (ROWSTEPS, 4)),
    (spec('rows-t4-n2-2500x(7,12)q9', 4, 2500, (7, 12), cons=(NN, 'ridge'), q=9), (ROWSTEPS, 16)),
    (spec('rows-nocon-t0-n2-2049x5', 0, 2049, (5, 5), cons=(None, None)), (ROWSTEPS, 8)),
] + [
    (spec('rows-%s-65' % c, (0, 4)[i % 2], 65, (3, 3) if i % 2 == 0 else (4, 3), cons=(NN, c), q=None if i % 2 == 0 else 4),
     (ROWSTEPS, 4)) for i, c in enumerate(NON_FUSABLE)
] + [
    (spec('rows-t0-n5-64x3', 0, 64, (3,) * 5, cons=(NN, None, 'box', NN, None)), (ROWSTEPS, 4)),
    (spec('rows-t0-n4-64x3b', 0, 64, (3,) * 4, cons=(NN, None, 'box', NN)), (WG, 4)),
    (spec('rows-t4-n8-64x2q5', 4, 64, (2,) * 8, q=5), (ROWSTEPS, 8)),
    (spec('rows-t0-n2-70001x3', 0, 70001, (3, 3), cons=(NN, 'box')), (ROWSTEPS, 4)),
]

GENERIC_CASES = [
    (spec('gen-t1', 1, (25, 50), (3, 3), drows=25), (GENERIC, 0)),
    (spec('gen-t1-nocon', 1, (25, 50), (3, 3), cons=(None, None), drows=25), (GENERIC, 0)),
    (spec('gen-t1-mixed', 1, (40, 25), (5, 5), cons=('box', None), drows=25), (GENERIC, 0)),
    (spec('gen-t2', 2, 24, (4, 3), q=3), (GENERIC, 0)),
    (spec('gen-t2-nocon', 2, 24, (4, 3), cons=(None, None), q=3), (GENERIC, 0)),
    (spec('gen-t2-mixed', 2, 700, (4, 6), cons=(None, 'l2-ball'), q=4), (GENERIC, 0)),
    (spec('gen-t3', 3, (30, 50), (3, 3), drows=25), (GENERIC, 0)),
    (spec('gen-t3-nocon', 3, (30, 50), (3, 3), cons=(None, None), drows=25), (GENERIC, 0)),
    (spec('gen-t3-mixed', 3, (30, 50), (3, 3), cons=('simplex row-wise', None), drows=25), (GENERIC, 0)),
    (spec('gen-t5', 5, (25, 50), (4, 3), q=4, drows=25), (GENERIC, 0)),
    (spec('gen-t5-nocon', 5, (25, 50), (4, 3), cons=(None, None), q=4, drows=25), (GENERIC, 0)),
    (spec('gen-t5-mixed', 5, (25, 50), (4, 3), cons=(None, 'box'), q=4, drows=25), (GENERIC, 0)),
    (spec('gen-t5-n3', 5, (25, 50, 30), (4, 3, 2), cons=(NN, None, 'box'), q=4, drows=25), (GENERIC, 0)),
    (spec('gen-t0-n2-64x17', 0, 64, (17, 17)), (GENERIC, 0)),
    (spec('gen-t0-n2-130x17', 0, 130, (17, 17), cons=('box', None)), (GENERIC, 0)),
    (spec('gen-t0-n2-64x32', 0, 64, (32, 32), cons=(None, 'l1 regularization')), (GENERIC, 0)),
    (spec('gen-t4-n2-64x(17,9)q17', 4, 64, (17, 9), q=17), (GENERIC, 0)),
    (spec('gen-t4-n2-64x(16,9)q16', 4, 64, (16, 9), q=16), (WG, 16)),
    (spec('gen-t4-n2-40x(32,20)q32', 4, 40, (32, 20), cons=(None, NN), q=32), (GENERIC, 0)),
]


@pytest.mark.parametrize('sid,path', _params(REGS_CASES))
def test_registers_one_workgroup_loop(eng, sid, path):
    check_case(eng, sid, path)


@pytest.mark.parametrize('sid,path', _params(WG_CASES))
def test_lds_one_workgroup_loop_and_its_thresholds(eng, sid, path):
    """couple_loop_wg_k and the other side of each of its thresholds: rows 256|257, rmax 8|9, n 3|4."""
    check_case(eng, sid, path)


@pytest.mark.parametrize('sid,path', _params(ROWSTEPS_CASES))
def test_row_kernels_per_step(eng, sid, path):
    """couple_primal_rows / couple_delta_rows / couple_dual_rows + constraint_update + admm_finalize_generic, and the other
    side of rows 2048|2049 and n 4|5."""
    check_case(eng, sid, path)


@pytest.mark.parametrize('sid,path', _params(GENERIC_CASES))
def test_generic_loop(eng, sid, path):
    """Types 1, 2, 3, 5, and types 0 / 4 beyond 16 columns (with the other side of rmax 16|17)."""
    check_case(eng, sid, path)


def test_nine_coupled_modes_are_refused(eng, pkg):
    sid = spec('refuse-n9', 0, 64, (3,) * 9)
    with pytest.raises(pkg.AoadmmError) as ei:
        declare(eng, sid)
    assert 'more than 8 modes' in str(ei.value)


# ---------------------------------------------------------------------------------------------------------------------
# early exit
# ---------------------------------------------------------------------------------------------------------------------
EXIT_INNER = 10
RES_NAME = ['prc', 'prz', 'duc', 'duz']               # order of tol and res


def pick_exit(series):
    """Iterations k in 2..9 (1-based) whose residual is below 0.8 x the smallest earlier one -> [(k, tolerance)]."""
    out = []
    for k in range(2, EXIT_INNER):
        lo = min(series[:k - 1])
        if 0 < series[k - 1] < 0.8 * lo:
            out.append((k, float(np.sqrt(series[k - 1] * lo))))
    return out


def assert_margin(hist, kstar, tol):
    """The loop stops at k*, and at no iteration up to k* does a residual come within 10 % of a finite tolerance."""
    assert 1 < kstar < EXIT_INNER
    for k in range(1, kstar + 1):
        for i in range(4):
            if np.isfinite(tol[i]):
                assert abs(hist[i][k - 1] / tol[i] - 1.0) > 0.1, \
                    '%s %.3e within 10 %% of the tolerance %.3e at iteration %d' % (RES_NAME[i], hist[i][k - 1], tol[i], k)
        assert any(hist[i][k - 1] > tol[i] for i in range(4)) == (k < kstar)


EXIT_SHAPES = {sid: path for sid, path in REGS_CASES + WG_CASES + ROWSTEPS_CASES + GENERIC_CASES}
# (case, deciding residual): found on the CPU from the reference histories; a pair not listed has no iteration in 2..9
# that undercuts every earlier value by 20 %
_ALL4, _COUPL = (0, 1, 2, 3), (0, 2)
EXIT_CASES = [(sid, w) for sid, ws in [
    ('regs-t0-n3-255x8', _ALL4), ('regs-mixed-t4-n2-65x(5,3)q5', _ALL4), ('regs-nocon-t0-n2-65x3', _COUPL),
    ('wg-t0-n2-513x9', _ALL4), ('wg-t4-n4-300x(2,5,9,3)q6', _ALL4), ('wg-nocon-t4-n2-300x(4,3)q4', _COUPL),
    ('rows-t4-n2-2500x(7,12)q9', _ALL4), ('rows-t0-n5-64x3', _ALL4), ('rows-unimodality-65', _ALL4),
    ('rows-nocon-t0-n2-2049x5', _COUPL), ('rows-t0-n2-70001x3', (1, 2)),
    ('gen-t1', _ALL4), ('gen-t2', _ALL4), ('gen-t3-mixed', _ALL4), ('gen-t5-n3', _ALL4), ('gen-t1-nocon', _COUPL),
    ('gen-t0-n2-130x17', _ALL4), ('gen-t4-n2-64x(17,9)q17', _ALL4)] for w in ws]


def exit_case(eng, sid, which):
    loop, _ = reference(sid)
    hist = loop.history(EXIT_INNER)
    picks = pick_exit(hist[which])
    assert picks, '%s no longer has a %s-driven exit iteration in 2..9 with the 0.8 gap: pick another input' % (sid, RES_NAME[which])
    kstar, t = picks[len(picks) // 2]
    tol = [np.inf] * 4
    tol[which] = t
    assert_margin(hist, kstar, tol)
    out, dev = check_case(eng, sid, EXIT_SHAPES[sid], EXIT_INNER, tuple(tol), expect_iters=kstar)
    last = loop.run(EXIT_INNER)                       # the state of iteration k*, not of iteration 10
    assert rel_fro(dev['fac'][0], last['fac'][0]) > 1e-6 or rel_fro(dev['muD'][0], last['muD'][0]) > 1e-6


def _exit_params():
    return [pytest.param(sid, which, id='exit-%s-%s' % (RES_NAME[which], sid)) for sid, which in EXIT_CASES]


@pytest.mark.parametrize('sid,which', _exit_params())
def test_early_exit_one_residual_decides(eng, sid, which):
    exit_case(eng, sid, which)


EXIT_ALL_CASES = ['regs-t0-n3-255x8', 'wg-t4-n4-300x(2,5,9,3)q6', 'rows-t4-n2-2500x(7,12)q9', 'gen-t1', 'gen-t2', 'gen-t3-mixed',
                  'gen-t5-n3', 'gen-t4-n2-64x(17,9)q17']


def all_four_tolerances(hist):
    """One exit tolerance per residual (pick_exit), the first combination in product order whose joint stopping iteration
    keeps every residual >= 10 % from its tolerance at every iteration -> (k*, tol) or None."""
    for combo in itertools.product(*[pick_exit(hist[i]) for i in range(4)]):
        tol = [c[1] for c in combo]
        kstar = min(k for k in range(1, EXIT_INNER + 1) if all(hist[i][k - 1] <= tol[i] for i in range(4)))
        try:
            assert_margin(hist, kstar, tol)
        except AssertionError:
            continue
        return kstar, tol
    return None


@pytest.mark.parametrize('sid', [pytest.param(s, id='exit-all-%s' % s) for s in EXIT_ALL_CASES])
def test_early_exit_all_four_tolerances(eng, sid):
    """All four tolerances finite, each one an exit tolerance of its own residual: the loop ends at the first iteration
    where all four hold."""
    loop, _ = reference(sid)
    hist = loop.history(EXIT_INNER)
    found = all_four_tolerances(hist)
    assert found, '%s: no four tolerances with the 10 %% margin: pick another input' % sid
    kstar, tol = found
    assert_margin(hist, kstar, tol)
    check_case(eng, sid, EXIT_SHAPES[sid], EXIT_INNER, tuple(tol), expect_iters=kstar)


# ---------------------------------------------------------------------------------------------------------------------
# degenerate inputs
# ---------------------------------------------------------------------------------------------------------------------
FORM_SHAPES = [('regs', 65, 3, (REGS, 4)), ('wg', 300, 3, (WG, 4)), ('rows', 2049, 3, (ROWSTEPS, 4)), ('gen', 64, 17, (GENERIC, 0))]


@pytest.mark.parametrize('sid,path', _params([(spec('zero-%s' % f, 0, rows, (R, R), kind='zero'), p) for f, rows, R, p in FORM_SHAPES] +
                                             [(spec('zero-gen-t3', 3, (30, 50), (3, 3), drows=25, kind='zero'), (GENERIC, 0))]))
def test_zero_input_stops_where_the_reference_stops(eng, sid, path):
    """All state and A zero: fac = Delta = 0, both primal residuals are 0/0 = NaN and both dual residuals 0; `NaN > tol`
    is false, so the reference leaves the loop after one iteration whatever the tolerances."""
    out, dev = check_case(eng, sid, path, 5, expect_iters=1)
    assert np.isnan(out['res'][0]) and np.isnan(out['res'][1]) and out['res'][2] == 0.0 and out['res'][3] == 0.0
    assert not dev['Delta'].any() and not any(f.any() for f in dev['fac'])


@pytest.mark.parametrize('sid,path', _params([(spec('ident-%s' % f, 0, rows, (R, R), kind='ident'), p) for f, rows, R, p in FORM_SHAPES]))
def test_zero_coupling_dual_takes_the_unscaled_dual_residual(eng, sid, path):
    """Two modes with identical A, C and state, mu_Delta = 0 and rho = 128: both solves give the same fac, Delta = fac
    bitwise, so mu_Delta stays exactly 0, ||mu_Delta|| = 0 and the dual coupling residual is the unscaled ||dDelta||
    (:1107-1112); the primal coupling residual is exactly 0."""
    out, dev = check_case(eng, sid, path, 5, expect_iters=5)
    assert not any(m.any() for m in dev['muD']) and out['res'][0] == 0.0 and out['res'][2] > 0.0


@pytest.mark.parametrize('sid,path', _params([(spec('inner1-%s' % f, 4 if f != 'gen' else 3, rows if f != 'gen' else (30, 50),
                                                    (R, R), q=R if f != 'gen' else None, drows=25, cons=(NN, None)), p)
                                              for f, rows, R, p in FORM_SHAPES]))
def test_one_inner_iteration(eng, sid, path):
    check_case(eng, sid, path, 1, expect_iters=1)


@pytest.mark.parametrize('sid', [spec('notpd-regs', 0, 65, (3, 3), kind='notpd'),
                                 spec('notpd-gen-t1', 1, (25, 50), (3, 3), drows=25, kind='notpd')])
def test_indefinite_system_is_reported(eng, pkg, sid):
    """C = -F'F on the last mode: its system matrix has no Cholesky factor (types 1/5 factor w*C itself)."""
    declare(eng, sid)
    put_state(eng, start_state(sid))
    with pytest.raises(pkg.NotPositiveDefinite):
        run_device(eng, sid, 3)


@pytest.mark.parametrize('sid,path', _params([(spec('exact-%s' % f, 0, rows, (R, R), kind='exact'), p) for f, rows, R, p in FORM_SHAPES]))
def test_integer_inputs_give_bitwise_results(eng, sid, path):
    """Integer-valued inputs, C = 2 I, both modes non-negative: rho = 2, the system is 4 I, L = 2 I, the Delta weights
    1/2 -- every operation of 4 iterations is exact in fp64, whatever its order."""
    out, dev = check_case(eng, sid, path, 4, expect_iters=4)
    ref, _ = host_pair(sid, 4)
    for k in STATE_KEYS:
        for a, b in zip(dev[k], ref[k]):
            assert np.array_equal(a, b), k
    assert np.array_equal(dev['Delta'], ref['Delta'])


# ---------------------------------------------------------------------------------------------------------------------
# re-entry
# ---------------------------------------------------------------------------------------------------------------------
TWICE = ['regs-mixed-t4-n2-65x(5,3)q5', 'wg-t4-n4-300x(2,5,9,3)q6', 'rows-t4-n2-2049x(4,3)q4', 'rows-unimodality-65',
         'gen-t1', 'gen-t3-mixed', 'gen-t5-n3', 'gen-t4-n2-64x(17,9)q17']


@pytest.mark.parametrize('sid', [pytest.param(s, id='twice-%s' % s) for s in TWICE])
def test_second_call_continues_the_first(eng, sid):
    """Two calls of 3 iterations on one engine, the second from the state the first left, equal one reference run of 6:
    nothing a call keeps (rho pointers, Delta weights, the images of Delta) may be stale in the next."""
    ref, floor = host_pair(sid, 6)
    start = start_state(sid)
    declare(eng, sid)
    put_state(eng, start)
    run_device(eng, sid, 3)
    out = run_device(eng, sid, 3)
    assert out['inner_iters'] == 3
    out['inner_iters'] = 6
    compare(sid, out, get_state(eng, start), ref, floor, EXIT_SHAPES[sid], start)


def test_refusals(pkg):
    """A coupling that holds a mode of a PARAFAC2 block, and a multi-device context: AOADMM_ERR_UNSUPPORTED."""
    from helpers import par2_C_coupled_model
    from oracle import aoadmm as OA
    rng = np.random.default_rng(3)
    Z, io = par2_C_coupled_model(rng, 0)
    G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=rng)
    Z['_ranks'] = [3] * 6
    _, drv = _mods()
    with pkg.Engine(0) as e:
        drv.build_model(e, Z)
        drv.upload_state(e, Z, G)
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.coupled_loop(0, [np.zeros((16, 3))] * 2, [np.eye(3)] * 2, 3, (0.0,) * 4)
    with pkg.Engine([0]) as e:
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.coupled_loop(0, [np.zeros((16, 3))], [np.eye(3)], 3, (0.0,) * 4)
