"""GPU: the best held-out iterate (include/aoadmm_hip.h aoadmm_heldout_keep_best / aoadmm_heldout_restore_best, DESIGN.md
section 9.4).  A solve with the switch on keeps the whole solver state of the iteration with the smallest weighted
held-out sum; restoring it must leave the engine exactly where a solve of that many iterations leaves it.

Most models' held-out sum falls monotonically, which would make the restore trivial, so the tests PLACE the minimum: solve
b iterations, take y = model_at(subs) of that state and attach (subs, y) as the list.  H_b is then zero or at rounding
level and every other H_i far above it; `heldout_best_iter == b` is asserted before anything is concluded from it."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import aoadmm as OA
from helpers import cp_model, options, script1_model, script4_model
from test_gpu_heldout import (NN, OBSERVED, SOLVE_CASES, cp_Z, make_list, par2_list, par2_ref, ref_values, same, solve_case,
                              some_entries)
from test_gpu_sparse_sharded import on_ranks

pytestmark = pytest.mark.gpu

capi = importlib.import_module('matlab-code_amd._capi')

STATE_KEYS = ('fac', 'constraint_fac', 'constraint_dual_fac', 'coupling_fac', 'coupling_dual_fac', 'DeltaB', 'P', 'mu_DeltaB')


class Case:
    """A model, its starting point G and a list of subscripts of block 1, run through the engine step by step."""

    def __init__(self, Z, io, opt, subs, hip=None, prec='f64', sharding=False):
        self.G = OA.init_coupled_AOADMM_CMTF({**Z, 'prox_operators': None}, io, rng=np.random.default_rng(7))
        ranks = [int((F[0] if isinstance(F, (list, tuple)) else F).shape[1]) for F in self.G['fac']]
        self.Z = dict(Z, _ranks=ranks)
        self.opt, self.hip, self.prec, self.subs, self.sharding = opt, dict(hip or {}), prec, np.asarray(subs, dtype=np.int64), sharding
        self.last = opt['MaxOuterIters']
        self.has_missing = bool(self.hip.get('sparse_observed_only')) or Z.get('miss') is not None

    def start(self, pkg, e, y=None, keep=False):
        pkg.build_model(e, self.Z, self.prec, sparse_sharding=self.sharding, observed_only=self.hip.get('sparse_observed_only', 0))
        if y is not None:
            e.set_heldout(0, self.subs, y)
        if keep:
            e.heldout_keep_best(True)
        pkg.upload_state(e, self.Z, copy.deepcopy(self.G))

    def solve(self, pkg, e, iters):
        out = pkg.run_solver(e, {**self.opt, 'MaxOuterIters': iters, 'hip': self.hip}, len(self.Z['size']),
                             has_missing=self.has_missing)
        del out['time_at_it']
        return out

    def state(self, pkg, e):
        return pkg.download_state(e, self.Z, self.G)

    def prefix(self, pkg, e, b):
        """The b-iteration solve from G: y = the model at the list, the state, and what two more iterations give."""
        self.start(pkg, e)
        self.solve(pkg, e, b)
        y = e.model_at(0, self.subs)
        st = self.state(pkg, e)
        more_out = self.solve(pkg, e, 2)
        return dict(y=y, state=st, more_out=more_out, more_state=self.state(pkg, e))

    def long(self, pkg, e, y, keep):
        """The solve of `last` iterations with the list (subs, y) attached: (state, out, trace, best_iter)."""
        self.start(pkg, e, y, keep)
        out = self.solve(pkg, e, self.last)
        tr, best = e.heldout_trace(0)
        return self.state(pkg, e), out, tr, best


def state_bytes(F):
    def count(v):
        if v is None:
            return 0
        if isinstance(v, dict):
            return sum(count(x) for x in v.values())
        if isinstance(v, (list, tuple)):
            return sum(count(x) for x in v)
        return 8 * int(np.asarray(v).size)
    return sum(count(F.get(k)) for k in STATE_KEYS)


def improving(T):
    """iterations at which the trace is strictly below everything before it, iteration 0 included"""
    best, n = None, 0
    for v in T:
        if best is None or v < best:
            best, n = v, n + 1
    return n


def assert_state(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), '%s: G.%s differs' % (what, k)


_cases, _refs = {}, {}


def case_of(pkg, name):
    if name not in _cases:
        Z, io, opt, held, hip, prec = solve_case(pkg, name)
        _cases[name] = Case(Z, io, opt, held[1][0], hip, prec)
    return _cases[name]


def reference(pkg, eng, name, b):
    """Computed once per (case, b) and left unchanged: the prefix solve and the long solve with the switch off."""
    if (name, b) not in _refs:
        c = case_of(pkg, name)
        ref = c.prefix(pkg, eng, b)
        ref['off'] = c.long(pkg, eng, ref['y'], keep=False)
        _refs[(name, b)] = ref
    return _refs[(name, b)]


def kept_and_restored(pkg, eng, name, b, c=None, ref=None):
    """The long solve with the switch on, checked against the one with it off, then restored."""
    c = c or case_of(pkg, name)
    ref = ref or reference(pkg, eng, name, b)
    st, out, tr, best = c.long(pkg, eng, ref['y'], keep=True)
    st0, out0, tr0, best0 = ref['off']
    print('%s b = %d: H_b = %.3e, smallest other H_i = %.3e' % (name, b, tr[b], np.delete(tr, b).min()))
    assert best == b, 'precondition: the minimum was placed at %d, the trace has it at %d' % (b, best)
    assert_state(st, st0, 'the solve with the switch on')
    assert same(out, out0) and np.array_equal(tr, tr0) and best == best0
    info = eng.heldout_best_info()
    assert info['have'] and info['iter'] == b and info['launches'] == improving(tr)
    assert eng.heldout_restore_best() == b
    return c, ref, out, tr


# ---- 1. restore equals the prefix solve -------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [0, 3, 'last'])
@pytest.mark.parametrize('name', SOLVE_CASES)
def test_restore_equals_the_prefix_solve(pkg, eng, name, b):
    b = case_of(pkg, name).last if b == 'last' else b
    c, ref, _, _ = kept_and_restored(pkg, eng, name, b)
    assert_state(c.state(pkg, eng), ref['state'], 'restored')
    assert eng.heldout_restore_best() == b                    # the kept copy survives the call
    assert_state(c.state(pkg, eng), ref['state'], 'restored twice')


# ---- 2. nothing stale is left behind ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SOLVE_CASES)
def test_nothing_stale_after_restore(pkg, eng, name):
    nothing_stale(pkg, eng, name, 3, *kept_and_restored(pkg, eng, name, 3))


def test_nothing_stale_with_tensor_passes(pkg, eng, tensor_passes):
    """The fp64 dense block through the tensor-pass kernels (at this size it would take the one-launch MTTKRP): the next
    solve reduces over the partial contraction the last passes of iteration b left, which the restore replays."""
    Z, io, opt, held, hip, prec = solve_case(pkg, 'dense')
    c = Case(Z, io, opt, held[1][0], hip, prec)
    ref = c.prefix(pkg, eng, 3)
    ref['off'] = c.long(pkg, eng, ref['y'], keep=False)
    nothing_stale(pkg, eng, 'dense, tensor passes', 3, *kept_and_restored(pkg, eng, 'dense, tensor passes', 3, c, ref))


def nothing_stale(pkg, eng, name, b, c, ref, _, tr):
    st = eng.heldout_stats(0)
    print('%s: heldout_stats %.17g, func_heldout[%d] %.17g' % (name, st[0], b, tr[b]))
    assert abs(st[0] - tr[b]) <= 1e-11 * tr[b]
    Fb = ref['state']
    md = [m - 1 for m in c.Z['modes'][0]]
    if c.Z['model'][0] == 'PAR2':
        m_ref, bound = par2_ref(Fb['fac'][md[0]], Fb['fac'][md[1]], Fb['fac'][md[2]], c.subs)
    else:
        m_ref, bound = ref_values([Fb['fac'][m] for m in md], c.subs)
    assert abs(st[2] - float(np.sum(m_ref * m_ref))) <= 1e-11 * float(np.sum(m_ref * m_ref))
    worst = float(np.max(np.abs(eng.model_at(0, c.subs) - m_ref) / bound))
    assert worst <= 1e-12, worst                              # the bar of test_model_at_values
    # two more iterations from the engine's state: Gram matrices, row-major copies, the cached pass, the B_k Gram matrices,
    # the Y cache of sparse slabs and the imputed entries of Z.miss all have to be those of iteration b
    more_out = c.solve(pkg, eng, 2)
    assert same(more_out, ref['more_out'])
    assert_state(c.state(pkg, eng), ref['more_state'], 'two iterations after the restore')


# ---- 3. early stopping, end to end ------------------------------------------------------------------------------------
def test_early_stopping_returns_the_best_iterate(pkg, eng):
    """The over-fitting case of test_gpu_heldout.py: minimum at iteration 29, patience 5 stops at 34."""
    rng = np.random.default_rng(33)
    shape = (30, 25, 20)
    Z, io, _ = cp_model(shape, 2, rng, [None] * 3, noise=1.0)
    io['lambdas_init'] = [[1] * 4]
    X = np.asarray(Z['object'][0])
    u = rng.random(shape)
    train, hold = u < 0.05, (u >= 0.05) & (u < 0.10)
    assert train.sum() == 702 and hold.sum() == 754
    Zs = dict(Z, object=[pkg.sptensor(np.argwhere(train), X[train], shape)])
    subs, y = np.argwhere(hold), X[hold]
    G = OA.init_coupled_AOADMM_CMTF({**Zs, 'prox_operators': None}, io, rng=np.random.default_rng(7))

    def run(iters=60, **hip):
        alg = {**options(MaxOuterIters=iters, MaxInnerIters=5), 'hip': {**OBSERVED, **hip}}
        _, F, _, out = pkg.cmtf_AOADMM(Zs, alg_options=alg, init=copy.deepcopy(G), engine=eng)
        return F, out

    def heldout_sum(F):
        return float(np.sum((y - ref_values(F['fac'], subs)[0]) ** 2))

    F34, out34 = run(heldout={1: (subs, y)}, heldout_patience=5)
    Fb, out = run(heldout={1: (subs, y)}, heldout_patience=5, heldout_keep_best=1)
    assert out['OuterIterations'] == 34 and out['heldout_restored_iter'] == 29 == out['heldout_best_iter']
    assert out['exit_flag'] == 'heldoutPatience'
    assert set(out) - set(out34) == {'heldout_restored_iter'}
    for k in out34:                                           # every other field still describes the whole run
        if k != 'time_at_it':
            assert same(out[k], out34[k]), k
    F29, _ = run(iters=29)
    assert same(Fb, F29)
    T = out['func_heldout'][1]
    got, last = heldout_sum(Fb), heldout_sum(F34)
    print('held-out sum: returned factors %.6f, trace minimum %.6f, 34-iteration factors %.6f' % (got, T.min(), last))
    assert abs(got - T.min()) <= 1e-11 * T.min() and got < last


# ---- 4. copy-kernel shapes --------------------------------------------------------------------------------------------
def shape_case(pkg, name):
    rng = np.random.default_rng(404)
    if name == 'rows-1-31-70001':
        # 3, 93 and 210 003 doubles per array: odd counts, arrays shorter than a chunk, and one that spans 103 chunks
        shape, R = (1, 31, 70001), 3
        Z = cp_Z(shape, R, some_entries(pkg, rng, shape, 4000))
        Z.update(constrained_modes=[0, 0, 1], constraints=[None, None, NN])
        del Z['_ranks']
        io = dict(lambdas_init=[[1] * R], nvecs=0, distr=[lambda a, b: rng.random((a, b))] * 3, normalize=1)
        return Case(Z, io, options(MaxOuterIters=5), make_list(rng, shape, 300))
    Z, io = script4_model(rng, K=4)                           # ragged J_k = 61, 68, 75, 82
    I, Jk, K = Z['size']
    return Case(Z, io, options(MaxOuterIters=5), par2_list(rng, I, Jk, 300))


@pytest.mark.parametrize('b', [0, 2])
@pytest.mark.parametrize('name', ['rows-1-31-70001', 'par2-ragged-K4'])
def test_copy_kernel_shapes_and_counters(pkg, eng, name, b):
    c = shape_case(pkg, name)
    ref = c.prefix(pkg, eng, b)
    st, _, tr, best = c.long(pkg, eng, ref['y'], keep=True)
    assert best == b, 'precondition: the minimum was placed at %d, the trace has it at %d' % (b, best)
    info = eng.heldout_best_info()
    nbytes = state_bytes(st)
    print('%s: %d state bytes, %d snapshot launches' % (name, nbytes, info['launches']))
    assert info['launches'] == improving(tr) and info['bytes'] == info['launches'] * 2 * nbytes
    assert eng.heldout_restore_best() == b
    assert_state(c.state(pkg, eng), ref['state'], 'restored')
    assert eng.heldout_best_info() == info                    # a restore is not a snapshot


# ---- 5. ranks ---------------------------------------------------------------------------------------------------------
def _rank_flow(pkg, c, b, e):
    ref = c.prefix(pkg, e, b)
    st, out, tr, best = c.long(pkg, e, ref['y'], keep=True)
    info = e.heldout_best_info()
    it = e.heldout_restore_best()
    got = c.state(pkg, e)
    it2 = e.heldout_restore_best()
    return dict(ref=ref['state'], last=st, best=best, it=(it, it2), got=got, again=c.state(pkg, e), info=info,
                nbytes=state_bytes(st))


def test_ranks_with_sharded_nonzeros(pkg):
    """World 2, the block's nonzeros sharded over the ranks: the ranks are bit-identical and each equals its own prefix."""
    Z, io, opt, held, hip, prec = solve_case(pkg, 'sparse')
    c = Case(Z, io, opt, held[1][0], hip, prec, sharding=True)
    res = on_ranks(pkg, 2, lambda e, r: _rank_flow(pkg, c, 3, e))
    for r in res:
        assert r['best'] == 3 and r['it'] == (3, 3)
        assert_state(r['got'], r['ref'], 'restored')
        assert_state(r['again'], r['ref'], 'restored twice')
    assert same(res[0]['got'], res[1]['got']) and same(res[0]['last'], res[1]['last'])


def test_ranks_with_a_slab_sharded_parafac2_block(pkg):
    """World 2, CP + PARAFAC2 (K = 20) coupled in their first modes, the slabs sharded over the ranks, the list on the CP
    block: every rank keeps and restores its own slabs, and the gather that follows gives each the world-2 prefix state."""
    rng = np.random.default_rng(505)
    Z, io = script1_model(rng, noise=0.05)
    c = Case(Z, io, options(MaxOuterIters=6), make_list(rng, (20, 30, 40), 300), hip={'par2_slab_sharding': 1})
    res = on_ranks(pkg, 2, lambda e, r: _rank_flow(pkg, c, 3, e))
    for r in res:
        assert r['best'] == 3 and r['it'] == (3, 3)
        assert_state(r['got'], r['ref'], 'restored')
        assert_state(r['again'], r['ref'], 'restored twice')
        # the slabs were sharded: a rank's snapshot is smaller than the whole state
        assert 0 < r['info']['bytes'] < r['info']['launches'] * 2 * r['nbytes']
    assert same(res[0]['got'], res[1]['got'])


# ---- 6. lifetime and refusals -----------------------------------------------------------------------------------------
def _invalid(pkg, fn):
    with pytest.raises(pkg.AoadmmError) as ei:
        fn()
    assert ei.value.code == capi.ERR_INVALID


def test_lifetime_and_refusals(pkg, eng):
    c = case_of(pkg, 'sparse')
    y = np.zeros(len(c.subs))
    c.start(pkg, eng, y, keep=True)
    assert eng.heldout_best_info() == dict(have=False, iter=-1, bytes=0, launches=0)
    _invalid(pkg, eng.heldout_restore_best)                   # before any solve
    c.solve(pkg, eng, 4)
    it = eng.heldout_restore_best()
    assert it == eng.heldout_trace(0)[1] and eng.heldout_best_info()['have']
    F = c.state(pkg, eng)
    pkg.upload_state(eng, c.Z, F)                             # any aoadmm_state_set invalidates the copy
    assert not eng.heldout_best_info()['have']
    _invalid(pkg, eng.heldout_restore_best)
    c.solve(pkg, eng, 2)
    assert eng.heldout_best_info()['have']
    eng.heldout_keep_best(False)                              # releases the copy
    assert eng.heldout_best_info() == dict(have=False, iter=-1, bytes=0, launches=0)
    _invalid(pkg, eng.heldout_restore_best)
    c.solve(pkg, eng, 2)                                      # the switch is off: nothing is kept
    assert not eng.heldout_best_info()['have']
    for bad in (2, -1):
        _invalid(pkg, lambda: capi.check(eng.lib.aoadmm_heldout_keep_best(eng.h, bad)))
    eng.heldout_keep_best(True)
    c.solve(pkg, eng, 2)
    assert eng.heldout_best_info()['have']
    pkg.build_model(eng, c.Z)                                 # aoadmm_model_begin clears the switch and the copy
    assert eng.heldout_best_info() == dict(have=False, iter=-1, bytes=0, launches=0)
    _invalid(pkg, eng.heldout_restore_best)
    # the switch on and no list: refused before any work, the state untouched
    c.start(pkg, eng, None, keep=True)
    before = c.state(pkg, eng)
    drv = importlib.import_module('matlab-code_amd.driver')
    o = drv._make_options(options(MaxOuterIters=3))
    res = capi.Result()
    assert eng.lib.aoadmm_solve(eng.h, C.byref(o), C.byref(res)) == capi.ERR_INVALID
    assert_state(c.state(pkg, eng), before, 'after the refused solve')
    eng.heldout_keep_best(False)
    c.solve(pkg, eng, 1)                                      # and the model still solves


def test_multi_device_context_is_refused(pkg):
    rng = np.random.default_rng(53)
    shape, R = (12, 10, 8), 3
    Z = cp_Z(shape, R, some_entries(pkg, rng, shape, 100))
    with pkg.Engine([0, 0]) as e:
        pkg.build_model(e, Z)
        pkg.upload_state(e, Z, {'fac': [rng.random((s, R)) for s in shape]})
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.heldout_keep_best(True)
        with pytest.raises(pkg.UnsupportedOnDevice):
            e.heldout_restore_best()
