"""GPU: the sparse team kernels (csrc/coo_team.h: mttkrp_coo_k, coo_carry_k, sem_pass_k, model_at_k and the two
finishers) return the bits they returned before their team layout and launch ladders were written once.
tests/golden/sparse_team_bits.json holds one sha256 per output array, recorded by tools/record_sparse_team_bits.py from
a build of the commit before that change; the case list below is the one the tool records.  Every case is computed
twice: the two runs must agree before they are compared with the fixture, so a case that is not stable run to run is
not mistaken for a change of the arithmetic.

Inputs come from numpy.random.default_rng([seed of the kind, N, R, nnz]); the seeds are SEED below."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import options
from test_gpu_heldout import par2_block, par2_list
from test_gpu_sparse_nvecs import generator_a, upload
from test_gpu_sparse_observed import cp_Z, put_factors, signed

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sparse_team_bits.json')

DIMS = (37, 29, 23, 11, 7)                                   # a case of order N takes the first N
# both edges of every team width (4, 8, 16, 32, 64); orders 2-4 are compiled in, order 5 is read at run time
PAIRS = [(2, 1), (3, 4), (4, 5), (5, 8), (3, 9), (2, 16), (4, 17), (3, 20), (5, 32), (3, 33), (4, 64), (2, 64)]
ROW_MAJOR = [(4, 17), (5, 32)]                               # also gathered from the row-major factor copies
NNZ = 1003                                                   # four teams; the last holds 235 entries = 3 mod 4 = 3 mod 8
LIST = 1003                                                  # subscripts of the model_at / held-out list
CARRY_SHAPE, CARRY_NNZ = (400, 300, 200), 70000              # 274 teams -> 548 slots -> 3 teams -> 6 slots -> 1
ALPHAS = (0.0, 0.25)
SEED = {'cp': 9100, 'carry': 9200, 'par2': 9300, 'nvecs': 9400}

# (kind, N, R, nnz)
CASES = ([('cp', N, R, NNZ) for N, R in PAIRS] + [('cp', 3, 4, 256), ('cp', 3, 20, 257), ('carry', 3, 16, CARRY_NNZ),
                                                   ('par2', 3, 3, 0), ('nvecs', 3, 3, 0)])


def case_id(case):
    return '%s-N%d-R%d-nnz%d' % case


def digest(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float64, np.int64)
    return hashlib.sha256(a.tobytes()).hexdigest()


def distinct_subs(rng, shape, nnz):
    cells = rng.choice(int(np.prod(shape)), nnz, replace=False)
    return np.stack(np.unravel_index(cells, shape), axis=1).astype(np.int64)


def carry_subs(rng, shape, nnz):
    """nnz distinct subscripts in shuffled order, half of them in row 1 of mode 0"""
    rest = int(np.prod(shape[1:]))
    heavy = rng.choice(rest, nnz // 2, replace=False)
    other = rng.choice((shape[0] - 1) * rest, nnz - nnz // 2, replace=False)
    row = np.concatenate([np.ones(len(heavy), dtype=np.int64), other // rest + (other // rest >= 1)])
    tail = np.stack(np.unravel_index(np.concatenate([heavy, other % rest]), shape[1:]), axis=1)
    subs = np.concatenate([row[:, None], tail], axis=1).astype(np.int64)
    assert len(np.unique(subs, axis=0)) == nnz and np.count_nonzero(subs[:, 0] == 1) == nnz // 2
    return subs[rng.permutation(nnz)]


def em_steps(pkg, eng, shape, R, F1, F2, tag, out):
    """Two consecutive steps (the first without a snapshot: STAT 1 / form 1; the second with it: STAT 2 / form 2) and
    the imputed MTTKRP of every mode between them"""
    put_factors(pkg, eng, shape, F1)
    out[tag + 'em1'] = np.array(eng.em_step(0))
    put_factors(pkg, eng, shape, F2)
    for n in range(len(shape)):
        out[tag + 'imputed%d' % n] = eng.resident_mttkrp(0, n, shape[n], R)
    out[tag + 'em2'] = np.array(eng.em_step(0))


def compute_cp(pkg, eng, rng, shape, R, subs, row_major):
    N = len(shape)
    out = {}
    vals = rng.standard_normal(len(subs))
    pkg.build_model(eng, cp_Z(shape, R, pkg.sptensor(subs, vals, shape)))
    F1, F2 = signed(rng, shape, R), signed(rng, shape, R)
    lsubs = np.stack([rng.integers(0, s, LIST) for s in shape], axis=1).astype(np.int64)
    y = rng.standard_normal(LIST)
    wsubs = subs[rng.permutation(len(subs))]
    wts = rng.uniform(0.0, 2.0, len(subs)) / 2.0             # drawn in (0, 2); the library takes weights divided by their bound
    put_factors(pkg, eng, shape, F1)
    for n in range(N):
        out['mttkrp%d' % n] = eng.resident_mttkrp(0, n, shape[n], R)
    out['model_at'] = eng.model_at(0, lsubs)
    if row_major:                                            # one outer iteration leaves the row-major copies current
        pkg.run_solver(eng, options(MaxOuterIters=1), N)
        for n in range(N):
            out['rowmajor_mttkrp%d' % n] = eng.resident_mttkrp(0, n, shape[n], R)
        out['rowmajor_model_at'] = eng.model_at(0, lsubs)
    eng.set_heldout(0, lsubs, y)
    st = eng.heldout_stats(0)
    assert st[3] == LIST
    out['heldout_stats'] = np.array(st[:3])
    eng.set_observed_only(0)
    em_steps(pkg, eng, shape, R, F1, F2, 'observed_', out)
    for alpha in ALPHAS:
        eng.set_entry_weights(0, wsubs, wts, alpha)          # sets again: no snapshot
        em_steps(pkg, eng, shape, R, F1, F2, 'weighted%g_' % alpha, out)
    return out


def compute(pkg, eng, case):
    """name -> array of every output of one case"""
    kind, N, R, nnz = case
    rng = np.random.default_rng([SEED[kind], N, R, nnz])
    if kind == 'cp':
        shape = DIMS[:N]
        return compute_cp(pkg, eng, rng, shape, R, distinct_subs(rng, shape, nnz), (N, R) in ROW_MAJOR)
    if kind == 'carry':
        return compute_cp(pkg, eng, rng, CARRY_SHAPE, R, carry_subs(rng, CARRY_SHAPE, nnz), False)
    if kind == 'par2':                                       # the P2 instance of model_at_k
        Z, _, _, _ = par2_block(pkg, eng, rng, True)
        I, Jk, _ = Z['size']
        subs = par2_list(rng, I, Jk, LIST)
        out = {'model_at': eng.model_at(0, subs)}
        eng.set_heldout(0, subs, rng.standard_normal(LIST))
        out['heldout_stats'] = np.array(eng.heldout_stats(0)[:3])
        return out
    assert kind == 'nvecs'                                   # coo_list_pass: the team kernel with one gathered factor
    X = generator_a(rng, (40, 30, 20), 0.15, R)
    upload(pkg, eng, X, R)
    out = {}
    for n in range(3):
        U, ev, info = eng.resident_nvecs(0, n, X.shape[n], R, seed=5)
        out['U%d' % n], out['eigvals%d' % n] = U, ev
        out['info%d' % n] = np.array([info['iterations'], info['converged'], info['block'], info['fibers']], dtype=np.int64)
    return out


def hashes(pkg, eng, case):
    return {k: digest(v) for k, v in compute(pkg, eng, case).items()}


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_same_bits_as_recorded(pkg, eng, recorded, case):
    first, second = hashes(pkg, eng, case), hashes(pkg, eng, case)
    assert first == second, 'two runs of this build differ in ' + ', '.join(k for k in first if first[k] != second[k])
    want = recorded[case_id(case)]
    assert sorted(first) == sorted(want)
    assert first == want, 'differs from the recorded build in ' + ', '.join(k for k in first if first[k] != want[k])
