"""CPU: ranking metrics tracked inside a solve, the parts that need no device: the C entries and
their ids, the options `cmtf_AOADMM` checks before it touches the engine, the host statement of the best / patience rule
(`rank_rule`, which the GPU tests apply to un-stopped traces), and the place of the ranking slots in the read-back arena."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from test_capi_symbols import HEADER, declared_functions
from test_gpu_heldout import cp_Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['aoadmm_tensor_set_ranklist', 'aoadmm_ranklist_info', 'aoadmm_rank_track', 'aoadmm_rank_trace', 'aoadmm_ranklist_last',
           'aoadmm_op_rank_metrics']
WRAPPERS = ['set_ranklist', 'ranklist_info', 'rank_track', 'rank_trace', 'ranklist_last', 'op_rank_metrics']


# ---- 1. header and binding ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
def test_entries_are_declared_bound_and_exported(pkg, entry):
    capi = importlib.import_module('matlab-code_amd._capi')
    assert entry in declared_functions() and entry in capi.SYMBOLS
    lib = pkg.load_library()
    assert hasattr(lib, entry) and getattr(lib, entry).argtypes is not None
    assert lib.aoadmm_abi_version() == 3                      # functions were added, nothing moved: the version stays


def test_engine_and_package_have_the_wrappers(pkg):
    for w in WRAPPERS:
        assert hasattr(pkg.Engine, w), w
    for name in ('rank_options', 'rank_rule', 'pooled_score', 'parse_rank_metric'):
        assert hasattr(pkg, name), name


def test_options_struct_is_where_it_was(pkg):
    capi = importlib.import_module('matlab-code_amd._capi')
    assert C.sizeof(capi.Options) == 120 and capi.Options.reserved.offset == 104
    assert capi.Options.heldout_patience.offset == 100


def test_metric_ids_of_header_and_binding_agree(pkg):
    capi = importlib.import_module('matlab-code_amd._capi')
    text = open(HEADER).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r'AOADMM_RANK_([A-Z]+)\s*=\s*(\d+)', text)}
    assert ids == dict(HIT=capi.RANK_HIT, NDCG=capi.RANK_NDCG, MRR=capi.RANK_MRR, AUC=capi.RANK_AUC)
    assert capi.RANK_METRICS == dict(hit=capi.RANK_HIT, ndcg=capi.RANK_NDCG, mrr=capi.RANK_MRR, auc=capi.RANK_AUC)
    sums = {m.group(1): int(m.group(2)) for m in re.finditer(r'AOADMM_RANKSUM_([A-Z_]+)\s*=\s*(\d+)', text)}
    assert sums == dict(N=capi.RANKSUM_N, N_AUC=capi.RANKSUM_N_AUC, HITS=capi.RANKSUM_HITS, NDCG=capi.RANKSUM_NDCG,
                        MRR=capi.RANKSUM_MRR, AUC=capi.RANKSUM_AUC, COUNT=capi.RANKSUM_COUNT)


def test_null_context_is_refused(pkg):
    capi = importlib.import_module('matlab-code_amd._capi')
    lib = pkg.load_library()
    assert lib.aoadmm_rank_track(None, 1, 10, 1, 0, 0) == capi.ERR_INVALID
    assert lib.aoadmm_tensor_set_ranklist(None, 0, 0, 0, None, None, None) == capi.ERR_INVALID
    assert lib.aoadmm_op_rank_metrics(None, 0, None, None, 1, None) == capi.ERR_INVALID


# ---- 2. option validation -------------------------------------------------------------------------------------------------
def two_block_Z():
    shape = (6, 5, 4)
    Z = cp_Z(shape, 3, None)
    Z.update(model=['CP', 'PAR2'], modes=[[1, 2, 3], [4, 5, 6]], size=[6, 5, 4, 7, [3, 3], 2], object=[None, None],
             weights=[1.0, 1.0])
    return Z


def good_list():
    subs = np.array([[0, 1, 2], [5, 4, 3], [2, 2, 2]], dtype=np.int64)
    return dict(mode=3, subs=subs, exclude=(np.array([0, 2, 2, 3]), np.array([3, 3, 0])))


def test_rank_options_defaults_and_a_good_list(pkg):
    Z = two_block_Z()
    o = pkg.rank_options(Z, {})
    assert o == dict(lists={}, metric='ndcg', k=10, every=1, patience=0, criterion=0)
    o = pkg.rank_options(Z, dict(rank_lists={1: good_list()}, rank_metric='hit@5', rank_every=3, rank_patience=2, rank_criterion=1))
    assert (o['metric'], o['k'], o['every'], o['patience'], o['criterion']) == ('hit', 5, 3, 2, 1)
    mode, subs, ex = o['lists'][0]
    assert mode == 2 and subs.dtype == np.int64 and subs.shape == (3, 3) and ex[0].dtype == np.int64 and len(ex[1]) == 3
    assert pkg.rank_options(Z, dict(rank_lists={1: dict(mode=1, subs=np.zeros((0, 3), dtype=np.int64))}))['lists'] == {}
    assert [pkg.parse_rank_metric(s) for s in ('ndcg@10', 'hit@5', 'mrr', 'auc', ' NDCG@1 ', 'hit')] == [
        ('ndcg', 10), ('hit', 5), ('mrr', 10), ('auc', 10), ('ndcg', 1), ('hit', 10)]


@pytest.mark.parametrize('hip', [
    dict(rank_metric='precision@5'), dict(rank_metric='ndcg@'), dict(rank_metric='ndcg@0'), dict(rank_metric='hit@-1'),
    dict(rank_metric='hit@2.5'), dict(rank_metric='mrr@3'), dict(rank_metric='auc@10'), dict(rank_metric=10), dict(rank_metric=None),
    dict(rank_metric='hit@%d' % 2 ** 31),
    dict(rank_every=0), dict(rank_every=-2), dict(rank_every=1.5), dict(rank_every='3'),
    dict(rank_patience=-1), dict(rank_patience=2), dict(rank_patience=2, rank_criterion=0),
    dict(rank_criterion=2), dict(rank_criterion=-1),
    dict(rank_criterion=1),                                                          # no list
    dict(rank_lists='x'), dict(rank_lists={0: good_list()}), dict(rank_lists={3: good_list()}), dict(rank_lists={True: good_list()}),
    dict(rank_lists={2: good_list()}),                                               # a PARAFAC2 block
    dict(rank_lists={1: (1, 2)}), dict(rank_lists={1: dict(mode=0, subs=good_list()['subs'])}),
    dict(rank_lists={1: dict(mode=4, subs=good_list()['subs'])}),
    dict(rank_lists={1: dict(mode=1, subs=np.zeros((3, 2), dtype=np.int64))}),
    dict(rank_lists={1: dict(mode=1, subs=np.array([[0, 0, 4]]))}), dict(rank_lists={1: dict(mode=1, subs=np.array([[-1, 0, 0]]))}),
    dict(rank_lists={1: dict(mode=1, subs=np.array([[0.5, 0, 0]]))}),
    dict(rank_lists={1: dict(mode=3, subs=good_list()['subs'], exclude=(np.array([0, 1, 2]), np.array([0, 1])))}),
    dict(rank_lists={1: dict(mode=3, subs=good_list()['subs'], exclude=(np.array([0, 1, 2, 3]), np.array([0, 1, 4])))}),
    dict(rank_lists={1: dict(mode=3, subs=good_list()['subs'], exclude=(np.array([0, 2, 1, 3]), np.array([0, 1, 2])))}),
    dict(rank_lists={1: dict(mode=3, subs=good_list()['subs'], exclude=7)}),
])
def test_rank_options_refusals(pkg, hip):
    with pytest.raises(ValueError):
        pkg.rank_options(two_block_Z(), hip)


def test_criterion_with_heldout_patience_is_refused(pkg):
    hip = dict(rank_lists={1: good_list()}, rank_criterion=1)
    assert pkg.rank_options(two_block_Z(), hip, 0)['criterion'] == 1
    with pytest.raises(ValueError):
        pkg.rank_options(two_block_Z(), hip, 3)
    assert pkg.rank_options(two_block_Z(), dict(rank_lists={1: good_list()}), 3)['criterion'] == 0   # trace only: allowed


def test_cmtf_checks_the_options_before_the_engine(pkg):
    """`cmtf_AOADMM` raises before the engine is touched: the engine here is an object with no methods at all."""
    Z = cp_Z((6, 5, 4), 3, np.zeros((6, 5, 4)))
    del Z['_ranks']
    G = {'fac': [np.ones((s, 3)) for s in (6, 5, 4)]}
    for hip in (dict(rank_metric='nope'), dict(rank_criterion=1), dict(rank_lists={2: good_list()}),
                dict(rank_lists={1: good_list()}, rank_criterion=1, heldout_patience=2,
                     heldout={1: (np.zeros((1, 3), dtype=np.int64), np.ones(1))})):
        with pytest.raises(ValueError):
            pkg.cmtf_AOADMM(Z, alg_options={'hip': hip}, init=G, engine=object())


# ---- 3. the host rule --------------------------------------------------------------------------------------------------------
NAN = float('nan')


@pytest.mark.parametrize('scores,patience,want', [
    ([], 0, (-1, None)), ([0.5], 3, (0, None)),
    ([0.1, 0.2, 0.3], 1, (2, None)),                          # always improving: never fires
    ([0.3, 0.2, 0.1], 1, (0, 1)), ([0.3, 0.2, 0.1], 2, (0, 2)), ([0.3, 0.2, 0.1], 3, (0, None)),
    ([0.3, 0.3, 0.3], 2, (0, 2)),                              # a tie is no improvement: the earliest stays
    ([0.1, 0.5, 0.5, 0.4, 0.6], 2, (1, 3)),                    # stops before the later maximum
    ([0.1, 0.5, 0.5, 0.4, 0.6], 3, (4, None)), ([0.1, 0.5, 0.5, 0.4, 0.6], 0, (4, None)),
    ([NAN, NAN, 0.2, 0.1], 3, (2, None)),                     # a NaN start is replaced by the first number
    ([NAN, NAN, NAN, 0.2], 2, (0, 2)),                         # ... unless the patience runs out on NaNs first
    ([0.2, NAN, 0.3], 2, (2, None)), ([0.2, NAN, NAN], 2, (0, 2)),   # a NaN never becomes the best
    ([0.2, 1.0, 1.0, 1.0, 1.0, 1.0], 4, (1, 5)),
])
def test_rank_rule(pkg, scores, patience, want):
    assert pkg.rank_rule(scores, patience) == want


def test_pooled_score(pkg):
    a = dict(n=np.array([2, 0, 3]), n_auc=np.array([1, 0, 0]), hits=np.array([1.0, 0.0, 3.0]), ndcg_sum=np.array([0.5, 0, 1.5]),
             mrr_sum=np.array([1.0, 0, 1.5]), auc_sum=np.array([0.25, 0, 0]))
    b = dict(n=np.array([2, 0, 1]), n_auc=np.array([1, 0, 0]), hits=np.array([2.0, 0.0, 0.0]), ndcg_sum=np.array([1.5, 0, 0.5]),
             mrr_sum=np.array([2.0, 0, 0.5]), auc_sum=np.array([0.75, 0, 0]))
    assert np.array_equal(pkg.pooled_score([a, b], 'hit'), [0.75, NAN, 0.75], equal_nan=True)    # pooled, not a mean of means
    assert np.array_equal(pkg.pooled_score([a, b], 'ndcg'), [0.5, NAN, 0.5], equal_nan=True)
    assert np.array_equal(pkg.pooled_score([a, b], 'auc'), [0.5, NAN, NAN], equal_nan=True)
    assert np.array_equal(pkg.pooled_score([a], 'mrr'), [0.5, NAN, 0.5], equal_nan=True)


def test_trace_dict_means(pkg):
    capi = importlib.import_module('matlab-code_amd._capi')
    sums = np.zeros((capi.RANKSUM_COUNT, 2))
    sums[:, 0] = [4, 2, 3, 2.5, 3.0, 1.5]
    d = pkg.Engine._rank_trace_dict(np.array([0, 3]), sums, 3)
    assert d['n'].tolist() == [4, 0] and d['n_auc'].tolist() == [2, 0] and d['iters'].tolist() == [0, 3] and d['best_iter'] == 3
    assert d['hit'][0] == 0.75 and d['ndcg'][0] == 0.625 and d['mrr'][0] == 0.75 and d['auc'][0] == 0.75
    assert all(np.isnan(d[k][1]) for k in ('hit', 'ndcg', 'mrr', 'auc'))


# ---- 4. the arena ------------------------------------------------------------------------------------------------------------
ARENA_PROGRAM = r'''
#include <cstdio>
#include "readback.h"
using namespace aoadmm;
int main() {
  int bad = 0;
  const int cases[3][3] = {{3, 1, 0}, {6, 2, 1}, {5, 3, 2}};
  for (auto& c : cases) {
    ArenaLayout L;
    L.build(c[0], c[1], c[2], std::vector<int>(c[1], 0));
    const ArenaView v = L.at(nullptr);
    const int before = c[0] * (kSlotsPerMode + kResidPerMode) + (kSlotsPerTensor + kEmStats + kHoSlots) * c[1] + kScratchSlots;
    bad += L.n_doubles() != before + 8 * c[1];
    bad += kRankSlots != 8 || kRankUsed != 6;
    for (int p = 0; p < c[1]; ++p) bad += v.rank(p) != v.heldout(c[1]) + 8 * p;
    bad += v.heldout(c[1] - 1) + kHoSlots != v.rank(0);
    bad += (char*)(v.rank(c[1] - 1) + 8) > (char*)v.ctl(0);
    bad += (size_t)((char*)v.ctl(0) - (char*)v.doubles()) != L.off_ctl || L.off_ctl % 64 != 0;
    std::printf("%d %d %d: n_doubles %d rank(0) at %td\n", c[0], c[1], c[2], L.n_doubles(), v.rank(0) - v.doubles());
  }
  return bad;
}
'''


def test_arena_layout(tmp_path):
    """`ArenaView::rank(p)` follows `heldout(p)`, `n_doubles()` grew by 8 per tensor, and the control records still follow
    the doubles: a small host program over csrc/readback.h."""
    src = tmp_path / 'arena.cpp'
    src.write_text(ARENA_PROGRAM)
    exe = tmp_path / 'arena'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include',
                    '-I', os.path.join(ROOT, 'matlab-code_amd', 'csrc'), str(src), '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
