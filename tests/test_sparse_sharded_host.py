"""CPU: the host side of sharded sparse CP blocks -- the cut rule (`_capi.coo_share`), the binding list, the header and
the signatures of the host layers."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'aoadmm_hip.h')


@pytest.fixture(scope='module')
def capi():
    return __import__('importlib').import_module('matlab-code_amd._capi')


@pytest.mark.parametrize('world', range(1, 10))
def test_shares_cover_every_nonzero_exactly_once(capi, world):
    for nnz in (0, 1, 2, world - 1, world, world + 1, 255, 256, 257, world * 256, world * 256 + 1, 3001, 10 ** 8 + 7,
                2 ** 31 - 2):
        cuts = [capi.coo_share(nnz, r, world) for r in range(world)]
        assert cuts[0][0] == 0 and cuts[-1][1] == nnz
        for (lo, hi), (lo2, _) in zip(cuts, cuts[1:]):
            assert hi == lo2                                    # contiguous: no gap, no overlap
        sizes = [hi - lo for lo, hi in cuts]
        assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1 and sum(sizes) == nnz
        assert cuts == [(r * nnz // world, (r + 1) * nnz // world) for r in range(world)]


def test_share_arguments_are_checked(capi):
    for bad in ((-1, 0, 1), (5, 2, 2), (5, -1, 2), (5, 0, 0)):
        with pytest.raises(ValueError):
            capi.coo_share(*bad)


def test_entry_is_declared_and_bound(capi):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'\bint\s+aoadmm_tensor_upload_coo_sharded\s*\(\s*aoadmm_ctx\s*\*\s*ctx\s*,\s*int\s+p\s*,\s*int64_t\s+nnz\s*,'
                     r'\s*const\s+int64_t\s*\*\s*subs\s*,\s*const\s+double\s*\*\s*vals\s*\)\s*;', text)
    assert 'aoadmm_tensor_upload_coo_sharded' in capi.SYMBOLS
    assert re.search(r'#define\s+AOADMM_ABI_VERSION\s+3\b', open(HEADER).read())


def test_host_layers_take_the_switch(pkg):
    assert inspect.signature(pkg.Engine.upload_coo).parameters['sharded'].default is False
    assert inspect.signature(pkg.build_model).parameters['sparse_sharding'].default is False
    gateway = open(os.path.join(ROOT, 'matlab-code_amd', 'mex', 'aoadmm_mex.cpp')).read()
    assert '"sparse_sharding"' in gateway and 'aoadmm_tensor_upload_coo_sharded' in gateway
