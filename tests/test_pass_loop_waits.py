"""CPU: the steady loops of the tensor-pass kernels keep their load ring in flight -- read from the compiled gfx950 code.

tools/pass_loop_waits.py compiles csrc/contract.hip to assembly (device side only, no GPU) and lists, per pass kernel,
the operand of every `s_waitcnt vmcnt(N)` of the steady loop.  The compiler derives these from the loads pending on every
path into the loop header; when a conditional, freely scheduled prologue reached the header, it put vmcnt(0..2) there
and every revolution waited for nearly all loads in flight (the headline kernel contract16_f32<1,true,true>: 2 where one
ring stage is 7 loads).  With the ordered prologue as the only way into the loop the waits are counted ones.

Bounds:
  three-stage ring: while a stage is consumed the next one is complete in flight and the third is being issued, so no
      wait may ask for fewer outstanding loads than one stage holds: min vmcnt >= loads of one stage.
  two-stage ring (contract_f64<NT,true>): a stage is refilled in place while it is consumed, so when its last operand
      is waited for (the second leftover-column fragment, the last load the stage issued) only the OTHER stage is
      certain to be outstanding -- the stage that a three-stage ring has in flight on top of that does not exist here.
      The bound is one stage: min vmcnt >= loads of one stage = 8 + NT (4 tensor loads, NT fragments, 2 leftover-column
      fragments of two 16-byte loads each).  What the shallower ring lowers is the other end: its largest operand is
      one stage plus the consumed stage's own four fragment loads (13 at NT = 1), where a ring of three such stages
      would reach two stages (18).
No kernel uses scratch, and none has a lower occupancy than before the restructuring (profiles/pass_loop_waits_parent.jsonl,
the tool's output for the commit before it)."""
import importlib.util
import json
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('pass_loop_waits', os.path.join(ROOT, 'tools', 'pass_loop_waits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def rows():
    tool = _tool()
    hipcc = tool.makefile_flags(os.path.join(ROOT, 'matlab-code_amd', 'csrc'))[0]
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip('no hipcc: the pass kernels cannot be compiled to assembly here')
    out = tool.run()
    for r in out:
        print(json.dumps(r))
    return out


def test_every_pass_kernel_is_found(rows):
    names = {r['kernel'] for r in rows}
    want = ({'contract16_f32<1,true,true>', 'contract16_f32<1,false,true>', 'contract16_f32<2,false,false>',
             'contract16_f32<2,true,false>', 'contract16_f32<3,false,false>', 'contract16_f32<3,true,false>',
             'contract16_f32<4,false,false>'} |
            {'contract_f64<%d,%s>' % (nt, ex) for nt in (1, 2, 3) for ex in ('true', 'false')} | {'contract_f64<4,false>'} |
            {'contract16_f16<%d>' % nt for nt in (1, 2, 3, 4)})
    assert names == want, names ^ want
    for r in rows:
        assert r['mfma'] > 0 and r['loads'] > 0 and r['vmcnt'], r
        assert r['loads'] % r['ring_stages'] == 0, r
    head = next(r for r in rows if r['kernel'] == 'contract16_f32<1,true,true>')
    assert (head['loads'], head['loads_per_stage'], head['mfma']) == (21, 7, 48), head


def test_three_stage_rings_wait_for_no_more_than_one_stage(rows):
    for r in rows:
        if r['ring_stages'] == 3:
            assert min(r['vmcnt']) >= r['loads_per_stage'], r


def test_two_stage_fp64_ring_keeps_one_stage_in_flight(rows):
    two = [r for r in rows if r['ring_stages'] == 2]
    assert sorted(r['kernel'] for r in two) == ['contract_f64<%d,true>' % nt for nt in (1, 2, 3)]
    for r in two:
        nt = int(r['kernel'].split('<')[1].split(',')[0])
        assert r['loads_per_stage'] == 8 + nt, r
        assert min(r['vmcnt']) >= 8 + nt, r


def test_no_scratch_and_no_lost_occupancy(rows):
    with open(os.path.join(ROOT, 'profiles', 'pass_loop_waits_parent.jsonl')) as f:
        parent = {r['kernel']: r for r in map(json.loads, f)}
    assert set(parent) == {r['kernel'] for r in rows}
    for r in rows:
        assert r['scratch'] == 0, r
        assert r['occupancy'] >= parent[r['kernel']]['occupancy'], (r, parent[r['kernel']])
