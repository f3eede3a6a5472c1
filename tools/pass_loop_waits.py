#!/usr/bin/env python3
"""Wait counts of the tensor-pass kernels' steady loops, read from the compiled gfx950 code.

Compiles matlab-code_amd/csrc/contract.hip to assembly (device side only: no GPU is needed) with the flags of
csrc/Makefile and prints one JSON line per tensor-pass kernel (contract16_f32, contract_f64, contract16_f16; every
instantiation):

  kernel          demangled-enough name, e.g. contract16_f32<1,true,true>
  ring_stages     stages of the register ring (3; 2 in the fp64 form with leftover columns)
  mfma            MFMA instructions of the steady loop: the innermost loop with the most of them
  loads           vector memory loads of one revolution of that loop
  loads_per_stage loads / ring_stages
  vmcnt           the operand of every `s_waitcnt vmcnt(N)` of the loop, in loop order
  vgprs, scratch, occupancy   from the kernel's metadata

A ring keeps its stages in flight only if no wait of the loop asks for fewer outstanding loads than one stage holds:
min(vmcnt) >= loads_per_stage.  The tool looks at wait counts, loads and MFMAs only.

  python tools/pass_loop_waits.py                  # the working tree
  python tools/pass_loop_waits.py --parent HEAD~1  # another revision's csrc/ and include/
"""
import argparse
import io
import json
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('matlab-code_amd', 'csrc')

PASS_KERNELS = ('contract16_f32', 'contract_f64', 'contract16_f16')


def makefile_flags(csrc):
    """HIPCC, ARCH and CXXFLAGS as csrc/Makefile sets them (environment overrides HIPCC and ARCH, as make does)."""
    text = open(os.path.join(csrc, 'Makefile')).read()

    def var(name):
        m = re.search(r'^%s\s*\??=\s*(.*)$' % name, text, re.M)
        return m.group(1).strip() if m else ''

    hipcc = os.environ.get('HIPCC') or var('HIPCC')
    arch = os.environ.get('ARCH') or var('ARCH')
    flags = var('CXXFLAGS').replace('$(ARCH)', arch).split()
    return hipcc, flags


def compile_to_asm(csrc, out):
    hipcc, flags = makefile_flags(csrc)
    cmd = [hipcc] + flags + ['--cuda-device-only', '-S', os.path.join(csrc, 'contract.hip'), '-o', out]
    subprocess.run(cmd, check=True, cwd=csrc)


def checkout_revision(rev, dest):
    """csrc/ and include/ of a revision, laid out as in the repository (contract.hip includes ../../include)."""
    data = subprocess.run(['git', 'archive', rev, CSRC, 'include'], check=True, cwd=ROOT, stdout=subprocess.PIPE).stdout
    with tarfile.open(fileobj=io.BytesIO(data)) as tar:
        tar.extractall(dest)
    return os.path.join(dest, CSRC)


def pretty_name(sym):
    """_ZN6aoadmm14contract16_f32ILi1ELb1ELb1EEEvNS_5KArgsE -> contract16_f32<1,true,true>"""
    m = re.match(r'_ZN6aoadmm\d+([A-Za-z0-9_]+?)I((?:L[ib]\d+E)+)E', sym)
    if not m:
        return sym
    args = []
    for kind, val in re.findall(r'L([ib])(\d+)E', m.group(2)):
        args.append(val if kind == 'i' else ('true' if val == '1' else 'false'))
    return '%s<%s>' % (m.group(1), ','.join(args))


def ring_stages(name):
    m = re.match(r'contract_f64<\d+,(true|false)>', name)
    return 2 if m and m.group(1) == 'true' else 3


def kernels_of(asm_lines):
    """{symbol: (body lines, metadata dict)} for every kernel of the file."""
    out = {}
    i, n = 0, len(asm_lines)
    while i < n:
        m = re.match(r'^(_Z\w+):\s*; @', asm_lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        j = i + 1
        while j < n and not asm_lines[j].lstrip().startswith('.amdhsa_kernel'):
            j += 1
        body = asm_lines[i + 1:j]
        meta = {}
        k = j
        while k < n and not re.match(r'^_Z\w+:\s*; @', asm_lines[k]):
            mm = re.match(r'^; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy): (\d+)', asm_lines[k])
            if mm:
                meta[mm.group(1)] = int(mm.group(2))
                if mm.group(1) == 'Occupancy':
                    break
            k += 1
        out[sym] = (body, meta)
        i = k
    return out


def is_instr(line):
    s = line.strip()
    return bool(s) and not s.startswith((';', '.', '//')) and not s.endswith(':') and not re.match(r'^\.?\w+:', s)


def steady_loop(body):
    """The innermost loop with the most MFMA instructions: (mfma count, its instructions in loop order).

    The compiler marks every basic block of a loop in a comment: `=>This Inner Loop Header` on the header's label and
    `in Loop: Header=BBn_m` on the others (labelled `.LBBn_m:` or, for fall-through blocks, `; %bb.k:`).  A rotated loop
    may have its latch block placed in front of its header, so membership is taken from these marks, not from the span
    between the header and a back branch; loop order is the header first, then the blocks after it, then those in front."""
    blocks = []                                       # [label or None, comment, [lines]]
    for line in body:
        m = re.match(r'^(\.LBB\d+_\d+):(.*)$', line) or re.match(r'^; (%bb\.\d+):(.*)$', line)
        if m:
            blocks.append([m.group(1), m.group(2), []])
        elif blocks:
            blocks[-1][2].append(line)
    best = None
    for hi, (lab, comment, _) in enumerate(blocks):
        if 'Inner Loop Header' not in comment:
            continue
        mark = 'Header=%s ' % lab[2:]                 # .LBB16_12 -> BB16_12
        members = [k for k, b in enumerate(blocks) if k == hi or mark in b[1] + ' ']
        order = [k for k in members if k >= hi] + [k for k in members if k < hi]
        lines = [l.split(';')[0].strip() for k in order for l in blocks[k][2] if is_instr(l)]
        mfma = sum(1 for l in lines if l.startswith('v_mfma'))
        if best is None or mfma > best[0]:
            best = (mfma, lines)
    return best


def analyse(asm_path):
    with open(asm_path) as f:
        asm = f.read().splitlines()
    rows = []
    for sym, (body, meta) in kernels_of(asm).items():
        name = pretty_name(sym)
        if not name.startswith(tuple(k + '<' for k in PASS_KERNELS)):
            continue
        loop = steady_loop(body)
        if loop is None:
            raise SystemExit('no loop found in %s' % name)
        mfma, lines = loop
        loads = sum(1 for l in lines if re.match(r'^(global|flat|buffer)_load_', l))
        waits = []
        for l in lines:
            if l.startswith('s_waitcnt'):
                m = re.search(r'vmcnt\((\d+)\)', l)
                if m:
                    waits.append(int(m.group(1)))
        stages = ring_stages(name)
        rows.append(dict(kernel=name, ring_stages=stages, mfma=mfma, loads=loads, loads_per_stage=loads // stages,
                         vmcnt=waits, min_vmcnt=min(waits) if waits else None,
                         vgprs=meta.get('TotalNumVgprs', meta.get('NumVgprs')), scratch=meta.get('ScratchSize'),
                         occupancy=meta.get('Occupancy')))
    rows.sort(key=lambda r: r['kernel'])
    return rows


def run(parent=None):
    """The rows of the working tree, or of revision `parent`."""
    tmp = tempfile.mkdtemp(prefix='pass_loop_waits_')
    try:
        csrc = checkout_revision(parent, tmp) if parent else os.path.join(ROOT, CSRC)
        asm = os.path.join(tmp, 'contract.s')
        compile_to_asm(csrc, asm)
        rows = analyse(asm)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for r in rows:
        r['revision'] = parent or 'worktree'
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent', metavar='REV', help='analyse this git revision instead of the working tree')
    ap.add_argument('--asm', metavar='FILE', help='analyse an assembly file that exists already (no compile)')
    args = ap.parse_args()
    rows = analyse(args.asm) if args.asm else run(args.parent)
    for r in rows:
        print(json.dumps(r))
    return 0


if __name__ == '__main__':
    sys.exit(main())
