#!/usr/bin/env python3
"""Records tests/golden/sparse_team_bits.json: one sha256 per output array of every case of
tests/test_gpu_sparse_team_bits.py, from the library this tree has built.  Run it on an MI355X from a build of the
commit whose bits are the reference; the test then holds later builds to them.  Every case is computed twice and must
agree with itself before it is written.

    python tools/record_sparse_team_bits.py [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import test_gpu_sparse_team_bits as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--out', default=T.FIXTURE)
    args = ap.parse_args()
    pkg = importlib.import_module('matlab-code_amd')
    fixture = {}
    with pkg.Engine(0) as eng:
        for case in T.CASES:
            first, second = T.hashes(pkg, eng, case), T.hashes(pkg, eng, case)
            if first != second:
                sys.exit('%s: two runs differ in %s' % (T.case_id(case), [k for k in first if first[k] != second[k]]))
            fixture[T.case_id(case)] = first
            print('%s: %d arrays' % (T.case_id(case), len(first)), flush=True)
    with open(args.out, 'w') as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d cases' % (args.out, len(fixture)))


if __name__ == '__main__':
    main()
