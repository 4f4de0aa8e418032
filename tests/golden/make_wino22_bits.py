#!/usr/bin/env python
"""Write tests/golden/wino22_bits.json: the sha256 and the shape of every output map -- every layer, the returned
feature map, the bottleneck -- of the cases of tests/test_gpu_wino22_bits.py, which run the fp32 nets on the
F(2x2,3x3) Winograd kernel.  Needs an MI355X and the built library:

    [DODT_HIP_LIB=<another build of the library>] python tests/golden/make_wino22_bits.py [--out FILE]

The file is the record of the kernel's results BIT FOR BIT.  It was written from the library as it stood before the
kernel's K loop was hand-ordered (built into a second file, selected with DODT_HIP_LIB); a change that reorders
instructions, moves registers or removes redundant work must pass tests/test_gpu_wino22_bits.py against the file
as it stands.  Regenerating it is legitimate only in a pull request that means to change the kernel's arithmetic
-- another summation order, another transform -- and says so."""
import argparse
import collections
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root
import _conv_cases as cc  # noqa: E402
import test_gpu_wino22_bits as t  # noqa: E402


def dumps(cases):
    """One map per line, so that a changed map shows as a changed line."""
    out = []
    for cid, maps in cases.items():
        rows = ['   "%s": %s' % (n, json.dumps(v, separators=(',', ':'))) for n, v in maps.items()]
        out.append('  "%s": {\n%s\n  }' % (cid, ',\n'.join(rows)))
    return '{\n "cases": {\n' + ',\n'.join(out) + '\n }\n}\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'wino22_bits.json'))
    args = ap.parse_args()
    got = {}
    for mode in collections.OrderedDict.fromkeys(c.mode for c in t.CASES):     # each mode in a child of its own
        got.update(t.digests_in_child(mode))
    cases = collections.OrderedDict((cc.case_id(c), got[cc.case_id(c)]) for c in t.CASES)
    text = dumps(cases)
    assert json.loads(text) == {'cases': json.loads(json.dumps(cases))}
    with open(args.out, 'w') as f:
        f.write(text)
    print('%d cases, %d maps, %d bytes, library %s' % (len(cases), sum(len(m) for m in cases.values()), len(text),
                                                      os.environ.get('DODT_HIP_LIB', '(the tree\'s)')))


if __name__ == '__main__':
    main()
