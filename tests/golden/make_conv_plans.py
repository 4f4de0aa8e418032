#!/usr/bin/env python
"""Write tests/golden/conv_plans.json: for every configuration of tests/_conv_cases.py's pin_configs() -- the case
table, the bench rows in every mode their data type can feel, the bench shapes over batch sizes and CU counts -- what
the conv planner (pick_variant, plan_layer, plan_convs in conv.hip) decides per layer: the main and the tail variant
by signature (interned: the variant table's indices shift when entries come and go), items, grid, pool_fused,
bneck_fused, folded.  Needs no GPU, only the built library:

    python tests/golden/make_conv_plans.py

The file is the record of the planner's choices as they were when they were last changed ON PURPOSE.  Regenerating it
is legitimate in a pull request that means to change a choice -- another rule, another threshold, another kernel for
a layer -- and says so; it is then written from that pull request's code and reviewed as a change of behaviour.  A
pull request that only moves selection code around or removes table entries must pass
tests/test_conv_plan.py::test_plans_are_the_pinned_plans against the file as it stands."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root
import _conv_cases as cc  # noqa: E402


def dumps(pinned):
    """One configuration per line, so that a changed choice shows as a changed line."""
    rows = ['"%s":%s' % (k, json.dumps(v, separators=(',', ':'))) for k, v in pinned['plans'].items()]
    head = json.dumps(dict(signatures=pinned['signatures'], layers=pinned['layers']), indent=1)
    return head[:-2] + ',\n "plans": {\n  ' + ',\n  '.join(rows) + '\n }\n}\n'


def main():
    pinned = cc.pinned_plans()
    text = dumps(pinned)
    assert json.loads(text) == json.loads(json.dumps(pinned))
    with open(os.path.join(HERE, 'conv_plans.json'), 'w') as f:
        f.write(text)
    print('%d configurations, %d signatures, %d bytes' % (len(pinned['plans']), len(pinned['signatures']), len(text)))


if __name__ == '__main__':
    main()
