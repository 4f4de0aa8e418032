#!/usr/bin/env python
"""Write tests/golden/pipeline_schedule.json: for every case of tests/_pipeline_trace.py's CASES, what
FramePairPipeline enqueues over the recording stand-ins -- per API call and per stream the number of entries and the
SHA-1 of their text (schedule_digest()).  Needs no GPU and nothing but this repository:

    python tests/golden/make_pipeline_schedule.py

The file is the record of the schedule as it was when it was last changed ON PURPOSE.  Regenerating it is legitimate
in a pull request that means to change the schedule -- another order on a stream, another wait, another buffer -- and
says so; it is then written from that pull request's code and reviewed as a change of behaviour.  A pull request that
only moves code around (a refactor) must pass tests/test_pipeline_schedule.py against the file as it stands; if it
renames an attribute of the pipeline, roles() in tests/_pipeline_trace.py maps the new name back to the old one."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root
import _pipeline_trace as pt  # noqa: E402


def main():
    out = {}
    for name in sorted(pt.CASES):
        with pytest.MonkeyPatch.context() as mp:
            pipe, trace, calls, extra = pt.run_case(name, mp)
            bad = pt.races(pipe, trace)
            if bad:
                raise SystemExit('%s: unordered launches %s' % (name, sorted(bad)))
            out[name] = pt.schedule_digest(pipe, trace, calls, extra)
        print('%-30s %3d calls %6d entries' % (name, len(calls), len(trace)))
    with open(os.path.join(HERE, 'pipeline_schedule.json'), 'w') as f:
        json.dump(out, f, sort_keys=True, separators=(',', ':'))
        f.write('\n')


if __name__ == '__main__':
    main()
