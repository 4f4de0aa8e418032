"""resolve_schedule(): the pipeline's switches and the T branch's placement, from an environment and how the pipeline was
built.  And the schedule FramePairPipeline enqueues, pinned: every case of tests/_pipeline_trace.py's CASES is run over
the recording stand-ins and compared with tests/golden/pipeline_schedule.json (written by
tests/golden/make_pipeline_schedule.py) -- per API call and per stream what was enqueued, with which buffers, behind
which recording of which mark; in pair mode, the benchmark's path, also the order in which each call fed the streams,
which is part of its speed.  No case has two unordered launches on a buffer that streams share.  No device."""
import json
import os

import pytest

import _pipeline_trace as pt
from dodt_amd.pipeline import resolve_schedule

# (computed heads, frames per sample, environment, T form, side streams) -> (placement, frames of a pair alternate)
ROWS = [
    # injected heads, or single frames: no T branch whatever else is set
    (False, 2, {}, 'proposals', 2, ('none', False)),
    (False, 2, {}, 'detections', 2, ('none', False)),
    (False, 1, {}, 'proposals', 1, ('none', False)),
    (True, 1, {}, 'proposals', 2, ('none', False)),
    (True, 1, {}, 'detections', 2, ('none', False)),
    (True, 1, {'DODT_PIPE_CORR_MAP': 'f1'}, 'proposals', 2, ('none', False)),
    # DODT_PIPE_NO_CORR
    (True, 2, {'DODT_PIPE_NO_CORR': '1'}, 'detections', 2, ('none', True)),
    (True, 2, {'DODT_PIPE_NO_CORR': '1'}, 'detections', 4, ('none', True)),
    (True, 2, {'DODT_PIPE_NO_CORR': '1'}, 'detections', 1, ('none', False)),
    (True, 2, {'DODT_PIPE_NO_CORR': '1'}, 'proposals', 2, ('none', False)),
    (True, 2, {'DODT_PIPE_NO_CORR': '1'}, 'proposals', 1, ('none', False)),
    (True, 2, {'DODT_PIPE_NO_CORR': '1', 'DODT_PIPE_CORR_MAP': 'f1'}, 'proposals', 2, ('none', False)),
    # the kept detections' rows
    (True, 2, {}, 'detections', 2, ('detections', True)),
    (True, 2, {}, 'detections', 3, ('detections', True)),
    (True, 2, {}, 'detections', 1, ('detections', False)),
    (True, 2, {'DODT_PIPE_CORR_MAP': 'f1'}, 'detections', 2, ('detections', True)),
    (True, 2, {'DODT_PIPE_NO_CORR': ''}, 'detections', 2, ('detections', True)),
    # every proposal's rows
    (True, 2, {}, 'proposals', 2, ('img', False)),
    (True, 2, {'DODT_PIPE_CORR_MAP': 'img'}, 'proposals', 2, ('img', False)),
    (True, 2, {'DODT_PIPE_NO_CORR': ''}, 'proposals', 2, ('img', False)),
    (True, 2, {'DODT_PIPE_CORR_MAP': 'f1'}, 'proposals', 2, ('f1', False)),
    (True, 2, {'DODT_PIPE_CORR_MAP': 'f0'}, 'proposals', 2, ('f1', False)),
    (True, 2, {'DODT_PIPE_CORR_MAP': ''}, 'proposals', 2, ('f1', False)),
    (True, 2, {'DODT_PIPE_CORR_MAP': 'f1'}, 'proposals', 4, ('f1', False)),
    (True, 2, {}, 'proposals', 1, ('f0', False)),
    (True, 2, {'DODT_PIPE_CORR_MAP': 'f1'}, 'proposals', 1, ('f0', False)),
    (True, 2, {'DODT_PIPE_CORR_MAP': 'img'}, 'proposals', 1, ('f0', False)),
]


@pytest.mark.parametrize('computed,fps,env,form,n_side,want', ROWS)
def test_placement_table(computed, fps, env, form, n_side, want):
    assert resolve_schedule(env, computed, fps, n_side).t_placement(form) == want


@pytest.mark.parametrize('env,want', [({}, True), ({'DODT_PIPE_FUSED_TAIL': '1'}, True),
                                      ({'DODT_PIPE_FUSED_TAIL': '0'}, False), ({'DODT_PIPE_FUSED_TAIL': ''}, True),
                                      ({'DODT_PIPE_FUSED_TAIL': 'no'}, True)])
def test_fused_tail_is_off_for_0_only(env, want):
    assert resolve_schedule(env, True, 2, 2).fused_tail is want


def test_diagnostic_switches_are_set_by_any_non_empty_value():
    s = resolve_schedule({}, True, 2, 2)
    assert (s.no_tail, s.no_corr, s.no_rpn) == (False, False, False)
    s = resolve_schedule({'DODT_PIPE_NO_TAIL': '', 'DODT_PIPE_NO_CORR': '', 'DODT_PIPE_NO_RPN': ''}, True, 2, 2)
    assert (s.no_tail, s.no_corr, s.no_rpn) == (False, False, False)
    assert resolve_schedule({'DODT_PIPE_NO_TAIL': '1'}, True, 2, 2)[1:4] == (True, False, False)
    assert resolve_schedule({'DODT_PIPE_NO_CORR': '0'}, True, 2, 2)[1:4] == (False, True, False)
    assert resolve_schedule({'DODT_PIPE_NO_RPN': 'x'}, True, 2, 2)[1:4] == (False, False, True)


def test_removed_switches_change_nothing():
    removed = {'DODT_PIPE_TAIL_SETS': '2', 'DODT_PIPE_STREAMS': 'conv', 'DODT_PIPE_PRIO': '1',
               'DODT_PIPE_EARLY_PREP': '0', 'DODT_PIPE_IMG_WAIT': 'none', 'DODT_PIPE_CORR_ON_F1': '0'}
    for env in ({}, {'DODT_PIPE_CORR_MAP': 'f1', 'DODT_PIPE_FUSED_TAIL': '0'}, {'DODT_PIPE_NO_CORR': '1'}):
        for computed, fps, n_side in ((True, 2, 2), (True, 2, 1), (False, 2, 2), (True, 1, 1)):
            want = resolve_schedule(env, computed, fps, n_side)
            got = resolve_schedule(dict(env, **removed), computed, fps, n_side)
            assert got == want
            for form in ('proposals', 'detections'):
                assert got.t_placement(form) == want.t_placement(form)
    # ... and in particular the default placement stays 'img' (DODT_PIPE_CORR_ON_F1=0 used to give 'f0')
    assert resolve_schedule(removed, True, 2, 2).t_placement('proposals') == ('img', False)


def test_schedule_is_immutable_and_reads_the_process_environment_by_default(monkeypatch):
    monkeypatch.setenv('DODT_PIPE_CORR_MAP', 'f1')
    monkeypatch.delenv('DODT_PIPE_FUSED_TAIL', raising=False)
    s = resolve_schedule(None, True, 2, 2)
    assert s.t_placement('proposals') == ('f1', False) and s.fused_tail
    with pytest.raises(AttributeError):
        s.fused_tail = False


# ---- the schedule itself ---------------------------------------------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pipeline_schedule.json')


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(pt.CASES)


@pytest.mark.parametrize('name', sorted(pt.CASES))
def test_schedule_equals_the_fixture(name, golden, monkeypatch):
    pipe, trace, calls, extra = pt.run_case(name, monkeypatch)
    got, want = pt.schedule_digest(pipe, trace, calls, extra), golden[name]
    assert [c['call'] for c in got['calls']] == [c['call'] for c in want['calls']]
    text = pt.canonical(pipe, trace, extra)
    for (label, start, end), g, w in zip(calls, got['calls'], want['calls']):
        for s in pt.STREAMS:
            # (a) per stream, call by call: the entries and their digest
            if g['streams'].get(s) != w['streams'].get(s):
                mine = [pt.entry_text(t, pt.roles(pipe, extra)) for t in trace[start:end] if t['stream'] == s]
                pytest.fail('%s, call %r, stream %s: enqueued %s, the fixture has %s; enqueued now:\n%s'
                            % (name, label, s, g['streams'].get(s), w['streams'].get(s), '\n'.join(mine)))
        # (b) pair mode: the order across the streams
        if name in pt.PAIR_MODE:
            assert g['order'] == w['order'], '%s, call %r: the order in which the streams were fed' % (name, label)
    assert got['marks'] == want['marks'], '%s: the timing marks' % name
    assert sum(len(v) for v in text.values()) == len(trace)
    # (c) every shared buffer is ordered
    assert pt.races(pipe, trace) == set()
    assert pipe.pending is None
