"""What FramePairPipeline really enqueues, traced without a GPU: the pipeline is built over recording stand-ins for the
contexts, the device arrays, dodt_amd.ops and the extractors, driven through push_frame() / run(), and every launch is
logged with its stream, the buffers it touches and a vector clock (a wait for a mark or a stream merges the clock the
other stream had there).  Two launches that touch the same shared buffer, at least one of them writing, on different
streams must be ordered by those waits.  Checked for sequence mode's rings and parity buffers -- with and without
look-ahead, with finish() in between, over two sequences, from pinned memory -- and, so that the tracer's silence means
something, for pair mode (no race) and for shallower rings (the races DESIGN section 8d names)."""
import functools

import pytest

from _pipeline_trace import _heads, _frame, install, races
from dodt_amd import pipeline as pl


@pytest.fixture
def build(monkeypatch):
    """build(**kw) -> (pipeline, trace, contexts) over the stand-ins of tests/_pipeline_trace.py."""
    return install(monkeypatch)


def _drive(pipe, keyframes, lookahead, finish_every=0, host=False):
    push = pipe.push_frame_from_host if host else pipe.push_frame
    frames = [_frame(pipe) for _ in range(keyframes)]
    heads = _heads(pipe)
    for j, fr in enumerate(frames):
        la = frames[j + 1] if lookahead and j + 1 < keyframes else None
        ret = push(*fr, heads=heads if j else None, lookahead=la)
        assert (ret is None) == (j == 0)
        if finish_every and j and j % finish_every == 0:
            pipe.finish()                          # (a look-ahead may stand announced behind it)
    pipe.finish()
    assert pipe.end_sequence() is None


@pytest.mark.parametrize('host', [False, True])
@pytest.mark.parametrize('finish_every', [0, 1, 3])
@pytest.mark.parametrize('lookahead', [False, True])
def test_sequence_mode_orders_every_shared_buffer(build, lookahead, finish_every, host):
    pipe, trace, _ = build(sequence=True)
    _drive(pipe, 14, lookahead, finish_every, host)
    _drive(pipe, 5, lookahead, finish_every, host)          # a second sequence primes over the first
    _drive(pipe, 4, not lookahead, 0, host)
    assert races(pipe, trace) == set()
    ops_seen = {t['op'] for t in trace}
    assert {'bev_slices', 'anchor_filter', 'forward_device_padded', 'crop_and_resize', 'nms'} <= ops_seen
    assert ('upload_async' in ops_seen) == host and ('gather_rows' in ops_seen) == (not host)


def test_sequence_step_launches_one_image_forward_and_three_voxelisations(build):
    """Per step: the BEV net once (two frames), the image net once (one frame), the new frame's full prep and the
    carried frame's plain voxelisation -- against pair mode's two of everything."""
    def count(trace, start):
        out = {}
        for t in trace[start:]:
            out[t['op'], t['stream']] = out.get((t['op'], t['stream']), 0) + 1
        return out
    seq, strace, _ = build(sequence=True)
    pair, ptrace, _ = build()
    assert seq.img_net.batch == 1 and seq.bev_net.batch == 2 and pair.img_net.batch == 2
    assert seq.flops_per_step() == 300.0 and pair.flops_per_step() == 400.0
    heads = _heads(seq)
    seq.push_frame(*_frame(seq))
    seq.push_frame(*_frame(seq), heads=heads)
    n = len(strace)
    seq.push_frame(*_frame(seq), heads=heads)
    got = count(strace, n)
    fr = [_frame(pair) for _ in range(2)]
    args = [list(a) for a in zip(*fr)]
    pair.run(*args, heads=heads)
    n = len(ptrace)
    pair.run(*args, heads=heads)
    want = count(ptrace, n)
    assert got['forward_device_padded', 'main'] == want['forward_device_padded', 'main'] == 1
    assert got['forward_device_padded', 'img'] == want['forward_device_padded', 'img'] == 1
    assert got['bev_slices', 'c0'] == got['bev_slices', 'c1'] == 1
    assert ('anchor_filter', 'c0') not in got and ('img_preprocess', 'c0') not in got
    assert got['anchor_filter', 'c1'] == got['project_anchors_f64', 'c1'] == got['img_preprocess', 'c1'] == 1
    assert want['anchor_filter', 'c0'] == want['img_preprocess', 'c0'] == 1
    # the tails are the same launches, stream by stream
    tail_ops = ('crop_and_resize', 'rpn_decode', 'nms', 'gather_project', 'final_decode', 'pack_detections')
    for op in tail_ops:
        for c in ('c0', 'c1'):
            assert got[op, c] == want[op, c], (op, c)


def test_pair_mode_is_traced_without_a_race(build):
    """The tracer on the code it was not written for: run() with and without look-ahead."""
    pipe, trace, _ = build()
    heads = _heads(pipe)
    steps = [[list(a) for a in zip(*[_frame(pipe) for _ in range(2)])] for _ in range(12)]
    for k, s in enumerate(steps):
        pipe.run(*s, heads=heads, lookahead=steps[k + 1] if k % 5 and k + 1 < len(steps) else None)
        if k == 6:
            pipe.finish()
    pipe.finish()
    assert races(pipe, trace) == set()


@pytest.mark.parametrize('lookahead', [False, True])
def test_two_image_slots_race(build, monkeypatch, lookahead):
    monkeypatch.setattr(pl, 'IMG_RING', 2)
    monkeypatch.setattr(pl, 'sequence_slots', functools.partial(pl.sequence_slots, img_ring=2))
    pipe, trace, _ = build(sequence=True)
    _drive(pipe, 12, lookahead)
    bad = races(pipe, trace)
    assert bad and all(b[0].startswith('img_ring') for b in bad)
    assert any(b[1:] == ('forward_device_padded on img', 'crop_and_resize on c0') for b in bad)


def test_three_prep_sets_race_under_lookahead(build, monkeypatch):
    monkeypatch.setattr(pl, 'PREP_RING', 3)
    monkeypatch.setattr(pl, 'sequence_slots', functools.partial(pl.sequence_slots, prep_ring=3))
    pipe, trace, _ = build(sequence=True)
    _drive(pipe, 12, True)
    bad = races(pipe, trace)
    assert bad and all(b[0].startswith('prep_sets') for b in bad)
    assert any(b[1].endswith('on c1') and b[2].endswith('on c0') for b in bad)      # new prep under frame 0's tail
    pipe, trace, _ = build(sequence=True)
    _drive(pipe, 12, False)
    assert races(pipe, trace) == set()              # (pair mode's depth holds without look-ahead)
