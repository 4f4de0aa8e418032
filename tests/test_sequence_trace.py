"""What FramePairPipeline really enqueues, traced without a GPU: the pipeline is built over recording stand-ins for the
contexts, the device arrays, dodt_amd.ops and the extractors, driven through push_frame() / run(), and every launch is
logged with its stream, the buffers it touches and a vector clock (a wait for a mark or a stream merges the clock the
other stream had there).  Two launches that touch the same shared buffer, at least one of them writing, on different
streams must be ordered by those waits.  Checked for sequence mode's rings and parity buffers -- with and without
look-ahead, with finish() in between, over two sequences, from pinned memory -- and, so that the tracer's silence means
something, for pair mode (no race) and for shallower rings (the races DESIGN section 8d names)."""
import functools
import types

import numpy as np
import pytest

from dodt_amd import config
from dodt_amd import pipeline as pl

STREAMS = ('main', 'img', 'c0', 'c1')
# array arguments an op WRITES, by position among its array arguments; every other array argument is read
WRITES = {'bev_slices': (1, 2), 'anchor_filter': (2, 3), 'project_anchors_f64': (3, 4, 5), 'img_preprocess': (1,),
          'gather_rows': (2,), 'forward_device_padded': (1, 2), 'upload_async': (0,), 'correlation': (2,)}


class Array(object):
    _next = [1 << 20]

    def __init__(self, shape, dtype=np.float32, base=None, ptr=None):
        self.shape, self.dtype = tuple(int(s) for s in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        if base is None:
            ptr = Array._next[0]
            Array._next[0] += (self.nbytes + 255) // 256 * 256 + 256
        self.base, self.ptr = base or self, ptr

    def offset(self, nbytes, shape, dtype=None):
        v = Array(shape, dtype or self.dtype, base=self.base, ptr=self.ptr + int(nbytes))
        assert v.ptr + v.nbytes <= self.base.ptr + self.base.nbytes, 'view past the end of its allocation'
        return v

    def upload_async(self, pinned, ctx=None, nbytes=None):
        ctx.log('upload_async', [self])
        return self

    def upload(self, host):
        return self

    def zero(self):
        return self


class Ctx(object):
    device_id, lib = 0, None

    def __init__(self, name, trace):
        self.name, self.trace, self.marks = name, trace, {}
        self.clock = {s: 0 for s in STREAMS}

    def log(self, op, arrays):
        self.clock[self.name] += 1
        self.trace.append(dict(stream=self.name, index=self.clock[self.name], clock=dict(self.clock), op=op,
                               arrays=[a for a in arrays if isinstance(a, Array)]))

    def _merge(self, clock):
        for s in STREAMS:
            self.clock[s] = max(self.clock[s], clock[s])

    def mark(self, slot):
        self.marks[slot] = dict(self.clock)

    def wait_mark(self, other, slot):
        self._merge(other.marks[slot])             # (KeyError: a mark never recorded, an error on the device too)

    def wait_for(self, other):
        self._merge(other.clock)

    def empty(self, shape, dtype=np.float32):
        return Array(shape, dtype)

    zeros = empty

    def array(self, host, dtype=None):
        host = np.asarray(host)
        return Array(host.shape, dtype or host.dtype)

    def sync(self):
        pass


class Ops(object):
    """dodt_amd.ops: every launch is logged on the context it is given."""

    def make_bev_params(self, *a, **k):
        return types.SimpleNamespace(point_format=0)

    def with_ego_motion(self, bp, trans, matrix):
        return bp

    def fetch_i32_end(self, ctx, slot, n):
        return [5000] * n

    def __getattr__(self, name):
        def launch(ctx, *args, **kw):
            ctx.log(name, list(args) + list(kw.values()))
        return launch


def _net(hwc):
    class Net(object):
        PAD_TOP, _R_MEAN, _G_MEAN, _B_MEAN = 4, 1.0, 2.0, 3.0

        def __init__(self, ctx=None, shared_gpu=False, conv_dtype='f32'):
            self.ctx = ctx

        def load_params(self, params):
            pass

        def _ensure(self, batch, h, w, c):
            self.batch = batch

        def output_shape(self):
            return hwc

        def forward_device_padded(self, d_x, d_feat, d_bneck=None):
            self.ctx.log('forward_device_padded', [d_x, d_feat, d_bneck])

        def flops(self):
            return 100.0 * self.batch
    return Net


@pytest.fixture
def build(monkeypatch):
    """build(**kw) -> (pipeline, trace, contexts) over the stand-ins."""
    monkeypatch.setattr(pl, 'ops', Ops())
    monkeypatch.setitem(pl.EXTRACTORS, 'vgg_pyr', (_net((700, 800, 32)), _net((360, 1200, 32))))

    def make(**kw):
        trace = []
        c = {s: Ctx(s, trace) for s in STREAMS}
        streams = types.SimpleNamespace(img_ctx=c['img'], sides=[c['c0'], c['c1']])
        pipe = pl.FramePairPipeline(c['main'], config.PYRAMID_DODT, {}, {}, reuse_streams_of=streams,
                                    bev_input_skip=False, **kw)
        return pipe, trace, c
    return make


def _shared(pipe):
    """The buffers more than one stream touches, by allocation: name of each."""
    names = {}
    for i in range(2):
        names[id(pipe.in_bev[i])] = 'in_bev[%d]' % i
        names[id(pipe.in_img[i])] = 'in_img[%d]' % i
        for n, a in pipe.feat[i].items():
            names[id(a)] = 'feat[%d].%s' % (i, n)
    if pipe.sequence:
        for i, d in enumerate(pipe.img_ring):
            for n, a in d.items():
                names[id(a)] = 'img_ring[%d].%s' % (i, n)
        for i, d in enumerate(pipe.prep_sets):
            for n, a in d.items():
                names[id(a)] = 'prep_sets[%d].%s' % (i, n)
        for i, a in enumerate(pipe.pts_ring):
            names[id(a)] = 'pts_ring[%d]' % i
    else:
        for i, frames in enumerate(pipe.prep3):
            for f, d in enumerate(frames):
                for n, a in d.items():
                    names[id(a)] = 'prep3[%d][%d].%s' % (i, f, n)
    return names


def races(pipe, trace):
    """{(buffer, earlier op, later op)} of the unordered pairs; views of one allocation count when their bytes overlap."""
    names = _shared(pipe)
    touches = {}                                   # allocation -> [(launch, view, writes)]
    for t in trace:
        for i, a in enumerate(t['arrays']):
            if id(a.base) in names:
                touches.setdefault(id(a.base), []).append((t, a, i in WRITES.get(t['op'], ())))
    bad = set()
    for key, ts in touches.items():
        for i, (ta, a, wa) in enumerate(ts):
            for tb, b, wb in ts[i + 1:]:
                if ta['stream'] == tb['stream'] or not (wa or wb):
                    continue
                if a.ptr + a.nbytes <= b.ptr or b.ptr + b.nbytes <= a.ptr:
                    continue
                if tb['clock'][ta['stream']] < ta['index']:
                    bad.add((names[key], '%s on %s' % (ta['op'], ta['stream']), '%s on %s' % (tb['op'], tb['stream'])))
    return bad


def _frame(pipe):
    return Array((pipe.n_points_max, 4)), 30000, Array((375, 1242, 3), np.uint8)


def _heads(pipe):
    N, P = pipe.n_all, pipe.P
    return [dict(rpn_logits=Array((N, 2)), rpn_offsets=Array((N, 6)), cls_logits=Array((P, 2)),
                 offsets_4c=Array((P, 10)), angle_vectors=Array((P, 2)), corr_offsets=Array((P, 3))) for _ in range(2)]


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
