"""Recording stand-ins over which the real FramePairPipeline runs without a GPU (tests/test_sequence_trace.py,
tests/test_pipeline_schedule.py, tests/golden/make_pipeline_schedule.py): contexts, device arrays, dodt_amd.ops, the
extractors, the head classes and the tracker.  Every launch is logged with its stream, the buffers it touches and a
vector clock (a wait for a mark or a stream merges the clock the other stream had there); marks, waits and the host's
reads of a fetched count are logged as events, which do not advance a clock.
races(): two launches that touch the same shared buffer, at least one of them writing, on different streams must be
ordered by those waits.
canonical(): the schedule as text, per stream, every array named by its role on the pipeline and never by its address;
schedule_digest() of it is what tests/golden/pipeline_schedule.json pins, for the cases of CASES driven by run_case()."""
import hashlib
import types

import numpy as np

from dodt_amd import config
from dodt_amd import pipeline as pl

STREAMS = ('main', 'img', 'c0', 'c1')
# array arguments an op WRITES, by position among its array arguments; every other array argument is read
WRITES = {'bev_slices': (1, 2), 'anchor_filter': (2, 3), 'project_anchors_f64': (3, 4, 5), 'img_preprocess': (1,),
          'gather_rows': (2,), 'forward_device_padded': (1, 2), 'upload_async': (0,), 'correlation': (2,),
          # the tail ops that write the detection records (boxes, scores[, types], det_idx, det_count, records, counts)
          'pack_detections': (4, 5), 'pack_detections_compact': (4, 5),
          'pack_detections_classes': (5, 6), 'pack_detections_compact_classes': (5, 6)}


class Array(object):
    _next = [1 << 20]
    _allocations = []

    def __init__(self, shape, dtype=np.float32, base=None, ptr=None, owner=None):
        self.shape, self.dtype = tuple(int(s) for s in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        if base is None:
            ptr = Array._next[0]
            Array._next[0] += (self.nbytes + 255) // 256 * 256 + 256
            Array._allocations.append(self)
        self.base, self.ptr, self.owner = base or self, ptr, owner

    def offset(self, nbytes, shape, dtype=None):
        v = Array(shape, dtype or self.dtype, base=self.base, ptr=self.ptr + int(nbytes))
        assert v.ptr + v.nbytes <= self.base.ptr + self.base.nbytes, 'view past the end of its allocation'
        return v

    def upload_async(self, pinned, ctx=None, nbytes=None):
        ctx.log('upload_async', [self])
        return self

    def upload(self, host):
        if self.base.owner is not None:            # (a synchronous copy: an event on the context that made the array)
            self.base.owner.event('upload', (self,))
        return self

    def zero(self):
        return self


class Ctx(object):
    device_id, lib = 0, None

    def __init__(self, name, trace):
        self.name, self.trace, self.marks = name, trace, {}
        self.clock = {s: 0 for s in STREAMS}
        self.fetches = {}                          # fetch slot -> what fetch_i32_end will return

    def log(self, op, arrays, args=None, kw=None):
        self.clock[self.name] += 1
        self.trace.append(dict(stream=self.name, index=self.clock[self.name], clock=dict(self.clock), op=op,
                               arrays=[a for a in arrays if isinstance(a, Array)],
                               args=tuple(arrays if args is None else args), kw=dict(kw or {})))

    def event(self, op, detail, clock=None):
        """A mark, a wait or a host read: in the trace, on no clock (races() sees no arrays and passes over it)."""
        self.trace.append(dict(stream=self.name, event=True, op=op, arrays=[], args=tuple(detail), kw={},
                               clock=None if clock is None else dict(clock)))

    def _merge(self, clock):
        for s in STREAMS:
            self.clock[s] = max(self.clock[s], clock[s])

    def mark(self, slot):
        self.marks[slot] = dict(self.clock)
        self.event('mark', (slot,))

    def wait_mark(self, other, slot):
        self._merge(other.marks[slot])             # (KeyError: a mark never recorded, an error on the device too)
        self.event('wait_mark', (slot, other.name), other.marks[slot])

    def wait_for(self, other):
        self._merge(other.clock)
        self.event('wait_for', (other.name,), other.clock)

    def empty(self, shape, dtype=np.float32):
        return Array(shape, dtype, owner=self)

    zeros = empty

    def array(self, host, dtype=None):
        host = np.asarray(host)
        return Array(host.shape, dtype or host.dtype, owner=self)

    def wrap(self, ptr, shape, dtype=np.float32):
        """A view of the allocation that holds `ptr` (caller-owned memory is one of this module's arrays too)."""
        for a in Array._allocations:
            if a.ptr <= ptr < a.ptr + max(a.nbytes, 1):
                return a.offset(ptr - a.ptr, shape, dtype)
        raise ValueError('wrap: no allocation holds this pointer')

    def sync(self):
        pass


class Ops(object):
    """dodt_amd.ops: every launch is logged on the context it is given; what the pipeline calls on the host is here."""
    CORR_TILE_LIST_MAX = 8192

    def make_bev_params(self, *a, **k):
        return types.SimpleNamespace(point_format=0)

    def with_ego_motion(self, bp, trans, matrix):
        return types.SimpleNamespace(point_format=0, ego_motion=True)

    def correlation_tile_capacity(self, out_hw):
        return -(-int(out_hw[0]) // 16) * -(-int(out_hw[1]) // 16)

    def temporal_calib(self, r0_rect, tr_velo_to_cam):
        return np.zeros(42)

    def temporal_ego(self, ego, n_frames):
        return np.zeros((n_frames, 13))

    def fetch_i32_begin(self, ctx, d_src, n, slot):
        ctx.log('fetch_i32_begin', [d_src, n, slot])
        ctx.fetches[slot] = [1000 + ctx.clock[ctx.name]] * n          # (a count that names the fetch it came from)

    def fetch_i32_end(self, ctx, slot, n):
        got = ctx.fetches.get(slot, [5000] * n)
        ctx.event('fetch_i32_end', (slot, n, got[0]))
        return got

    def __getattr__(self, name):
        def launch(ctx, *args, **kw):
            ctx.log(name, list(args) + list(kw.values()), args, kw)
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


class Head(object):
    """AnchorPredictor and EarlyFusionFcLayers: `params` is the head's name; forward() is one launch on its context."""
    in_ld = 1232

    def __init__(self, ctx, params, outputs=None, dtype='f32'):
        self.ctx, self.name, self.outputs = ctx, params, outputs

    def make_scratch(self, rows):
        return [self.ctx.empty((rows, 8))]

    def forward(self, ctx, *args):
        flat = []
        for a in args:
            flat += list(a) if isinstance(a, (list, tuple)) else [a]
        ctx.log('head_' + self.name, flat)

    def flops(self, rows):
        return 1.0 * rows

    def close(self):
        pass


class Tracker(object):
    """tracking.Tracker: its launches logged on the context they are given; nothing is ever tracked."""

    def __init__(self, ctx=None, log_capacity=65536, high_threshold=0.5, iou_threshold=0.005, t_min=3,
                 score_threshold=0.1):
        self.ctx = ctx
        self.d_state = ctx.empty((64,), np.uint8)
        self.reset()

    def reset(self, ctx=None):
        (ctx or self.ctx).log('track_reset', [self.d_state])

    def flush(self, ctx=None):
        (ctx or self.ctx).log('track_flush', [self.d_state])

    def track_records(self, d_records, d_counts, n_pairs, max_det, p2, image_wh, ctx=None):
        (ctx or self.ctx).log('track_records', [self.d_state, d_records, d_counts, n_pairs, max_det])

    def read(self):
        return []


def install(monkeypatch):
    """Put the stand-ins in place of what dodt_amd.pipeline uses.  -> build(n_side=2, cfg=PYRAMID_DODT, **kw) ->
    (pipeline, trace, contexts)."""
    monkeypatch.setattr(pl, 'ops', Ops())
    monkeypatch.setitem(pl.EXTRACTORS, 'vgg_pyr', (_net((700, 800, 32)), _net((360, 1200, 32))))
    monkeypatch.setattr(pl, 'AnchorPredictor', Head)
    monkeypatch.setattr(pl, 'EarlyFusionFcLayers', Head)
    monkeypatch.setattr(pl.tracking, 'Tracker', Tracker)

    def make(n_side=2, cfg=config.PYRAMID_DODT, **kw):
        trace = []
        c = {s: Ctx(s, trace) for s in STREAMS}
        streams = types.SimpleNamespace(img_ctx=c['img'], sides=[c['c0'], c['c1']][:n_side])
        pipe = pl.FramePairPipeline(c['main'], cfg, {}, {}, reuse_streams_of=streams, bev_input_skip=False, **kw)
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
    for i, maps in enumerate(getattr(pipe, 'corr_maps', None) or ()):
        for p, a in enumerate(maps):
            names[id(a)] = 'corr_maps[%d][%d]' % (i, p)
    # the record ring: the pipeline's own buffers, or views of the caller's one allocation
    for i, (r, c) in enumerate(zip(pipe.rec2, pipe.cnt2)):
        names.setdefault(id(r.base), 'rec2[%d]' % i if r.base is r else 'record ring')
        names.setdefault(id(c.base), 'cnt2[%d]' % i if c.base is c else 'count ring')
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


# ---- the schedule as text ---------------------------------------------------------------------------------------------
# attributes of the pipeline that only point at buffers other attributes own ("of the most recently finished step")
ALIASES = ('fr', 'd_records', 'd_rec_counts', 'd_bev_in', 'd_frames', 'd_frame_counts', 'd_frame_status')


def roles(pipe, extra=None):
    """{id(allocation): role}: the attribute path on the pipeline that owns it, such as 'fr2[1][0].top_bev' or
    'feat[0].bev_feat'; `extra`: {name: what the caller owns} (inputs, injected heads, a record ring), named the same
    way.  These names are part of the fixture: when an attribute of the pipeline is renamed, map the new name back to
    the old one HERE instead of regenerating the fixture."""
    out = {}

    def walk(o, name):
        if isinstance(o, Array):
            if o.base is o:
                out.setdefault(id(o), name)
        elif isinstance(o, dict):
            for k in sorted(o):
                walk(o[k], '%s.%s' % (name, k))
        elif isinstance(o, (list, tuple)):
            for i, v in enumerate(o):
                walk(v, '%s[%d]' % (name, i))
        elif isinstance(o, Tracker):
            walk(vars(o), name)
    for attr in sorted(vars(pipe)):
        if attr not in ALIASES:
            walk(getattr(pipe, attr), attr)
    for name in sorted(extra or {}):
        walk(extra[name], name)
    return out


def _render(x, names):
    if isinstance(x, Array):
        return '%s+%d%s%s' % (names.get(id(x.base), '?'), x.ptr - x.base.ptr, list(x.shape), x.dtype.char)
    if isinstance(x, (list, tuple)):
        return '(%s)' % ','.join(_render(v, names) for v in x)
    if isinstance(x, np.ndarray):
        return 'ndarray%s' % list(x.shape)
    if isinstance(x, types.SimpleNamespace):
        return 'ns(%s)' % ','.join('%s=%r' % kv for kv in sorted(vars(x).items()))
    if x is None or isinstance(x, (bool, int, float, str, np.integer, np.floating)):
        return repr(x if x is None or isinstance(x, (bool, str)) else (float(x) if isinstance(x, (float, np.floating))
                                                                        else int(x)))
    return type(x).__name__                        # (pinned host memory and the like)


def _clock(clock):
    return '' if clock is None else ' @' + ','.join('%s%d' % (s, clock[s]) for s in STREAMS)


def entry_text(t, names):
    args = [_render(a, names) for a in t['args']] + ['%s=%s' % (k, _render(v, names)) for k, v in sorted(t['kw'].items())]
    return '%s(%s)%s' % (t['op'], ', '.join(args), _clock(t['clock']))


def canonical(pipe, trace, extra=None):
    """{stream: the entries enqueued on it, in order, as text}: launches with their arguments and clock, marks, waits
    with the clock they merged, reads of a fetched count."""
    names = roles(pipe, extra)
    per = {s: [] for s in STREAMS}
    for t in trace:
        per[t['stream']].append(entry_text(t, names))
    return per


def _sha(lines):
    return hashlib.sha1('\n'.join(lines).encode()).hexdigest()


def schedule_digest(pipe, trace, calls, extra=None):
    """What the fixture holds of one case: per API call (label, first entry, end) of `calls`, per stream the number of
    entries that call enqueued and their SHA-1, and the SHA-1 of the order in which the call fed the streams; and the
    timing marks _mark left."""
    names = roles(pipe, extra)
    out = []
    for label, start, end in calls:
        part = trace[start:end]
        streams = {}
        for s in STREAMS:
            lines = [entry_text(t, names) for t in part if t['stream'] == s]
            if lines:
                streams[s] = [len(lines), _sha(lines)]
        out.append(dict(call=label, streams=streams, order=_sha([t['stream'] for t in part])))
    marks = _sha(['%s %s %d' % (k, c.name, slot) for k, (c, slot) in sorted(pipe.marks.items())])
    return dict(calls=out, marks=marks)


# ---- the cases the fixture pins ---------------------------------------------------------------------------------------
HP = dict(rpn='rpn', avod='avod', corr='corr')
PEOPLE_PAIR = dict(config.PYRAMID_DODT, classes=config.PYRAMID_PEOPLE['classes'],
                   anchor_sizes=config.PYRAMID_PEOPLE['anchor_sizes'],
                   anchor_strides=config.PYRAMID_PEOPLE['anchor_strides'])     # (tests/test_gpu_multiclass_pipeline.py)
# name -> kw: the pipeline's arguments; env: DODT_PIPE_* switches; n_side: side streams; cfg; drive: the driver's options
CASES = {
    'pair_img': dict(kw=dict(head_params=HP), drive=dict(mark_steps=(2, 3, 5))),
    'pair_f1': dict(kw=dict(head_params=HP), env={'DODT_PIPE_CORR_MAP': 'f1'}),
    'pair_f0': dict(kw=dict(head_params=HP), n_side=1),
    'pair_detections': dict(kw=dict(head_params=HP, t_branch_rows='detections')),
    'pair_detections_one_stream': dict(kw=dict(head_params=HP, t_branch_rows='detections'), n_side=1),
    'pairs_per_step_2': dict(kw=dict(head_params=HP, pairs_per_step=2)),
    'pair_injected': dict(kw={}),
    'pair_unfused': dict(kw=dict(head_params=HP), env={'DODT_PIPE_FUSED_TAIL': '0'}),
    'pair_injected_unfused': dict(kw={}, env={'DODT_PIPE_FUSED_TAIL': '0'}),
    'pair_no_corr': dict(kw=dict(head_params=HP), env={'DODT_PIPE_NO_CORR': '1'}),
    'classes_pair': dict(kw=dict(head_params=HP, rpn_nms_size=256, t_branch_rows='proposals'), cfg=PEOPLE_PAIR),
    'classes_pair_detections': dict(kw=dict(head_params=HP, rpn_nms_size=256, t_branch_rows='detections'),
                                    cfg=PEOPLE_PAIR),
    'classes_pair_unfused': dict(kw=dict(head_params=HP, rpn_nms_size=256), cfg=PEOPLE_PAIR,
                                 env={'DODT_PIPE_FUSED_TAIL': '0'}),
    'classes_single_frame': dict(kw=dict(head_params=HP, rpn_nms_size=256), cfg=config.PYRAMID_PEOPLE),
    'temporal_tracker': dict(kw=dict(head_params=HP, temporal=dict(n_frames=3), tracker={}),
                             drive=dict(recover=True, end_sequence=True)),
    'from_host': dict(kw=dict(head_params=HP), drive=dict(host=True)),
    'record_ring': dict(kw=dict(head_params=HP), drive=dict(ring=4)),
    'seq_img': dict(kw=dict(head_params=HP, sequence=True), drive=dict(mark_steps=(2, 3, 5))),
    'seq_img_from_host': dict(kw=dict(head_params=HP, sequence=True), drive=dict(host=True)),
    'seq_detections': dict(kw=dict(head_params=HP, sequence=True, t_branch_rows='detections')),
    'seq_detections_from_host': dict(kw=dict(head_params=HP, sequence=True, t_branch_rows='detections'),
                                     drive=dict(host=True)),
    'seq_injected': dict(kw=dict(sequence=True)),
    'seq_injected_from_host': dict(kw=dict(sequence=True), drive=dict(host=True)),
    'seq_temporal_tracker': dict(kw=dict(head_params=HP, sequence=True, temporal=dict(n_frames=3), tracker={}),
                                 drive=dict(recover=True)),
}
PAIR_MODE = [name for name, case in CASES.items() if not case['kw'].get('sequence')]
EGO = (np.zeros(3), np.eye(3))


class _Calls(object):
    """The API calls of a run and the part of the trace each enqueued."""

    def __init__(self, trace):
        self.trace, self.calls = trace, [('construct', 0, len(trace))]

    def __call__(self, label, fn, *args, **kw):
        start = len(self.trace)
        ret = fn(*args, **kw)
        self.calls.append((label, start, len(self.trace)))
        return ret


def _recover(pipe, on):
    if not on:
        return None
    return [[(np.zeros(3), np.eye(3), 0.1)] * (pipe.temporal['n_frames'] - 1) for _ in range(pipe.pairs)]


def _drive_pairs(pipe, call, extra, steps=9, host=False, recover=False, end_sequence=False):
    """run() / run_from_host(): a look-ahead on two steps of three (every second one with its ego-motion entry), a
    finish() in the middle behind an announced look-ahead and one at the end, ego-motion on every fourth step."""
    nf = pipe.nf

    def inputs():
        frames = [_frame(pipe) for _ in range(nf)]
        pts, n, imgs = [list(a) for a in zip(*frames)]
        return [[object() for _ in pts], n, [object() for _ in imgs]] if host else [pts, n, imgs]
    extra['inputs'] = ins = [inputs() for _ in range(steps)]
    ego = [[EGO] * pipe.pairs if k % 4 == 1 and pipe.fps == 2 else None for k in range(steps)]
    heads = None
    if pipe.rpn_head is None:
        extra['heads'] = heads = _heads(pipe) * pipe.pairs
    run = pipe.run_from_host if host else pipe.run
    for k in range(steps):
        la = None
        if k % 3 and k + 1 < steps:
            la = tuple(ins[k + 1]) + ((ego[k + 1],) if k % 2 else ())
        kw = dict(recover=_recover(pipe, k % 2 == 1)) if recover and not host else {}
        call('run %d' % k, run, *ins[k], heads=heads, ego_motion=ego[k], lookahead=la, **kw)
        if k == 4:
            call('finish %d' % k, pipe.finish)
    call('finish', pipe.finish)
    if end_sequence:
        call('end_sequence', pipe.end_sequence)


def _drive_sequence(pipe, call, extra, host=False, recover=False):
    """push_frame() / push_frame_from_host() over two sequences with end_sequence() between and behind them: the same
    pattern of look-aheads, finish() in the middle of the first."""
    push = pipe.push_frame_from_host if host else pipe.push_frame
    heads = None
    if pipe.rpn_head is None:
        extra['heads'] = heads = _heads(pipe)
    extra['inputs'] = []
    for seq, keyframes in enumerate((10, 4)):
        frames = [_frame(pipe) for _ in range(keyframes)]
        extra['inputs'].append(frames)
        if host:
            frames = [(object(), n, object()) for _, n, _ in frames]
        for j, fr in enumerate(frames):
            la = None
            if j % 3 and j + 1 < keyframes:
                la = tuple(frames[j + 1]) + ((EGO,) if j % 2 else ())
            ret = call('push %d.%d' % (seq, j), push, *fr, heads=heads if j else None, ego_motion=EGO if j % 4 == 1 else None,
                       lookahead=la, recover=_recover(pipe, recover and j % 2 == 1))
            assert (ret is None) == (j == 0)
            if seq == 0 and j == 5:
                call('finish %d.%d' % (seq, j), pipe.finish)
        call('finish %d' % seq, pipe.finish)
        call('end_sequence %d' % seq, pipe.end_sequence)


def run_case(name, monkeypatch):
    """Build and drive case `name`.  -> (pipeline, trace, calls, extra) for schedule_digest() / races()."""
    case = CASES[name]
    for key in ('DODT_PIPE_FUSED_TAIL', 'DODT_PIPE_CORR_MAP', 'DODT_PIPE_NO_TAIL', 'DODT_PIPE_NO_CORR', 'DODT_PIPE_NO_RPN'):
        monkeypatch.delenv(key, raising=False)
    for key, value in case.get('env', {}).items():
        monkeypatch.setenv(key, value)             # (before construction: resolve_schedule reads them there)
    build = install(monkeypatch)
    pipe, trace, _ = build(n_side=case.get('n_side', 2), cfg=case.get('cfg', config.PYRAMID_DODT), **case['kw'])
    call, extra = _Calls(trace), {}
    drive = dict(case.get('drive', {}))
    pipe.mark_steps = drive.pop('mark_steps', ())
    ring = drive.pop('ring', 0)
    if ring:
        extra['rec_ring'] = Array((ring, pipe.pairs, pipe.fps, pl.MAX_DET, pl.REC_COLS))
        extra['cnt_ring'] = Array((ring, pipe.pairs, pipe.fps), np.int32)
        call('use_record_ring', pipe.use_record_ring, extra['rec_ring'], extra['cnt_ring'])
    (_drive_sequence if pipe.sequence else _drive_pairs)(pipe, call, extra, **drive)
    return pipe, trace, call.calls, extra
