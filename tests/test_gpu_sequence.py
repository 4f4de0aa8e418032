"""Sequence mode (FramePairPipeline(sequence=True), push_frame()) against the pair-mode pipeline fed the same keyframes
as explicit pairs, one step at a time (run(); finish(); sync): the carried work -- a keyframe's image maps, anchor filter
and projections, made once and used by the two pairs the frame belongs to -- is the same bytes, so every comparison is
np.array_equal.  One synthetic sequence of keyframes 0, 2, 4, ...; consecutive pairs share a keyframe exactly."""
import numpy as np
import pytest

from dodt_amd import config, device, synth
from dodt_amd.pipeline import FramePairPipeline, MAX_DET, REC_COLS, IMG_RING, PREP_RING

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
SEQ, N_POINTS, N_KEY = 31, 30000, 8
PREP_MEMBERS = ('occ', 'keep', 'count', 'bev_norm', 'img_norm', 'anchors')
TRACKER = dict(score_threshold=0.1, high_threshold=0.3, iou_threshold=0.005, t_min=1, classes=('Car',),
               max_sequence_dets=1 << 15)
TEMPORAL = dict(n_frames=3, threshold=0.1, on_conflict='next_best')


def _ego(deg, trans):
    """(trans, matrix) of ops.with_ego_motion -- p' = (p + trans) @ matrix in the velodyne frame, whose z is the
    vertical axis."""
    a = np.deg2rad(deg)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return np.asarray(trans, np.float64), rot


# the registration of keyframe j + 1 into keyframe j, by pair j (None: identity, the parameters are not even set)
EGO = [None, _ego(3.0, (1.1, 0.15, 0.0)), _ego(-2.0, (0.9, -0.2, 0.02)), None, _ego(4.0, (1.3, 0.0, 0.0)),
       _ego(1.5, (0.8, 0.1, 0.0)), None]


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


@pytest.fixture(scope='module')
def keys(ctx):
    """The keyframes, on the host and on the device."""
    pts = [synth.lidar_frame(SEQ, 2 * j, N_POINTS) for j in range(N_KEY)]
    imgs = [synth.image_frame(SEQ, 2 * j) for j in range(N_KEY)]
    return dict(pts=pts, imgs=imgs, n=[len(p) for p in pts], d_pts=[ctx.array(p) for p in pts],
                d_imgs=[ctx.array(i) for i in imgs])


def _pair_args(keys, j):
    return [keys['d_pts'][j], keys['d_pts'][j + 1]], keys['n'][j:j + 2], [keys['d_imgs'][j], keys['d_imgs'][j + 1]]


def _frame_args(keys, j):
    return keys['d_pts'][j], keys['n'][j], keys['d_imgs'][j]


def _lookahead(keys, j):
    """Keyframe j as a look-ahead: registered into keyframe j - 1 by pair j - 1's ego-motion."""
    return _frame_args(keys, j) + (EGO[j - 1] if j >= 1 else None,)


def _snap(pipe):
    """What a finished, synchronised step left: records, and per frame the kept anchors, both NMS keep lists and what
    its prep made."""
    frames = []
    for f, b in enumerate(pipe.fr):
        A = pipe.last_anchor_counts[f]
        n_top, n_det = int(b['top_count'].download()[0]), int(b['det_count'].download()[0])
        d = dict(A=A, keep=b['keep'].download()[:A], top_idx=b['top_idx'].download()[:n_top],
                 det_idx=b['det_idx'].download()[:n_det], occ=b['occ'].download(), count=b['count'].download())
        for name in ('bev_norm', 'img_norm', 'anchors'):
            d[name] = b[name].download()[:A]
        frames.append(d)
    return dict(records=pipe.d_records.download().copy(), counts=pipe.d_rec_counts.download().copy(), frames=frames)


def _same_step(got, want, what):
    assert np.array_equal(got['counts'], want['counts']), what
    assert np.array_equal(got['records'], want['records']), what
    for f in range(2):
        for name in ('A', 'keep', 'top_idx', 'det_idx'):
            assert np.array_equal(got['frames'][f][name], want['frames'][f][name]), (what, f, name)


def _equal(a, b):
    """Nested tracks / frame lists, arrays by value."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


# ---- fp32, injected heads ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def injected(ctx, keys):
    """The pair-mode yardstick, the sequence pipeline on its streams, the injected heads of every keyframe, the
    yardstick's steps over pairs 0 .. 3, and a record ring that lives as long as the pipelines (a test installs it)."""
    pair = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024)
    seq = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024, sequence=True,
                            reuse_streams_of=pair)
    heads = [{k: ctx.array(v) for k, v in synth.head_outputs(SEQ, 2 * j, pair.n_all, pair.P).items()}
             for j in range(5)]
    want = []
    for j in range(4):
        pair.run(*_pair_args(keys, j), heads=heads[j:j + 2], ego_motion=[EGO[j]])
        pair.finish()
        ctx.sync()
        want.append(_snap(pair))
    assert all(w['counts'].sum() > 0 for w in want)
    ring = (ctx.zeros((4, 1, 2, MAX_DET, REC_COLS), np.float32), ctx.zeros((4, 1, 2), np.int32))
    return pair, seq, heads, want, ring


def test_a_frame_prepared_as_frame_1_leaves_what_it_leaves_as_frame_0(injected):
    """The premise of carrying a keyframe's prep set: the ego-motion registration reaches its BEV maps only.  Pair-mode
    runs alone: keyframe j + 1 is frame 1 of pair j (registered, pairs 1 and 2) and frame 0 of pair j + 1 (plain)."""
    _, _, _, want, _ = injected
    assert EGO[1] is not None and EGO[2] is not None
    for j in range(3):
        as_f1, as_f0 = want[j]['frames'][1], want[j + 1]['frames'][0]
        assert as_f1['A'] == as_f0['A'] > 1000
        for name in PREP_MEMBERS:
            assert np.array_equal(as_f1[name], as_f0[name]), (j, name)


def test_synchronised_pushes_equal_pair_mode(ctx, keys, injected):
    """Five keyframes, four pairs, two of them registered by a rotation about the vertical axis and a metre's
    translation: a registered BEV map reused as frame 0's plain one would show in pairs 2 and 3."""
    _, seq, heads, want, _ = injected
    assert seq.push_frame(*_frame_args(keys, 0)) is None
    for j in range(4):
        assert seq.push_frame(*_frame_args(keys, j + 1), heads=heads[j:j + 2], ego_motion=EGO[j]) in (0, 1)
        seq.finish()
        ctx.sync()
        _same_step(_snap(seq), want[j], 'pair %d' % j)
    seq.end_sequence()


def test_free_running_pushes_fill_the_record_ring(ctx, keys, injected):
    """No host sync between the pushes; the records of the four steps go to a caller's ring (from here on the
    pipeline's record buffers for the rest of the module)."""
    _, seq, heads, want, (rec_ring, cnt_ring) = injected
    R, k0 = rec_ring.shape[0], seq.step_idx
    seq.use_record_ring(rec_ring, cnt_ring)
    seq.push_frame(*_frame_args(keys, 0))
    for j in range(4):
        seq.push_frame(*_frame_args(keys, j + 1), heads=heads[j:j + 2], ego_motion=EGO[j])
    seq.finish()
    ctx.sync()
    recs, cnts = rec_ring.download(), cnt_ring.download()
    for j in range(4):
        assert np.array_equal(cnts[(k0 + j) % R], want[j]['counts']), j
        assert np.array_equal(recs[(k0 + j) % R], want[j]['records']), j
    _same_step(_snap(seq), want[3], 'last pair')
    seq.end_sequence()


def test_the_callers_arrays_are_free_after_a_push(ctx, keys, injected):
    """A keyframe is voxelised a second time one step after it was pushed, as frame 0 of the next pair: from the
    pipeline's own copy, not from the caller's array."""
    _, seq, heads, want, _ = injected
    mine = [(ctx.array(keys['pts'][j]), keys['n'][j], ctx.array(keys['imgs'][j])) for j in range(2)]
    seq.push_frame(*mine[0])
    seq.push_frame(*mine[1], heads=heads[0:2], ego_motion=EGO[0])
    seq.finish()
    ctx.sync()
    for d_pts, _, d_img in mine:
        d_pts.zero()
        d_img.zero()
    ctx.sync()
    seq.push_frame(*_frame_args(keys, 2), heads=heads[1:3], ego_motion=EGO[1])
    seq.finish()
    ctx.sync()
    _same_step(_snap(seq), want[1], 'pair 1 after the arrays were zeroed')
    seq.end_sequence()


def test_push_from_pinned_host_memory(ctx, keys, injected):
    _, seq, heads, want, _ = injected
    pinned = []
    for j in range(3):
        hp, hi = ctx.pinned((seq.n_points_max, 4), np.float32), ctx.pinned(keys['imgs'][j].shape, np.uint8)
        hp.a[:keys['n'][j]] = keys['pts'][j]
        hi.a[...] = keys['imgs'][j]
        pinned.append((hp, keys['n'][j], hi))
    assert seq.push_frame_from_host(*pinned[0]) is None
    seq.push_frame_from_host(*pinned[1], heads=heads[0:2], ego_motion=EGO[0])
    seq.push_frame_from_host(*pinned[2], heads=heads[1:3], ego_motion=EGO[1])
    ctx.sync()
    _same_step(_snap(seq), want[0], 'pair 0')
    seq.finish()
    ctx.sync()
    _same_step(_snap(seq), want[1], 'pair 1')
    seq.end_sequence()
    for hp, _, hi in pinned:
        hp.free()
        hi.free()


def test_argument_checks(ctx, keys, injected):
    pair, seq, heads, _, _ = injected
    w = synth.pipeline_weights(C)
    with pytest.raises(ValueError):
        FramePairPipeline(ctx, C, sequence=True, pairs_per_step=2, **w)
    with pytest.raises(ValueError):
        FramePairPipeline(ctx, config.CARS_EXAMPLE, sequence=True, **synth.pipeline_weights(config.CARS_EXAMPLE))
    with pytest.raises(ValueError):
        seq.run(*_pair_args(keys, 0), heads=heads[0:2])
    with pytest.raises(ValueError):
        seq.run_from_host(*_pair_args(keys, 0), heads=heads[0:2])
    with pytest.raises(ValueError):
        pair.push_frame(*_frame_args(keys, 0))
    with pytest.raises(ValueError):
        pair.push_frame_from_host(*_frame_args(keys, 0))
    with pytest.raises(ValueError):
        pair.end_sequence()                     # (no tracker: as before)
    assert seq.end_sequence() is None           # (sequence mode: just the reset)
    seq.push_frame(*_frame_args(keys, 0))
    seq.push_frame(*_frame_args(keys, 1), heads=heads[0:2])
    with pytest.raises(ValueError):
        seq.end_sequence()                      # (finish() first)
    seq.finish()
    ctx.sync()
    assert seq.end_sequence() is None


def test_accounting(ctx, injected):
    """A sequence step is the BEV net over two frames and the image net over one.  (Without the BEV skip tables, whose
    per-frame share of the BEV net's count follows the last input.)"""
    first, seq0, _, _, _ = injected
    assert seq0.img_net._shape[0] == 1 and seq0.bev_net._shape[0] == 2 and first.img_net._shape[0] == 2
    assert len(seq0.img_ring) == IMG_RING and len(seq0.prep_sets) == PREP_RING
    assert seq0.flops_per_step() == seq0.bev_net.flops() + seq0.img_net.flops()
    kw = dict(rpn_nms_size=1024, bev_input_skip=False, reuse_streams_of=first)
    pair = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), **kw)
    seq = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), sequence=True, **kw)
    img_one = pair.img_net.flops() / 2
    assert seq.img_net.flops() == img_one
    assert abs(img_one - 100.28e9) < 0.01e9 and abs(pair.bev_net.flops() - 2 * 131.71e9) < 0.02e9
    assert seq.bev_net.flops() == pair.bev_net.flops()
    assert seq.flops_per_step() == seq.flops_per_pair() == pair.bev_net.flops() + img_one
    assert pair.flops_per_step() - seq.flops_per_step() == img_one
    assert seq.mfma_flops_per_step() == pair.bev_net.mfma_flops() + pair.img_net.mfma_flops() / 2
    assert seq.conv_bytes_per_step() == seq.bev_net.bytes() + seq.img_net.bytes() < pair.conv_bytes_per_step()
    assert seq.head_flops_per_step() == pair.head_flops_per_step() == 0.0
    pair.close()
    seq.close()


# ---- computed heads, temporal module, tracker; two sequences --------------------------------------------------------
def test_two_sequences_with_computed_heads_temporal_module_and_tracker(ctx, keys):
    kw = dict(rpn_nms_size=1024, head_params=synth.head_params(), temporal=TEMPORAL, tracker=TRACKER)
    pair = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), **kw)
    seq = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), sequence=True, reuse_streams_of=pair, **kw)
    sequences = [(0, 1, 2, 3), (3, 4, 5)]           # keyframes: three pairs, then two (keyframe 3 primes again)
    want = []
    for ks in sequences:
        steps = []
        for j in ks[:-1]:
            pair.run(*_pair_args(keys, j), ego_motion=[EGO[j]])
            pair.finish()
            ctx.sync()
            steps.append((_snap(pair), pair.frames()))
        want.append((steps, pair.end_sequence()))
    assert all(step[0]['counts'].sum() > 0 for steps, _ in want for step in steps)
    for (steps, tracks), ks in zip(want, sequences):
        assert seq.push_frame(*_frame_args(keys, ks[0])) is None
        for i, j in enumerate(ks[:-1]):
            assert seq.push_frame(*_frame_args(keys, j + 1), ego_motion=EGO[j]) is not None
            seq.finish()
            ctx.sync()
            _same_step(_snap(seq), steps[i][0], 'pair %d' % j)
            assert _equal(seq.frames(), steps[i][1]), j
            assert seq.head_flops_per_step() == pair.head_flops_per_step(
                [steps[i][0]['frames'][f]['A'] for f in range(2)])
        assert _equal(seq.end_sequence(), tracks)
    pair.close()
    seq.close()


# ---- bf16 convs and heads, look-ahead, no host sync ------------------------------------------------------------------
def test_bf16_free_running_with_lookahead(ctx, keys):
    kw = dict(rpn_nms_size=1024, head_params=synth.head_params(), conv_dtype='bf16', head_dtype='bf16')
    pair = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), **kw)
    seq = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), sequence=True, reuse_streams_of=pair, **kw)
    n_pairs = N_KEY - 1
    rings = [(ctx.zeros((n_pairs, 1, 2, MAX_DET, REC_COLS), np.float32), ctx.zeros((n_pairs, 1, 2), np.int32))
             for _ in range(2)]
    pair.use_record_ring(*rings[0])
    seq.use_record_ring(*rings[1])
    assert pair.t_branch_form() == seq.t_branch_form() == 'detections'
    last = None
    for j in range(n_pairs):
        pair.run(*_pair_args(keys, j), ego_motion=[EGO[j]])
        pair.finish()
        ctx.sync()
        last = _snap(pair)
    # keyframes 0 .. 4 with the next one announced every time; then finish() instead of the push of keyframe 5, which
    # follows it; the last push announces nothing
    for j in range(5):
        seq.push_frame(*_frame_args(keys, j), ego_motion=EGO[j - 1] if j else None, lookahead=_lookahead(keys, j + 1))
    seq.finish()
    for j in range(5, N_KEY):
        seq.push_frame(*_frame_args(keys, j), ego_motion=EGO[j - 1],
                       lookahead=_lookahead(keys, j + 1) if j + 1 < N_KEY else None)
    seq.finish()
    ctx.sync()
    want_r, want_c = rings[0][0].download(), rings[0][1].download()
    got_r, got_c = rings[1][0].download(), rings[1][1].download()
    assert want_c.sum() > 0
    for j in range(n_pairs):
        assert np.array_equal(got_c[j], want_c[j]), j
        assert np.array_equal(got_r[j], want_r[j]), j
    _same_step(_snap(seq), last, 'last pair')
    pair.close()
    seq.close()
