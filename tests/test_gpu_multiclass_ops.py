"""The n-class entries of the stage-2 tail on the device -- dodt_class_scores, dodt_final_decode_classes and the
record kernels with a type column -- against tf.nn.softmax as oracle.tfops states it plus np.argmax, and against the
reference's own records for 3- and 4-column softmax (tests/golden/make_goldens_multiclass.py).  Needs an MI355X."""
import os

import numpy as np
import pytest

from dodt_amd import config, device, ops
from dodt_amd.core import orientation_encoder as gpu_orient
from oracle import tfops

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
F32 = np.float32
SENTINEL = F32(-12345.5)
SENTINEL_I = np.int32(-77)
MIN_GAP = 1e-3
# the bar tests/test_gpu_ops.py::test_softmax_and_gather sets for the two-way softmax
SCORE_TOL = dict(rtol=2e-6, atol=1e-7)


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


@pytest.fixture(scope='module')
def mc(golden_dir):
    return np.load(os.path.join(golden_dir, 'multiclass.npz'))


def _logits(rng, n, n_cls):
    """(n, n_cls) float32: normal rows whose two largest non-background logits are exactly tied (every fifth row) or at
    least MIN_GAP apart (closer ones redrawn) -- so that a device expf a rounding off numpy's cannot change a winner --,
    plus rows of +-80 (exponentials that underflow to 0: ties at 0) and rows with all columns equal."""
    lg = rng.normal(0, 2.0, size=(n, n_cls)).astype(F32)
    if n_cls > 2:
        while True:
            s = np.sort(lg[:, 1:].astype(np.float64), axis=1)
            close = (s[:, -1] - s[:, -2]) < MIN_GAP
            if not close.any():
                break
            lg[close] = rng.normal(0, 2.0, size=(int(close.sum()), n_cls)).astype(F32)
        for r in range(0, n, 5):
            order = np.argsort(lg[r, 1:])[::-1] + 1
            lg[r, order[1]] = lg[r, order[0]]
    for r in range(1, n, 7):
        lg[r] = rng.choice(np.array([-80.0, 80.0], F32), n_cls)
    for r in range(2, n, 11):
        lg[r] = lg[r, 0]
    if n > 3:
        lg[3] = 80.0
        lg[3, 0] = -80.0                       # every non-background column at the maximum: type 0
    return lg


def _want(logits):
    sm = tfops.softmax2(logits)
    types = np.argmax(sm[:, 1:], axis=1)
    return sm[np.arange(len(sm)), types + 1], types.astype(np.int32), logits[:, 1:].max(axis=1)


def _anchors(rng, n):
    return np.stack([rng.uniform(-30, 30, n), rng.uniform(1.2, 1.9, n), rng.uniform(5, 60, n), rng.uniform(0.5, 4.5, n),
                     rng.uniform(1.3, 1.9, n), rng.uniform(0.5, 4.5, n)], 1).astype(F32)


def _filled(ctx, shape, dtype=F32):
    return ctx.array(np.full(shape, SENTINEL_I if dtype == np.int32 else SENTINEL, dtype))


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1024])
@pytest.mark.parametrize('n_cls', [2, 3, 4, 8])
def test_class_scores_and_final_decode_classes(ctx, n_cls, n):
    rng = np.random.default_rng(1000 * n_cls + n)
    lim = max(n - 3, 1)
    logits = _logits(rng, n, n_cls)
    want_score, want_type, want_nms = _want(logits)
    d_logits, d_n = ctx.array(logits), ctx.array(np.array([lim], np.int32))
    # ---- class_scores ------------------------------------------------------------------------------------------
    d_s, d_t = _filled(ctx, (n,)), _filled(ctx, (n,), np.int32)
    ops.class_scores(ctx, d_logits, n_cls, n, d_n, d_s, d_t)
    s, t = d_s.download(), d_t.download()
    print('class_scores n_cls %d n %d: max |score diff| %.3g, type mismatches %d'
          % (n_cls, n, np.abs(s[:lim] - want_score[:lim]).max(), int((t[:lim] != want_type[:lim]).sum())))
    assert t.dtype == np.int32 and np.array_equal(t[:lim], want_type[:lim])
    np.testing.assert_allclose(s[:lim], want_score[:lim], **SCORE_TOL)
    assert np.all(s[lim:] == SENTINEL) and np.all(t[lim:] == SENTINEL_I)
    if n_cls > 2 and n >= 255:
        assert len(np.unique(want_type[:lim])) == n_cls - 1             # every type occurs
    # ---- final_decode_classes ----------------------------------------------------------------------------------
    top, off = _anchors(rng, n), rng.normal(0, 0.15, size=(n, 10)).astype(F32)
    ang = rng.normal(0, 1.0, size=(n, 2)).astype(F32)
    d_top, d_off, d_ang = ctx.array(top), ctx.array(off), ctx.array(ang)
    plane, ext = C['ground_plane'], np.asarray(C['bev_extents']).reshape(-1)
    names = ('boxes_3d', 'pred_anchors', 'bev', 'nms', 'score', 'ori')
    widths = dict(boxes_3d=7, pred_anchors=6, bev=4)

    def outs():
        return {k: _filled(ctx, (n, widths[k]) if k in widths else (n,)) for k in names}
    o = outs()
    d_types = _filled(ctx, (n,), np.int32)
    ops.final_decode_classes(ctx, d_top, d_off, d_logits, n_cls, d_ang, n, d_n, plane, ext, o['boxes_3d'],
                             o['pred_anchors'], o['bev'], o['nms'], o['score'], d_types, o['ori'])
    got = {k: v.download() for k, v in o.items()}
    types = d_types.download()
    assert np.array_equal(types[:lim], want_type[:lim])
    assert np.array_equal(got['nms'][:lim], want_nms[:lim])             # a maximum of inputs: exact
    np.testing.assert_allclose(got['score'][:lim], want_score[:lim], **SCORE_TOL)
    assert np.array_equal(got['score'][:lim], s[:lim])                  # the same device function as class_scores
    for k in names:
        assert np.all(got[k][lim:] == SENTINEL), k
    assert np.all(types[lim:] == SENTINEL_I)
    # the box arithmetic and the orientation are the separate entries', value for value
    r = outs()
    ops.box_4c_decode(ctx, d_top, d_off, n, d_n, plane, ext, r['boxes_3d'], r['pred_anchors'], r['bev'])
    ops.angle_vector_to_orientation(ctx, d_ang, n, d_n, r['ori'])
    for k in ('boxes_3d', 'pred_anchors', 'bev', 'ori'):
        assert got[k].tobytes() == r[k].download().tobytes(), k
    assert np.isfinite(got['boxes_3d'][:lim]).all()
    if n_cls == 2:
        # one class: every output byte-equal to dodt_final_decode, the types all 0
        e = outs()
        ops.final_decode(ctx, d_top, d_off, d_logits, d_ang, n, d_n, plane, ext, e['boxes_3d'], e['pred_anchors'],
                         e['bev'], e['nms'], e['score'], e['ori'])
        for k in names:
            assert got[k].tobytes() == e[k].download().tobytes(), k
        assert not types[:lim].any()
        # box_4c: no angle vectors, no orientations
        o2 = outs()
        ops.final_decode_classes(ctx, d_top, d_off, d_logits, n_cls, None, n, d_n, plane, ext, o2['boxes_3d'],
                                 o2['pred_anchors'], o2['bev'], o2['nms'], o2['score'], d_types, None)
        assert o2['boxes_3d'].download().tobytes() == got['boxes_3d'].tobytes()
        assert np.all(o2['ori'].download() == SENTINEL)


def test_class_count_is_checked(ctx):
    d = ctx.zeros((4, 16), F32)
    d_s, d_t = ctx.zeros((4,), F32), ctx.zeros((4,), np.int32)
    for bad in (0, 1, 9, 16):
        with pytest.raises(ValueError):
            ops.class_scores(ctx, d, bad, 4, None, d_s, d_t)
        with pytest.raises(ValueError):
            ops.final_decode_classes(ctx, d, d, d, bad, None, 4, None, C['ground_plane'],
                                     np.asarray(C['bev_extents']).reshape(-1), None, None, None, d_s, d_s, d_t, None)


def _device_records(ctx, boxes, ori, logits, corr, frame, compact, rng):
    """logits -> class_scores -> the *_classes record entry, the proposals scattered by a permutation that the
    selection undoes (so that a per-proposal and a per-detection offsets array differ)."""
    n, n_cls = logits.shape
    perm = rng.permutation(n).astype(np.int32)

    def scattered(a):
        out = np.zeros_like(a)
        out[perm] = a
        return out
    d_s, d_t = ctx.empty((n,), F32), ctx.empty((n,), np.int32)
    ops.class_scores(ctx, ctx.array(scattered(logits)), n_cls, n, None, d_s, d_t)
    d_rec, d_cnt = ctx.empty((n, 17), F32), ctx.empty((1,), np.int32)
    args = (ctx, ctx.array(scattered(boxes)), d_s, d_t, ctx.array(perm), ctx.array(np.array([n], np.int32)), n,
            float(frame), d_rec, d_cnt)
    d_ori = ctx.array(scattered(ori))
    if compact:
        ops.pack_detections_compact_classes(*args, d_det_offsets=None if corr is None else ctx.array(corr),
                                            d_orientations=d_ori)
    else:
        ops.pack_detections_classes(*args, d_corr_offsets=None if corr is None else ctx.array(scattered(corr)),
                                    d_orientations=d_ori)
    assert int(d_cnt.download()[0]) == n
    return d_rec.download()


def test_records_match_reference_goldens(ctx, mc):
    """Every case of the goldens (3- and 4-column softmax, exact ties included): box and shifted-box columns bit for
    bit, the type exact, the score within the softmax bar."""
    rng = np.random.default_rng(77)
    assert int(mc['n_cases']) == 6
    for c in range(int(mc['n_cases'])):
        want = mc['c%d_records' % c]
        row = 0
        for f in range(2):
            boxes, ori = mc['c%d_boxes_3d_%d' % (c, f)], mc['c%d_orientations_%d' % (c, f)]
            logits = mc['c%d_logits_%d' % (c, f)]
            w = want[row:row + len(boxes)]
            row += len(boxes)
            for compact in ((False, True) if f == 0 else (False,)):
                got = _device_records(ctx, boxes, ori, logits, mc['c%d_corr_offsets' % c] if f == 0 else None, f,
                                      compact, rng).astype(np.float64)
                what = (c, f, compact)
                print('records case %d frame %d compact %d: max |score diff| %.3g'
                      % (c, f, compact, np.abs(got[:, 7] - w[:, 7]).max()))
                assert np.array_equal(got[:, 0:7], w[:, 0:7]), what
                assert np.array_equal(got[:, 9:17], w[:, 9:17]), what
                assert np.array_equal(got[:, 8], w[:, 8]), what
                np.testing.assert_allclose(got[:, 7], w[:, 7], **SCORE_TOL)
        assert row == len(want)
        assert len(np.unique(want[:, 8])) > 1 or len(want) < 10
    # the host wrapper's types=
    boxes, ori, sm = mc['c3_boxes_3d_1'], mc['c3_orientations_1'], mc['c3_softmax_1']
    types = np.argmax(sm[:, 1:], axis=1)
    got = gpu_orient.predicted_boxes_3d_and_scores(boxes, sm[np.arange(len(sm)), types + 1], ori, None, 1, ctx=ctx,
                                                   types=types)
    assert np.array_equal(got.astype(np.float64), mc['c3_records'][len(mc['c3_boxes_3d_0']):])


def test_records_without_types_are_the_existing_entries(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, 'box4ca.npz'))
    boxes, ori, corr = g['c0_boxes_3d_0'], g['c0_orientations_0'], g['c0_corr_offsets']
    scores = g['c0_softmax_0'][:, 1]
    n = len(boxes)
    sel = np.random.default_rng(5).permutation(n).astype(np.int32)[:n - 7]
    d = dict(b=ctx.array(boxes), s=ctx.array(scores), o=ctx.array(ori), c=ctx.array(corr), sel=ctx.array(sel),
             cnt=ctx.array(np.array([len(sel)], np.int32)))

    def run(fn, *types, **kw):
        d_rec, d_cnt = _filled(ctx, (n, 17)), ctx.empty((1,), np.int32)
        fn(ctx, d['b'], d['s'], *types, d['sel'], d['cnt'], n, 0.0, d_rec, d_cnt, d_orientations=d['o'], **kw)
        return d_rec.download().tobytes(), int(d_cnt.download()[0])
    a = run(ops.pack_detections, d_corr_offsets=d['c'])
    assert a == run(ops.pack_detections_classes, None, d_corr_offsets=d['c']) and a[1] == len(sel)
    a = run(ops.pack_detections_compact, d_det_offsets=d['c'])
    assert a == run(ops.pack_detections_compact_classes, None, d_det_offsets=d['c'])
