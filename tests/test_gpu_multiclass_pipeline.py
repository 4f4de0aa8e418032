"""Several classes end to end on the device: the people configuration's single frame and a DODT pair with two classes
through FramePairPipeline (free-running, computed heads) against the oracle applied to the pipeline's own
intermediates, and the temporal module and the tracker on records whose types are not all 0.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _multiclass_pipeline as job
from dodt_amd import config, device
from dodt_amd import temporal as dev_temporal
from dodt_amd import tracking as dev_tracking
from dodt_amd.core import dt_evaluator_utils as host
from dodt_amd.pipeline import MAX_DET, FramePairPipeline
from oracle import anchors as oanchors
from oracle import boxes as oboxes
from oracle import points as opoints
from oracle import postprocess as opost
from oracle import tfops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P2, WH = config.KITTI_P2, config.KITTI_IMAGE_WH
SCORE_TOL = dict(rtol=2e-6, atol=1e-7)          # tests/test_gpu_ops.py::test_softmax_and_gather's bar
PAIR_CFG = dict(config.PYRAMID_DODT, classes=job.PEOPLE, anchor_sizes=config.PYRAMID_PEOPLE['anchor_sizes'],
                anchor_strides=config.PYRAMID_PEOPLE['anchor_strides'])
_shift = [0.0]          # the cls_out bias shift the single-frame test settled on: where the pair test starts


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


def _top_logits(pipe, f=0):
    b = pipe.fr[f]
    return b['cls_logits'].download()[:int(b['top_count'].download()[0])]


def _oracle_upstream(pts, cfg):
    """oracle.pipeline.frame_inputs' anchor half with the oracle's single-class grid called per class."""
    sizes, strides = config.class_anchor_params(cfg)
    boxes = np.concatenate([oanchors.tile_anchors_3d(cfg['area_extents'], s, st, cfg['ground_plane'])
                            for s, st in zip(sizes, strides)])
    anchors = oanchors.box_3d_to_anchor(boxes)
    cloud = opoints.lidar_in_camera_view(pts, config.KITTI_R0_RECT, config.KITTI_TR_VELO_TO_CAM, P2, WH)
    vox = oanchors.sliced_voxel_grid_2d(cloud, cfg['ground_plane'], cfg['area_extents'], cfg['voxel_size'],
                                        cfg['anchor_filter_lo'], cfg['anchor_filter_hi'])
    keep = np.nonzero(oanchors.empty_anchor_filter_2d(anchors, vox))[0]
    kept = anchors[keep]
    _, bev_norm = oboxes.project_to_bev(kept, cfg['bev_extents'])
    _, img_norm = oboxes.project_to_image_space(kept, P2, [WH[1], WH[0]])
    return dict(n_all=len(anchors), keep=keep, anchors=kept.astype(np.float32),
                bev_norm_tf=bev_norm.astype(np.float32)[:, [1, 0, 3, 2]], img_norm_tf=img_norm[:, [1, 0, 3, 2]])


def test_people_single_frame_matches_oracle(ctx, tmp_path):
    cfg = config.PYRAMID_PEOPLE
    shift = 0.0
    pipe, pts = job.run_single_frame(ctx, shift)
    for _ in range(3):
        # the test needs both types among the kept detections: where the seeded weights prefer one class, the bias of
        # the other's cls_out column moves until they do not
        n_det = int(pipe.d_rec_counts.download().reshape(-1)[0])
        shares = job.type_shares(pipe.d_records.download().reshape(-1, 17), n_det)
        print('cls_out bias shift %.4f: %d detections, type shares %s' % (shift, n_det, shares.tolist()))
        if n_det >= 20 and shares.min() >= 0.1:
            break
        shift += job.balancing_shift(_top_logits(pipe))
        pipe.close()
        pipe, pts = job.run_single_frame(ctx, shift)
    _shift[0] = shift
    assert pipe.fps == 1 and pipe.n_cls == 3 and pipe.classes == job.PEOPLE and pipe.placement == 'none'
    b = pipe.fr[0]
    recs = pipe.d_records.download().reshape(MAX_DET, 17)
    n_det = int(b['det_count'].download()[0])
    assert n_det == int(pipe.d_rec_counts.download().reshape(-1)[0]) >= 20
    shares = job.type_shares(recs, n_det)
    assert shares.min() >= 0.1, shares
    # ---- upstream: kept anchors of the two-class grid, proposals --------------------------------------------------
    inp = _oracle_upstream(pts, cfg)
    A = len(inp['keep'])
    n0 = inp['n_all'] // 2
    assert pipe.n_all == inp['n_all'] == 89600 and pipe.last_anchor_counts[0] == A > 200
    assert (inp['keep'] < n0).any() and (inp['keep'] >= n0).any()          # both classes' anchors are kept
    assert np.array_equal(b['keep'].download()[:A], inp['keep'])
    assert np.array_equal(b['anchors'].download()[:A], inp['anchors'])
    assert np.array_equal(b['bev_norm'].download()[:A], inp['bev_norm_tf'])
    assert np.array_equal(b['img_norm'].download()[:A], inp['img_norm_tf'])
    rpn_logits, rpn_offsets = b['rpn_logits'].download()[:A], b['rpn_offsets'].download()[:A]
    assert rpn_logits.shape == (A, 2)                                      # the RPN stays two-way objectness
    regressed = oboxes.offset_to_anchor(inp['anchors'], rpn_offsets, np.float32)
    _, prop_norm = oboxes.project_to_bev(regressed, cfg['bev_extents'], np.float32)
    top = tfops.non_max_suppression_fast(prop_norm, tfops.softmax2(rpn_logits)[:, 1], pipe.P,
                                         cfg['rpn_nms_iou_thresh'])
    n_top = int(b['top_count'].download()[0])
    assert n_top == len(top) and MAX_DET < n_top <= job.RPN_NMS_SIZE
    assert np.array_equal(b['top_idx'].download()[:n_top], top)
    # ---- tail: NMS #2 on the largest non-background logit, records from the pipeline's own intermediates -----------
    cls = b['cls_logits'].download()[:n_top]
    assert cls.shape == (n_top, 3)
    boxes_3d, ori = b['boxes_3d'].download()[:n_top], b['orientations'].download()[:n_top]
    nms2_boxes, det_idx = b['nms2_boxes'].download()[:n_top], b['det_idx'].download()[:n_det]
    want_det = tfops.non_max_suppression_fast(nms2_boxes, cls[:, 1:].max(axis=1), cfg['avod_nms_size'],
                                              cfg['avod_nms_iou_thresh'])
    assert np.array_equal(det_idx, want_det)
    assert np.array_equal(b['nms2_scores'].download()[:n_top], cls[:, 1:].max(axis=1))
    none = np.zeros((0, 7), np.float32)
    want = opost.avod_predicted_boxes_3d_and_scores(
        [boxes_3d[det_idx], none], [ori[det_idx], none[:, 0]], [tfops.softmax2(cls)[det_idx], none[:, :3]],
        np.zeros((n_det, 3), np.float32))
    assert want.shape == (n_det, 17)
    got = recs[:n_det].astype(np.float64)
    print('single frame: %d kept anchors, %d proposals, %d detections, max |score diff| %.3g'
          % (A, n_top, n_det, np.abs(got[:, 7] - want[:, 7]).max()))
    assert np.array_equal(got[:, 0:7], want[:, 0:7])
    assert np.array_equal(got[:, 8], want[:, 8])
    np.testing.assert_allclose(got[:, 7], want[:, 7], **SCORE_TOL)
    assert np.array_equal(b['det_types'].download()[det_idx], want[:, 8].astype(np.int32))
    assert not got[:, 9:17].any() and not recs[n_det:].any()               # no pair: no shifted box, mark 0
    # ---- the tail's unfused form, in a process of its own: the same records, byte for byte ------------------------
    assert pipe.sched.fused_tail
    fused = (pipe.d_records.download().tobytes(), pipe.d_rec_counts.download().tobytes())
    pipe.close()
    path = str(tmp_path / 'unfused.npz')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_multiclass_pipeline.py'), repr(shift), path],
                       cwd=ROOT, env=dict(os.environ, DODT_PIPE_FUSED_TAIL='0'), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    child = np.load(path)
    assert not bool(child['fused_tail'])
    assert (child['records'].tobytes(), child['counts'].tobytes()) == fused


def _run_pair(ctx, shift, made, **kw):
    pipe = FramePairPipeline(ctx, PAIR_CFG, rpn_nms_size=job.RPN_NMS_SIZE, head_params=job.head_params(shift),
                             reuse_streams_of=made[0] if made else None, **job.synth.pipeline_weights(PAIR_CFG), **kw)
    made.append(pipe)
    frames = [job.frame_inputs(job.SEQ, f) for f in (0, 2)]
    pipe.run([ctx.array(p) for p, _ in frames], [len(p) for p, _ in frames], [ctx.array(i) for _, i in frames])
    pipe.finish()
    ctx.sync()
    return pipe


def test_pair_with_two_classes_same_records_in_both_t_branch_forms(ctx):
    made = []
    shift = _shift[0]
    prop = _run_pair(ctx, shift, made, t_branch_rows='proposals')
    for _ in range(3):
        cnt = prop.d_rec_counts.download().reshape(-1)
        recs = prop.d_records.download().reshape(2, MAX_DET, 17)
        types = np.concatenate([recs[f, :cnt[f], 8] for f in range(2)])
        print('pair, cls_out bias shift %.4f: counts %s, types %s' % (shift, cnt.tolist(), np.bincount(types.astype(int))))
        if set(np.unique(recs[0, :cnt[0], 8])) == {0.0, 1.0}:
            break
        shift += job.balancing_shift(_top_logits(prop))
        prop = _run_pair(ctx, shift, made, t_branch_rows='proposals')
    det = _run_pair(ctx, shift, made, t_branch_rows='detections')
    assert (prop.t_branch_form(), det.t_branch_form()) == ('proposals', 'detections')
    assert prop.n_cls == det.n_cls == 3 and prop.n_all == 89600
    cnt = prop.d_rec_counts.download()
    recs = prop.d_records.download()
    assert cnt.shape == (1, 2) and cnt.min() > 0
    assert np.array_equal(cnt, det.d_rec_counts.download())
    assert recs.tobytes() == det.d_records.download().tobytes()
    r0 = recs[0, 0, :cnt[0, 0]]
    assert set(np.unique(r0[:, 8])) == {0.0, 1.0}                          # both types are there ...
    assert np.abs(r0[:, 9:16]).max() > 0 and np.all(recs[0, 1, :cnt[0, 1], 16] == 1)   # ... with frame 0's shifted boxes
    # the type column is the n_cls-way softmax's argmax at the kept boxes, in both forms
    for p in (prop, det):
        b = p.fr[0]
        idx = b['det_idx'].download()[:cnt[0, 0]]
        cls = b['cls_logits'].download()
        assert cls.shape == (p.P, 3)
        assert np.array_equal(np.argmax(tfops.softmax2(cls[idx])[:, 1:], axis=1).astype(np.float32), r0[:, 8])
    for p in made:
        p.close()


# ---- temporal module and tracker: class-agnostic, column 8 travels with its row ---------------------------------------
GRID = [(x, z) for z in (12.0, 22.0, 32.0, 42.0) for x in (-9.0, -3.0, 3.0, 9.0)]


def _box(rng, o, t, vel):
    x, z = GRID[o]
    return np.array([x + vel[o, 0] * t + rng.normal(0, 0.02), 1.6, z + vel[o, 1] * t + rng.normal(0, 0.02),
                     1.2 + 0.05 * o, 0.6 + 0.01 * o, 1.7, 0.3 * o - 1.5])


def _keyframe_pair(rng, types0, types1, in0, in1, vel, j=0, zero_shift=()):
    """(n,17) records: objects `in0` in keyframe 0 (mark 0, the box shifted into keyframe 1 in cols 9:16) and `in1` in
    keyframe 1, types from types0 / types1."""
    rows = []
    for o in in0:
        shifted = np.zeros(7) if o in zero_shift else _box(rng, o, j + 1, vel)
        rows.append(np.concatenate([_box(rng, o, j, vel), [rng.uniform(0.3, 1.0), types0[o]], shifted, [0]]))
    for o in in1:
        rows.append(np.concatenate([_box(rng, o, j + 1, vel), [rng.uniform(0.3, 1.0), types1[o]], np.zeros(7), [1]]))
    return np.asarray(rows).reshape(-1, 17)


def test_temporal_module_carries_types(ctx):
    rng = np.random.default_rng(31)
    n_obj = 14
    vel = rng.uniform(-0.3, 0.3, (n_obj, 2))
    types0 = rng.integers(0, 2, n_obj).astype(np.float64)
    types0[:4] = [0, 1, 0, 1]
    types1 = types0.copy()
    types1[4] = 1 - types0[4]                    # one object is matched across different types
    in0, in1 = list(range(0, 12)), list(range(2, 14))       # 0, 1 die; 12, 13 are born; 12 rows per keyframe
    pred = _keyframe_pair(rng, types0, types1, in0, in1, vel, zero_shift=(1,)).astype(np.float32)
    pred = pred[rng.permutation(len(pred))]
    n_frames = 4
    want = host.interpolate_non_keyframe_predictions(pred, n_frames, 0.1)
    got = dev_temporal.interpolate_non_keyframe_predictions(pred, n_frames, 0.1, ctx=ctx)
    assert len(got) == len(want) == n_frames
    # 10 matched pairs; 12 and 13 are born (no offsets: traced back through every frame); 1 dies near (zero offsets:
    # carried through every frame) and 0 dies far (gone in the last frame)
    assert [len(w) for w in want] == [14, 14, 14, 13]
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, f
        assert np.array_equal(g[:, 8], w[:, 8]), f                          # every output row's type
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12)
        assert set(np.unique(g[:, 8])) == {0.0, 1.0}, f
    k0 = pred[pred[:, 16] == 0]
    assert len(k0) == (pred[:, 16] == 1).sum() == 12
    # the cross-type pair: interpolated rows carry keyframe 0's type, the last frame keyframe 1's
    a = k0[np.argmin(np.abs(k0[:, 0] - GRID[4][0]) + np.abs(k0[:, 2] - GRID[4][1]))]
    for f in range(n_frames):
        row = got[f][np.argmin(np.abs(got[f][:, 0] - a[0]) + np.abs(got[f][:, 2] - a[2]))]
        assert row[8] == (types1[4] if f == n_frames - 1 else types0[4]), f


def test_tracker_carries_types_and_names_both_classes(ctx):
    rng = np.random.default_rng(32)
    n_obj, n_pairs = 14, 6
    vel = rng.uniform(-0.25, 0.25, (n_obj, 2))
    types = rng.integers(0, 2, n_obj).astype(np.float64)
    types[:4] = [0, 1, 0, 1]
    pairs = []
    for j in range(n_pairs):
        in0 = [o for o in range(n_obj) if o < 12 or j >= 2]
        in1 = [o for o in range(n_obj) if (o < 12 or j >= 1) and not (o == 3 and j >= 3)]
        rec = _keyframe_pair(rng, types, types, in0[:12] if j < 2 else in0, in1, vel, j).astype(np.float32)
        pairs.append((2 * j, 2 * j + 2, rec[rng.permutation(len(rec))]))
    score, high, iou, t_min = 0.1, 0.5, 0.005, 3
    classes = list(job.PEOPLE)
    dft, dfi = host.encode_tracking_dets(pairs, P2, WH, classes, score)
    want = host.track_through_ious(dft, dfi, high, iou, t_min)
    assert len(want) >= 8 and {d['info'][0] for t in want for d in t['trajectory']} == set(classes)
    recs, counts, max_det = dev_tracking._pack_records(pairs)
    tr = dev_tracking.Tracker(ctx, 4096, high, iou, t_min, score)
    tr.track_records(ctx.array(recs), ctx.array(counts), len(pairs), max_det, P2, WH)
    tr.flush()
    got = dev_tracking.tracks_from_log(tr.read(), lambda pair, kf: 2 * pair + 2 * kf, classes)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g['start_frame'] == w['start_frame'] and g['max_score'] == w['max_score']
        assert len(g['trajectory']) == len(w['trajectory'])
        for a, b in zip(g['trajectory'], w['trajectory']):
            assert a['info'] == b['info'] and a['frame_id'] == b['frame_id']          # every row's type
            assert np.array_equal(a['boxes3d'], b['boxes3d']) and a['scores'] == b['scores']
    rows = FramePairPipeline.kitti_tracking_rows(None, got)
    assert np.array_equal(rows, host.convert_trajectory_to_kitti_format(want))
    assert set(rows[:, 2]) == set(classes)
