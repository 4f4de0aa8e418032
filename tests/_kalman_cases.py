"""Shared by the Kalman tracker's tests: the scenarios, the host run with its own IoU matrices recorded, the fairness
conditions on those matrices (a unique optimum, nothing near the gate) and the track-by-track comparison."""
import numpy as np
from scipy.optimize import linear_sum_assignment

from dodt_amd import config
from dodt_amd.experiments import video_detection_kf as vkf

PARKED = lambda a, b: (np.zeros(3), np.eye(3), 0.0)         # noqa: E731
CALIB_ID = (np.eye(3), np.hstack([np.eye(3), np.zeros((3, 1))]))
CALIB_KITTI = (np.asarray(config.KITTI_R0_RECT, np.float64), np.asarray(config.KITTI_TR_VELO_TO_CAM, np.float64))


def moving(a, b):
    """0.3 m forward (velodyne x) and 0.01 rad of yaw per frame: the later frame's points, shifted and turned (as row
    vectors, `@ matrix`) into the earlier frame."""
    n = b - a
    yaw = 0.01 * n
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([0.3 * n, 0.0, 0.0]), np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]), yaw


def det(frame, x, z, score=0.9, ry=0.1, dims=(1.5, 1.6, 4.0)):
    return {'frame_id': frame, 'boxes3d': np.array([dims[0], dims[1], dims[2], x, 1.6, z, ry]),
            'boxes2d': np.array([0., 0., 10., 10.]) + x, 'scores': score}


def follow_scenario():
    """test_kalman.py::test_kf_pipeline_follows_objects_and_drops_noise: three objects, nine keyframes, stride 2, one
    missed detection, two clutter boxes, one detection below sigma_l in every keyframe."""
    rng = np.random.default_rng(3)
    stride, n_key = 2, 9
    starts = [(-6.0, 15.0, 0.15, 1.9), (5.0, 40.0, -0.1, -1.2), (0.5, 25.0, 0.0, 0.8)]
    frames = []
    for k in range(n_key):
        dets = [det(k * stride, x0 + vx * k + rng.normal(0, 0.02), z0 + vz * k + rng.normal(0, 0.02), ry=1.5)
                for (x0, z0, vx, vz) in starts]
        if k == 4:
            dets.pop(1)
        if k in (2, 6):
            dets.append(det(k * stride, rng.uniform(-3, 3), rng.uniform(50, 60), score=0.95))
        dets.append(det(k * stride, 1.0, 30.0, score=0.05))
        frames.append(dets)
    return frames, stride, n_key * stride


def host_run(ego, calib, frames, stride, frame_total, sigma_l, iou_threshold, **kw):
    """vkf.kf_pipeline and the (nt, nd) float32 IoU matrix of every assignment it solved."""
    seen = []
    real = vkf.linear_sum_assignment

    def spy(cost):
        seen.append(-np.asarray(cost))
        return real(cost)
    vkf.linear_sum_assignment = spy
    try:
        tracks = vkf.kf_pipeline(ego, calib, frames, stride, frame_total, sigma_l, iou_threshold, **kw)
    finally:
        vkf.linear_sum_assignment = real
    return tracks, seen


def second_best_gap(iou):
    """Total of the optimal assignment minus the best total of any other assignment of the same size: every other
    assignment lacks at least one pair of the optimum, so forbid each in turn."""
    cost = -np.asarray(iou, np.float64)
    r, c = linear_sum_assignment(cost)
    best = -cost[r, c].sum()
    gap = np.inf
    for i, j in zip(r, c):
        alt = cost.copy()
        alt[i, j] = 1e6
        r2, c2 = linear_sum_assignment(alt)
        if alt[r2, c2].sum() < 1e5:
            gap = min(gap, best + alt[r2, c2].sum())
    return gap, iou[r, c]


def assert_fair(matrices, iou_threshold, margin=1e-3):
    """The reference alone decides whether a case is fair: a unique optimum at every keyframe, no assigned IoU near
    the gate.  -> the smallest gap."""
    worst = np.inf
    for m in matrices:
        gap, assigned = second_best_gap(m)
        assert gap >= margin, 'an assignment with a second best %g away' % gap
        assert np.all(np.abs(assigned.astype(np.float64) - iou_threshold) >= margin), 'an assigned IoU at the gate'
        worst = min(worst, gap)
    return worst


def _where(d, frames):
    for k, frame in enumerate(frames):
        for i, x in enumerate(frame):
            if x is d:
                return (k, i)
    return None


def assert_same_tracks(got, got_frames, want, want_frames, atol=1e-9):
    """Exactly: number and order of tracks, id, hits, no_losses, every det's frame_id and is_virtual flag, which input
    detection a real entry is (got_frames None: `got` holds no caller's dicts, the boxes alone say it).  To atol:
    x_state, P, box, every det's boxes and score."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.id, g.hits, g.no_losses) == (w.id, w.hits, w.no_losses)
        assert g.x_state.shape == (8, 1) and np.asarray(g.P).shape == (8, 8)
        np.testing.assert_allclose(g.x_state, w.x_state, rtol=0, atol=atol)
        np.testing.assert_allclose(g.P, w.P, rtol=0, atol=atol)
        np.testing.assert_allclose(g.box, w.box, rtol=0, atol=atol)
        assert [d['frame_id'] for d in g.dets] == [d['frame_id'] for d in w.dets]
        assert [bool(d.get('is_virtual')) for d in g.dets] == [bool(d.get('is_virtual')) for d in w.dets]
        for dg, dw in zip(g.dets, w.dets):
            if not dw.get('is_virtual'):
                at = _where(dw, want_frames)
                assert at is not None and (got_frames is None or _where(dg, got_frames) == at)
            np.testing.assert_allclose(dg['boxes3d'], dw['boxes3d'], rtol=0, atol=atol)
            np.testing.assert_allclose(dg['boxes2d'], dw['boxes2d'], rtol=0, atol=atol)
            assert abs(dg['scores'] - dw['scores']) <= atol
