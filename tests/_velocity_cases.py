"""Shared by the velocity tracker's tests: detections, scenarios, the host run with its own IoUs recorded, the fairness
conditions on those IoUs (nothing near sigma_iou, every argmax clearly won) and the track-by-track comparison."""
import numpy as np

from _kalman_cases import CALIB_ID, CALIB_KITTI, PARKED, moving  # noqa: F401
from dodt_amd.experiments import video_detection_iou as vit
from dodt_amd.experiments.video_detection import label_transform_box

PARAMS = dict(sigma_l=0.1, sigma_h=0.5, sigma_iou=0.1, t_min=3, extend_len=3)      # the reference's __main__
INFO = ['Car', '-1', '-1', '-10']


def det(frame, x, z, score=0.9, ry=1.5, dims=(1.5, 1.6, 4.0), dtype=np.float32):
    """A car whose length lies along z (ry near pi / 2): under this tracker's l/h swap its IoU with itself is 0.23."""
    return {'video_id': 0, 'frame_id': int(frame), 'info': np.array(INFO),
            'boxes2d': np.array([100. + 7 * x, 150., 180. + 7 * x, 210. + z], dtype),
            'boxes3d': np.array([dims[0], dims[1], dims[2], x, 1.6, z, ry], dtype), 'score': dtype(score)}


def unregister(box, ego3, calib):
    """The box [l, w, h, x, y, z, ry] that label_transform_box moves onto `box` under the ego-motion `ego3` (the map of
    the centre is affine: four probes give it)."""
    def moved(c):
        return label_transform_box(list(box[:3]) + list(c) + [0.0], calib[0], calib[1], *ego3)[3:6]
    t0 = moved(np.zeros(3))
    m = np.stack([moved(e) - t0 for e in np.eye(3)], 1)
    return list(box[:3]) + list(np.linalg.solve(m, np.asarray(box[3:6]) - t0)) + [box[6] - ego3[2]]


def seq(objects, n_key, stride, ego=PARKED, calib=CALIB_ID, dtype=np.float32, extra=None):
    """objects: (x0, z0, vx, vz per frame, ry, score, keyframes it is seen at).  Every keyframe's box is the one that,
    registered into the keyframe before it, lies one stride of the object's own motion ahead of the box there.
    extra: {keyframe: [det() arguments]}.  -> build() -> (frames of fresh dicts, stride, frame_num)."""
    def build():
        latent = [[4.0, 1.6, 1.5, x0, 1.6, z0, ry] for (x0, z0, vx, vz, ry, score, seen) in objects]
        frames = []
        for k in range(n_key):
            if k > 0:
                e3 = ego(k * stride - stride, k * stride)
                for o, (x0, z0, vx, vz, ry, score, seen) in enumerate(objects):
                    b = list(latent[o])
                    b[3] += vx * stride
                    b[5] += vz * stride
                    latent[o] = unregister(b, e3, calib)
            f = []
            for o, (x0, z0, vx, vz, ry, score, seen) in enumerate(objects):
                if k in seen:
                    b = latent[o]
                    d = det(k * stride, b[3], b[5], score, b[6], dtype=dtype)
                    d['boxes3d'][4] = b[4]
                    f.append(d)
            frames.append(f + [det(k * stride, *e, dtype=dtype) for e in (extra or {}).get(k, [])])
        return frames, stride, (n_key - 1) * stride + 1
    return build


def host_run(ego, calib, frames, stride, frame_num, **params):
    """vit.interpolate_by_track and, per (track, keyframe), the IoUs of its candidates."""
    groups, keys = [], []
    real = vit.cal_transformed_ious

    def spy(ego_, calib_, track, detection):
        v = real(ego_, calib_, track, detection)
        key = (id(track), detection['frame_id'])
        if not keys or keys[-1] != key:
            keys.append(key)
            groups.append([])
        groups[-1].append(v)
        return v
    vit.cal_transformed_ious = spy
    try:
        p = dict(PARAMS, **params)
        tracks = vit.interpolate_by_track(ego, calib, frames, stride, frame_num, p['sigma_l'], p['sigma_h'],
                                          p['sigma_iou'], p['t_min'], p['extend_len'])
    finally:
        vit.cal_transformed_ious = real
    return tracks, groups


def host_run_so_far(ego, calib, frames, stride, **params):
    """What a sequence has FINISHED after frames[0:n] (tracks_so_far): host_run on those keyframes, frame_num the last
    one's frame + 1, without the tracks that were still live at the end -- those that predict_det did not finish."""
    cut = set()
    real = vit.predict_det

    def spy(track, tracks_finished, *args):
        before = len(tracks_finished)
        out = real(track, tracks_finished, *args)
        if len(tracks_finished) > before:
            cut.add(id(track))
        return out
    vit.predict_det = spy
    try:
        tracks, groups = host_run(ego, calib, frames, stride, (len(frames) - 1) * stride + 1, **params)
    finally:
        vit.predict_det = real
    return [t for t in tracks if id(t) in cut], groups


def assert_fair(groups, sigma_iou, margin=1e-6):
    """The host alone decides whether a case is fair: no IoU within `margin` of sigma_iou, every argmax wins by
    `margin` or every candidate is exactly 0.  -> (the nearest IoU to sigma_iou, the smallest contested win)."""
    near, win = np.inf, np.inf
    for g in groups:
        v = np.asarray(g, np.float64)
        assert np.all(np.isfinite(v))
        near = min(near, np.abs(v - sigma_iou).min())
        if not v.any():
            continue
        s = np.sort(v)[::-1]
        if len(s) > 1:
            win = min(win, s[0] - s[1])
    assert near >= margin, 'an IoU %g from sigma_iou' % near
    assert win >= margin, 'an argmax won by %g' % win
    return near, win


def _where(d, frames):
    for k, frame in enumerate(frames):
        for i, x in enumerate(frame):
            if x is d:
                return (k, i)
    return None


def assert_same_tracks(got, got_frames, want, want_frames):
    """Exactly: number and order of tracks, every entry's frame id, which input detection an entry is (got_frames None:
    `got` holds no caller's dicts, the boxes alone say it), every bit of boxes3d and boxes2d, max_score, speed,
    extend_len."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [d['frame_id'] for d in g['dets']] == [d['frame_id'] for d in w['dets']]
        for dg, dw in zip(g['dets'], w['dets']):
            at = _where(dw, want_frames)
            if got_frames is not None:
                assert _where(dg, got_frames) == at
            assert dg['boxes3d'].dtype == dw['boxes3d'].dtype and dg['boxes2d'].dtype == dw['boxes2d'].dtype
            assert np.array_equal(dg['boxes3d'], dw['boxes3d']), (dg['frame_id'], dg['boxes3d'], dw['boxes3d'])
            assert np.array_equal(dg['boxes2d'], dw['boxes2d'])
            assert dg['score'] == dw['score']
        assert g['max_score'] == w['max_score']
        assert np.array_equal(np.asarray(g['speed']), np.asarray(w['speed'])), (g['speed'], w['speed'])
        assert g['extend_len'] == w['extend_len']
