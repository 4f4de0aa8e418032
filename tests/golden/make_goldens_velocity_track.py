#!/usr/bin/env python3
"""Golden vectors for the velocity-extrapolating greedy IoU tracker: the reference's own iou_3d (:164-173),
cal_transformed_ious (:215-233), interpolate_by_track (:413-470, with interpolate_det, predict_det and the two end
extensions) and convert_trajectory_to_kitti_format (:472-490) of avod/experiments/video_detection_iou.py, run in the
build container on seeded synthetic detections and the OXTS / calibration files of tracking video 0 that the
reference's tests bundle.

Run:  python tests/golden/make_goldens_velocity_track.py     (needs /root/reference; writes velocity_track.npz)

The scaffolding is make_goldens_tracking.py's: inert stand-ins for the config system's generated modules, a plain
object carrying KittiTrackingDataset's unbound methods as the dataset.  Stored as flat arrays: every input detection
gets a serial number; a finished track is the rows of its entries [track, frame id, serial of the real detection or -1,
boxes3d (7), boxes2d (4)] and one row [max_score, speed (3), entries].

Fairness, asserted here: the reference rasterises the bases of two boxes at 1 cm where this repository clips the
polygons exactly (at most 0.0038 apart over 1 078 calls), so a scenario is only kept if every IoU the reference computes
while it tracks, and the exact IoU of the same call, lie at least 0.01 from sigma_iou, and every argmax wins by at
least 0.01 in both (or every candidate is exactly 0).  Smallest gap found over the three stored runs: 0.0266 to
sigma_iou (stride 1: 0.0411, stride 2: 0.0266, stride 3: 0.0962); every argmax had a single non-zero candidate.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_goldens as mg  # noqa: E402
import make_goldens_box4ca as mb  # noqa: E402
import make_goldens_tracking as mt  # noqa: E402

PARAMS = dict(sigma_l=0.1, sigma_h=0.5, sigma_iou=0.1, t_min=3, extend_len=3)      # the reference's __main__
MARGIN = 0.01
RUNS = {1: 13, 2: 14, 3: 5}          # stride -> seed (the first ones found that are fair by 0.02)
INFO = ['Car', '-1', '-1', '-10']


def ego_from(lines):
    from dodt_amd.datasets.kitti import kitti_tracking_utils as ktu

    def ego(fa, fb):
        return ktu.coordinate_transform(ktu.Oxts(lines[int(fa)]), ktu.Oxts(lines[int(fb)]))
    return ego


def make_det(serial, frame, box3d, box2d, score):
    return {'video_id': 0, 'frame_id': int(frame), 'info': np.array(INFO), 'serial': serial,
            'boxes2d': np.array(box2d, dtype=np.float32), 'boxes3d': np.array(box3d, dtype=np.float32),
            'score': np.array(score, dtype=np.float32)}


def unregister(box, ego3, calib):
    """The box [l, w, h, x, y, z, ry] that label_transform_box moves onto `box` under the ego-motion `ego3` (the map of
    the centre is affine: four probes give it)."""
    from dodt_amd.experiments.video_detection import label_transform_box

    def moved(c):
        return label_transform_box(list(box[:3]) + list(c) + [0.0], calib[0], calib[1], *ego3)[3:6]
    t0 = moved(np.zeros(3))
    m = np.stack([moved(e) - t0 for e in np.eye(3)], 1)
    return list(box[:3]) + list(np.linalg.solve(m, np.asarray(box[3:6]) - t0)) + [box[6] - ego3[2]]


def scenario(seed, stride, ego, calib, n_key=10, n_obj=7):
    """Cars driving along their length: every keyframe's box is the one that, registered into the keyframe before it,
    lies one stride of the car's own motion ahead of the box there -> the input table [serial, keyframe, frame, score,
    boxes3d (7), boxes2d (4)].  Object 1 misses two keyframes, object 2 vanishes for good, object 3 scores below
    sigma_h, object 4 below sigma_l, object 5 changes the sign of its heading, object 6 appears late; keyframe 5 is
    empty."""
    rng = np.random.default_rng(seed)
    x0 = np.linspace(-14, 14, n_obj) + rng.uniform(-1, 1, n_obj)
    z0 = rng.uniform(25, 45, n_obj)
    vz = rng.uniform(0.03, 0.15, n_obj)
    vx = rng.uniform(-0.03, 0.03, n_obj)
    dims = np.stack([rng.uniform(1.4, 1.7, n_obj), rng.uniform(1.5, 1.8, n_obj), rng.uniform(3.6, 4.6, n_obj)], 1)
    ry = np.pi / 2 + rng.uniform(-0.08, 0.08, n_obj)
    latent = [[dims[o][2], dims[o][1], dims[o][0], x0[o], 1.6, z0[o], ry[o]] for o in range(n_obj)]
    table, serial = [], 0
    for k in range(n_key):
        f = k * stride
        if k > 0:
            e3 = ego(f - stride, f)
            for o in range(n_obj):
                b = list(latent[o])
                b[3] += vx[o] * stride
                b[5] += vz[o] * stride
                latent[o] = unregister(b, e3, calib)
        if k == 5:
            continue
        for o in range(n_obj):
            if (o == 1 and k in (3, 6)) or (o == 2 and k >= 4) or (o == 6 and k < 3):
                continue
            box = list(latent[o])
            box[3] += rng.normal(0, 0.02)
            box[5] += rng.normal(0, 0.02)
            if o == 5 and k % 2:
                box[6] -= np.pi
            score = rng.uniform(0.55, 0.99)
            if o == 3:
                score = rng.uniform(0.15, 0.45)
            if o == 4:
                score = rng.uniform(0.01, 0.09)
            box2d = [300 + 40 * o + 3 * f, 150 + o, 380 + 40 * o + 4 * f, 210 + 2 * o]
            table.append([serial, k, f, score, box[2], box[1], box[0]] + list(box[3:7]) + box2d)
            serial += 1
    return np.asarray(table, np.float64)


def frames_of(table, n_key):
    frames = [[] for _ in range(n_key)]
    for r in table:
        frames[int(r[1])].append(make_det(int(r[0]), r[2], r[4:11], r[11:15], r[3]))
    return frames


def pack_tracks(tracks, frames):
    real = {id(d): d['serial'] for f in frames for d in f}
    entries, heads = [], []
    for t, trk in enumerate(tracks):
        for d in trk['dets']:
            entries.append([t, d['frame_id'], real.get(id(d), -1)] + list(d['boxes3d'].astype(np.float64))
                           + list(d['boxes2d'].astype(np.float64)))
        heads.append([float(trk['max_score'])] + [float(v) for v in trk['speed']] + [len(trk['dets'])])
    return np.asarray(entries, np.float64).reshape(-1, 14), np.asarray(heads, np.float64).reshape(-1, 5)


def check_fair(groups, sigma_iou, margin=MARGIN):
    """groups: per (track, keyframe) the (reference, exact) IoUs of its candidates -> the smallest distance to
    sigma_iou, the smallest winning margin of a contested argmax (inf: none was contested)."""
    near, win = np.inf, np.inf
    for g in groups:
        both = np.asarray(g, np.float64)
        near = min(near, np.abs(both - sigma_iou).min())
        assert np.abs(both - sigma_iou).min() >= margin, 'an IoU %r at the threshold' % (g,)
        if not both.any():
            continue
        assert np.argmax(both[:, 0]) == np.argmax(both[:, 1])
        for col in (0, 1):
            s = np.sort(both[:, col])[::-1]
            if len(s) > 1 and s[1] > 0:
                win = min(win, s[0] - s[1])
            assert len(s) == 1 or s[0] - s[1] >= margin, 'an argmax won by %g' % (s[0] - s[1])
    return near, win


def load_reference():
    mb.import_evaluator()
    sys.meta_path.insert(0, mt._InertPb2())
    from avod.experiments import video_detection_iou as vi
    from avod.datasets.kitti.kitti_tracking_dataset import KittiTrackingDataset as DS
    from wavedata.tools.core import calib_utils
    root = os.path.join(mg.REF, 'avod/tests/datasets/Kitti/tracking/training')
    ds = types.SimpleNamespace(oxts_dir=root + '/oxts', calib_dir=root + '/calib', bev_source='lidar')
    ds.get_oxts = lambda n: DS.get_oxts(ds, n)
    ds.coordinate_transform = lambda n: DS.coordinate_transform(ds, n)
    ds.label_transform = lambda labels, names: DS.label_transform(ds, labels, names)
    ds.kitti_utils = types.SimpleNamespace(
        get_calib=lambda src, name: calib_utils.read_tracking_calibration(ds.calib_dir, int(name[:2])))
    calib = calib_utils.read_tracking_calibration(ds.calib_dir, 0)
    lines = open(root + '/oxts/0000.txt').read().splitlines()[:40]
    return vi, ds, (calib.r0_rect, calib.tr_velodyne_to_cam), lines


def run_reference(vi, ds, ego, calib, table, stride, n_key):
    """The reference's interpolate_by_track on the table, its IoUs and the exact ones recorded per argmax."""
    from dodt_amd.experiments import video_detection_iou as host
    frames = frames_of(table, n_key)
    groups, keys = [], []
    real = vi.cal_transformed_ious

    def spy(dataset, video_id, track, detection):
        v = float(real(dataset, video_id, track, detection))
        key = (id(track), detection['frame_id'])
        if not keys or keys[-1] != key:
            keys.append(key)
            groups.append([])
        groups[-1].append((v, host.cal_transformed_ious(ego, calib, track, detection)))
        return v
    vi.cal_transformed_ious = spy
    try:
        tracks = vi.interpolate_by_track(ds, 0, [list(f) for f in frames], stride, (n_key - 1) * stride + 1, **PARAMS)
    finally:
        vi.cal_transformed_ious = real
    return tracks, frames, groups


def main():
    vi, ds, calib, lines = load_reference()
    ego = ego_from(lines)
    rng = np.random.default_rng(20261021)
    out = {'r0': calib[0], 'tr': calib[1], 'oxts_lines': np.array(lines)}

    # (a) iou_3d and (b) cal_transformed_ious (frames 2 -> 4) on seeded pairs [h, w, l, x, y, z, ry]
    n = 40
    a = np.stack([rng.uniform(1.4, 1.7, n), rng.uniform(1.5, 1.8, n), rng.uniform(3.4, 4.6, n), rng.uniform(-15, 15, n),
                  1.6 + rng.normal(0, 0.1, n), rng.uniform(10, 50, n), rng.uniform(-3.1, 3.1, n)], 1)
    b = a.copy()
    b[:, 0:3] *= rng.uniform(0.9, 1.1, (n, 3))
    b[:, 3] += rng.uniform(-1.5, 1.5, n)
    b[:, 5] += rng.uniform(-1.5, 1.5, n)
    b[:, 6] += rng.uniform(-0.4, 0.4, n)
    b[:4] = a[:4]                                    # identical boxes: l and h still enter swapped on one side
    out['iou3d_a'], out['iou3d_b'] = a, b
    out['iou3d'] = np.asarray([float(vi.iou_3d(a[i].copy(), b[i].copy())) for i in range(n)])
    out['iou3d_swapped'] = np.asarray([float(vi.iou_3d(b[i].copy(), a[i].copy())) for i in range(n)])
    c = b.copy()
    c[:, 5] += 1.5                                   # (the ego drives on between frames 2 and 4)
    out['trans_b'] = c
    out['trans_iou'] = np.asarray([float(vi.cal_transformed_ious(
        ds, 0, {'dets': [{'frame_id': 2, 'boxes3d': a[i].copy()}]}, {'frame_id': 4, 'boxes3d': c[i].copy()}))
        for i in range(n)])
    print('iou_3d: %d of %d non-zero; cal_transformed_ious: %d non-zero'
          % ((out['iou3d'] > 0).sum(), n, (out['trans_iou'] > 0).sum()))

    # (c) whole runs, (d) their KITTI rows
    worst = np.inf
    for stride, seed in sorted(RUNS.items()):
        n_key = 10
        table = scenario(seed, stride, ego, calib, n_key)
        tracks, frames, groups = run_reference(vi, ds, ego, calib, table, stride, n_key)
        near, win = check_fair(groups, PARAMS['sigma_iou'])
        worst = min(worst, near, win)
        entries, heads = pack_tracks(tracks, frames)
        out['s%d_table' % stride], out['s%d_entries' % stride], out['s%d_heads' % stride] = table, entries, heads
        out['s%d_frame_num' % stride] = np.asarray((n_key - 1) * stride + 1)
        out['s%d_kitti' % stride] = vi.convert_trajectory_to_kitti_format(tracks).astype(str)
        print('stride %d seed %d: %d detections -> %d tracks, %d entries (%d real, %d others); %d argmaxes, nearest IoU '
              'to sigma_iou %.4f, smallest contested win %s'
              % (stride, seed, len(table), len(tracks), len(entries), (entries[:, 2] >= 0).sum(),
                 (entries[:, 2] < 0).sum(), len(groups), near, win))
    print('smallest gap found: %.4f' % worst)
    out['params'] = np.asarray([PARAMS[k] for k in ('sigma_l', 'sigma_h', 'sigma_iou', 't_min', 'extend_len')])
    np.savez_compressed(os.path.join(HERE, 'velocity_track.npz'), **out)


if __name__ == '__main__':
    main()
