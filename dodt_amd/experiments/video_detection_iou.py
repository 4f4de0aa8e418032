"""The velocity-extrapolating greedy IoU tracker of the video-level association on the host: stands where
avod/experiments/video_detection_iou.py stands for

  iou_3d                              :164-173  3-D IoU of KITTI-ordered boxes [h, w, l, x, y, z, ry]
  cal_transformed_ious                :215-233  the detection registered into the frame of the track's last entry first
  get_boundary_dis / inside           :235-251  distance to, and a box centre inside, the camera's BEV wedge
  interpolate_det                     :297-328  the frames between two keyframes of a match; the track's speed
  extend_track_start / _end           :330-367  finished tracks extended at both ends
  predict_det                         :369-397  a track without a match, extrapolated by its last displacement
  update_dierection                   :400-410  heading sign by the majority of a track (the reference's spelling)
  interpolate_by_track                :413-470  greedy association in track order over the keyframes of a video
  convert_trajectory_to_kitti_format  :472-490  KITTI tracking rows, as strings

numpy.  As in dodt_amd.experiments.video_detection the caller passes `ego(frame_a, frame_b) -> (trans, matrix, delta)`
and `calib = (r0_rect, tr_velo_to_cam)` where the reference looks them up in its dataset object.  Detections are dicts:
'video_id' (optional), 'frame_id' (int), 'info', 'boxes2d' (4,), 'boxes3d' [h, w, l, x, y, z, ry] (box3d_to_label reads
l from slot 2), 'score' (this file's key).  Tracks are dicts 'dets', 'direction', 'max_score', 'speed', 'extend_len'.

Parity: everything but the IoU is pinned bit for bit by runs of the reference's own functions
(tests/golden/velocity_track.npz): the box arithmetic happens in the dtype of the detections' arrays with the
reference's expressions.  The IoU is the exact polygon one of dodt_amd.core.dt_evaluator_utils where the reference
rasterises the bases at 1 cm with PIL (at most 0.0038 apart over 1 078 calls; the golden scenarios keep every decision
0.01 away from a threshold).  Quirks kept: iou_3d permutes its two arguments differently, so the TRACK's box enters
with l and h swapped and IoUs are small; a frame gap of 1 leaves `speed` at [0, 0, 0]; `speed` is the displacement of
a whole gap yet is added per predicted frame; extend_len = 0 would empty a coasting track (dets[:-0]).
"""
from copy import deepcopy

import numpy as np

from dodt_amd.core.dt_evaluator_utils import three_d_iou
from dodt_amd.experiments.video_detection import label_transform_box

_XZR = [3, 5, 6]            # x, z, ry of a KITTI-ordered box: what `speed` moves


def iou_3d(box3d_1, box3d_2):
    """Boxes [h, w, l, x, y, z, ry] -> IoU of the two cuboids.  The reference hands wavedata's three_d_iou (which reads
    [ry, l, h, w, x, y, z]) box 1 as [ry, h, l, w, ...] and box 2 as [ry, l, h, w, ...]: box 1 with l and h swapped."""
    a = np.asarray(box3d_1, np.float64)
    b = np.asarray(box3d_2, np.float64)
    a = np.array([a[3], a[4], a[5], a[0], a[1], a[2], a[6]])
    if b.ndim == 1:
        return float(three_d_iou(a, np.array([b[3], b[4], b[5], b[2], b[1], b[0], b[6]])[None])[0])
    return three_d_iou(a, b[:, [3, 4, 5, 2, 1, 0, 6]])


def cal_transformed_ious(ego, calib, track, detection):
    """The detection's box moved into the frame of the track's last entry by the ego-motion between the two
    (label_transform, kitti_tracking_dataset.py:338-372), then iou_3d.  float64."""
    last = track['dets'][-1]
    trans, matrix, delta = ego(last['frame_id'], detection['frame_id'])
    h, w, l, x, y, z, ry = [float(v) for v in detection['boxes3d']]
    m = label_transform_box([l, w, h, x, y, z, ry], calib[0], calib[1], trans, matrix, delta)
    return iou_3d(last['boxes3d'], np.array([m[2], m[1], m[0], m[3], m[4], m[5], m[6]]))


def get_boundary_dis(det):
    """The smallest distance of the box centre to the five borders of the wedge."""
    x, z = det['boxes3d'][3], det['boxes3d'][5]
    return min([abs(x - z) / np.sqrt(2), abs(40 - x), abs(70 - z), abs(x + 40), abs(x + z) / np.sqrt(2)])


def inside(det):
    """The box centre lies in 0 < z < 70, |x| < 40 and inside the wedge z > 1.3 |x|."""
    x, z = det['boxes3d'][3], det['boxes3d'][5]
    if (x > -40) & (x < 40) and (z > 0) & (z < 70):
        if (z + 1.3 * x) > 0 and (z - 1.3 * x) > 0:
            return True
    return False


def interpolate_det(track, next_det, frame_num=None):
    """Before next_det joins the track: a copy of the last entry for every frame in between, advanced by i / gap of the
    difference (boxes2d, x, y, z; ry only if both headings have the same sign, else it is next_det's), and
    speed = the displacement of the whole gap.  A gap of 1 appends nothing and leaves speed alone."""
    pre_det = track['dets'][-1]
    pre_id, next_id = pre_det['frame_id'], next_det['frame_id']
    gap = int(next_id) - int(pre_id)
    if gap == 0:
        return None
    if gap == 1:
        return track
    for i in range(1, gap):
        new_det = deepcopy(pre_det)
        new_det['frame_id'] = pre_id + i
        new_det['boxes2d'] += i / gap * (next_det['boxes2d'] - pre_det['boxes2d'])
        new_det['boxes3d'][3:6] += i / gap * (next_det['boxes3d'][3:6] - pre_det['boxes3d'][3:6])
        if next_det['boxes3d'][-1] * pre_det['boxes3d'][-1] > 0:
            new_det['boxes3d'][-1] += i / gap * (next_det['boxes3d'][-1] - pre_det['boxes3d'][-1])
        else:
            new_det['boxes3d'][-1] = next_det['boxes3d'][-1]
        track['dets'].append(new_det)
    track['speed'] = next_det['boxes3d'][_XZR] - pre_det['boxes3d'][_XZR]
    return track


def extend_track_start(trajectories, stride):
    """A track that starts inside the wedge after frame 0: up to `stride` copies of its first entry backwards, each
    moved by -(dets[1] - dets[0]), not below frame 0."""
    for track in trajectories:
        if len(track['dets']) < 2:
            continue
        first_det = track['dets'][0]
        if not inside(first_det) or first_det['frame_id'] == 0:
            continue
        speed = track['dets'][1]['boxes3d'][_XZR] - first_det['boxes3d'][_XZR]
        for _ in range(stride):
            pre_det = deepcopy(track['dets'][0])
            pre_det['frame_id'] -= 1
            if pre_det['frame_id'] < 0:
                break
            pre_det['boxes3d'][_XZR] -= speed
            track['dets'].insert(0, pre_det)
    return trajectories


def extend_track_end(trajectories, stride, frame_num):
    """A track that ends inside the wedge before frame_num - 1: `stride` copies of its last entry forwards, each moved
    by the track's speed (no upper bound on the frame id)."""
    for track in trajectories:
        if len(track['dets']) < 2:
            continue
        last_det = track['dets'][-1]
        if not inside(last_det) or last_det['frame_id'] >= frame_num - 1:
            continue
        for _ in range(stride):
            next_det = deepcopy(track['dets'][-1])
            next_det['frame_id'] += 1
            next_det['boxes3d'][_XZR] += track['speed']
            track['dets'].append(next_det)
    return trajectories


def predict_det(track, tracks_finished, frame_num, stride, sigma_h, t_min, extend_len):
    """A keyframe without a match: up to `stride` times, while fewer than extend_len predictions trail the track, a
    copy of the last entry one frame on and moved by speed; otherwise the trailing predictions are cut, the track is
    finished if max_score >= sigma_h and it has >= t_min entries, and it leaves the live list (returns None for it)."""
    speed = track['speed']
    for _ in range(stride):
        if track['extend_len'] < extend_len:
            next_det = deepcopy(track['dets'][-1])
            next_det['frame_id'] += 1
            next_det['boxes3d'][_XZR] += speed
            track['extend_len'] += 1
            track['dets'].append(next_det)
        else:
            track['dets'] = track['dets'][:-extend_len]
            if track['max_score'] >= sigma_h and len(track['dets']) >= t_min:
                tracks_finished.append(track)
            return None, tracks_finished
    return track, tracks_finished


def update_dierection(track, det):
    """With three or more headings in the track the detection's takes the sign of their majority (ties: negative).
    The reference defines it and calls it nowhere."""
    directions = track['direction']
    angle = det['boxes3d'][-1]
    track['direction'].append(1 if angle > 0 else -1)
    if len(directions) >= 3:
        det['boxes3d'][-1] = abs(angle) if sum(directions) > 0 else -abs(angle)
    return track, det


def _open_track(det):
    """A track of one detection: no speed yet (a list of zeros, as the reference has it), nothing predicted."""
    heading = 1 if det['boxes3d'][-1] > 0 else -1
    return dict(dets=[det], direction=[heading], max_score=det['score'], speed=[0.0, 0.0, 0.0], extend_len=0)


def interpolate_by_track(ego, calib, detections, stride, frame_num, sigma_l, sigma_h, sigma_iou, t_min, extend_len):
    """detections[k]: the detection dicts of keyframe k (frame k * stride).  Greedy in track order (updated tracks, then
    new ones): each live track takes the first maximum of its IoUs with the detections still free, matches if that is
    > sigma_iou, coasts otherwise; the remaining detections open tracks.  Returns the finished tracks, whose real
    entries are the caller's dicts."""
    tracks_active, tracks_finished = [], []
    for frame in detections:
        dets = [det for det in frame if det['score'] >= sigma_l]
        updated_tracks = []
        for track in tracks_active:
            best = -1
            if len(dets) > 0:
                ious = [cal_transformed_ious(ego, calib, track, x) for x in dets]
                best = int(np.argmax(ious))
                if not ious[best] > sigma_iou:
                    best = -1
            if best >= 0:
                if track['extend_len'] > 0:
                    track['extend_len'] = 0
                track = interpolate_det(track, dets[best], frame_num)
                track['dets'].append(dets[best])
                track['max_score'] = max(track['max_score'], dets[best]['score'])
                updated_tracks.append(track)
                del dets[best]
            else:
                track, tracks_finished = predict_det(track, tracks_finished, frame_num, stride, sigma_h, t_min,
                                                     extend_len)
                if track is not None:
                    updated_tracks.append(track)
        tracks_active = updated_tracks + [_open_track(det) for det in dets]
    tracks_finished += [track for track in tracks_active
                        if track['max_score'] >= sigma_h and len(track['dets']) >= t_min]
    tracks_finished = extend_track_start(tracks_finished, stride)
    tracks_finished = extend_track_end(tracks_finished, stride, frame_num)
    return tracks_finished


def convert_trajectory_to_kitti_format(trajectories):
    """[frame, track id, info (4), boxes2d (4), boxes3d (7), max_score] per entry, boxes rounded to 3 decimals, sorted
    by 100 * frame + id (stable), as one array of strings; a track's id is its position in the list."""
    rows = []
    for tid, trace in enumerate(trajectories):
        score = trace['max_score']
        for obj in trace['dets']:
            info = np.asarray(obj['info']).tolist()
            boxes2d = [round(i, 3) for i in obj['boxes2d']]
            boxes3d = [round(i, 3) for i in obj['boxes3d']]
            rows.append([obj['frame_id']] + [tid] + info + boxes2d + boxes3d + [score])
    rows.sort(key=lambda obj: 100 * int(obj[0]) + int(obj[1]))
    return np.asarray(rows)
