"""Temporal module on the host (the "M" of S+T+M): associate the
detections of a keyframe pair and fill in the frames between them.

Mirrors avod/core/dt_evaluator_utils.py:212-362 (interpolate_non_keyframe_predicitons,
interpolate_trajectory).  Input: the 17-column records of one pair as the device writes them
(FramePairPipeline.d_records, gathered across ranks by dodt_amd.sharding).  The reference
scores candidate matches with a 3-D IoU whose base overlap is rasterised at 1 cm with PIL
(wavedata/.../evaluation.py:182-261); here the overlap of the two rotated rectangles is
computed exactly by polygon clipping ("an exact polygon 3-D IoU") -- the
association only uses argmax and `> 0`, and reproduces the reference's outputs on the golden
cases (tests/test_temporal.py).  `recover(frame_index, rows)` stands for the reference's
recovery_coordinate (dodt_amd.datasets.kitti.kitti_tracking_utils.recovery_coordinate with the
pair's OXTS-derived ego-motion); None keeps keyframe-0 coordinates.

track_through_ious (avod/core/dt_evaluator_utils.py:436-511) is the tracker over a sequence
of keyframe pairs: greedy IoU association of each track's last box, shifted by its
correlation offsets, with the next pair's detections.
"""
import numpy as np


def _rect(b):
    """(4,2) corners (x,z) of the base of [x,y,z,l,w,h,ry], counter-clockwise or clockwise."""
    c, s = np.cos(b[6]), np.sin(b[6])
    xc = b[3] / 2 * np.array([1, 1, -1, -1])
    zc = b[4] / 2 * np.array([1, -1, -1, 1])
    return np.stack([c * xc + s * zc + b[0], -s * xc + c * zc + b[2]], 1)


def _clip(poly, a, b):
    """Sutherland-Hodgman: keep the part of `poly` on the inner side of edge a->b."""
    out = []
    n = len(poly)
    if n == 0:
        return poly
    d = b - a
    side = d[0] * (poly[:, 1] - a[1]) - d[1] * (poly[:, 0] - a[0])
    for i in range(n):
        j = (i + 1) % n
        pi, pj, si, sj = poly[i], poly[j], side[i], side[j]
        if si >= 0:
            out.append(pi)
        if (si >= 0) != (sj >= 0):
            t = si / (si - sj)
            out.append(pi + t * (pj - pi))
    return np.asarray(out).reshape(-1, 2)


def _area(poly):
    if len(poly) < 3:
        return 0.0
    x, z = poly[:, 0], poly[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(z, -1)) - np.dot(z, np.roll(x, -1)))


def base_intersection(box, other):
    """Exact overlap area of the two boxes' bases (rotated rectangles in the xz plane)."""
    p, q = _rect(box), _rect(other)
    e0, e1 = q[1] - q[0], q[2] - q[1]
    if e0[0] * e1[1] - e0[1] * e1[0] < 0:          # make the clip polygon counter-clockwise
        q = q[::-1]
    for i in range(4):
        p = _clip(p, q[i], q[(i + 1) % 4])
        if len(p) == 0:
            return 0.0
    return _area(p)


def _rects(b):
    """(m,4,2) base corners of boxes (m,7), the same corner order and arithmetic as _rect."""
    c, s = np.cos(b[:, 6, None]), np.sin(b[:, 6, None])
    xc = b[:, 3, None] / 2 * np.array([1, 1, -1, -1])
    zc = b[:, 4, None] / 2 * np.array([1, -1, -1, 1])
    return np.stack([c * xc + s * zc + b[:, 0, None], -s * xc + c * zc + b[:, 2, None]], 2)


def _clip_batch(poly, cnt, a, b):
    """_clip for m polygons at once.  poly (m,V,2) with cnt (m,) valid vertices each, edge a->b (m,2) each;
    returns (m,V+1,2), counts.  Every vertex and every crossing point is computed by the same expressions
    as in _clip, in the same order, so the polygons are bit-identical to the one-by-one form."""
    m, V, _ = poly.shape
    d = b - a
    side = d[:, 0, None] * (poly[:, :, 1] - a[:, 1, None]) - d[:, 1, None] * (poly[:, :, 0] - a[:, 0, None])
    idx = np.arange(V)[None, :]
    valid = idx < cnt[:, None]
    nxt = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
    pj = np.take_along_axis(poly, nxt[:, :, None], 1)
    sj = np.take_along_axis(side, nxt, 1)
    keep = valid & (side >= 0)
    cross = valid & ((side >= 0) != (sj >= 0))
    with np.errstate(divide='ignore', invalid='ignore'):      # slots that are not crossings are not read
        t = side / (side - sj)
        inter = poly + t[:, :, None] * (pj - poly)
    emit = keep.astype(np.intp) + cross
    first = np.cumsum(emit, 1) - emit
    out = np.zeros((m, V + 1, 2))
    r, v = np.nonzero(keep)
    out[r, first[r, v]] = poly[r, v]
    r, v = np.nonzero(cross)
    out[r, first[r, v] + keep[r, v]] = inter[r, v]
    return out, emit.sum(1)


def base_intersections(boxes_a, boxes_b):
    """Exact overlap areas of the bases of boxes_a[i] and boxes_b[i] (m,7 each): the Sutherland-Hodgman
    clipping of base_intersection, all m pairs per numpy call."""
    p, q = _rects(boxes_a), _rects(boxes_b)
    e0, e1 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 1]
    flip = e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0] < 0
    q[flip] = q[flip, ::-1]
    cnt = np.full(len(p), 4, np.intp)
    for i in range(4):
        p, cnt = _clip_batch(p, cnt, q[:, i], q[:, (i + 1) % 4])
    # shoelace over the valid vertices: the slots behind them repeat vertex 0, which adds exact zeros
    idx = np.arange(p.shape[1])[None, :]
    p = np.where((idx < cnt[:, None])[:, :, None], p, p[:, :1])
    x, z = p[:, :, 0], p[:, :, 1]
    area = 0.5 * np.abs((x * np.roll(z, -1, 1)).sum(1) - (z * np.roll(x, -1, 1)).sum(1))
    return np.where(cnt >= 3, area, 0.0)


def three_d_iou_matrix(boxes_a, boxes_b):
    """(na,nb) 3-D IoU of every box of boxes_a (na,7) with every box of boxes_b (nb,7), [x,y,z,l,w,h,ry]
    (y = bottom, down positive).  Pairs whose bounding spheres do not touch are 0 without clipping (the
    reference's own early exit, wavedata/.../evaluation.py:60-75); the others are clipped in one batch."""
    a = np.atleast_2d(np.asarray(boxes_a, dtype=np.float64))
    b = np.atleast_2d(np.asarray(boxes_b, dtype=np.float64))
    iou = np.zeros((len(a), len(b)))
    if iou.size == 0:
        return iou
    diag_a = np.sqrt((a[:, 3:6] ** 2).sum(1)) / 2
    diag_b = np.sqrt((b[:, 3:6] ** 2).sum(1)) / 2
    dist = np.sqrt(((b[None, :, 0:3] - a[:, None, 0:3]) ** 2).sum(2))
    i, j = np.nonzero(diag_a[:, None] + diag_b[None, :] >= dist)
    if len(i) == 0:
        return iou
    ba, bb = a[i], b[j]
    h_int = np.maximum(0.0, np.minimum(ba[:, 1], bb[:, 1]) - np.maximum(ba[:, 1] - ba[:, 5], bb[:, 1] - bb[:, 5]))
    inter = h_int * base_intersections(ba, bb)
    iou[i, j] = inter / (np.prod(ba[:, 3:6], 1) + np.prod(bb[:, 3:6], 1) - inter)
    return iou


def three_d_iou(box, boxes):
    """box (7,), boxes (n,7), both [x,y,z,l,w,h,ry] (y = bottom, down positive) -> (n,) IoU."""
    return three_d_iou_matrix(np.asarray(box, dtype=np.float64)[None], boxes)[0]


def three_d_iou_one_by_one(box, boxes):
    """The same IoU with the bases clipped pair by pair in Python (base_intersection): what three_d_iou was
    before it was batched; kept as the cross-check of the batched form (tests/test_temporal.py)."""
    boxes = np.atleast_2d(np.asarray(boxes, dtype=np.float64))
    box = np.asarray(box, dtype=np.float64)
    diag = np.sqrt((box[3:6] ** 2).sum()) / 2
    diags = np.sqrt((boxes[:, 3:6] ** 2).sum(1)) / 2
    dist = np.sqrt(((boxes[:, 0:3] - box[0:3]) ** 2).sum(1))
    iou = np.zeros(len(boxes))
    for i in np.nonzero(diag + diags >= dist)[0]:
        o = boxes[i]
        h_int = max(0.0, min(box[1], o[1]) - max(box[1] - box[5], o[1] - o[5]))
        inter = h_int * base_intersection(box, o)
        iou[i] = inter / (np.prod(box[3:6]) + np.prod(o[3:6]) - inter)
    return iou


def _fill(track_a, track_b, num):
    """One trajectory over num frames (dt_evaluator_utils.py:296-362); None = no object."""
    if track_a is not None and track_b is not None:
        a, b = track_a[:-4].copy(), track_b[:-4].copy()
        score = max(a[7], b[7])
        steps = (b[[0, 2, 6]] - a[[0, 2, 6]])
        out = [a]
        for i in range(num - 2):
            o = a.copy()
            o[[0, 2, 6]] += steps * (i + 1.0) / (num - 1)
            o[7] = score
            out.append(o)
        b[7] = score
        return out + [b]
    only, first = (track_b, False) if track_a is None else (track_a, True)
    offsets, o = only[-4:-1], only[:-4].copy()
    d = np.sqrt(offsets[0] ** 2 + offsets[1] ** 2)
    near = d <= o[4] / 2
    dx, dz = d * np.cos(o[6]), d * np.sin(o[6])
    out = []
    if first:       # seen in keyframe 0 only: moves on, or dies after half of the frames
        out.append(o)
        for i in range(num - 1):
            if near:
                n = o.copy()
                n[0] += dx * (i + 1.0) / (num - 1)
                n[2] += dz * (i + 1.0) / (num - 1)
                out.append(n)
            else:
                out.append(None if i >= num / 2 else o.copy())
    else:           # seen in keyframe 1 only: traced back, or born after half of the frames
        for i in range(num - 1):
            if near:
                n = o.copy()
                n[0] -= dx * (num - i - 2) / (num - 1)
                n[2] -= dz * (num - i - 2) / (num - 1)
                out.append(n)
            else:
                out.append(None if i <= num / 2 else o.copy())
        out.append(o)
    return out


def interpolate_non_keyframe_predictions(predictions, n_frames, threshold, recover=None, on_conflict='raise'):
    """predictions (n,17): box_3d(7), score, type, shifted box(7), frame mark (0/1).
    n_frames: frames from keyframe 0 to keyframe 1 inclusive (tau + 1; 1 = a lone frame).
    Returns n_frames arrays (k,13), like the reference (columns [:-4] of the records).
    on_conflict: two keyframe-0 detections whose best match is the same keyframe-1 detection make the
    reference raise ValueError (`next_idx.remove`, dt_evaluator_utils.py:266-268) -- 'raise', the default,
    does the same; 'next_best' gives the later one its best still-free match instead (IoU > 0, else none),
    for callers that must not stop on such a pair."""
    if on_conflict not in ('raise', 'next_best'):
        raise ValueError("on_conflict must be 'raise' or 'next_best'")
    p = np.asarray(predictions, dtype=np.float64).reshape(-1, 17)
    rec = recover or (lambda i, rows: rows)
    kept = [p[(p[:, -1] == i) & (p[:, 7] > threshold)] for i in range(min(n_frames, 2))]
    if n_frames == 1:
        return [kept[0][:, :-4]]
    if n_frames == 2:
        return [kept[0][:, :-4], rec(1, kept[1][:, :-4])]
    k0, k1 = kept
    if len(k0) == 0 and len(k1) == 0:      # nothing to track (and nothing to recover)
        return [np.zeros((0, 13)) for _ in range(n_frames)]
    pairs = []
    if len(k0) == 0:
        pairs = [(None, o) for o in k1]
    else:
        free = list(range(len(k1)))
        # every keyframe-0 detection against all of frame 1 (as the reference: not only the free ones),
        # all of them in one batch
        iou_all = three_d_iou_matrix(k0[:, :7], k1[:, :7]) if len(k1) else None
        for n, cur in enumerate(k0):
            match = None
            if free:
                ious = iou_all[n]
                best = int(np.argmax(ious))
                if ious[best] > 0 and best not in free and on_conflict == 'next_best':
                    best = free[int(np.argmax(ious[free]))]
                if ious[best] > 0:
                    match = k1[best]
                    free.remove(best)
            pairs.append((cur, match))
        pairs += [(None, k1[j]) for j in free]
    out = [[] for _ in range(n_frames)]
    for a, b in pairs:
        for i, o in enumerate(_fill(a, b, n_frames)):
            if o is not None:
                out[i].append(o)
    out = [np.asarray(o, dtype=np.float64).reshape(-1, 13) for o in out]
    return [out[0]] + [rec(i, out[i]) for i in range(1, n_frames)]


def _kitti_rows(boxes):
    """iou_3d of track_through_ious (dt_evaluator_utils.py:439-447) takes KITTI-ordered boxes
    [h, w, l, x, y, z, ry].  The reference builds its [ry, l, h, w, tx, ty, tz] rows with the
    index list [-2, 0, 2, 1, 3, 4, 5]: the angle slot receives z, the l slot h and the h slot
    l -- reproduced as written.  Returns the rows as [x, y, z, l, w, h, ry] for three_d_iou."""
    b = np.atleast_2d(np.asarray(boxes, dtype=np.float64))
    # reference slots: ry = b[-2], l = b[0], h = b[2], w = b[1], t = b[3:6]
    return b[:, [3, 4, 5, 0, 1, 2, -2]]


def _iou_3d_kitti(box3d_1, box3d_2):
    return float(three_d_iou_matrix(_kitti_rows(box3d_1), _kitti_rows(box3d_2))[0, 0])


def _iou_3d_kitti_many(box3d, boxes3d):
    """One box against a list of boxes: the values of [_iou_3d_kitti(box3d, b) for b in boxes3d], one batch."""
    if len(boxes3d) == 0:
        return np.zeros(0)
    return three_d_iou_matrix(_kitti_rows(box3d), _kitti_rows(np.stack([np.asarray(b, np.float64) for b in boxes3d])))[0]


def encode_tracking_dets(pairs, calib_p2, image_size, classes, threshold):
    """encoder_tracking_dets + decode_tracking_file (dt_evaluator_utils.py:368-434) without the text
    files in between.  pairs: [(frame_0, frame_1, records (n,17))] of one sequence in frame order, the
    records as the device writes them.  A pair's keyframe-0 detections (with 'offsets' = the box shifted
    by the correlation head into keyframe 1) go to dets_for_track, its keyframe-1 detections to
    dets_for_ious, both as KITTI label rows (convert_pred_to_kitti_format; the offsets rows are converted
    on their own, so a shifted box that leaves the image drops out of ITS list only and the zip pairs what
    is left, as in the reference).  Pairs without any detection are skipped."""
    from dodt_amd.core.dt_inference_utils import kitti_label_table

    # The reference's rows are strings (np.column_stack with the class names) that it parses back with
    # np.array(row[...], dtype=np.float32): numpy prints a float64 in its shortest round-trip form, so the
    # parsed value is float32(the 3-decimal float64) -- taken here without the text in between.
    def kitti(rows):
        if len(rows) == 0:
            return []
        types, k = kitti_label_table(rows, calib_p2, image_size, threshold)
        return [] if k is None else list(zip(types, k))

    def item(frame_id, row, offset=None):
        t, k = row
        d = {'frame_id': str(frame_id), 'info': [classes[t], '-1', '-1', '-10.0'],
             'boxes2d': k[4:8].astype(np.float32), 'boxes3d': k[8:15].astype(np.float32),
             'scores': np.float32(k[15])}
        if offset is not None:
            d['offsets'] = offset[1][8:15].astype(np.float32)
        return d

    dets_for_track, dets_for_ious = [], [{}]
    for frame_0, frame_1, rec in pairs:
        rec = np.asarray(rec, dtype=np.float32).reshape(-1, 17)
        r0, r1 = rec[rec[:, -1] == 0], rec[rec[:, -1] == 1]
        k0, k1 = kitti(r0[:, :9]), kitti(r1[:, :9])
        shifted = r0[:, :9].copy()
        shifted[:, :7] = r0[:, 9:-1]
        koff = kitti(shifted)
        if len(k0) == 0 and len(k1) == 0:
            continue
        dets_for_track.append([item(frame_0, f, o) for f, o in zip(k0, koff)])
        dets_for_ious.append([item(frame_1, f) for f in k1])
    return dets_for_track, dets_for_ious


def track_through_ious(dets_for_track, dets_for_ious, high_threshold, iou_threshold, t_min):
    """dt_evaluator_utils.py:436-511.  dets_for_track[k]: detections of pair k's first frame
    (dicts with 'boxes3d' (7,) [h,w,l,x,y,z,ry], 'offsets' = the box shifted into the pair's
    second frame, 'scores', ...); dets_for_ious[k]: detections the previous pair reported for
    that same frame ([{}] for k = 0, dt_evaluator_utils.py:398).  Returns the finished tracks:
    dicts 'trajectory' (list of detections), 'max_score', 'start_frame'.  The inputs are not
    modified (the reference appends merged detections to them)."""
    # (the reference appends to and deletes from the lists it is given and sets 'offsets' on merged
    #  detections: lists and dicts are copied here, the arrays inside are never written)
    dets_for_track = [[dict(d) for d in f] for f in dets_for_track]
    dets_for_ious = [[dict(d) for d in f] if isinstance(f, list) else f for f in dets_for_ious]

    def boxes_of(items):
        return _kitti_rows(np.stack([np.asarray(x['boxes3d'], np.float64) for x in items]))

    def merge_dets(dets, dets_iou):
        """The reference's merge_dets: a detection of dets_iou that overlaps nothing in `dets` is appended to it
        (with 'offsets' = its own box) -- `dets` grows while the loop runs, so later ones are also tested against
        the ones appended before them.  Both IoU tables of the frame in two batches; the loop only reads them."""
        merged = dets
        if len(dets_iou) == 0:
            return merged
        b_iou = boxes_of(dets_iou)
        hits = (three_d_iou_matrix(b_iou, boxes_of(dets)) > 0).any(1) if len(dets) else np.zeros(len(dets_iou), bool)
        among = three_d_iou_matrix(b_iou, b_iou) > 0
        appended = []
        for i, item1 in enumerate(dets_iou):
            if not hits[i] and not among[i, appended].any():
                item1['offsets'] = item1['boxes3d']
                merged.append(item1)
                appended.append(i)
        return merged

    tracks_active, tracks_finished = [], []
    for frame_num, dets in enumerate(dets_for_track):
        update_tracks = []
        dets_iou = dets_for_ious[frame_num]
        # The reference walks the active tracks and, per track, (a) merges the two lists if their lengths differ
        # -- which can only happen at the first track: afterwards both lose the same entry per match --, (b) takes
        # the IoU of the track's shifted last box with every remaining detection.  Same decisions here with the
        # merge done once and all IoUs of the frame in one batch; `alive` maps the shrinking lists' positions to
        # columns of that matrix.
        if tracks_active and len(dets) > 0:
            if len(dets_iou) != len(dets):
                merged = merge_dets(dets, dets_iou)
                dets = [dict(d) for d in merged]
                dets_iou = [dict(d) for d in merged]
            ious_all = three_d_iou_matrix(
                _kitti_rows(np.stack([np.asarray(t['trajectory'][-1]['offsets'], np.float64) for t in tracks_active])),
                boxes_of(dets_iou))
        alive = list(range(len(dets)))
        for n, track in enumerate(tracks_active):
            if len(dets) > 0:
                ious = ious_all[n, alive]
                best = int(np.argmax(ious))
                if ious[best] > iou_threshold:
                    track['trajectory'].append(dets[best])
                    track['max_score'] = max(track['max_score'], dets[best]['scores'])
                    update_tracks.append(track)
                    del dets[best]
                    del dets_iou[best]
                    del alive[best]
            if len(update_tracks) == 0 or track is not update_tracks[-1]:
                if track['max_score'] >= high_threshold and len(track['trajectory']) >= t_min:
                    tracks_finished.append(track)
        new_tracks = [{'trajectory': [det], 'max_score': det['scores'], 'start_frame': frame_num}
                      for det in dets]
        tracks_active = update_tracks + new_tracks
    tracks_finished += [t for t in tracks_active
                        if t['max_score'] >= high_threshold and len(t['trajectory']) >= t_min]
    return tracks_finished


def convert_trajectory_to_kitti_format(trajectories):
    """dt_evaluator_utils.py:514-532: finished tracks -> KITTI tracking rows [frame_id, track id, type, truncated,
    occluded, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score], the track id being the position in
    `trajectories`.  The rows are sorted by 100 * frame_id + id as written -- ids of 100 and more interleave with
    later frames -- and returned as np.asarray of the mixed list (strings)."""
    final_pred_label = []
    for id in range(len(trajectories)):
        trace = trajectories[id]
        score = trace['max_score']
        for obj in trace['trajectory']:
            label = ([obj['frame_id']] + [id] + np.asarray(obj['info']).tolist() + obj['boxes2d'].tolist()
                     + obj['boxes3d'].tolist() + [score])
            final_pred_label.append(label)
    final_pred_label.sort(key=lambda obj: 100 * int(obj[0]) + int(obj[1]))
    return np.asarray(final_pred_label)
