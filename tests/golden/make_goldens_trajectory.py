#!/usr/bin/env python3
"""Golden vectors for convert_trajectory_to_kitti_format (avod/core/dt_evaluator_utils.py:514-532): the
reference's own function, run in the build container on seeded synthetic tracks shaped like the ones
track_through_ious returns (the detections as decode_tracking_file builds them: 'info' a numpy array of
strings, float32 boxes and score).

Run:  python tests/golden/make_goldens_trajectory.py     (needs /root/reference; writes trajectory.npz)

Stored as flat arrays: per case the tracks' detections as rows [track, frame_id, boxes2d (4), boxes3d (7)]
in float64 (the float32 values widened; 'info' is ['Car', '-1', '-1', '-10.0'] throughout), the tracks' max
scores (float32) and the reference's output table (strings).  Case 2 has 130 tracks: ids of 100 and more, whose sort key
100 * frame_id + id interleaves them with later frames.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402
import make_goldens_box4ca as mb  # noqa: E402


def tracks_of(rng, n_tracks, n_frames):
    """n_tracks tracks over frames 0..n_frames-1, each over a run of consecutive frames."""
    tracks, rows, scores = [], [], []
    for t in range(n_tracks):
        start = int(rng.integers(0, n_frames))
        length = int(rng.integers(1, min(6, n_frames - start) + 1))
        score = np.float32(rng.uniform(0.5, 1.0))
        traj = []
        for f in range(start, start + length):
            b2 = rng.uniform(0, 1200, 4).astype(np.float32)
            b3 = np.concatenate([rng.uniform(1.3, 4.5, 3), rng.uniform(-20, 20, 1), rng.uniform(1, 2, 1),
                                 rng.uniform(5, 60, 1), rng.uniform(-3, 3, 1)]).astype(np.float32)
            b2, b3 = np.round(b2, 3), np.round(b3, 3)
            traj.append({'frame_id': str(f), 'info': np.array(['Car', '-1', '-1', '-10.0']),
                         'boxes2d': b2, 'boxes3d': b3, 'scores': score})
            rows.append([t, f] + list(b2.astype(np.float64)) + list(b3.astype(np.float64)))
        tracks.append({'trajectory': traj, 'max_score': score, 'start_frame': start})
        scores.append(score)
    return tracks, np.asarray(rows, np.float64), np.asarray(scores, np.float32)


def main():
    mb.import_evaluator()
    import avod.core.dt_evaluator_utils as deu
    rng = np.random.default_rng(20261016)
    out = {}
    for case, (n_tracks, n_frames) in enumerate([(3, 5), (12, 20), (130, 8)]):
        tracks, rows, scores = tracks_of(rng, n_tracks, n_frames)
        table = deu.convert_trajectory_to_kitti_format(tracks)
        out['c%d_rows' % case], out['c%d_scores' % case] = rows, scores
        out['c%d_table' % case] = table.astype(str)
        print('case', case, ':', n_tracks, 'tracks ->', table.shape, table.dtype)
    tracks, _, _ = tracks_of(rng, 0, 1)
    out['empty_table'] = np.asarray(deu.convert_trajectory_to_kitti_format(tracks)).astype(str)
    np.savez_compressed(os.path.join(mg.HERE, 'trajectory.npz'), **out)


if __name__ == '__main__':
    main()
