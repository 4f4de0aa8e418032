"""convert_trajectory_to_kitti_format (avod/core/dt_evaluator_utils.py:514-532) on the host against the
reference's own output on the same tracks (tests/golden/make_goldens_trajectory.py), including a case with
130 tracks, whose ids of 100 and more interleave with later frames under the sort key 100 * frame + id."""
import os

import numpy as np
import pytest

from dodt_amd.core import dt_evaluator_utils as host

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'trajectory.npz'))


def _tracks(case):
    rows, scores = G['c%d_rows' % case], G['c%d_scores' % case]
    tracks = [{'trajectory': [], 'max_score': scores[t], 'start_frame': None} for t in range(len(scores))]
    for r in rows:
        tracks[int(r[0])]['trajectory'].append({
            'frame_id': str(int(r[1])), 'info': np.array(['Car', '-1', '-1', '-10.0']),
            'boxes2d': r[2:6].astype(np.float32), 'boxes3d': r[6:13].astype(np.float32), 'scores': scores[int(r[0])]})
    for t in tracks:
        t['start_frame'] = int(t['trajectory'][0]['frame_id'])
    return tracks


@pytest.mark.parametrize('case', [0, 1, 2])
def test_convert_trajectory_matches_reference(case):
    got = host.convert_trajectory_to_kitti_format(_tracks(case))
    want = G['c%d_table' % case]
    assert got.shape == want.shape and got.shape[1] == 18
    assert np.array_equal(got.astype(str), want)


def test_convert_trajectory_sort_key_interleaves_large_ids():
    got = host.convert_trajectory_to_kitti_format(_tracks(2))
    frames, ids = got[:, 0].astype(int), got[:, 1].astype(int)
    assert ids.max() >= 100
    key = 100 * frames + ids
    assert np.all(np.diff(key) >= 0)
    assert np.any(np.diff(frames) < 0)              # as written: not sorted by frame once ids reach 100


def test_convert_trajectory_accepts_list_info_and_empty():
    tracks = _tracks(0)
    for t in tracks:
        for d in t['trajectory']:
            d['info'] = list(d['info'])             # encode_tracking_dets' items hold a list
    assert np.array_equal(host.convert_trajectory_to_kitti_format(tracks).astype(str), G['c0_table'])
    assert host.convert_trajectory_to_kitti_format([]).shape == G['empty_table'].shape == (0,)
