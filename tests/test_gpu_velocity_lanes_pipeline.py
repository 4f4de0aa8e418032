"""FramePairPipeline(tracker=dict(kind='velocity', lanes=True)) on the device: two videos side by side, pair p of every
step in lane p with its own calibration, image size and ego motion, an idle step, a video that ends early and a third
one that starts in its lane; each lane's tracks against a one-pair-per-step pipeline with the single velocity tracker
and against the host module on the pipeline's own records; the KITTI rows per lane; and what such a pipeline refuses.
The bodies are tests/_kind_lanes_pipeline.py's, shared with the Kalman tracker."""
import numpy as np
import pytest

import _kind_lanes_pipeline as P
from dodt_amd import device
from dodt_amd.experiments import video_detection_iou as vit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def world():
    w = P.make_world(device.default_context(), P.Velocity())
    yield w
    P.close_world(w)


def test_two_videos_side_by_side(world):
    got_a, got_b, got_c = P.two_videos_side_by_side(world)
    pipe = world['lanes']
    # the KITTI rows are per lane: the last sequence each lane ended
    for lane, got in ((0, got_c), (1, got_b)):
        rows = pipe.kitti_tracking_rows(lane=lane)
        assert rows.shape[1] == 18 and np.array_equal(rows.astype(str),
                                                      vit.convert_trajectory_to_kitti_format(got).astype(str))
    with pytest.raises(ValueError):
        pipe.kitti_tracking_rows()


def test_refusals(world):
    P.refusals(world)
