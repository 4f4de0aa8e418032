"""FramePairPipeline(tracker=dict(kind='kalman', lanes=True)) on the device: two videos side by side, pair p of every
step in lane p with its own calibration, image size and ego motion, an idle step, a video that ends early and a third
one that starts in its lane; each lane's tracks against a one-pair-per-step pipeline with the single Kalman tracker and
against the host module on the pipeline's own records; and what such a pipeline refuses.  The bodies are
tests/_kind_lanes_pipeline.py's, shared with the velocity tracker."""
import pytest

import _kind_lanes_pipeline as P
from dodt_amd import device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def world():
    w = P.make_world(device.default_context(), P.Kalman())
    yield w
    P.close_world(w)


def test_two_videos_side_by_side(world):
    got_a, got_b, got_c = P.two_videos_side_by_side(world)
    assert all(t.x_state.shape == (8, 1) for t in got_a + got_b + got_c)
    with pytest.raises(ValueError):              # (the Kalman tracker's objects have no KITTI rows)
        world['lanes'].kitti_tracking_rows(lane=0)


def test_refusals(world):
    P.refusals(world)
