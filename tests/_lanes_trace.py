"""The recording stand-in for dodt_amd.tracking.TrackerLanes, on top of tests/_geometry_trace.py (which is on top of
tests/_pipeline_trace.py; both are left alone): the lanes launch is logged on the context it is given with every lane's
calibration and the step's `active`, a lane's reset / flush on that lane's slice of the one state buffer."""
import numpy as np

import _geometry_trace as gt
import _pipeline_trace as tr
from dodt_amd import pipeline as pl

STRIDE = 256


class LaneTracker(tr.Tracker):
    """tracking.Tracker over an existing state view."""

    def __init__(self, ctx, d_state):
        self.ctx, self.d_state = ctx, d_state
        self.reset()


class TrackerLanes(object):
    def __init__(self, ctx=None, n_lanes=1, log_capacity=65536, high_threshold=0.5, iou_threshold=0.005, t_min=3,
                 score_threshold=0.1):
        self.ctx, self.n_lanes, self.stride = ctx, int(n_lanes), STRIDE
        self.d_states = ctx.empty((self.n_lanes * STRIDE,), np.uint8)
        self.lanes = [LaneTracker(ctx, self.d_states.offset(i * STRIDE, (64,), np.uint8)) for i in range(self.n_lanes)]

    def lane(self, i):
        return self.lanes[i]

    def track_records(self, d_records, d_counts, max_det, p2s, image_whs, active=None, ctx=None):
        (ctx or self.ctx).log('track_lanes', [self.d_states, d_records, d_counts, max_det, list(p2s), list(image_whs),
                                              None if active is None else tuple(active)])


def install(monkeypatch):
    """gt.install() with TrackerLanes in place of the pipeline's.  -> (build, uploads)."""
    build, uploads = gt.install(monkeypatch)
    monkeypatch.setattr(pl.tracking, 'TrackerLanes', TrackerLanes)
    return build, uploads
