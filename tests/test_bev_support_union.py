"""The BEV skip tables under a changing calibration: the mask in force is the OR of the masks of every calibration seen so
far, and the tables are rebuilt only when it gains a cell.  The masks are the real ones (ops.bev_support_mask, host
code) of the three real calibrations of tests/golden/all_frames.json, fed in the order A, B, A, C, B -- to the rule
itself (pipeline.SupportUnion), and through FramePairPipeline over the recording stand-ins, whose BEV net logs every
set_input_support() so that the mask in force at each BEV forward can be read off the trace."""
import types

import numpy as np

import _geometry_trace as gt
import _pipeline_trace as tr
from dodt_amd import config, ops
from dodt_amd import pipeline as pl

A, B, C = gt.real_calibrations()
ORDER = (A, B, A, C, B)
PAD = 4


def _mask(calib):
    bp = ops.make_bev_params(config.PYRAMID_DODT, config.velo_to_cam(calib.r0_rect, calib.tr_velo_to_cam), calib.p2,
                             calib.image_wh)
    return ops.bev_support_mask(bp, PAD)


def test_the_real_masks_differ():
    """The premise: no one of the three supports holds the other two (else a union would never grow)."""
    m = [_mask(c) != 0 for c in (A, B, C)]
    assert all(x.shape == (PAD + 700, 800) and x.any() and not x.all() for x in m)
    assert np.any(m[1] & ~m[0]) and np.any(m[2] & ~(m[0] | m[1]))


def test_union_rule():
    geoms = {c.key(): types.SimpleNamespace(key=c.key(), calib=c) for c in (A, B, C)}
    calls = []

    def mask_of(g):
        calls.append(g.key)
        return _mask(g.calib)
    u = pl.SupportUnion(mask_of)
    grew = []
    for c in ORDER:
        grew.append(u.add([geoms[c.key()]]))
        own = _mask(c) != 0
        assert not np.any(own & (u.mask == 0))          # its own mask lies inside the mask in force at its step
    assert grew == [True, True, False, True, False] and u.rebuilds == 3
    assert len(calls) == 3                               # each calibration's mask is made once
    assert np.array_equal(u.mask != 0, (_mask(A) != 0) | (_mask(B) != 0) | (_mask(C) != 0))
    assert u.mask.dtype == np.uint8
    # a calibration whose support lies inside the union rebuilds nothing
    inside = types.SimpleNamespace(key='inside', calib=None)
    v = pl.SupportUnion(lambda g: _mask(A) if g.calib is None else _mask(g.calib))
    assert v.add([geoms[A.key()]]) and not v.add([inside]) and v.rebuilds == 1


class _RealMaskOps(tr.Ops):
    """The stand-in ops with the real bev parameters and the real support mask."""
    make_bev_params = staticmethod(ops.make_bev_params)
    with_ego_motion = staticmethod(ops.with_ego_motion)
    bev_support_mask = staticmethod(ops.bev_support_mask)


class _SkipNet(tr._net((700, 800, 32))):
    def set_input_support(self, mask, frame_tables=False):
        self.ctx.log('set_input_support', [np.array(mask, copy=True), bool(frame_tables)])
        return int(np.count_nonzero(mask == 0))


def test_a_dropped_pipeline_is_freed_at_once(monkeypatch):
    """A pipeline frees gigabytes of device memory when its last reference goes; a reference cycle through the mask
    logic would leave that to the cycle collector, which may run in the middle of another pipeline's steps."""
    import gc
    import weakref
    build, _ = gt.install(monkeypatch, ops=_RealMaskOps())
    monkeypatch.setitem(pl.EXTRACTORS, 'vgg_pyr', (_SkipNet, tr._net((360, 1200, 32))))
    first, trace, c = build()
    gc.collect()
    gc.disable()
    try:
        pipe = pl.FramePairPipeline(c['main'], config.PYRAMID_DODT, {}, {}, reuse_streams_of=first, bev_input_skip=True)
        assert pipe.support is not None
        ins = [list(a) for a in zip(*[gt.frame(pipe, B) for _ in range(2)])]
        pipe.run(*ins, heads=tr._heads(pipe), calib=B)
        pipe.finish()
        ref = weakref.ref(pipe)
        del pipe
        assert ref() is None
    finally:
        gc.enable()


def test_through_the_pipeline(monkeypatch):
    build, _ = gt.install(monkeypatch, ops=_RealMaskOps())
    monkeypatch.setitem(pl.EXTRACTORS, 'vgg_pyr', (_SkipNet, tr._net((360, 1200, 32))))
    first, trace, c = build()
    pipe = pl.FramePairPipeline(c['main'], config.PYRAMID_DODT, {}, {}, reuse_streams_of=first, bev_input_skip=True,
                                bev_frame_tables=False)
    heads = tr._heads(pipe)
    start = len(trace)
    skipped = []
    ins = [[list(a) for a in zip(*[gt.frame(pipe, cal) for _ in range(2)])] for cal in ORDER]
    for k, cal in enumerate(ORDER):
        # (with a look-ahead on two steps, which brings the NEXT calibration a call early: the rebuild belongs in front
        #  of that step's BEV forward, not in its prep)
        nxt = tuple(ins[k + 1]) + (None, ORDER[k + 1]) if k in (1, 2) else None
        pipe.run(*ins[k], heads=heads, calib=None if k == 0 else cal, lookahead=nxt)
        skipped.append(pipe.bev_skipped_items)
    pipe.finish()
    sets = [t for t in trace if t['op'] == 'set_input_support']
    assert len(sets) == 3 and pipe.support.rebuilds == 3            # the constructor's (A), then B, then C
    assert all(t['stream'] == 'main' and t['args'][1] is False for t in sets)
    in_force, at_forward = None, []
    for i, t in enumerate(trace):
        if t['op'] == 'set_input_support':
            in_force = t['args'][0] != 0
        elif t['op'] == 'forward_device_padded' and t['stream'] == 'main' and i >= start:
            at_forward.append(in_force)
    assert len(at_forward) == len(ORDER)
    for cal, m in zip(ORDER, at_forward):
        assert not np.any((_mask(cal) != 0) & ~m)
    # the union only grows, so what is skipped only shrinks; bev_skipped_items reports the current union's count
    assert skipped[0] > skipped[1] == skipped[2] > skipped[3] == skipped[4]
    assert skipped[4] == int(np.count_nonzero(pipe.support.mask == 0))
