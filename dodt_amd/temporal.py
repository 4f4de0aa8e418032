"""The temporal module "M" of S+T+M on the device, with the host module's own interface
(dodt_amd.core.dt_evaluator_utils): numpy in, numpy out, one dodt_interpolate_pairs launch.

The pipeline runs the same kernel on its detection records in place (FramePairPipeline(temporal=...),
frames()); these wrappers are what the tests compare with the host module and the goldens.
"""
import numpy as np

from dodt_amd import device, ops

MAX_ROWS = 128          # keyframe rows per mark the kernel takes (dodt_interpolate_pairs: max_det <= 128)


def three_d_iou_matrix(boxes_a, boxes_b, ctx=None):
    """(na,nb) 3-D IoU of boxes (na,7) and (nb,7), [x,y,z,l,w,h,ry], computed on the device."""
    ctx = ctx or device.default_context()
    a = np.ascontiguousarray(np.atleast_2d(np.asarray(boxes_a, np.float64)))
    b = np.ascontiguousarray(np.atleast_2d(np.asarray(boxes_b, np.float64)))
    if a.shape[1:] != (7,) or b.shape[1:] != (7,):
        raise ValueError('boxes must be (n,7)')
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)))
    d_out = ctx.empty((len(a), len(b)), np.float64)
    ops.three_d_iou_matrix(ctx, ctx.array(a), len(a), ctx.array(b), len(b), d_out)
    return d_out.download()


def interpolate_non_keyframe_predictions(predictions, n_frames, threshold, recover=None, on_conflict='raise',
                                         ctx=None):
    """dt_evaluator_utils.interpolate_non_keyframe_predictions on the device.  predictions (n,17): box_3d(7), score,
    type, shifted box(7), frame mark (0/1); rows of any other mark are ignored, as by the host.  recover: None, or
    dict(r0_rect=(3,3), tr_velo_to_cam=(3,4), ego=[(trans, matrix, delta)] for frames 1..n_frames-1) -- the host's
    recover callback with kitti_tracking_utils.recovery_coordinate.  Returns n_frames arrays (k,13) float64; raises
    ValueError on a conflict in 'raise' mode."""
    if on_conflict not in ('raise', 'next_best'):
        raise ValueError("on_conflict must be 'raise' or 'next_best'")
    n_frames = int(n_frames)
    ctx = ctx or device.default_context()
    p = np.asarray(predictions, dtype=np.float64).reshape(-1, 17)
    # each keyframe's rows in their own slot, in order: filtering and associating them is what the host does on
    # the mixed array
    split = [p[p[:, -1] == f] for f in range(2)]
    max_det = max(1, len(split[0]), len(split[1]))
    if max_det > MAX_ROWS:
        raise ValueError('at most %d rows per keyframe' % MAX_ROWS)
    rec = np.zeros((1, 2, max_det, 17))
    for f in range(2):
        rec[0, f, :len(split[f])] = split[f]
    counts = np.array([[len(split[0]), len(split[1])]], np.int32)
    d_recover = calib = None
    if recover is not None and n_frames >= 2:
        d_recover = ctx.array(ops.temporal_ego(recover['ego'], n_frames)[None])
        calib = ops.temporal_calib(recover['r0_rect'], recover['tr_velo_to_cam'])
    max_out = 2 * max_det
    d_out = ctx.empty((1, n_frames, max_out, 13), np.float64)
    d_cnt = ctx.empty((1, n_frames), np.int32)
    d_st = ctx.empty((1,), np.int32)
    ops.interpolate_pairs(ctx, ctx.array(rec), ctx.array(counts), 1, max_det, n_frames, threshold, on_conflict,
                          d_out, d_cnt, d_st, d_recover=d_recover, calib=calib, max_out=max_out)
    return unpack_frames(d_out.download(), d_cnt.download(), d_st.download(), on_conflict)[0]


def unpack_frames(out, counts, status, on_conflict):
    """The kernel's outputs (pairs, n_frames, max_out, 13), (pairs, n_frames), (pairs,) -> per pair the host
    function's list of n_frames (k,13) arrays.  Raises ValueError for a pair whose status is a 'raise'-mode
    conflict (the reference's next_idx.remove)."""
    res = []
    for pair in range(out.shape[0]):
        if status[pair] != 0:
            if on_conflict == 'raise':
                raise ValueError('pair %d: two keyframe-0 detections claim the same keyframe-1 detection' % pair)
            raise RuntimeError('pair %d: temporal module status %d' % (pair, status[pair]))
        res.append([out[pair, f, :counts[pair, f]].copy() for f in range(out.shape[1])])
    return res
