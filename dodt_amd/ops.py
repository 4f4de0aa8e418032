"""Thin device-level wrappers: DeviceArray in, DeviceArray out, one C-ABI call each.

These are what the frame-pair pipeline is made of; the avod.core-shaped host API
in dodt_amd/core/ wraps them with numpy upload/download.
"""
import ctypes as C

import numpy as np

from dodt_amd import _lib


def _arr(ctype, values):
    values = [float(v) for v in np.asarray(values, dtype=np.float64).reshape(-1)]
    return (ctype * len(values))(*values)


def _p(a):
    return None if a is None else C.c_void_p(a.ptr)


def make_bev_params(cfg, velo_to_cam=None, p2=None, im_wh=None,
                    point_format=_lib.PTS_VELO_XYZI, ground_plane=None,
                    area_extents=None, voxel_size=None):
    """dodt_bev_params from a config dict (dodt_amd.config) and calibration."""
    bp = _lib.BevParams()
    bp.point_format = point_format
    bp.num_slices = int(cfg['num_slices'])
    m = np.zeros(12) if velo_to_cam is None else \
        np.asarray(velo_to_cam, dtype=np.float64).reshape(-1)[:12]
    p = np.zeros(12) if p2 is None else np.asarray(p2, dtype=np.float64).reshape(-1)
    bp.velo_to_cam = (C.c_double * 12)(*m)
    bp.p2 = (C.c_double * 12)(*p)
    bp.im_w, bp.im_h = (0.0, 0.0) if im_wh is None else (float(im_wh[0]), float(im_wh[1]))
    plane = cfg['ground_plane'] if ground_plane is None else ground_plane
    bp.plane = (C.c_double * 4)(*[float(v) for v in plane])
    ext = cfg['area_extents'] if area_extents is None else area_extents
    bp.extents = (C.c_double * 6)(*[float(v) for v in np.asarray(ext).reshape(-1)])
    bp.voxel_size = float(cfg['voxel_size'] if voxel_size is None else voxel_size)
    bp.height_lo = float(cfg['height_lo'])
    bp.height_hi = float(cfg['height_hi'])
    bp.occ_lo = float(cfg['anchor_filter_lo'])
    bp.occ_hi = float(cfg['anchor_filter_hi'])
    bp.has_pre_transform = 0
    return bp


def with_ego_motion(bev_params, trans, matrix):
    """Copy of bev_params that registers a pair's second frame into the first frame's
    coordinates first: p' = (p + trans) @ matrix in the velodyne frame
    (kitti_tracking_dataset.py:303-335; trans, matrix from
    dodt_amd.datasets.kitti.kitti_tracking_utils.coordinate_transform)."""
    bp = _lib.BevParams.from_buffer_copy(bev_params)
    t = np.asarray(trans, np.float64).reshape(3)
    m = np.asarray(matrix, np.float64).reshape(9)
    bp.has_pre_transform = 1
    bp.pre_translate = (C.c_double * 3)(*t)
    bp.pre_rotate = (C.c_double * 9)(*m)
    return bp


def bev_slices(ctx, d_points, n_points, bev_params, d_bev_out, d_occ_bits=None):
    _lib.check(ctx.lib.dodt_bev_slices(ctx.handle, _p(d_points), int(n_points),
                                       C.byref(bev_params), _p(d_bev_out),
                                       _p(d_occ_bits)), 'dodt_bev_slices')


def bev_support_mask(bev_params, pad_top=0, lib=None):
    """(pad_top + Z, X) uint8: the BEV cells dodt_bev_slices can ever write under bev_params (velodyne points: the
    image-frustum filter), in a pyramid extractor's padded input layout; host only (dodt_bev_support_mask)."""
    lib = lib or _lib.load()
    vs = bev_params.voxel_size
    ext = list(bev_params.extents)
    nx = int(np.ceil(ext[1] / vs - 1) - np.floor(ext[0] / vs) + 1)
    nz = int(np.ceil(ext[5] / vs - 1) - np.floor(ext[4] / vs) + 1)
    out = np.zeros((int(pad_top) + nz, nx), np.uint8)
    _lib.check(lib.dodt_bev_support_mask(C.byref(bev_params), int(pad_top), out.ctypes.data, out.shape[0],
                                         out.shape[1]), 'dodt_bev_support_mask')
    return out


def frame_tables_host(masks, layer, th, tw, items, prev=None, lib=None):
    """The per-frame skip-table rule of the fp32 pyramid net on the host (dodt_frame_tables_host): masks (frames, rows,
    cols) non-zero where each frame's padded input is, layer 0 .. 15 in launch order, items (n, 4) int32 {frame,
    channel tile, y0, x0} in table order with th x tw tiles; prev (n,) uint8: the items the last forward reached.
    Returns the (k, 4) items the forward runs, in table order."""
    lib = lib or _lib.load()
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    items = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 4)
    prev = None if prev is None else np.ascontiguousarray(prev, dtype=np.uint8)
    run = np.zeros((max(len(items), 1), 4), np.int32)
    n = C.c_int()
    _lib.check(lib.dodt_frame_tables_host(masks.ctypes.data, masks.shape[0], masks.shape[1], masks.shape[2], int(layer),
                                          int(th), int(tw), items.ctypes.data, len(items),
                                          None if prev is None else prev.ctypes.data, run.ctypes.data, C.byref(n)),
               'dodt_frame_tables_host')
    return run[:n.value].copy()


def frame_lists_host(masks, layer, th, tw, items, prev=None, lib=None):
    """The two lists of frame_tables_host's union (dodt_frame_lists_host), each (k, 4) in table order: the items this
    input reaches (computed) and the items of prev it does not reach (restored from the constants store)."""
    lib = lib or _lib.load()
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    items = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 4)
    prev = None if prev is None else np.ascontiguousarray(prev, dtype=np.uint8)
    run = np.zeros((max(len(items), 1), 4), np.int32)
    restore = np.zeros((max(len(items), 1), 4), np.int32)
    n, nr = C.c_int(), C.c_int()
    _lib.check(lib.dodt_frame_lists_host(masks.ctypes.data, masks.shape[0], masks.shape[1], masks.shape[2], int(layer),
                                         int(th), int(tw), items.ctypes.data, len(items),
                                         None if prev is None else prev.ctypes.data, run.ctypes.data, C.byref(n),
                                         restore.ctypes.data, C.byref(nr)),
               'dodt_frame_lists_host')
    return run[:n.value].copy(), restore[:nr.value].copy()


def frame_restore_host(item, f, th, tw, bn, ch0, dst, src, dst2=None, src2=None, pad_top=-1, lib=None):
    """The copy the restore launch makes for one item, on host arrays and in place (dodt_frame_restore_host).  pad_top
    < 0: dst (frames, C / 8, rows, cols, 8) channel-blocked, src one frame of it, dst2 / src2 the pooled maps.
    pad_top >= 0: dst (frames, rows - pad_top, cols, C) NHWC, src one frame of it, dst2 / src2 the bottleneck maps."""
    lib = lib or _lib.load()
    for a in (dst, src, dst2, src2):
        assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous)
    item = np.ascontiguousarray(item, dtype=np.int32)
    if pad_top < 0:
        rows, cols, channels = dst.shape[2], dst.shape[3], dst.shape[1] * 8
    else:
        rows, cols, channels = dst.shape[1] + pad_top, dst.shape[2], dst.shape[3]
    _lib.check(lib.dodt_frame_restore_host(item.ctypes.data, int(f), int(th), int(tw), int(bn), int(ch0), rows, cols,
                                           channels, int(pad_top), dst.ctypes.data, src.ctypes.data,
                                           None if dst2 is None else dst2.ctypes.data,
                                           None if src2 is None else src2.ctypes.data), 'dodt_frame_restore_host')


def bev_status(ctx):
    f = C.c_int()
    _lib.check(ctx.lib.dodt_bev_status(ctx.handle, C.byref(f)), 'dodt_bev_status')
    return f.value


def anchor_filter(ctx, d_occ_bits, nx, nz, d_cells, n_anchors, d_keep_idx, d_count,
                  density_threshold=1):
    _lib.check(ctx.lib.dodt_anchor_filter(
        ctx.handle, _p(d_occ_bits), int(nx), int(nz), _p(d_cells), int(n_anchors),
        int(density_threshold), _p(d_keep_idx), _p(d_count)), 'dodt_anchor_filter')


def project_anchors_f64(ctx, d_anchors, d_idx, n, d_n, bev_extents, p2, im_wh,
                        d_bev_norm=None, d_img_norm=None, d_anchors_f32=None):
    _lib.check(ctx.lib.dodt_project_anchors_f64(
        ctx.handle, _p(d_anchors), _p(d_idx), int(n), _p(d_n),
        _arr(C.c_double, bev_extents), _arr(C.c_double, p2),
        float(im_wh[0]), float(im_wh[1]), _p(d_bev_norm), _p(d_img_norm),
        _p(d_anchors_f32)), 'dodt_project_anchors_f64')


def project_anchors_f32(ctx, d_anchors, n, d_n, bev_extents, p2, im_wh,
                        d_bev=None, d_bev_norm_tf=None, d_img_norm_tf=None):
    _lib.check(ctx.lib.dodt_project_anchors_f32(
        ctx.handle, _p(d_anchors), int(n), _p(d_n), _arr(C.c_float, bev_extents),
        _arr(C.c_float, p2), float(im_wh[0]), float(im_wh[1]), _p(d_bev),
        _p(d_bev_norm_tf), _p(d_img_norm_tf)), 'dodt_project_anchors_f32')


def img_preprocess(ctx, d_img_u8, in_hw, out_hw, out_c, mean_rgb, d_out):
    _lib.check(ctx.lib.dodt_img_preprocess(
        ctx.handle, _p(d_img_u8), int(in_hw[0]), int(in_hw[1]), int(out_hw[0]),
        int(out_hw[1]), int(out_c), _arr(C.c_float, mean_rgb), _p(d_out)),
        'dodt_img_preprocess')


def crop_and_resize(ctx, d_image, hwc, d_boxes, n, d_n, crop_hw, d_out, out_box_stride=None):
    """out_box_stride (floats): box b's crop starts at d_out + b * out_box_stride (default: packed)."""
    if out_box_stride is None:
        out_box_stride = int(crop_hw[0]) * int(crop_hw[1]) * int(hwc[2])
    _lib.check(ctx.lib.dodt_crop_and_resize_strided(
        ctx.handle, _p(d_image), int(hwc[0]), int(hwc[1]), int(hwc[2]), _p(d_boxes),
        int(n), _p(d_n), int(crop_hw[0]), int(crop_hw[1]), _p(d_out), int(out_box_stride)),
        'dodt_crop_and_resize')


def crop_and_resize_indexed(ctx, d_image, hwc, d_boxes, n_boxes, d_box_idx, n, d_n, crop_hw, d_out,
                            out_box_stride=None):
    """crop_and_resize whose output row j (j < min(n, *d_n)) is the crop at box d_box_idx[j] of the n_boxes boxes."""
    if out_box_stride is None:
        out_box_stride = int(crop_hw[0]) * int(crop_hw[1]) * int(hwc[2])
    _lib.check(ctx.lib.dodt_crop_and_resize_indexed(
        ctx.handle, _p(d_image), int(hwc[0]), int(hwc[1]), int(hwc[2]), _p(d_boxes), int(n_boxes),
        _p(d_box_idx), int(n), _p(d_n), int(crop_hw[0]), int(crop_hw[1]), _p(d_out), int(out_box_stride)),
        'dodt_crop_and_resize_indexed')


def nms_plan(n, max_out):
    """What dodt_nms decides on the host for (n, max_out): the fields of dodt_nms_plan plus 'chunks', the
    (row0, rows) of its mask + scan launch pairs in order (dodt_nms_plan_host).  Host only: needs no GPU."""
    lib = _lib.load()
    p = _lib.NmsPlan()
    _lib.check(lib.dodt_nms_plan_host(int(n), int(max_out), C.byref(p), None, 0), 'dodt_nms_plan_host')
    chunks = (C.c_int32 * (2 * p.n_chunks))()
    _lib.check(lib.dodt_nms_plan_host(int(n), int(max_out), C.byref(p), chunks, p.n_chunks), 'dodt_nms_plan_host')
    plan = dict((name, int(getattr(p, name))) for name, _ in p._fields_)
    plan['ranked'] = bool(p.ranked)
    plan['chunks'] = [(int(chunks[2 * c]), int(chunks[2 * c + 1])) for c in range(p.n_chunks)]
    return plan


def nms_scratch_bytes(ctx):
    """Bytes of the context's NMS scratch (dodt_nms_scratch_bytes): grown, with a quarter to spare, whenever a call's
    plan needs more than there is."""
    return int(ctx.lib.dodt_nms_scratch_bytes(ctx.handle))


def nms(ctx, d_boxes, d_scores, n, d_n, max_out, iou_threshold, d_sel, d_count):
    _lib.check(ctx.lib.dodt_nms(
        ctx.handle, _p(d_boxes), _p(d_scores), int(n), _p(d_n), int(max_out),
        float(iou_threshold), _p(d_sel), _p(d_count)), 'dodt_nms')


def offset_to_anchor(ctx, d_anchors, d_offsets, n, d_n, d_out):
    _lib.check(ctx.lib.dodt_offset_to_anchor(
        ctx.handle, _p(d_anchors), _p(d_offsets), int(n), _p(d_n), _p(d_out)),
        'dodt_offset_to_anchor')


def softmax_fg(ctx, d_logits, n, d_n, d_scores):
    _lib.check(ctx.lib.dodt_softmax_fg(
        ctx.handle, _p(d_logits), int(n), _p(d_n), _p(d_scores)), 'dodt_softmax_fg')


def rpn_decode(ctx, d_anchors, d_offsets, d_logits, n, d_n, bev_extents, d_regressed, d_bev_norm_tf, d_scores):
    """offset_to_anchor + project_anchors_f32 (normalised BEV boxes) + softmax_fg in one launch."""
    _lib.check(ctx.lib.dodt_rpn_decode(
        ctx.handle, _p(d_anchors), _p(d_offsets), _p(d_logits), int(n), _p(d_n), _arr(C.c_float, bev_extents),
        _p(d_regressed), _p(d_bev_norm_tf), _p(d_scores)), 'dodt_rpn_decode')


def gather_project(ctx, d_src, d_idx, n, d_n, bev_extents, p2, im_wh, d_rows, d_bev_norm_tf, d_img_norm_tf):
    """gather_rows (width 6) + project_anchors_f32 (both views) in one launch."""
    _lib.check(ctx.lib.dodt_gather_project(
        ctx.handle, _p(d_src), _p(d_idx), int(n), _p(d_n), _arr(C.c_float, bev_extents), _arr(C.c_float, p2),
        float(im_wh[0]), float(im_wh[1]), _p(d_rows), _p(d_bev_norm_tf), _p(d_img_norm_tf)), 'dodt_gather_project')


def final_decode(ctx, d_top_anchors, d_offsets, d_cls_logits, d_angle_vectors, n, d_n, plane, bev_extents,
                 d_boxes_3d, d_pred_anchors, d_bev_tf, d_nms_scores, d_det_scores, d_orientations):
    """box_4c_decode + max_fg_logit + softmax_fg [+ angle_vector_to_orientation] in one launch."""
    _lib.check(ctx.lib.dodt_final_decode(
        ctx.handle, _p(d_top_anchors), _p(d_offsets), _p(d_cls_logits), _p(d_angle_vectors), int(n), _p(d_n),
        _arr(C.c_float, plane), _arr(C.c_float, bev_extents), _p(d_boxes_3d), _p(d_pred_anchors), _p(d_bev_tf),
        _p(d_nms_scores), _p(d_det_scores), _p(d_orientations)), 'dodt_final_decode')


def gather_rows(ctx, d_src, width, d_idx, n, d_n, d_out):
    _lib.check(ctx.lib.dodt_gather_rows(
        ctx.handle, _p(d_src), int(width), _p(d_idx), int(n), _p(d_n), _p(d_out)),
        'dodt_gather_rows')


def box_4c_decode(ctx, d_top_anchors, d_offsets, n, d_n, plane, bev_extents,
                  d_boxes_3d=None, d_pred_anchors=None, d_bev_tf=None):
    _lib.check(ctx.lib.dodt_box_4c_decode(
        ctx.handle, _p(d_top_anchors), _p(d_offsets), int(n), _p(d_n),
        _arr(C.c_float, plane), _arr(C.c_float, bev_extents), _p(d_boxes_3d),
        _p(d_pred_anchors), _p(d_bev_tf)), 'dodt_box_4c_decode')


def max_fg_logit(ctx, d_logits, n_cls, n, d_n, d_scores):
    _lib.check(ctx.lib.dodt_max_fg_logit(
        ctx.handle, _p(d_logits), int(n_cls), int(n), _p(d_n), _p(d_scores)),
        'dodt_max_fg_logit')


def angle_vector_to_orientation(ctx, d_angle_vectors, n, d_n, d_orientations):
    _lib.check(ctx.lib.dodt_angle_vector_to_orientation(
        ctx.handle, _p(d_angle_vectors), int(n), _p(d_n), _p(d_orientations)),
        'dodt_angle_vector_to_orientation')


def pack_detections(ctx, d_boxes_3d, d_scores, d_sel, d_count, max_det, frame_mark,
                    d_rec, d_count_out, d_corr_offsets=None, d_orientations=None):
    _lib.check(ctx.lib.dodt_pack_detections(
        ctx.handle, _p(d_boxes_3d), _p(d_scores), _p(d_orientations), _p(d_corr_offsets),
        _p(d_sel), _p(d_count), int(max_det), float(frame_mark), _p(d_rec), _p(d_count_out)),
        'dodt_pack_detections')


def pack_detections_compact(ctx, d_boxes_3d, d_scores, d_sel, d_count, max_det, frame_mark,
                            d_rec, d_count_out, d_det_offsets=None, d_orientations=None):
    """pack_detections with one row of offsets per detection: d_det_offsets (max_det, 3), row j for box d_sel[j]."""
    _lib.check(ctx.lib.dodt_pack_detections_compact(
        ctx.handle, _p(d_boxes_3d), _p(d_scores), _p(d_orientations), _p(d_det_offsets),
        _p(d_sel), _p(d_count), int(max_det), float(frame_mark), _p(d_rec), _p(d_count_out)),
        'dodt_pack_detections_compact')


def class_scores(ctx, d_logits, n_cls, n, d_n, d_scores, d_types):
    """Record score (largest non-background softmax value) and type (its index among the non-background columns, the
    first maximum; int32) of n rows of (n, n_cls) logits (dodt_class_scores)."""
    _lib.check(ctx.lib.dodt_class_scores(
        ctx.handle, _p(d_logits), int(n_cls), int(n), _p(d_n), _p(d_scores), _p(d_types)), 'dodt_class_scores')


def final_decode_classes(ctx, d_top_anchors, d_offsets, d_cls_logits, n_cls, d_angle_vectors, n, d_n, plane,
                         bev_extents, d_boxes_3d, d_pred_anchors, d_bev_tf, d_nms_scores, d_det_scores, d_det_types,
                         d_orientations):
    """final_decode for (n, n_cls) logits: box_4c_decode + max_fg_logit + class_scores [+ angle_vector_to_orientation]
    in one launch."""
    _lib.check(ctx.lib.dodt_final_decode_classes(
        ctx.handle, _p(d_top_anchors), _p(d_offsets), _p(d_cls_logits), int(n_cls), _p(d_angle_vectors), int(n),
        _p(d_n), _arr(C.c_float, plane), _arr(C.c_float, bev_extents), _p(d_boxes_3d), _p(d_pred_anchors),
        _p(d_bev_tf), _p(d_nms_scores), _p(d_det_scores), _p(d_det_types), _p(d_orientations)),
        'dodt_final_decode_classes')


def pack_detections_classes(ctx, d_boxes_3d, d_scores, d_types, d_sel, d_count, max_det, frame_mark,
                            d_rec, d_count_out, d_corr_offsets=None, d_orientations=None):
    """pack_detections with record column 8 = d_types[d_sel[row]] (d_types None: 0)."""
    _lib.check(ctx.lib.dodt_pack_detections_classes(
        ctx.handle, _p(d_boxes_3d), _p(d_scores), _p(d_types), _p(d_orientations), _p(d_corr_offsets),
        _p(d_sel), _p(d_count), int(max_det), float(frame_mark), _p(d_rec), _p(d_count_out)),
        'dodt_pack_detections_classes')


def pack_detections_compact_classes(ctx, d_boxes_3d, d_scores, d_types, d_sel, d_count, max_det, frame_mark,
                                    d_rec, d_count_out, d_det_offsets=None, d_orientations=None):
    """pack_detections_compact with record column 8 = d_types[d_sel[row]] (d_types None: 0)."""
    _lib.check(ctx.lib.dodt_pack_detections_compact_classes(
        ctx.handle, _p(d_boxes_3d), _p(d_scores), _p(d_types), _p(d_orientations), _p(d_det_offsets),
        _p(d_sel), _p(d_count), int(max_det), float(frame_mark), _p(d_rec), _p(d_count_out)),
        'dodt_pack_detections_compact_classes')


def fetch_i32_begin(ctx, d_src, n, slot):
    _lib.check(ctx.lib.dodt_fetch_i32_begin(ctx.handle, _p(d_src), int(n), int(slot)),
               'dodt_fetch_i32_begin')


def fetch_i32_end(ctx, slot, n):
    buf = (C.c_int32 * n)()
    _lib.check(ctx.lib.dodt_fetch_i32_end(ctx.handle, int(slot), buf, int(n)),
               'dodt_fetch_i32_end')
    return list(buf)


def correlation(ctx, d_a, d_b, hwc, max_displacement, stride_2, pad, d_out):
    _lib.check(ctx.lib.dodt_correlation(
        ctx.handle, _p(d_a), _p(d_b), int(hwc[0]), int(hwc[1]), int(hwc[2]),
        int(max_displacement), int(stride_2), int(pad), _p(d_out)), 'dodt_correlation')


def correlation_tile_list(ctx, out_hw, d_boxes, n_boxes, d_box_idx, n, d_n, crop_hw, d_tiles, capacity, d_n_tiles):
    """The 16 x 16 tiles of an out_hw correlation map that crops at boxes d_box_idx[0 .. min(n, *d_n)) can read
    (a superset), in the kernel's walking order, into d_tiles (capacity ints) and their number into d_n_tiles."""
    _lib.check(ctx.lib.dodt_correlation_tile_list(
        ctx.handle, int(out_hw[0]), int(out_hw[1]), _p(d_boxes), int(n_boxes), _p(d_box_idx), int(n), _p(d_n),
        int(crop_hw[0]), int(crop_hw[1]), _p(d_tiles), int(capacity), _p(d_n_tiles)), 'dodt_correlation_tile_list')


def correlation_tiles(ctx, d_a, d_b, hwc, max_displacement, stride_2, pad, d_tiles, capacity, d_n_tiles, d_out):
    """correlation() over the listed tiles only; the rest of d_out is left as it is."""
    _lib.check(ctx.lib.dodt_correlation_tiles(
        ctx.handle, _p(d_a), _p(d_b), int(hwc[0]), int(hwc[1]), int(hwc[2]), int(max_displacement),
        int(stride_2), int(pad), _p(d_tiles), int(capacity), _p(d_n_tiles), _p(d_out)), 'dodt_correlation_tiles')


# the largest map correlation_tile_list takes, in tiles (its flags live in one workgroup's LDS: kListMaxTiles)
CORR_TILE_LIST_MAX = 8192


def correlation_tile_capacity(out_hw):
    """Entries a tile list of an out_hw map needs."""
    return -(-int(out_hw[0]) // 16) * -(-int(out_hw[1]) // 16)


def mean_fusion(ctx, d_a, d_b, rows, d_n, row_floats, d_out):
    """d_out = (d_a + d_b) / 2 over min(*d_n, rows) rows of row_floats floats."""
    _lib.check(ctx.lib.dodt_mean_fusion(ctx.handle, _p(d_a), _p(d_b), int(rows), _p(d_n),
                                        int(row_floats), _p(d_out)), 'dodt_mean_fusion')


def rows_to_bf16(ctx, d_a, d_b, rows, d_n, row_floats, in_ld, d_out, out_ld):
    """d_out (rows, out_ld) bf16 (uint16 storage) = bf16((d_a + d_b) / 2) [bf16(d_a) when d_b is None] over the first
    row_floats elements of min(*d_n, rows) rows (input rows in_ld floats apart), zeros behind them: the first
    layer's rows of a bf16 head (dodt_rows_to_bf16)."""
    _lib.check(ctx.lib.dodt_rows_to_bf16(ctx.handle, _p(d_a), _p(d_b), int(rows), _p(d_n), int(row_floats),
                                         int(in_ld), _p(d_out), int(out_ld)), 'dodt_rows_to_bf16')


def bf16_to_float(a):
    """uint16 array of bf16 bit patterns -> float32 (host side of tests and tools)."""
    return (np.asarray(a, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _fc_plan_record(p):
    rec = dict((name, int(getattr(p, name))) for name, _ in p._fields_ if name not in ('name', 'grid'))
    rec['name'] = p.name.decode('ascii')
    rec['grid'] = (int(p.grid[0]), int(p.grid[1]))
    return rec


def fc_plan_host(K, N, M, dtype='f32', ldx=None, ldy=None, x_off=0, x2_off=None, y_off=0, x_bf16=False, y_bf16=False,
                 bf16_bk=32, lib=None):
    """Which kernel a call of a (K, N) layer would run, the fields of dodt_fc_plan as a dict: 'name' / 'form' the
    selector's form ('kNone': the call is refused), 'xvec' / 'fuse' the register-staged kernel's instantiation,
    'vec_store' the small-K kernel's row store, 'grid', and the layer's traits.  x_off, x2_off, y_off: the addresses
    modulo 16 (x2_off None: no second input); bf16_bk: DODT_FC_BF16_DMA_BK of the creating process.  Host only:
    needs no GPU (dodt_fc_plan_host)."""
    lib = lib or _lib.load()
    p = _lib.FcPlan()
    _lib.check(lib.dodt_fc_plan_host(
        int(K), int(N), _lib.FC_BF16 if dtype == 'bf16' else 0, int(M), int(K if ldx is None else ldx),
        int(N if ldy is None else ldy), int(x_off), -1 if x2_off is None else int(x2_off), int(y_off),
        1 if x_bf16 else 0, 1 if y_bf16 else 0, int(bf16_bk), C.byref(p)), 'dodt_fc_plan_host')
    return _fc_plan_record(p)


class FullyConnected(object):
    """y = act(x w + b) on the device (dodt_fc_*).  w (K,N) row-major, the layout of the
    TF variable (conv kernels reshaped (kh*kw*cin, cout))."""

    def __init__(self, ctx, w, b, relu, dtype='f32'):
        """dtype 'bf16': bf16 MFMA, fp32 accumulate (DODT_FC_BF16)."""
        if dtype not in ('f32', 'bf16'):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if w.ndim != 2 or b.shape != (w.shape[1],):
            raise ValueError('weights must be (K,N) and bias (N,)')
        self.ctx, self.K, self.N, self.dtype = ctx, int(w.shape[0]), int(w.shape[1]), dtype
        h = C.c_void_p()
        flags = (_lib.FC_RELU if relu else 0) | (_lib.FC_BF16 if dtype == 'bf16' else 0)
        _lib.check(ctx.lib.dodt_fc_create_ex(ctx.handle, self.K, self.N,
                                             w.ctypes.data_as(C.c_void_p),
                                             b.ctypes.data_as(C.c_void_p), flags, C.byref(h)),
                   'dodt_fc_create_ex')
        self.handle = h

    def forward(self, d_x, M, d_y, ldx=None, ldy=None, d_x2=None, d_m=None, ctx=None):
        c = ctx or self.ctx
        _lib.check(c.lib.dodt_fc_forward(
            self.handle, c.handle, _p(d_x), _p(d_x2), int(self.K if ldx is None else ldx),
            int(M), _p(d_m), _p(d_y), int(self.N if ldy is None else ldy)), 'dodt_fc_forward')

    def can_split(self, ldx=None):
        """Whether forward_split takes this layer (dodt_fc_forward_split's conditions)."""
        return self.N <= 32 and self.K % 16 == 0 and (self.K if ldx is None else ldx) % 4 == 0

    def forward_split(self, d_x, M, d_ys, widths, ldx=None, d_m=None, ctx=None):
        """One launch, columns [0, widths[0]) to d_ys[0] (M, widths[0]), the next widths[1] to d_ys[1], ..."""
        c = ctx or self.ctx
        w = (C.c_int * len(widths))(*[int(v) for v in widths])
        ys = (C.c_void_p * len(d_ys))(*[_p(y) for y in d_ys])
        _lib.check(c.lib.dodt_fc_forward_split(
            self.handle, c.handle, _p(d_x), int(self.K if ldx is None else ldx), int(M), _p(d_m),
            len(widths), w, ys), 'dodt_fc_forward_split')

    def bf16_row_elems(self):
        """bf16 elements an input row of forward_bf16 must hold (zeros beyond K); 0: the layer has no such path."""
        return int(self.ctx.lib.dodt_fc_bf16_row_elems(self.handle)) if self.dtype == 'bf16' else 0

    def forward_bf16(self, d_x, M, d_y, ldx, ldy=None, d_m=None, y_bf16=True, ctx=None):
        """The layer on rows that are already bf16 (d_x: uint16 storage, ldx elements per row); d_y bf16 rows
        (y_bf16) or float32."""
        c = ctx or self.ctx
        _lib.check(c.lib.dodt_fc_forward_bf16(self.handle, c.handle, _p(d_x), int(ldx), int(M), _p(d_m), _p(d_y),
                                              int(self.N if ldy is None else ldy), 1 if y_bf16 else 0),
                   'dodt_fc_forward_bf16')

    def forward_split_bf16(self, d_x, M, d_ys, widths, ldx, d_m=None, ctx=None):
        c = ctx or self.ctx
        w = (C.c_int * len(widths))(*[int(v) for v in widths])
        ys = (C.c_void_p * len(d_ys))(*[_p(y) for y in d_ys])
        _lib.check(c.lib.dodt_fc_forward_split_bf16(
            self.handle, c.handle, _p(d_x), int(ldx), int(M), _p(d_m), len(widths), w, ys), 'dodt_fc_forward_split_bf16')

    def form(self, d_x, M, d_y=None, ldx=None, ldy=None, d_x2=None, x_bf16=False, y_bf16=False):
        """The record of fc_plan_host for this layer and a call's real device pointers (d_y None: the split entries);
        launches nothing (dodt_fc_form)."""
        p = _lib.FcPlan()
        _lib.check(self.ctx.lib.dodt_fc_form(
            self.handle, _p(d_x), _p(d_x2), int(self.K if ldx is None else ldx), int(M), _p(d_y),
            int(self.N if ldy is None else ldy), 1 if x_bf16 else 0, 1 if y_bf16 else 0, C.byref(p)), 'dodt_fc_form')
        return _fc_plan_record(p)

    def flops(self, M):
        return 2.0 * M * self.K * self.N

    def close(self):
        if self.handle is not None:
            self.ctx.lib.dodt_fc_destroy(self.handle)
            self.handle = None


def three_d_iou_matrix(ctx, d_a, na, d_b, nb, d_iou_out):
    """d_iou_out (na,nb) float64 = 3-D IoU of boxes d_a (na,7) and d_b (nb,7), [x,y,z,l,w,h,ry] float64
    (dt_evaluator_utils.three_d_iou_matrix on the device)."""
    _lib.check(ctx.lib.dodt_three_d_iou_matrix(ctx.handle, _p(d_a), int(na), _p(d_b), int(nb), _p(d_iou_out)),
               'dodt_three_d_iou_matrix')


def temporal_calib(r0_rect, tr_velo_to_cam):
    """The 42 doubles dodt_interpolate_pairs takes for recovery: inv(R0_rect), inv(Tr_velo_to_cam) (3x4, as
    kitti_tracking_utils._rect_to_velo builds it), Tr_velo_to_cam, R0_rect."""
    r0 = np.asarray(r0_rect, np.float64).reshape(3, 3)
    tr = np.asarray(tr_velo_to_cam, np.float64).reshape(3, 4)
    inv = np.zeros_like(tr)
    inv[0:3, 0:3] = np.transpose(tr[0:3, 0:3])
    inv[0:3, 3] = np.dot(-np.transpose(tr[0:3, 0:3]), tr[0:3, 3])
    return np.concatenate([np.linalg.inv(r0).reshape(-1), inv.reshape(-1), tr.reshape(-1), r0.reshape(-1)])


def temporal_ego(ego, n_frames):
    """(n_frames, 13) float64 recovery parameters of one pair: ego = one (trans (3,), matrix (3,3), delta) per frame
    1..n_frames-1 (kitti_tracking_utils.coordinate_transform); row 0 unused.  The inverse of matrix is taken here."""
    if len(ego) != n_frames - 1:
        raise ValueError('recovery needs one (trans, matrix, delta) per frame 1..n_frames-1')
    out = np.zeros((n_frames, 13))
    for i, (trans, matrix, delta) in enumerate(ego):
        out[i + 1, 0:3] = np.asarray(trans, np.float64).reshape(3)
        out[i + 1, 3:12] = np.linalg.inv(np.asarray(matrix, np.float64).reshape(3, 3)).reshape(-1)
        out[i + 1, 12] = float(delta)
    return out


def interpolate_pairs(ctx, d_records, d_counts, n_pairs, max_det, n_frames, threshold, on_conflict, d_out,
                      d_out_counts, d_status, d_recover=None, calib=None, max_out=None, d_calibs=None):
    """Temporal module M for n_pairs keyframe pairs in one launch (dodt_interpolate_pairs): d_records
    (n_pairs, 2, max_det, 17) float32 or float64, d_counts (n_pairs, 2) int32 -> d_out (n_pairs, n_frames, max_out,
    13) float64, d_out_counts (n_pairs, n_frames) int32, d_status (n_pairs,) int32 (1: a 'raise'-mode conflict).
    d_recover (n_pairs, n_frames, 13) float64 (temporal_ego) with calib (temporal_calib), or None.
    d_calibs instead of calib: (n_pairs, 42) float64 on the device, pair p recovers with row p
    (dodt_interpolate_pairs_calibs)."""
    if on_conflict not in ('raise', 'next_best'):
        raise ValueError("on_conflict must be 'raise' or 'next_best'")
    if d_records.dtype not in (np.float32, np.float64):
        raise ValueError('records must be float32 or float64')
    if d_calibs is not None:
        if calib is not None or d_recover is None:
            raise ValueError('d_calibs: instead of calib, with d_recover')
        if tuple(d_calibs.shape) != (int(n_pairs), 42) or d_calibs.dtype != np.float64:
            raise ValueError('d_calibs must be (n_pairs, 42) float64')
        _lib.check(ctx.lib.dodt_interpolate_pairs_calibs(
            ctx.handle, _p(d_records), int(d_records.dtype == np.float64), _p(d_counts), int(n_pairs), int(max_det),
            int(n_frames), float(threshold),
            _lib.CONFLICT_NEXT_BEST if on_conflict == 'next_best' else _lib.CONFLICT_RAISE, _p(d_recover), _p(d_calibs),
            int(2 * max_det if max_out is None else max_out), _p(d_out), _p(d_out_counts), _p(d_status)),
            'dodt_interpolate_pairs_calibs')
        return
    cal = None if calib is None else _arr(C.c_double, calib)
    _lib.check(ctx.lib.dodt_interpolate_pairs(
        ctx.handle, _p(d_records), int(d_records.dtype == np.float64), _p(d_counts), int(n_pairs), int(max_det),
        int(n_frames), float(threshold), _lib.CONFLICT_NEXT_BEST if on_conflict == 'next_best' else _lib.CONFLICT_RAISE,
        _p(d_recover), cal, int(2 * max_det if max_out is None else max_out), _p(d_out), _p(d_out_counts),
        _p(d_status)), 'dodt_interpolate_pairs')


def track_state_bytes(log_capacity):
    """Bytes of a tracker state buffer (dodt_track_state_bytes)."""
    n = C.c_size_t()
    _lib.check(_lib.load().dodt_track_state_bytes(int(log_capacity), C.byref(n)), 'dodt_track_state_bytes')
    return int(n.value)


def track_reset(ctx, d_state, log_capacity):
    _lib.check(ctx.lib.dodt_track_reset(ctx.handle, _p(d_state), int(log_capacity)), 'dodt_track_reset')


def track_flush(ctx, d_state, high_threshold, t_min):
    _lib.check(ctx.lib.dodt_track_flush(ctx.handle, _p(d_state), float(high_threshold), int(t_min)), 'dodt_track_flush')


def track_encode(ctx, d_records, d_counts, n_pairs, max_det, p2, image_wh, threshold, d_track, d_ious, d_enc_counts):
    """kitti_label_table of n_pairs record pairs (dodt_track_encode): d_records (n_pairs, 2, max_det, 17) float32 or
    float64, d_counts (n_pairs, 2) -> d_track (n_pairs, 128, 23), d_ious (n_pairs, 128, 16) float32, d_enc_counts
    (n_pairs, 4) int32."""
    if d_records.dtype not in (np.float32, np.float64):
        raise ValueError('records must be float32 or float64')
    _lib.check(ctx.lib.dodt_track_encode(
        ctx.handle, _p(d_records), int(d_records.dtype == np.float64), _p(d_counts), int(n_pairs), int(max_det),
        _arr(C.c_double, np.asarray(p2, np.float64).reshape(12)), float(image_wh[0]), float(image_wh[1]),
        float(threshold), _p(d_track), _p(d_ious), _p(d_enc_counts)), 'dodt_track_encode')


def track_pairs(ctx, d_state, d_records, d_counts, n_pairs, max_det, p2, image_wh, score_threshold, high_threshold,
                iou_threshold, t_min):
    """Encode and track n_pairs record pairs of one sequence, continuing d_state (dodt_track_pairs)."""
    if d_records.dtype not in (np.float32, np.float64):
        raise ValueError('records must be float32 or float64')
    _lib.check(ctx.lib.dodt_track_pairs(
        ctx.handle, _p(d_state), _p(d_records), int(d_records.dtype == np.float64), _p(d_counts), int(n_pairs),
        int(max_det), _arr(C.c_double, np.asarray(p2, np.float64).reshape(12)), float(image_wh[0]),
        float(image_wh[1]), float(score_threshold), float(high_threshold), float(iou_threshold), int(t_min)),
        'dodt_track_pairs')


def track_lanes_stride(log_capacity):
    """Bytes between two lanes' states in one buffer (dodt_track_lanes_stride)."""
    n = C.c_size_t()
    _lib.check(_lib.load().dodt_track_lanes_stride(int(log_capacity), C.byref(n)), 'dodt_track_lanes_stride')
    return int(n.value)


def track_lanes(ctx, d_states, stride, n_lanes, d_records, d_counts, max_det, p2s, image_whs, score_threshold,
                high_threshold, iou_threshold, t_min, active=None):
    """One pair per lane, lane i on the state at d_states + i * stride with its own p2s[i] (3, 4) and image_whs[i]
    (w, h) (dodt_track_lanes): d_records (n_lanes, 2, max_det, 17), d_counts (n_lanes, 2); active: None, or one
    truth value per lane (a lane that is not active keeps its state untouched)."""
    if d_records.dtype not in (np.float32, np.float64):
        raise ValueError('records must be float32 or float64')
    n_lanes = int(n_lanes)
    p2s, whs = np.asarray(p2s, np.float64).reshape(-1), np.asarray(image_whs, np.float64).reshape(-1)
    if len(p2s) != 12 * n_lanes or len(whs) != 2 * n_lanes:
        raise ValueError('track_lanes: one p2 (3, 4) and one image_wh per lane')
    act = None
    if active is not None:
        if len(active) != n_lanes:
            raise ValueError('track_lanes: active has %d entries for %d lanes' % (len(active), n_lanes))
        act = (C.c_ubyte * n_lanes)(*[1 if a else 0 for a in active])
    _lib.check(ctx.lib.dodt_track_lanes(
        ctx.handle, _p(d_states), int(stride), n_lanes, act, _p(d_records), int(d_records.dtype == np.float64),
        _p(d_counts), int(max_det), _arr(C.c_double, p2s), _arr(C.c_double, whs), float(score_threshold),
        float(high_threshold), float(iou_threshold), int(t_min)), 'dodt_track_lanes')


def track_encoded(ctx, d_state, d_track, d_ious, d_counts, n_pairs, max_rows, high_threshold, iou_threshold, t_min):
    """Track n_pairs already encoded pairs (dodt_track_encoded): d_track (n_pairs, max_rows, 23), d_ious (n_pairs,
    max_rows, 16) float32, d_counts (n_pairs, 2) int32."""
    _lib.check(ctx.lib.dodt_track_encoded(
        ctx.handle, _p(d_state), _p(d_track), _p(d_ious), _p(d_counts), int(n_pairs), int(max_rows),
        float(high_threshold), float(iou_threshold), int(t_min)), 'dodt_track_encoded')


# ---- the Kalman-filter tracker (dodt_kf_*, dodt_amd/csrc/kalman.hip) ---------------------------------------------------
def kf_ego_rows(ego):
    """One (trans (3,), matrix (3,3), delta) per keyframe, or None for a parked ego -> (n, 13) float64: the rows
    dodt_kf_* take (the forward transform, no inverse is taken)."""
    out = np.zeros((len(ego), 13))
    for i, e in enumerate(ego):
        if e is None:
            out[i, 3:12] = np.eye(3).reshape(-1)
            continue
        trans, matrix, delta = e
        out[i, 0:3] = np.asarray(trans, np.float64).reshape(3)
        out[i, 3:12] = np.asarray(matrix, np.float64).reshape(9)
        out[i, 12] = float(delta)
    return out


def _kf_tail(p):
    return (float(p['sigma_l']), float(p['iou_threshold']), int(p['max_age']), int(p['min_hits']), float(p['L']),
            float(p['R_scaler']))


def kf_state_bytes(log_capacity):
    """Bytes of a Kalman tracker state buffer (dodt_kf_state_bytes)."""
    n = C.c_size_t()
    _lib.check(_lib.load().dodt_kf_state_bytes(int(log_capacity), C.byref(n)), 'dodt_kf_state_bytes')
    return int(n.value)


def kf_reset(ctx, d_state, log_capacity):
    _lib.check(ctx.lib.dodt_kf_reset(ctx.handle, _p(d_state), int(log_capacity)), 'dodt_kf_reset')


def kf_track_keyframes(ctx, d_state, d_rows, d_counts, n_keyframes, max_rows, ego_rows, calib42, params):
    """n_keyframes encoded lists (dodt_kf_track_keyframes): d_rows (n, max_rows, 16) float64, d_counts (n,) int32,
    ego_rows (n, 13) (kf_ego_rows), calib42 (temporal_calib), params: sigma_l, iou_threshold, max_age, min_hits, L,
    R_scaler."""
    if d_rows.dtype != np.float64:
        raise ValueError('keyframe rows must be float64')
    ego_rows = np.asarray(ego_rows, np.float64).reshape(-1)
    if len(ego_rows) != 13 * int(n_keyframes):
        raise ValueError('kf_track_keyframes: one ego row (13) per keyframe')
    _lib.check(ctx.lib.dodt_kf_track_keyframes(
        ctx.handle, _p(d_state), _p(d_rows), _p(d_counts), int(n_keyframes), int(max_rows),
        _arr(C.c_double, ego_rows), _arr(C.c_double, calib42), *_kf_tail(params)), 'dodt_kf_track_keyframes')


def kf_track_pairs(ctx, d_state, d_records, d_counts, n_pairs, max_det, p2, image_wh, score_threshold, ego_rows,
                   calib42, params):
    """Encode n_pairs record pairs and track their keyframe-0 lists (dodt_kf_track_pairs); ego_rows[j]: the motion
    into pair j's keyframe 0."""
    if d_records.dtype not in (np.float32, np.float64):
        raise ValueError('records must be float32 or float64')
    ego_rows = np.asarray(ego_rows, np.float64).reshape(-1)
    if len(ego_rows) != 13 * int(n_pairs):
        raise ValueError('kf_track_pairs: one ego row (13) per pair')
    _lib.check(ctx.lib.dodt_kf_track_pairs(
        ctx.handle, _p(d_state), _p(d_records), int(d_records.dtype == np.float64), _p(d_counts), int(n_pairs),
        int(max_det), _arr(C.c_double, np.asarray(p2, np.float64).reshape(12)), float(image_wh[0]),
        float(image_wh[1]), float(score_threshold), _arr(C.c_double, ego_rows), _arr(C.c_double, calib42),
        *_kf_tail(params)), 'dodt_kf_track_pairs')


KIND_LANES_CHUNK = 8            # lanes per launch triple of dodt_kf_track_lanes / dodt_vt_track_lanes (kLaneChunk)


def _lanes_stride(name, log_capacity):
    n = C.c_size_t()
    _lib.check(getattr(_lib.load(), name)(int(log_capacity), C.byref(n)), name)
    return int(n.value)


def _kind_lanes(name, ctx, d_states, stride, n_lanes, d_records, d_counts, max_det, p2s, image_whs, ego_rows, calibs,
                score_threshold, tail, active):
    """The common arguments of dodt_kf_track_lanes / dodt_vt_track_lanes, checked."""
    if d_records.dtype not in (np.float32, np.float64):
        raise ValueError('records must be float32 or float64')
    n_lanes = int(n_lanes)
    per_lane = (('p2s', p2s, 12), ('image_whs', image_whs, 2), ('egos', ego_rows, 13), ('calibs', calibs, 42))
    flat = []
    for what, a, width in per_lane:
        a = np.asarray(a, np.float64).reshape(-1)
        if len(a) != width * n_lanes:
            raise ValueError('%s: %s needs %d doubles per lane, %d lanes' % (name, what, width, n_lanes))
        flat.append(_arr(C.c_double, a))
    act = None
    if active is not None:
        if len(active) != n_lanes:
            raise ValueError('%s: active has %d entries for %d lanes' % (name, len(active), n_lanes))
        act = (C.c_ubyte * n_lanes)(*[1 if a else 0 for a in active])
    _lib.check(getattr(ctx.lib, name)(
        ctx.handle, _p(d_states), int(stride), n_lanes, act, _p(d_records), int(d_records.dtype == np.float64),
        _p(d_counts), int(max_det), flat[0], flat[1], flat[2], flat[3], float(score_threshold), *tail), name)


def kf_lanes_stride(log_capacity):
    """Bytes between two lanes' Kalman states in one buffer (dodt_kf_lanes_stride)."""
    return _lanes_stride('dodt_kf_lanes_stride', log_capacity)


def kf_track_lanes(ctx, d_states, stride, n_lanes, d_records, d_counts, max_det, p2s, image_whs, ego_rows, calibs,
                   score_threshold, params, active=None):
    """One pair per lane, lane i on the Kalman state at d_states + i * stride (dodt_kf_track_lanes): d_records (n_lanes,
    2, max_det, 17), d_counts (n_lanes, 2); per lane p2s[i] (3, 4), image_whs[i] (w, h), ego_rows[i] (13: the motion into
    the lane's current keyframe, kf_ego_rows) and calibs[i] (42, temporal_calib); active: None, or one truth value per
    lane (a lane that is not active keeps its state untouched)."""
    _kind_lanes('dodt_kf_track_lanes', ctx, d_states, stride, n_lanes, d_records, d_counts, max_det, p2s, image_whs,
                ego_rows, calibs, score_threshold, _kf_tail(params), active)


def kf_flush(ctx, d_state, ego_row, calib42, params):
    """The kept keyframe-1 rows as the final keyframe (ego_row: 13 doubles or None), then finish (dodt_kf_flush)."""
    ego = None if ego_row is None else _arr(C.c_double, np.asarray(ego_row, np.float64).reshape(13))
    _lib.check(ctx.lib.dodt_kf_flush(ctx.handle, _p(d_state), ego, _arr(C.c_double, calib42), *_kf_tail(params)),
               'dodt_kf_flush')


def kf_filter_steps(ctx, d_x0, d_ops, d_z, d_n_ops, d_LR, n_tracks, max_ops, d_x_out, d_P_out):
    """The track filter alone (dodt_kf_filter_steps): x (n, max_ops, 8) and P (n, max_ops, 8, 8) after every
    operation."""
    _lib.check(ctx.lib.dodt_kf_filter_steps(ctx.handle, _p(d_x0), _p(d_ops), _p(d_z), _p(d_n_ops), _p(d_LR),
                                            int(n_tracks), int(max_ops), _p(d_x_out), _p(d_P_out)),
               'dodt_kf_filter_steps')


def kf_assign(ctx, d_iou, n_tracks, n_dets, iou_threshold, d_matches, d_unmatched_dets, d_unmatched_tracks,
              d_counts):
    """Optimal assignment + gate of a float32 (n_tracks, n_dets) IoU matrix (dodt_kf_assign)."""
    _lib.check(ctx.lib.dodt_kf_assign(ctx.handle, _p(d_iou), int(n_tracks), int(n_dets), float(iou_threshold),
                                      _p(d_matches), _p(d_unmatched_dets), _p(d_unmatched_tracks), _p(d_counts)),
               'dodt_kf_assign')


def kf_iou_matrix(ctx, d_last, n_tracks, d_dets, n_dets, ego_row, calib42, d_iou_out):
    """cal_transformed_ious of boxes [h,w,l,x,y,z,ry] float64 as float32 (dodt_kf_iou_matrix)."""
    ego = None if ego_row is None else _arr(C.c_double, np.asarray(ego_row, np.float64).reshape(13))
    _lib.check(ctx.lib.dodt_kf_iou_matrix(ctx.handle, _p(d_last), int(n_tracks), _p(d_dets), int(n_dets), ego,
                                          _arr(C.c_double, calib42), _p(d_iou_out)), 'dodt_kf_iou_matrix')


# ---- the velocity-extrapolating IoU tracker (dodt_vt_*, dodt_amd/csrc/velocity_track.hip) ------------------------------
def _vt_tail(p):
    return (float(p['sigma_l']), float(p['sigma_h']), float(p['sigma_iou']), int(p['t_min']), int(p['extend_len']),
            int(p['stride']))


def vt_state_bytes(log_capacity):
    """Bytes of a velocity tracker state buffer (dodt_vt_state_bytes)."""
    n = C.c_size_t()
    _lib.check(_lib.load().dodt_vt_state_bytes(int(log_capacity), C.byref(n)), 'dodt_vt_state_bytes')
    return int(n.value)


def vt_reset(ctx, d_state, log_capacity):
    _lib.check(ctx.lib.dodt_vt_reset(ctx.handle, _p(d_state), int(log_capacity)), 'dodt_vt_reset')


def vt_track_keyframes(ctx, d_state, d_rows, d_counts, n_keyframes, max_rows, ego_rows, calib42, params, box_f64=None,
                       score_f64=None):
    """n_keyframes encoded lists (dodt_vt_track_keyframes): d_rows (n, max_rows, 16) float32 or float64, d_counts (n,)
    int32, ego_rows (n, 13) (kf_ego_rows), calib42 (temporal_calib), params: sigma_l, sigma_h, sigma_iou, t_min,
    extend_len, stride.  box_f64 / score_f64: the dtype the host holds boxes3d / the scores in -- the speed and the
    predictions are computed, the scores compared in it (None: the rows' dtype; True only with float64 rows)."""
    if d_rows.dtype not in (np.float32, np.float64):
        raise ValueError('keyframe rows must be float32 or float64')
    f64 = d_rows.dtype == np.float64
    box_f64, score_f64 = (f64 if v is None else bool(v) for v in (box_f64, score_f64))
    if (box_f64 or score_f64) and not f64:
        raise ValueError('vt_track_keyframes: float64 boxes or scores need float64 rows')
    ego_rows = np.asarray(ego_rows, np.float64).reshape(-1)
    if len(ego_rows) != 13 * int(n_keyframes):
        raise ValueError('vt_track_keyframes: one ego row (13) per keyframe')
    _lib.check(ctx.lib.dodt_vt_track_keyframes(
        ctx.handle, _p(d_state), _p(d_rows), int(d_rows.dtype == np.float64), _p(d_counts), int(n_keyframes),
        int(max_rows), _arr(C.c_double, ego_rows), _arr(C.c_double, calib42), *_vt_tail(params), int(box_f64),
        int(score_f64)), 'dodt_vt_track_keyframes')


def vt_track_pairs(ctx, d_state, d_records, d_counts, n_pairs, max_det, p2, image_wh, score_threshold, ego_rows,
                   calib42, params):
    """Encode n_pairs record pairs and track their keyframe-0 lists (dodt_vt_track_pairs); ego_rows[j]: the motion
    into pair j's keyframe 0."""
    if d_records.dtype not in (np.float32, np.float64):
        raise ValueError('records must be float32 or float64')
    ego_rows = np.asarray(ego_rows, np.float64).reshape(-1)
    if len(ego_rows) != 13 * int(n_pairs):
        raise ValueError('vt_track_pairs: one ego row (13) per pair')
    _lib.check(ctx.lib.dodt_vt_track_pairs(
        ctx.handle, _p(d_state), _p(d_records), int(d_records.dtype == np.float64), _p(d_counts), int(n_pairs),
        int(max_det), _arr(C.c_double, np.asarray(p2, np.float64).reshape(12)), float(image_wh[0]),
        float(image_wh[1]), float(score_threshold), _arr(C.c_double, ego_rows), _arr(C.c_double, calib42),
        *_vt_tail(params)), 'dodt_vt_track_pairs')


def vt_lanes_stride(log_capacity):
    """Bytes between two lanes' velocity tracker states in one buffer (dodt_vt_lanes_stride)."""
    return _lanes_stride('dodt_vt_lanes_stride', log_capacity)


def vt_track_lanes(ctx, d_states, stride, n_lanes, d_records, d_counts, max_det, p2s, image_whs, ego_rows, calibs,
                   score_threshold, params, active=None):
    """kf_track_lanes for the velocity tracker's states and parameters (dodt_vt_track_lanes)."""
    _kind_lanes('dodt_vt_track_lanes', ctx, d_states, stride, n_lanes, d_records, d_counts, max_det, p2s, image_whs,
                ego_rows, calibs, score_threshold, _vt_tail(params), active)


def vt_flush(ctx, d_state, ego_row, calib42, params):
    """The kept keyframe-1 rows as the final keyframe (ego_row: 13 doubles or None), then finish (dodt_vt_flush)."""
    ego = None if ego_row is None else _arr(C.c_double, np.asarray(ego_row, np.float64).reshape(13))
    _lib.check(ctx.lib.dodt_vt_flush(ctx.handle, _p(d_state), ego, _arr(C.c_double, calib42), *_vt_tail(params)),
               'dodt_vt_flush')


def vt_iou_matrix(ctx, d_last, n_tracks, d_dets, n_dets, ego_row, calib42, d_iou_out):
    """video_detection_iou.cal_transformed_ious of boxes [h,w,l,x,y,z,ry] float64 as float64 (dodt_vt_iou_matrix)."""
    ego = None if ego_row is None else _arr(C.c_double, np.asarray(ego_row, np.float64).reshape(13))
    _lib.check(ctx.lib.dodt_vt_iou_matrix(ctx.handle, _p(d_last), int(n_tracks), _p(d_dets), int(n_dets), ego,
                                          _arr(C.c_double, calib42), _p(d_iou_out)), 'dodt_vt_iou_matrix')
