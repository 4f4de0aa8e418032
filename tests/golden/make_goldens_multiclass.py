#!/usr/bin/env python3
"""Golden vectors for configurations with several classes (classes: ['Pedestrian', 'Cyclist'],
avod/configs/pyramid_people_example.config), from the reference's own code run in the build
container:

(a) records   DtEvaluator.get_avod_predicted_boxes_3d_and_scores (avod/core/dt_evaluator.py:
              1134-1259) on seeded network outputs whose softmax has 3 and 4 columns -- the
              score is the largest non-background value and the type its np.argmax (:1226-1255);
(b) anchors   the grid generator run once per class and concatenated class-major
              (avod/core/models/dt_rpn_model.py:894-909) for two single-cluster classes;
(c) filter    get_empty_anchor_filter_2d's keep mask for that grid on the cloud of
              object/training/velodyne/000001.bin (the cloud frames.npz stores as obj000001).

Run:  python tests/golden/make_goldens_multiclass.py    (needs /root/reference; writes multiclass.npz)

The reference is imported as in make_goldens_box4ca.py: TensorFlow as inert stand-ins, the
evaluator's method called unbound.  Only data is stored.

The logits of (a) are drawn so that no comparison of two softmax values can come out
differently with another float32 exp: in every row the two largest non-background logits are
either EXACTLY equal (a tie, which np.argmax resolves to the lower index; equal logits give
equal exponentials and equal quotients whatever exp is used) or at least 1e-3 apart (a relative
difference of 1e-3 between the two softmax values, four orders above an exp's rounding).  Rows
that come out closer are redrawn; main() asserts the property and prints the redraw count.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402
import make_goldens_box4ca as mb  # noqa: E402

F32 = np.float32
MIN_GAP = 1e-3
# stand-ins for the clusters the reference takes from the training labels (l, w, h), one per class
PEOPLE_SIZES = [[[0.844, 0.661, 1.763]], [[1.763, 0.597, 1.737]]]
PEOPLE_STRIDES = [mg.ANCHOR_STRIDE, mg.ANCHOR_STRIDE]         # anchor_strides: [0.5, 0.5, 0.5, 0.5]


def softmax_f32(logits):
    """tf.nn.softmax in float32: max-subtracted exponentials over their sum."""
    x = np.asarray(logits, F32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(F32)


def top_two_gap(fg):
    s = np.sort(fg.astype(np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def class_logits(rng, n, n_cls, tie_every=5):
    """(n, n_cls) float32 logits, decisive or exactly tied (see the module docstring) -> logits, tied rows, redraws."""
    lg = rng.normal(0, 2.0, size=(n, n_cls)).astype(F32)
    redrawn = 0
    while True:
        close = top_two_gap(lg[:, 1:]) < MIN_GAP
        if not close.any():
            break
        redrawn += int(close.sum())
        lg[close] = rng.normal(0, 2.0, size=(int(close.sum()), n_cls)).astype(F32)
    tied = np.zeros(n, bool)
    for r in range(0, n, tie_every):
        # the two largest non-background logits become one value; the remaining ones stay >= MIN_GAP below
        order = np.argsort(lg[r, 1:])[::-1] + 1
        lg[r, order[1]] = lg[r, order[0]]
        tied[r] = True
    return lg, tied, redrawn


def records_cases(DtEvaluator, M, rng, out):
    shapes = [(100, 100), (37, 64), (1, 5)]
    ci = 0
    for n_cls in (3, 4):
        for n0, n1 in shapes:
            b, ori, _, corr = mb.case(rng, n0, n1, special=(n0 == 37))
            lg, sm, tied, redrawn = [], [], [], 0
            for n in (n0, n1):
                l, t, r = class_logits(rng, n, n_cls)
                lg.append(l)
                sm.append(softmax_f32(l))
                tied.append(t)
                redrawn += r
            for f in range(2):
                gap = top_two_gap(lg[f][:, 1:])
                assert np.all((gap == 0) == tied[f]) and np.all(gap[~tied[f]] >= MIN_GAP)
                fg = sm[f][:, 1:]
                top = np.sort(fg, axis=1)
                assert np.all((top[:, -1] == top[:, -2]) == tied[f])     # tied logits are tied softmax values
            pred = {M.PRED_TOP_PREDICTION_BOXES_3D: [x.copy() for x in b],
                    M.PRED_TOP_ORIENTATIONS: [x.copy() for x in ori],
                    M.PRED_TOP_CLASSIFICATION_SOFTMAX: [x.copy() for x in sm],
                    M.PRED_TOP_CORR_OFFSETS: corr.copy()}
            res = DtEvaluator.get_avod_predicted_boxes_3d_and_scores(None, pred, 'box_4ca')
            assert res.shape == (n0 + n1, 17)
            for f in range(2):
                out['c%d_boxes_3d_%d' % (ci, f)] = b[f]
                out['c%d_orientations_%d' % (ci, f)] = ori[f]
                out['c%d_logits_%d' % (ci, f)] = lg[f]
                out['c%d_softmax_%d' % (ci, f)] = sm[f]
            out['c%d_corr_offsets' % ci] = corr
            out['c%d_records' % ci] = res
            print('case %d: n_cls %d, %d + %d rows, %d tied, %d redrawn, types %s'
                  % (ci, n_cls, n0, n1, int(tied[0].sum() + tied[1].sum()), redrawn,
                     np.bincount(res[:, 8].astype(int), minlength=n_cls - 1).tolist()))
            ci += 1
    out['n_cases'] = np.asarray(ci)


def anchor_parts(out):
    from wavedata.tools.core import calib_utils
    from wavedata.tools.core.voxel_grid_2d import VoxelGrid2D
    from wavedata.tools.obj_detection import obj_utils
    from avod.core import anchor_filter, box_3d_encoder
    from avod.core.anchor_generators import grid_anchor_3d_generator

    plane = np.asarray([0, -1, 0, 1.65]) / np.linalg.norm([0, -1, 0])
    gen = grid_anchor_3d_generator.GridAnchor3dGenerator()
    per_class = [gen.generate(area_3d=mg.AREA_EXTENTS, anchor_3d_sizes=np.asarray(PEOPLE_SIZES[c]),
                              anchor_stride=PEOPLE_STRIDES[c], ground_plane=plane)
                 for c in range(len(PEOPLE_SIZES))]
    boxes = np.concatenate(per_class)                            # dt_rpn_model.py:900-909
    out['anchor_sizes'] = np.asarray(PEOPLE_SIZES)
    out['anchor_strides'] = np.asarray(PEOPLE_STRIDES)
    out['anchor_class_counts'] = np.asarray([len(b) for b in per_class])
    for c, b in enumerate(per_class):
        out['anchor_first64_%d' % c] = b[:64]
        out['anchor_last64_%d' % c] = b[-64:]
    out['anchor_sha1'] = np.frombuffer(hashlib.sha1(np.ascontiguousarray(boxes).tobytes()).digest(), np.uint8)

    # (c): the cloud of make_goldens.run_frame for object sample 000001, full size
    d = os.path.join(mg.REF, 'avod/tests/datasets/Kitti/object/training')
    calib = calib_utils.read_calibration(d + '/calib', 1)
    xyzi = np.fromfile(d + '/velodyne/%06d.bin' % 1, dtype=np.float32).reshape(-1, 4)
    im_wh = mg.png_size(d + '/image_2/%06d.png' % 1)
    pts = calib_utils.lidar_to_cam_frame(xyzi[:, :3], calib)
    ptsf = pts[pts[:, 2] > 0]
    uv = calib_utils.project_to_image(ptsf.T, p=calib.p2).T
    imf = (uv[:, 0] > 0) & (uv[:, 0] < im_wh[0]) & (uv[:, 1] > 0) & (uv[:, 1] < im_wh[1])
    cloud = ptsf[imf].T
    sf = np.logical_xor(obj_utils.get_point_filter(cloud, mg.AREA_EXTENTS, plane, 2.0),
                        obj_utils.get_point_filter(cloud, mg.AREA_EXTENTS, plane, 0.2))
    vg = VoxelGrid2D()
    vg.voxelize_2d(cloud.T[sf], mg.VOXEL_SIZE, extents=mg.AREA_EXTENTS, ground_plane=plane,
                   create_leaf_layout=True)
    keep = anchor_filter.get_empty_anchor_filter_2d(box_3d_encoder.box_3d_to_anchor(boxes), vg, 1)
    out['filter_keep_bits'] = np.packbits(keep)
    out['filter_n_kept'] = np.asarray(int(keep.sum()))
    n0 = len(per_class[0])
    print('anchors %s, kept %d (class 0: %d, class 1: %d)'
          % (boxes.shape, int(keep.sum()), int(keep[:n0].sum()), int(keep[n0:].sum())))


def main():
    DtEvaluator, M = mb.import_evaluator()
    out = {}
    records_cases(DtEvaluator, M, np.random.default_rng(20261018), out)
    anchor_parts(out)
    path = os.path.join(mg.HERE, 'multiclass.npz')
    np.savez_compressed(path, **out)
    print('multiclass.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
