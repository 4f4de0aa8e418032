"""Frozen configurations of the hot path.

The reference reads these from protobuf text files; only the two configurations
the path is quoted on are kept, as plain dicts.  Proto `float` fields are
32-bit, and python then does float64 arithmetic on the float32-rounded values,
so they are stored here exactly as python sees them in the reference
(avod/protos/kitti_utils.proto:10,29-34).

  PYRAMID_DODT  avod/configs/pyramid_cars_with_aug_dt_5_tracking.config
  CARS_EXAMPLE  avod/configs/avod_cars_example.config

and the second family of the reference's configurations, two classes in one model
(throughput unmeasured):

  PYRAMID_PEOPLE  avod/configs/pyramid_people_example.config
  AVOD_PEOPLE     avod/configs/avod_people_example.config

Class-aware keys: `classes` names the detected classes in the order of the stage-2 head's
non-background columns; with `anchor_strides` (one [x, z] stride pair per class) `anchor_sizes`
holds one list of clusters per class.  A configuration without `anchor_strides` has one
class, whose clusters are `anchor_sizes` and whose stride is `anchor_stride`
(class_anchor_params()).
"""
import collections

import numpy as np


def _f32(x):
    return float(np.float32(x))


_COMMON = dict(
    area_extents=np.array([[-40., 40.], [-5., 3.], [0., 70.]]),
    bev_extents=np.array([[-40., 40.], [0., 70.]]),
    voxel_size=_f32(0.1),
    anchor_stride=[_f32(0.5), _f32(0.5)],
    height_lo=_f32(-0.2),
    height_hi=_f32(2.3),
    num_slices=5,
    # obj_utils.get_road_plane overwrites the plane file
    ground_plane=np.array([0., -1., 0., 1.65]),
    # slice used for the empty-anchor filter (kitti_utils.py:212-213)
    anchor_filter_lo=0.2,
    anchor_filter_hi=2.0,
    # The reference clusters car sizes from the training labels
    # (label_cluster_utils.py); those labels are not part of this build, so
    # the published AVOD car clusters stand in (l, w, h).
    anchor_sizes=[[3.514, 1.581, 1.511], [4.236, 1.653, 1.547]],
    bev_dims=(700, 800),
    bev_depth=6,
    rpn_roi_crop_size=3,
    avod_roi_crop_size=7,
    rpn_nms_iou_thresh=_f32(0.8),
    avod_nms_size=100,
    avod_nms_iou_thresh=_f32(0.01),
    rpn_train_nms_size=1024,
    rpn_test_nms_size=300,
    # avod_box_representation (both configs, e.g. ...dt_5_tracking.config:29): box_4c offsets
    # plus a regressed angle vector that fixes the heading (dt_evaluator.py:1166-1212)
    box_representation='box_4ca',
    classes=('Car',),
)

# frames_per_sample: 2 = DODT's Siamese model over a (t, t + tau) frame pair with the
# correlation branch (dt_rpn_model.py / dt_avod_model.py); 1 = single-frame AVOD
# (rpn_model.py / avod_model.py).  feat_stride / feat_depth: the extractor's output map
# relative to its input (pyramid: full resolution x 32; plain VGG: H/8*4 x 256).
PYRAMID_DODT = dict(_COMMON,
                    name='pyramid_cars_with_aug_dt_5_tracking',
                    model='dt_avod_model',
                    frames_per_sample=2,
                    extractor='vgg_pyr',
                    img_dims=(360, 1200),
                    img_depth=3)

CARS_EXAMPLE = dict(_COMMON,
                    name='avod_cars_example',
                    model='avod_model',
                    frames_per_sample=1,
                    extractor='vgg',
                    img_dims=(480, 1590),
                    img_depth=3)

# Two classes (avod/configs/pyramid_people_example.config:143-152, avod_people_example.config:142-151): the anchor grid
# is tiled once per class and concatenated, class-major (dt_rpn_model.py:894-909); the stage-2 head has one column per
# class behind the background's.  The reference clusters the sizes from the training labels, which are not part of this
# build; stand-ins (l, w, h), one cluster per class.
_PEOPLE = dict(classes=('Pedestrian', 'Cyclist'),
               anchor_sizes=[[[0.844, 0.661, 1.763]], [[1.763, 0.597, 1.737]]],
               anchor_strides=[[_f32(0.5), _f32(0.5)], [_f32(0.5), _f32(0.5)]],
               rpn_test_nms_size=1024)

PYRAMID_PEOPLE = dict(_COMMON, **dict(_PEOPLE,
                                      name='pyramid_people_example',
                                      model='avod_model',
                                      frames_per_sample=1,
                                      extractor='vgg_pyr',
                                      img_dims=(360, 1200),
                                      img_depth=3))

AVOD_PEOPLE = dict(_COMMON, **dict(_PEOPLE,
                                   name='avod_people_example',
                                   model='avod_model',
                                   frames_per_sample=1,
                                   extractor='vgg',
                                   img_dims=(480, 1590),
                                   img_depth=3))


def class_anchor_params(cfg):
    """(sizes_per_class, strides_per_class) of a configuration: its per-class keys, or the one class that
    `anchor_sizes` / `anchor_stride` describe."""
    if 'anchor_strides' in cfg:
        sizes, strides = list(cfg['anchor_sizes']), list(cfg['anchor_strides'])
        if len(sizes) != len(strides) or len(sizes) != len(cfg.get('classes', sizes)):
            raise ValueError('anchor_sizes, anchor_strides and classes must have one entry per class')
        return sizes, strides
    return [cfg['anchor_sizes']], [cfg['anchor_stride']]


# Calibration of the tracking sequence the reference's tests bundle
# (avod/tests/datasets/Kitti/tracking/training/calib/0000.txt, numbers only) and the KITTI
# image size: the default camera of the synthetic benchmarks and parity tests.
KITTI_P2 = np.array([[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01],
                     [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01],
                     [0.0, 0.0, 1.0, 2.745884e-03]])
KITTI_R0_RECT = np.array([[9.999239e-01, 9.837760e-03, -7.445048e-03],
                          [-9.869795e-03, 9.999421e-01, -4.278459e-03],
                          [7.402527e-03, 4.351614e-03, 9.999631e-01]])
KITTI_TR_VELO_TO_CAM = np.array(
    [[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03],
     [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
     [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]])
KITTI_IMAGE_WH = (1242, 375)


class Calibration(collections.namedtuple('Calibration', 'p2 r0_rect tr_velo_to_cam image_wh')):
    """The geometry of one sample (a frame pair, or a single frame): p2 (3,4), r0_rect (3,3), tr_velo_to_cam (3,4) as
    float64 arrays, image_wh (w, h) ints.  KITTI has one per tracking video and one per object frame; both frames of a
    pair share it.  What the pipeline takes per step (FramePairPipeline.run(..., calib=)); equal by value through
    key()."""
    __slots__ = ()

    def __new__(cls, p2, r0_rect, tr_velo_to_cam, image_wh):
        return super().__new__(cls, np.array(p2, dtype=np.float64).reshape(3, 4),
                               np.array(r0_rect, dtype=np.float64).reshape(3, 3),
                               np.array(tr_velo_to_cam, dtype=np.float64).reshape(3, 4),
                               (int(image_wh[0]), int(image_wh[1])))

    def key(self):
        """Hashable, equal exactly when every number is (arrays do not compare with ==)."""
        return (self.p2.tobytes(), self.r0_rect.tobytes(), self.tr_velo_to_cam.tobytes(), self.image_wh)


KITTI_CALIBRATION = Calibration(KITTI_P2, KITTI_R0_RECT, KITTI_TR_VELO_TO_CAM, KITTI_IMAGE_WH)


def velo_to_cam(r0_rect=KITTI_R0_RECT, tr=KITTI_TR_VELO_TO_CAM):
    """(3,4) = (R0_rect padded . Tr_velo_to_cam padded)[0:3], float64
    (wavedata/.../calib_utils.py:502-519)."""
    r0 = np.zeros((4, 4)); r0[:3, :3] = r0_rect; r0[3, 3] = 1
    t = np.zeros((4, 4)); t[:3, :4] = tr; t[3, 3] = 1
    return np.dot(r0, t)[:3]
