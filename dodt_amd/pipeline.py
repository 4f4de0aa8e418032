"""Frame-pair pipeline: the per-frame hot path of DODT chained on one GPU.

Order of work follows the reference's inference call stack:
create_feed_dict (points -> BEV maps, anchor grid -> empty filter -> projections;
avod/core/models/dt_rpn_model.py:732-1042) then the graph
(dt_rpn_model.py:355-730, dt_avod_model.py:128-711).  The dense heads between
crop and NMS (anchor predictor, stage-2 FC, correlation branch: SURVEY 8(f) items 1-2)
run on the device when the pipeline is built with `head_params`; without them their
outputs are inputs of the pipeline (`heads`, resident in HBM), which is what the
index-exact parity tests use.

Frame pairs are independent (batch size 1 in the reference, no cross-pair state),
so a step may carry several pairs: all their frames go through the conv stacks as
one batch.

Streams (four at one pair per step: the hardware-queue budget of a process -- a fifth shares a queue
with another one and runs behind its launches): `ctx`, the main stream, carries the BEV stack; `img_ctx`
the image stack and, behind it, the 'img' placement's correlation maps, the temporal module and the
tracker; every frame of a pair has a side stream (`sides`) for its "prep" (points -> BEV maps, anchors,
image preprocessing) and its "tail" (crops, heads, decode, NMS, records), so the single-workgroup stages
(NMS scan) of different frames overlap.  The order on a side stream is prep k, tail k-1, prep k+1, ...:
run(k) enqueues the prep of step k behind the tail of step k-2 and in front of the convs of its own step
(0.1 ms), then the tail of step k-1, which waits for that step's convs (CONV_DONE_MARK) and so runs under
the convs of step k.  With look-ahead run(k) also enqueues the prep of step k+1, in front of the tail of
step k-1.  Inputs, feature maps, per-frame buffers and detection records are double-buffered by step
parity for that (what a prep leaves for its tail three deep), and `finish()` drains the last step.
Where the T branch of a computed pair runs -- its placement -- is one value, resolved with the
environment's switches by resolve_schedule() when the pipeline is built.
Everything stays on the device; the only host round trip per step is the kept-anchor count
of each frame, fetched one step after it was produced (the host runs one step ahead of the
GPU and otherwise waits in that read).
Sequence mode (FramePairPipeline(sequence=True), push_frame()): the steps are the overlapping keyframe pairs of one
sequence, a step takes ONE new frame, and what does not depend on a keyframe's role in a pair -- its image stack, image
preprocessing, anchor filter and projections -- is computed once and read by both steps it belongs to (sequence_slots(),
DESIGN section 8d).
Both modes enqueue a step through one body, _step(), behind the checks of run() / push_frame().  A mode is three things:
its prep (_prep, _seq_prep: both run the one per-frame chain, _prep_frame), where the image stack writes (_image_forward),
and which buffers frame f of step k uses -- its prep set, the slot of its count's fetch, its feature views
(_frame_buffers, asked by the preps and by _tail alike).  A step's record (_Step) is made by the call that enqueues it,
waits in `pending`, and is completed by its tail.
The geometry -- calibration and image size -- belongs to the step, not to the pipeline: the constructor's is the default,
every step call takes `calib=` per sample, and what a step was given travels with it (_Geometry: beside its prep sets and
in its record) to its tail, the temporal module and the tracker, which are enqueued a call later.
"""
import os
from collections import namedtuple

import numpy as np

from dodt_amd import config as _config
from dodt_amd import _lib, device, ops, tracking
from dodt_amd.core.anchor_generators import grid_anchor_3d_generator as gen
from dodt_amd.core.avod_fc_layers.fusion_fc_layers import EarlyFusionFcLayers
from dodt_amd.core.feature_extractors.vgg import BevVgg, ImgVgg
from dodt_amd.core.feature_extractors.vgg_pyramid import BevVggPyr, ImgVggPyr
from dodt_amd.core.models.anchor_predictor import AnchorPredictor
from dodt_amd.temporal import unpack_frames

# feature_extractor_builder.get_extractor (avod/builders/feature_extractor_builder.py:8-24)
EXTRACTORS = {'vgg_pyr': (BevVggPyr, ImgVggPyr), 'vgg': (BevVgg, ImgVgg)}

MAX_DET = 100            # avod_nms_size
REC_COLS = 17            # dt_evaluator.py:1217-1257
ROI = 7                  # avod_proposal_roi_crop_size
CORR_MAX_DISP, CORR_STRIDE2, CORR_PAD = 5, 2, 5     # correlation_config; correlation.py:7
CORR_CH = (2 * (CORR_MAX_DISP // CORR_STRIDE2) + 1) ** 2

# Mark slots (Context.mark / wait_mark; slots below 64 are the timing marks of _mark):    recorded by -> waited for by
PREP_DONE_MARK = 244    # .. 246, by step % 3: every side stream at the end of a step's prep (_prep; _seq_prep and
                        # _seq_prep_new) -> the main and the image stream in front of that step's conv stacks (_step);
                        # sequence mode: frame 1's stream also -> frame 0's in front of the next step's plain
                        # voxelisation (_seq_prep), and -> the image stream in front of a priming forward (_push)
TAIL_DONE_MARK = 247    # every side stream at the end of a step's tail (_pending_tail) -> the main stream (the step's
                        # records are complete there; the next BEV stack of that parity overwrites maps the tail reads) and
                        # the image stream (the same for the image net's maps; the temporal module and the tracker read the
                        # records)
CORR_MAP_MARK = 248     # 249, by parity: the image stream behind a step's correlation maps (_step, placement 'img')
                        # -> frame 1's side stream in front of the T branch's crops (_pair_img)
CONV_DONE_MARK = 250    # 251, by parity: the main and the image stream behind a step's stacks (_step; the image stream
                        # also behind a priming forward, _push) -> the side streams (_wait_convs) in front of that step's
                        # tail (_tail) and of the look-ahead prep of the step after next (_prep, _seq_prep); the main
                        # stream's also -> the image stream in front of the correlation maps (_step); a priming forward's
                        # -> frame 1's stream in front of the next prep of that parity (_seq_prep_new)
PROPOSALS_MARK = 252    # frame 0's side stream where its proposals stand -> frame 1's in front of the T branch's crops
CORR_ROIS_MARK = 253    # frame 1's side stream behind its share of the T branch -> frame 0's in front of what reads it


# Sequence mode (FramePairPipeline(sequence=True)): what a keyframe leaves for the two steps it
# belongs to lives in rings of single-frame slots, keyframe j (frame f of step k: j = k + f) in slot j % depth
IMG_RING = 3       # the image net's maps: forward j + 3 is the first writer enqueued behind the last tail that reads j
PREP_RING = 4      # occ / keep / count / projections / anchors: one more than pair mode's three, see sequence_slots()
POINT_RING = 3     # the pipeline's copy of a keyframe's points, read by its plain voxelisation one step later

SeqSlots = namedtuple('SeqSlots', 'img prep points')


def sequence_slots(step, img_ring=IMG_RING, prep_ring=PREP_RING, point_ring=POINT_RING):
    """The ring slots of sequence step `step`, whose frames are keyframes step and step + 1: per ring a pair
    (slot frame 0 reads, slot frame 1 reads).  The second of each is also what the step's NEW frame writes: its image
    forward, its prep and the copy of its points.  Pure arithmetic; the depths are arguments only so that
    tests/test_sequence_slots.py can show what a shallower ring collides with:
    - image ring: the tail of step k is enqueued in the call for step k + 1, behind that call's image forward, which
      writes keyframe k + 2 -- with two slots the slot of keyframe k, frame 0 of that tail;
    - prep ring: a look-ahead prep is enqueued one call early, in front of the tail of that call.  The one in the call
      for step k + 2 writes keyframe k + 4; the tail behind it, of step k + 1, reads keyframes k + 1 and k + 2, and with
      four slots the last reader of the written one -- the tail of step k, frame 0 -- was enqueued a call before."""
    return SeqSlots(img=(step % img_ring, (step + 1) % img_ring),
                    prep=(step % prep_ring, (step + 1) % prep_ring),
                    points=(step % point_ring, (step + 1) % point_ring))


class Schedule(namedtuple('Schedule', 'fused_tail no_tail no_corr no_rpn t_branch two_streams corr_map_img')):
    """What resolve_schedule() found: the tail's elementwise runs as one launch each (fused_tail), tools/' switches that
    leave work out (no_tail, no_corr, no_rpn), and what places the T branch once its form is known."""
    __slots__ = ()

    def t_placement(self, t_form):
        """(placement, alternate) for the T branch's form, 'proposals' or 'detections'.  placement: where the branch
        (correlation map, its crops, the correlation head) of a pair runs --
        'none': nowhere (injected heads, single frames, DODT_PIPE_NO_CORR);
        'detections': behind frame 0's NMS #2 on frame 0's stream, for the kept boxes;
        'img': the map behind the image stack on its stream, crops and head on frame 1's stream;
        'f1': map and crops on frame 1's stream, the head on frame 0's;
        'f0': all of it on frame 0's stream (one side stream).
        alternate: the launches of a pair's two frames alternate stage by stage ('detections' form on two streams: two
        independent chains) instead of one frame after the other; 'img' and 'f1' have orders of their own."""
        if not self.t_branch:
            return 'none', False
        if t_form == 'detections':
            return ('none' if self.no_corr else 'detections'), self.two_streams
        if self.no_corr:
            return 'none', False
        if not self.two_streams:
            return 'f0', False
        return ('img' if self.corr_map_img else 'f1'), False


def resolve_schedule(environ, computed_heads, frames_per_sample, n_side_streams):
    """The pipeline's schedule from the DODT_PIPE_* switches of `environ` (a mapping; None: the process's own) and how it
    was built: the one place that reads them, once per pipeline.  DODT_PIPE_FUSED_TAIL=0: the tail's elementwise ops as
    separate launches; DODT_PIPE_CORR_MAP other than 'img': placement 'f1' instead of 'img'; DODT_PIPE_NO_TAIL /
    _NO_CORR / _NO_RPN (any non-empty value): tools/' steps without the tail / the T branch / the RPN head."""
    if environ is None:
        environ = os.environ
    return Schedule(fused_tail=environ.get('DODT_PIPE_FUSED_TAIL', '1') != '0',
                    no_tail=bool(environ.get('DODT_PIPE_NO_TAIL')), no_corr=bool(environ.get('DODT_PIPE_NO_CORR')),
                    no_rpn=bool(environ.get('DODT_PIPE_NO_RPN')),
                    t_branch=bool(computed_heads) and frames_per_sample == 2, two_streams=n_side_streams >= 2,
                    corr_map_img=environ.get('DODT_PIPE_CORR_MAP', 'img') == 'img')


# One step from the call that enqueues it (FramePairPipeline._step_record: the step, its parity, its record slot, the
# injected heads or None, whether `recover` came with it) to its tail, which adds (_tail) every frame's buffers (its own +
# what its prep left), feature-map views and kept-anchor count, resolves `heads` to those buffers when the pipeline
# computes them, and adds the side streams' head scratch
# `geoms`: the geometry (_Geometry) of every frame of the step, as its prep used it
# `active`: None, or per tracker lane whether the step's pair belongs to that lane's video (tracker=dict(lanes=True))
# `ego`: per pair of the step its (trans, matrix, delta) or None (pipelines with the Kalman tracker, which associates the
# NEXT keyframe with it)
_Step = namedtuple('_Step', 'step cur rslot heads recover geoms fr feat counts scratch active ego', defaults=(None,) * 6)


def _pad_lookahead(lookahead):
    """A call's `lookahead` with its optional entries: None, or (points, n_points, image(s), ego_motion, calib)."""
    return None if lookahead is None else tuple(lookahead) + (None,) * (5 - len(lookahead))


class _Geometry(object):
    """One calibration (config.Calibration) as the launches take it, made once per value (FramePairPipeline._geometry):
    the voxeliser's parameters, the projection and the image size; M's 42 doubles and the BEV support mask when first
    asked for.  Travels with the step it was given for."""

    def __init__(self, cfg, calib):
        self.calib, self.key = calib, calib.key()
        self.p2, self.image_wh = calib.p2, calib.image_wh
        self.bp = ops.make_bev_params(cfg, _config.velo_to_cam(calib.r0_rect, calib.tr_velo_to_cam), self.p2,
                                      self.image_wh)
        self.temporal_calib = None

    def temporal_rows(self):
        if self.temporal_calib is None:
            self.temporal_calib = ops.temporal_calib(self.calib.r0_rect, self.calib.tr_velo_to_cam)
        return self.temporal_calib


class SupportUnion(object):
    """The BEV net's input-support mask under changing calibrations: the OR of the masks (ops.bev_support_mask) of every
    calibration seen so far.  Any superset of a step's true support is sound -- a cell marked "possibly written" that
    receives no point is a zero input, and what the tables skip depends on the weights alone either way (DESIGN
    section 5.0b) --, so the tables are rebuilt only when the union gains a cell: once per calibration of a data set at
    the most.  mask_of(geometry) -> the (PAD_TOP + Z, X) uint8 mask; geometries are told apart by their `key`."""

    def __init__(self, mask_of):
        self.mask_of = mask_of
        self.mask = None               # the union in force
        self.covered = set()           # keys whose own mask is known to lie inside it (it only grows)
        self.rebuilds = 0              # times add() found a new cell

    def add(self, geoms):
        """Take in the geometries of a step.  True when the union gained a cell: the tables are to be rebuilt from
        `mask` before the step's forward."""
        grew = False
        for g in geoms:
            if g.key in self.covered:
                continue
            m = self.mask_of(g) != 0
            if self.mask is None:
                self.mask, grew = m.astype(np.uint8), True
            elif np.any(m & (self.mask == 0)):
                self.mask = (m | (self.mask != 0)).astype(np.uint8)
                grew = True
            self.covered.add(g.key)
        self.rebuilds += int(grew)
        return grew


class FramePairPipeline(object):
    """One GPU's pipeline over samples of the configuration: frame pairs for DODT
    (cfg['frames_per_sample'] == 2: Siamese extractors + correlation branch,
    dt_rpn_model.py / dt_avod_model.py) or single frames for plain AVOD
    (frames_per_sample == 1, e.g. config.CARS_EXAMPLE: rpn_model.py / avod_model.py, no
    correlation branch; `pairs_per_step` then counts frames).  The extractor pair follows
    cfg['extractor'] ('vgg_pyr' or 'vgg')."""

    def __init__(self, ctx, cfg, bev_params, img_params, p2=_config.KITTI_P2,
                 r0_rect=_config.KITTI_R0_RECT, tr_velo_to_cam=_config.KITTI_TR_VELO_TO_CAM,
                 image_wh=_config.KITTI_IMAGE_WH, n_points_max=120000, rpn_nms_size=1024,
                 pairs_per_step=1, side_streams=None, head_params=None, conv_dtype='f32',
                 head_dtype='f32', reuse_streams_of=None, temporal=None, tracker=None,
                 bev_input_skip=True, bev_frame_tables=True, t_branch_rows=None, sequence=False, image_wh_max=None):
        """p2, r0_rect, tr_velo_to_cam, image_wh: the DEFAULT calibration -- what a step without `calib=` uses (self.calib,
        a config.Calibration); every step call takes another one per sample (run()).
        image_wh_max: None (= image_wh), or the (w, h) no host image exceeds in either dimension: the size of the
        staging buffers of run_from_host() / push_frame_from_host().
        temporal: None, or dict(n_frames=tau + 1, threshold=0.1, on_conflict='raise' | 'next_best') -- the temporal
        module M on the device after every step (see _temporal_step, frames()); None enqueues nothing for it.
        tracker: None, or dict(score_threshold=0.1, high_threshold=0.5, iou_threshold=0.005, t_min=3,
        classes=cfg['classes'], max_sequence_dets=65536) -- the IoU tracker on the device after every step: the pairs of
        the steps, in order, are one sequence until end_sequence() (see _tracker_step, tracks_so_far()); None enqueues and allocates nothing
        for it.  With lanes=True pair p of every step belongs to LANE p instead: pairs_per_step (at most 5, the
        pipeline's limit) videos side by side, each lane with its own tracker state, calibration and
        end_sequence(lane=) (run()'s `active`); needs sequence=False.
        With kind='kalman' (default 'iou') the stage is the Kalman-filter tracker instead:
        dict(kind='kalman', sigma_l=0.0, iou_threshold=0.1, max_age=3, min_hits=3, stride=None, L=10.0, R_scaler=1/16,
        score_threshold=0.1, max_sequence_dets=65536) -- pair j's keyframe 0 is keyframe j of the sequence, the last
        pair's keyframe 1 the final one; stride: frames between two keyframes (None: tau of `temporal`, or 1).  Every
        ego_motion entry of its steps is None (parked) or (trans, matrix, delta); tracks_so_far() and end_sequence()
        return kalman_tracker.Tracker objects.
        With kind='velocity' it is the velocity-extrapolating greedy IoU tracker:
        dict(kind='velocity', sigma_l=0.1, sigma_h=0.5, sigma_iou=0.1, t_min=3, extend_len=3, stride=None,
        score_threshold=0.1, log_capacity=65536) -- keyframes, stride and ego_motion entries as for kind='kalman';
        tracks_so_far() and end_sequence(frame_total=None) return video_detection_iou.interpolate_by_track's track dicts
        (None: the sequence ends at the last keyframe), kitti_tracking_rows() that module's rows; no frame_ids.
        Both kinds take lanes=True beside their keys (DESIGN sections 8g, 8h): pair p of every step is lane p, each lane
        with its own tracker state, its pair's calibration (p2, image size and recovery rows) and its pair's ego_motion
        entry -- a lane's own motion associates THAT lane's next keyframe; an inactive lane's entry is ignored and its
        pending one kept.  Needs sequence=False and pairs_per_step >= 2 (one lane is the plain tracker).  run()'s
        `active`, tracks_so_far(lane=), end_sequence(lane=, frame_total=) and kitti_tracking_rows(lane=) work per lane under
        the single forms' rules (frame ids keyframe * stride, no frame_ids); end_sequence(lane=p) flushes lane p with its
        own calibration and pending ego, downloads and resets it, and leaves the other lanes running.
        bev_input_skip: the fp32 BEV net skips the tiles that no BEV cell inside the camera's frustum reaches (their
        values depend on the weights alone, dodt_extractor_set_input_support); False: full tables.
        bev_frame_tables: with bev_input_skip, every step also filters those tables on the device by the cells that are
        non-zero in its own BEV maps (dodt_extractor_set_frame_tables); False: the static tables alone.
        t_branch_rows: the rows the T branch (correlation map, its crops, the correlation head) is computed for when the
        pipeline computes its heads.  'proposals': all P proposals of a pair's frame 0, the map on the image stream
        behind the image stack; fr[f]['corr_rois'] / ['corr_offsets'] then hold every proposal's row (inspection
        outputs of this form only).  'detections': the <= MAX_DET boxes NMS #2 keeps, the only rows the records read --
        behind frame 0's NMS #2 on its own stream: the map at the tiles those boxes' crops touch, the crops, the head at
        MAX_DET rows (fr[f]['det_corr_rois'] / ['det_corr_offsets'], row j for box det_idx[j]); the same records, bit for
        bit.  None (default): 'detections' when the records go to caller-owned memory (use_record_buffers /
        use_record_ring called before the first run(): the streaming use, whose caller reads records and nothing else),
        'proposals' otherwise.  The tile list of 'detections' is built in one workgroup's LDS, which holds a map of up to
        ops.CORR_TILE_LIST_MAX 16 x 16 tiles (the 700 x 800 map has 2200): on a larger map None means 'proposals' and
        'detections' is refused here.  t_branch_form() gives the form in use; the first run() fixes it.  Injected heads
        keep their per-proposal offsets array whatever the argument.
        sequence: the steps are the overlapping keyframe pairs of one sequence (the reference's evaluation order,
        kitti_tracking_dataset.py:266-272): push_frame() takes ONE new frame per step and pairs it with the previous one,
        whose image maps, anchor filter and projections are kept from the step before.  Needs frame
        pairs, one per step; run() / run_from_host() are refused on such a pipeline, push_frame() on any other."""
        self.sequence = bool(sequence)
        if self.sequence and (int(cfg.get('frames_per_sample', 2)) != 2 or int(pairs_per_step) != 1):
            raise ValueError('sequence: needs frames_per_sample == 2 and pairs_per_step == 1')
        if t_branch_rows not in (None, 'proposals', 'detections'):
            raise ValueError("t_branch_rows must be None, 'proposals' or 'detections'")
        self.t_branch_rows = t_branch_rows
        self._t_form = None                         # (the first run() fixes it, _resolve_t_branch)
        self._caller_records = False
        self.ctx = ctx
        self.cfg = cfg
        self.p2 = np.asarray(p2, dtype=np.float64)
        self.image_wh = tuple(image_wh)
        self.P = int(rpn_nms_size)
        self.n_points_max = int(n_points_max)
        self.pairs = int(pairs_per_step)               # samples per step
        self.fps = int(cfg.get('frames_per_sample', 2))
        # stage-2 classification columns: the background and one per class.  Two (one class) take the two-way kernels;
        # more take the *_classes entries, which also give every record its type (_decode_nms2, _records)
        self.classes = tuple(cfg.get('classes', ('Car',)))
        self.n_cls = len(self.classes) + 1
        if not 2 <= self.n_cls <= 8:
            raise ValueError('1 to 7 classes')
        if self.fps not in (1, 2):
            raise ValueError('frames_per_sample must be 1 or 2')
        self.temporal = self._temporal_args(temporal)
        self.tracker = self._tracker_args(tracker)
        self.nf = self.fps * self.pairs                # frames per step
        self.bev_h, self.bev_w = cfg['bev_dims']
        self.img_h, self.img_w = cfg['img_dims']
        self.n_slices = cfg['num_slices']
        self.bev_extents_flat = np.asarray(cfg['bev_extents'], np.float64).reshape(-1)
        # the geometries seen so far, by value; the default one also as the attributes it has always been
        self._geoms = {}
        self.geom0 = self._geometry(_config.Calibration(self.p2, r0_rect, tr_velo_to_cam, self.image_wh))
        self.calib, self.p2, self.image_wh, self.bp = self.geom0.calib, self.geom0.p2, self.geom0.image_wh, self.geom0.bp
        self.image_wh_max = self.image_wh if image_wh_max is None else (int(image_wh_max[0]), int(image_wh_max[1]))
        if self.image_wh_max[0] < self.image_wh[0] or self.image_wh_max[1] < self.image_wh[1]:
            raise ValueError('image_wh_max is smaller than image_wh')
        self.track_geom = None         # the geometry of the tracker's current sequence (None: none has begun)
        self.lanes = self.tracker is not None and self.tracker['lanes']
        self.kalman = self.tracker is not None and self.tracker.get('kind') == 'kalman'
        self.velocity = self.tracker is not None and self.tracker.get('kind') == 'velocity'
        self.track_geoms = [None] * self.pairs      # (lanes: the same per lane)
        # streams: conv stacks of the two nets side by side, per-frame work on its own.  A second pipeline in the same
        # process takes the first one's streams (`reuse_streams_of`): new ones would share hardware queues with them
        if reuse_streams_of is not None:
            self.img_ctx, self.sides = reuse_streams_of.img_ctx, reuse_streams_of.sides
        else:
            # one side stream per frame of a pair (or `side_streams`): ROCm maps a process's streams onto 4 hardware
            # queues; a fifth stream shares a queue with another one and runs behind its launches (measured: 6 streams
            # 164, 5 streams 180, 4 streams 191 pairs/s), so a frame's prep and tail share a stream
            self.img_ctx = device.Context(ctx.device_id)
            n_side = min(self.nf, 2) if side_streams is None else int(side_streams)
            self.sides = [device.Context(ctx.device_id) for _ in range(max(n_side, 1))]
        self.sched = resolve_schedule(None, head_params is not None, self.fps, len(self.sides))
        self.placement = self.alternate = None      # (of the T branch: the first run() fixes them with its form)
        # ---- constants of the configuration, resident on the device ----------------
        # (one grid per class, concatenated class-major: dt_rpn_model.py:894-909; the filter, the compaction and the RPN
        #  take the rows as they come)
        sizes, strides = _config.class_anchor_params(cfg)
        boxes = gen.tile_anchors_3d_classes(cfg['area_extents'], sizes, strides, cfg['ground_plane'])
        self.anchors_all = gen.box_3d_to_anchor(boxes)            # (N,6) float64
        cells, self.nx, self.nz = gen.anchor_grid_cells(
            self.anchors_all, cfg['area_extents'], cfg['voxel_size'])
        self.n_all = len(self.anchors_all)
        self.d_anchor_table = ctx.array(self.anchors_all)
        self.d_cells = ctx.array(cells)

        # ---- extractors: every frame of the step is one batch ------------------------
        bev_cls, img_cls = EXTRACTORS[cfg.get('extractor', 'vgg_pyr')]
        self.bev_net = bev_cls(ctx=ctx, shared_gpu=True, conv_dtype=conv_dtype)
        self.bev_net.load_params(bev_params)
        self.bev_net._ensure(self.nf, self.bev_h, self.bev_w, cfg['bev_depth'])
        # only cells inside the image frustum are ever non-zero (the ego-motion warp comes before the frustum test)
        # (under several calibrations: the union of their supports, grown in front of the first BEV forward that needs
        #  it, _grow_support; bev_skipped_items is the current union's count)
        self.bev_skipped_items = 0
        self.support = None
        if bev_input_skip and conv_dtype == 'f32' and hasattr(self.bev_net, 'set_input_support') \
                and self.bp.point_format == _lib.PTS_VELO_XYZI:
            # (the callable holds the pad and the library, not the pipeline: a reference cycle would keep a dropped
            #  pipeline's device memory until the cycle collector happens to run, and free it under another one's steps)
            pad_top, lib = self.bev_net.PAD_TOP, ctx.lib
            self.support = SupportUnion(lambda g: ops.bev_support_mask(g.bp, pad_top, lib))
            self._bev_frame_tables = bev_frame_tables
            self._grow_support([self.geom0])
        self.img_net = img_cls(ctx=self.img_ctx, shared_gpu=True, conv_dtype=conv_dtype)
        self.img_net.load_params(img_params)
        n_img = 1 if self.sequence else self.nf        # (sequence mode: one forward per NEW frame)
        self.img_net._ensure(n_img, self.img_h, self.img_w, 4)
        # feature maps the crops read: (700,800,32) / (360,1200,32) for the pyramid,
        # (350,400,256) / (240,795,256) for the plain VGG
        self.bev_fh, self.bev_fw, self.feat_c = self.bev_net.output_shape()
        self.img_fh, self.img_fw, img_c = self.img_net.output_shape()
        if img_c != self.feat_c:
            raise ValueError('mean fusion needs equal feature depths')
        # conv inputs, double-buffered so that step k+1 is prepared under the convs of step k
        # (in the extractors' own input layout -- the BEV maps behind four zero rows, bev_vgg_pyramid.py:58 --, so
        #  that the first conv layer reads them in place: forward_device_padded)
        self.bev_pad = self.bev_net.PAD_TOP
        self.in_bev = [ctx.zeros((self.nf, self.bev_pad + self.bev_h, self.bev_w, cfg['bev_depth']), np.float32)
                       for _ in range(2)]
        self.in_img = [ctx.zeros((n_img, self.img_net.PAD_TOP + self.img_h, self.img_w, 4), np.float32)
                       for _ in range(2)]
        # per-frame views of them, by parity
        self.bev_in = [self._views(a, (self.bev_h, self.bev_w, cfg['bev_depth']), self.bev_pad) for a in self.in_bev]
        self.img_in = [self._views(a, (self.img_h, self.img_w, 4), self.img_net.PAD_TOP, n_img) for a in self.in_img]
        self.d_bev_in = self.bev_in[0]             # (of the most recently finished step)

        # ---- dense heads (weights shared, scratch per side stream) ------------------------
        f32, i32 = np.float32, np.int32
        N, P = self.n_all, self.P
        self.rpn_head = self.avod_head = self.corr_head = self.head_scratch = None
        rep = cfg.get('box_representation', 'box_4ca')
        if rep not in ('box_4c', 'box_4ca'):
            raise NotImplementedError('Regression not implemented for %s' % rep)
        self.box_4ca = rep == 'box_4ca'
        if head_params is not None:
            self.rpn_head = AnchorPredictor(ctx, head_params['rpn'], dtype=head_dtype)
            self.avod_head = EarlyFusionFcLayers(
                ctx, head_params['avod'], dtype=head_dtype,
                outputs=('cls_out', 'off_out') + (('ang_out',) if self.box_4ca else ()))
            if self.fps == 2:
                self.corr_head = EarlyFusionFcLayers(ctx, head_params['corr'],
                                                     outputs=('off_out',), dtype=head_dtype)
            self.head_scratch = [dict(rpn=self.rpn_head.make_scratch(N), fc=self.avod_head.make_scratch(P),
                                      corr_map=ctx.empty((self.bev_fh, self.bev_fw, CORR_CH), f32)
                                      if self.fps == 2 else None) for _ in self.sides]
            # the pairs' correlation maps, by step parity (written behind the image stack on its stream, see _step();
            # 'proposals' form only: made by _resolve_t_branch at the first run())
            self.corr_maps = None
            if t_branch_rows == 'detections' and self.corr_head is not None and not self._tile_list_fits():
                raise ValueError("t_branch_rows='detections': the %d x %d map has more than %d tiles"
                                 % (self.bev_fh, self.bev_fw, ops.CORR_TILE_LIST_MAX))

        # ---- work buffers ----------------------------------------------------------------
        FC = self.feat_c
        # (sequence mode: the image net's maps of a keyframe serve two steps and live in img_ring instead)
        self.feat = []
        for _ in range(2):
            d = dict(bev_feat=ctx.empty((self.nf, self.bev_fh, self.bev_fw, FC), f32),
                     bev_bneck=ctx.empty((self.nf, self.bev_fh, self.bev_fw, 1), f32))
            if not self.sequence:
                d.update(img_feat=ctx.empty((self.nf, self.img_fh, self.img_fw, FC), f32),
                         img_bneck=ctx.empty((self.nf, self.img_fh, self.img_fw, 1), f32))
            self.feat.append(d)
        if self.sequence:
            # a ring of single-frame slots, keyframe j in slot j % IMG_RING (sequence_slots)
            self.img_ring = [dict(img_feat=ctx.empty((1, self.img_fh, self.img_fw, FC), f32),
                                  img_bneck=ctx.empty((1, self.img_fh, self.img_fw, 1), f32)) for _ in range(IMG_RING)]
            self.img_ring_views = [{name: a.offset(0, a.shape[1:]) for name, a in d.items()} for d in self.img_ring]
        # per-frame views of them: feat_views[parity][frame][name]
        self.feat_views = [[{name: a.offset(a.nbytes // self.nf * f, a.shape[1:]) for name, a in d.items()}
                            for f in range(self.nf)] for d in self.feat]
        # what a step's prep leaves for its tail, THREE deep (step k: set k % 3): with look-ahead (run(...,
        # lookahead=)) the prep of step k + 1 is enqueued in front of the tail of step k - 1, which still reads
        # the set of its own step
        def prep_set():
            return dict(occ=ctx.empty((self.nz, (self.nx + 31) // 32), np.uint32),
                        keep=ctx.empty((N,), i32), count=ctx.zeros((1,), i32),
                        bev_norm=ctx.empty((N, 4), f32), img_norm=ctx.empty((N, 4), f32),
                        anchors=ctx.empty((N, 6), f32))
        if self.sequence:
            # ... one set per KEYFRAME, shared by the two steps it belongs to, PREP_RING deep (sequence_slots); and the
            # pipeline's own copy of each keyframe's points for its plain voxelisation as frame 0, one step after the
            # caller handed them over
            self.prep_sets = [prep_set() for _ in range(PREP_RING)]
            self.pts_ring = [ctx.empty((self.n_points_max, 4), f32) for _ in range(POINT_RING)]
            self.pts_n = [0] * POINT_RING
            # ... and each keyframe's geometry beside both: what its tails project with, what the plain voxelisation takes
            self.prep_geoms = [self.geom0] * PREP_RING
            self.pts_geoms = [self.geom0] * POINT_RING
            self.seq_geom = self.geom0     # the geometry of the current sequence (a priming push sets it)
            self.d_row_ids = ctx.array(np.arange(self.n_points_max, dtype=i32))     # (the copy is a gather of all rows)
            self.seq_primed = False        # a keyframe stands ready to be frame 0 of the next step
            self.seq_prime_parity = None   # parity of the image input a priming push's forward read (_seq_prep_new)
        else:
            self.prep3 = [[prep_set() for _ in range(self.nf)] for _ in range(3)]
            self.prep_geoms = [[self.geom0] * self.nf for _ in range(3)]      # (per frame, beside prep3)
        if 3 * self.nf > 32:
            raise ValueError('at most 10 frames per step (count fetch slots)')
        # fetch slot -> the kept-anchor count read from it; None between a prep's fetch_i32_begin and the first tail that
        # reads it (a sequence's keyframe has two tails and one fetch)
        self.kept_counts = {}
        self.fr2 = [[], []]
        for f in range(2 * self.nf):
            b = dict(
                rpn_bev_roi=ctx.empty((N, 3, 3, 1), f32), rpn_img_roi=ctx.empty((N, 3, 3, 1), f32),
                regressed=ctx.empty((N, 6), f32), prop_bev=ctx.empty((N, 4), f32),
                scores=ctx.empty((N,), f32),
                top_idx=ctx.empty((P,), i32), top_count=ctx.zeros((1,), i32),
                top_anchors=ctx.empty((P, 6), f32),
                top_bev=ctx.empty((P, 4), f32), top_img=ctx.empty((P, 4), f32),
                bev_rois=ctx.empty((P, ROI, ROI, FC), f32),
                img_rois=ctx.empty((P, ROI, ROI, FC), f32),
                boxes_3d=ctx.empty((P, 7), f32), pred_anchors=ctx.empty((P, 6), f32),
                nms2_boxes=ctx.empty((P, 4), f32), nms2_scores=ctx.empty((P,), f32),
                det_idx=ctx.empty((MAX_DET,), i32), det_count=ctx.zeros((1,), i32),
                det_scores=ctx.empty((P,), f32), orientations=ctx.empty((P,), f32))
            if self.n_cls > 2:
                b.update(det_types=ctx.zeros((P,), i32))
            if head_params is not None:
                b.update(rpn_logits=ctx.empty((N, 2), f32), rpn_offsets=ctx.empty((N, 6), f32),
                         cls_logits=ctx.empty((P, self.n_cls), f32), offsets_4c=ctx.empty((P, 10), f32))
                if self.box_4ca:
                    b.update(angle_vectors=ctx.empty((P, 2), f32))
                if self.fps == 2 and f % 2 == 0:
                    # rows of the correlation head's padded K (zeros behind each 7x7x25 crop)
                    b.update(corr_rois=ctx.zeros((P, self.corr_head.in_ld), f32),
                             corr_offsets=ctx.empty((P, 3), f32))
            self.fr2[f // self.nf].append(b)
        # buffers of the most recently finished step
        self.fr = [dict(b, **p) for b, p in zip(self.fr2[0], self.prep_sets if self.sequence else self.prep3[0])]
        self.prepped = -1              # step whose prep a look-ahead has already enqueued
        self.step_idx = 0
        self.pending = None            # step whose tail has not been enqueued yet
        # detection records of a step: what the all-gather ships.  A ring of R >= 2
        # buffers, step k fills slot k % R (R = 2: by step parity); use_record_ring() makes it
        # longer so that the exchange step can ship several steps at once
        self.rec2 = [ctx.empty((self.pairs, self.fps, MAX_DET, REC_COLS), f32) for _ in range(2)]
        self.cnt2 = [ctx.zeros((self.pairs, self.fps), i32) for _ in range(2)]
        self.d_records, self.d_rec_counts = self.rec2[0], self.cnt2[0]   # last finished step
        self.last_anchor_counts = [0] * self.nf
        # hook(slot, side contexts), called before a tail refills record slot `slot`: the exchange
        # step (sharding.Communicator.join) makes the tails wait for the all-gather that last
        # read it, at least a ring's half earlier
        self.on_records_reuse = None
        # ---- temporal module M (opt-in): the frames between a pair's keyframes -----------------
        if self.temporal is not None:
            self.temporal_calib = self.geom0.temporal_rows()
            self._alloc_frames()
        # ---- the IoU tracker (opt-in): one sequence's state on the device, launches on the image stream ------------
        if self.tracker is not None:
            tk = self.tracker
            if self.kalman and self.lanes:      # one state per pair of a step, in one buffer
                self.track_state = tracking.KalmanTrackerLanes(self.ctx, self.pairs, tk['sigma_l'], tk['iou_threshold'],
                                                               tk['max_age'], tk['min_hits'], tk['L'], tk['R_scaler'],
                                                               log_capacity=tk['max_sequence_dets'],
                                                               score_threshold=tk['score_threshold'])
            elif self.velocity and self.lanes:
                self.track_state = tracking.VelocityTrackerLanes(self.ctx, self.pairs, tk['sigma_l'], tk['sigma_h'],
                                                                 tk['sigma_iou'], tk['t_min'], tk['extend_len'],
                                                                 self._kalman_stride(), log_capacity=tk['log_capacity'],
                                                                 score_threshold=tk['score_threshold'])
            elif self.kalman:
                self.track_state = tracking.KalmanTracker(self.ctx, tk['sigma_l'], tk['iou_threshold'], tk['max_age'],
                                                          tk['min_hits'], tk['L'], tk['R_scaler'],
                                                          log_capacity=tk['max_sequence_dets'])
            elif self.velocity:
                self.track_state = tracking.VelocityTracker(self.ctx, tk['sigma_l'], tk['sigma_h'], tk['sigma_iou'],
                                                            tk['t_min'], tk['extend_len'], self._kalman_stride(),
                                                            log_capacity=tk['log_capacity'])
            elif self.lanes:     # one state per pair of a step, in one buffer
                self.track_state = tracking.TrackerLanes(self.ctx, self.pairs, tk['max_sequence_dets'],
                                                         tk['high_threshold'], tk['iou_threshold'], tk['t_min'],
                                                         tk['score_threshold'])
            else:
                self.track_state = tracking.Tracker(self.ctx, tk['max_sequence_dets'], tk['high_threshold'],
                                                    tk['iou_threshold'], tk['t_min'], tk['score_threshold'])
            self.img_ctx.wait_for(self.ctx)          # (the state's reset went on the main stream)
            self.last_sequence_tracks = [None] * self.pairs if self.lanes else None
        self.mark_steps = ()           # tools/pipe_marks.py: steps whose stages get timing marks
        self.marks = {}                # name -> (context, slot)
        ctx.sync()

    def _temporal_args(self, temporal):
        if temporal is None:
            return None
        if self.fps != 2:
            raise ValueError('temporal: needs frame pairs (frames_per_sample == 2)')
        t = dict(temporal)
        tm = dict(n_frames=int(t.pop('n_frames')), threshold=float(t.pop('threshold', 0.1)),
                  on_conflict=t.pop('on_conflict', 'raise'))
        if t:
            raise ValueError('temporal: unknown keys %s' % sorted(t))
        if tm['on_conflict'] not in ('raise', 'next_best'):
            raise ValueError("temporal: on_conflict must be 'raise' or 'next_best'")
        if not 1 <= tm['n_frames'] <= 64:
            raise ValueError('temporal: n_frames must be 1..64')
        return tm

    def _tracker_args(self, tracker):
        if tracker is None:
            return None
        if self.fps != 2:
            raise ValueError('tracker: needs frame pairs (frames_per_sample == 2)')
        t = dict(tracker)
        kind = t.pop('kind', 'iou')
        if kind == 'kalman':
            return self._kalman_args(t)
        if kind == 'velocity':
            return self._velocity_args(t)
        if kind != 'iou':
            raise ValueError("tracker: kind must be 'iou', 'kalman' or 'velocity'")
        tk = dict(score_threshold=float(t.pop('score_threshold', 0.1)),
                  high_threshold=float(t.pop('high_threshold', 0.5)),
                  iou_threshold=float(t.pop('iou_threshold', 0.005)), t_min=int(t.pop('t_min', 3)),
                  classes=tuple(t.pop('classes', self.classes)), max_sequence_dets=int(t.pop('max_sequence_dets', 65536)),
                  lanes=bool(t.pop('lanes', False)))
        if t:
            raise ValueError('tracker: unknown keys %s' % sorted(t))
        if tk['lanes'] and self.sequence:
            raise ValueError('tracker: lanes need sequence=False (one lane per pair of a step)')
        if tk['max_sequence_dets'] < 1:
            raise ValueError('tracker: max_sequence_dets must be >= 1')
        return tk

    def _kind_lanes(self, t, kind):
        """The `lanes` key of tracker=dict(kind='kalman' | 'velocity', ...): what it needs, refused before anything
        touches the context."""
        lanes = bool(t.pop('lanes', False))
        if lanes and self.sequence:
            raise ValueError('tracker: lanes need sequence=False (one lane per pair of a step)')
        if lanes and self.pairs < 2:
            raise ValueError("tracker: kind='%s' with lanes=True needs pairs_per_step >= 2 (one lane per pair of a step; "
                             "one lane is the plain tracker, lanes=False)" % kind)
        return lanes

    def _kalman_args(self, t):
        """tracker=dict(kind='kalman', ...) without its kind."""
        lanes = self._kind_lanes(t, 'kalman')
        stride = t.pop('stride', None)
        tk = dict(kind='kalman', lanes=lanes, score_threshold=float(t.pop('score_threshold', 0.1)),
                  sigma_l=float(t.pop('sigma_l', 0.0)), iou_threshold=float(t.pop('iou_threshold', 0.1)),
                  max_age=int(t.pop('max_age', 3)), min_hits=int(t.pop('min_hits', 3)),
                  stride=None if stride is None else int(stride), L=float(t.pop('L', 10.0)),
                  R_scaler=float(t.pop('R_scaler', 1.0 / 16)), classes=tuple(t.pop('classes', self.classes)),
                  max_sequence_dets=int(t.pop('max_sequence_dets', 65536)))
        if t:
            raise ValueError('tracker: unknown keys %s' % sorted(t))
        if tk['stride'] is not None and tk['stride'] < 1:
            raise ValueError('tracker: stride must be >= 1')
        if tk['max_sequence_dets'] < 1:
            raise ValueError('tracker: max_sequence_dets must be >= 1')
        return tk

    def _velocity_args(self, t):
        """tracker=dict(kind='velocity', ...) without its kind."""
        lanes = self._kind_lanes(t, 'velocity')
        stride = t.pop('stride', None)
        tk = dict(kind='velocity', lanes=lanes, score_threshold=float(t.pop('score_threshold', 0.1)),
                  sigma_l=float(t.pop('sigma_l', 0.1)), sigma_h=float(t.pop('sigma_h', 0.5)),
                  sigma_iou=float(t.pop('sigma_iou', 0.1)), t_min=int(t.pop('t_min', 3)),
                  extend_len=int(t.pop('extend_len', 3)), stride=None if stride is None else int(stride),
                  classes=tuple(t.pop('classes', self.classes)), log_capacity=int(t.pop('log_capacity', 65536)))
        if t:
            raise ValueError('tracker: unknown keys %s' % sorted(t))
        if tk['stride'] is not None and not 1 <= tk['stride'] <= tracking.VT_MAX_STEP:
            raise ValueError('tracker: stride must be 1..%d' % tracking.VT_MAX_STEP)
        if not 1 <= tk['extend_len'] <= tracking.VT_MAX_STEP:
            raise ValueError('tracker: extend_len must be 1..%d' % tracking.VT_MAX_STEP)
        if tk['log_capacity'] < 1:
            raise ValueError('tracker: log_capacity must be >= 1')
        return tk

    def _ego_deltas(self):
        """The tracker stage associates across the ego-motion: every ego_motion entry must bring its yaw delta."""
        # (getattr: __init__ always sets `velocity`; objects made bare by __new__, as tests/test_kalman_device_args.py
        #  makes them, set `kalman` alone)
        return self.kalman or getattr(self, 'velocity', False)

    def _check_ego(self, *ego_motions):
        """Kalman and velocity trackers: what the association cannot take, refused before anything is enqueued.
        ego_motions: a step's ego_motion (None, or a list of entries) -- this call's and its look-ahead's."""
        if not self._ego_deltas():
            return
        for em in ego_motions:
            if em is not None and len(em) != (1 if self.sequence else self.pairs):
                raise ValueError('ego_motion: one entry per pair of the step')
            for e in em or ():
                if e is not None and len(e) != 3:
                    raise ValueError("ego_motion: with tracker kind='%s' an entry is None (parked) or (trans, matrix, "
                                     "delta); the association needs the yaw delta"
                                     % ('kalman' if self.kalman else 'velocity'))

    # ---- per-sample geometry -------------------------------------------------------------------
    def _geometry(self, calib):
        """The _Geometry of a calibration, one per value."""
        if not isinstance(calib, _config.Calibration):
            calib = _config.Calibration(*calib)
        key = calib.key()
        g = self._geoms.get(key)
        if g is None:
            g = self._geoms[key] = _Geometry(self.cfg, calib)
        return g

    def _step_geoms(self, calib):
        """A step call's `calib` -> the geometry of every FRAME of the step: None -- the constructor's calibration --, one
        Calibration for every sample, or a list with one per sample."""
        if calib is None:
            return [self.geom0] * self.nf
        if isinstance(calib, _config.Calibration):
            return [self._geometry(calib)] * self.nf
        if len(calib) != self.pairs:
            raise ValueError('calib: one Calibration, or a list of %d (one per sample of the step)' % self.pairs)
        return [g for cal in calib for g in [self._geometry(cal)] * self.fps]

    @staticmethod
    def _same_geoms(a, b):
        return all(x is y for x, y in zip(a, b))       # (one object per value, _geometry)

    def _check_images(self, images, geoms, host):
        """Every image of a step against its sample's image size, where the array carries a shape; a host image also
        against the staging buffers."""
        for f, (img, g) in enumerate(zip(images, geoms)):
            w, h = g.image_wh
            shape = getattr(img, 'shape', None)
            if shape is not None and tuple(shape) != (h, w, 3):
                raise ValueError('frame %d: the image is %s, its calibration says (%d, %d, 3)' % (f, tuple(shape), h, w))
            if host and (w > self.image_wh_max[0] or h > self.image_wh_max[1]):
                raise ValueError('frame %d: a %d x %d host image exceeds image_wh_max %s' % (f, w, h, self.image_wh_max))

    def _grow_support(self, geoms):
        """In front of a BEV forward: the skip tables follow the union of the supports of every calibration seen so far
        (SupportUnion) and are rebuilt -- a stream synchronisation, every table freed and made again, the next forward
        on full tables -- only when a step brings a calibration whose support has a cell outside it."""
        if self.support is not None and self.support.add(geoms):
            self.bev_skipped_items = self.bev_net.set_input_support(self.support.mask,
                                                                    frame_tables=self._bev_frame_tables)

    def _mark(self, c, step, name):
        """Timing mark `name` of step `step` on context c (only for steps in mark_steps)."""
        if step in self.mark_steps:
            slot = sum(1 for (cc, _) in self.marks.values() if cc is c)
            if slot < 64:
                c.mark(slot)
                self.marks['%d:%s' % (step, name)] = (c, slot)

    def _views(self, arr, shape, pad_top=0, n=None):
        """Per-frame views of a batch buffer whose frames are pad_top + shape[0] rows tall: the rows behind the pad."""
        row = int(np.prod(shape[1:])) * 4
        frame = (pad_top + shape[0]) * row
        return [arr.offset(frame * f + pad_top * row, shape) for f in range(self.nf if n is None else n)]

    def _tile_list_fits(self):
        return ops.correlation_tile_capacity((self.bev_fh, self.bev_fw)) <= ops.CORR_TILE_LIST_MAX

    def t_branch_form(self):
        """'proposals' or 'detections': t_branch_rows, None resolved by the rule of __init__ -- as it stands now until
        the first run(), as that run found it from then on."""
        if self._t_form is not None:
            return self._t_form
        if self.t_branch_rows is not None:
            return self.t_branch_rows
        return 'detections' if self._caller_records and self._tile_list_fits() else 'proposals'

    def _t_detections(self):
        return self.corr_head is not None and self.t_branch_form() == 'detections'

    def _resolve_t_branch(self):
        """Fix the T branch's form at the first run() and make that form's buffers."""
        if self._t_form is not None:
            return
        self._t_form = self.t_branch_form()
        self.placement, self.alternate = self.sched.t_placement(self._t_form)
        if self.corr_head is None:
            return
        ctx, f32, i32 = self.ctx, np.float32, np.int32
        if self._t_form == 'proposals':
            self.corr_maps = [[ctx.empty((self.bev_fh, self.bev_fw, CORR_CH), f32) for _ in range(self.pairs)]
                              for _ in range(2)]
            return
        self.corr_tile_cap = ops.correlation_tile_capacity((self.bev_fh, self.bev_fw))
        for s in self.head_scratch:    # one tile list per side stream, beside its correlation map
            s.update(corr_tiles=ctx.empty((self.corr_tile_cap,), i32), corr_ntiles=ctx.zeros((1,), i32))
        for frames in self.fr2:
            for f, b in enumerate(frames):
                if f % 2 == 0:
                    # row j: the crop / the offsets of box det_idx[j] (zeros behind each 7x7x25 crop, as in corr_rois;
                    # the offsets start as zeros: DODT_PIPE_NO_CORR=1 leaves them so)
                    b.update(det_corr_rois=ctx.zeros((MAX_DET, self.corr_head.in_ld), f32),
                             det_corr_offsets=ctx.zeros((MAX_DET, 3), f32))
        ctx.sync()

    def use_record_buffers(self, rec_ptrs, cnt_ptrs):
        """Write detection records into caller-owned device memory (e.g. buffers registered with
        a communication library): R >= 2 of each, step k fills number k % R.  Called before the first run() on a
        pipeline built with t_branch_rows=None, it also selects the T branch's 'detections' form (see __init__)."""
        if len(rec_ptrs) < 2 or len(rec_ptrs) != len(cnt_ptrs):
            raise ValueError('use_record_buffers: at least two record and count buffers, as many of each')
        self._caller_records = True
        self.rec2 = [self.ctx.wrap(p, (self.pairs, self.fps, MAX_DET, REC_COLS), np.float32)
                     for p in rec_ptrs]
        self.cnt2 = [self.ctx.wrap(p, (self.pairs, self.fps), np.int32) for p in cnt_ptrs]
        self.d_records, self.d_rec_counts = self.rec2[0], self.cnt2[0]
        self._alloc_frames()

    def _alloc_frames(self):
        """M's outputs (and the recovery parameters it reads): a ring as long as the record ring, step k in slot k % R."""
        if self.temporal is None:
            return
        R, n = len(self.rec2), self.temporal['n_frames']
        self.frames2 = [self.ctx.empty((self.pairs, n, 2 * MAX_DET, 13), np.float64) for _ in range(R)]
        self.fcnt2 = [self.ctx.zeros((self.pairs, n), np.int32) for _ in range(R)]
        self.fst2 = [self.ctx.zeros((self.pairs,), np.int32) for _ in range(R)]
        # (on the image stream, which M runs on: an upload there is ordered behind M of the step that last read the slot)
        self.ego2 = [self.img_ctx.zeros((self.pairs, n, 13), np.float64) for _ in range(R)]
        # ... and, for a step whose pairs differ in calibration, M's 42 doubles per pair (_upload_recover)
        self.cal2 = [self.img_ctx.zeros((self.pairs, 42), np.float64) for _ in range(R)]
        self.d_frames, self.d_frame_counts, self.d_frame_status = self.frames2[0], self.fcnt2[0], self.fst2[0]

    def use_record_ring(self, d_rec_ring, d_cnt_ring):
        """The same with one contiguous ring: d_rec_ring (R, pairs, fps, MAX_DET, REC_COLS) float32,
        d_cnt_ring (R, pairs, fps) int32 -- so that any run of consecutive slots is one message."""
        R = d_rec_ring.shape[0]
        if tuple(d_rec_ring.shape[1:]) != (self.pairs, self.fps, MAX_DET, REC_COLS) or \
                tuple(d_cnt_ring.shape) != (R, self.pairs, self.fps):
            raise ValueError('use_record_ring: shapes do not match the pipeline')
        nr, nc = 4 * self.pairs * self.fps * MAX_DET * REC_COLS, 4 * self.pairs * self.fps
        self.use_record_buffers([d_rec_ring.ptr + nr * i for i in range(R)],
                                [d_cnt_ring.ptr + nc * i for i in range(R)])

    # ------------------------------------------------------------------------------------
    def _stage_image(self, c, d_stage, h_image, g):
        """Enqueue the copy of a host image of g's size into the head of the max-sized staging buffer d_stage on stream
        c.  -> the device array the prep reads: the buffer itself, or its head viewed as that image."""
        w, h = g.image_wh
        if (h, w, 3) == d_stage.shape:
            return d_stage.upload_async(h_image, ctx=c)
        d_stage.upload_async(h_image, ctx=c, nbytes=h * w * 3)
        return d_stage.offset(0, (h, w, 3))

    def _stage_from_host(self, k, h_points, n_points, h_images, geoms):
        """Enqueue the copies of step k's raw frames from pinned host memory on its frames' side streams."""
        cur = k & 1
        ns = len(self.sides)
        if not hasattr(self, 'stage'):
            H, W = self.image_wh_max[1], self.image_wh_max[0]
            self.stage = [[(self.ctx.empty((self.n_points_max, 4), np.float32),
                            self.ctx.empty((H, W, 3), np.uint8)) for _ in range(self.nf)]
                          for _ in range(2)]
        d_pts, d_imgs = [], []
        for f in range(self.nf):
            c = self.sides[f % ns]
            dp, di = self.stage[cur][f]
            if n_points[f] > self.n_points_max:
                raise ValueError('frame %d has more than n_points_max points' % f)
            dp.upload_async(h_points[f], ctx=c, nbytes=16 * int(n_points[f]))
            d_pts.append(dp)
            d_imgs.append(self._stage_image(c, di, h_images[f], geoms[f]))
        return d_pts, d_imgs

    def run_from_host(self, h_points, n_points, h_images, heads=None, ego_motion=None, lookahead=None, calib=None,
                      active=None):
        """run() for raw frames still in (page-locked) host memory: lists of PinnedArray --
        points (n_max,4) float32 of which n_points[f] rows are valid, images (H,W,3) uint8.
        The copies are enqueued on each frame's side stream in front of its prep kernels, so
        they travel under the kernels of the previous step; the host does not wait for them
        (the caller keeps the pinned buffers untouched until that step's prep has run, e.g.
        by alternating two sets)."""
        if self.sequence:
            raise ValueError('run_from_host: a sequence pipeline takes push_frame_from_host()')
        la = _pad_lookahead(lookahead)
        geoms, la_geoms, active = self._check_run(h_images, heads, la, calib, host=True, active=active)
        self._check_ego(ego_motion, None if la is None else la[3])
        if self.prepped == self.step_idx:       # staged and prepared by the previous call's look-ahead
            d_pts = d_imgs = None
        else:
            d_pts, d_imgs = self._stage_from_host(self.step_idx, h_points, n_points, h_images, geoms)
        if la is not None:
            # (the copies of step k + 1 go behind what its side streams hold now, i.e. behind step k's prep)
            nd_pts, nd_imgs = self._stage_from_host(self.step_idx + 1, la[0], la[1], la[2], la_geoms)
            la = (nd_pts, la[1], nd_imgs, la[3], la_geoms)
        return self._step(self._prep, (d_pts, n_points, d_imgs, ego_motion, geoms), heads, la, None, geoms, active)

    def _prep(self, k, d_points, n_points, d_images, ego_motion, geoms, ahead):
        """a0-a7 of step k: the data side of the reference's create_feed_dict, one frame per side stream; its end
        is marked on those streams (PREP_DONE_MARK + k % 3).  `ahead`: enqueued by the previous step's run()
        (look-ahead): the conv inputs of this parity were last read by the convs of step k - 2, which the side
        streams are told to wait for (with the usual order, behind the tail of step k - 2, that is implied)."""
        cur = k & 1
        if ahead and k >= 2:
            self._wait_convs(cur)
        for f in range(self.nf):
            b, c, slot, _ = self._frame_buffers(k, f)
            self._mark(c, k, 'prep%d_start' % f)
            ego = ego_motion[f // 2] if ego_motion is not None and self.fps == 2 and f % 2 == 1 else None
            self._prep_frame(c, d_points[f], n_points[f], d_images[f], ego, self.bev_in[cur][f], self.img_in[cur][f],
                             b, slot, geoms[f])
            self._mark(c, k, 'prep%d_end' % f)
        for c in self.sides:
            c.mark(PREP_DONE_MARK + k % 3)
        self.prep_geoms[k % 3] = list(geoms)
        self.prepped = k

    def _frame_buffers(self, k, f):
        """Which buffers frame f of step k uses, for its prep and its tail alike: (what the prep leaves the tail -- occ /
        keep / count / projections / anchors --, the stream and the slot of the kept-anchor count's fetch, the frame's
        views of the feature maps).  Pair mode: the step's own, three deep (set k % 3) and by parity.  Sequence mode: the
        frame is keyframe k + f, whose set and image maps lie in the ring slots sequence_slots(k) gives it -- fetched on
        frame 1's stream, where every keyframe is prepared --, beside the step's own BEV maps."""
        ns, views = len(self.sides), self.feat_views[k & 1][f]
        if not self.sequence:
            return self.prep3[k % 3][f], self.sides[f % ns], 3 * f + k % 3, views
        slots = sequence_slots(k)
        views = dict(views, **self.img_ring_views[slots.img[f]])
        return self.prep_sets[slots.prep[f]], self.sides[1 % ns], PREP_RING * (1 % ns) + slots.prep[f], views

    def _prep_frame(self, c, d_points, n_points, d_image, ego_motion, d_bev, d_img, b, slot, g):
        """One frame's prep chain on stream c (a0-a7): BEV maps (registered by `ego_motion`, a pair's (trans, matrix), or
        None) into d_bev, the anchor filter on the un-registered grid, the fetch of its count into `slot`, the kept
        anchors' projections -- all into the set b --, and the preprocessed image into d_img; under the geometry g of the
        frame's sample."""
        bp = g.bp if ego_motion is None else ops.with_ego_motion(g.bp, *ego_motion[:2])   # (a third entry: the yaw delta)
        ops.bev_slices(c, d_points, n_points, bp, d_bev, b['occ'])
        ops.anchor_filter(c, b['occ'], self.nx, self.nz, self.d_cells, self.n_all, b['keep'], b['count'])
        ops.fetch_i32_begin(c, b['count'], 1, slot)
        self.kept_counts[slot] = None
        ops.project_anchors_f64(c, self.d_anchor_table, b['keep'], self.n_all, b['count'], self.bev_extents_flat,
                                g.p2, g.image_wh, b['bev_norm'], b['img_norm'], b['anchors'])
        ops.img_preprocess(c, d_image, (g.image_wh[1], g.image_wh[0]), (self.img_h, self.img_w), 4,
                           (self.img_net._R_MEAN, self.img_net._G_MEAN, self.img_net._B_MEAN), d_img)

    def run(self, d_points, n_points, d_images, heads=None, ego_motion=None, lookahead=None, recover=None, calib=None,
            active=None):
        """Enqueue one step.  Lists of length 2 * pairs_per_step, frame order
        [pair0 f0, pair0 f1, pair1 f0, ...]: d_points[f] (n,4) float32 velodyne xyzi;
        d_images[f] (H,W,3) uint8; heads[f] dict of device arrays rpn_logits (N,2),
        rpn_offsets (N,6), cls_logits (P,n_cls), offsets_4c (P,10), angle_vectors (P,2) (box_4ca)
        [, corr_offsets (P,3) on frame 0 of a pair]; None when the pipeline computes the heads
        itself (head_params).
        ego_motion: None, or one (trans (3,), matrix (3,3)) per pair of the step -- the
        registration of the pair's second frame into the first frame's coordinates
        (datasets.kitti.kitti_tracking_utils.coordinate_transform; applied to the second
        frame's BEV maps, not to its anchor-filter grid, like the reference).  An entry may be None (a parked ego) and
        may carry a third element, the yaw delta of coordinate_transform: the Kalman tracker's association needs it
        (a 2-tuple is refused there), every other pipeline ignores it.
        lookahead: None, or (d_points, n_points, d_images[, ego_motion[, calib]]) of the NEXT step: its prep is enqueued now,
        in front of the previous step's tail on the side streams, so that the next step's convs do not wait for
        that tail (a caller that knows its next inputs -- a stream of frames -- should pass them; the next call
        must then be made with those inputs).
        recover (pipelines built with `temporal` only): None, or per pair of the step a list of (trans (3,), matrix (3,3),
        delta) for frames 1..n_frames-1 -- the recovery of those frames' detections into their own coordinates
        (kitti_tracking_utils.recovery_coordinate).  Copied to the device behind the main stream's work so far, which
        the host waits for.
        calib: the geometry of the step's samples -- None: the constructor's calibration; one config.Calibration: every
        sample's; a list of pairs_per_step of them: one per sample (both frames of a pair share it, and d_images[f] is
        (h, w, 3) for its sample's image_wh).  It travels with the step: its prep, its tail -- enqueued by the NEXT call --,
        M and the tracker all take it, whatever the calls in between bring.  A step announced by a look-ahead must come
        with an equal calibration; with a tracker it changes only behind end_sequence().  Everything refused here is
        refused before anything is enqueued.
        active (pipelines built with tracker=dict(lanes=True) only): None -- every lane --, or one truth value per pair of
        the step: whether the pair belongs to its lane's video.  An idle lane's slot is computed like any other (records,
        M; fill it with any valid frames, such as that lane's previous pair), but its tracker state stays untouched and its
        pair numbering does not advance.  The pairs of a step may differ in calibration; lane i's changes only on its first
        active step after construction or end_sequence(lane=i).
        Returns the parity (0/1) of the record buffers this step will fill.  The
        detections of the PREVIOUS step are complete on the main stream when this returns
        (self.d_records / self.fr / self.last_anchor_counts then describe that step);
        call finish() after the last step (run(); finish() is the unpipelined form)."""
        if self.sequence:
            raise ValueError('run: a sequence pipeline takes push_frame()')
        la = _pad_lookahead(lookahead)
        geoms, la_geoms, active = self._check_run(d_images, heads, la, calib, host=False, active=active)
        self._check_ego(ego_motion, None if la is None else la[3])
        if la is not None:
            la = la[:4] + (la_geoms,)
        return self._step(self._prep, (d_points, n_points, d_images, ego_motion, geoms), heads, la, recover, geoms,
                          active)

    def _check_run(self, images, heads, la, calib, host, active=None):
        """What run() / run_from_host() refuse, before anything is enqueued.  -> the frames' geometries of this step and
        of the look-ahead's (None without one), and the step's `active` as the step record takes it (lanes: a tuple of
        bool, one per lane; None otherwise)."""
        if (heads is None) != (self.rpn_head is not None):
            raise ValueError('pass `heads` exactly when the pipeline has no head_params')
        geoms = self._step_geoms(calib)
        la_geoms = None if la is None else self._step_geoms(la[4])
        if self.prepped == self.step_idx:
            if not self._same_geoms(geoms, self.prep_geoms[self.step_idx % 3]):
                raise ValueError('calib: not the calibration the previous call announced with its look-ahead')
        elif images is not None:
            self._check_images(images, geoms, host)
        if la is not None:
            self._check_images(la[2], la_geoms, host)
        if active is not None and not self.lanes:
            raise ValueError('active: needs a pipeline built with tracker=dict(lanes=True)')
        if self.lanes:
            # (pair p of every step is lane p's: one video, one calibration per LANE until end_sequence(lane=p); an idle
            #  lane's slot may hold anything)
            active = (True,) * self.pairs if active is None else tuple(bool(a) for a in active)
            if len(active) != self.pairs:
                raise ValueError('active: one entry per lane (%d), not %d' % (self.pairs, len(active)))
            for i, on in enumerate(active):
                if on and self.track_geoms[i] not in (None, geoms[self.fps * i]):
                    raise ValueError('calib: lane %d\'s calibration changes only behind end_sequence(lane=%d)' % (i, i))
        elif self.tracker is not None:
            # (the pairs of the steps, in order, are ONE sequence until end_sequence(): one video, one calibration.  A
            #  look-ahead may already belong to the next sequence: it is checked when its step comes)
            if any(g is not geoms[0] for g in geoms) or self.track_geom not in (None, geoms[0]):
                raise ValueError('calib: with a tracker the calibration changes only behind end_sequence()')
        return geoms, la_geoms, active

    def _step(self, prep, inputs, heads, lookahead, recover, geoms, active=None):
        """The step body of run() and push_frame(): `prep`(k, points, n_points, image(s), ego_motion, geometry, ahead=)
        is the mode's prep (_prep, _seq_prep), `inputs` and the padded `lookahead` its arguments for this step and the
        next; `geoms` the geometry of every frame of this step (what its prep takes or, enqueued a call ago, took), which
        the step's record carries to its tail, M and the tracker, like `active` (lanes)."""
        main, img = self.ctx, self.img_ctx
        self._resolve_t_branch()
        self._upload_recover(recover, geoms)
        if self.lanes:
            for i, on in enumerate(active):
                if on:
                    self.track_geoms[i] = geoms[self.fps * i]
        elif self.tracker is not None:
            self.track_geom = geoms[0]
        k = self.step_idx
        cur = k & 1
        feat = self.feat[cur]
        if self.prepped != k:      # (else: enqueued by the previous call's look-ahead)
            prep(k, *inputs, ahead=False)
        for c in self.sides:
            main.wait_mark(c, PREP_DONE_MARK + k % 3)
            img.wait_mark(c, PREP_DONE_MARK + k % 3)
        # -- a8-a10: conv stacks, all frames per launch, the two nets side by side (sequence mode: the BEV stack over both
        # frames, the image stack over the new one) --------
        self._mark(main, k, 'bev_start')
        self._mark(img, k, 'img_start')
        self._grow_support(geoms)
        self.bev_net.forward_device_padded(self.in_bev[cur], feat['bev_feat'], feat['bev_bneck'])
        self._image_forward(k)
        self._mark(main, k, 'bev_end')
        self._mark(img, k, 'img_end')
        # The tail of THIS step (next call) starts when these convs are done.  The point is marked now and waited
        # for when the tail is enqueued -- behind the NEXT step's prep on the same side stream, which therefore
        # runs under these convs instead of behind them
        main.mark(CONV_DONE_MARK + cur)
        img.mark(CONV_DONE_MARK + cur)
        # Placement 'img': the T branch's correlation map needs the two frames' BEV maps and nothing else: it runs HERE,
        # behind the image stack on its stream (the shorter of the two stacks), not inside a frame's tail, whose dependent
        # launch chain -- with its prep what bounds the bf16 step -- it made 50 us longer
        if self.placement == 'img':
            img.wait_mark(main, CONV_DONE_MARK + cur)
            for pair in range(self.pairs):
                self._correlation_map(img, cur, 2 * pair, self.corr_maps[cur][pair])
            img.mark(CORR_MAP_MARK + cur)
        # -- the next step's prep, when the caller has given its inputs: in front of the previous step's tail ----
        if lookahead is not None:
            prep(k + 1, *lookahead, ahead=True)
        # -- the previous step's tail runs under this step's convs --------------------------
        self._pending_tail()
        ego = None
        if self._ego_deltas():  # (run(): one entry per pair or None; push_frame(): the new frame's entry or None)
            em = inputs[3]
            ego = [em] if self.sequence else [None] * self.pairs if em is None else list(em)
        self.pending = self._step_record(k, heads, recover is not None, geoms, active, ego)
        self.step_idx += 1
        return cur

    def _step_record(self, k, heads=None, recover=False, geoms=None, active=None, ego=None):
        """The record of step k as the call that enqueues it leaves it in `pending` (_Step)."""
        return _Step(step=k, cur=k & 1, rslot=k % len(self.rec2), heads=heads, recover=recover,
                     geoms=[self.geom0] * self.nf if geoms is None else geoms, active=active, ego=ego)

    def _image_forward(self, k):
        """The image stack of step k on the image stream: over every frame of the step into feat[k & 1]; in sequence
        mode over the step's new frame (batch 1) into its slot of the image ring.  That slot's last reader is the tail of
        step k - 2 (its frame 0), enqueued in the call before this one, whose end the image stream has been told to wait
        for (TAIL_DONE_MARK, _pending_tail); a tail finish() enqueued stands in front of this step's preps on both side
        streams, which the stream waits for in front of its stack."""
        cur = k & 1
        dst = self.img_ring[sequence_slots(k).img[1]] if self.sequence else self.feat[cur]
        self.img_net.forward_device_padded(self.in_img[cur], dst['img_feat'], dst['img_bneck'])

    # ---- sequence mode ------------------------------------------------------------------------
    def _seq_streams(self):
        """(stream of a step's frame 0: the carried keyframe's plain voxelisation and its tail, stream of its frame 1:
        every NEW keyframe's prep and its tail)."""
        return self.sides[0], self.sides[1 % len(self.sides)]

    def _seq_prep_new(self, k, d_points, n_points, d_image, ego_motion, g, host):
        """The full prep of a NEW keyframe, as frame 1 of step k, on frame 1's side stream: the chain of _prep_frame
        into the ring slots sequence_slots(k) gives it -- its BEV maps (registered by ego_motion) are the only output
        that is this step's alone; occ / keep / count / the projections / anchors and the preprocessed image also serve
        step k + 1, where the frame is frame 0.  host: the frame is in pinned host memory; its points are copied
        straight into the pipeline's point ring, which otherwise gets a device copy of the caller's array.  g: the
        keyframe's geometry, kept beside its prep set and its points for the step after this one."""
        cur, ps = k & 1, sequence_slots(k).points[1]
        c0 = self._seq_streams()[0]
        b, c, slot, _ = self._frame_buffers(k, 1)
        if n_points > self.n_points_max:
            raise ValueError('the frame has more than n_points_max points')
        # The set and the point slot were last read on frame 0's stream: by the tail of step k + 1 - PREP_RING and by the
        # plain voxelisation of step k + 1 - POINT_RING, both enqueued there a call or more ago (sequence_slots)
        c.wait_for(c0)
        if self.seq_prime_parity == cur:
            # in_img[cur] was last read by a priming push's image forward, which no tail in front of this prep waited for
            c.wait_mark(self.img_ctx, CONV_DONE_MARK + cur)
            self.seq_prime_parity = None
        d_pts = self.pts_ring[ps]
        self._mark(c, k, 'prep1_start')
        if host:
            if not hasattr(self, 'seq_img_stage'):       # (read by this stream's own preprocessing only: one buffer)
                self.seq_img_stage = self.ctx.empty((self.image_wh_max[1], self.image_wh_max[0], 3), np.uint8)
            d_pts.upload_async(d_points, ctx=c, nbytes=16 * int(n_points))
            d_image = self._stage_image(c, self.seq_img_stage, d_image, g)
            d_points = d_pts
        self._prep_frame(c, d_points, n_points, d_image, ego_motion, self.bev_in[cur][1], self.img_in[cur][0], b, slot, g)
        if not host and n_points > 0:
            ops.gather_rows(c, d_points, 4, self.d_row_ids, n_points, None, d_pts)
        self.pts_n[ps] = int(n_points)
        self.pts_geoms[ps] = self.prep_geoms[sequence_slots(k).prep[1]] = g
        self._mark(c, k, 'prep1_end')
        c.mark(PREP_DONE_MARK + k % 3)

    def _seq_prep(self, k, d_points, n_points, d_image, ego_motion, g, ahead, host):
        """The prep of sequence step k: on frame 0's stream what is left to do for the carried keyframe -- the plain,
        un-registered voxelisation of the pipeline's copy of its points into in_bev[k & 1][0]; as frame 1 of step
        k - 1 its maps were registered, everything else stands in its ring slots --, beside it on frame 1's stream the new
        frame's full prep.  `ahead`: as for _prep."""
        cur, slots = k & 1, sequence_slots(k)
        c0, c1 = self._seq_streams()
        if ahead and k >= 2:
            self._wait_convs(cur)
        # the copy of the carried frame's points was made at the end of its prep as a new frame, on frame 1's stream
        # (as frame 1 of step k - 1; that mark's next recording is the prep of step k + 2, not enqueued yet)
        self._mark(c0, k, 'prep0_start')
        if c0 is not c1:
            c0.wait_mark(c1, PREP_DONE_MARK + (k - 1) % 3)
        ps = slots.points[0]
        # (no occupancy output: the frame's grid, from the same un-registered cloud, is in its prep set)
        # (under the geometry the keyframe came with, kept beside its points)
        ops.bev_slices(c0, self.pts_ring[ps], self.pts_n[ps], self.pts_geoms[ps].bp, self.bev_in[cur][0], None)
        self._mark(c0, k, 'prep0_end')
        if c0 is not c1:
            c0.mark(PREP_DONE_MARK + k % 3)
        self._seq_prep_new(k, d_points, n_points, d_image, ego_motion, g, host)
        self.prepped = k

    def push_frame(self, d_points, n_points, d_image, heads=None, ego_motion=None, lookahead=None, recover=None,
                   calib=None):
        """Sequence mode's run(): ONE new keyframe -- d_points (n,4) float32 velodyne xyzi of which n_points rows are
        valid, d_image (H,W,3) uint8.  The first push of a sequence (after construction or end_sequence()) only primes:
        the frame is prepared, its image forward enqueued, and None returned.  Every later push enqueues the step of
        the pair (previous frame, new frame), as run() enqueues a pair, and returns the parity of its record buffers;
        the previous step's detections are then complete on the main stream, and finish() drains the last step.
        heads: as for run(), the two frames' dicts in the pair's order (injected logits are inputs: nothing of them is
        carried); ignored by a priming push.  ego_motion: None, or the (trans, matrix) that registers the new frame into
        the previous one; lookahead: None, or (d_points, n_points, d_image[, ego_motion[, calib]]) of the NEXT frame, which
        the next push must then bring; recover: as for run().  The arrays may be reused once this call's work has run: the
        pipeline voxelises the frame a second time one step later, from a copy of its own.
        calib: None (the constructor's calibration) or the Calibration of the frame's sequence: one per sequence, so it
        may differ from the current one only on a priming push."""
        return self._push(d_points, n_points, d_image, heads, ego_motion, lookahead, recover, calib, host=False)

    def push_frame_from_host(self, h_points, n_points, h_image, heads=None, ego_motion=None, lookahead=None,
                             recover=None, calib=None):
        """push_frame() for a frame still in (page-locked) host memory, PinnedArrays as for run_from_host(): the points
        are copied straight into the pipeline's point ring and the image into a staging buffer, on the new frame's side
        stream in front of its prep; the host does not wait.  A look-ahead's frame is in pinned memory too."""
        return self._push(h_points, n_points, h_image, heads, ego_motion, lookahead, recover, calib, host=True)

    def _push(self, d_points, n_points, d_image, heads, ego_motion, lookahead, recover, calib, host):
        if not self.sequence:
            raise ValueError('push_frame: the pipeline was built without sequence=True')
        img = self.img_ctx
        c0, c1 = self._seq_streams()
        la = _pad_lookahead(lookahead)
        k = self.step_idx
        # -- what is refused, before anything is enqueued: a sequence is one video, so it has one calibration ----
        g = self._step_geoms(calib)[0]
        if self.seq_primed and g is not self.seq_geom:
            raise ValueError('calib: a sequence has one calibration; it changes only on the push that begins one')
        if self.seq_primed and (heads is None) != (self.rpn_head is not None):
            raise ValueError('pass `heads` exactly when the pipeline has no head_params')
        self._check_ego([ego_motion] if self.seq_primed else None, None if la is None else [la[3]])
        if self.prepped != k or not self.seq_primed:         # (else: prepared, and checked, by the previous call)
            self._check_images([d_image], [g], host)
        if la is not None:
            if self._step_geoms(la[4])[0] is not g:
                raise ValueError('calib: the look-ahead frame belongs to the same sequence, its calibration differs')
            self._check_images([la[2]], [g], host)
            la = la[:4] + (g,)

        def prep(k, *inputs, ahead):
            self._seq_prep(k, *inputs, ahead=ahead, host=host)
        if not self.seq_primed:
            self.seq_geom = g
            # the frame is prepared as if it were frame 1 of step k - 1: every buffer it writes is that step's, whose
            # readers a finished sequence has left behind (end_sequence() follows finish()); its image forward is marked
            # as that step's image stack
            self._seq_prep_new(k - 1, d_points, n_points, d_image, None, g, host)
            img.wait_mark(c1, PREP_DONE_MARK + (k - 1) % 3)
            img.wait_for(c0)                            # (the last sequence's tails, frame 0's, read the image ring too)
            self._mark(img, k - 1, 'img_start')
            self._image_forward(k - 1)
            self._mark(img, k - 1, 'img_end')
            img.mark(CONV_DONE_MARK + ((k - 1) & 1))
            self.seq_primed, self.seq_prime_parity = True, (k - 1) & 1
            if la is not None:
                prep(k, *la, ahead=True)
            return None
        return self._step(prep, (d_points, n_points, d_image, ego_motion, g), heads, la, recover, [g, g])

    @staticmethod
    def _mixed(geoms):
        """The pairs of a step differ in calibration (M then takes one row per pair)."""
        return any(x is not geoms[0] for x in geoms)

    def _upload_recover(self, recover, geoms):
        """The step's recovery parameters for M (run()'s `recover`), into the slot of the step about to be enqueued; with
        them, when its pairs differ in calibration, M's 42 doubles per pair."""
        if recover is None:
            return
        if self.temporal is None:
            raise ValueError('recover: the pipeline has no temporal module')
        if len(recover) != self.pairs:
            raise ValueError('recover: one entry per pair of the step')
        n = self.temporal['n_frames']
        # slot k % R was last read by M of step k - R, enqueued on `main` before this copy
        self.ego2[self.step_idx % len(self.rec2)].upload(np.stack([ops.temporal_ego(e, n) for e in recover]))
        if self._mixed(geoms):      # (the same slot, the same ordering argument)
            self.cal2[self.step_idx % len(self.rec2)].upload(np.stack([g.temporal_rows() for g in geoms[::self.fps]]))

    def _pending_tail(self):
        """Enqueue the tail of the step before the one just enqueued, then M and the tracker over its records."""
        main, img = self.ctx, self.img_ctx
        if self.pending is not None:
            self._tail(self.pending)
            for s in self.sides:
                # one event at the tail's end, two waiters: `main` (the previous step's records are complete there, and
                # the BEV stack of the next step of that parity overwrites the maps the tail reads) and the image stream
                # (the same for the image net's maps: without look-ahead that wait is implied -- the next prep sits behind
                # the tail on the side stream and the conv streams wait for the prep --, with look-ahead the prep is in
                # front of it).  (A mark after the tail's LAST READ of the image maps instead -- its stage-2 crops -- was
                # measured: the extra event inside the tail's launch chain costs more than the earlier release returns,
                # 868 against 899 pairs/s with the bf16 path.)
                s.mark(TAIL_DONE_MARK)
                main.wait_mark(s, TAIL_DONE_MARK)
                img.wait_mark(s, TAIL_DONE_MARK)
            self._after_tail(self.pending)

    def finish(self):
        """Enqueue the tail of the last step; afterwards self.fr / d_records hold it."""
        st = self.pending
        if st is not None:
            self._tail(st)
            self.pending = None
        for s in self.sides:
            self.ctx.wait_for(s)
        self.ctx.wait_for(self.img_ctx)
        if st is not None and (self.temporal is not None or self.tracker is not None):
            self.img_ctx.wait_for(self.ctx)         # (the main stream has joined every stream, the last tails included)
            self._after_tail(st)
            self.ctx.wait_for(self.img_ctx)

    def _after_tail(self, st):
        """What reads the records of step `st` on the image stream: M, then the tracker."""
        self._temporal_step(st)
        self._tracker_step(st)

    def _temporal_step(self, st):
        """M of step `st` (pipelines built with `temporal`): one launch for all its pairs on the IMAGE stream, behind the
        next step's image stack (the shorter of the two; on the main stream, behind the BEV stack, M's 0.1 ms lengthened
        the step by 3 %).  That stream already waits for the step's tails (TAIL_DONE_MARK, _pending_tail) -- its records are
        complete there; the next writer of the record slot, the tail of step st + R, waits for the conv stacks of step
        st + R on both conv streams (CONV_DONE_MARK), i.e. behind this launch: no marks of its own.  The outputs go to
        slot st % R of the frames ring (d_frames, frames()); finish() makes the main stream wait for them."""
        if self.temporal is None:
            return
        T, r, c = self.temporal, st.rslot, self.img_ctx
        self._mark(c, st.step, 'temporal_start')
        # the recovery's calibration: the step's one, by value; pairs that differ in it (pairs_per_step > 1, samples of
        # several videos) take one row each from the slot _upload_recover filled (dodt_interpolate_pairs_calibs)
        if st.recover and self._mixed(st.geoms):
            cal = dict(d_calibs=self.cal2[r])
        else:
            cal = dict(calib=st.geoms[0].temporal_rows() if st.recover else None)
        ops.interpolate_pairs(c, self.rec2[r], self.cnt2[r], self.pairs, MAX_DET, T['n_frames'], T['threshold'],
                              T['on_conflict'], self.frames2[r], self.fcnt2[r], self.fst2[r],
                              d_recover=self.ego2[r] if st.recover else None, max_out=2 * MAX_DET, **cal)
        self._mark(c, st.step, 'temporal_end')
        self.d_frames, self.d_frame_counts, self.d_frame_status = self.frames2[r], self.fcnt2[r], self.fst2[r]

    def _tracker_step(self, st):
        """The tracker over the pairs of step `st` (pipelines built with `tracker`): three launches on the IMAGE stream,
        right behind M (or where M would be), under the same record-slot argument as _temporal_step -- the next
        writer of slot st % R, the tail of step st + R, waits for both conv streams of that step, i.e. behind these
        launches.  The state carries over to the next step; nothing is downloaded."""
        if self.tracker is None:
            return
        r, c = st.rslot, self.img_ctx
        self._mark(c, st.step, 'tracker_start')
        if self.lanes:
            # every lane's pair in one launch triple: lane i under the calibration the step brought for pair i, the idle
            # lanes of the step left as they are
            gs = st.geoms[::self.fps]
            if self.kalman or self.velocity:
                # lane p also under pair p's recovery calibration and ego entry: each lane's own motion associates that
                # lane's next keyframe (the lane objects keep it), all of it by value in the kernel arguments
                self.track_state.track_records(self.rec2[r], self.cnt2[r], MAX_DET, [g.p2 for g in gs],
                                               [g.image_wh for g in gs], st.ego or [None] * self.pairs,
                                               [g.temporal_rows() for g in gs], active=st.active, ctx=c)
                self._mark(c, st.step, 'tracker_end')
                return
            self.track_state.track_records(self.rec2[r], self.cnt2[r], MAX_DET, [g.p2 for g in gs],
                                           [g.image_wh for g in gs], active=st.active, ctx=c)
            self._mark(c, st.step, 'tracker_end')
            return
        g = st.geoms[0]        # (one per sequence, _check_run / _push)
        if self.kalman or self.velocity:
            # the same place and slot argument; each pair's own motion associates the keyframe after it (the state
            # object keeps the last one for the next step), all of it by value in the kernel arguments
            self.track_state.track_records(self.rec2[r], self.cnt2[r], self.pairs, MAX_DET, g.p2, g.image_wh,
                                           st.ego or [None] * self.pairs, g.temporal_rows(),
                                           self.tracker['score_threshold'], ctx=c)
            self._mark(c, st.step, 'tracker_end')
            return
        self.track_state.track_records(self.rec2[r], self.cnt2[r], self.pairs, MAX_DET, g.p2, g.image_wh, ctx=c)
        self._mark(c, st.step, 'tracker_end')

    def _frame_ids(self, frame_ids):
        if frame_ids is not None:
            ids = [tuple(f) for f in frame_ids]
            return lambda pair, kf: ids[pair][kf]
        tau = self.temporal['n_frames'] - 1 if self.temporal is not None else 1
        return lambda pair, kf: pair * tau + kf * tau

    def _lane(self, lane, what):
        """The Tracker a per-sequence method works on: the pipeline's one, or lane `lane` of a lanes pipeline."""
        if self.tracker is None:
            raise ValueError('%s: the pipeline has no tracker' % what)
        if not self.lanes:
            if lane is not None:
                raise ValueError('%s: lane= needs a pipeline built with tracker=dict(lanes=True)' % what)
            return self.track_state
        if lane is None or isinstance(lane, bool) or not 0 <= int(lane) < self.pairs:
            raise ValueError('%s: a lanes pipeline needs lane=0..%d' % (what, self.pairs - 1))
        return self.track_state.lane(int(lane))

    def tracks_so_far(self, frame_ids=None, lane=None):
        """The tracks the device has finished so far in this sequence, up to the last step whose tail has been enqueued
        (every step after finish()), downloaded: the host's track dicts (dt_evaluator_utils.track_through_ious on
        encode_tracking_dets of the same records).  frame_ids: None -- pair j of the sequence is frames (j * tau,
        j * tau + tau), tau = n_frames - 1 of `temporal` or 1 --, or one (frame_0, frame_1) per pair.  lane: which lane's
        sequence (lanes pipelines, where a pair's number counts the lane's own active steps)."""
        state = self._lane(lane, 'tracks_so_far')
        self.ctx.wait_for(self.img_ctx)             # (the downloads go through the main stream)
        if self.kalman:
            return self._kalman_tracks(frame_ids, None, state)
        if self.velocity:
            return self._velocity_tracks(frame_ids, None, state)
        return tracking.tracks_from_log(state.read(), self._frame_ids(frame_ids), self.tracker['classes'])

    def _kalman_stride(self):
        if self.tracker['stride'] is not None:
            return self.tracker['stride']
        return self.temporal['n_frames'] - 1 if self.temporal is not None else 1

    def _kalman_tracks(self, frame_ids, frame_total, state=None):
        """The Kalman tracker's finished tracks as kf_pipeline returns them: kalman_tracker.Tracker objects whose dets
        (dicts 'frame_id' = keyframe * stride, 'boxes3d' [h,w,l,x,y,z,ry], 'boxes2d', 'scores'; virtual ones included)
        are rebuilt from the device's log by interpolation_detections.  state: a lane's tracker (None: the pipeline's)."""
        if frame_ids is not None:
            raise ValueError("frame_ids: the Kalman tracker numbers frames keyframe * stride (tracker=dict(stride=))")
        fin, log = (state or self.track_state).read()
        tk = self.tracker
        return tracking.kf_tracks_from_log(fin, log, self._kalman_stride(), frame_total, L=tk['L'],
                                           R_scaler=tk['R_scaler'])

    def _velocity_tracks(self, frame_ids, frame_total, state=None):
        """The velocity tracker's finished tracks as interpolate_by_track returns them: dicts 'dets' (dicts 'frame_id' =
        keyframe * stride, 'info', 'boxes2d', 'boxes3d' [h,w,l,x,y,z,ry], 'score', float32; interpolated, predicted and
        extended entries included), 'direction', 'max_score', 'speed', 'extend_len', rebuilt from the device's log
        (tracking.vt_tracks_from_log).  frame_total None: the sequence ends at the last keyframe tracked."""
        if frame_ids is not None:
            raise ValueError("frame_ids: the velocity tracker numbers frames keyframe * stride (tracker=dict(stride=))")
        state = state or self.track_state           # (a lane's tracker, or the pipeline's)
        fin, log = state.read()
        stride = self._kalman_stride()
        if frame_total is None:
            frame_total = max(state.header()['keyframe'] - 1, 0) * stride + 1
        return tracking.vt_tracks_from_log(fin, log, stride, self.tracker['extend_len'], frame_total,
                                           classes=self.tracker['classes'])

    def end_sequence(self, frame_ids=None, lane=None, frame_total=None):
        """End the sequence after finish(): finish the remaining active tracks, download, and start a new sequence.
        Returns the host function's tracks_finished (kept as last_sequence_tracks for kitti_tracking_rows()).
        Sequence mode: the next push_frame() primes again, and a look-ahead that no push followed is dropped; without a
        tracker that is all (returns None).  Lanes: ends lane `lane`'s sequence alone -- its state is flushed, downloaded
        and reset, the other lanes go on --, kept as last_sequence_tracks[lane]; finish() first all the same, so ending one
        video drains the pipeline once.  Kalman tracker: the last pair's keyframe 1 is tracked as the final keyframe
        first; returns kf_pipeline's Tracker objects, frame ids keyframe * stride, a coasting track's virtual detections
        at most at frame_total - 1 (None: no clamp)."""
        if self.tracker is None and not self.sequence:
            raise ValueError('end_sequence: the pipeline has no tracker')
        if self.lanes:
            state = self._lane(lane, 'end_sequence')
            if self.pending is not None:
                raise ValueError('end_sequence: call finish() first (the last step is not tracked yet)')
            if (self.kalman or self.velocity) and frame_ids is not None:    # (refused before the lane is touched)
                raise ValueError("frame_ids: the %s tracker numbers frames keyframe * stride (tracker=dict(stride=))"
                                 % ('Kalman' if self.kalman else 'velocity'))
            lane = int(lane)
            geom = self.geom0 if self.track_geoms[lane] is None else self.track_geoms[lane]
            self.track_geoms[lane] = None           # (the lane's next video may bring another calibration)
            if self.kalman or self.velocity:
                # the lane's last pair's keyframe 1 is its final keyframe, under the lane's calibration and pending ego
                state.flush(geom.temporal_rows(), ctx=self.img_ctx)
                self.ctx.wait_for(self.img_ctx)
                tracks = (self._kalman_tracks if self.kalman else self._velocity_tracks)(frame_ids, frame_total, state)
                state.reset(ctx=self.img_ctx)
                self.last_sequence_tracks[lane] = tracks
                return tracks
            state.flush(ctx=self.img_ctx)
            tracks = self.tracks_so_far(frame_ids, lane=lane)
            state.reset(ctx=self.img_ctx)
            self.last_sequence_tracks[lane] = tracks
            return tracks
        if lane is not None:
            raise ValueError('end_sequence: lane= needs a pipeline built with tracker=dict(lanes=True)')
        if self.pending is not None:
            raise ValueError('end_sequence: call finish() first (the last step is not tracked yet)')
        geom = self.geom0 if self.track_geom is None else self.track_geom
        self.track_geom = None         # (the next sequence may bring another calibration)
        if self.sequence:
            self.seq_primed, self.prepped = False, -1
            if self.tracker is None:
                return None
        if self.kalman or self.velocity:
            # the last pair's keyframe 1 is the sequence's final keyframe, then the host function's last statements
            self.track_state.flush(geom.temporal_rows(), ctx=self.img_ctx)
            self.ctx.wait_for(self.img_ctx)
            tracks = (self._kalman_tracks if self.kalman else self._velocity_tracks)(frame_ids, frame_total)
            self.track_state.reset(ctx=self.img_ctx)
            self.last_sequence_tracks = tracks
            return tracks
        self.track_state.flush(ctx=self.img_ctx)
        tracks = self.tracks_so_far(frame_ids)
        self.track_state.reset(ctx=self.img_ctx)
        self.last_sequence_tracks = tracks
        return tracks

    def kitti_tracking_rows(self, tracks=None, lane=None):
        """convert_trajectory_to_kitti_format of `tracks` (default: the last sequence end_sequence() returned, on a lanes
        pipeline the last one of lane `lane`): the reference's KITTI tracking rows, as strings."""
        from dodt_amd.core.dt_evaluator_utils import convert_trajectory_to_kitti_format
        if tracks is None and self.tracker is not None and self.velocity:
            if self.lanes:
                self._lane(lane, 'kitti_tracking_rows')
                tracks = self.last_sequence_tracks[int(lane)]
            else:
                tracks = self.last_sequence_tracks
            if tracks is None:
                raise ValueError('kitti_tracking_rows: no sequence has ended')
        # the velocity tracker's dicts ('dets') go through its own converter (video_detection_iou.py)
        if tracks is not None and len(tracks) and isinstance(tracks[0], dict) and 'dets' in tracks[0]:
            from dodt_amd.experiments import video_detection_iou
            return video_detection_iou.convert_trajectory_to_kitti_format(tracks)
        # (the converter takes encode_tracking_dets' label items -- 'info', 'offsets', string frame ids --, which a Kalman
        #  track's detections are not)
        if tracks is not None and len(tracks) and not isinstance(tracks[0], dict):
            raise ValueError('kitti_tracking_rows: not for the Kalman tracker\'s Tracker objects (DESIGN section 8g)')
        if tracks is None:
            if self.kalman:
                raise ValueError("kitti_tracking_rows: not for tracker kind='kalman' (DESIGN section 8g)")
            if self.lanes:
                self._lane(lane, 'kitti_tracking_rows')
                tracks = self.last_sequence_tracks[int(lane)]
            else:
                tracks = None if self.tracker is None else self.last_sequence_tracks
            if tracks is None:
                raise ValueError('kitti_tracking_rows: no sequence has ended')
        return convert_trajectory_to_kitti_format(tracks)           # (a track's type is its name in cfg['classes'])

    def frames(self):
        """Every frame's detections of the last finished step (as d_records: after finish(), or of the previous step
        once run() has returned), downloaded: per pair, the host function's list of n_frames (k,13) float64 arrays
        (dt_evaluator_utils.interpolate_non_keyframe_predictions on that pair's records).  Raises ValueError if a pair
        had a conflict and on_conflict is 'raise'."""
        if self.temporal is None:
            raise ValueError('frames: the pipeline has no temporal module')
        self.ctx.wait_for(self.img_ctx)             # (the downloads go through the main stream)
        return unpack_frames(self.d_frames.download(), self.d_frame_counts.download(),
                             self.d_frame_status.download(), self.temporal['on_conflict'])

    def _wait_convs(self, cur):
        """The side streams wait for both conv stacks of the last step of parity `cur` (marked behind them, _step): in
        front of that step's tail, and of a look-ahead prep, which overwrites the conv inputs that step read."""
        for s in self.sides:
            s.wait_mark(self.ctx, CONV_DONE_MARK + cur)
            s.wait_mark(self.img_ctx, CONV_DONE_MARK + cur)

    def _tail(self, st):
        """Stages after the extractors for every frame of step `st` (a11-a14), behind its conv stacks: the per-step
        state, then the stages of its frames in the order of the T branch's placement (Schedule.t_placement)."""
        cur, nf, ns = st.cur, self.nf, len(self.sides)
        self._wait_convs(cur)
        counts, preps, feat = [], [], []
        for f in range(nf):
            b, c, slot, views = self._frame_buffers(st.step, f)
            # the frame's kept-anchor count: fetched by its prep, long complete (sequence mode: a carried frame's was
            # read by the tail of the step before)
            if self.kept_counts[slot] is None:
                self.kept_counts[slot] = ops.fetch_i32_end(c, slot, 1)[0]
            counts.append(self.kept_counts[slot])
            preps.append(b)
            feat.append(views)
        self.last_anchor_counts = counts
        self.fr = [dict(b, **p) for b, p in zip(self.fr2[cur], preps)]   # the tail's buffers + what its prep left
        self.d_records, self.d_rec_counts = self.rec2[st.rslot], self.cnt2[st.rslot]
        self.d_bev_in = self.bev_in[cur]
        if self.sched.no_tail:      # (tools/: the step without its tail)
            return
        if self.on_records_reuse is not None:
            self.on_records_reuse(st.rslot, self.sides)
        t = st._replace(fr=self.fr, feat=feat, counts=counts, heads=self.fr if st.heads is None else st.heads,
                        scratch=self.head_scratch)
        if self.placement == 'img':
            for f0 in range(0, nf, 2):
                self._pair_img(t, f0)
        elif self.placement == 'f1':
            for f0 in range(0, nf, 2):
                self._pair_f1(t, f0)
        elif self.alternate:
            # the frames of a pair are independent chains on two streams: their launches alternate stage by stage
            for f0 in range(0, nf, 2):
                for stage in (self._proposals, self._head2, self._decode_nms2, self._records):
                    stage(t, f0)
                    stage(t, f0 + 1)
        else:
            for f in range(nf):
                self._proposals(t, f)
                self._head2(t, f)
                if self.placement == 'f0' and f % 2 == 0:
                    self._t_map_crops(t, f, on=f)
                    self._mark(self.sides[f % ns], t.step, 'tail%d_corrmap' % f)
                    self._t_head(t, f, on=f)
                self._decode_nms2(t, f)
                self._records(t, f)

    def _pair_img(self, t, f0):
        """Placement 'img', pair (f0, f0 + 1).  The map stands since the convs ended (_step).  Its crops at frame 0's
        proposals and the correlation head go onto frame 1's stream, in front of that frame's own head -- frame 0's
        stream, which carried them, was the longer chain by their 0.1 ms -- and frame 0's records wait for the offsets."""
        ns = len(self.sides)
        c0, c1 = self.sides[f0 % ns], self.sides[(f0 + 1) % ns]
        self._proposals(t, f0)
        c0.mark(PROPOSALS_MARK)
        self._head2(t, f0)
        self._decode_nms2(t, f0)
        self._proposals(t, f0 + 1)
        c1.wait_mark(c0, PROPOSALS_MARK)
        c1.wait_mark(self.img_ctx, CORR_MAP_MARK + t.cur)
        self._t_crops(t, f0, f0 + 1, self.corr_maps[t.cur][f0 // 2])
        self._t_head(t, f0, on=f0 + 1)
        c1.mark(CORR_ROIS_MARK)
        c0.wait_mark(c1, CORR_ROIS_MARK)
        self._records(t, f0)
        self._head2(t, f0 + 1)
        self._decode_nms2(t, f0 + 1)
        self._records(t, f0 + 1)

    def _pair_f1(self, t, f0):
        """Placement 'f1', pair (f0, f0 + 1).  The T branch hangs on frame 0's tail, which makes it half as long again
        as frame 1's: its map and crops (not the head) go onto frame 1's stream, between that frame's own crops and
        head, and frame 0's stream waits for them in front of the correlation head."""
        ns = len(self.sides)
        c0, c1 = self.sides[f0 % ns], self.sides[(f0 + 1) % ns]
        self._proposals(t, f0)
        c0.mark(PROPOSALS_MARK)
        self._head2(t, f0)
        self._proposals(t, f0 + 1)
        c1.wait_mark(c0, PROPOSALS_MARK)
        self._t_map_crops(t, f0, on=f0 + 1)
        c1.mark(CORR_ROIS_MARK)
        self._head2(t, f0 + 1)
        self._decode_nms2(t, f0 + 1)
        self._records(t, f0 + 1)
        c0.wait_mark(c1, CORR_ROIS_MARK)
        self._mark(c0, t.step, 'tail%d_corrmap' % f0)
        self._t_head(t, f0, on=f0)
        self._decode_nms2(t, f0)
        self._records(t, f0)

    def _proposals(self, t, f):
        """Frame f up to its 7x7 crops: RPN crops, RPN head, decode, NMS #1, the kept proposals and their projections."""
        c, b, h, A, v = self.sides[f % len(self.sides)], t.fr[f], t.heads[f], t.counts[f], t.feat[f]
        g = t.geoms[f]             # (of the step the tail belongs to, not of the call that enqueues it)
        bev_hw, img_hw, FC = (self.bev_fh, self.bev_fw), (self.img_fh, self.img_fw), self.feat_c
        self._mark(c, t.step, 'tail%d_start' % f)
        # -- a11: RPN crops (3x3 on the 1-channel bottlenecks) ------------------------
        ops.crop_and_resize(c, v['bev_bneck'], bev_hw + (1,), b['bev_norm'], A, None, (3, 3), b['rpn_bev_roi'])
        ops.crop_and_resize(c, v['img_bneck'], img_hw + (1,), b['img_norm'], A, None, (3, 3), b['rpn_img_roi'])
        self._mark(c, t.step, 'tail%d_crops' % f)
        if self.rpn_head is not None and not self.sched.no_rpn:      # (no_rpn: tools/' timing experiment)
            self.rpn_head.forward(c, b['rpn_bev_roi'], b['rpn_img_roi'], A, b['rpn_logits'],
                                  b['rpn_offsets'], t.scratch[f % len(self.sides)]['rpn'])
        self._mark(c, t.step, 'tail%d_rpn' % f)
        # -- a12, a5, a13: decode, project, NMS #1; stage 2: the kept proposals and their projections ---------
        # (the elementwise runs of a frame's launch chain are one launch each -- rpn_decode, gather_project, final_decode
        #  below: the same arithmetic value for value, six launches fewer per frame; DODT_PIPE_FUSED_TAIL=0: the separate ops)
        if self.sched.fused_tail:
            ops.rpn_decode(c, b['anchors'], h['rpn_offsets'], h['rpn_logits'], A, None, self.bev_extents_flat,
                           b['regressed'], b['prop_bev'], b['scores'])
        else:
            ops.offset_to_anchor(c, b['anchors'], h['rpn_offsets'], A, None, b['regressed'])
            ops.project_anchors_f32(c, b['regressed'], A, None, self.bev_extents_flat, g.p2,
                                    g.image_wh, d_bev_norm_tf=b['prop_bev'])
            ops.softmax_fg(c, h['rpn_logits'], A, None, b['scores'])
        ops.nms(c, b['prop_bev'], b['scores'], A, None, self.P, self.cfg['rpn_nms_iou_thresh'], b['top_idx'], b['top_count'])
        if self.sched.fused_tail:
            ops.gather_project(c, b['regressed'], b['top_idx'], self.P, b['top_count'], self.bev_extents_flat,
                               g.p2, g.image_wh, b['top_anchors'], b['top_bev'], b['top_img'])
            self._mark(c, t.step, 'tail%d_nms1' % f)
        else:
            ops.gather_rows(c, b['regressed'], 6, b['top_idx'], self.P, b['top_count'], b['top_anchors'])
            self._mark(c, t.step, 'tail%d_nms1' % f)
            ops.project_anchors_f32(c, b['top_anchors'], self.P, b['top_count'], self.bev_extents_flat, g.p2,
                                    g.image_wh, d_bev_norm_tf=b['top_bev'], d_img_norm_tf=b['top_img'])
        ops.crop_and_resize(c, v['bev_feat'], bev_hw + (FC,), b['top_bev'], self.P, b['top_count'], (ROI, ROI),
                            b['bev_rois'])
        ops.crop_and_resize(c, v['img_feat'], img_hw + (FC,), b['top_img'], self.P, b['top_count'], (ROI, ROI),
                            b['img_rois'])

    def _head2(self, t, f):
        """Frame f's stage-2 head on its 7x7 crops (computed heads)."""
        c, b = self.sides[f % len(self.sides)], t.fr[f]
        self._mark(c, t.step, 'tail%d_crops2' % f)
        if self.rpn_head is not None:
            self.avod_head.forward(c, b['bev_rois'], b['img_rois'], self.P, b['top_count'],
                                   [b['cls_logits'], b['offsets_4c']] + ([b['angle_vectors']] if self.box_4ca else []),
                                   t.scratch[f % len(self.sides)]['fc'])
            self._mark(c, t.step, 'tail%d_fc2' % f)

    def _correlation_map(self, c, cur, f0, d_map):
        """The correlation map of pair (f0, f0 + 1) from the BEV feature maps of parity `cur`, on context c."""
        v = self.feat_views[cur]
        ops.correlation(c, v[f0]['bev_feat'], v[f0 + 1]['bev_feat'], (self.bev_fh, self.bev_fw, self.feat_c),
                        CORR_MAX_DISP, CORR_STRIDE2, CORR_PAD, d_map)

    def _t_crops(self, t, f0, on, d_map):
        """T branch ('proposals' form): 7x7 crops of the pair's map at frame f0's proposals, on frame `on`'s stream
        (dt_rpn_model.py:324-331, dt_avod_model.py:267-273,300-304)."""
        b = t.fr[f0]
        ops.crop_and_resize(self.sides[on % len(self.sides)], d_map, (self.bev_fh, self.bev_fw, CORR_CH), b['top_bev'],
                            self.P, b['top_count'], (ROI, ROI), b['corr_rois'], out_box_stride=self.corr_head.in_ld)

    def _t_map_crops(self, t, f0, on):
        """... the map in that stream's scratch first."""
        i = on % len(self.sides)
        self._correlation_map(self.sides[i], t.cur, f0, t.scratch[i]['corr_map'])
        self._t_crops(t, f0, on, t.scratch[i]['corr_map'])

    def _t_head(self, t, f0, on):
        """... the correlation head on those crops, on frame `on`'s stream with its scratch."""
        i, b = on % len(self.sides), t.fr[f0]
        self.corr_head.forward(self.sides[i], b['corr_rois'], None, self.P, b['top_count'], [b['corr_offsets']],
                               t.scratch[i]['fc'])

    def _decode_nms2(self, t, f):
        """a14, a13 of frame f: box_4c decode, NMS #2."""
        c, b, h, plane = self.sides[f % len(self.sides)], t.fr[f], t.heads[f], self.cfg['ground_plane']
        self._mark(c, t.step, 'tail%d_heads' % f)
        # record score = softmax over [background, class] (dt_evaluator.py:1226-1248)
        # box_4ca: all_orientations = atan2 of the angle vectors (dt_avod_model.py:547-548),
        # gathered with the boxes by NMS #2's indices (:631-634) inside the record kernel,
        # which applies the evaluator's heading correction (dt_evaluator.py:1166-1212)
        # several classes: NMS #2 stays class-agnostic on the largest non-background logit (dt_avod_model.py:606); score
        # and type come from the n_cls-way softmax (dt_evaluator.py:1226-1255), through the *_classes entries, which
        # take the column count behind the logits and the types behind the scores
        if self.n_cls > 2:
            decode, scores, n_cls, types = ops.final_decode_classes, ops.class_scores, (self.n_cls,), (b['det_types'],)
        else:
            decode, scores, n_cls, types = ops.final_decode, ops.softmax_fg, (), ()
        fused = self.sched.fused_tail
        if fused:
            decode(c, b['top_anchors'], h['offsets_4c'], h['cls_logits'], *n_cls,
                   h['angle_vectors'] if self.box_4ca else None, self.P, b['top_count'], plane,
                   self.bev_extents_flat, b['boxes_3d'], b['pred_anchors'], b['nms2_boxes'],
                   b['nms2_scores'], b['det_scores'], *types, b['orientations'] if self.box_4ca else None)
        else:
            ops.box_4c_decode(c, b['top_anchors'], h['offsets_4c'], self.P, b['top_count'],
                              plane, self.bev_extents_flat, b['boxes_3d'], b['pred_anchors'], b['nms2_boxes'])
            ops.max_fg_logit(c, h['cls_logits'], self.n_cls, self.P, b['top_count'], b['nms2_scores'])
        ops.nms(c, b['nms2_boxes'], b['nms2_scores'], self.P, b['top_count'], MAX_DET,
                self.cfg['avod_nms_iou_thresh'], b['det_idx'], b['det_count'])
        if not fused:
            scores(c, h['cls_logits'], *n_cls, self.P, b['top_count'], b['det_scores'], *types)
            if self.box_4ca:
                ops.angle_vector_to_orientation(c, h['angle_vectors'], self.P, b['top_count'], b['orientations'])

    def _records(self, t, f):
        """Frame f's detection records; in the 'detections' form, behind the T branch of its pair on frame 0."""
        c, b = self.sides[f % len(self.sides)], t.fr[f]
        frame0 = self.fps == 2 and f % 2 == 0
        d_rec = self.d_records.offset(4 * MAX_DET * REC_COLS * f, (MAX_DET, REC_COLS))
        d_cnt = self.d_rec_counts.offset(4 * f, (1,), np.int32)
        d_orient = b['orientations'] if self.box_4ca else None
        # (one class: the two-way entries, column 8 is 0; several: the same kernel with every box's type)
        if self.n_cls > 2:
            types, pack, pack_compact = (b['det_types'],), ops.pack_detections_classes, ops.pack_detections_compact_classes
        else:
            types, pack, pack_compact = (), ops.pack_detections, ops.pack_detections_compact
        if frame0 and self._t_detections():
            if self.placement == 'detections':
                self._t_detection_rows(t, f)
            # (placement 'none', DODT_PIPE_NO_CORR: the offsets stay the zeros they were made as)
            pack_compact(c, b['boxes_3d'], b['det_scores'], *types, b['det_idx'], b['det_count'], MAX_DET,
                         float(f % self.fps), d_rec, d_cnt, d_det_offsets=b['det_corr_offsets'], d_orientations=d_orient)
        else:
            pack(c, b['boxes_3d'], b['det_scores'], *types, b['det_idx'], b['det_count'], MAX_DET,
                 float(f % self.fps), d_rec, d_cnt,
                 d_corr_offsets=t.heads[f].get('corr_offsets') if frame0 else None, d_orientations=d_orient)
        self._mark(c, t.step, 'tail%d_end' % f)

    def _t_detection_rows(self, t, f):
        """T branch for the boxes NMS #2 kept of frame f (placement 'detections'): the tiles of the correlation map their
        crops can read, the map at those tiles, the crops at top_bev[det_idx], the correlation head at MAX_DET rows (the
        same GEMM kernels as at P rows: the same sums); the records read row j of the offsets for box det_idx[j]."""
        i = f % len(self.sides)
        c, b, scratch, v = self.sides[i], t.fr[f], t.scratch[i], t.feat
        bev_hw, FC = (self.bev_fh, self.bev_fw), self.feat_c
        ops.correlation_tile_list(c, bev_hw, b['top_bev'], self.P, b['det_idx'], MAX_DET, b['det_count'],
                                  (ROI, ROI), scratch['corr_tiles'], self.corr_tile_cap, scratch['corr_ntiles'])
        ops.correlation_tiles(c, v[f]['bev_feat'], v[f + 1]['bev_feat'], bev_hw + (FC,), CORR_MAX_DISP, CORR_STRIDE2,
                              CORR_PAD, scratch['corr_tiles'], self.corr_tile_cap, scratch['corr_ntiles'],
                              scratch['corr_map'])
        self._mark(c, t.step, 'tail%d_corrmap' % f)
        ops.crop_and_resize_indexed(c, scratch['corr_map'], bev_hw + (CORR_CH,), b['top_bev'], self.P,
                                    b['det_idx'], MAX_DET, b['det_count'], (ROI, ROI),
                                    b['det_corr_rois'], out_box_stride=self.corr_head.in_ld)
        self.corr_head.forward(c, b['det_corr_rois'], None, MAX_DET, b['det_count'],
                               [b['det_corr_offsets']], scratch['fc'])

    def sync(self):
        self.ctx.sync()

    def flops_per_step(self):
        """Conv stacks only (the roofline kernel); see head_flops_per_step."""
        return self.bev_net.flops() + self.img_net.flops()

    def mfma_flops_per_step(self):
        """FLOPs the matrix pipe executes for the two conv stacks (Winograd layers count 16/36)."""
        return self.bev_net.mfma_flops() + self.img_net.mfma_flops()

    def conv_bytes_per_step(self):
        """Algorithmic HBM bytes of the two conv stacks per step."""
        return self.bev_net.bytes() + self.img_net.bytes()

    def head_flops_per_step(self, anchor_counts=None):
        if self.rpn_head is None:
            return 0.0
        counts = anchor_counts or self.last_anchor_counts
        return (sum(self.rpn_head.flops(a) for a in counts)
                + self.nf * self.avod_head.flops(self.P)
                + (self.pairs * self.corr_head.flops(MAX_DET if self._t_detections() else self.P)
                   if self.corr_head else 0.0))

    def flops_per_pair(self):
        return self.flops_per_step() / self.pairs

    def close(self):
        self.bev_net.close()
        self.img_net.close()
        for hd in (self.rpn_head, self.avod_head, self.corr_head):
            if hd is not None:
                hd.close()
