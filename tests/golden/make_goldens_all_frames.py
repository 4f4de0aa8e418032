#!/usr/bin/env python3
"""Digests of the reference's point path on EVERY real cloud its tests bundle, and the inputs of
a fixed selection of them.

Run:  python tests/golden/make_goldens_all_frames.py
      (needs /root/reference; writes all_frames.json and real_clouds_*.npz; about five minutes)

For each of the 63 bundled clouds (13 object frames, 50 tracking frames in four sequences) the
reference's own numpy code is run exactly as run_frame() of make_goldens.py runs it, and for each
of the 42 pairs (k, k + 2) whose clouds and OXTS lines exist exactly as make_goldens_egomotion.py
runs it: BEV maps of the (registered) cloud, anchor-filter occupancy of the cloud as read, keep
mask over the anchor grid, normalised BEV / image projections of ALL kept anchors.  What is stored
per record is data only: identity, calibration numbers, counts and SHA-1 digests (recipe in
tests/_real_clouds.py); for pairs also (trans, matrix, delta) and the two OXTS text lines.

The oracle runs beside the reference on every record (`oracle_equal`), and the reference runs once
more on the "FOV + margin" subset of the cloud (`subset_equal`, rows in original order; see
_real_clouds.margin_mask); the script exits non-zero if either ever differs.  Only subsets are
shipped, for the selection in _real_clouds.SHIPPED_FRAMES / SHIPPED_PAIRS, at full resolution.

Both outputs are reproducible byte for byte: sorted keys, fixed order, and a zip writer with a
fixed time stamp (np.savez_compressed stamps each member with the wall clock).
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root
import make_goldens as mg  # noqa: E402
import make_goldens_box4ca as mb  # noqa: E402
import _real_clouds as rc  # noqa: E402

KITTI = rc.REFERENCE_KITTI
MAX_FILE = 1 << 20          # no fixture file above 1 MiB
MAX_TOTAL = 5 * 10 ** 6
PER_FILE = {'frames': 3, 'pairs': 2}


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member order and time stamp."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    mb.import_evaluator()            # tensorflow / tensorflow.contrib / cv2 stand-ins
    from avod.datasets.kitti.kitti_tracking_dataset import KittiTrackingDataset as DS
    from avod.core.bev_generators.bev_slices import BevSlices
    from avod.core import anchor_projector, box_3d_encoder, anchor_filter
    from avod.core.anchor_generators import grid_anchor_3d_generator
    from wavedata.tools.core import calib_utils
    from wavedata.tools.core.voxel_grid_2d import VoxelGrid2D
    from wavedata.tools.obj_detection import obj_utils, tracking_utils

    ku = types.SimpleNamespace(area_extents=mg.AREA_EXTENTS, voxel_size=mg.VOXEL_SIZE)
    ku.create_slice_filter = lambda pc, ext, plane, lo, hi: np.logical_xor(
        obj_utils.get_point_filter(pc, ext, plane, hi), obj_utils.get_point_filter(pc, ext, plane, lo))
    bev_gen = BevSlices(mg._Cfg(), ku)
    plane = np.asarray([0, -1, 0, 1.65]) / np.linalg.norm([0, -1, 0])
    boxes = grid_anchor_3d_generator.tile_anchors_3d(mg.AREA_EXTENTS, mg.CAR_CLUSTERS,
                                                     mg.ANCHOR_STRIDE, plane)
    anchors = box_3d_encoder.box_3d_to_anchor(boxes)
    assert np.array_equal(anchors, rc.anchor_grid())

    def maps_and_anchors(cloud, raw_cloud, p2, im_wh):
        """(3,N) camera-view clouds -> the outputs dict _real_clouds.digests() reads."""
        bev = bev_gen.generate_bev('lidar', cloud, plane, mg.AREA_EXTENTS, mg.VOXEL_SIZE)
        sf = ku.create_slice_filter(raw_cloud, mg.AREA_EXTENTS, plane, 0.2, 2.0)
        vg = VoxelGrid2D()
        vg.voxelize_2d(raw_cloud.T[sf], mg.VOXEL_SIZE, extents=mg.AREA_EXTENTS,
                       ground_plane=plane, create_leaf_layout=True)
        keep = anchor_filter.get_empty_anchor_filter_2d(anchors, vg, 1)
        kept = anchors[keep]
        _, bev_n = anchor_projector.project_to_bev(kept, mg.BEV_EXTENTS)
        _, img_n = anchor_projector.project_to_image_space(kept, p2, [im_wh[1], im_wh[0]])
        return dict(n_fov=cloud.shape[1],
                    stack=np.dstack(bev['height_maps'] + [bev['density_map']]),
                    occ=(np.squeeze(vg.leaf_layout_2d) + 1).astype(bool), keep=keep,
                    bev_norm=bev_n, img_norm=img_n)

    def ref_frame(xyzi, calib, im_wh):
        """run_frame() of make_goldens.py."""
        pts = calib_utils.lidar_to_cam_frame(xyzi[:, :3], calib)
        ptsf = pts[pts[:, 2] > 0]
        uv = calib_utils.project_to_image(ptsf.T, p=calib.p2).T
        imf = (uv[:, 0] > 0) & (uv[:, 0] < im_wh[0]) & (uv[:, 1] > 0) & (uv[:, 1] < im_wh[1])
        cloud = ptsf[imf].T
        return maps_and_anchors(cloud, cloud, calib.p2, im_wh)

    def ref_pair(ds, names, xyzi1, calib, im_wh):
        """main() of make_goldens_egomotion.py on the second frame's (N,4) cloud."""
        raw1 = np.ascontiguousarray(xyzi1.T).copy()
        warped = DS.point_cloud_transform(ds, [None, raw1], names)[1]
        assert warped.dtype == np.float32
        cloud = tracking_utils.get_lidar_in_camera_view(warped, names[1], ds.calib_dir,
                                                        im_size=list(im_wh))
        un = tracking_utils.get_lidar_in_camera_view(np.ascontiguousarray(xyzi1.T), names[1],
                                                     ds.calib_dir, im_size=list(im_wh))
        out = maps_and_anchors(cloud, un, calib.p2, im_wh)
        out['n_fov_unwarped'] = un.shape[1]
        return out

    def load(split, video, frame):
        d = os.path.join(KITTI, split)
        if video is None:
            calib = calib_utils.read_calibration(d + '/calib', frame)
            png = d + '/image_2/%06d.png' % frame
        else:
            calib = calib_utils.read_tracking_calibration(d + '/calib', video)
            png = d + '/image_2/%04d/%06d.png' % (video, frame)
        xyzi = np.fromfile(rc.bin_path(KITTI, split, video, frame), dtype=np.float32).reshape(-1, 4)
        return xyzi, calib, mg.png_size(png)

    def calib_fields(calib, im_wh):
        return dict(p2=np.asarray(calib.p2, np.float64).tolist(),
                    r0_rect=np.asarray(calib.r0_rect, np.float64).tolist(),
                    tr_velodyne_to_cam=np.asarray(calib.tr_velodyne_to_cam, np.float64).tolist(),
                    w=int(im_wh[0]), h=int(im_wh[1]))

    # ---- what is bundled ------------------------------------------------------------------------
    frames = []
    for split in ('object/training', 'tracking/training', 'tracking/testing'):
        velo = os.path.join(KITTI, split, 'velodyne')
        if split.startswith('object'):
            frames += [(split, None, int(f[:6])) for f in sorted(os.listdir(velo))]
        else:
            for v in sorted(os.listdir(velo)):
                frames += [(split, int(v), int(f[:6])) for f in sorted(os.listdir(velo + '/' + v))]
    have = set(frames)
    pairs = [(s, v, f, f + 2) for (s, v, f) in frames if v is not None and (s, v, f + 2) in have]

    ok = True
    shipped = {'frames': {}, 'pairs': {}}
    doc = {'frames': [], 'pairs': []}

    def finish(rec, want, sub, out_oracle, out_sub):
        nonlocal ok
        rec.update(want)
        rec['oracle_equal'] = rc.digests(out_oracle) == want
        rec['subset_equal'] = rc.digests(out_sub) == want
        rec['n_subset'] = int(len(sub))
        ok = ok and rec['oracle_equal'] and rec['subset_equal']
        print(rec['tag'], 'raw', rec['n_raw'], 'subset', rec['n_subset'], 'fov', rec['n_fov'],
              'bev nnz', rec['bev_nnz'], 'occupied', rec['occ_count'], 'anchors', rec['anchors_kept'],
              'oracle', rec['oracle_equal'], 'subset', rec['subset_equal'], flush=True)

    for split, video, frame in frames:
        xyzi, calib, im_wh = load(split, video, frame)
        tag = rc.frame_tag(split, video, frame)
        rec = dict(tag=tag, split=split, video=video, frame=frame, n_raw=int(len(xyzi)),
                   shipped=tag in rc.SHIPPED_FRAMES, **calib_fields(calib, im_wh))
        want = rc.digests(ref_frame(xyzi, calib, im_wh))
        r0, tr, p2 = calib.r0_rect, calib.tr_velodyne_to_cam, calib.p2
        sub = np.ascontiguousarray(xyzi[rc.margin_mask(xyzi, r0, tr, p2, im_wh)])
        finish(rec, want, sub, rc.oracle_outputs(xyzi, r0, tr, p2, im_wh),
               ref_frame(sub, calib, im_wh))
        doc['frames'].append(rec)
        if rec['shipped']:
            shipped['frames'][tag] = dict(xyzi=sub, p2=p2, r0=r0, tr=tr,
                                          imwh=np.asarray(im_wh, np.int32))

    for split, video, f0, f1 in pairs:
        root = os.path.join(KITTI, split)
        ds = types.SimpleNamespace(oxts_dir=root + '/oxts', calib_dir=root + '/calib',
                                   bev_source='lidar')
        ds.get_oxts = lambda n, ds=ds: DS.get_oxts(ds, n)
        ds.coordinate_transform = lambda n, ds=ds: DS.coordinate_transform(ds, n)
        names = ['%02d%04d' % (video, f0), '%02d%04d' % (video, f1)]
        trans, matrix, delta = ds.coordinate_transform(names)
        with open(root + '/oxts/%04d.txt' % video) as f:
            lines = [line.rstrip() for line in f.readlines()]
        xyzi, calib, im_wh = load(split, video, f1)
        tag = rc.pair_tag(split, video, f0, f1)
        rec = dict(tag=tag, split=split, video=video, frame=f1, frames=[f0, f1], n_raw=int(len(xyzi)),
                   shipped=tag in rc.SHIPPED_PAIRS, trans=np.asarray(trans, np.float64).tolist(),
                   matrix=np.asarray(matrix, np.float64).tolist(), delta=float(delta),
                   oxts_lines=[lines[f0], lines[f1]], **calib_fields(calib, im_wh))
        want = rc.digests(ref_pair(ds, names, xyzi, calib, im_wh))
        r0, tr, p2 = calib.r0_rect, calib.tr_velodyne_to_cam, calib.p2
        m = rc.margin_mask(xyzi, r0, tr, p2, im_wh) | \
            rc.margin_mask(xyzi, r0, tr, p2, im_wh, trans, matrix)
        sub = np.ascontiguousarray(xyzi[m])
        finish(rec, want, sub, rc.oracle_outputs(xyzi, r0, tr, p2, im_wh, trans, matrix),
               ref_pair(ds, names, sub, calib, im_wh))
        doc['pairs'].append(rec)
        if rec['shipped']:
            shipped['pairs'][tag] = dict(xyzi=sub, p2=p2, r0=r0, tr=tr,
                                         imwh=np.asarray(im_wh, np.int32),
                                         trans=np.asarray(trans, np.float64),
                                         matrix=np.asarray(matrix, np.float64),
                                         oxts_lines=np.array([lines[f0], lines[f1]]))

    assert sorted(shipped['frames']) == sorted(rc.SHIPPED_FRAMES), sorted(shipped['frames'])
    assert sorted(shipped['pairs']) == sorted(rc.SHIPPED_PAIRS), sorted(shipped['pairs'])
    with open(os.path.join(HERE, 'all_frames.json'), 'w') as f:
        json.dump(doc, f, sort_keys=True, indent=1)
        f.write('\n')

    for old in rc.npz_files(HERE):
        os.remove(old)
    total = 0
    for kind, order in (('frames', rc.SHIPPED_FRAMES), ('pairs', rc.SHIPPED_PAIRS)):
        n = PER_FILE[kind]
        for k in range(0, len(order), n):
            arrays = {}
            for tag in order[k:k + n]:
                arrays.update({tag + '_' + key: v for key, v in shipped[kind][tag].items()})
            path = os.path.join(HERE, 'real_clouds_%s_%d.npz' % (kind, k // n))
            save_npz(path, arrays)
            size = os.path.getsize(path)
            total += size
            print(os.path.basename(path), size, 'bytes', order[k:k + n])
            assert size <= MAX_FILE, '%s is %d bytes' % (path, size)
    print('all_frames.json', os.path.getsize(os.path.join(HERE, 'all_frames.json')), 'bytes;',
          'clouds', total, 'bytes')
    assert total < MAX_TOTAL, total
    if not ok:
        sys.exit('a record is not reproduced by the oracle or by the reference on the subset')


if __name__ == '__main__':
    main()
