"""The native pieces of the T branch at the kept detections only (FramePairPipeline(t_branch_rows='detections')):
the crop with a row index, the record kernel with one row of offsets per detection, the correlation over a
device-built tile list, and the correlation head at MAX_DET rows.  Each is compared bit for bit with the form it
replaces.  Needs an MI355X."""
import functools

import numpy as np
import pytest

from _corr_cases import coords as _coords, curve as _curve, expected_tiles as _expected_tiles
from dodt_amd import device, ops, synth
from dodt_amd.core.avod_fc_layers.fusion_fc_layers import EarlyFusionFcLayers
from dodt_amd.pipeline import CORR_CH, CORR_MAX_DISP, CORR_PAD, CORR_STRIDE2, MAX_DET, REC_COLS, ROI

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
IN_LD = 1248            # the correlation head's padded row: 7 * 7 * 25 = 1225 floats and 23 zeros


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


def _count(ctx, n):
    return ctx.array(np.array([n], i32))


# ---- crop with a row index ------------------------------------------------------------------------------------------
def _crop_boxes():
    """13 boxes [y1, x1, y2, x2]: inside, partly and wholly outside, degenerate (y1 == y2), the whole map."""
    rng = np.random.default_rng(11)
    b = rng.uniform(0.05, 0.6, size=(13, 4)).astype(f32)
    b[:, 2:] = b[:, :2] + rng.uniform(0.05, 0.35, size=(13, 2)).astype(f32)
    b[1] = [-0.3, 0.2, 0.4, 0.7]          # reaches out above
    b[2] = [0.5, 0.6, 1.4, 1.3]           # ... below and to the right
    b[3] = [1.2, 1.1, 1.6, 1.5]           # wholly outside
    b[4] = [-0.9, -0.8, -0.2, -0.1]       # wholly outside, negative
    b[5] = [0.37, 0.2, 0.37, 0.8]         # degenerate: y1 == y2
    b[6] = [0.0, 0.0, 1.0, 1.0]           # the whole map
    return b


@pytest.fixture(scope='module')
def crop_case(ctx):
    rng = np.random.default_rng(12)
    img = rng.normal(size=(37, 45, CORR_CH)).astype(f32)
    boxes = _crop_boxes()
    idx = np.array([6, 3, 3, 0, 12, 5, 1, 6, 2, 4, 11, 0, 7, 8, 9, 10], i32)      # capacity 16, with repeats
    d_img = ctx.array(img)
    d_ref = ctx.empty((16, ROI, ROI, CORR_CH), f32)
    ops.crop_and_resize(ctx, d_img, img.shape, ctx.array(boxes[idx]), 16, None, (ROI, ROI), d_ref)
    ref = d_ref.download().reshape(16, -1)
    assert np.abs(ref).max() > 0 and not ref[1].any() and ref[5].any()
    return d_img, img.shape, ctx.array(boxes), ctx.array(idx), ref


@pytest.mark.parametrize('count', [0, 1, 7])
def test_indexed_crop_equals_crop_of_gathered_boxes(ctx, crop_case, count):
    d_img, hwc, d_boxes, d_idx, ref = crop_case
    k = ROI * ROI * CORR_CH
    before = np.full((16, IN_LD), -7.5, f32)
    before[:, k:] = 0.0
    d_out = ctx.array(before)
    ops.crop_and_resize_indexed(ctx, d_img, hwc, d_boxes, 13, d_idx, 16, _count(ctx, count), (ROI, ROI), d_out,
                                out_box_stride=IN_LD)
    got = d_out.download()
    assert np.array_equal(got[:count, :k], ref[:count])
    assert not got[:, k:].any()                                 # the row tails stay zero
    assert np.array_equal(got[count:], before[count:])          # rows past the count are untouched


# ---- record kernel with compact offsets -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pack_case(ctx):
    rng = np.random.default_rng(21)
    P = 256
    boxes = rng.normal(size=(P, 7)).astype(f32) * 5
    scores = rng.uniform(size=P).astype(f32)
    ori = rng.uniform(-np.pi, np.pi, size=P).astype(f32)
    corr = rng.normal(size=(P, 3)).astype(f32)
    sel = rng.permutation(P)[:MAX_DET].astype(i32)
    return dict(boxes=ctx.array(boxes), scores=ctx.array(scores), ori=ctx.array(ori), corr=ctx.array(corr),
                sel=ctx.array(sel), compact=ctx.array(corr[sel]))


@pytest.mark.parametrize('frame', [0, 1])
@pytest.mark.parametrize('count', [0, 1, MAX_DET])
def test_compact_records_equal_scattered_records(ctx, pack_case, count, frame):
    c = pack_case
    out = []
    for fn, off in ((ops.pack_detections, dict(d_corr_offsets=c['corr'] if frame == 0 else None)),
                    (ops.pack_detections_compact, dict(d_det_offsets=c['compact'] if frame == 0 else None))):
        d_rec = ctx.array(np.full((MAX_DET, REC_COLS), np.nan, f32))
        d_cnt = ctx.array(np.array([-1], i32))
        fn(ctx, c['boxes'], c['scores'], c['sel'], _count(ctx, count), MAX_DET, float(frame), d_rec, d_cnt,
           d_orientations=c['ori'], **off)
        out.append((d_rec.download(), d_cnt.download()))
    (want, want_n), (got, got_n) = out
    assert want_n[0] == count and np.array_equal(got_n, want_n)
    assert np.array_equal(got, want)
    if count:
        assert want[:count, 9:16].any() == (frame == 0)         # frame 1's offset columns are zeros
        assert np.all(want[:count, 16] == frame)


# ---- correlation over a tile list ----------------------------------------------------------------------------------
CH, CW = 40, 56            # 3 x 4 tiles of 16 x 16, the last row and column 8 pixels


@pytest.fixture(scope='module')
def corr_case(ctx):
    rng = np.random.default_rng(31)
    a = rng.normal(size=(CH, CW, 32)).astype(f32)
    b = rng.normal(size=(CH, CW, 32)).astype(f32)
    d_a, d_b = ctx.array(a), ctx.array(b)
    d_full = ctx.array(np.full((CH, CW, CORR_CH), np.nan, f32))
    ops.correlation(ctx, d_a, d_b, a.shape, CORR_MAX_DISP, CORR_STRIDE2, CORR_PAD, d_full)
    full = d_full.download()
    assert np.isfinite(full).all()
    return d_a, d_b, a.shape, d_full, full


def _partial(ctx, corr_case, d_tiles, cap, d_n):
    d_a, d_b, hwc, _, _ = corr_case
    d_out = ctx.array(np.full((CH, CW, CORR_CH), np.nan, f32))
    ops.correlation_tiles(ctx, d_a, d_b, hwc, CORR_MAX_DISP, CORR_STRIDE2, CORR_PAD, d_tiles, cap, d_n, d_out)
    return d_out


def _tile_mask(tiles):
    m = np.zeros((CH, CW), bool)
    for ty, tx in tiles:
        m[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = True
    return m


def test_listed_tiles_are_bit_equal_and_nothing_else_is_written(ctx, corr_case):
    full = corr_case[4]
    tiles = [(0, 0), (2, 3), (1, 1), (0, 3), (2, 0), (1, 2)]          # corners, borders, the middle
    n = 5                                                              # the sixth entry is beyond the device's count
    cap = ops.correlation_tile_capacity((CH, CW))
    assert cap == 12
    lst = np.full(cap, (1 << 16) | 2, i32)
    lst[:len(tiles)] = [ty << 16 | tx for ty, tx in tiles]
    got = _partial(ctx, corr_case, ctx.array(lst), cap, _count(ctx, n)).download()
    m = _tile_mask(tiles[:n])
    assert np.array_equal(got[m], full[m])
    assert np.isnan(got[~m]).all()


def _neighbours(v, k=40):
    """The 2k + 1 float32 values around v."""
    up, dn = [f32(v)], [f32(v)]
    for _ in range(k):
        up.append(np.nextafter(up[-1], f32(4.0)))
        dn.append(np.nextafter(dn[-1], f32(-4.0)))
    return np.array(dn[:0:-1] + up, f32)


def _edge_with_sample_at(target, size, sample):
    """(lo, hi) of a box edge pair whose sample `sample` of 7 lies exactly at pixel coordinate `target`: searched among
    the float32 neighbours of an edge pair eight pixels apart around it, with crop_coord's float32 arithmetic."""
    target, m1 = f32(target), f32(size - 1)
    first = float(target) - sample * 8.0 / (ROI - 1)
    lo = _neighbours(first / (size - 1))[:, None]
    hi = _neighbours((first + 8.0) / (size - 1))[None, :]
    step = ((hi - lo) * m1) / f32(ROI - 1)
    c = lo * m1 + f32(sample) * step
    assert c.dtype == f32
    hit = np.argwhere(c == target)
    assert len(hit), 'no box edge found with a sample at %r' % target
    i, j = hit[0]
    return lo[i, 0], hi[0, j]


@functools.lru_cache(maxsize=None)
def _seam_boxes():
    """Boxes whose sample coordinates lie exactly on tile seams -- pixel 15.0, 16.0 and the float just below 16 -- on
    either axis, boxes reaching outside the map, one wholly outside, one covering all of it."""
    below16 = np.nextafter(f32(16.0), f32(0.0))
    boxes = []
    for target in (f32(15.0), f32(16.0), below16):
        ylo, yhi = _edge_with_sample_at(target, CH, 3)
        xlo, xhi = _edge_with_sample_at(target, CW, 2)
        assert target in _coords(ylo, yhi, CH) and target in _coords(xlo, xhi, CW)
        boxes.append([ylo, 0.55, yhi, 0.8])
        boxes.append([0.1, xlo, 0.3, xhi])
        boxes.append([ylo, xlo, yhi, xhi])
    # a degenerate box: all seven rows at one coordinate near the seam
    ylo, _ = _edge_with_sample_at(f32(16.0), CH, 0)
    boxes.append([ylo, 0.2, ylo, 0.6])
    boxes += [[-0.2, 0.3, 0.3, 0.7], [0.6, 0.7, 1.3, 1.2], [1.3, 1.2, 1.8, 1.9], [0.0, 0.0, 1.0, 1.0]]
    return np.array(boxes, f32)


@pytest.mark.parametrize('case', ['seams', 'each', 'count0', 'count1'])
def test_crops_of_the_listed_map_equal_crops_of_the_full_map(ctx, corr_case, case):
    d_full, full = corr_case[3], corr_case[4]
    boxes = _seam_boxes()
    nb = len(boxes)
    runs = {'seams': [np.arange(nb)[::-1]], 'each': [np.array([j]) for j in range(nb)],
            'count0': [np.arange(nb)], 'count1': [np.arange(nb)]}[case]
    d_boxes = ctx.array(boxes)
    cap = ops.correlation_tile_capacity((CH, CW))
    for idx in runs:
        count = {'count0': 0, 'count1': 1}.get(case, len(idx))
        d_idx, d_n = ctx.array(idx.astype(i32)), _count(ctx, count)
        d_tiles, d_nt = ctx.array(np.full(cap, -1, i32)), ctx.array(np.array([-1], i32))
        ops.correlation_tile_list(ctx, (CH, CW), d_boxes, nb, d_idx, len(idx), d_n, (ROI, ROI), d_tiles, cap, d_nt)
        nt = int(d_nt.download()[0])
        tiles = [(int(t) >> 16, int(t) & 0xffff) for t in d_tiles.download()[:nt]]
        want = _expected_tiles(boxes[idx[:count]], CH, CW)
        assert tiles == [t for t in _curve(3, 4) if t in want], (case, idx)
        d_part = _partial(ctx, corr_case, d_tiles, cap, d_nt)
        part = d_part.download()
        m = _tile_mask(tiles)
        assert np.array_equal(part[m], full[m]) and np.isnan(part[~m]).all()
        outs = []
        for d_map in (d_full, d_part):
            d_out = ctx.array(np.full((nb, IN_LD), -7.5, f32))
            ops.crop_and_resize_indexed(ctx, d_map, (CH, CW, CORR_CH), d_boxes, nb, d_idx, len(idx), d_n, (ROI, ROI),
                                        d_out, out_box_stride=IN_LD)
            outs.append(d_out.download())
        assert np.isfinite(outs[0]).all()
        assert np.array_equal(outs[1], outs[0]), (case, idx)
        if case == 'seams':
            assert 0 < nt and np.abs(outs[0][:count, :ROI * ROI * CORR_CH]).max() > 0


def test_tile_list_follows_the_full_maps_order_across_blocks(ctx):
    """A 150 x 200 map: 10 x 13 tiles, two block rows and columns, ragged ones: the list is the full map's walking
    order restricted to the flagged tiles."""
    oh, ow = 150, 200
    rng = np.random.default_rng(41)
    boxes = rng.uniform(0.0, 0.8, size=(24, 4)).astype(f32)
    boxes[:, 2:] = boxes[:, :2] + rng.uniform(0.02, 0.25, size=(24, 2)).astype(f32)
    cap = ops.correlation_tile_capacity((oh, ow))
    assert cap == 130
    d_tiles, d_nt = ctx.array(np.full(cap, -1, i32)), ctx.array(np.array([-1], i32))
    ops.correlation_tile_list(ctx, (oh, ow), ctx.array(boxes), 24, None, 24, None, (ROI, ROI), d_tiles, cap, d_nt)
    nt = int(d_nt.download()[0])
    tiles = [(int(t) >> 16, int(t) & 0xffff) for t in d_tiles.download()[:nt]]
    want = _expected_tiles(boxes, oh, ow)
    assert 0 < len(want) < cap
    assert tiles == [t for t in _curve(10, 13) if t in want]


# ---- correlation head at the detections' rows ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def head_rows():
    rng = np.random.default_rng(51)
    x = np.zeros((1024, IN_LD), f32)
    x[:, :ROI * ROI * CORR_CH] = rng.normal(size=(1024, ROI * ROI * CORR_CH)).astype(f32)
    return x, rng.permutation(1024)[:MAX_DET]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_head_at_detection_rows_equals_rows_of_the_full_head(ctx, head_rows, dtype):
    """The GEMM kernels are chosen by the layer, not by M (launch_fc_dma: fc_dma_kernel<false, 1> below 512 tiles; the
    bf16 rows' fc_bf16_dma_kernel and the skinny output layer at any M), and a row's sums do not depend on the rows
    beside it: bit-equal for both arithmetics."""
    x, idx = head_rows
    head = EarlyFusionFcLayers(ctx, synth.head_params()['corr'], outputs=('off_out',), dtype=dtype)
    assert head.in_ld == IN_LD
    scratch = head.make_scratch(1024)
    d_full = ctx.array(np.full((1024, 3), np.nan, f32))
    head.forward(ctx, ctx.array(x), None, 1024, _count(ctx, 1024), [d_full], scratch)
    full = d_full.download()
    assert np.isfinite(full).all() and np.abs(full).max() > 0
    d_x = ctx.array(x[idx])
    for count in (0, 37, MAX_DET):
        d_y = ctx.array(np.full((MAX_DET, 3), np.nan, f32))
        head.forward(ctx, d_x, None, MAX_DET, _count(ctx, count), [d_y], scratch)
        assert np.array_equal(d_y.download()[:count], full[idx[:count]]), (dtype, count)
    head.close()
