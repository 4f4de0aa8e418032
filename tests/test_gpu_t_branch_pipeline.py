"""FramePairPipeline's two forms of the T branch -- every proposal's rows, or the kept detections' only -- give the same
records, bit for bit, and the default picks the form by where the records go.  Needs an MI355X."""
import numpy as np
import pytest

from dodt_amd import config, device, ops, synth
from dodt_amd.pipeline import CORR_CH, MAX_DET, REC_COLS, ROI, FramePairPipeline

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
STEPS = 3           # both parities of every double-buffered set are used again


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


@pytest.fixture(scope='module')
def frames(ctx):
    """Two seeded pairs, resident on the device: (points, counts, images) per frame."""
    out = []
    for seq, f in ((3, 0), (3, 2), (5, 1), (5, 3)):
        p = synth.lidar_frame(seq, f)
        out.append((ctx.array(p), len(p), ctx.array(synth.image_frame(seq, f))))
    return out


def _run(ctx, frames, pairs, made, ring=False, **kw):
    """STEPS consecutive steps over the same `pairs` pairs; the records and counts of every step."""
    pipe = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), head_params=synth.head_params(),
                             pairs_per_step=pairs, reuse_streams_of=made[0] if made else None, **kw)
    made.append(pipe)
    if ring:
        pipe.rings = (ctx.zeros((4, pairs, 2, MAX_DET, REC_COLS), np.float32), ctx.zeros((4, pairs, 2), np.int32))
        pipe.use_record_ring(*pipe.rings)
    fr = frames[:2 * pairs]
    d_pts, n, d_imgs = [f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr]
    got = []
    for k in range(STEPS):
        pipe.run(d_pts, n, d_imgs)
        if k > 0:
            ctx.sync()
            got.append((pipe.d_records.download().copy(), pipe.d_rec_counts.download().copy()))
    pipe.finish()
    ctx.sync()
    got.append((pipe.d_records.download().copy(), pipe.d_rec_counts.download().copy()))
    return pipe, got


def _same(a, b):
    assert len(a) == len(b) == STEPS
    for k, ((rec_a, n_a), (rec_b, n_b)) in enumerate(zip(a, b)):
        assert np.array_equal(n_a, n_b), k
        assert np.array_equal(rec_a, rec_b), k


def _three_forms(ctx, frames, pairs, **kw):
    made = []
    p_prop, prop = _run(ctx, frames, pairs, made, t_branch_rows='proposals', **kw)
    p_det, det = _run(ctx, frames, pairs, made, t_branch_rows='detections', **kw)
    p_ring, ring = _run(ctx, frames, pairs, made, ring=True, **kw)
    forms = (p_prop.t_branch_form(), p_det.t_branch_form(), p_ring.t_branch_form())
    assert forms == ('proposals', 'detections', 'detections')
    counts = prop[-1][1]
    assert counts.shape == (pairs, 2) and counts.min() > 0
    assert np.abs(prop[-1][0][:, 0, :, 9:16]).max() > 0          # frame 0's shifted boxes are there
    _same(prop, det)
    _same(prop, ring)
    assert p_det.head_flops_per_step() < p_prop.head_flops_per_step()
    return made, prop


def test_records_equal_in_every_form_and_default_follows_the_records(ctx, frames):
    made, prop = _three_forms(ctx, frames, 1)
    # a default pipeline that keeps its own records: the per-proposal form, whose inspection buffers hold every row
    p_def, rec = _run(ctx, frames, 1, made)
    assert p_def.t_branch_form() == 'proposals'
    b, d = p_def.fr[0], made[1].fr[0]
    n_top, n_det = int(b['top_count'].download()[0]), int(b['det_count'].download()[0])
    assert n_top > MAX_DET >= n_det > 0
    offs, rois = b['corr_offsets'].download(), b['corr_rois'].download()
    assert offs.shape == (p_def.P, 3) and np.isfinite(offs[:n_top]).all() and np.abs(rois[:n_top]).max() > 0
    # every proposal's row is there: more rows are filled than the detections form computes at all (a crop is all zeros
    # where the map is -- outside it, or where both frames' BEV features are empty -- so not every row is non-zero) ...
    assert (np.abs(rois[:n_top]).max(1) > 0).sum() > MAX_DET
    # ... and each row, the zero ones included, is the crop of the pair's full map at that proposal
    full = ctx.zeros(rois.shape, np.float32)
    ops.crop_and_resize(ctx, p_def.corr_maps[0][0], (p_def.bev_fh, p_def.bev_fw, CORR_CH), b['top_bev'], p_def.P,
                        b['top_count'], (ROI, ROI), full, out_box_stride=rois.shape[1])
    ctx.sync()
    assert np.array_equal(full.download()[:n_top], rois[:n_top])
    # ... and the detections form's rows are those rows, gathered by NMS #2's indices
    det_idx = d['det_idx'].download()[:n_det]
    assert np.array_equal(det_idx, b['det_idx'].download()[:n_det])
    assert np.array_equal(d['det_corr_offsets'].download()[:n_det], offs[det_idx])
    assert np.array_equal(d['det_corr_rois'].download()[:n_det], rois[det_idx])
    _same(rec, prop)
    for p in made:
        p.close()


def test_records_equal_with_two_pairs_per_step(ctx, frames):
    for p in _three_forms(ctx, frames, 2)[0]:
        p.close()


def test_records_equal_with_bf16_convs_and_heads(ctx, frames):
    for p in _three_forms(ctx, frames, 1, conv_dtype='bf16', head_dtype='bf16')[0]:
        p.close()


def test_records_equal_with_one_side_stream(ctx, frames):
    """side_streams=1: both frames' preps and tails on one stream, one frame after the other, and the whole T branch
    (map, crops, correlation head) between frame 0's stage-2 head and its decode on that stream (placement 'f0')."""
    p_two, two = _run(ctx, frames, 1, [], t_branch_rows='proposals')
    p_one, one = _run(ctx, frames, 1, [], t_branch_rows='proposals', side_streams=1)      # (streams of its own)
    assert len(p_two.sides) == 2 and p_two.placement == 'img'
    assert len(p_one.sides) == 1 and p_one.placement == 'f0' and p_one.t_branch_form() == 'proposals'
    counts = two[-1][1]
    assert counts.shape == (1, 2) and counts.min() > 0
    assert np.abs(one[-1][0][:, 0, :, 9:16]).max() > 0           # frame 0's shifted boxes are there
    _same(two, one)
    for p in (p_two, p_one):
        p.close()
