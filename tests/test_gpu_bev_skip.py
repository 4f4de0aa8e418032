"""The fp32 BEV net with skip tables (dodt_extractor_set_input_support): the BEV cells outside the camera's frustum
are zero in every frame, so the tiles whose receptive field holds only such cells are left out once a full forward
has written them.  Everything the net writes must stay bit-identical to full tables: every layer buffer, the feature
map and the bottleneck, after a weight reload too, and the pipeline's records over free-running steps."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from dodt_amd import config, device, ops, synth
from dodt_amd.core.feature_extractors.vgg_pyramid import BevVggPyr
from dodt_amd.pipeline import FramePairPipeline

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
LAYERS = ('conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2',
          'conv4_3', 'upconv3', 'pyramid_fusion3', 'upconv2', 'pyramid_fusion2', 'upconv1')
PAD = BevVggPyr.PAD_TOP
H, W = C['bev_dims']


def _bev_params(p2=synth.P2, r0=synth.R0_RECT, tr=synth.TR_VELO_TO_CAM, imwh=synth.IMAGE_WH):
    return ops.make_bev_params(C, config.velo_to_cam(np.asarray(r0, np.float64), np.asarray(tr, np.float64)),
                               np.asarray(p2, np.float64), tuple(imwh))


def _bev_maps(ctx, clouds, bp, ego=None):
    """(len(clouds), PAD + H, W, 6) device input in the extractor's padded layout, from dodt_bev_slices."""
    x = ctx.zeros((len(clouds), PAD + H, W, C['bev_depth']), np.float32)
    frame = (PAD + H) * W * C['bev_depth']
    d_pts = [ctx.array(np.ascontiguousarray(pts, np.float32)) for pts in clouds]
    for f, pts in enumerate(clouds):
        b = bp if ego is None or ego[f] is None else ops.with_ego_motion(bp, *ego[f])
        view = x.offset(4 * (f * frame + PAD * W * C['bev_depth']), (H, W, C['bev_depth']))
        ops.bev_slices(ctx, d_pts[f], len(pts), b, view)
    ctx.sync()
    return x


def _nets(ctx, batch, params, mask):
    nets = []
    for m in (mask, None):
        ex = BevVggPyr(ctx=ctx, shared_gpu=True)
        ex.load_params(params)
        ex._ensure(batch, H, W, C['bev_depth'])
        skipped = ex.set_input_support(m)
        assert (skipped > 0) == (m is not None)
        nets.append(ex)
    return nets


def _outputs(ctx, ex, x, feat, bneck):
    ex.forward_device_padded(x, feat, bneck)
    ctx.sync()
    out = {n: ex.activation(n) for n in LAYERS}
    out['feat'] = feat.download().copy()
    out['bneck'] = bneck.download().copy()
    return out


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), '%s: %s differs' % (what, k)


def _check_sequence(ctx, inputs, bp, params=None, reload=None):
    """inputs: device inputs of one batch size; the skip net primes on the first and skips on the rest.  reload:
    other weights loaded into both nets before the last input (the skip net must re-prime)."""
    params = params or synth.pyramid_params(C['bev_depth'])
    batch = inputs[0].shape[0]
    on, off = _nets(ctx, batch, params, ops.bev_support_mask(bp, PAD))
    outs = [ctx.empty((batch, H, W, 32), np.float32), ctx.empty((batch, H, W, 1), np.float32)]
    ref = [ctx.empty((batch, H, W, 32), np.float32), ctx.empty((batch, H, W, 1), np.float32)]
    for i, x in enumerate(inputs):
        if reload is not None and i == len(inputs) - 1:
            on.load_params(reload)
            off.load_params(reload)
        _assert_same(_outputs(ctx, on, x, *outs), _outputs(ctx, off, x, *ref), 'input %d' % i)
    return on


def test_skip_tables_drop_items_and_account_for_them():
    ctx = device.default_context()
    bp = _bev_params()
    x = _bev_maps(ctx, [synth.lidar_frame(3, f) for f in (0, 2)], bp)
    on, off = _nets(ctx, 2, synth.pyramid_params(C['bev_depth']), ops.bev_support_mask(bp, PAD))
    feat, bneck = ctx.empty((2, H, W, 32), np.float32), ctx.empty((2, H, W, 1), np.float32)
    for ex in (on, off):
        ex.set_input(x)            # (forward_timed takes no padded input: the nets read x in place)
    full = off.forward_timed(None, feat, bneck)
    first = on.forward_timed(None, feat, bneck)      # priming: full tables
    steady = on.forward_timed(None, feat, bneck)
    assert [l['items'] for l in first] == [l['items'] for l in full]
    for a, b in zip(steady, full):
        assert 0 < a['items'] <= b['items'], a['name']
        # (shared-GPU nets: one launch per layer, items of one size)
        assert abs(a['flops_executed'] / b['flops_executed'] - a['items'] / b['items']) < 1e-9, a['name']
    dropped = sum(b['items'] - a['items'] for a, b in zip(steady, full))
    assert dropped > 0.15 * sum(b['items'] for b in full)
    assert on.mfma_flops() < 0.9 * off.mfma_flops()
    assert on.flops() < 0.9 * off.flops()
    # the native propagation against the numpy one (tests/test_bev_support_mask.py), at each kernel's own tiles:
    # kept items = full items x the share of tiles with an input-dependent output (frames, channel tiles alike)
    if ctx.lib.dodt_conv_mode() != 2:
        return                     # (other conv forms tile differently; F(4x4) also reaches by blocks)
    from tests import test_bev_support_mask as geom
    masks = geom.layer_masks(ops.bev_support_mask(bp, PAD))
    tile = {'conv3x3_small_cin_kernel': (16, 32), 'wino3x3_f32_kernel': (16, 16), 'deconv3x3_dma_kernel': (32, 32)}
    for a, b in zip(steady, full):
        reached, tiles = geom.tiles_reached(masks[a['name']], *tile[b['kernel']])
        assert b['items'] % (2 * tiles) == 0, (a['name'], b['items'], tiles)
        assert a['items'] == b['items'] // tiles * reached, (a['name'], a['items'], b['items'], reached, tiles)


def test_each_output_pair_is_primed_before_it_is_skipped_into():
    """pyramid_fusion1 writes the caller's buffers, so every (feature, bottleneck) pair needs a full-table pass of its
    own before that layer may skip into it.  Eleven pairs -- more than the eight the extractor remembers --, some
    without a bottleneck, visited in an order that reuses remembered, forgotten and new pairs.  Every buffer starts as
    NaN: a skip into a pair that was never written leaves NaN in it."""
    ctx = device.default_context()
    bp = _bev_params()
    inputs = [_bev_maps(ctx, [synth.lidar_frame(s, 1)], bp) for s in (30, 31, 32)]
    on, off = _nets(ctx, 1, synth.pyramid_params(C['bev_depth']), ops.bev_support_mask(bp, PAD))

    def nan_buffer(c):
        a = ctx.empty((1, H, W, c), np.float32)
        assert ctx.lib.dodt_memset(ctx.handle, a.ptr, 0xFF, a.nbytes) == 0
        return a

    pairs = [(nan_buffer(32), nan_buffer(1) if k % 3 else None) for k in range(11)]
    ref = (ctx.empty((1, H, W, 32), np.float32), ctx.empty((1, H, W, 1), np.float32))
    ctx.sync()
    for i, k in enumerate([0, 1, 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 1, 10, 0, 5, 9, 2]):
        x = inputs[i % len(inputs)]
        feat, bneck = pairs[k]
        on.forward_device_padded(x, feat, bneck)
        off.forward_device_padded(x, *ref)
        ctx.sync()
        assert np.array_equal(feat.download().view(np.uint32), ref[0].download().view(np.uint32)), (i, k)
        if bneck is not None:
            assert np.array_equal(bneck.download().view(np.uint32), ref[1].download().view(np.uint32)), (i, k)


def test_synthetic_frames_bit_equal():
    ctx = device.default_context()
    bp = _bev_params()
    inputs = [_bev_maps(ctx, [synth.lidar_frame(s, f) for f in (0, 2)], bp) for s in (5, 6, 7)]
    _check_sequence(ctx, inputs, bp)


def test_golden_clouds_bit_equal():
    """The real clouds of the fixtures, each with its own calibration."""
    ctx = device.default_context()
    g = np.load(os.path.join(GOLDEN, 'frames.npz'))
    names = sorted({k[:-5] for k in g.files if k.endswith('_xyzi')})
    for name in names:
        bp = _bev_params(g[name + '_p2'], g[name + '_r0'], g[name + '_tr'], g[name + '_imwh'])
        other = synth.lidar_frame(9, 0)
        inputs = [_bev_maps(ctx, [other, other], bp), _bev_maps(ctx, [g[name + '_xyzi'], other], bp),
                  _bev_maps(ctx, [other, g[name + '_xyzi']], bp)]
        _check_sequence(ctx, inputs, bp)


def test_ego_motion_frame_bit_equal():
    ctx = device.default_context()
    e = np.load(os.path.join(GOLDEN, 'egomotion.npz'))
    bp = _bev_params(e['p2'], e['r0'], e['tr'], e['imwh'])
    ego = [None, (e['trans'], e['matrix'])]
    inputs = [_bev_maps(ctx, [synth.lidar_frame(4, 0)] * 2, bp),
              _bev_maps(ctx, [e['xyzi'], e['xyzi']], bp, ego=ego)]
    _check_sequence(ctx, inputs, bp)


def test_weight_reload_reprimes():
    ctx = device.default_context()
    bp = _bev_params()
    inputs = [_bev_maps(ctx, [synth.lidar_frame(s, f) for f in (0, 2)], bp) for s in (11, 12)]
    other = synth.pyramid_params(C['bev_depth'])
    rng = np.random.default_rng(1)
    for p in other.values():       # new weights and batch-norm shifts: the input-independent values change
        p['w'] = (p['w'] * rng.uniform(0.5, 1.5, size=p['w'].shape)).astype(np.float32)
        p['beta'] = (p['beta'] + rng.uniform(-0.1, 0.1, size=p['beta'].shape)).astype(np.float32)
    _check_sequence(ctx, inputs, bp, reload=other)


def _pipeline_steps(ctx, pipe, steps):
    recs, bev, keep = [], [], []     # (the inputs stay alive until the end: the streams read them behind the host)
    for k in range(steps + 1):
        if k < steps:
            seq, frames = 20 + k % 3, (k % 4, k % 4 + 2)
            pts = [synth.lidar_frame(seq, f) for f in frames]
            imgs = [ctx.array(synth.image_frame(seq, f)) for f in frames]
            heads = [{n: ctx.array(v) for n, v in synth.head_outputs(seq, f, pipe.n_all, pipe.P).items()}
                     for f in frames]
            keep.append(([ctx.array(p) for p in pts], imgs, heads))
            pipe.run(keep[-1][0], [len(p) for p in pts], imgs, heads)
        else:
            pipe.finish()
        ctx.sync()
        if k > 0:       # the previous step's records are complete
            recs.append((pipe.d_records.download().copy(), pipe.d_rec_counts.download().copy()))
        if k < steps:   # this step's BEV feature map and bottleneck (its parity's buffers), as digests
            feat = pipe.feat[(pipe.step_idx - 1) & 1]
            bev.append(tuple(hashlib.sha256(feat[n].download().tobytes()).hexdigest() for n in ('bev_feat', 'bev_bneck')))
    return recs, bev


def test_pipeline_bev_outputs_and_records_bit_equal_free_running():
    """Seven free-running steps: both parities of the double-buffered inputs and of bev_feat / bev_bneck (each parity
    pair primed by its own first step), fresh inputs each step.  The BEV feature map and bottleneck of every step are
    compared bit for bit (the records with injected heads do not read the skipped tiles), and the records too."""
    ctx = device.default_context()
    on = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024)
    assert on.bev_skipped_items > 0
    a, a_bev = _pipeline_steps(ctx, on, 7)
    del on
    off = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024, bev_input_skip=False)
    assert off.bev_skipped_items == 0
    b, b_bev = _pipeline_steps(ctx, off, 7)
    assert len(a_bev) == 7 and a_bev == b_bev
    for k, ((ra, ca), (rb, cb)) in enumerate(zip(a, b)):
        assert np.array_equal(ca, cb), k
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), k


@pytest.mark.parametrize('mode', ['0', '4'])
def test_other_conv_forms_in_child_process(mode):
    """DODT_CONV_WINO is read once per process: the direct kernels (0) and F(4x4,3x3) (4) in children."""
    env = dict(os.environ, DODT_CONV_WINO=mode)
    code = ('import sys; sys.path.insert(0, %r); import tests.test_gpu_bev_skip as t; '
            't.test_synthetic_frames_bit_equal(); t.test_weight_reload_reprimes(); '
            't.test_each_output_pair_is_primed_before_it_is_skipped_into(); print("ok")' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
