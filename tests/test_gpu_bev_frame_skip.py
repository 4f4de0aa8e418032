"""The fp32 BEV net with per-frame skip tables (dodt_extractor_set_frame_tables): every forward filters the static
skip tables on the device by the cells that are non-zero in its own input, and re-runs the items the last forward
into the same buffer ran.  After every forward every layer buffer and both outputs must be byte-equal to a net on full
tables, and the item counts the kernels read must be |A_now u A_prev| of the numpy geometry."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dodt_amd import config, device, ops, synth
from dodt_amd.core.feature_extractors.vgg_pyramid import BevVggPyr
from dodt_amd.pipeline import FramePairPipeline
from tests import test_bev_support_mask as geom
from tests import test_gpu_bev_skip as base

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
ROOT = base.ROOT
PAD, H, W = base.PAD, base.H, base.W
NAMES = base.LAYERS + ('pyramid_fusion1',)
TILE = {'conv3x3_small_cin_kernel': (16, 32), 'wino3x3_f32_kernel': (16, 16), 'deconv3x3_dma_kernel': (32, 32)}


def _nets(ctx, batch, params, mask):
    on = BevVggPyr(ctx=ctx, shared_gpu=True)
    on.load_params(params)
    on._ensure(batch, H, W, C['bev_depth'])
    assert on.set_input_support(mask, frame_tables=True) > 0
    off = BevVggPyr(ctx=ctx, shared_gpu=True)
    off.load_params(params)
    off._ensure(batch, H, W, C['bev_depth'])
    return on, off


def _tiles(out, th, tw):
    h, w = out.shape
    ty, tx = -(-h // th), -(-w // tw)
    p = np.zeros((ty * th, tx * tw), bool)
    p[:h, :w] = out
    return p.reshape(ty, th, tx, tw).any(axis=(1, 3))


class _Model:
    """The extractor's bookkeeping restated: which forwards run full tables, and the item sets they leave behind."""

    def __init__(self, static_mask, full_layers, batch):
        self.static = geom.layer_masks(static_mask)
        self.tile = {l['name']: TILE[l['kernel']] for l in full_layers}
        self.static_tiles = {n: _tiles(self.static[n], *self.tile[n]) for n in NAMES}
        # channel tiles per pixel tile: full items = frames x tiles x channel tiles
        self.nt = {l['name']: l['items'] // (batch * self.static_tiles[l['name']].size) for l in full_layers}
        self.reset()

    def reset(self):
        self.primed, self.prev, self.pairs = False, {}, []

    def forward(self, x_host, pair):
        """x_host: (batch, PAD + H, W, 6) input.  Returns the expected dodt_extractor_frame_items."""
        now = {n: [] for n in NAMES}
        for f in range(len(x_host)):
            m = geom.layer_masks(np.any(x_host[f] != 0, axis=2))
            for n in NAMES:
                now[n].append(_tiles(m[n], *self.tile[n]) & self.static_tiles[n])
        now = {n: np.stack(v) for n, v in now.items()}
        known = [k for k, (p, _) in enumerate(self.pairs) if p == pair]
        want = []
        for n in NAMES:
            last = n == 'pyramid_fusion1'
            prev = (self.pairs[known[0]][1] if known else False) if last else self.prev.get(n, False)
            runs = self.primed and (not last or bool(known))
            want.append(int((now[n] | prev).sum()) * self.nt[n] if runs else -1)   # (-1: a full table ran)
            if not last:
                self.prev[n] = now[n]
        if known:
            self.pairs[known[0]] = (pair, now['pyramid_fusion1'])
        else:
            self.pairs.append((pair, now['pyramid_fusion1']))
            self.pairs = self.pairs[-8:]
        self.primed = True
        return want


def _zero_input(ctx, batch):
    return ctx.zeros((batch, PAD + H, W, C['bev_depth']), np.float32)


def _run_sequence(check_counts):
    ctx = device.default_context()
    bp = base._bev_params()
    mask = ops.bev_support_mask(bp, PAD)
    params = synth.pyramid_params(C['bev_depth'])
    on, off = _nets(ctx, 2, params, mask)
    if ctx.lib.dodt_conv_mode() == 4:
        assert not on.frame_tables_on          # F(4x4) reaches block-wise: the static tables stay
    else:
        assert on.frame_tables_on
    dense = [synth.lidar_frame(40, 0), synth.lidar_frame(41, 2)]
    sparse = [synth.lidar_frame(42, 1, n_points=4000), synth.lidar_frame(43, 3, n_points=1500, n_boxes=2)]
    other = [synth.lidar_frame(44, 0, n_points=60000), synth.lidar_frame(45, 1)]
    inputs = {'dense': base._bev_maps(ctx, dense, bp), 'sparse': base._bev_maps(ctx, sparse, bp),
              'empty': _zero_input(ctx, 2), 'mixed': base._bev_maps(ctx, [dense[0], sparse[1]], bp),
              'other': base._bev_maps(ctx, other, bp)}
    host = {k: v.download() for k, v in inputs.items()}
    pairs = [(ctx.empty((2, H, W, 32), np.float32), ctx.empty((2, H, W, 1), np.float32)) for _ in range(9)]
    ref = (ctx.empty((2, H, W, 32), np.float32), ctx.empty((2, H, W, 1), np.float32))
    reload = synth.pyramid_params(C['bev_depth'], seed=77)
    model = None
    if check_counts and on.frame_tables_on and ctx.lib.dodt_conv_mode() == 2:
        off.set_input(inputs['dense'])
        model = _Model(mask, off.forward_timed(None, *ref), 2)
        off.set_input(None)
    # (input, output pair); 'reload' loads other weights into both nets.  Pairs 0 .. 7 are remembered, pair 8 evicts
    # pair 0, which is primed again when it comes back; pair 1 is reused with sparser and denser inputs in between.
    steps = [('dense', 0), ('sparse', 0), ('empty', 0), ('dense', 0), ('mixed', 1), ('sparse', 1), ('other', 0),
             'reload', ('dense', 1), ('empty', 1), ('sparse', 2), ('other', 3), ('mixed', 4), ('sparse', 5),
             ('dense', 6), ('empty', 7), ('other', 8), ('sparse', 0), ('dense', 1), ('empty', 8), ('mixed', 0)]
    n_forwards = 0
    for i, step in enumerate(steps):
        if step == 'reload':
            on.load_params(reload)
            off.load_params(reload)
            if model:
                model.reset()
            continue
        name, k = step
        got = base._outputs(ctx, on, inputs[name], *pairs[k])
        want = base._outputs(ctx, off, inputs[name], *ref)
        base._assert_same(got, want, 'step %d (%s into pair %d)' % (i, name, k))
        if model:
            items = on.frame_items()
            expect = model.forward(host[name], k)
            print('step %2d %-6s pair %d items %s' % (i, name, k, items))
            assert items == expect, (i, step, list(zip(NAMES, items, expect)))
        n_forwards += 1
    assert n_forwards >= 8
    if model:      # not vacuous: a sparse frame behind a sparse frame runs a small part of the static tables
        on.forward_device_padded(inputs['sparse'], *pairs[0])
        on.forward_device_padded(inputs['sparse'], *pairs[0])
        items = on.frame_items()
        full = [int(model.static_tiles[n].sum()) * 2 * model.nt[n] for n in NAMES]
        assert 0 < items[1] < 0.5 * full[1] and 0 < items[3] < 0.5 * full[3], (items, full)
        assert on.mfma_flops() < 0.7 * off.mfma_flops()


def test_sequence_bit_equal_and_item_counts():
    _run_sequence(True)


@pytest.mark.parametrize('mode', ['0', '4'])
def test_other_conv_forms_in_child_process(mode):
    """DODT_CONV_WINO is read once per process: the direct kernels (0) take per-frame tables too, F(4x4,3x3) (4)
    stays on its static tables; both byte-equal to full tables over the same sequence."""
    env = dict(os.environ, DODT_CONV_WINO=mode)
    code = ('import sys; sys.path.insert(0, %r); import tests.test_gpu_bev_frame_skip as t; '
            't._run_sequence(False); print("ok")' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_pipeline_records_and_bev_maps_bit_equal_free_running():
    """Seven free-running steps with fresh inputs, both parities of the output buffers: per-frame tables against the
    static tables alone."""
    ctx = device.default_context()
    on = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024)
    assert on.bev_net.frame_tables_on
    a, a_bev = base._pipeline_steps(ctx, on, 7)
    items = on.bev_net.frame_items()
    assert all(n >= 0 for n in items), items
    del on
    off = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024, bev_frame_tables=False)
    assert not off.bev_net.frame_tables_on and off.bev_skipped_items > 0
    b, b_bev = base._pipeline_steps(ctx, off, 7)
    assert len(a_bev) == 7 and a_bev == b_bev
    for k, ((ra, ca), (rb, cb)) in enumerate(zip(a, b)):
        assert np.array_equal(ca, cb), k
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), k
