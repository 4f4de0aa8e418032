"""The fp32 BEV net restores stale tiles by copy (per-frame tables, dodt_extractor_set_frame_tables): a forward computes
the items its input reaches, and the items the last forward into the same buffer reached go back to the values of a
constants store, the output of a forward on zeros.  The store must equal a full-table net fed zeros, every layer
buffer and both outputs must stay byte-equal to a net on full tables over a sequence of forwards, and the split the
extractor reports must be |A_now| and |A_prev \\ A_now| of the numpy geometry."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dodt_amd import config, device, ops, synth
from dodt_amd.core.feature_extractors.vgg_pyramid import BevVggPyr
from dodt_amd.pipeline import FramePairPipeline
from tests import test_bev_skip_soundness as sound
from tests import test_gpu_bev_frame_skip as fs
from tests import test_gpu_bev_skip as base

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
ROOT = base.ROOT
PAD, H, W = base.PAD, base.H, base.W
NAMES = fs.NAMES


class _Model(fs._Model):
    """The bookkeeping of tests/test_gpu_bev_frame_skip.py with the split: per layer (computed, restored) items."""

    def forward(self, x_host, pair):
        now = {n: [] for n in NAMES}
        for f in range(len(x_host)):
            m = fs.geom.layer_masks(np.any(x_host[f] != 0, axis=2))
            for n in NAMES:
                now[n].append(fs._tiles(m[n], *self.tile[n]) & self.static_tiles[n])
        now = {n: np.stack(v) for n, v in now.items()}
        known = [k for k, (p, _) in enumerate(self.pairs) if p == pair]
        computed, restored = [], []
        for n in NAMES:
            last = n == 'pyramid_fusion1'
            prev = (self.pairs[known[0]][1] if known else False) if last else self.prev.get(n, False)
            runs = self.primed and (not last or bool(known))
            computed.append(int(now[n].sum()) * self.nt[n] if runs else -1)
            restored.append(int((prev & ~now[n]).sum()) * self.nt[n] if runs else -1)
            if not last:
                self.prev[n] = now[n]
        if known:
            self.pairs[known[0]] = (pair, now['pyramid_fusion1'])
        else:
            self.pairs.append((pair, now['pyramid_fusion1']))
            self.pairs = self.pairs[-8:]
        self.primed = True
        return computed, restored


def _inputs(ctx, bp):
    dense = [synth.lidar_frame(40, 0), synth.lidar_frame(41, 2)]
    sparse = [synth.lidar_frame(42, 1, n_points=4000), synth.lidar_frame(43, 3, n_points=4000)]
    return {'dense': base._bev_maps(ctx, dense, bp), 'sparse': base._bev_maps(ctx, sparse, bp),
            'empty': fs._zero_input(ctx, 2), 'mixed': base._bev_maps(ctx, [dense[0], sparse[1]], bp)}


def test_store_equals_a_full_table_net_fed_zeros():
    ctx = device.default_context()
    bp = base._bev_params()
    params = synth.pyramid_params(C['bev_depth'])
    on, off = fs._nets(ctx, 2, params, ops.bev_support_mask(bp, PAD))
    if not on.frame_tables_on:
        assert ctx.lib.dodt_conv_mode() == 4
        return
    inputs = _inputs(ctx, bp)
    out = (ctx.empty((2, H, W, 32), np.float32), ctx.empty((2, H, W, 1), np.float32))
    ref = (ctx.empty((2, H, W, 32), np.float32), ctx.empty((2, H, W, 1), np.float32))
    assert on.store_bytes() == 0
    on.forward_device_padded(inputs['dense'], *out)          # primes on full tables: no store yet
    ctx.sync()
    assert on.store_bytes() == 0
    before = inputs['sparse'].download().copy()
    on.forward_device_padded(inputs['sparse'], *out)         # the first forward that restores takes the store
    ctx.sync()
    assert np.array_equal(inputs['sparse'].download().view(np.uint32), before.view(np.uint32))
    want = base._outputs(ctx, off, inputs['empty'], *ref)
    got = {n: on.activation('store:' + n) for n in base.LAYERS}
    got['feat'] = on.activation('store:pyramid_fusion1')
    got['bneck'] = on.activation('store:bottleneck')
    base._assert_same(got, want, 'constants store')
    # one frame of every map: the layer buffers, the three pooled maps, the output pair
    cells = (PAD + H) * W
    maps = 32 + 64 + 8 + 16 + 32 + 4 + 8 + 8 + 16 + 2 + 3 * 4 + 4 + 8
    print('constants store: %.1f MB' % (on.store_bytes() / 1e6))
    assert on.store_bytes() == 4 * (cells * maps + H * W * 33)
    # new weights: the store is taken again, by the first forward that restores
    reload = synth.pyramid_params(C['bev_depth'], seed=77)
    on.load_params(reload)
    off.load_params(reload)
    on.forward_device_padded(inputs['dense'], *out)
    on.forward_device_padded(inputs['empty'], *out)
    ctx.sync()
    want = base._outputs(ctx, off, inputs['empty'], *ref)
    got = {n: on.activation('store:' + n) for n in base.LAYERS}
    got['feat'] = on.activation('store:pyramid_fusion1')
    got['bneck'] = on.activation('store:bottleneck')
    base._assert_same(got, want, 'constants store after a weight reload')
    on.set_input_support(None)                               # frees it
    assert on.store_bytes() == 0


# the smallest net that still has every pyramid level and more than one tile per layer: 60 x 96 (padded 64 x 96, level
# 3 is 8 x 12), three frames -- the store's pass runs one frame beside them
SB, SH, SW, DEPTH = 3, 60, 96, C['bev_depth']


def _small_read(ctx, ex, feat, bneck):
    ctx.sync()
    out = {n: ex.activation(n) for n in base.LAYERS}
    out['feat'] = feat.download().copy()
    out['bneck'] = bneck.download().copy()
    return out


def _small_store(ex):
    got = {n: ex.activation('store:' + n) for n in base.LAYERS}
    got['feat'] = ex.activation('store:pyramid_fusion1')
    got['bneck'] = ex.activation('store:bottleneck')
    return got


def test_store_taken_inside_a_timed_forward_on_a_callers_input():
    """The constants store is a one-frame walk on zeros beside a three-frame extractor, taken here inside a timed
    forward while the input is a caller's buffer (set_input): the forward around it, the caller's input and the
    forwards after it through all three ways the input is chosen must be untouched by it."""
    ctx = device.default_context()
    nets = []
    for _ in range(2):
        ex = BevVggPyr(ctx=ctx, shared_gpu=True)
        ex.load_params(sound.live_fringe_params(DEPTH))
        ex._ensure(SB, SH, SW, DEPTH)
        nets.append(ex)
    on, off = nets
    mask = np.ones((PAD + SH, SW), np.uint8)     # every cell of the real rows
    mask[:PAD] = 0
    on.set_input_support(mask, frame_tables=True)
    if not on.frame_tables_on:
        assert ctx.lib.dodt_conv_mode() == 4
        return
    rng = np.random.default_rng(11)
    dense = np.zeros((SB, PAD + SH, SW, DEPTH), np.float32)
    dense[:, PAD:] = rng.uniform(0.1, 1.0, size=(SB, SH, SW, DEPTH))
    sparse = np.zeros_like(dense)      # a few isolated cells, other ones in every frame
    for f, y, x, c in ((0, PAD, 0, 0), (0, PAD + SH - 1, SW - 1, 5), (1, PAD + 30, 47, 2), (2, PAD + 17, 64, 5)):
        sparse[f, y, x, c] = 0.75
    other = np.zeros_like(dense)
    for f, y, x, c in ((0, PAD + 40, 20, 1), (1, PAD + 5, 90, 3), (2, PAD + 59, 33, 0), (2, PAD + 8, 8, 4)):
        other[f, y, x, c] = 0.5
    zeros = ctx.zeros(dense.shape, np.float32)
    new_pair = lambda: (ctx.empty((SB, SH, SW, 32), np.float32), ctx.empty((SB, SH, SW, 1), np.float32))
    pair_a, pair_b, ref = new_pair(), new_pair(), new_pair()

    def want(host):
        d = ctx.array(host)
        off.forward_device_padded(d, *ref)
        return _small_read(ctx, off, *ref)

    # 1. prime through set_input on a caller's buffer
    x = ctx.array(dense)
    on.set_input(x)
    on.forward_timed(None, *pair_a)
    base._assert_same(_small_read(ctx, on, *pair_a), want(dense), 'priming forward')
    assert on.store_bytes() == 0
    # 2. the first restoring forward is a timed one, on the same buffer: it takes the store
    x.upload(sparse)
    info = on.forward_timed(None, *pair_a)
    base._assert_same(_small_read(ctx, on, *pair_a), want(sparse), 'first restoring forward (timed, set_input)')
    assert np.array_equal(x.download().view(np.uint32), sparse.view(np.uint32))
    assert on.store_bytes() > 0
    assert all(np.isfinite(l['ms']) and l['ms'] >= 0 for l in info), [l['ms'] for l in info]
    computed, restored = on.frame_split()
    assert min(computed) >= 0 and min(restored) >= 0 and sum(restored) > 0, (computed, restored)
    assert [l['items'] for l in info] == computed
    zero_maps = want(np.zeros_like(dense))
    base._assert_same(_small_store(on), zero_maps, 'constants store')
    # 3. the extractor's own input buffer (the host-side copy), then a padded caller's buffer
    on.set_input(None)
    d_other, d_dense, d_sparse = ctx.array(np.ascontiguousarray(other[:, PAD:])), ctx.array(dense), ctx.array(sparse)
    on.forward_device(d_other, *pair_b)
    base._assert_same(_small_read(ctx, on, *pair_b), want(other), 'forward_device into a second pair')
    on.forward_device_padded(d_dense, *pair_a)
    base._assert_same(_small_read(ctx, on, *pair_a), want(dense), 'forward_device_padded into the first pair')
    # 4. new weights (a store that is not zero): one priming and one restoring forward
    reload = synth.pyramid_params(DEPTH, seed=77)
    on.load_params(reload)
    off.load_params(reload)
    on.forward_device_padded(d_dense, *pair_a)
    base._assert_same(_small_read(ctx, on, *pair_a), want(dense), 'priming forward after a weight reload')
    on.forward_device_padded(d_sparse, *pair_a)
    base._assert_same(_small_read(ctx, on, *pair_a), want(sparse), 'restoring forward after a weight reload')
    off.forward_device_padded(zeros, *ref)
    zero_maps = _small_read(ctx, off, *ref)
    assert any(v.any() for v in zero_maps.values())
    base._assert_same(_small_store(on), zero_maps, 'constants store after a weight reload')


def _run_sequence(check_counts):
    ctx = device.default_context()
    bp = base._bev_params()
    mask = ops.bev_support_mask(bp, PAD)
    params = synth.pyramid_params(C['bev_depth'])
    on, off = fs._nets(ctx, 2, params, mask)
    assert on.frame_tables_on == (ctx.lib.dodt_conv_mode() != 4)
    inputs = _inputs(ctx, bp)
    host = {k: v.download() for k, v in inputs.items()}
    pairs = [(ctx.empty((2, H, W, 32), np.float32), ctx.empty((2, H, W, 1), np.float32)) for _ in range(9)]
    ref = (ctx.empty((2, H, W, 32), np.float32), ctx.empty((2, H, W, 1), np.float32))
    reload = synth.pyramid_params(C['bev_depth'], seed=77)
    model, full = None, None
    if check_counts and on.frame_tables_on and ctx.lib.dodt_conv_mode() == 2:
        off.set_input(inputs['dense'])
        full = off.forward_timed(None, *ref)
        model = _Model(mask, full, 2)
        off.set_input(None)
    # dense -> 4 000 points -> empty -> dense -> mixed into alternating pairs, twice with a weight reload in between;
    # then pairs 2 .. 8 (the ninth evicts pair 0, which is primed again when it comes back)
    steps = [('dense', 0), ('dense', 1), ('sparse', 0), ('empty', 1), ('dense', 0), ('mixed', 1), 'reload',
             ('dense', 1), ('dense', 0), ('sparse', 1), ('empty', 0), ('dense', 1), ('mixed', 0),
             ('sparse', 2), ('dense', 3), ('mixed', 4), ('empty', 5), ('dense', 6), ('sparse', 7), ('dense', 8),
             ('sparse', 0), ('empty', 1), ('mixed', 8), ('sparse', 0)]
    seen_dense_to_sparse = False
    last = None
    for i, step in enumerate(steps):
        if step == 'reload':
            on.load_params(reload)
            off.load_params(reload)
            if model:
                model.reset()
            last = None
            continue
        name, k = step
        got = base._outputs(ctx, on, inputs[name], *pairs[k])
        want = base._outputs(ctx, off, inputs[name], *ref)
        base._assert_same(got, want, 'step %d (%s into pair %d)' % (i, name, k))
        if model:
            computed, restored = on.frame_split()
            items = on.frame_items()
            expect = model.forward(host[name], k)
            print('step %2d %-6s pair %d computed %s restored %s' % (i, name, k, computed, restored))
            assert (computed, restored) == expect, (i, step, list(zip(NAMES, computed, restored, *expect)))
            assert items == [a + b if a >= 0 else -1 for a, b in zip(computed, restored)], (i, step)
            if last == 'dense' and name == 'sparse' and min(computed) >= 0:
                # every layer restores; the matrix pipe's count is the computed items', below the union's
                seen_dense_to_sparse = True
                assert all(r > 0 for r in restored), restored
                per_item = [l['flops_executed'] / l['items'] for l in full]
                flops = on.mfma_flops()
                assert abs(flops - sum(p * a for p, a in zip(per_item, computed))) <= 1e-9 * flops
                assert flops < sum(p * (a + b) for p, a, b in zip(per_item, computed, restored))
                # the byte count: the computed share of every layer's maps, its weights, the bottleneck map, and the
                # copies -- a restored item's outputs read from the store and written (with the pooled tile behind
                # conv1_2 / conv2_2 / conv3_3 and the bottleneck cells of a pyramid_fusion1 tile)
                want_bytes = 2.0 * H * W * 4
                for l, a, r in zip(full, computed, restored):
                    n = l['name']
                    w_bytes = 4.0 * reload[n]['w'].size
                    th, tw = model.tile[n]
                    bn = reload[n]['w'].shape[2 if n.startswith('up') else 3] // model.nt[n]
                    per = th * tw * bn * (1.25 if n in ('conv1_2', 'conv2_2', 'conv3_3') else 1.0)
                    per += th * tw if n == 'pyramid_fusion1' else 0
                    want_bytes += (l['bytes'] - w_bytes) * a / l['items'] + w_bytes + 2.0 * 4 * per * r
                assert abs(on.bytes() - want_bytes) <= 1e-9 * want_bytes, (on.bytes(), want_bytes)
        last = name
    if model:
        assert seen_dense_to_sparse


def test_sequence_bit_equal_and_split_counts():
    _run_sequence(True)


@pytest.mark.parametrize('mode', ['0', '4'])
def test_other_conv_forms_in_child_process(mode):
    """DODT_CONV_WINO is read once per process: the direct kernels (0) restore from a store of their own, F(4x4,3x3)
    (4) stays on its static tables and takes none; both byte-equal to full tables over the same sequence."""
    env = dict(os.environ, DODT_CONV_WINO=mode)
    code = ('import sys; sys.path.insert(0, %r); import tests.test_gpu_bev_restore as t; '
            't._run_sequence(False); t.test_store_equals_a_full_table_net_fed_zeros(); print("ok")' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _free_running(ctx, pipe, steps):
    """steps pipeline steps with fresh inputs and no host sync in between; the last step's records and both parities'
    BEV feature map and bottleneck."""
    keep = []      # (the inputs stay alive until the end: the streams read them behind the host)
    for k in range(steps):
        seq, frames = 20 + k % 3, (k % 4, k % 4 + 2)
        pts = [synth.lidar_frame(seq, f) for f in frames]
        imgs = [ctx.array(synth.image_frame(seq, f)) for f in frames]
        heads = [{n: ctx.array(v) for n, v in synth.head_outputs(seq, f, pipe.n_all, pipe.P).items()} for f in frames]
        keep.append(([ctx.array(p) for p in pts], imgs, heads))
        pipe.run(keep[-1][0], [len(p) for p in pts], imgs, heads)
    pipe.finish()
    ctx.sync()
    out = [pipe.d_records.download().copy(), pipe.d_rec_counts.download().copy()]
    for parity in (0, 1):
        out += [pipe.feat[parity][n].download().copy() for n in ('bev_feat', 'bev_bneck')]
    return out


def test_pipeline_records_and_bev_maps_bit_equal_free_running():
    """Eight free-running steps with fresh inputs, no host sync between them, both parities of the output buffers:
    restoring per-frame tables against the static tables alone."""
    ctx = device.default_context()
    on = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024)
    assert on.bev_net.frame_tables_on
    a = _free_running(ctx, on, 8)
    computed, restored = on.bev_net.frame_split()
    assert all(n >= 0 for n in computed) and all(n > 0 for n in restored), (computed, restored)
    assert on.bev_net.store_bytes() > 0
    del on
    off = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024, bev_frame_tables=False)
    assert not off.bev_net.frame_tables_on and off.bev_skipped_items > 0
    b = _free_running(ctx, off, 8)
    assert a[1].sum() > 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
