"""Every case of tests/_conv_cases.py on the device against the oracle.  Needs an MI355X.

What the older conv tests cannot see (tests/test_conv_plan.py proves on the host that these cases do): every kernel
variant a configuration can select, persistent workgroups that walk four and more work items (8 plan CUs: a grid of
8 .. 32 workgroups) through the grouped and the single queues, ragged tiles, tail launches -- on DENSE inputs, with
batch-norm statistics that differ per layer and channel (_conv_cases.varied_bn), EVERY layer, the returned map and
the bottleneck compared for EVERY frame.  Each case runs twice on one extractor and must return the same bytes: the
second forward starts from the counters and the LDS the first one left.

Bars, the project's own: 1e-4 of a layer's scale for the fp32 and the split path (test_gpu_conv.py,
test_gpu_conv_split.py); test_gpu_conv_bf16.py's `_bars` for the bf16 path, its stored maps bf16 values, a folded
conv1_1 refused.  The library reads its switches once per process: the default mode runs here, every other mode of
_conv_cases.MODES in one child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_cases as cc
from dodt_amd import device
from oracle import extractors as oext
from oracle import tfops
from tests.test_gpu_conv_bf16 import _bars

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _extractor(c, ctx):
    from dodt_amd.core.feature_extractors import vgg, vgg_pyramid
    cls = {'bev': vgg_pyramid.BevVggPyr, 'img': vgg_pyramid.ImgVggPyr, 'bev_plain': vgg.BevVgg,
           'img_plain': vgg.ImgVgg}[c.net]
    return cls(ctx=ctx, shared_gpu=c.shared, conv_dtype=c.dtype)


def _rel(got, want):
    d = np.abs(got - want)
    scale = float(np.abs(want).max()) + 1e-12
    return float(d.max()) / scale, float(d.mean()) / scale


def run_case(c):
    """Runs a case in this process (whose environment must be the case's mode); prints each figure, then asserts."""
    ctx = device.Context(plan_cus=c.cus)
    ex = _extractor(c, ctx)
    try:
        ex.load_params(cc.case_params(c))
        x = cc.case_input(c)
        feat, ends = ex.build(x, with_bottleneck=True)
        assert ex.plan() == cc.host_plan(c), 'the extractor planned something else than dodt_conv_plan_host'
        plan = ex.plan()
        folded = ex.first_layers_folded
        assert folded == plan[0]['folded']
        names = [r['name'] for r in plan if not r['folded']]
        if not cc.NETS[c.net]['plain']:
            names.remove('pyramid_fusion1')        # the returned map
        got = {n: ex.activation(n) for n in names}
        if folded:
            with pytest.raises(ValueError, match='folded'):
                ex.activation('conv1_1')
        # the second forward on the same extractor: the same bytes
        feat2, ends2 = ex.build(x, with_bottleneck=True)
        same = [n for n in names if not np.array_equal(got[n], ex.activation(n))]
        assert not same, 'second forward differs in %s' % same
        assert np.array_equal(feat, feat2) and np.array_equal(ends['bottleneck'], ends2['bottleneck'])
    finally:
        ex.close()
        ctx.close()
    maps, want, want_bn = cc.oracle(cc.oracle_key(c, folded))
    if cc.NETS[c.net]['plain']:
        # (test_gpu_vgg_plain.py: the upsampling is exact arithmetic on the device's conv4_3, the bottleneck is
        #  compared on the device's own map)
        for f in range(c.batch):
            assert np.array_equal(feat[f], tfops.resize_bilinear(got['conv4_3'][f], feat.shape[1], feat.shape[2]))
        want_bn = np.stack([oext.bottleneck_1x1(feat[f], cc.case_params(c)['bottleneck']) for f in range(c.batch)])
    figures = [(n, got[n], maps[n]) for n in names] + [('feature_maps', feat, want),
                                                       ('bottleneck', ends['bottleneck'], want_bn)]
    worst = max((_rel(g, w) + (n,) for n, g, w in figures))
    print('%s: worst layer %s max %.3e mean %.3e of its scale' % (cc.case_id(c), worst[2], worst[0], worst[1]))
    for n, g, w in figures:
        assert g.shape == w.shape, n
        if c.dtype == 'bf16':
            if n not in ('feature_maps', 'bottleneck'):
                assert np.array_equal(g, tfops.round_bf16(g)), n          # stored maps ARE bf16
            if n == 'bottleneck':
                _bars(g, w, n, max_rel=3e-2, mean_rel=2e-3)
            else:
                _bars(g, w, n)
        else:
            for f in range(c.batch):        # 1e-4 of the layer's scale, in every frame
                err = float(np.abs(g[f] - w[f]).max())
                scale = float(np.abs(w).max()) + 1e-12
                assert err <= 1e-4 * scale, '%s frame %d: max abs err %g vs scale %g' % (n, f, err, scale)
    return worst


def run_mode(mode):
    """Every case of a mode, in this process (a child of test_other_modes_in_a_child_process)."""
    assert all(os.environ.get(k) == v for k, v in cc.MODES[mode].items())
    for c in cc.CASES:
        if c.mode == mode:
            run_case(c)
    print('MODE %s ok' % mode)


DEFAULT = [c for c in cc.CASES if c.mode == 'default']


@pytest.mark.parametrize('case', DEFAULT, ids=[cc.case_id(c) for c in DEFAULT])
def test_case_matches_oracle_in_every_layer_and_frame(case):
    assert not [k for k in os.environ if k.startswith(cc.CONV_SWITCH_PREFIX)], 'the default mode has no switch set'
    run_case(case)


@pytest.mark.parametrize('mode', [m for m in cc.MODES if m != 'default'])
def test_other_modes_in_a_child_process(mode):
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_conv_paths as t; '
            't.run_mode(%r)' % (ROOT, os.path.join(ROOT, 'tests'), mode))
    r = subprocess.run([sys.executable, '-c', code], env=cc.mode_env(mode), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'MODE %s ok' % mode in r.stdout


def test_plan_cus_takes_multiples_of_8_up_to_the_devices_count():
    ctx = device.Context()
    try:
        for bad in (0, 4, 7, 12, 20, -8, 1 << 20):
            assert ctx.lib.dodt_ctx_set_plan_cus(ctx.handle, bad) != 0, bad
        for good in (8, 64, 16):
            assert ctx.lib.dodt_ctx_set_plan_cus(ctx.handle, good) == 0, good
        with pytest.raises(ValueError):
            device.Context(plan_cus=12)
        # extractors created afterwards plan with it; the default context is untouched
        case = cc.Case('bev', 'f32', 64, 96, 2, 16, 'default')
        ex = _extractor(case, ctx)
        ex.load_params(cc.case_params(case))
        ex.build(cc.case_input(case))
        assert ex.plan() == cc.host_plan(case)
        assert ex.plan() != cc.host_plan(case._replace(cus=256))
        ex.close()
    finally:
        ctx.close()
