"""What the conv path's small test cases reach, proved on the host's plan (no GPU).

The planner (pick_variant, plan_layer in conv.hip) chooses a layer's kernel and cuts its work by CU count, batch
and map size, so a small map on a 256-CU device runs other kernels than the workload, one work item per persistent
workgroup, and never a tail launch.  tests/_conv_cases.py lists cases that plan with 8 CUs (device.Context(
plan_cus=)); this file computes their plans with dodt_conv_plan_host and asserts that together they

  * select every entry of the variant table, but for an explicit list with the reason no case can (UNREACHABLE),
  * walk at least four items per workgroup in every persistent kernel family, with item counts that leave the
    eight grouped queues uneven,
  * cut ragged tiles at the right and at the bottom edge in every family,
  * make tail launches, one of which changes whether the layer pools in its epilogue,
  * run every variant the bench configurations run.

tests/test_gpu_conv_paths.py runs the same cases on the device; a table entry added without a case that reaches
it, or a case that stops walking several items, fails here first."""
import json
import os

import numpy as np
import pytest

import _conv_cases as cc
from dodt_amd import _lib
from oracle import tfops

POOLED = ('conv1_2', 'conv2_2', 'conv3_3')


signature = cc.signature

# variants no case of the table can select, each with the reason
UNREACHABLE = {
    'conv3x3_bf16_stream_kernel 32x6 bn32 ck16 lds74176 bf16':
        'conv1_2 of a bf16 net (two input chunks); by default conv1_1 runs folded into its launch, on the first2 '
        'kernel with the same tiles and ring.  Only DODT_CONV_BF16_FIRST2=0 launches this entry '
        '(tests/test_gpu_conv_bf16.py::test_two_launch_first_layers_match_the_same_bars).',
}

# Families whose workgroups cannot walk four items under the default rule, with the reason and the bound that is
# asserted in its place (so that a change of the rule that lifts the bound fails here and asks for a case).
NO_FOUR_ITEMS = {
    'bf16_dma8': 'pick_variant takes the 8-row tiles only where the 16-row tiles give fewer than 1.6 items per CU; '
                 'an 8-row table has at most twice those items, 3.2 per CU, on three workgroups per CU: 1.07 items '
                 'per workgroup at the most.  The kernel is the 16-row kernel (one template, MT = 2): its queue, its '
                 'look-ahead and its carried state are the ones bf16_dma16 walks.',
}
# Tail launches: what the issue asks to state where no case exists.
NO_TAIL = {
    'split': 'a split (and a bf16) extractor plans single launches: the bf16 instantiations have no quarter tiles '
             '(dodt_extractor_create: shared_gpu is forced)',
    'bneck_fused': 'a tail never decides bneck_fused differently from the main launch: pyramid_fusion1 has 32 output '
                   'channels, so its main variant and every quarter-tile companion have BN = 32',
}


@pytest.fixture(scope='module')
def planned():
    plans, variants = cc.plans(cc.CASES + cc.BENCH)
    return plans, variants


def _props(case, plan, variants):
    """What a case's plan shows, as (family, property) pairs and ('variant', signature)."""
    vs, out = variants[case.mode], set()
    capable = {i for i, v in enumerate(variants['default']) if v['flags'] & _lib.VARIANT_XCD_QUEUE}
    for r, j, vi in cc.launches(plan):
        v = vs[vi]
        fam = cc.family(v)
        out.add(('variant', signature(v)))
        n, g = r['items'][j], r['grid'][j]
        grouped = bool(v['flags'] & _lib.VARIANT_XCD_QUEUE)
        # four items per workgroup, on a grid of whole groups of eight, the queues' shares of the items uneven
        if n >= 4 * g and g % 8 == 0 and n % 8 != 0:
            if vi not in capable or grouped:
                out.add((fam, 'four_items'))
            if vi in capable and not grouped:
                out.add((fam, 'four_items_one_queue'))
        if r['w'] % v['tw']:
            out.add((fam, 'ragged_right'))
        if r['h'] % v['th']:
            out.add((fam, 'ragged_bottom'))
        if j == 1:
            out.add((fam, 'tail'))
            main = vs[r['variant'][0]]
            if (r['name'] in POOLED and main['flags'] & _lib.VARIANT_CAN_POOL
                    and not v['flags'] & _lib.VARIANT_CAN_POOL and not r['pool_fused']):
                out.add((fam, 'tail_unfuses_pool'))
    return out


@pytest.fixture(scope='module')
def reached(planned):
    plans, variants = planned
    out = set()
    for c in cc.CASES:
        out |= _props(c, plans[c], variants)
    return out


def test_cases_are_distinct_and_small():
    assert len(set(cc.CASES)) == len(cc.CASES)
    assert {c.mode for c in cc.CASES} == set(cc.MODES)
    for c in cc.CASES:
        assert c.cus % 8 == 0 and 8 <= c.cus <= 256
        assert c.H * c.W * c.batch <= 200 * 264 * 3, cc.case_id(c)     # an oracle of a second or two


def test_the_variant_table_is_one_table_in_every_mode(planned):
    _, variants = planned
    strip = lambda vs: [dict(v, flags=v['flags'] & ~_lib.VARIANT_XCD_QUEUE) for v in vs]
    for mode, vs in variants.items():
        assert strip(vs) == strip(variants['default']), mode
    sigs = [signature(v) for v in variants['default']]
    assert len(set(sigs)) == len(sigs)
    # the grouped queues are what DODT_CONV_*_XCD=0 turns off, and nothing else does
    assert not any(v['flags'] & _lib.VARIANT_XCD_QUEUE for v in variants['one_queue'])
    assert any(v['flags'] & _lib.VARIANT_XCD_QUEUE for v in variants['default'])


def test_every_variant_is_reached_or_listed_with_a_reason(planned, reached):
    _, variants = planned
    table = {signature(v) for v in variants['default']}
    run = {s for k, s in reached if k == 'variant'}
    assert set(UNREACHABLE) <= table, 'listed as unreachable but not in the table: %s' % sorted(set(UNREACHABLE) - table)
    assert not run & set(UNREACHABLE), 'listed as unreachable but reached: %s' % sorted(run & set(UNREACHABLE))
    missing = table - run - set(UNREACHABLE)
    assert not missing, 'no case of tests/_conv_cases.py selects: %s' % sorted(missing)
    assert all(len(reason) > 40 for reason in UNREACHABLE.values())


FAMILIES = ['direct', 'direct_deconv', 'small_cin', 'wino22', 'wino43', 'deconv_dma', 'bf16_dma8', 'bf16_dma16',
            'bf16_stream', 'bf16_first2', 'bf16_template', 'bf16_template_deconv', 'split', 'split_deconv']


def test_the_families_are_the_tables(planned):
    _, variants = planned
    assert {cc.family(v) for v in variants['default']} == set(FAMILIES)


@pytest.mark.parametrize('fam', FAMILIES)
def test_some_case_walks_four_items_per_workgroup(planned, reached, fam):
    """items >= 4 x grid, grid a multiple of 8, items no multiple of 8 (the eight queues' shares differ) -- with the
    grouped queues on wherever the family has them, and once more with one queue per launch."""
    plans, variants = planned
    if fam in NO_FOUR_ITEMS:
        assert len(NO_FOUR_ITEMS[fam]) > 40
        for c in cc.CASES + cc.BENCH:
            for r, j, vi in cc.launches(plans[c]):
                if cc.family(variants[c.mode][vi]) == fam:
                    assert r['items'][j] < 2 * r['grid'][j], (cc.case_id(c), r['name'])
        return
    assert (fam, 'four_items') in reached
    if any(cc.family(v) == fam and v['flags'] & _lib.VARIANT_XCD_QUEUE for v in variants['default']):
        assert (fam, 'four_items_one_queue') in reached


@pytest.mark.parametrize('fam', FAMILIES)
def test_some_case_cuts_ragged_tiles_at_both_edges(reached, fam):
    assert (fam, 'ragged_right') in reached
    assert (fam, 'ragged_bottom') in reached


def test_tail_launches(planned, reached):
    """The fp32 direct kernels make tail launches (conv and transposed conv), and in one case the tail's quarter
    tiles cannot pool where the main launch's tiles can, so the layer's pool runs as a launch of its own."""
    plans, variants = planned
    assert ('direct', 'tail') in reached and ('direct_deconv', 'tail') in reached
    assert ('direct', 'tail_unfuses_pool') in reached
    assert all(len(reason) > 40 for reason in NO_TAIL.values())
    for c in cc.CASES + cc.BENCH:
        for r in plans[c]:
            if r['variant'][1] >= 0:
                fam = cc.family(variants[c.mode][r['variant'][1]])
                assert fam in ('direct', 'direct_deconv'), (cc.case_id(c), r['name'], fam)     # NO_TAIL['split']
                assert variants[c.mode][r['variant'][1]]['flags'] & _lib.VARIANT_TAIL_ONLY or fam == 'direct_deconv'
            if r['name'] == 'pyramid_fusion1':
                assert r['bneck_fused'], cc.case_id(c)                                           # NO_TAIL['bneck_fused']


def test_small_grids_and_empty_queues_are_reached(planned):
    """Fewer than 8 items: a grid of fewer than 8 workgroups, grouped queues with no item."""
    plans, variants = planned
    fams = set()
    for c in cc.CASES:
        for r, j, vi in cc.launches(plans[c]):
            v = variants[c.mode][vi]
            if r['items'][j] < 8 and v['flags'] & _lib.VARIANT_XCD_QUEUE:
                fams.add(cc.family(v))
    assert {'wino22', 'deconv_dma', 'bf16_dma8'} <= fams, fams


def test_bench_configurations_run_only_variants_a_small_case_runs(planned, reached):
    plans, variants = planned
    run = {s for k, s in reached if k == 'variant'}
    for c in cc.BENCH:
        assert plans[c][0]['name'] == 'conv1_1' and len(plans[c]) == 16
        for r, j, vi in cc.launches(plans[c]):
            assert signature(variants[c.mode][vi]) in run, (cc.case_id(c), r['name'])


def test_grids_are_what_a_launch_takes(planned):
    """grid = min(items, CUs x workgroups per CU); a folded conv1_1 has no launch."""
    plans, variants = planned
    for c in cc.CASES + cc.BENCH:
        for r, j, vi in cc.launches(plans[c]):
            v = variants[c.mode][vi]
            bpc = 3 if v['flags'] & _lib.VARIANT_SMALL_CIN else v['blocks_per_cu']
            assert r['grid'][j] == min(r['items'][j], c.cus * bpc), (cc.case_id(c), r['name'])
        if plans[c][0]['folded']:
            assert plans[c][0]['variant'] == [-1, -1] and plans[c][0]['grid'] == [0, 0]
            assert variants[c.mode][plans[c][1]['variant'][0]]['flags'] & _lib.VARIANT_FIRST2
            assert plans[c][1]['pool_fused']


def test_plans_are_the_pinned_plans():
    """The planner decides what tests/golden/conv_plans.json records: per layer of every pinned configuration the main
    and the tail kernel (by signature), items, grid, pool_fused, bneck_fused, folded.  A change of the selection
    code that means to keep every choice passes against the file as it stands (tests/golden/make_conv_plans.py)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plans.json')) as f:
        want = json.load(f)
    got = json.loads(json.dumps(cc.pinned_plans()))
    assert list(got['plans']) == list(want['plans'])
    assert len(want['plans']) >= len(cc.CASES + cc.BENCH) + 2 * len(cc.PIN_BATCHES) * len(cc.PIN_CUS)

    def named(pinned, rec):      # a layer's record with its two variants as text
        return [pinned['signatures'][i] if i >= 0 else None for i in rec[:2]] + rec[2:]
    for cid in want['plans']:
        for name, w, g in zip(want['layers'], want['plans'][cid], got['plans'][cid]):
            assert named(got, g) == named(want, w), (cid, name)
        assert len(got['plans'][cid]) == len(want['plans'][cid]), cid
    assert got == want          # ... and the file is what the generator writes


def test_plan_host_refuses_what_create_refuses():
    from dodt_amd.core.feature_extractors import vgg_pyramid
    with pytest.raises(ValueError):
        vgg_pyramid.conv_plan_host(_lib.EXTRACTOR_VGG_PYR, 30, 40, 6, 4, 1, 8)        # 34 rows: not divisible by 8
    with pytest.raises(ValueError):
        vgg_pyramid.conv_plan_host(_lib.EXTRACTOR_VGG | _lib.EXTRACTOR_BF16, 32, 32, 6, 0, 1, 8)
    with pytest.raises(ValueError):
        vgg_pyramid.conv_plan_host(_lib.EXTRACTOR_VGG_PYR, 28, 40, 6, 4, 1, 0)
    assert len(vgg_pyramid.conv_plan_host(_lib.EXTRACTOR_VGG, 33, 41, 6, 0, 1, 8)) == 10


# ---- the inputs: dense enough to show a wrong channel ---------------------------------------------------------

# (every distinct input of the table, through the fp32 oracle)
INPUTS = sorted({(c.net, 'f32', c.H, c.W, c.batch, False) for c in cc.CASES})


@pytest.mark.parametrize('key', INPUTS, ids=['%s-%dx%d-b%d' % (k[0], k[2], k[3], k[4]) for k in INPUTS])
def test_inputs_keep_the_channels_alive(key):
    """With the varied batch-norm statistics: in every layer at least 90 % of the channels have a non-zero output
    somewhere, and at least 20 % of all outputs are non-zero -- a dead channel would hide a wrong scale."""
    maps, feat, bneck = cc.oracle(key)
    nz = total = 0
    for name, m in list(maps.items()) + [('bottleneck', bneck)]:
        alive = (np.abs(m).reshape(-1, m.shape[-1]).max(axis=0) > 0).mean()
        assert alive >= 0.9, '%s: %.3f of the channels alive' % (name, alive)
        nz += np.count_nonzero(m)
        total += m.size
    assert nz >= 0.2 * total
    assert nz <= 0.9 * total          # ... and the ReLU still clips


# ---- teeth ------------------------------------------------------------------------------------------------

def _layer_inputs(maps, feat, pad_top):
    return {'conv1_2': ('conv', maps['conv1_1']), 'conv3_2': ('conv', maps['conv3_1']),
            'upconv2': ('deconv', maps['pyramid_fusion3']),
            'pyramid_fusion1': ('conv', np.concatenate([maps['conv1_2'], maps['upconv1']], axis=3)),
            'bottleneck': ('1x1', feat)}


def _mutants(x, kind, p, frame=0):
    """(true output, output with the BN scale rolled by one channel, output without the mean) of one layer."""
    if kind == 'conv':
        pre = tfops.conv2d_same(x[frame], p['w'])
    elif kind == 'deconv':
        pre = tfops.conv2d_transpose_s2_same(x[frame], p['w'])
    else:
        pre = (x[frame].reshape(-1, p['w'].shape[2]) @ p['w'].reshape(-1, 1)).reshape(x[frame].shape[:2] + (1,))
    scale, shift = tfops.bn_scale_shift(p['beta'], p['mean'], p['var'])
    true = tfops.bn_relu(pre, p['beta'], p['mean'], p['var'])
    rolled = np.maximum(pre * np.roll(scale, 1) + shift, np.float32(0))
    no_mean = tfops.bn_relu(pre, p['beta'], np.zeros_like(p['mean']), p['var'])
    return true, rolled, no_mean


@pytest.mark.parametrize('layer', ['conv1_2', 'conv3_2', 'upconv2', 'pyramid_fusion1', 'bottleneck'])
def test_varied_statistics_show_a_wrong_channel_and_a_lost_mean(layer):
    """The gap these tests close.  Two deliberately wrong copies of the oracle's output of a layer -- the per-channel
    BN scale rolled by one channel (an epilogue that reads the neighbour's scale), and the mean dropped from the shift
    (a host fold that loses it) -- lie further than 100 x the fp32 bar (1e-4 of the layer's scale) from the true
    output when the statistics vary per channel.  With synth.pyramid_params' statistics (mean 0, var 1: what every GPU
    conv test ran before) the SAME two mutations do not exceed the bar: they change nothing at all, so the suite
    could not see either bug.  (The bottleneck has one output channel: rolling its scale is the identity with any
    statistics, so only the lost mean is asserted there.)"""
    case = cc.Case('bev', 'f32', 64, 96, 2, 256, 'default')
    assert case in cc.CASES
    bar = 1e-4
    for varied in (True, False):
        params = cc.net_params('bev', varied=varied)
        if varied:
            maps, feat, bneck = cc.oracle(cc.oracle_key(case))
        else:
            from oracle import extractors as oext
            x, col = cc.case_input(case), {}
            f = oext.vgg_pyramid(x[0], params, pad_top=4, collect=col)
            maps, feat = {k: v[None] for k, v in col.items()}, f[None]
            bneck = oext.bottleneck_1x1(f, params['bottleneck'])[None]
        kind, x_in = _layer_inputs(maps, feat, 4)[layer]
        true, rolled, no_mean = _mutants(x_in, kind, params[layer])
        want = bneck[0] if layer == 'bottleneck' else feat[0] if layer == 'pyramid_fusion1' else maps[layer][0]
        if layer == 'pyramid_fusion1':
            true, rolled, no_mean = true[4:], rolled[4:], no_mean[4:]
        assert np.array_equal(true, want)          # the copy is the oracle's own arithmetic
        scale = float(np.abs(true).max())
        d_roll = float(np.abs(rolled - true).max()) / scale
        d_mean = float(np.abs(no_mean - true).max()) / scale
        if varied:
            assert d_mean > 100 * bar, d_mean
            if layer != 'bottleneck':
                assert d_roll > 100 * bar, d_roll
        else:
            assert d_roll <= bar and d_mean <= bar, (d_roll, d_mean)
