"""The case table of the conv path's tests, and the helpers both of them share.

tests/test_conv_plan.py (no GPU) proves on the host's plan that these cases reach every kernel variant, walk several
work items per persistent workgroup, cut ragged tiles and make tail launches; tests/test_gpu_conv_paths.py runs
the same cases on the device against the oracle.  A case is (net, dtype, padded size, batch, plan CUs, mode, shared):
plan CUs is the CU count the extractor plans with (device.Context(plan_cus=)), mode an environment the library
reads once per process -- so everything of one mode runs in one child process."""
import collections
import functools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the environment modes of the issue: the default, the forms of the fp32 3x3 layers, the register-staged
# transposed convs, the template's bf16 instantiation, one work queue per launch
MODES = collections.OrderedDict([
    ('default', {}),
    ('wino0', {'DODT_CONV_WINO': '0'}),
    ('wino4', {'DODT_CONV_WINO': '4'}),
    ('deconv_direct', {'DODT_CONV_DECONV_DMA': '0'}),
    ('bf16_template', {'DODT_CONV_BF16_DMA': '0'}),
    ('one_queue', {'DODT_CONV_BF16_XCD': '0', 'DODT_CONV_F32_XCD': '0'}),
])
# two more forms a switch keeps, planned for the pin of tests/golden/conv_plans.json only (the device tests run them
# from tests/test_gpu_conv_bf16.py): the level-1 layers without the streaming kernel, conv1_1 and conv1_2 as two launches
PIN_MODES = collections.OrderedDict([
    ('no_stream', {'DODT_CONV_BF16_STREAM': '0'}),
    ('two_launch', {'DODT_CONV_BF16_FIRST2': '0'}),
])
# every switch of the conv path a mode does not set must be unset: the plans are the library's defaults
CONV_SWITCH_PREFIX = 'DODT_CONV_'

NETS = {   # stored input channels (the image's three are padded to four), zero rows on top, plain VGG?
    'bev': dict(in_c=6, pad_top=4, plain=False),
    'img': dict(in_c=4, pad_top=0, plain=False),
    'bev_plain': dict(in_c=6, pad_top=0, plain=True),
    'img_plain': dict(in_c=4, pad_top=0, plain=True),
}

Case = collections.namedtuple('Case', 'net dtype H W batch cus mode shared')
Case.__new__.__defaults__ = (False,)


def case_id(c):
    return '%s-%s-%dx%d-b%d-cu%d-%s%s' % (c.net, c.dtype, c.H, c.W, c.batch, c.cus, c.mode, '-shared' if c.shared else '')


# The table.  Sizes are padded sizes (BEV: 4 rows of them are the pad).  Chosen with test_conv_plan.py's
# assertions, which state what each of them is there for; 8 plan CUs make a grid of 8 .. 32 workgroups.
CASES = [
    # levels 200x264, 100x132, 50x66, 25x33: ragged tiles at every level, up to nine items per workgroup
    Case('bev', 'f32', 200, 264, 3, 8, 'default'),
    Case('bev', 'bf16', 200, 264, 2, 8, 'default'),
    # what the older tests run: one item per workgroup on the device's own count
    Case('bev', 'f32', 64, 96, 2, 256, 'default'),
    Case('bev', 'bf16', 64, 96, 2, 256, 'default'),
    # fewer than 8 items in the deep layers: grids below 8 workgroups, queues without items
    Case('bev', 'f32', 24, 40, 2, 8, 'default'),
    Case('bev', 'bf16', 24, 40, 2, 8, 'default'),
    Case('bev', 'f32s', 24, 40, 1, 8, 'default'),
    Case('img', 'f32s', 24, 40, 3, 8, 'default'),
    Case('img', 'f32s', 32, 48, 1, 8, 'default'),
    Case('bev', 'f32s', 200, 72, 1, 8, 'default'),
    Case('bev', 'f32s', 16, 136, 1, 8, 'default'),
    Case('bev', 'f32s', 104, 72, 3, 16, 'default'),
    # the direct fp32 kernels, their tail launches (not shared: tails allowed) and the plain net's odd sizes
    Case('img', 'f32', 24, 40, 1, 8, 'wino0'),
    Case('bev', 'f32', 56, 88, 1, 8, 'wino0'),
    Case('bev', 'f32', 128, 48, 1, 8, 'wino0'),
    Case('bev_plain', 'f32', 44, 52, 3, 8, 'wino0'),
    Case('bev_plain', 'f32', 33, 42, 3, 8, 'wino0'),      # (a frame is whole float4s: 33 x 41 x 6 is not)
    Case('bev', 'f32', 104, 72, 1, 8, 'wino0'),
    Case('bev', 'f32', 200, 72, 2, 8, 'wino0'),
    Case('img', 'f32', 32, 48, 1, 8, 'wino0'),            # (the fp32 first-layer kernel's 16 x 32 tile of four channels)
    Case('bev', 'f32', 24, 40, 1, 8, 'wino4'),
    Case('bev', 'f32', 40, 104, 3, 8, 'wino4'),
    # the register-staged transposed convs, fp32 and bf16
    Case('img', 'bf16', 24, 40, 1, 8, 'deconv_direct'),
    Case('bev', 'f32', 24, 40, 1, 8, 'deconv_direct'),
    Case('bev', 'f32', 56, 88, 1, 8, 'deconv_direct'),
    Case('bev', 'f32', 16, 136, 1, 8, 'deconv_direct'),
    Case('bev', 'bf16', 200, 72, 2, 8, 'deconv_direct'),
    Case('bev', 'f32', 200, 72, 2, 8, 'deconv_direct'),
    # the template's bf16 instantiation (and the bf16 first-layer kernels: nothing folds without the streaming kernel)
    Case('bev', 'bf16', 24, 40, 3, 8, 'bf16_template'),
    Case('img', 'bf16', 24, 40, 1, 8, 'bf16_template'),
    Case('img', 'bf16', 32, 48, 1, 8, 'bf16_template'),
    Case('bev', 'bf16', 16, 136, 1, 8, 'bf16_template'),
    Case('bev', 'bf16', 104, 72, 3, 8, 'bf16_template'),
    Case('bev', 'bf16', 64, 80, 3, 8, 'bf16_template'),
    # one queue per launch: the same multi-item walks without the XCD groups
    Case('bev', 'bf16', 64, 48, 3, 8, 'one_queue'),
    Case('bev', 'f32', 200, 72, 1, 8, 'one_queue'),
    Case('bev', 'bf16', 200, 136, 2, 8, 'one_queue'),
    Case('bev', 'bf16', 200, 264, 2, 8, 'one_queue'),
]

# the bench configurations (bench.py: FramePipeline's two nets, one and two pairs per step), 256 CUs
BENCH = [Case(net, dtype, H, W, batch, 256, 'default', True)
         for dtype in ('f32', 'f32s', 'bf16') for batch in (2, 4)
         for net, H, W in (('bev', 704, 800), ('img', 360, 1200))]


def kind_flags(c):
    from dodt_amd import _lib
    return ((_lib.EXTRACTOR_VGG if NETS[c.net]['plain'] else _lib.EXTRACTOR_VGG_PYR)
            | (_lib.EXTRACTOR_SHARED_GPU if c.shared else 0)
            | {'f32': 0, 'bf16': _lib.EXTRACTOR_BF16, 'f32s': _lib.EXTRACTOR_SPLIT}[c.dtype])


def host_plan(c):
    """The plan of a case in THIS process (its mode must be the process's environment)."""
    from dodt_amd.core.feature_extractors import vgg_pyramid
    n = NETS[c.net]
    return vgg_pyramid.conv_plan_host(kind_flags(c), c.H - n['pad_top'], c.W, n['in_c'], n['pad_top'], c.batch, c.cus)


def mode_env(mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith(CONV_SWITCH_PREFIX)}
    env.update(MODES[mode] if mode in MODES else PIN_MODES[mode])
    return env


_CHILD = '''
import json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import _conv_cases as cc
from dodt_amd.core.feature_extractors import vgg_pyramid
cases = [cc.Case(*c) for c in json.loads(sys.argv[1])]
print('PLANS ' + json.dumps(dict(variants=vgg_pyramid.conv_variants(), plans=[cc.host_plan(c) for c in cases])))
'''


@functools.lru_cache(maxsize=None)
def _plans_of_mode(mode, cases):
    r = subprocess.run([sys.executable, '-c', _CHILD % (ROOT, os.path.join(ROOT, 'tests')), json.dumps(cases)],
                       env=mode_env(mode), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('PLANS ')][-1]
    return json.loads(line[6:])


def plans(cases):
    """{case: plan} and the variant table per mode, every mode's plans computed in one child process of that mode."""
    out, variants = {}, {}
    for mode in list(MODES) + list(PIN_MODES):
        mine = tuple(c for c in cases if c.mode == mode)
        if not mine:
            continue
        got = _plans_of_mode(mode, tuple(tuple(c) for c in mine))
        variants[mode] = got['variants']
        out.update(zip(mine, got['plans']))
    return out, variants


def family(v):
    """The kernel family of a variant-table entry (conv_variants()): what shares a __global__ template and its
    queue code.  The register-staged template's families are told apart by data type and by conv / transposed conv."""
    from dodt_amd import _lib
    f = v['flags']
    if f & _lib.VARIANT_SMALL_CIN:
        return 'small_cin'
    if f & _lib.VARIANT_WINO43:
        return 'wino43'
    if f & _lib.VARIANT_WINO:
        return 'wino22'
    if f & _lib.VARIANT_DECONV_DMA:
        return 'deconv_dma'
    if f & _lib.VARIANT_FIRST2:
        return 'bf16_first2'
    if f & _lib.VARIANT_STREAM:
        return 'bf16_stream'
    if f & _lib.VARIANT_DMA:
        return 'bf16_dma8' if v['th'] == 8 else 'bf16_dma16'
    d = '_deconv' if f & _lib.VARIANT_DECONV else ''
    if f & _lib.VARIANT_SPLIT:
        return 'split' + d
    if f & _lib.VARIANT_BF16:
        return 'bf16_template' + d
    return 'direct' + d


def signature(v):
    """A variant by what it is, not by its place in the table."""
    from dodt_amd import _lib
    names = [(_lib.VARIANT_DECONV, 'deconv'), (_lib.VARIANT_SMALL_CIN, 'small'), (_lib.VARIANT_TAIL_ONLY, 'tail'),
             (_lib.VARIANT_BF16, 'bf16'), (_lib.VARIANT_SPLIT, 'split')]
    return '%s %dx%d bn%d ck%d lds%d%s' % (v['kernel'], v['tw'], v['th'], v['bn'], v['ck'], v['lds_bytes'],
                                           ''.join(' ' + n for bit, n in names if v['flags'] & bit))


def launches(plan):
    """(layer record, 0 main / 1 tail, variant index) of every launch of a plan."""
    return [(r, j, r['variant'][j]) for r in plan for j in (0, 1) if r['variant'][j] >= 0]


# ---- the pinned plans (tests/golden/conv_plans.json) ----------------------------------------------------------

# the non-default modes a data type's plans can feel: fp32 layers take Winograd and the fp32 grouped queues, the
# LDS-DMA transposed conv serves fp32 and bf16 (split stays on the template), the rest is bf16 only
MODES_FELT = {
    'f32': ('wino0', 'wino4', 'deconv_direct', 'one_queue'),
    'f32s': (),
    'bf16': ('deconv_direct', 'bf16_template', 'one_queue', 'no_stream', 'two_launch'),
}
PIN_BATCHES, PIN_CUS = (1, 2, 4, 10), (8, 64, 128, 256)
LAYER_NAMES = ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2',
               'conv4_3', 'upconv3', 'pyramid_fusion3', 'upconv2', 'pyramid_fusion2', 'upconv1', 'pyramid_fusion1']


def pin_configs():
    """Every configuration whose plan is pinned: the cases and the bench rows in their own mode, the bench rows in
    every other mode their data type can feel, the bench shapes over PIN_BATCHES x PIN_CUS."""
    out = list(CASES + BENCH)
    out += [c._replace(mode=m) for c in BENCH for m in MODES_FELT[c.dtype]]
    out += [c._replace(batch=b, cus=n) for c in BENCH if c.batch == 2 for b in PIN_BATCHES for n in PIN_CUS]
    return list(collections.OrderedDict.fromkeys(out))


def pin_record(plan, variants, intern):
    """A plan as the golden file holds it: per layer [main, tail, items, grid, pool_fused, bneck_fused, folded] with
    the two variants as intern(signature) (-1: no launch), never as table indices."""
    assert [r['name'] for r in plan] == LAYER_NAMES[:len(plan)]
    sig = lambda vi: intern(signature(variants[vi])) if vi >= 0 else -1
    return [[sig(r['variant'][0]), sig(r['variant'][1]), r['items'], r['grid'], int(r['pool_fused']),
             int(r['bneck_fused']), int(r['folded'])] for r in plan]


def pinned_plans():
    """What tests/golden/conv_plans.json holds, computed from the library as built: the interned signatures in
    order of first use and {case id: pin_record}."""
    configs = pin_configs()
    got, variants = plans(configs)
    sigs = []

    def intern(s):
        if s not in sigs:
            sigs.append(s)
        return sigs.index(s)
    return dict(signatures=sigs, layers=LAYER_NAMES,
                plans=collections.OrderedDict((case_id(c), pin_record(got[c], variants[c.mode], intern)) for c in configs))


# ---- inputs and weights -------------------------------------------------------------------------------------

def varied_bn(params, seed, unit=1.0):
    """The weights of synth.pyramid_params (bottleneck included) with batch-norm statistics that differ per layer
    and channel: var ~ U(0.25, 4), mean ~ N(0, 0.3) and beta ~ N(0.5, 0.3), the latter two in the input's unit
    (1 for BEV maps, the image's standard deviation for images: He-initialised weights keep the activations at
    the input's scale, and a statistic far below it would not show in any output).  beta centred at 0 leaves a
    fifth of the deep layers' channels dead on the small maps (3 x 5 pixels at 24 x 40) and, by its one draw, the
    whole BEV bottleneck; centred at 0.5, every layer of every case keeps more than 90 % of its channels while
    the ReLU still clips about 30 % of the outputs (test_conv_plan.py checks both).
    synth.pyramid_params has mean 0 and var 1 everywhere: one scale for every channel of every layer, and a
    shift without its mean term."""
    out = {}
    for li, (name, p) in enumerate(params.items()):
        rng = np.random.default_rng(seed + 7919 * (li + 1))
        n = p['beta'].shape[0]
        out[name] = dict(w=p['w'],
                         var=rng.uniform(0.25, 4.0, size=n).astype(np.float32),
                         mean=(unit * rng.normal(0, 0.3, size=n)).astype(np.float32),
                         beta=(unit * rng.normal(0.5, 0.3, size=n)).astype(np.float32))
    return out


IMAGE_STD = 60.0


def net_params(net, varied=True):
    """A net's weights: synth.pyramid_params with the seeds every parity test uses, with varied_bn's statistics."""
    from dodt_amd import synth
    bev = net.startswith('bev')
    p = synth.pyramid_params(6 if bev else 3, seed=42 if bev else 142, plain=NETS[net]['plain'])
    return varied_bn(p, seed=1000 + (0 if bev else 1), unit=1.0 if bev else IMAGE_STD) if varied else p


def case_params(c):
    return net_params(c.net)


def case_input(c):
    """Dense input of a case, (batch, h, w, channels) without the pad rows: BEV-like uniform with about 30 % zeros,
    image-like normal with standard deviation 60."""
    n = NETS[c.net]
    h = c.H - n['pad_top']
    rng = np.random.default_rng(c.H * 10007 + c.W * 101 + c.batch)
    if c.net.startswith('bev'):
        x = rng.uniform(0, 1, size=(c.batch, h, c.W, 6)).astype(np.float32)
        x[rng.uniform(size=x.shape) < 0.3] = 0
        return x
    return rng.normal(0, IMAGE_STD, size=(c.batch, h, c.W, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle(c_key):
    """The oracle's maps of a case's input: ({layer: (batch, h, w, c)}, feature maps, bottleneck).  Keyed by what the
    oracle depends on, (net, dtype, H, W, batch, first layers folded), so that the cases and modes that share an
    input share the result; callers must not write into it."""
    from oracle import extractors as oext
    net, dtype, H, W, batch, folded = c_key
    c = Case(net, dtype, H, W, batch, 8, 'default')
    x, params, n = case_input(c), case_params(c), NETS[net]
    maps, feats, bns = {}, [], []
    for f in range(batch):
        col = {}
        if n['plain']:
            feat = oext.vgg_plain(x[f], params, collect=col)
        else:
            feat = oext.vgg_pyramid(x[f], params, pad_top=n['pad_top'], collect=col,
                                    conv_dtype='bf16' if dtype == 'bf16' else 'f32',
                                    first_layer='split' if folded else 'fp32')
        for k, v in col.items():
            maps.setdefault(k, []).append(v)
        feats.append(feat)
        bns.append(oext.bottleneck_1x1(feat, params['bottleneck']))
    return {k: np.stack(v) for k, v in maps.items()}, np.stack(feats), np.stack(bns)


def oracle_key(c, folded=False):
    # (split mode claims the fp32 oracle)
    return (c.net, 'bf16' if c.dtype == 'bf16' else 'f32', c.H, c.W, c.batch, bool(folded) and c.dtype == 'bf16')
