"""The fp32 F(2x2,3x3) Winograd kernel computes the same BITS as when tests/golden/wino22_bits.json was recorded.
Needs an MI355X.

wino3x3_f32_kernel's K loop is hand-ordered (wino_kernels.h): the order of its instructions, the registers of its
accumulators and the start of an item's accumulation (SrcC = 0 in the first chunk, nothing zeroed) may change, the
operations per accumulator and their order may not -- so every output map of a net that runs on it keeps its bytes.
The golden file holds the sha256 and the shape of every layer's map, the returned feature map and the bottleneck
per case (tests/golden/make_wino22_bits.py wrote it on the device from the library as it was BEFORE the K loop was
pinned); this test asserts the same digests from the tree's library.

Cases, seeded inputs and per-channel batch-norm from tests/_conv_cases.py: few items and queues without items;
ragged tiles at every level with up to nine items per workgroup (an item after the first must not see the previous
item's sums); one queue per launch (a child process: the library reads its switches once); the image net.  Together
4 to 32 chunks per item, fused pools, the NHWC and the bottleneck epilogue."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_cases as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'wino22_bits.json')

CASES = [
    cc.Case('bev', 'f32', 24, 40, 2, 8, 'default'),
    cc.Case('bev', 'f32', 200, 264, 3, 8, 'default'),
    cc.Case('bev', 'f32', 200, 72, 1, 8, 'one_queue'),
    cc.Case('img', 'f32', 32, 48, 1, 8, 'default'),
]


def digests(c):
    """{map name: [sha256 of its bytes, shape]} of a case run in this process (whose environment must be the
    case's mode): every layer's map, the returned feature map, the bottleneck."""
    from dodt_amd import device
    from dodt_amd.core.feature_extractors import vgg_pyramid
    assert all(os.environ.get(k) == v for k, v in cc.MODES[c.mode].items())
    ctx = device.Context(plan_cus=c.cus)
    ex = {'bev': vgg_pyramid.BevVggPyr, 'img': vgg_pyramid.ImgVggPyr}[c.net](ctx=ctx, shared_gpu=c.shared,
                                                                             conv_dtype=c.dtype)
    try:
        ex.load_params(cc.case_params(c))
        feat, ends = ex.build(cc.case_input(c), with_bottleneck=True)
        plan = ex.plan()
        variants = vgg_pyramid.conv_variants()
        on_wino22 = [r['name'] for r, _, vi in cc.launches(plan) if cc.family(variants[vi]) == 'wino22']
        assert len(on_wino22) >= 8, 'the case does not run on the F(2x2) kernel: %s' % on_wino22
        names = [r['name'] for r in plan if not r['folded']]
        names.remove('pyramid_fusion1')        # the returned map
        maps = [(n, ex.activation(n)) for n in names] + [('feature_maps', feat), ('bottleneck', ends['bottleneck'])]
    finally:
        ex.close()
        ctx.close()
    return {n: [hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest(), list(m.shape)] for n, m in maps}


def run_mode(mode):
    """Every case of a mode, in this process: prints 'BITS ' + {case id: digests}."""
    print('BITS ' + json.dumps({cc.case_id(c): digests(c) for c in CASES if c.mode == mode}))


def digests_in_child(mode):
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_wino22_bits as t; '
            't.run_mode(%r)' % (ROOT, os.path.join(ROOT, 'tests'), mode))
    r = subprocess.run([sys.executable, '-c', code], env=cc.mode_env(mode), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('BITS ')][-1][5:])


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)['cases']


def _compare(cid, got):
    want = _golden()[cid]
    assert sorted(got) == sorted(want)
    differ = [n for n in want if got[n] != want[n]]
    print('%s: %d maps, %d differ' % (cid, len(want), len(differ)))
    assert not differ, '%s: other bytes than recorded in %s' % (cid, differ)


DEFAULT = [c for c in CASES if c.mode == 'default']


@pytest.mark.parametrize('case', DEFAULT, ids=[cc.case_id(c) for c in DEFAULT])
def test_every_map_has_the_recorded_bytes(case):
    assert not [k for k in os.environ if k.startswith(cc.CONV_SWITCH_PREFIX)], 'the default mode has no switch set'
    _compare(cc.case_id(case), digests(case))


@pytest.mark.parametrize('mode', sorted({c.mode for c in CASES} - {'default'}))
def test_every_map_has_the_recorded_bytes_in_other_modes(mode):
    got = digests_in_child(mode)
    assert sorted(got) == [cc.case_id(c) for c in CASES if c.mode == mode]
    for cid, d in got.items():
        _compare(cid, d)
