"""The case table of the fully connected layers' tests, and the helpers both of them share.

tests/test_fc_plan.py (no GPU) proves on the host's plan (ops.fc_plan_host: the library's own selector) that these
cases reach every kernel form and instantiation of csrc/gemm.hip, take every fallback of the selector, cut ragged tiles
and rows by the device count -- and that each case's comparison rejects a reference with a k lost, two k swapped or an
edge zeroed; tests/test_gpu_fc_forms.py runs the same cases on the device.

Data kinds.  'int': x, x2, w, b integers in [-8, 8] (the fused mean then a multiple of 0.5; all exact in bf16):
|sum| <= 64 K + 8 < 2^24 for K <= 2048, so every float32 summation order gives the bits of the float64 product rounded
once, and the comparison is np.array_equal.  'normal': the data and the bars of tests/test_gpu_heads.py (1e-4 of the
output scale; bf16 output within half a bf16 ulp of it).

Poison.  x and x2 hold NaN in the columns from K (bf16 rows: from the layer's row elements, which must be zero up to
there) to ldx and in the rows from the resolved row count on; y has three more rows than M and ldy > N where the entry
takes a stride, prefilled with a NaN bit pattern of which no bit may change outside [:rows, :N]."""
import collections
import functools
import zlib

import numpy as np

from dodt_amd import ops
from oracle import heads as oheads
from oracle import tfops

Y_EXTRA_ROWS = 3
SENTINEL32 = np.uint32(0x7fa5a5a5)     # NaNs with a payload no kernel produces
SENTINEL16 = np.uint16(0x7fa5)
NAN16 = np.uint16(0x7fc0)
MAX_WORK = 32705 * 64 * 128            # M K N of the largest case

# entry: 'forward' | 'split' (forward_split, widths) | 'bf16' (forward_bf16, y_bf16) | 'split_bf16'
# x_off, x2_off, y_off: bytes added to 256-byte aligned allocations; d_m: None or the device row count
# expect: the selector's form; xvec / fuse: fc_mfma_kernel's instantiation where the form is a register-staged one
Case = collections.namedtuple(
    'Case', 'name M K N dtype relu fuse ldx ldy x_off x2_off y_off d_m entry widths y_bf16 data expect xvec')


def case(name, M, K, N, expect, dtype='f32', relu=False, fuse=False, ldx=None, ldy=None, x_off=0, x2_off=0, y_off=0,
         d_m=None, entry='forward', widths=None, y_bf16=False, data='int', xvec=None):
    if ldx is None:
        ldx = K
    if entry in ('split', 'split_bf16'):
        assert sum(widths) == N and ldy is None
        ldy = 0
    elif ldy is None:
        ldy = N + (8 if entry == 'bf16' else 4)
    return Case(name, M, K, N, dtype, relu, fuse, ldx, ldy, x_off, x2_off, y_off, d_m, entry, widths, y_bf16, data,
                expect, xvec)


def _both(name, M, K, N, expect, **kw):
    """A case on a float32 layer and on a bf16 layer (float32 rows): expect / xvec are (f32, bf16) pairs."""
    xv = kw.pop('xvec', (None, None))
    return [case(name + '-f32', M, K, N, expect[0], dtype='f32', xvec=xv[0], **kw),
            case(name + '-bf16', M, K, N, expect[1], dtype='bf16', xvec=xv[1], **kw)]


def _d_m(base, cuts):
    """The case `base` once more per device row count of `cuts` (same layer, same rows)."""
    return [base._replace(name='%s-dm%d' % (base.name, v), d_m=v) for v in cuts]


T32, T32B, T128, T128B = 'kTiled128x32', 'kTiled128x32Bf16', 'kTiled64x128', 'kTiled64x128Bf16'

CASES = []

# ---- fc_smallk_kernel (K <= 16, N >= 64, N % 4 == 0, y 16-byte aligned) and what falls off it --------------------
CASES += _both('smallk-37x9x64', 37, 9, 64, ('kSmallK', 'kSmallK'), relu=True, ldx=10)
CASES += _both('smallk-37x16x68-fused', 37, 16, 68, ('kSmallK', 'kSmallK'), fuse=True, ldx=20)   # three 32-wide bias blocks
CASES += _both('smallk-1x1x64', 1, 1, 64, ('kSmallK', 'kSmallK'), ldx=4)
CASES += _both('smallk-37x9x64-ldy65', 37, 9, 64, ('kSmallK', 'kSmallK'), ldy=65)               # scalar row store
CASES += _both('smallk-yoff4-37x9x64', 37, 9, 64, (T32, T32B), y_off=4, xvec=(0, 0))
CASES += _both('smallk-yoff4-37x9x128', 37, 9, 128, (T128, T128B), y_off=4, xvec=(0, 0))
CASES += _both('smallk-n66-37x12x66', 37, 12, 66, (T32, T32B), xvec=(1, 0))                       # N % 4 != 0: three n-tiles
_smallk = case('smallk-dm-37x9x64', 37, 9, 64, 'kSmallK', relu=True, ldx=10)
CASES += _d_m(_smallk, (0, 20, 37, 42)) + _d_m(_smallk._replace(name='smallk-dm-37x9x64-bf16', dtype='bf16'), (20,))
CASES += [case('smallk-normal-37x16x68-fused', 37, 16, 68, 'kSmallK', fuse=True, relu=True, data='normal'),
          case('smallk-normal-37x9x64-bf16', 37, 9, 64, 'kSmallK', dtype='bf16', data='normal')]

# ---- fc_skinny_kernel (N <= 32, K % 16 == 0, rows 16-byte aligned, one input) ------------------------------------
for _n, (_M, _K, _N, _kw) in enumerate([
        (1, 16, 1, {}),                       # one step, seven idle waves
        (15, 144, 16, {}),                    # nine steps: wave 0 takes two
        (16, 528, 17, dict(relu=True)),       # 33 steps: two rounds of the four-step unroll
        (17, 144, 32, dict(ldx=148)),
        (33, 16, 32, dict(ldx=20))]):
    CASES += _both('skinny%d-%dx%dx%d' % (_n, _M, _K, _N), _M, _K, _N, ('kSkinny', 'kSkinnyBf16'), **_kw)
CASES += [
    # rows that are bf16 already: 8-byte aligned rows do
    case('skinny-bf16_rows-33x144x17-xoff8', 33, 144, 17, 'kSkinnyBf16Rows', dtype='bf16', entry='bf16', ldx=148,
         x_off=8, ldy=21),
    case('skinny-bf16_rows-16x528x32', 16, 528, 32, 'kSkinnyBf16Rows', dtype='bf16', entry='bf16', relu=True, ldy=36),
    case('skinny-bf16_rows-split-33x144x17', 33, 144, 17, 'kSkinnyBf16Rows', dtype='bf16', entry='split_bf16',
         widths=(2, 13, 2), ldx=148, x_off=8),
]
for _dt, _form in (('f32', 'kSkinny'), ('bf16', 'kSkinnyBf16')):
    CASES += [case('skinny-split1-33x144x3-%s' % _dt, 33, 144, 3, _form, dtype=_dt, entry='split', widths=(3,)),
              case('skinny-split2-17x16x8-%s' % _dt, 17, 16, 8, _form, dtype=_dt, entry='split', widths=(2, 6), ldx=20),
              case('skinny-split3-33x144x32-%s' % _dt, 33, 144, 32, _form, dtype=_dt, entry='split',
                   widths=(1, 30, 1), ldx=148)]
# the selector's fallbacks of a skinny layer: the 128 x 32 register-staged kernel
CASES += _both('skinny-x2-33x16x17', 33, 16, 17, (T32, T32B), fuse=True, xvec=(1, 1))
CASES += _both('skinny-ldx17-33x16x17', 33, 16, 17, (T32, T32B), ldx=17, xvec=(0, 0))
CASES += _both('skinny-xoff4-33x16x17', 33, 16, 17, (T32, T32B), ldx=20, x_off=4, xvec=(1, 1))
_skinny = case('skinny-dm-33x144x17', 33, 144, 17, 'kSkinny')
CASES += _d_m(_skinny, (0, 20, 33, 38))
CASES += _d_m(_skinny._replace(name='skinny-dm-split-33x144x17', entry='split', widths=(2, 13, 2), ldy=0), (0, 20))
CASES += _d_m(case('skinny-bf16_rows-dm-33x144x17', 33, 144, 17, 'kSkinnyBf16Rows', dtype='bf16', entry='bf16'), (20,))
CASES += [case('skinny-normal-33x528x17', 33, 528, 17, 'kSkinny', data='normal'),
          case('skinny-normal-33x528x17-bf16', 33, 528, 17, 'kSkinnyBf16', dtype='bf16', data='normal'),
          case('skinny-bf16_rows-normal-33x528x17', 33, 528, 17, 'kSkinnyBf16Rows', dtype='bf16', entry='bf16',
               data='normal')]

# ---- fc_mfma_kernel, 128 x 32 tiles (N < 128): vector / scalar loads x plain / fused, float32 and bf16 ------------
# K = 40 / 41 / 64 / 65: loads by float4 and by element, exactly one and just over one padded stage
CASES += _both('t32-127x40x33', 127, 40, 33, (T32, T32B), ldx=44, xvec=(1, 1))          # second n-tile: one column
CASES += _both('t32-128x41x100-fused', 128, 41, 100, (T32, T32B), fuse=True, relu=True, ldx=43, xvec=(0, 0))
CASES += _both('t32-129x64x100-fused', 129, 64, 100, (T32, T32B), fuse=True, xvec=(1, 1))   # ragged fourth n-tile
CASES += _both('t32-129x65x33', 129, 65, 33, (T32, T32B), relu=True, ldx=68, xvec=(0, 0))
CASES += _both('t32-129x44x33', 129, 44, 33, (T32, T32B), xvec=(1, 0))                  # K % 8 != 0: bf16 by element
_t32 = case('t32-dm-129x64x100', 129, 64, 100, T32, xvec=1)
CASES += _d_m(_t32, (0, 100, 129, 134)) + _d_m(_t32._replace(name='t32-dm-129x64x100-bf16', dtype='bf16', expect=T32B), (100,))
CASES += [case('t32-normal-129x65x100-fused', 129, 65, 100, T32, fuse=True, relu=True, data='normal', xvec=0),
          case('t32-normal-129x64x100-bf16', 129, 64, 100, T32B, dtype='bf16', data='normal', xvec=1)]

# ---- fc_mfma_kernel, 64 x 128 tiles (N >= 128; float32: K no multiple of 32, or below two stages) ----------------
CASES += _both('t128-63x32x128', 63, 32, 128, (T128, T128B), xvec=(1, 1))
CASES += _both('t128-64x36x129-fused', 64, 36, 129, (T128, T128B), fuse=True, ldx=40, xvec=(1, 0))
CASES += _both('t128-65x37x200', 65, 37, 200, (T128, T128B), relu=True, ldx=38, xvec=(0, 0))
CASES += _both('t128-65x100x200-fused', 65, 100, 200, (T128, T128B), fuse=True, relu=True, xvec=(1, 0))
CASES += _both('t128-64x37x129-fused', 64, 37, 129, (T128, T128B), fuse=True, xvec=(0, 0))
CASES += _both('t128-65x32x200-fused', 65, 32, 200, (T128, T128B), fuse=True, xvec=(1, 1))
# the selector's fallbacks of a layer that has the LDS-DMA kernel
CASES += [case('t128-xoff4-65x64x128', 65, 64, 128, T128, ldx=68, x_off=4, xvec=1),
          case('t128-ldx65-65x64x128', 65, 64, 128, T128, ldx=65, xvec=0),
          case('t128-x2off4-65x64x128', 65, 64, 128, T128, fuse=True, x2_off=4, xvec=1)]
_t128 = case('t128-dm-65x37x200', 65, 37, 200, T128, xvec=0)
CASES += _d_m(_t128, (0, 40, 65, 70)) + _d_m(_t128._replace(name='t128-dm-65x37x200-bf16', dtype='bf16', expect=T128B), (40,))
CASES += [case('t128-normal-65x100x200-fused', 65, 100, 200, T128, fuse=True, data='normal', xvec=1),
          case('t128-normal-65x100x200-bf16', 65, 100, 200, T128B, dtype='bf16', relu=True, data='normal', xvec=0)]

# ---- fc_dma_kernel<false, 1>: 2, 3, 4, 5 stages of the three-deep ring ------------------------------------------
CASES += [case('dma1-1x64x128', 1, 64, 128, 'kDmaNt1'),
          case('dma1-63x96x130', 63, 96, 130, 'kDmaNt1', relu=True),       # the last 64-column tile stores nothing
          case('dma1-65x128x200', 65, 128, 200, 'kDmaNt1', ldx=132),
          case('dma1-130x160x256', 130, 160, 256, 'kDmaNt1', relu=True),    # 12 tiles
          case('dma1-128x128x256', 128, 128, 256, 'kDmaNt1')]               # 8 tiles: the XCD map
CASES += _d_m(case('dma1-dm-130x160x256', 130, 160, 256, 'kDmaNt1', relu=True), (0, 70, 130, 135))
CASES += [case('dma1-normal-130x160x200', 130, 160, 200, 'kDmaNt1', data='normal')]
# ---- fc_dma_kernel<true, 1> ---------------------------------------------------------------------------------------
CASES += [case('dmaf-65x160x200', 65, 160, 200, 'kDmaFused', fuse=True, relu=True, ldx=164),
          case('dmaf-130x64x128', 130, 64, 128, 'kDmaFused', fuse=True)]
CASES += _d_m(case('dmaf-dm-130x64x128', 130, 64, 128, 'kDmaFused', fuse=True), (0, 70, 130, 135))
CASES += [case('dmaf-normal-65x160x200', 65, 160, 200, 'kDmaFused', fuse=True, data='normal')]
# ---- fc_dma_kernel<false, 2> and its threshold of 512 tiles of 64 x 128 ------------------------------------------
CASES += [case('dma2-4040x64x1024', 4040, 64, 1024, 'kDmaNt2', relu=True),          # 512 tiles: the XCD map
          case('dma2-3648x64x1100', 3648, 64, 1100, 'kDmaNt2', ldx=68),             # 513 tiles, ragged N
          case('dma1-32704x64x128', 32704, 64, 128, 'kDmaNt1'),                     # 511 tiles of 64 x 128
          case('dma2-32705x64x128', 32705, 64, 128, 'kDmaNt2')]                     # 512
CASES += _d_m(case('dma2-dm-3648x64x1100', 3648, 64, 1100, 'kDmaNt2', ldx=68), (0, 3600, 3648, 3653))
CASES += [case('dma2-normal-3648x64x1100', 3648, 64, 1100, 'kDmaNt2', ldx=68, relu=True, data='normal')]

# ---- fc_bf16_dma_kernel: bf16 rows made by ops.rows_to_bf16, float32 and bf16 output ------------------------------
BF16_ROWS = {32: 'kBf16RowsDma32', 64: 'kBf16RowsDma64'}      # by DODT_FC_BF16_DMA_BK of the process
for _M, _K, _N, _relu in [(65, 128, 128, False), (65, 129, 256, True),     # Kd = 192: the tail is zero
                          (1, 160, 128, False), (130, 2048, 128, True)]:
    for _yb in (False, True):
        CASES.append(case('bf16_rows-%dx%dx%d-y%s' % (_M, _K, _N, 'bf16' if _yb else 'f32'), _M, _K, _N,
                          'kBf16RowsDma32', dtype='bf16', entry='bf16', y_bf16=_yb, relu=_relu,
                          ldx=-(-_K // 64) * 64 + 8))
_rows = case('bf16_rows-dm-130x2048x128', 130, 2048, 128, 'kBf16RowsDma32', dtype='bf16', entry='bf16', y_bf16=True,
             relu=True, ldx=2048)
CASES += _d_m(_rows, (0, 70, 130, 135))
CASES += [case('bf16_rows-normal-130x2048x128-ybf16', 130, 2048, 128, 'kBf16RowsDma32', dtype='bf16', entry='bf16',
               y_bf16=True, ldx=2056, data='normal'),
          case('bf16_rows-normal-65x129x256-yf32', 65, 129, 256, 'kBf16RowsDma32', dtype='bf16', entry='bf16',
               relu=True, ldx=200, data='normal')]
# bf16 rows no kernel of the layer reads: planned kNone and refused before any launch
REFUSED = [case('bf16_rows-refused-k120', 65, 120, 128, 'kNone', dtype='bf16', entry='bf16', ldx=128),
           case('bf16_rows-refused-n130', 65, 128, 130, 'kNone', dtype='bf16', entry='bf16', ldx=128),
           case('bf16_rows-refused-skinny-ybf16', 33, 144, 17, 'kNone', dtype='bf16', entry='bf16', y_bf16=True)]

assert len(set(c.name for c in CASES + REFUSED)) == len(CASES) + len(REFUSED)

# The workload's own layer calls at 1024 proposals (core/models/anchor_predictor.py on 5500 anchors, core/
# avod_fc_layers/fusion_fc_layers.py for the stage-2 head and the correlation head on proposals and on 100 detections):
# (what, K, N, M, dtype, keywords of ops.fc_plan_host).
WORKLOAD = []
for _dt in ('f32', 'bf16'):
    WORKLOAD += [
        ('rpn fc6 [cls | reg], mean inside', 9, 512, 5500, _dt, dict(x2_off=0)),
        ('rpn cls_fc7', 256, 256, 5500, _dt, dict(ldx=512, ldy=512)),
        ('rpn reg_fc7', 256, 256, 5500, _dt, dict(ldx=512, ldy=512, x_off=1024 % 16, y_off=1024 % 16)),
        ('rpn fc8 as one split layer', 512, 8, 5500, _dt, dict(y_off=0)),
    ]
WORKLOAD += [
    ('avod fc6 on the fused rows', 1568, 2048, 1024, 'f32', {}),
    ('avod fc7 / fc8, corr fc7 / fc8', 2048, 2048, 1024, 'f32', {}),
    ('avod cls | off | ang', 2048, 14, 1024, 'f32', {}),
    ('corr fc6, K padded to 1248', 1248, 2048, 1024, 'f32', {}),
    ('corr off_out', 2048, 3, 1024, 'f32', {}),
    ('corr fc6 on detections', 1248, 2048, 100, 'f32', {}),
    ('corr fc7 / fc8 on detections', 2048, 2048, 100, 'f32', {}),
    ('corr off_out on detections', 2048, 3, 100, 'f32', {}),
    ('avod fc6 on bf16 rows', 1568, 2048, 1024, 'bf16', dict(x_bf16=True, y_bf16=True, ldx=1600)),
    ('avod fc7 / fc8, corr fc7 / fc8 on bf16 rows', 2048, 2048, 1024, 'bf16', dict(x_bf16=True, y_bf16=True)),
    ('avod cls | off | ang on bf16 rows', 2048, 14, 1024, 'bf16', dict(x_bf16=True)),
    ('corr fc6 on bf16 rows', 1248, 2048, 1024, 'bf16', dict(x_bf16=True, y_bf16=True, ldx=1280)),
    ('corr off_out on bf16 rows', 2048, 3, 1024, 'bf16', dict(x_bf16=True)),
    ('corr fc6 on bf16 rows of detections', 1248, 2048, 100, 'bf16', dict(x_bf16=True, y_bf16=True, ldx=1280)),
]


# ---- plans ----------------------------------------------------------------------------------------------------------

def host_plan(c, bf16_bk=32):
    """The library's plan of a case's call (ops.fc_plan_host), host only."""
    split = c.entry in ('split', 'split_bf16')
    return ops.fc_plan_host(c.K, c.N, c.M, dtype=c.dtype, ldx=c.ldx, ldy=c.ldy, x_off=c.x_off % 16,
                            x2_off=c.x2_off % 16 if c.fuse else None, y_off=0 if split else c.y_off % 16,
                            x_bf16=c.entry in ('bf16', 'split_bf16'), y_bf16=c.y_bf16, bf16_bk=bf16_bk)


def expected_form(c, bf16_bk=32):
    return BF16_ROWS[bf16_bk] if c.expect == 'kBf16RowsDma32' else c.expect


GROUPS = ('smallk', 'skinny', 'dma_nt1', 'dma_nt2', 'dma_fused', 'bf16_rows_dma', 'tiled')


def group(form):
    """The kernel a form runs on, the three fc_dma_kernel instances apart."""
    if form.startswith('kSkinny'):
        return 'skinny'
    if form.startswith('kTiled'):
        return 'tiled'
    if form.startswith('kBf16RowsDma'):
        return 'bf16_rows_dma'
    return {'kSmallK': 'smallk', 'kDmaNt1': 'dma_nt1', 'kDmaNt2': 'dma_nt2', 'kDmaFused': 'dma_fused'}[form]


def instantiation(plan, dtype, fuse):
    """The kernel instantiation a plan launches, in gemm.hip's template arguments; None for kNone."""
    f = plan['name']
    if f == 'kNone':
        return None
    if f.startswith('kTiled'):
        assert bool(plan['fuse']) == bool(fuse)
        return 'fc_mfma_kernel<%s, XVEC=%d, FUSE=%d, BF16=%d>' % (
            '64x128' if '64x128' in f else '128x32', plan['xvec'], plan['fuse'], f.endswith('Bf16'))
    if f.startswith('kDma'):
        return 'fc_dma_kernel<FUSE=%d, NT=%d>' % (f == 'kDmaFused', 2 if f == 'kDmaNt2' else 1)
    if f.startswith('kBf16RowsDma'):
        return 'fc_bf16_dma_kernel<YBF16=%d, BK=%d>' % (plan['y_bf16'], plan['dma_bk'])
    if f.startswith('kSkinny'):
        return 'fc_skinny_kernel<BF16=%d, XB16=%d>' % (f != 'kSkinny', f == 'kSkinnyBf16Rows')
    assert f == 'kSmallK'
    return 'fc_smallk_kernel<BF16=%d>' % (dtype == 'bf16')


ALL_INSTANTIATIONS = sorted(
    ['fc_mfma_kernel<%s, XVEC=%d, FUSE=%d, BF16=%d>' % (t, v, f, b)
     for t in ('64x128', '128x32') for v in (0, 1) for f in (0, 1) for b in (0, 1)] +
    ['fc_dma_kernel<FUSE=0, NT=1>', 'fc_dma_kernel<FUSE=0, NT=2>', 'fc_dma_kernel<FUSE=1, NT=1>'] +
    ['fc_bf16_dma_kernel<YBF16=%d, BK=%d>' % (y, k) for y in (0, 1) for k in (32, 64)] +
    ['fc_skinny_kernel<BF16=0, XB16=0>', 'fc_skinny_kernel<BF16=1, XB16=0>', 'fc_skinny_kernel<BF16=1, XB16=1>'] +
    ['fc_smallk_kernel<BF16=0>', 'fc_smallk_kernel<BF16=1>'])
assert len(ALL_INSTANTIATIONS) == 28


# ---- data and references --------------------------------------------------------------------------------------------

def layer_key(c):
    """Cases of one key run on one layer object, back to back."""
    return (c.K, c.N, c.dtype, c.relu, c.data)


# Every draw starts from this.  Any value serves with which tests/test_fc_plan.py's mutant proofs pass: they are what
# keeps a degenerate draw out (a one-row case whose first and last k happen to be equal, a last column that sums to 0).
SEED = 5


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr((SEED,) + key).encode('ascii')))


@functools.lru_cache(maxsize=None)
def layer_params(key):
    K, N, _, _, data = key
    rng = _rng('layer', key)
    if data == 'int':
        return (rng.integers(-8, 9, size=(K, N)).astype(np.float32), rng.integers(-8, 9, size=N).astype(np.float32))
    return (rng.normal(0, np.sqrt(2.0 / K), size=(K, N)).astype(np.float32),
            rng.normal(0, 0.1, size=N).astype(np.float32))


def rows_key(c):
    """Cases that differ in the device row count, the strides or the offsets only share their rows."""
    return (c.M, c.fuse) + layer_key(c)


@functools.lru_cache(maxsize=8)
def _inputs(key):
    M, fuse, K, data = key[0], key[1], key[2], key[-1]
    rng = _rng('rows', key)
    draw = (lambda: rng.integers(-8, 9, size=(M, K)).astype(np.float32)) if data == 'int' else \
        (lambda: rng.normal(size=(M, K)).astype(np.float32))
    x = draw()
    return x, (draw() if fuse else None)


def case_inputs(c):
    """x (M, K) and x2 (or None), float32."""
    return _inputs(rows_key(c))


def fused_rows(c):
    x, x2 = case_inputs(c)
    return oheads.mean_fusion(x, x2) if c.fuse else x


def rows(c):
    """The rows a call computes: M cut by the device count."""
    return c.M if c.d_m is None else max(0, min(c.d_m, c.M))


@functools.lru_cache(maxsize=8)
def _reference(key, dtype, relu):
    M, fuse = key[0], key[1]
    c = case('ref', M, key[2], key[3], None, dtype=dtype, relu=relu, fuse=fuse, data=key[-1])
    w, b = layer_params(layer_key(c))
    return oheads.fc(fused_rows(c), w, b, relu, dtype=dtype)


def reference(c):
    """(M, N) float32: the float64 product rounded once (oracle/heads.py), all M rows."""
    return _reference(rows_key(c), c.dtype, c.relu)


def output_value(c, want):
    """What the entry stores of the float32 reference."""
    return tfops.round_bf16(want) if c.y_bf16 else want


def accepts(c, got, want):
    """The case's own comparison of the valid region, got against the float32 reference `want`: equality for 'int'
    data, the bars of tests/test_gpu_heads.py for 'normal' data."""
    if got.shape != want.shape:
        return False
    if got.size == 0:
        return True
    if c.data == 'int':
        return bool(np.array_equal(got, output_value(c, want)))
    scale = np.abs(want).max() + 1e-12
    if c.y_bf16:
        return bool((np.abs(got - want) <= 2.0 ** -8 * np.abs(want) * 1.001 + 1e-4 * scale).all() and
                    np.array_equal(got, tfops.round_bf16(got)))
    return bool(np.abs(got - want).max() <= 1e-4 * scale)


# ---- the images of a call's arrays (host side; the device test uploads and downloads them) -------------------------

def x_row_elems(c, row_elems=0):
    """Elements of an x row the kernel may read: K, or the layer's bf16 row elements (zero from K on)."""
    return max(c.K, row_elems) if c.entry in ('bf16', 'split_bf16') else c.K


def x_image(c, values, row_elems=0):
    """(M + 1, ldx) float32, or uint16 for bf16 rows: `values` (M, row elements) in the resolved rows, NaN in the
    padding columns and in every row from the resolved count on."""
    n, cols = rows(c), x_row_elems(c, row_elems)
    assert values.shape == (c.M, cols) and c.ldx >= cols
    if values.dtype == np.uint16:
        img = np.full((c.M + 1, c.ldx), NAN16, np.uint16)
    else:
        img = np.full((c.M + 1, c.ldx), np.nan, np.float32)
    img[:n, :cols] = values[:n]
    return img


def y_shapes(c):
    """Per output array: (allocated rows, row stride, columns written)."""
    if c.entry in ('split', 'split_bf16'):
        return [(c.M + Y_EXTRA_ROWS, w, w) for w in c.widths]
    return [(c.M + Y_EXTRA_ROWS, c.ldy, c.N)]


def y_sentinel(c):
    return SENTINEL16 if c.y_bf16 else SENTINEL32


def y_values(c, image):
    """The float32 values of a downloaded output image (raw bits)."""
    return ops.bf16_to_float(image) if c.y_bf16 else image.view(np.float32)


def check_outputs(c, images, want):
    """images: the raw bits of every output array after the call.  Nothing outside [:rows, :columns] changed, and the
    case's comparison accepts what is inside.  Returns a list of complaints (empty: the case passes)."""
    bad, n, c0 = [], rows(c), 0
    for (alloc, ld, cols), img in zip(y_shapes(c), images):
        assert img.shape == (alloc, ld)
        if (img[n:] != y_sentinel(c)).any():
            bad.append('rows from %d on were written' % n)
        if (img[:n, cols:] != y_sentinel(c)).any():
            bad.append('columns from %d on were written' % cols)
        if not accepts(c, y_values(c, np.ascontiguousarray(img[:n, :cols])), want[:n, c0:c0 + cols]):
            bad.append('columns %d..%d differ from the reference' % (c0, c0 + cols))
        c0 += cols
    return bad


def expected_images(c, want):
    """The images a correct call leaves ('int' data: exactly these)."""
    out, n, c0 = [], rows(c), 0
    for alloc, ld, cols in y_shapes(c):
        v = np.ascontiguousarray(output_value(c, want[:n, c0:c0 + cols]), np.float32)
        img = np.full((alloc, ld), y_sentinel(c), np.uint16 if c.y_bf16 else np.uint32)
        img[:n, :cols] = (v.view(np.uint32) >> 16).astype(np.uint16) if c.y_bf16 else v.view(np.uint32)
        out.append(img)
        c0 += cols
    return out
