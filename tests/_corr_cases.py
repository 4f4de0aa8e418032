"""The correlation tests' shared pieces: a float64 reference with a derived element-wise bound, a model of
correlation_sp_kernel's tile walk, the case table, the tile-list rule in numpy, and the child runner.

tests/test_corr_walk.py (no GPU) proves on the model that the cases reach the persistent workgroups' second and later
tiles in every way the kernel distinguishes; tests/test_gpu_correlation.py runs them on the device.  The library reads
its DODT_CORR_* switches once per process, so everything of one mode runs in one child process (run_mode), which
writes what the device returned into an .npz; the parent compares.

Tolerance.  An output is 1/32 * sum of 32 products.  Any float32 evaluation -- fused or unfused multiply-adds, one
chain or two chains added at the end, any order -- has at most 33 roundings on the path of a term (32 multiply-adds
of a chain, one add of two chains; the scale by 1/32 is exact), so |got - exact| <= gamma_33 * 1/32 sum |a b| with
gamma_33 = 33 u / (1 - 33 u) < 34 u, u = 2^-24.  bound() is that, element by element, plus 1e-30 where the magnitude is
0.  Maps of small integers make every product and partial sum an integer below 2^24 and the scale exact: any correct
kernel equals the reference bit for bit."""
import collections
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32 = np.float32, np.int32

C = 32                  # channels: the only depth the kernels take
ROI = 7                 # crop samples per axis (dodt_amd.pipeline.ROI)
TILE = 16               # correlation_sp_kernel's tile edge
GUARD = 4096            # floats behind every output buffer that must keep their NaN
DEFAULT_GRID = 512      # 2 * 256 CUs


# ---- reference ---------------------------------------------------------------------------------------------------
def out_shape(H, W, md, s2, pad):
    gw = 2 * (md // s2) + 1
    return H + 2 * pad - 2 * md, W + 2 * pad - 2 * md, gw * gw


def reference(a, b, md, s2, pad, rows=None):
    """(out, mag) in float64: out[y,x,k] = 1/C sum_c Apad[y+d, x+d, c] * Bpad[y+d+s2p, x+d+s2o, c], k as in
    oracle/tfops.correlation, mag the same sum over |A B|.  rows = (y0, y1): only output rows y0 .. y1 - 1, from
    only the input rows they read."""
    H, W, ch = a.shape
    r = md // s2
    gw, R = 2 * r + 1, r * s2
    OH, OW, K = out_shape(H, W, md, s2, pad)
    y0, y1 = (0, OH) if rows is None else rows
    assert 0 <= y0 <= y1 <= OH
    n = y1 - y0
    p0, p1 = y0 + md - R, y1 + md + R              # rows of the padded maps the band reads
    i0, i1 = max(p0 - pad, 0), min(p1 - pad, H)    # ... and the input rows among them

    def band(m):
        out = np.zeros((p1 - p0, W + 2 * pad, ch), np.float64)
        if i1 > i0:
            out[i0 + pad - p0:i1 + pad - p0, pad:pad + W] = m[i0:i1]
        return out

    ap, bp = band(a), band(b)
    ac = ap[R:R + n, md:md + OW]
    out, mag = np.zeros((n, OW, K)), np.zeros((n, OW, K))
    with np.errstate(invalid='ignore'):            # (the locality test's inf values)
        for k in range(K):
            s2p, s2o = (k // gw - r) * s2, (k % gw - r) * s2
            prod = ac * bp[R + s2p:R + s2p + n, md + s2o:md + s2o + OW]
            out[:, :, k] = prod.sum(-1) / ch
            mag[:, :, k] = np.abs(prod).sum(-1) / ch
    return out, mag


def bound(mag):
    return 34.0 * 2.0 ** -24 * mag + 1e-30


def worst_ratio(got, ref, mag):
    """max |got - ref| / bound over the finite elements of ref."""
    ok = np.isfinite(ref) & np.isfinite(mag)
    with np.errstate(invalid='ignore'):
        return float((np.abs(got.astype(np.float64) - ref)[ok] / bound(mag)[ok]).max()) if ok.any() else 0.0


# ---- the tile walk of correlation_sp_kernel ------------------------------------------------------------------------
def curve(tiles_y, tiles_x):
    """The order correlation_sp_kernel walks a full map in: 8 x 8-tile blocks in raster order, raster inside."""
    return [(ty, tx) for by in range(0, tiles_y, 8) for bx in range(0, tiles_x, 8)
            for ty in range(by, min(by + 8, tiles_y)) for tx in range(bx, min(bx + 8, tiles_x))]


def grid_of(n, G=DEFAULT_GRID):
    """launch_sp's grid for n listed tiles: G (DODT_CORR_GRID, or two workgroups per CU) rounded down to a multiple
    of 8, no more than 8 * ceil(n / 8)."""
    return min(G // 8 * 8, 8 * -(-n // 8))


def walk(n, grid):
    """{block: [slots]} of n listed tiles: block b belongs to XCD b % 8 as its workgroup b // 8; XCD x owns slots
    [x per, min((x + 1) per, n)), per = ceil(n / 8); its workgroup i takes x per + i, + grid / 8, ..."""
    per, stride = -(-n // 8), grid // 8
    out = {}
    for b in range(grid):
        xcd, wg = b % 8, b // 8
        out[b] = list(range(xcd * per + wg, min((xcd + 1) * per, n), stride))
    return out


def two_pass_tiles(n):
    """correlation_kernel's (DODT_CORR_TWO_PASS=1) block -> tile map: one 16 x 32 tile per block, none if >= n."""
    per = -(-n // 8)
    return {b: (b % 8) * per + b // 8 for b in range(8 * per)}


# ---- modes: environments of a child process -----------------------------------------------------------------------
MODES = collections.OrderedDict([
    ('default', {}),
    ('grid8', {'DODT_CORR_GRID': '8'}),
    ('grid16', {'DODT_CORR_GRID': '16'}),
    ('grid24', {'DODT_CORR_GRID': '24'}),
    ('two_pass', {'DODT_CORR_TWO_PASS': '1'}),
    ('halves2', {'DODT_CORR_HALVES': '2'}),
    ('halves2_grid8', {'DODT_CORR_HALVES': '2', 'DODT_CORR_GRID': '8'}),
])
CORR_SWITCH_PREFIX = 'DODT_CORR_'
ALL_MODES = tuple(MODES)
# seconds a mode's child may take: the process start, the library's first launch and its cases (the default's child
# also runs the 700 x 800 maps and the tile lists)
MODE_TIMEOUT = {'default': 120}


def mode_grid(mode):
    """DODT_CORR_GRID of a mode, or the device's own 512."""
    return int(MODES[mode].get('DODT_CORR_GRID', DEFAULT_GRID))


def mode_env(mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith(CORR_SWITCH_PREFIX)}
    env.update(MODES[mode])
    return env


# ---- the case table ------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'H W md s2 pad modes')


def case_id(c):
    return '%dx%d-md%d-s%d-pad%d' % (c.H, c.W, c.md, c.s2, c.pad)


WALK = [               # the 5 x 5 grid, every mode; what each is there for: test_corr_walk.py
    Case(72, 88, 5, 2, 5, ALL_MODES),
    Case(150, 200, 5, 2, 5, ALL_MODES),
    Case(70, 90, 4, 2, 5, ALL_MODES),
    Case(76, 95, 5, 2, 3, ALL_MODES),
    Case(40, 56, 5, 2, 5, ALL_MODES),
]
DEGENERATE = [Case(H, W, 5, 2, 5, ('default', 'grid8')) for H, W in ((1, 1), (1, 40), (40, 1), (5, 5))] + \
             [Case(18, 33, 5, 2, 3, ('default', 'grid8'))]
DEFAULT_GRID_CASE = Case(368, 368, 5, 2, 5, ('default',))
GENERIC = [Case(21, 35, 0, 1, 0, ('default',)),      # K = 1
           Case(21, 35, 3, 2, 1, ('default',)),      # r = 1, md not a multiple of s2
           Case(33, 20, 4, 4, 2, ('default',)),      # r = 1, stride 4
           Case(40, 37, 6, 3, 6, ('default',)),      # r = 2, patch edge 28
           Case(16, 16, 2, 1, 4, ('default',))]      # output larger than input
CASES = WALK + DEGENERATE + [DEFAULT_GRID_CASE] + GENERIC
SP_CASES = WALK + DEGENERATE + [DEFAULT_GRID_CASE]   # the cases correlation_sp_kernel takes
KINDS = ('int', 'normal')
FULL = Case(700, 800, 5, 2, 5, ('default',))
FULL_BANDS = ((0, 16), (120, 136), (344, 360), (688, 700))
BASE = WALK[0]          # (72,88): the aliasing, locality and listed-tiles tests' map


def tiles_of(c):
    OH, OW, _ = out_shape(c.H, c.W, c.md, c.s2, c.pad)
    return -(-OH // TILE), -(-OW // TILE)


def tile_store_path(c, tile):
    """'vec' if correlation_sp_kernel stores the tile's rows as 16-byte quads, 'scalar' otherwise."""
    OH, OW, K = out_shape(c.H, c.W, c.md, c.s2, c.pad)
    return 'vec' if (OW * K) % 4 == 0 and tile[1] * TILE + TILE <= OW else 'scalar'


def pair(c, kind):
    """The case's two maps: integers of [-4, 4] ('int') or standard normal ('normal'), float32."""
    rng = np.random.default_rng(((c.H * 1009 + c.W) * 31 + c.md) * 31 + c.pad + (0 if kind == 'int' else 1 << 24))
    shape = (c.H, c.W, C)
    if kind == 'int':
        return rng.integers(-4, 5, size=shape).astype(f32), rng.integers(-4, 5, size=shape).astype(f32)
    return rng.normal(size=shape).astype(f32), rng.normal(size=shape).astype(f32)


def full_pair():
    """The (700,800,32) maps of the full-size test, a != b, standard normal."""
    rng = np.random.default_rng(700800)
    return rng.normal(size=(FULL.H, FULL.W, C)).astype(f32), rng.normal(size=(FULL.H, FULL.W, C)).astype(f32)


POISON = ((0, 0, 0), (15, 15, 5), (16, 16, 16), (15, 16, 31), (BASE.H - 1, BASE.W - 1, 17))    # (y, x, channel) of B


def locality_pair():
    a, b = pair(BASE, 'normal')
    a, b = a.copy(), b.copy()
    a[a == 0] = 1.0
    for y, x, ch in POISON:
        b[y, x, ch] = np.inf if (y + x) % 2 == 0 else -np.inf
    return a, b


LISTED = dict(n_list=17, counts=(13, 0, 1, 1000, -5))


def listed_tiles():
    """A shuffled list of 17 of BASE's 30 tiles, in a buffer of 30 entries (the rest repeat a listed tile)."""
    ty, tx = tiles_of(BASE)
    order = np.random.default_rng(77).permutation(ty * tx)[:LISTED['n_list']]
    tiles = [(int(t) // tx, int(t) % tx) for t in order]
    lst = np.full(ty * tx, tiles[0][0] << 16 | tiles[0][1], i32)
    lst[:len(tiles)] = [y << 16 | x for y, x in tiles]
    return tiles, lst


# ---- the tile-list rule of dodt_correlation_tile_list in numpy -----------------------------------------------------
def coords(lo, hi, size, crop=ROI):
    """crop_coord of csrc/crop_coords.h in numpy float32, every sample."""
    lo, hi, m1 = f32(lo), f32(hi), f32(size - 1)
    with np.errstate(all='ignore'):
        step = f32(f32(f32(hi - lo) * m1) / f32(crop - 1))
        return np.array([f32(f32(lo * m1) + f32(f32(i) * step)) for i in range(crop)], f32)


def axis_range(lo, hi, size):
    """The pixel range [p0, p1] corr_tile_list_kernel takes of one axis, or None: the samples that are not NaN
    (the kernel's v == v), clamped before they become integers, one pixel wider on either side, clipped."""
    mn, mx = f32(3.0e38), f32(-3.0e38)
    for v in coords(lo, hi, size):
        if v == v:
            mn, mx = min(mn, v), max(mx, v)
    if mn > mx:
        return None
    cap = f32(size) + f32(1.0)
    p0 = max(int(np.floor(min(max(mn, f32(-2.0)), cap))) - 1, 0)
    p1 = min(int(np.floor(min(max(mx, f32(-4.0)), cap))) + 2, size - 1)
    return (p0, p1) if p0 <= p1 else None


def expected_tiles(boxes, oh, ow):
    """The rectangle rule of dodt_correlation_tile_list in numpy: (ty, tx) set."""
    want = set()
    for y1, x1, y2, x2 in boxes:
        ry, rx = axis_range(y1, y2, oh), axis_range(x1, x2, ow)
        if ry is not None and rx is not None:
            want |= {(ty, tx) for ty in range(ry[0] // TILE, ry[1] // TILE + 1)
                     for tx in range(rx[0] // TILE, rx[1] // TILE + 1)}
    return want


def expected_list(boxes, oh, ow):
    want = expected_tiles(boxes, oh, ow)
    return [t for t in curve(-(-oh // TILE), -(-ow // TILE)) if t in want]


LIST_HW = (150, 200)        # 10 x 13 tiles
N_BOXES = 700               # three chunks of 256 boxes, the last one of 188


def list_boxes():
    """700 boxes [y1, x1, y2, x2]: chunk 0 in the top left of the map, chunk 1 in the top right, chunk 2 in a band
    below them, the last box alone near the bottom right corner -- so a chunk that is dropped, or cut short, shows in
    the list -- and among them boxes with NaN, infinite and huge edges, flipped, degenerate and outside ones."""
    rng = np.random.default_rng(701)
    b = np.zeros((N_BOXES, 4), f32)
    for lo, hi, (y0, y1, x0, x1) in ((0, 256, (0.0, 0.4, 0.0, 0.4)), (256, 512, (0.0, 0.4, 0.6, 0.95)),
                                     (512, N_BOXES, (0.62, 0.78, 0.1, 0.5))):
        n = hi - lo
        b[lo:hi, 0] = rng.uniform(y0, y1, n)
        b[lo:hi, 1] = rng.uniform(x0, x1, n)
        b[lo:hi, 2] = b[lo:hi, 0] + rng.uniform(0.01, 0.05, n)
        b[lo:hi, 3] = b[lo:hi, 1] + rng.uniform(0.01, 0.05, n)
    b[N_BOXES - 1] = [0.92, 0.86, 0.95, 0.9]
    nan, inf = np.nan, np.inf
    special = [
        [nan, 0.1, 0.2, 0.2], [0.1, nan, 0.2, 0.2], [0.1, 0.1, nan, 0.2], [0.1, 0.1, 0.2, nan], [nan] * 4,
        [0.1, 0.1, inf, 0.2], [-inf, 0.1, 0.2, 0.2], [0.1, inf, 0.2, inf], [0.1, 0.1, 0.2, -inf], [inf, -inf, -inf, inf],
        [0.1, 0.12, 1e30, 0.14], [-1e30, 0.12, 0.3, 0.14], [0.1, -1e30, 0.12, 1e30], [1e30, 1e30, 1e30, 1e30],
        [-1e30, 0.1, -1e30, 0.2], [0.1, 0.1, 0.12, 1e30],
        [0.3, 0.3, 0.1, 0.1], [0.3, 0.1, 0.1, 0.3], [0.1, 0.3, 0.3, 0.1],            # flipped
        [0.2, 0.1, 0.2, 0.3], [0.1, 0.2, 0.3, 0.2], [0.25, 0.25, 0.25, 0.25],        # degenerate
        [1.2, 1.1, 1.6, 1.5], [-0.9, -0.8, -0.2, -0.1], [0.1, 1.3, 0.2, 1.5], [-3.0, 0.1, -2.5, 0.2],   # outside
        [-0.2, 0.1, 0.1, 0.2], [0.3, -0.1, 0.35, 0.05],                              # reaching out
    ]
    # every chunk gets all of them; the rows they overwrite keep the chunks' regions (the top left quarter, or
    # a column strip of it that huge edges stretch over the whole height)
    for base in (3, 256 + 40, 512 + 100):
        b[base:base + len(special)] = np.array(special, f32)
    return b


def list_index():
    """700 rows into list_boxes: none of chunk 1, repeats, negative and too-large indices."""
    rng = np.random.default_rng(702)
    pool = np.concatenate([np.arange(-5, 256), np.arange(512, N_BOXES + 20)])
    idx = rng.choice(pool, size=N_BOXES).astype(i32)
    idx[:6] = [-1, N_BOXES, 2 ** 31 - 1, -2 ** 31, N_BOXES - 1, N_BOXES - 1]
    return idx


def index_rows(boxes, idx):
    """The boxes an index list selects (an index outside the boxes selects nothing)."""
    return boxes[[j for j in idx if 0 <= j < len(boxes)]]


BIG_HW = (1440, 1456)       # 90 x 91 = 8190 tiles: just inside the list kernel's 8192 flags
TOO_BIG_HW = (1456, 1456)   # 8281 tiles


def big_boxes():
    rng = np.random.default_rng(703)
    b = rng.uniform(0.0, 0.95, size=(40, 4)).astype(f32)
    b[:, 2:] = b[:, :2] + rng.uniform(0.005, 0.04, size=(40, 2)).astype(f32)
    b[0] = [0.97, 0.97, 1.0, 1.0]         # the last tile of the curve
    b[1] = [0.0, 0.0, 0.01, 0.01]         # ... and the first
    return b


# ---- device jobs: run in a child process of the mode ---------------------------------------------------------------
def _run(ctx, ops, a, b, c, d_a=None, d_b=None):
    """One dodt_correlation into a NaN-filled buffer with GUARD floats behind the map; the whole buffer."""
    OH, OW, K = out_shape(c.H, c.W, c.md, c.s2, c.pad)
    d_a = d_a or ctx.array(a)
    d_b = d_b or (d_a if b is a else ctx.array(b))
    d_out = ctx.array(np.full(OH * OW * K + GUARD, np.nan, f32))
    ops.correlation(ctx, d_a, d_b, (c.H, c.W, C), c.md, c.s2, c.pad, d_out)
    return d_out.download()


def _count(ctx, n):
    return ctx.array(np.array([n], i32))


def _job_parity(ctx, ops, mode, out):
    for c in CASES:
        if mode in c.modes:
            for kind in KINDS:
                a, b = pair(c, kind)
                out['par__%s__%s' % (case_id(c), kind)] = _run(ctx, ops, a, b, c)


def _job_alias(ctx, ops, mode, out):
    for kind in KINDS:
        a, _ = pair(BASE, kind)
        out['alias__' + kind] = _run(ctx, ops, a, a, BASE)


def _job_locality(ctx, ops, mode, out):
    a, b = locality_pair()
    out['locality'] = _run(ctx, ops, a, b, BASE)


def _job_listed(ctx, ops, mode, out):
    c = BASE
    a, b = pair(c, 'normal')
    d_a, d_b = ctx.array(a), ctx.array(b)
    out['listed__full'] = _run(ctx, ops, a, b, c, d_a, d_b)
    OH, OW, K = out_shape(c.H, c.W, c.md, c.s2, c.pad)
    _, lst = listed_tiles()
    d_list = ctx.array(lst)
    for count in LISTED['counts']:
        d_out = ctx.array(np.full(OH * OW * K + GUARD, np.nan, f32))
        ops.correlation_tiles(ctx, d_a, d_b, (c.H, c.W, C), c.md, c.s2, c.pad, d_list, LISTED['n_list'],
                              _count(ctx, count), d_out)
        out['listed__%d' % count] = d_out.download()
    d_out = ctx.array(np.full(OH * OW * K + GUARD, np.nan, f32))       # capacity 0: nothing is launched
    ops.correlation_tiles(ctx, d_a, d_b, (c.H, c.W, C), c.md, c.s2, c.pad, d_list, 0, _count(ctx, 5), d_out)
    out['listed__cap0'] = d_out.download()


def _job_full(ctx, ops, mode, out):
    c = FULL
    a, b = full_pair()
    got = _run(ctx, ops, a, b, c)
    OH, OW, K = out_shape(c.H, c.W, c.md, c.s2, c.pad)
    m = got[:OH * OW * K].reshape(OH, OW, K)
    out['full__nans'] = np.array(int(np.isnan(m).sum()))
    out['full__guard'] = got[OH * OW * K:]
    for y0, y1 in FULL_BANDS:
        out['full__band_%d' % y0] = m[y0:y1].copy()


def _tile_list(ctx, ops, hw, d_boxes, n_boxes, d_idx, n, d_n):
    cap = ops.correlation_tile_capacity(hw)
    d_tiles, d_nt = ctx.array(np.full(cap, -1, i32)), ctx.array(np.array([-77], i32))
    ops.correlation_tile_list(ctx, hw, d_boxes, n_boxes, d_idx, n, d_n, (ROI, ROI), d_tiles, cap, d_nt)
    return d_tiles, d_nt, cap


def _job_tile_list(ctx, ops, mode, out):
    oh, ow = LIST_HW
    K = 25
    boxes, idx = list_boxes(), list_index()
    d_boxes, d_idx = ctx.array(boxes), ctx.array(idx)
    c = Case(oh, ow, 5, 2, 5, ())
    a, b = pair(c, 'normal')
    d_a, d_b = ctx.array(a), ctx.array(b)
    d_full = ctx.array(np.full((oh, ow, K), np.nan, f32))
    ops.correlation(ctx, d_a, d_b, (oh, ow, C), 5, 2, 5, d_full)
    for name, d_ix in (('plain', None), ('indexed', d_idx)):
        d_tiles, d_nt, cap = _tile_list(ctx, ops, LIST_HW, d_boxes, N_BOXES, d_ix, N_BOXES,
                                        None if d_ix is None else _count(ctx, N_BOXES))
        out['tl__%s__tiles' % name], out['tl__%s__n' % name] = d_tiles.download(), d_nt.download()
        d_part = ctx.array(np.full((oh, ow, K), np.nan, f32))
        ops.correlation_tiles(ctx, d_a, d_b, (oh, ow, C), 5, 2, 5, d_tiles, cap, d_nt, d_part)
        out['tl__%s__part_nan' % name] = np.isnan(d_part.download()).all(-1)
        for which, d_map in (('full', d_full), ('part', d_part)):
            d_crops = ctx.array(np.full((N_BOXES, ROI * ROI * K), -7.5, f32))
            if d_ix is None:
                ops.crop_and_resize(ctx, d_map, (oh, ow, K), d_boxes, N_BOXES, None, (ROI, ROI), d_crops)
            else:
                ops.crop_and_resize_indexed(ctx, d_map, (oh, ow, K), d_boxes, N_BOXES, d_ix, N_BOXES,
                                            _count(ctx, N_BOXES), (ROI, ROI), d_crops)
            out['tl__%s__crops_%s' % (name, which)] = d_crops.download()
    # the clamps of *d_n, and no boxes at all
    for name, n, d_n in (('neg', N_BOXES, _count(ctx, -3)), ('above', 300, _count(ctx, 100000))):
        d_tiles, d_nt, _ = _tile_list(ctx, ops, LIST_HW, d_boxes, N_BOXES, None, n, d_n)
        out['tl__%s__tiles' % name], out['tl__%s__n' % name] = d_tiles.download(), d_nt.download()
    d_tiles, d_nt, _ = _tile_list(ctx, ops, LIST_HW, None, 0, None, 0, None)
    out['tl__none__tiles'], out['tl__none__n'] = d_tiles.download(), d_nt.download()
    # 8190 tiles
    bb = big_boxes()
    d_tiles, d_nt, _ = _tile_list(ctx, ops, BIG_HW, ctx.array(bb), len(bb), None, len(bb), None)
    out['tl__big__tiles'], out['tl__big__n'] = d_tiles.download(), d_nt.download()


def _job_errors(ctx, ops, mode, out):
    """What the entry points refuse: '<exception type>: <message>' of each, '' where nothing was raised."""
    small = ctx.array(np.zeros(64 * 64 * 32, f32))
    ints = ctx.array(np.zeros(130, i32))
    calls = {
        'c16': lambda: ops.correlation(ctx, small, small, (8, 8, 16), 5, 2, 5, small),
        'k121': lambda: ops.correlation(ctx, small, small, (8, 8, 32), 10, 2, 10, small),
        'empty': lambda: ops.correlation(ctx, small, small, (4, 4, 32), 5, 2, 2, small),
        'tiles_c16': lambda: ops.correlation_tiles(ctx, small, small, (8, 8, 16), 5, 2, 5, ints, 1, ints, small),
        'tiles_empty': lambda: ops.correlation_tiles(ctx, small, small, (4, 4, 32), 5, 2, 2, ints, 1, ints, small),
        'tiles_generic': lambda: ops.correlation_tiles(ctx, small, small, (8, 8, 32), 2, 1, 2, ints, 1, ints, small),
        'list_too_big': lambda: ops.correlation_tile_list(ctx, TOO_BIG_HW, small, 1, None, 1, None, (ROI, ROI), ints,
                                                          8281, ints),
        'list_capacity': lambda: ops.correlation_tile_list(ctx, LIST_HW, small, 1, None, 1, None, (ROI, ROI), ints,
                                                           129, ints),
    }
    got = {}
    for name, call in calls.items():
        try:
            call()
            got[name] = ''
        except Exception as e:       # noqa: BLE001  (the type is what the parent checks)
            got[name] = '%s: %s' % (type(e).__name__, e)
    ctx.sync()
    out['errors'] = np.array(json.dumps(got))


JOBS = {
    'default': (_job_parity, _job_locality, _job_full, _job_tile_list, _job_errors),
    'grid8': (_job_parity, _job_alias, _job_locality, _job_listed),
}


def child_main(mode, path):
    """Every device job of a mode, in this process (whose environment must be the mode's), into one .npz."""
    switches = {k: v for k, v in os.environ.items() if k.startswith(CORR_SWITCH_PREFIX)}
    assert switches == MODES[mode], (mode, switches)
    from dodt_amd import device, ops
    ctx = device.default_context()
    # every device array of this process is kept, and zeroed before the process ends: the NaN pre-fills and the
    # locality test's infinities are not left in memory that a later process gets uninitialised
    made, array = [], ctx.array
    ctx.array = lambda host, dtype=None: (made.append(array(host, dtype)), made[-1])[1]
    out = {}
    for job in JOBS.get(mode, (_job_parity,)):
        job(ctx, ops, mode, out)
    ctx.sync()
    np.savez(path, **out)
    for d in made:
        d.zero()
    ctx.sync()
    print('MODE %s ok' % mode)


# ---- the parent's side ---------------------------------------------------------------------------------------------
_results = {}
_casualty = []          # the first child that ended by a signal, an abort or its time limit


def run_mode(mode, tmp_dir):
    """{name: array} of a mode's child, run once.  After a child has ended by a signal, with status 134 or 139 or at
    its time limit, nothing is started on the device any more: every later call fails, naming that child."""
    if mode in _results:
        assert not isinstance(_results[mode], str), _results[mode]
        return _results[mode]
    assert not _casualty, 'not started: %s' % _casualty[0]
    path = os.path.join(str(tmp_dir), 'corr_%s.npz' % mode)
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import _corr_cases as cc; '
            'cc.child_main(%r, %r)' % (ROOT, os.path.join(ROOT, 'tests'), mode, path))
    limit = MODE_TIMEOUT.get(mode, 60)
    try:
        r = subprocess.run([sys.executable, '-c', code], env=mode_env(mode), cwd=ROOT, capture_output=True, text=True,
                           timeout=limit)
    except subprocess.TimeoutExpired:
        _casualty.append("the child of mode '%s' did not end within %d s" % (mode, limit))
        raise AssertionError(_casualty[0])
    tail = r.stdout[-2000:] + r.stderr[-3000:]
    if r.returncode < 0 or r.returncode in (134, 139):
        _casualty.append("the child of mode '%s' ended with status %d" % (mode, r.returncode))
        raise AssertionError(_casualty[0] + '\n' + tail)
    if r.returncode != 0 or 'MODE %s ok' % mode not in r.stdout:
        _results[mode] = "the child of mode '%s' failed with status %d\n%s" % (mode, r.returncode, tail)
        raise AssertionError(_results[mode])
    with np.load(path) as z:
        _results[mode] = {k: z[k] for k in z.files}
    return _results[mode]
