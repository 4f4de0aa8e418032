"""Soundness of the fp32 BEV net's skip rule ("a 3x3 conv reaches 1, a pool ORs 2x2 windows, a transposed conv is the
nearest 2x upsampling dilated by 2"), which frame_tables.h, the Support functions of conv_skip.hip and layer_masks of
tests/test_bev_support_mask.py all restate.

1. The rule against the network's arithmetic: the oracle net with live-fringe weights (|w|, beta = 0: nothing cancels,
   ReLU clips nothing, a zero input gives a zero map) is fed single cells and small cell sets; the pixels of a layer
   that become non-zero ARE the layer's dependency on those cells.  It must equal the rule in the encoder, lie inside
   it in the decoder, and equal everywhere the exact propagation with the transposed conv's measured footprint.
2. The library's rule (dodt_frame_tables_host, the functions the device builder runs) at pixel resolution: 1 x 1 items
   over every pixel of every layer's grid (2 x 2 blocks for the transposed convs) against layer_masks."""
import numpy as np
import pytest

from dodt_amd import ops, synth
from oracle import extractors as oext
from oracle import tfops
from tests import test_bev_support_mask as geom

LAYERS = tuple(oext.pyramid_layer_names())
ENCODER = LAYERS[:10]
DECODER = LAYERS[10:]
# the level of a layer's item grid (level l is (H >> l) x (W >> l)): a transposed conv's items lie on its input's grid
LEVEL = dict(conv1_1=0, conv1_2=0, conv2_1=1, conv2_2=1, conv3_1=2, conv3_2=2, conv3_3=2, conv4_1=3, conv4_2=3,
             conv4_3=3, upconv3=3, pyramid_fusion3=2, upconv2=2, pyramid_fusion2=1, upconv1=1, pyramid_fusion1=0)
# rows and columns divisible by 8: narrower than one mask word, exactly two words, three words, a ragged last word
SHAPES = ((40, 24), (48, 64), (64, 96), (72, 136))


def live_fringe_params(in_ch=6):
    """synth.pyramid_params with w = |w| and beta = 0: every tap of every receptive field adds a positive amount to
    every output channel, and an all-zero input gives an all-zero map at every layer."""
    params = synth.pyramid_params(in_ch)
    for p in params.values():
        p['w'] = np.abs(p['w']).astype(np.float32)
        p['beta'] = np.zeros_like(p['beta'])
    assert all((p['w'] > 0).all() for p in params.values())
    return params


def _impulse_reach(h, w, i, j):
    x = np.zeros((h, w, 1), np.float32)
    x[i, j, 0] = 1.0
    out = tfops.conv2d_transpose_s2_same(x, np.ones((3, 3, 1, 1), np.float32))[:, :, 0]
    assert out.shape == (2 * h, 2 * w)
    return {(int(y) - 2 * i, int(xx) - 2 * j) for y, xx in np.argwhere(out != 0)}


def upconv_footprint():
    """{(dy, dx)}: input (i, j) of the oracle's transposed conv reaches outputs (2i + dy, 2j + dx).  Measured with unit
    impulses and an all-ones kernel: the same offsets at every interior position, clipped at the borders."""
    found = None
    for h, w in ((5, 5), (4, 6)):
        for i in range(h):
            for j in range(w):
                got = _impulse_reach(h, w, i, j)
                if 0 < i < h - 1 and 0 < j < w - 1:
                    assert found is None or got == found
                    found = got
        for i in range(h):
            for j in range(w):
                want = {(dy, dx) for dy, dx in found if 0 <= 2 * i + dy < 2 * h and 0 <= 2 * j + dx < 2 * w}
                assert _impulse_reach(h, w, i, j) == want, (h, w, i, j)
    return found


def _up_exact(m, footprint):
    h, w = m.shape
    o = np.zeros((2 * h, 2 * w), bool)
    ys, xs = np.nonzero(m)
    for dy, dx in footprint:
        yy, xx = 2 * ys + dy, 2 * xs + dx
        ok = (yy >= 0) & (yy < 2 * h) & (xx >= 0) & (xx < 2 * w)
        o[yy[ok], xx[ok]] = True
    return o


def exact_masks(mask, footprint):
    """The boolean propagation of the oracle net itself: layer_masks with the transposed conv's true footprint."""
    d, p = geom._dilate, geom._pool
    x = np.asarray(mask).astype(bool)
    L = {}
    L['conv1_1'] = a = d(x, 1)
    L['conv1_2'] = c12 = d(a, 1)
    L['conv2_1'] = a = d(p(c12), 1)
    L['conv2_2'] = c22 = d(a, 1)
    L['conv3_1'] = a = d(p(c22), 1)
    L['conv3_2'] = a = d(a, 1)
    L['conv3_3'] = c33 = d(a, 1)
    L['conv4_1'] = a = d(p(c33), 1)
    L['conv4_2'] = a = d(a, 1)
    L['conv4_3'] = c43 = d(a, 1)
    L['upconv3'] = u3 = _up_exact(c43, footprint)
    L['pyramid_fusion3'] = f3 = d(c33 | u3, 1)
    L['upconv2'] = u2 = _up_exact(f3, footprint)
    L['pyramid_fusion2'] = f2 = d(c22 | u2, 1)
    L['upconv1'] = u1 = _up_exact(f2, footprint)
    L['pyramid_fusion1'] = d(c12 | u1, 1)
    return L


def seam_columns(w):
    """Columns on both sides of the 32-bit word seams of a row's mask, tile corners, and the row's ends."""
    return sorted({x for x in (0, 15, 16, 31, 32, 33, 47, 48, 63, 64, 65, 95, 96, w - 1) if 0 <= x < w})


def cell_cases(h, w):
    """[(label, [(y, x, channel), ...])]: the inputs of the dependency test on an h x w map."""
    cases = []
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        cases.append(('corner', [(y, x, 0)]))
    for k, x in enumerate(seam_columns(w)):
        cases.append(('seam', [((5 * k + 3) % h, x, k % 6)]))
    # every residue mod 8 on both axes: the 2x2 windows of all three pools split on either side of the cell
    for r in range(8):
        cases.append(('parity', [(8 + r, 8 + (3 * r + 1) % 8, r % 6)]))
        cases.append(('parity', [(h - 16 + (5 * r + 2) % 8, w - 16 + r, (r + 3) % 6)]))
    for c in range(6):
        cases.append(('channel', [(h // 2 + 1, w // 2 - 2, c)]))
    # small sets: diagonal neighbours across a word seam (or the map's middle), far-apart cells, a short row
    sx = 32 if w > 32 else w // 2
    cases.append(('set', [(11, sx - 1, 1), (12, sx, 4)]))
    cases.append(('set', [(0, 0, 2), (h - 1, w - 1, 3)]))
    cases.append(('set', [(h // 2, x, 5) for x in range(w // 2 - 2, w // 2 + 2)]))
    cases.append(('set', [(3, w - 2, 0), (h - 3, 1, 5), (h // 2, w // 2, 2)]))
    return cases


@pytest.mark.parametrize('shape', SHAPES)
def test_rule_against_the_oracle_nets_true_dependency(shape):
    h, w = shape
    params = live_fringe_params()
    footprint = upconv_footprint()
    zero = {}
    oext.vgg_pyramid(np.zeros((h, w, 6), np.float32), params, collect=zero)
    assert all(not zero[n].any() for n in LAYERS)      # (so act != 0 is the dependency on the cells)
    over = {n: 0 for n in DECODER}
    room = {n: False for n in DECODER}
    cases = cell_cases(h, w)
    for label, cells in cases:
        x = np.zeros((h, w, 6), np.float32)
        for y, cx, c in cells:
            x[y, cx, c] = 1.0
        acts = {}
        oext.vgg_pyramid(x, params, collect=acts)
        mask = np.any(x != 0, axis=2)
        rule = geom.layer_masks(mask)
        exact = exact_masks(mask, footprint)
        for n in LAYERS:
            what = (shape, label, cells, n)
            assert np.isfinite(acts[n]).all(), what
            dep = np.any(acts[n] != 0, axis=2)
            assert dep.shape == rule[n].shape, what
            assert dep.any(), what
            assert np.array_equal(dep, exact[n]), (what, np.argwhere(dep != exact[n])[:8])
            assert not (exact[n] & ~rule[n]).any(), (what, np.argwhere(exact[n] & ~rule[n])[:8])
            if n in ENCODER:
                assert np.array_equal(dep, rule[n]), (what, np.argwhere(dep != rule[n])[:8])
            else:
                assert not (dep & ~rule[n]).any(), (what, np.argwhere(dep & ~rule[n])[:8])
                over[n] += int((rule[n] & ~dep).sum())
                room[n] |= not dep.all()
    assert len(cases) >= 30
    # the rule over-reaches in the decoder wherever the dependency leaves it room on the map (the subset assertions
    # above are not equalities in disguise); on the larger maps that is every decoder layer
    assert all(over[n] > 0 for n in DECODER if room[n]), (over, room)
    assert all(room.values()) or h * w < 48 * 64, room


def test_upconv_footprint_lies_inside_the_rule_at_every_position():
    """One transposed conv alone, every input position of a small map: the measured footprint is 2i .. 2i + 2 on both
    axes, and the rule's _up (2i - 2 .. 2i + 3) covers it."""
    footprint = upconv_footprint()
    assert footprint == {(dy, dx) for dy in range(3) for dx in range(3)}
    h, w = 5, 7
    for i in range(h):
        for j in range(w):
            m = np.zeros((h, w), bool)
            m[i, j] = True
            exact, rule = _up_exact(m, footprint), geom._up(m)
            assert exact.any() and not (exact & ~rule).any(), (i, j)


# -- the library's rule at pixel resolution ---------------------------------------------------------------------------

def _pixel_items(frames, gh, gw):
    f, y, x = np.meshgrid(np.arange(frames), np.arange(gh), np.arange(gw), indexing='ij')
    return np.stack([f.ravel(), np.zeros(f.size, np.int64), y.ravel(), x.ravel()], axis=1).astype(np.int32)


def _check_pixels(frame_masks, rng):
    """Every layer: 1 x 1 items over every pixel of the layer's grid (a transposed conv's item writes the 2 x 2 outputs
    from (2 y0, 2 x0)), all frames in one call, against layer_masks; then the union with a random prev vector."""
    frame_masks = [np.asarray(m, np.uint8) for m in frame_masks]
    frames = len(frame_masks)
    rows, cols = frame_masks[0].shape
    rule = [geom.layer_masks(m) for m in frame_masks]
    stacked = np.stack(frame_masks)
    for li, name in enumerate(LAYERS):
        gh, gw = rows >> LEVEL[name], cols >> LEVEL[name]
        want = np.stack([geom._pool(r[name]) if name.startswith('up') else r[name] for r in rule])
        assert want.shape == (frames, gh, gw), name
        items = _pixel_items(frames, gh, gw)
        reach = want.ravel()
        got = ops.frame_tables_host(stacked, li, 1, 1, items)
        assert np.array_equal(got, items[reach]), (name, rows, cols)       # (the kept items, in table order)
        prev = (rng.uniform(size=len(items)) < 0.2).astype(np.uint8)
        got = ops.frame_tables_host(stacked, li, 1, 1, items, prev=prev)
        assert np.array_equal(got, items[reach | (prev != 0)]), (name, rows, cols)


def _cells(shape, cells):
    m = np.zeros(shape, np.uint8)
    for y, x in cells:
        m[y, x] = 1
    return m


@pytest.mark.parametrize('shape', SHAPES + ((704, 800),))
def test_library_rule_at_pixel_resolution(shape):
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    empty = np.zeros(shape, np.uint8)
    full = np.ones(shape, np.uint8)
    sparse = (rng.uniform(size=shape) < 0.01).astype(np.uint8)
    other = (rng.uniform(size=shape) < 0.01).astype(np.uint8)
    corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    seams = seam_columns(w) + [x for x in (767, 768) if x < w]
    if h * w > 100000:
        # the full-size map: a few calls, two different frames each
        pairs = [(_cells(shape, [(350, x) for x in seams]), _cells(shape, corners)), (sparse, full), (other, empty),
                 (_cells(shape, [(h - 1, 31)]), _cells(shape, [(0, 32)]))]
    else:
        pairs = [(_cells(shape, [c]), _cells(shape, [corners[3 - k]])) for k, c in enumerate(corners)]
        for k, x in enumerate(seams):
            y = (7 * k + 2) % h
            pairs.append((_cells(shape, [(y, x)]), _cells(shape, [(h - 1 - y, seams[-1 - k])])))
        for r in range(8):
            pairs.append((_cells(shape, [(8 + r, 8 + (3 * r + 1) % 8)]), _cells(shape, [(h - 9 - r, w - 16 + r)])))
        pairs += [(sparse, other), (other, full), (full, empty), (empty, sparse)]
    for a, b in pairs:
        _check_pixels([a, b], rng)
    _check_pixels([sparse], rng)        # (and a single frame)
