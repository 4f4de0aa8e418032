"""The copy the restore launch makes for one item (dodt_frame_restore_host: restore_item of frame_tables.h, the function
the device kernel runs): exactly the item's output region goes from the store to the live map, nothing else is
touched.  Channel-blocked layer buffers with their pooled halves, transposed-conv items, clipped tiles on the map's
edge, and pyramid_fusion1's NHWC rows with the pad rows sliced off and the bottleneck cells."""
import numpy as np
import pytest

from dodt_amd import ops

LIVE = -1.0     # what the live maps hold before the copy


def _store(shape, seed):
    return np.random.default_rng(seed).uniform(1, 2, size=shape).astype(np.float32)


@pytest.mark.parametrize('case', [
    # rows, cols, channels, ch0, bn, f, th, tw, item, pooled
    (44, 56, 64, 0, 32, 1, 16, 16, (1, 1, 16, 32), True),       # interior tile, second channel tile, pooled half
    (44, 56, 64, 0, 64, 1, 16, 16, (0, 0, 32, 48), True),       # clipped at the bottom and the right edge
    (44, 56, 64, 0, 32, 1, 16, 32, (1, 0, 0, 32), False),       # the first layer's 16 x 32 tiles, clipped on the right
    (44, 56, 96, 64, 16, 2, 16, 16, (0, 1, 16, 16), False),     # transposed conv into the concat's upper planes, clipped
    (32, 32, 32, 0, 32, 2, 16, 16, (1, 0, 0, 0), False),        # transposed conv, 32 x 32 outputs
])
def test_layer_buffer_item(case):
    rows, cols, ch, ch0, bn, f, th, tw, item, pooled = case
    frames = 2
    src = _store((ch // 8, rows, cols, 8), 1)
    dst = np.full((frames,) + src.shape, LIVE, np.float32)
    psrc = _store((ch // 8, rows // 2, cols // 2, 8), 2) if pooled else None
    pdst = np.full((frames,) + psrc.shape, LIVE, np.float32) if pooled else None
    ops.frame_restore_host(item, f, th, tw, bn, ch0, dst, src, pdst, psrc)
    fr, n, y0, x0 = item
    want = np.full_like(dst, LIVE)
    p0, p1 = (ch0 + n * bn) // 8, (ch0 + (n + 1) * bn) // 8
    ys, xs = slice(f * y0, f * (y0 + th)), slice(f * x0, f * (x0 + tw))
    want[fr, p0:p1, ys, xs] = src[p0:p1, ys, xs]
    assert np.array_equal(dst, want)
    assert (dst != LIVE).any()
    if pooled:
        pwant = np.full_like(pdst, LIVE)
        q0, q1 = n * bn // 8, (n + 1) * bn // 8
        ys, xs = slice(y0 // 2, (y0 + th) // 2), slice(x0 // 2, (x0 + tw) // 2)
        pwant[fr, q0:q1, ys, xs] = psrc[q0:q1, ys, xs]
        assert np.array_equal(pdst, pwant)
        assert (pdst != LIVE).any()


@pytest.mark.parametrize('case', [
    # rows (with pad), cols, pad_top, bn, th, tw, item, bottleneck
    (44, 56, 4, 32, 16, 16, (0, 0, 0, 0), True),        # the tile that holds the pad rows: 12 rows of the map
    (44, 56, 4, 32, 16, 16, (1, 0, 32, 48), True),      # clipped at the bottom and the right edge
    (44, 56, 4, 32, 16, 16, (1, 0, 16, 16), False),     # no bottleneck asked for
    (44, 56, 4, 16, 16, 32, (0, 1, 16, 32), True),      # 16-channel tiles: channel tile 1 leaves the bottleneck alone
    (40, 48, 0, 32, 8, 8, (1, 0, 8, 44), True),         # no padding, 8 x 8 tiles, x0 not a multiple of the tile (clipped)
])
def test_output_pair_item(case):
    rows, cols, pad, bn, th, tw, item, with_bneck = case
    frames, ch = 2, 32
    out_h = rows - pad
    src = _store((out_h, cols, ch), 3)
    dst = np.full((frames,) + src.shape, LIVE, np.float32)
    bsrc = _store((out_h, cols), 4) if with_bneck else None
    bdst = np.full((frames, out_h, cols), LIVE, np.float32) if with_bneck else None
    ops.frame_restore_host(item, 1, th, tw, bn, 0, dst, src, bdst, bsrc, pad_top=pad)
    fr, n, y0, x0 = item
    ys, xs = slice(max(y0 - pad, 0), max(y0 + th - pad, 0)), slice(x0, x0 + tw)
    want = np.full_like(dst, LIVE)
    want[fr, ys, xs, n * bn:(n + 1) * bn] = src[ys, xs, n * bn:(n + 1) * bn]
    assert np.array_equal(dst, want)
    assert (dst != LIVE).any()
    if with_bneck:
        bwant = np.full_like(bdst, LIVE)
        if n == 0:
            bwant[fr, ys, xs] = bsrc[ys, xs]
        assert np.array_equal(bdst, bwant)
        assert (bdst != LIVE).any() == (n == 0)


def test_bad_arguments_are_refused():
    src = np.zeros((4, 16, 16, 8), np.float32)
    dst = np.zeros((1, 4, 16, 16, 8), np.float32)
    with pytest.raises(ValueError):
        ops.frame_restore_host((0, 1, 0, 0), 1, 16, 16, 32, 0, dst, src)          # channel tile beyond the map
    with pytest.raises(ValueError):
        ops.frame_restore_host((0, 0, 0, 0), 1, 16, 16, 32, 0, dst, src, dst2=src)    # half a pooled pair
