"""A numpy model of how dodt_nms is put together -- not of its arithmetic.

hits() holds which sorted row suppresses which later row, by the oracle's float32 IoU arithmetic (tfops._iou_gt,
vectorised).  run() then walks the rows the way the kernels do: candidate order from 64-bit keys, the row chunks
of the host plan (ops.nms_plan), every 64-row block resolved as the fixed point
alive[j] = init[j] & !(cols[j] & alive), the selection cut to the room left, the kept rows of a block ORed into
`removed` for the chunk's later blocks, a sweep at the chunk's end for the column blocks behind it (64 per trip),
`done` once max_out is reached or the candidates run out.  Each of DEFECTS breaks one of these the way a slip in
the kernel would; tests/test_nms_cases.py asserts that the model without a defect equals the oracle and that every
defect changes the keep list of some case of tests/_nms_cases.py.
"""
import numpy as np

F32 = np.float32

DEFECTS = (
    'fixed_point_8',    # the block's fixed point stopped after 8 iterations
    'no_sweep',         # the kept rows of a chunk never reach the column blocks of later chunks
    'sweep_one_trip',   # ... reach only the first 64 column blocks behind the chunk
    'reach_short',      # in-chunk removal one column block short: a full chunk has 64 blocks, so the first block's rows
                        # must reach 63 blocks ahead; the defect stops at 62
    'pads_unmasked',    # rows from *d_n on take part (keys, boxes and the block's valid bits)
    'neg_zero_below',   # -0.0 ordered below +0.0 instead of tying with it
    'no_room_cut',      # the block that reaches max_out hands out all its alive rows
)


def iou_gt(bi, bj, thr):
    """tfops._iou_gt on rows of (m,4) arrays, the same float32 operations in the same order."""
    ymin_i, xmin_i = np.minimum(bi[:, 0], bi[:, 2]), np.minimum(bi[:, 1], bi[:, 3])
    ymax_i, xmax_i = np.maximum(bi[:, 0], bi[:, 2]), np.maximum(bi[:, 1], bi[:, 3])
    ymin_j, xmin_j = np.minimum(bj[:, 0], bj[:, 2]), np.minimum(bj[:, 1], bj[:, 3])
    ymax_j, xmax_j = np.maximum(bj[:, 0], bj[:, 2]), np.maximum(bj[:, 1], bj[:, 3])
    with np.errstate(all='ignore'):
        area_i = (ymax_i - ymin_i).astype(F32) * (xmax_i - xmin_i).astype(F32)
        area_j = (ymax_j - ymin_j).astype(F32) * (xmax_j - xmin_j).astype(F32)
        iy = np.maximum((np.minimum(ymax_i, ymax_j) - np.maximum(ymin_i, ymin_j)).astype(F32), F32(0))
        ix = np.maximum((np.minimum(xmax_i, xmax_j) - np.maximum(xmin_i, xmin_j)).astype(F32), F32(0))
        inter = (iy * ix).astype(F32)
        iou = (inter / ((area_i + area_j).astype(F32) - inter).astype(F32)).astype(F32)
        return ~(area_i <= 0) & ~(area_j <= 0) & (iou > F32(thr))


def _keys(scores, n_eff, neg_zero_below):
    """The kernel's 64-bit keys of the first n_eff rows: ascending key = (score descending, index ascending)."""
    bits = np.ascontiguousarray(scores[:n_eff], F32).view(np.uint32).copy()
    if not neg_zero_below:
        bits[bits == 0x80000000] = 0
    neg = (bits & 0x80000000) != 0
    ordered = np.where(neg, ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)     # monotone increasing in the score
    return ((~ordered & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | np.arange(n_eff, dtype=np.uint64)


def order(scores, n_eff, neg_zero_below=False):
    return np.argsort(_keys(scores, n_eff, neg_zero_below), kind='stable')


def hits(boxes, thr):
    """Pairs (r, c), r < c, of rows of `boxes` (already in candidate order) with IoU > thr, as CSR over r:
    -> ptr (n+1), cols.  Only pairs whose x intervals meet are evaluated: every other pair has an intersection of
    0 and an IoU of 0 or NaN, which exceeds no threshold >= 0."""
    b = np.asarray(boxes, F32)
    n = len(b)
    xmin, xmax = np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 1], b[:, 3])
    by_x = np.argsort(xmin, kind='stable')          # NaN rows sort last and meet nobody
    xs = xmin[by_x]
    with np.errstate(invalid='ignore'):
        hi = np.searchsorted(xs, xmax[by_x], side='right')
    pos = np.arange(n)
    cnt = np.maximum(hi - (pos + 1), 0)
    cnt[np.isnan(xs) | np.isnan(xmax[by_x])] = 0
    rows, cols = np.zeros(0, np.int64), np.zeros(0, np.int64)
    step = max(1, 4000000 // max(int(cnt.max(initial=1)), 1))
    out_r, out_c = [rows], [cols]
    for a in range(0, n, step):
        c = cnt[a:a + step]
        tot = int(c.sum())
        if tot == 0:
            continue
        i_pos = np.repeat(pos[a:a + step], c)
        start = np.repeat(np.cumsum(c) - c, c)
        j_pos = i_pos + 1 + (np.arange(tot) - start)
        i, j = by_x[i_pos], by_x[j_pos]
        r, c2 = np.minimum(i, j), np.maximum(i, j)
        ok = iou_gt(b[r], b[c2], thr)
        out_r.append(r[ok])
        out_c.append(c2[ok])
    rows, cols = np.concatenate(out_r), np.concatenate(out_c)
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, rows + 1, 1)
    return np.cumsum(ptr), cols


class Sorted(object):
    """A case in candidate order with its hits: what the keys, rank / sort, scatter and mask kernels leave."""

    def __init__(self, boxes, scores, thr, n_eff=None, pads_unmasked=False, neg_zero_below=False):
        n = len(scores)
        n_eff = n if n_eff is None else max(min(int(n_eff), n), 0)
        self.n = n
        self.n_eff = n if pads_unmasked else n_eff
        self.idx = order(scores, self.n_eff, neg_zero_below)
        self.ptr, self.cols = hits(np.asarray(boxes, F32)[self.idx], thr)


def run(srt, plan, max_out, defect=None):
    """-> the keep list (original indices, int32) the structure gives on the sorted case `srt`."""
    assert defect is None or defect in DEFECTS
    n_eff, nb = srt.n_eff, plan['nb']
    ptr, cols = srt.ptr, srt.cols
    removed = np.zeros(nb * 64, bool)
    keep, done = [], n_eff <= 0
    max_iter = 8 if defect == 'fixed_point_8' else 1 << 30
    for row0, rows in plan['chunks']:
        if done:
            break                       # the remaining launches are no-ops
        b0, b1 = row0 // 64, min((row0 + rows + 63) // 64, (n_eff + 63) // 64)
        kept_rows, stop = [], False
        for b in range(b0, b1):
            valid = min(64, n_eff - b * 64)
            init = ~removed[b * 64:b * 64 + 64]
            init[valid:] = False
            diag = np.zeros((64, 64), bool)            # diag[r, j]: row r of the block suppresses its row j
            lo, hi = ptr[b * 64], ptr[min(b * 64 + valid, len(ptr) - 1)]
            c = cols[lo:hi]
            r = np.repeat(np.arange(valid), np.diff(ptr[b * 64:b * 64 + valid + 1]))
            inside = c < b * 64 + 64
            diag[r[inside], c[inside] - b * 64] = True
            alive = init.copy()
            for _ in range(max_iter):
                na = init & ~(diag & alive[:, None]).any(axis=0)
                if np.array_equal(na, alive):
                    break
                alive = na
            sel = np.flatnonzero(alive)
            room = max_out - len(keep)
            if len(sel) > room and defect != 'no_room_cut':
                sel = sel[:room]
            keep.extend(int(i) for i in srt.idx[b * 64 + sel])
            kept_rows.extend(b * 64 + sel)
            if len(keep) >= max_out:
                stop = True
                break
            reach = b1 if defect != 'reach_short' else min(b1, b + 63)      # column blocks b + 1 .. reach - 1
            for row in b * 64 + sel:
                c = cols[ptr[row]:ptr[row + 1]]
                removed[c[(c >= b * 64 + 64) & (c < reach * 64)]] = True
        if not stop and row0 + rows < n_eff and defect != 'no_sweep':
            end = nb if defect != 'sweep_one_trip' else min(nb, b1 + 64)
            for row in kept_rows:
                c = cols[ptr[row]:ptr[row + 1]]
                removed[c[(c >= b1 * 64) & (c < end * 64)]] = True
        if stop or row0 + rows >= n_eff:
            done = True
    return np.asarray(keep, np.int32)
