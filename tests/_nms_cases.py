"""NMS cases whose keep list follows from how they are built, not from the oracle.

The generators are numpy only.  Each returns float32 boxes [y1,x1,y2,x2], float32 scores and the int32 keep list
for max_output_size = n (a smaller k keeps its first k entries: greedy NMS is a prefix).  The table at the end lists what
tests/test_nms_cases.py proves things about on the host and tests/test_gpu_nms.py runs on the device; the planted
ranks of its grid cases come from the chunk plan of dodt_nms (ops.nms_plan), so they sit on the seams of the plan
the call really takes.
"""
import collections
import functools

import numpy as np

F32 = np.float32

Case = collections.namedtuple('Case', 'id boxes scores k thr n_eff keep')
# keep: the construction's list, already cut to k; None where only the oracle knows (random boxes)


def random_boxes(rng, n, scale):
    """The random boxes and scores of tests/test_gpu_ops.py::_nms_case, same draws in the same order."""
    cy, cx = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    h, w = rng.uniform(0.01, scale, n), rng.uniform(0.01, scale, n)
    boxes = np.stack([cy - h, cx - w, cy + h, cx + w], 1).astype(F32)
    scores = rng.uniform(0, 1, n).astype(F32)
    return boxes, scores


def _distinct_scores(n):
    """scores[r] of score rank r: strictly descending, exact in float32 (n < 2^17)."""
    assert n < (1 << 17)
    return ((n - np.arange(n)).astype(np.float64) / float(1 << 17)).astype(F32)


def chain(n, lead, seed=0):
    """n boxes, threshold 0.5.  Score ranks lead.. are the chain [0, i/4, 1, i/4 + 1], i = rank - lead: neighbours
    have IoU 0.75 / 1.25 = 0.6, boxes two apart 0.5 / 1.5 = 1/3, so greedy keeps i = 0, 2, 4, ... and every box's
    fate hangs on the whole chain before it (64 fixed-point iterations inside a 64-row block).  The `lead` top ranks
    are isolated boxes far away: they shift the chain's parity against the block and chunk seams.  The input order
    is a random permutation of the rank order.  All coordinates are exact in float32."""
    assert 0 <= lead < n
    by_rank = np.zeros((n, 4), np.float64)
    for r in range(lead):
        by_rank[r] = [10.0 + 2 * r, -10.0, 11.0 + 2 * r, -9.0]
    i = np.arange(n - lead, dtype=np.float64)
    by_rank[lead:] = np.stack([0 * i, i / 4, 0 * i + 1, i / 4 + 1], 1)
    assert np.array_equal(by_rank.astype(F32).astype(np.float64), by_rank)
    perm = np.random.default_rng(seed).permutation(n)          # perm[r] = input index of rank r
    boxes, scores = np.zeros((n, 4), F32), np.zeros(n, F32)
    boxes[perm], scores[perm] = by_rank.astype(F32), _distinct_scores(n)
    kept_ranks = list(range(lead)) + list(range(lead, n, 2))
    return boxes, scores, perm[kept_ranks].astype(np.int32)


def _grid_boxes(n, rng):
    """n pairwise disjoint boxes of side 1/2 in the cells of a square grid of pitch 1, cells in random order."""
    side = int(np.ceil(np.sqrt(n)))
    cell = rng.permutation(side * side)[:n]
    gy, gx = (cell // side).astype(np.float64), (cell % side).astype(np.float64)
    return np.stack([gy, gx, gy + 0.5, gx + 0.5], 1)


def grid_with_plants(n, ranks, seed=0):
    """n disjoint grid boxes with distinct scores, threshold 0.5; the boxes at the score ranks `ranks` (none of them
    rank 0) are replaced by copies of the top box shifted by 1/64: IoU (1/2 - 1/64) / (1/2 + 1/64) = 0.94 with the
    top box, 0 with every other unplanted one.  Keep list = score order minus the plants.
    -> boxes, scores, keep, plants (the planted boxes' input indices)."""
    ranks = sorted(set(int(r) for r in ranks))
    assert ranks and 0 < ranks[0] and ranks[-1] < n
    rng = np.random.default_rng(seed)
    by_rank = _grid_boxes(n, rng)
    by_rank[ranks] = by_rank[0] + np.array([0.0, 1.0 / 64, 0.0, 1.0 / 64])
    assert np.array_equal(by_rank.astype(F32).astype(np.float64), by_rank)
    perm = rng.permutation(n)
    boxes, scores = np.zeros((n, 4), F32), np.zeros(n, F32)
    boxes[perm], scores[perm] = by_rank.astype(F32), _distinct_scores(n)
    planted = np.zeros(n, bool)
    planted[ranks] = True
    return boxes, scores, perm[~planted].astype(np.int32), perm[planted].astype(np.int32)


def plant_ranks(plan, n):
    """The ranks grid_with_plants plants for a call with this plan (ops.nms_plan): the last row of each chunk, the
    first row of the next, rank n - 1, and a rank in the column blocks 64 and 65 behind the first chunk's end -- the
    first two column blocks of the second trip of the sweep that hands the first chunk's kept rows on."""
    ranks = set([n - 1])
    for row0, rows in plan['chunks']:
        ranks.update(r for r in (row0 + rows - 1, row0 + rows) if 0 < r < n)
    b1 = (plan['chunks'][0][0] + plan['chunks'][0][1]) // 64
    ranks.update(r for r in ((b1 + 64) * 64 + 5, (b1 + 65) * 64 + 7) if r < n)
    return sorted(ranks)


def exact_threshold():
    """Pairs whose float32 IoU equals the threshold bit for bit, at the threshold (`>` is false: both stay) and at
    the next float32 below it (the later one goes).  Rows are in score order.
    -> list of (id, boxes, scores, thr, keep)."""
    out = []
    triple = np.array([[0, 0, 1, 1], [0, 0, 1, .5], [0, 0, 1, .25]], F32)     # IoU: 01 = 1/2, 02 = 1/4, 12 = 1/2
    s3 = np.array([3, 2, 1], F32)
    half, quarter = F32(0.5), F32(0.25)
    out.append(('triple-0.5', triple, s3, half, [0, 1, 2]))
    out.append(('triple-below-0.5', triple, s3, np.nextafter(half, F32(0)), [0, 2]))       # 0 takes 1; 1 is gone
    out.append(('triple-0.25', triple, s3, quarter, [0, 2]))                               # 0 takes 1, not 2
    out.append(('triple-below-0.25', triple, s3, np.nextafter(quarter, F32(0)), [0]))
    # the pipeline's own thresholds: widths 5/8 and 4/8 -> 0.5 / 0.625, widths 100/128 and 1/128 -> (1/128) / (100/128);
    # the sums and differences are exact and a float32 division rounds 4/5 and 1/100 as the literals round
    s2 = np.array([2, 1], F32)
    for name, thr, wa, wb in (('0.8', F32(0.8), 0.625, 0.5), ('0.01', F32(0.01), 100.0 / 128, 1.0 / 128)):
        pair = np.array([[0, 0, 1, wa], [0, 0, 1, wb]], F32)
        out.append(('pair-' + name, pair, s2, thr, [0, 1]))
        out.append(('pair-below-' + name, pair, s2, np.nextafter(thr, F32(0)), [0]))
    return [(i, b, s, t, np.asarray(k, np.int32)) for i, b, s, t, k in out]


def _order(scores):
    """(score descending, index ascending) as a Python sort on floats: -0.0 == 0.0 there."""
    return np.asarray(sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i)), np.int32)


def ties(n, seed=0):
    """Disjoint grid boxes (nothing is suppressed: the keep list is the candidate order itself).  Scores: 256
    quantised levels, negative but for every 331st row, so the zeros come within the first few hundred candidates;
    level 0 of a negative row is -0.0; a block of -0.0 / +0.0 at random and a block of equal negative scores."""
    rng = np.random.default_rng(seed)
    boxes = _grid_boxes(n, rng).astype(F32)
    scores = (-np.floor(rng.uniform(0, 1, n) * 256) / 256).astype(F32)
    scores[::331] = -scores[::331]
    m = max(min(n // 10, 100), 2)
    scores[n // 5:n // 5 + m] = F32(-0.5)
    scores[n // 2:n // 2 + m] = np.where(rng.integers(0, 2, m) == 1, F32(-0.0), F32(0.0))
    zeros = scores == 0
    assert (zeros & np.signbit(scores)).sum() > m // 4 and (zeros & ~np.signbit(scores)).sum() > m // 4
    assert (scores > 0).sum() + zeros.sum() < 500 or n > 40000     # k = 500 takes every zero and some negatives
    return boxes, scores, _order(scores)


def signed_zeros():
    """Four disjoint boxes scored [-0.0, +0.0, -0.0, +0.0]: all tie, so index order."""
    boxes = np.array([[0, 2 * i, 1, 2 * i + 1] for i in range(4)], F32)
    return boxes, np.array([-0.0, 0.0, -0.0, 0.0], F32), np.arange(4, dtype=np.int32)


def poison(boxes, scores, n_eff):
    """Copies in which the rows from n_eff on, which a call with *d_n = n_eff must not read, hold scores of +inf and
    NaN alternately (a counted +inf would sort first) and boxes of NaN and of +-1e30."""
    b, s = np.array(boxes, F32), np.array(scores, F32)
    lo = max(int(n_eff), 0)
    if lo < len(s):
        odd = (np.arange(len(s) - lo) & 1) == 1         # the first poisoned row scores +inf
        s[lo:] = np.where(odd, F32(np.nan), F32(np.inf))
        b[lo:] = np.where(odd[:, None], np.array([-1e30, -1e30, 1e30, 1e30], F32), F32(np.nan))
    return b, s


# ---- the table --------------------------------------------------------------------------------------------------

CHAINS = ([(n, 0, k) for n in (64, 65, 128, 4500) for k in (1, 32, 33)] +
          [(4500, 0, k) for k in (1024, 2250, 5000)] +
          [(n, 1, 33) for n in (64, 65, 128, 4500)] + [(4500, 1, 1024), (4500, 1, 5000)])
GRIDS = {9000: (300, 9000), 5700: (1024,), 66000: (66000, 3000)}
TIES = [(3000, 3000), (3000, 500), (32768, 500), (32769, 500), (33000, 500)]     # 32768: the last counted-rank size
# device counts: n -> (k, box scale); every n with the n_eff of COUNT_N_EFF, both thresholds
COUNTS = {130: (100, 0.2), 2049: (300, 0.1), 9000: (1024, 0.1), 40000: (300, 0.015)}
COUNT_THRESHOLDS = (0.8, 0.3)


def count_n_eff(n):
    extra = [1000] if n == 9000 else []         # every chunk behind the first lies beyond it
    return [0, 1, 63, 64, 65] + extra + [n // 2, n, n + 1000]


@functools.lru_cache(maxsize=None)
def _chain(n, lead):
    return chain(n, lead, seed=n + lead)


@functools.lru_cache(maxsize=None)
def grid_case(n):
    """The planted grid of n boxes: plants for the plans of every k the table runs it with."""
    from dodt_amd import ops
    ranks = set()
    for k in GRIDS[n]:
        ranks.update(plant_ranks(ops.nms_plan(n, k), n))
    return grid_with_plants(n, ranks, seed=n)


@functools.lru_cache(maxsize=None)
def _ties(n):
    return ties(n, seed=n)


@functools.lru_cache(maxsize=None)
def count_base(n):
    return random_boxes(np.random.default_rng(7 * n + 1), n, COUNTS[n][1])


def chain_cases():
    for n, lead, k in CHAINS:
        b, s, keep = _chain(n, lead)
        yield Case('chain-n%d-lead%d-k%d' % (n, lead, k), b, s, k, F32(0.5), None, keep[:k])


def grid_cases():
    for n, ks in sorted(GRIDS.items()):
        for k in ks:
            b, s, keep, _ = grid_case(n)
            yield Case('grid-n%d-k%d' % (n, k), b, s, k, F32(0.5), None, keep[:k])


def threshold_cases():
    for name, b, s, thr, keep in exact_threshold():
        yield Case('thr-' + name, b, s, 3, thr, None, keep)


def tie_cases():
    b, s, keep = signed_zeros()
    yield Case('zeros-tiny', b, s, 4, F32(0.5), None, keep)
    for n, k in TIES:
        b, s, keep = _ties(n)
        yield Case('ties-n%d-k%d' % (n, k), b, s, k, F32(0.5), None, keep[:k])


def count_cases(sizes=None):
    """Random boxes with poisoned rows behind a device row count; the keep list is the oracle's on the valid rows."""
    for n in sorted(COUNTS):
        if sizes is not None and n not in sizes:
            continue
        k = COUNTS[n][0]
        base_b, base_s = count_base(n)
        for n_eff in count_n_eff(n):
            b, s = poison(base_b, base_s, n_eff)
            for thr in COUNT_THRESHOLDS:
                yield Case('count-n%d-neff%d-thr%g' % (n, n_eff, thr), b, s, k, F32(thr), n_eff, None)


def constructed_cases():
    """Every case with a keep list of its own."""
    for gen in (chain_cases, grid_cases, threshold_cases, tie_cases):
        for c in gen():
            yield c
