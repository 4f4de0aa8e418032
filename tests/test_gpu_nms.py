"""dodt_nms on the device against keep lists known from construction (tests/_nms_cases.py) and the oracle.

Every call goes to ops.nms directly -- a device row count, max_out beyond n, a d_sel of exactly max_out entries
pre-filled with -7 -- and every comparison is exact: the int32 keep list, count_out, and the untouched tail of d_sel.
tests/test_nms_cases.py proves on the host which plan branch each case takes and which structural defect it would
notice.  Needs an MI355X."""
import numpy as np
import pytest

import _nms_cases as nc
from dodt_amd import device, ops
from oracle import tfops

pytestmark = pytest.mark.gpu
FILL = -7


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


def run_nms(ctx, boxes, scores, k, thr, n_eff=None):
    """-> (d_sel as downloaded, all k entries; count)"""
    n = len(scores)
    d_sel = ctx.array(np.full(k, FILL, np.int32))
    d_cnt = ctx.array(np.full(1, FILL, np.int32))
    d_n = None if n_eff is None else ctx.array(np.array([n_eff], np.int32))
    d_boxes = ctx.array(np.ascontiguousarray(boxes, np.float32))
    d_scores = ctx.array(np.ascontiguousarray(scores, np.float32))
    ops.nms(ctx, d_boxes, d_scores, n, d_n, k, float(thr), d_sel, d_cnt)
    sel, cnt = d_sel.download(), int(d_cnt.download()[0])
    # Nothing of the poison (+inf, NaN, 1e30; -7 is a NaN's bit pattern) stays behind in freed device memory: later
    # tests of the suite allocate it again (see the note on uninitialised reads in profiles/nms_tests_summary.md).
    for a in (d_boxes, d_scores, d_sel, d_cnt):
        a.zero()
    ctx.sync()
    return sel, cnt


def check(ctx, c, want):
    sel, cnt = run_nms(ctx, c.boxes, c.scores, c.k, c.thr, c.n_eff)
    assert sel.dtype == np.int32 and len(sel) == c.k
    assert cnt == len(want), (c.id, cnt, len(want))
    assert np.array_equal(sel[:cnt], want), c.id
    assert np.all(sel[cnt:] == FILL), c.id
    return sel[:cnt]


def _ids(cases):
    return [c.id for c in cases]


_CHAINS = list(nc.chain_cases())
_THRESHOLDS = list(nc.threshold_cases())
_TIES = list(nc.tie_cases())


@pytest.mark.parametrize('c', _CHAINS, ids=_ids(_CHAINS))
def test_suppression_chains(ctx, c):
    """Every second box of a chain as long as the input: 64 fixed-point iterations per block, the parity carried
    over every block and chunk seam; k on and around a block's last kept row, in the second chunk, = kept, > n."""
    check(ctx, c, c.keep)


@pytest.mark.parametrize('n,k', [(n, k) for n in sorted(nc.GRIDS) for k in nc.GRIDS[n]])
def test_planted_grids(ctx, n, k):
    """Score order minus the plants: copies of the top box on each chunk's last row, the next chunk's first, the
    last rank, and in the second trip of the sweep behind the first chunk."""
    boxes, scores, keep, plants = nc.grid_case(n)
    got = check(ctx, nc.Case('grid-n%d-k%d' % (n, k), boxes, scores, k, np.float32(0.5), None, keep[:k]), keep[:k])
    assert not np.isin(plants, got).any()
    if k <= 3000:
        assert np.array_equal(got, tfops.non_max_suppression_fast(boxes, scores, k, np.float32(0.5)))


@pytest.mark.parametrize('c', _THRESHOLDS, ids=_ids(_THRESHOLDS))
def test_iou_equal_to_the_threshold_does_not_suppress(ctx, c):
    check(ctx, c, c.keep)


@pytest.mark.parametrize('c', _TIES, ids=_ids(_TIES))
def test_ties_and_signed_zeros_fall_back_to_index_order(ctx, c):
    """Equal scores, -0.0 and +0.0 among them, keep their input order on the counted-rank and the bitonic path."""
    check(ctx, c, c.keep)


@pytest.mark.parametrize('n', sorted(nc.COUNTS))
def test_device_row_count_hides_the_rows_behind_it(ctx, n):
    """n_eff = *d_n from 0 to beyond n, the rows behind it poisoned (+inf / NaN scores, NaN / 1e30 boxes): the
    oracle on the first min(n_eff, n) rows, at both thresholds."""
    seen = 0
    for c in nc.count_cases((n,)):
        valid = min(c.n_eff, n)
        want = tfops.non_max_suppression_fast(c.boxes[:valid], c.scores[:valid], c.k, c.thr)
        check(ctx, c, want)
        seen += 1
    assert seen == 2 * len(nc.count_n_eff(n))


def test_calls_in_sequence_leave_nothing_behind(ctx):
    """One context, so one scratch: a large call stopped early, a tiny one, one walked to the end, the same with 64
    valid rows, and the walked one again -- each checked, so nothing stale in state, keys, ranks, masks or the
    blocks' column form carries over."""
    big_b, big_s = nc.count_base(40000)
    small_b, small_s = nc.count_base(130)
    b9, s9, keep9, _ = nc.grid_case(9000)
    thr = np.float32(0.5)
    steps = [
        nc.Case('40000 stopped early', big_b, big_s, 50, np.float32(0.8), None, None),
        nc.Case('130', small_b, small_s, 130, np.float32(0.3), None, None),
        nc.Case('9000 walked', b9, s9, 9000, thr, None, keep9),
        nc.Case('9000 with 64 rows', b9, s9, 9000, thr, 64, None),
        nc.Case('9000 walked again', b9, s9, 9000, thr, None, keep9),
    ]
    for c in steps:
        want = c.keep
        if want is None:
            valid = len(c.scores) if c.n_eff is None else c.n_eff
            want = tfops.non_max_suppression_fast(c.boxes[:valid], c.scores[:valid], c.k, c.thr)
        check(ctx, c, want)
    assert len(tfops.non_max_suppression_fast(big_b, big_s, 50, np.float32(0.8))) == 50


def test_call_reserves_what_the_plan_says():
    """A fresh context's NMS scratch follows the scratch_bytes of dodt_nms_plan_host call by call (a scratch that has
    to grow takes a quarter more than asked, rounded up to 256 bytes): the call launches from that plan."""
    own = device.Context()
    try:
        assert ops.nms_scratch_bytes(own) == 0
        b, s, keep = nc.chain(4500, 1)
        have = 0
        for n, k in ((130, 10), (4500, 1024), (64, 5), (4500, 5000)):
            sel, cnt = run_nms(own, b[:n], s[:n], k, np.float32(0.5))
            assert 0 < cnt <= k
            need = ops.nms_plan(n, k)['scratch_bytes']
            if need > have:
                have = -(-(need + need // 4) // 256) * 256
            assert ops.nms_scratch_bytes(own) == have
    finally:
        own.close()
