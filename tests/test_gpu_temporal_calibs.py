"""dodt_interpolate_pairs_calibs -- the temporal module with one calibration per pair -- against dodt_interpolate_pairs,
byte for byte.  3 pairs of at most 8 detections per keyframe, n_frames = 3, max_det = 16, with `recover`: the smallest
case in which the pair index is non-zero and both recovered frames (1 and 2) go through recover_row.  Needs an MI355X."""
import numpy as np
import pytest

import _real_clouds as rc
from dodt_amd import device, ops

pytestmark = pytest.mark.gpu
N_PAIRS, MAX_DET, N_FRAMES, MAX_OUT = 3, 16, 3, 32
TAGS = ('trk0001_000000', 'obj000006', 'obj000000')          # three real calibrations


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


def _calib_rows():
    rows = []
    for tag in TAGS:
        r0, tr, _, _ = rc.calib_of(rc.records_by_tag()[tag])
        rows.append(ops.temporal_calib(r0, tr))
    rows = np.stack(rows)
    assert rows.shape == (N_PAIRS, 42) and len({r.tobytes() for r in rows}) == 3
    return rows


def _records(rng):
    """(3, 2, 16, 17) float32 records and (3, 2) counts: per pair some detections seen in both keyframes (moved a
    little), some in one only; scores above the threshold but for one row per keyframe."""
    rec = np.zeros((N_PAIRS, 2, MAX_DET, 17), np.float32)
    cnt = np.zeros((N_PAIRS, 2), np.int32)
    for p in range(N_PAIRS):
        n0, n1 = [(8, 6), (5, 8), (7, 7)][p]
        b0 = np.zeros((n0, 17))
        b0[:, 0] = rng.uniform(-30, 30, n0)
        b0[:, 1] = 1.65 + rng.normal(0, 0.05, n0)
        b0[:, 2] = np.linspace(6, 62, n0) + rng.normal(0, 0.3, n0)
        b0[:, 3:6] = [3.9, 1.6, 1.5] + rng.normal(0, 0.05, (n0, 3))
        b0[:, 6] = rng.uniform(-3.1, 3.1, n0)
        b0[:, 7] = rng.uniform(0.3, 0.9, n0)
        b0[:, 9:16] = b0[:, :7] + rng.normal(0, 0.3, (n0, 7))
        b0[::2, 13:15] = rng.normal(0, 0.3, (len(b0[::2]), 2))
        shared = min(n0, n1) - 2
        b1 = np.zeros((n1, 17))
        b1[:, :9] = np.concatenate([b0[:shared, :9], b0[:n1 - shared, :9] + [100.0, 0, 0, 0, 0, 0, 0, 0, 0]])
        b1[:shared, [0, 2]] += rng.normal(0, 0.2, (shared, 2))
        b1[:, 6] += rng.normal(0, 0.03, n1)
        b1[:, 7] = rng.uniform(0.3, 0.9, n1)
        b1[:, 16] = 1
        b0[-1, 7] = b1[-1, 7] = 0.05                 # below the threshold
        rec[p, 0, :n0], rec[p, 1, :n1] = b0, b1
        cnt[p] = n0, n1
    return rec, cnt


def _ego(rng):
    ego = []
    for _ in range(N_PAIRS):
        per_frame = []
        for f in range(1, N_FRAMES):
            a = rng.uniform(-0.05, 0.05)
            m = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
            per_frame.append((rng.normal(0, 0.6, 3) * [1, 0.2, 0.02] * f, m, a))
        ego.append(per_frame)
    return np.stack([ops.temporal_ego(e, N_FRAMES) for e in ego])


@pytest.fixture(scope='module')
def case(ctx):
    rng = np.random.default_rng(20261019)
    rec, cnt = _records(rng)
    return dict(rec=rec, cnt=cnt, ego=_ego(rng), rows=_calib_rows(), d_rec=ctx.array(rec), d_cnt=ctx.array(cnt))


def _run(ctx, case, d_rec, d_cnt, n_pairs, ego, on_conflict='next_best', **calib):
    out = ctx.zeros((n_pairs, N_FRAMES, MAX_OUT, 13), np.float64)
    counts = ctx.zeros((n_pairs, N_FRAMES), np.int32)
    status = ctx.zeros((n_pairs,), np.int32)
    ops.interpolate_pairs(ctx, d_rec, d_cnt, n_pairs, MAX_DET, N_FRAMES, 0.1, on_conflict, out, counts, status,
                          d_recover=ctx.array(ego), max_out=MAX_OUT, **calib)
    ctx.sync()
    return out.download(), counts.download(), status.download()


def _same_bytes(got, want, what):
    for g, w, name in zip(got, want, ('frames', 'counts', 'status')):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert g.tobytes() == w.tobytes(), (what, name)


def test_identical_rows_equal_the_one_calibration_entry(ctx, case):
    for i in range(N_PAIRS):
        rows = np.stack([case['rows'][i]] * N_PAIRS)
        got = _run(ctx, case, case['d_rec'], case['d_cnt'], N_PAIRS, case['ego'], d_calibs=ctx.array(rows))
        want = _run(ctx, case, case['d_rec'], case['d_cnt'], N_PAIRS, case['ego'], calib=case['rows'][i])
        assert np.all(want[2] == 0) and np.all(want[1] > 0)            # every frame of every pair has rows
        _same_bytes(got, want, 'calibration %d' % i)


def test_different_rows_equal_the_entry_called_once_per_pair(ctx, case):
    got = _run(ctx, case, case['d_rec'], case['d_cnt'], N_PAIRS, case['ego'], d_calibs=ctx.array(case['rows']))
    one = _run(ctx, case, case['d_rec'], case['d_cnt'], N_PAIRS, case['ego'], calib=case['rows'][0])
    for p in range(N_PAIRS):
        want = _run(ctx, case, ctx.array(case['rec'][p:p + 1]), ctx.array(case['cnt'][p:p + 1]), 1,
                    case['ego'][p:p + 1], calib=case['rows'][p])
        _same_bytes([g[p:p + 1] for g in got], want, 'pair %d' % p)
        # ... and the calibration matters: pairs 1 and 2 recovered with pair 0's are other bytes (frames 1 and 2; frame
        # 0 is never recovered)
        same_as_one = got[0][p].tobytes() == one[0][p].tobytes()
        assert same_as_one == (p == 0)
        assert got[0][p, 0].tobytes() == one[0][p, 0].tobytes()
        for f in (1, 2):
            assert (got[0][p, f].tobytes() == one[0][p, f].tobytes()) == (p == 0)


def test_float64_records_and_raise_mode(ctx, case):
    d_rec64 = ctx.array(case['rec'].astype(np.float64))
    got = _run(ctx, case, d_rec64, case['d_cnt'], N_PAIRS, case['ego'], on_conflict='raise',
               d_calibs=ctx.array(case['rows']))
    for p in range(N_PAIRS):
        want = _run(ctx, case, ctx.array(case['rec'][p:p + 1].astype(np.float64)), ctx.array(case['cnt'][p:p + 1]), 1,
                    case['ego'][p:p + 1], on_conflict='raise', calib=case['rows'][p])
        _same_bytes([g[p:p + 1] for g in got], want, 'pair %d' % p)


def test_argument_checks(ctx, case):
    out = ctx.zeros((N_PAIRS, N_FRAMES, MAX_OUT, 13), np.float64)
    counts, status = ctx.zeros((N_PAIRS, N_FRAMES), np.int32), ctx.zeros((N_PAIRS,), np.int32)
    args = (ctx, case['d_rec'], case['d_cnt'], N_PAIRS, MAX_DET, N_FRAMES, 0.1, 'raise', out, counts, status)
    d_ego, d_rows = ctx.array(case['ego']), ctx.array(case['rows'])
    with pytest.raises(ValueError):                  # rows without recover
        ops.interpolate_pairs(*args, d_calibs=d_rows, max_out=MAX_OUT)
    with pytest.raises(ValueError):                  # both forms
        ops.interpolate_pairs(*args, d_recover=d_ego, d_calibs=d_rows, calib=case['rows'][0], max_out=MAX_OUT)
    with pytest.raises(ValueError):                  # one row too few
        ops.interpolate_pairs(*args, d_recover=d_ego, d_calibs=ctx.array(case['rows'][:2]), max_out=MAX_OUT)
    with pytest.raises(ValueError):
        ops.interpolate_pairs(*args, d_recover=d_ego, d_calibs=ctx.array(case['rows'].astype(np.float32)),
                              max_out=MAX_OUT)
