"""The Kalman-filter tracker on the device: time per step from HIP events, (i) one dodt_kf_track_pairs step (one pair:
encode, IoU matrix, step kernel) beside one dodt_track_pairs step of the IoU tracker on the same records and stream, and
(ii) dodt_kf_assign alone on random matrices.

    python tools/kalman_tracker_rate.py [--steps 300] [--warmup 60] [--assign 16,128] [--out kalman_tracker_rate.json]

Records: the tests' generator (tests/_tracking_cases.py sequence(), n_obj = 20, 48 pairs), taken in turn -- both states
run on through the wrap, as one long sequence --, resident on the device before timing; the ego moves 0.6 m and turns
0.02 rad per pair.  A step's time is the span between two events on the stream, one recorded behind every step, 100
steps enqueued back to back between two synchronisations: what the stream needs per step, the host's enqueueing included
where the device waits for it.  Median, fastest and slowest decile over `steps` steps behind `warmup`; the two trackers
alternate batch by batch in one process.  The assignment: square float32 matrices of uniform entries in [0, 1), a new
one per call out of eight."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _tracking_cases as tc  # noqa: E402
from dodt_amd import config, device, ops, tracking  # noqa: E402

N_PAIRS, BATCH = 48, 100


def _stats(us):
    us = np.sort(np.asarray(us))
    return dict(median=round(float(np.median(us)), 1), p10=round(float(us[len(us) // 10]), 1),
                p90=round(float(us[len(us) * 9 // 10]), 1), steps=len(us))


def _timed(ctx, fns, steps, warmup):
    """{name: us per step} of the step functions fns[name](k), alternating batch by batch."""
    times, k = {n: [] for n in fns}, {n: 0 for n in fns}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn(k[name])
            k[name] += 1
    ctx.sync()
    for _ in range(-(-steps // BATCH)):
        for name, fn in fns.items():
            ctx.mark(0)
            for j in range(BATCH):
                fn(k[name])
                k[name] += 1
                ctx.mark(j + 1)
            ctx.sync()
            times[name] += [ctx.elapsed_ms(j, ctx, j + 1) * 1e3 for j in range(BATCH)]
    return {n: _stats(v) for n, v in times.items()}


def kalman_against_iou(ctx, steps, warmup, cap):
    score, high, iou, t_min = tc.REFERENCE
    seq = tc.sequence(1000, N_PAIRS, n_obj=20, empty=(9, 30))
    max_det = tc.max_rows(seq)
    recs_h, cnts_h = tc.pack(seq, max_det)
    recs, cnts = ctx.array(recs_h), ctx.array(cnts_h)
    views = [(recs.offset(k * 2 * max_det * 17 * 4, (1, 2, max_det, 17)), cnts.offset(k * 8, (1, 2), np.int32))
             for k in range(N_PAIRS)]
    cal = config.KITTI_CALIBRATION
    cal42 = ops.temporal_calib(cal.r0_rect, cal.tr_velo_to_cam)
    c, s = np.cos(0.02), np.sin(0.02)
    ego = [(np.array([0.6, 0.0, 0.0]), np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]), 0.02)]
    kf = tracking.KalmanTracker(ctx, sigma_l=0.3, iou_threshold=0.1, log_capacity=cap)
    it = tracking.Tracker(ctx, cap, high, iou, t_min, score)

    def step_kf(k):
        kf.track_records(*views[k % N_PAIRS], 1, max_det, cal.p2, cal.image_wh, ego, cal42, score_threshold=score)

    def step_iou(k):
        it.track_records(*views[k % N_PAIRS], 1, max_det, cal.p2, cal.image_wh)

    us = _timed(ctx, {'kalman': step_kf, 'iou': step_iou}, steps, warmup)
    h = kf.header()
    return dict(max_det=max_det, us_kalman=us['kalman'], us_iou=us['iou'], launches_kalman=3, launches_iou=3,
                kalman_state={k: h[k] for k in ('n_live', 'next_id', 'n_log', 'n_fin', 'keyframe', 'status')},
                iou_status=it.header()['status'])


def assign_alone(ctx, n, steps, warmup):
    rng = np.random.default_rng(n)
    mats = [ctx.array(rng.uniform(0, 1, size=(n, n)).astype(np.float32)) for _ in range(8)]
    d_m, d_ud, d_ut, d_c = (ctx.zeros((n, 2), np.int32), ctx.zeros((n,), np.int32), ctx.zeros((n,), np.int32),
                            ctx.zeros((4,), np.int32))

    def step(k):
        ops.kf_assign(ctx, mats[k % 8], n, n, 0.1, d_m, d_ud, d_ut, d_c)

    us = _timed(ctx, {'assign': step}, steps, warmup)['assign']
    return dict(n=n, us_assign=us, matched=int(d_c.download()[0]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=60)
    ap.add_argument('--log', type=int, default=1 << 17)
    ap.add_argument('--assign', default='16,128')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.steps < 200:
        ap.error('--steps: at least 200')
    ctx = device.default_context()
    results = dict(step=kalman_against_iou(ctx, args.steps, args.warmup, args.log), assign=[])
    print(json.dumps(results['step']), flush=True)
    for n in (int(v) for v in args.assign.split(',')):
        res = assign_alone(ctx, n, args.steps, args.warmup)
        print(json.dumps(res), flush=True)
        results['assign'].append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
