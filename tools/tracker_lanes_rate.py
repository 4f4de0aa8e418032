"""Tracker lanes: time per step of S videos side by side, (i) as one dodt_track_lanes call over S lanes and (ii) as S
dodt_track_pairs calls on S separate states on the same stream (what a caller has to do without lanes), from HIP events;
and one lanes pipeline (two videos, two pairs per step) for the record.

    python tools/tracker_lanes_rate.py [--kind iou|kalman|velocity] [--lanes 1,2,4,5,16] [--steps 300] [--warmup 60]
                                       [--pipeline-steps 400] [--out tracker_lanes_rate.json]

--kind kalman / velocity: the same comparison for that tracker -- one dodt_kf_track_lanes / dodt_vt_track_lanes call
against S dodt_kf_track_pairs / dodt_vt_track_pairs calls, every lane parked under KITTI's calibration -- without the
pipeline run.

Records: the tests' generator (tests/_tracking_cases.py sequence(), n_obj = 20, 48 pairs per lane, another seed per
lane), taken in turn -- every lane's state runs on through the wrap, as one long sequence --, resident on the device
before timing.  A step's time is the span between two events on the stream, one recorded behind every step, 100 steps
enqueued back to back between two synchronisations: what the stream needs per step, the host's enqueueing included
where the device waits for it.  Median, fastest and slowest decile over `steps` steps behind `warmup`; both forms
alternate batch by batch in one process.  The pipeline: bench.py's fp32 workload at two pairs per step, tracker off,
the single tracker (both pairs one sequence) and lanes, alternating; pairs/s through finish(), and the marks around the
tracker's launches."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _tracking_cases as tc  # noqa: E402
from dodt_amd import config, device, ops, synth, tracking  # noqa: E402
from dodt_amd.pipeline import FramePairPipeline  # noqa: E402

PARAMS = tc.REFERENCE
N_PAIRS, BATCH = 48, 100


def _stats(us):
    us = np.sort(np.asarray(us))
    return dict(median=round(float(np.median(us)), 1), p10=round(float(us[len(us) // 10]), 1),
                p90=round(float(us[len(us) * 9 // 10]), 1), steps=len(us))


KIND_PARAMS = dict(kalman=dict(sigma_l=0.3, iou_threshold=0.1, max_age=3, min_hits=3),
                   velocity=dict(sigma_l=0.3, sigma_h=0.5, sigma_iou=0.1, t_min=3, extend_len=3, stride=2))


def _kind_forms(ctx, kind, n_lanes, cap):
    """The two forms for kind 'kalman' / 'velocity' -> (lanes object, single trackers, step_lanes(views), step_call(i,
    views)): every lane parked under KITTI's calibration, the score threshold PARAMS'."""
    cal = config.KITTI_CALIBRATION
    c42 = ops.temporal_calib(cal.r0_rect, cal.tr_velo_to_cam)
    p2s, whs, c42s, parked = [cal.p2] * n_lanes, [cal.image_wh] * n_lanes, [c42] * n_lanes, [None] * n_lanes
    lanes_cls, single_cls = ((tracking.KalmanTrackerLanes, tracking.KalmanTracker) if kind == 'kalman'
                             else (tracking.VelocityTrackerLanes, tracking.VelocityTracker))
    lanes = lanes_cls(ctx, n_lanes, log_capacity=cap, score_threshold=PARAMS[0], **KIND_PARAMS[kind])
    singles = [single_cls(ctx, log_capacity=cap, **KIND_PARAMS[kind]) for _ in range(n_lanes)]

    def step_lanes(views, max_det):
        lanes.track_records(*views, max_det, p2s, whs, parked, c42s)

    def step_call(i, views, max_det):
        singles[i].track_records(*views, 1, max_det, cal.p2, cal.image_wh, [None], c42, score_threshold=PARAMS[0])
    return lanes, singles, step_lanes, step_call


def lanes_against_calls(ctx, n_lanes, steps, warmup, cap, kind='iou'):
    score, high, iou, t_min = PARAMS
    seqs = [tc.sequence(1000 + i, N_PAIRS, n_obj=20, empty=(9, 30)) for i in range(n_lanes)]
    max_det = tc.max_rows(*seqs)
    packed = [tc.pack(s, max_det) for s in seqs]
    recs = ctx.array(np.stack([p[0] for p in packed], 1))          # (pairs, lanes, 2, max_det, 17)
    cnts = ctx.array(np.stack([p[1] for p in packed], 1))
    rec_step, cnt_step = n_lanes * 2 * max_det * 17 * 4, n_lanes * 2 * 4
    step_views = [(recs.offset(k * rec_step, (n_lanes, 2, max_det, 17)), cnts.offset(k * cnt_step, (n_lanes, 2), np.int32))
                  for k in range(N_PAIRS)]
    lane_views = [[(recs.offset(k * rec_step + i * rec_step // n_lanes, (1, 2, max_det, 17)),
                    cnts.offset(k * cnt_step + i * 8, (1, 2), np.int32)) for i in range(n_lanes)]
                  for k in range(N_PAIRS)]
    cal = config.KITTI_CALIBRATION
    p2s, whs = [cal.p2] * n_lanes, [cal.image_wh] * n_lanes
    if kind == 'iou':
        lanes = tracking.TrackerLanes(ctx, n_lanes, cap, high, iou, t_min, score)
        singles = [tracking.Tracker(ctx, cap, high, iou, t_min, score) for _ in range(n_lanes)]

        def step_lanes(k):
            lanes.track_records(*step_views[k % N_PAIRS], max_det, p2s, whs)

        def step_calls(k):
            for i, tr in enumerate(singles):
                tr.track_records(*lane_views[k % N_PAIRS][i], 1, max_det, cal.p2, cal.image_wh)
    else:
        lanes, singles, kind_lanes, kind_call = _kind_forms(ctx, kind, n_lanes, cap)

        def step_lanes(k):
            kind_lanes(step_views[k % N_PAIRS], max_det)

        def step_calls(k):
            for i in range(n_lanes):
                kind_call(i, lane_views[k % N_PAIRS][i], max_det)

    times, k = {'lanes': [], 'calls': []}, {'lanes': 0, 'calls': 0}
    for name, fn in (('lanes', step_lanes), ('calls', step_calls)):
        for _ in range(warmup):
            fn(k[name])
            k[name] += 1
    ctx.sync()
    for _ in range(-(-steps // BATCH)):
        for name, fn in (('lanes', step_lanes), ('calls', step_calls)):
            ctx.mark(0)
            for j in range(BATCH):
                fn(k[name])
                k[name] += 1
                ctx.mark(j + 1)
            ctx.sync()
            times[name] += [ctx.elapsed_ms(j, ctx, j + 1) * 1e3 for j in range(BATCH)]
    # both forms tracked the same pairs: the same states
    same = all(lanes.lane(i).header() == singles[i].header() for i in range(n_lanes))
    status = max(tr.header()['status'] for tr in singles)
    chunk = 16 if kind == 'iou' else ops.KIND_LANES_CHUNK
    return dict(kind=kind, lanes=n_lanes, max_det=max_det, us_lanes=_stats(times['lanes']),
                us_calls=_stats(times['calls']), launches_lanes=3 * -(-n_lanes // chunk), launches_calls=3 * n_lanes,
                same_headers=same, status=status)


def pipeline_rates(ctx, steps, warmup, rounds, points, proposals):
    cfg = config.PYRAMID_DODT
    tk = dict(score_threshold=PARAMS[0], high_threshold=PARAMS[1], iou_threshold=PARAMS[2], t_min=PARAMS[3],
              max_sequence_dets=1 << 21)
    hp = synth.head_params()
    batches = []
    for i in range(3):              # two videos: synthetic sequences i and 10 + i, three pairs each in turn
        frames = [(s, f) for s in (i, 10 + i) for f in (0, 2)]
        pts = [synth.lidar_frame(s, f, points) for s, f in frames]
        batches.append(([ctx.array(p) for p in pts], [len(p) for p in pts],
                        [ctx.array(synth.image_frame(s, f)) for s, f in frames]))
    pipes, first = {}, None
    for label, k in (('off', None), ('single', tk), ('lanes', dict(tk, lanes=True))):
        pipes[label] = FramePairPipeline(ctx, cfg, **synth.pipeline_weights(cfg), n_points_max=points,
                                         rpn_nms_size=proposals, head_params=hp, pairs_per_step=2,
                                         reuse_streams_of=first, tracker=k)
        first = first or pipes[label]

    def run(pipe, n):
        for _ in range(n):
            pipe.run(*batches[pipe.step_idx % 3])
        pipe.finish()
        ctx.sync()

    rates = {label: [] for label in pipes}
    for pipe in pipes.values():
        run(pipe, warmup)
    for _ in range(rounds):
        for label, pipe in pipes.items():
            t0 = time.perf_counter()
            run(pipe, steps)
            rates[label].append(2 * steps / (time.perf_counter() - t0))
    marks = {}
    for label in ('single', 'lanes'):
        pipe = pipes[label]
        k0 = pipe.step_idx
        pipe.marks, pipe.mark_steps = {}, set(range(k0 + 5, k0 + 15))
        run(pipe, 20)
        us = []
        for k in sorted(pipe.mark_steps):
            (c0, s0), (c1, s1) = pipe.marks['%d:tracker_start' % k], pipe.marks['%d:tracker_end' % k]
            us.append(round(c0.elapsed_ms(s0, c1, s1) * 1e3, 1))
        pipe.mark_steps, pipe.marks = (), {}
        marks[label] = us
    lanes = pipes['lanes']
    hdr = [lanes.track_state.lane(i).header() for i in range(2)]
    res = dict(pairs_per_step=2, steps=steps, rounds=rounds,
               pairs_per_s={label: [round(r, 1) for r in v] for label, v in rates.items()},
               tracker_us_in_pipeline=marks,
               tracker_us_in_pipeline_median={label: float(np.median(v)) for label, v in marks.items()},
               lane_states=[{k: h[k] for k in ('n_active', 'n_log', 'n_fin', 'seq_pair', 'status')} for h in hdr])
    for p in pipes.values():
        p.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lanes', default='1,2,4,5,16')
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=60)
    ap.add_argument('--log', type=int, default=1 << 16)
    ap.add_argument('--pipeline-steps', type=int, default=400, help='0: no pipeline run')
    ap.add_argument('--pipeline-rounds', type=int, default=2)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--proposals', type=int, default=1024)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kind', default='iou', choices=('iou', 'kalman', 'velocity'),
                    help="which tracker's lanes; the pipeline run is the IoU tracker's only")
    args = ap.parse_args()
    if args.steps < 200:
        ap.error('--steps: at least 200')
    ctx = device.default_context()
    results = dict(tracker=[], pipeline=None)
    for s in (int(v) for v in args.lanes.split(',')):
        res = lanes_against_calls(ctx, s, args.steps, args.warmup, args.log, args.kind)
        print(json.dumps(res), flush=True)
        results['tracker'].append(res)
    if args.pipeline_steps and args.kind == 'iou':
        results['pipeline'] = pipeline_rates(ctx, args.pipeline_steps, 30, args.pipeline_rounds, args.points,
                                             args.proposals)
        print(json.dumps(results['pipeline']), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
