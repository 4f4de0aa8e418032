"""The velocity-extrapolating IoU tracker on the device: (i) keyframes per second of tracking.interpolate_by_track (upload,
launches, download and the host-side rebuild of the tracks included) beside the host module
(dodt_amd.experiments.video_detection_iou) on the same synthetic sequence, and (ii) what the stage adds to a pipeline
step: the same pipeline with tracker=dict(kind='velocity') and without a tracker.

    python tools/velocity_tracker_rate.py [--keyframes 120] [--objects 20] [--reps 3] [--steps 60] [--warmup 10]
                                          [--out velocity_tracker_rate.json]

Sequence: `objects` cars driving along their length under a moving ego (0.6 m, 0.02 rad per keyframe of stride 2), every
car missing one keyframe in eight; float32 rows.  A repetition runs the whole sequence; the rate is keyframes divided by
the median wall time of `reps` repetitions behind one warm-up.  The two results are compared track by track before
anything is timed.  Pipeline: synthetic weights, one synthetic frame pair per step with injected heads (the tests'
set-up), wall time of `steps` steps behind `warmup`, enqueued back to back and synchronised once; the two pipelines
alternate, three rounds, the median round counts."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _velocity_cases as V  # noqa: E402
from dodt_amd import config, device, synth, tracking  # noqa: E402
from dodt_amd.experiments import video_detection_iou as vit  # noqa: E402
from dodt_amd.pipeline import FramePairPipeline  # noqa: E402

STRIDE = 2


def ego(a, b):
    trans, matrix, yaw = V.moving(a, b)         # 0.3 m and 0.01 rad per frame
    return trans, matrix, yaw


def sequence(n_key, n_obj):
    rng = np.random.default_rng(n_key * 1000 + n_obj)
    objs = []
    for o in range(n_obj):
        seen = tuple(k for k in range(n_key) if (k + o) % 8 != 7)
        objs.append((-14.0 + 28.0 * (o % 10) / 9 + rng.uniform(-0.5, 0.5), 22.0 + 14.0 * (o // 10) + rng.uniform(-2, 2),
                     rng.uniform(-0.01, 0.01), rng.uniform(0.02, 0.08), 1.5 + rng.uniform(-0.05, 0.05),
                     rng.uniform(0.55, 0.95), seen))
    return V.seq(objs, n_key, STRIDE, ego, V.CALIB_KITTI, np.float32)


def tracker_rates(ctx, n_key, n_obj, reps):
    build = sequence(n_key, n_obj)
    frames_h, stride, frame_num = build()
    frames_d, _, _ = build()
    p = V.PARAMS
    args = (stride, frame_num, p['sigma_l'], p['sigma_h'], p['sigma_iou'], p['t_min'], p['extend_len'])
    want = vit.interpolate_by_track(ego, V.CALIB_KITTI, frames_h, *args)
    got = tracking.interpolate_by_track(ego, V.CALIB_KITTI, frames_d, *args, ctx=ctx)
    V.assert_same_tracks(got, frames_d, want, frames_h)

    def timed(fn):
        out = []
        for _ in range(reps):
            frames = build()[0]
            t0 = time.perf_counter()
            fn(frames)
            out.append(time.perf_counter() - t0)
        return float(np.median(out))
    t_dev = timed(lambda f: tracking.interpolate_by_track(ego, V.CALIB_KITTI, f, *args, ctx=ctx))
    t_host = timed(lambda f: vit.interpolate_by_track(ego, V.CALIB_KITTI, f, *args))
    return dict(keyframes=n_key, objects=n_obj, tracks=len(want), entries=sum(len(t['dets']) for t in want),
                device_keyframes_per_s=round(n_key / t_dev, 1), host_keyframes_per_s=round(n_key / t_host, 1),
                device_ms=round(t_dev * 1e3, 2), host_ms=round(t_host * 1e3, 2))


def pipeline_step(ctx, steps, warmup):
    C = config.PYRAMID_DODT
    kw = dict(rpn_nms_size=1024)
    plain = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), **kw)
    tk = dict(kind='velocity', stride=STRIDE, log_capacity=1 << 16)
    staged = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), tracker=tk, reuse_streams_of=plain, **kw)
    pts = synth.lidar_frame(20, 0)
    d_pts, d_img = ctx.array(pts), ctx.array(synth.image_frame(20, 0))
    heads = {k: ctx.array(v) for k, v in synth.head_outputs(20, 0, plain.n_all, plain.P).items()}
    e = [ego(0, STRIDE)]

    def run(pipe, n):
        for _ in range(n):
            pipe.run([d_pts] * 2, [pts.shape[0]] * 2, [d_img] * 2, heads=[heads] * 2, ego_motion=e)
        pipe.finish()
        ctx.sync()
    rounds = {'plain': [], 'velocity': []}
    for _ in range(3):
        for name, pipe in (('plain', plain), ('velocity', staged)):
            run(pipe, warmup)
            t0 = time.perf_counter()
            run(pipe, steps)
            rounds[name].append((time.perf_counter() - t0) / steps * 1e6)
            if name == 'velocity':
                staged.end_sequence()
    us = {k: float(np.median(v)) for k, v in rounds.items()}
    for p in (staged, plain):
        p.close()
    return dict(steps=steps, us_per_step_plain=round(us['plain'], 1), us_per_step_velocity=round(us['velocity'], 1),
                us_added=round(us['velocity'] - us['plain'], 1),
                rounds={k: [round(x, 1) for x in v] for k, v in rounds.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--keyframes', type=int, default=120)
    ap.add_argument('--objects', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = device.default_context()
    results = dict(tracker=tracker_rates(ctx, args.keyframes, args.objects, args.reps))
    print(json.dumps(results['tracker']), flush=True)
    results['pipeline'] = pipeline_step(ctx, args.steps, args.warmup)
    print(json.dumps(results['pipeline']), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
