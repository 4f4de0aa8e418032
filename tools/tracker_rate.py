"""Sustained pairs/s of the headline workload with the IoU tracker off, on, and on together with the temporal module M
(FramePairPipeline(tracker=, temporal=)), all in one process, and the tracker's own time per step from HIP events.

    python tools/tracker_rate.py [--kind iou|kalman|velocity] [--steps 2000] [--rounds 2] [--modes f32,bf16]
                                 [--out tracker_rate.json]

Workload (bench.py's headline): tau = 2, 120 000 points, 1 024 proposals, computed heads, one pair per step.  Modes:
f32 (fp32 convs and heads, no look-ahead -- bench.py's fp32 default) and bf16 (--conv-dtype bf16 --head-dtype bf16
with look-ahead).  Every mode times off / on / on+M alternately, `rounds` times, `steps` steps each, behind a warm-up;
the tracked pipelines run one sequence throughout (the reference thresholds, a log of --log entries).  The tracker's
time per step: marks around its launches inside the running pipeline (median over 10 steps), and its launches alone on
the last step's records (mean over 200 back-to-back steps)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dodt_amd import config, device, synth  # noqa: E402
from dodt_amd.pipeline import FramePairPipeline  # noqa: E402


# what the result line shows of the tracker's header, per kind (a missing key is an error, not a gap in the output)
STATE_KEYS = dict(iou=('n_active', 'n_slots', 'n_log', 'n_fin', 'frame_num', 'status'),
                  kalman=('n_live', 'next_id', 'keyframe', 'n_log', 'n_fin', 'status'),
                  velocity=('n_live', 'next_id', 'keyframe', 'n_log', 'n_fin', 'status'))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--modes', default='f32,bf16')
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--proposals', type=int, default=1024)
    ap.add_argument('--tau', type=int, default=2)
    ap.add_argument('--log', type=int, default=1 << 21)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kind', default='iou', choices=('iou', 'kalman', 'velocity'),
                    help='the tracker stage: its default parameters, a parked ego')
    args = ap.parse_args()
    cfg = config.PYRAMID_DODT
    ctx = device.default_context()
    tm = dict(n_frames=args.tau + 1, threshold=0.1, on_conflict='next_best')
    tk = dict(score_threshold=0.1, high_threshold=0.5, iou_threshold=0.005, t_min=3, max_sequence_dets=args.log)
    if args.kind == 'kalman':
        tk = dict(kind='kalman', max_sequence_dets=args.log)
    elif args.kind == 'velocity':
        tk = dict(kind='velocity', log_capacity=args.log)
    hp = synth.head_params()
    # three distinct pairs, resident before timing (bench.py's ring of batches)
    batches = []
    for i in range(3):
        frames = [args.tau * i, args.tau * i + args.tau]
        pts = [synth.lidar_frame(i, f, args.points) for f in frames]
        batches.append(([ctx.array(p) for p in pts], [len(p) for p in pts],
                        [ctx.array(synth.image_frame(i, f)) for f in frames]))
    results = []
    first = None
    for mode in args.modes.split(','):
        dt = 'bf16' if mode == 'bf16' else 'f32'
        ahead = mode == 'bf16'
        pipes = {}
        for label, t, k in (('off', None, None), ('on', None, tk), ('on_m', tm, tk)):
            pipes[label] = FramePairPipeline(ctx, cfg, **synth.pipeline_weights(cfg), n_points_max=args.points,
                                             rpn_nms_size=args.proposals, head_params=hp, conv_dtype=dt, head_dtype=dt,
                                             reuse_streams_of=first, temporal=t, tracker=k)
            first = first or pipes[label]

        def steps(pipe, n):
            for _ in range(n):
                k = pipe.step_idx
                pipe.run(*batches[k % 3], lookahead=batches[(k + 1) % 3] if ahead else None)
            pipe.finish()
            ctx.sync()

        rates = {'off': [], 'on': [], 'on_m': []}
        for pipe in pipes.values():
            steps(pipe, args.warmup)
        for _ in range(args.rounds):
            for label in ('off', 'on', 'on_m'):
                t0 = time.perf_counter()
                steps(pipes[label], args.steps)
                rates[label].append(args.steps / (time.perf_counter() - t0))
        # the tracker inside the running pipeline: marks around its launches on the stream it runs on
        on = pipes['on']
        k0 = on.step_idx
        on.marks, on.mark_steps = {}, set(range(k0 + 5, k0 + 15))
        steps(on, 20)
        inside = []
        for k in sorted(on.mark_steps):
            (c0, s0), (c1, s1) = on.marks['%d:tracker_start' % k], on.marks['%d:tracker_end' % k]
            inside.append(c0.elapsed_ms(s0, c1, s1) * 1e3)
        on.mark_steps, on.marks = (), {}
        # the launches alone, back to back on the last step's records (continuing the sequence)
        st = on._step_record(on.step_idx - 1)
        mc = on.img_ctx         # (the stream the tracker runs on)
        mc.mark(0)
        for _ in range(200):
            on._tracker_step(st)
        mc.mark(1)
        mc.sync()
        alone = mc.elapsed_ms(0, mc, 1) * 1e3 / 200
        ctx.wait_for(mc)
        hdr = on.track_state.header()
        res = dict(kind=args.kind, mode=mode, conv_dtype=dt, head_dtype=dt, lookahead=ahead, steps=args.steps, rounds=args.rounds,
                   pairs_per_s_off=[round(r, 1) for r in rates['off']], pairs_per_s_on=[round(r, 1) for r in rates['on']],
                   pairs_per_s_on_m=[round(r, 1) for r in rates['on_m']],
                   ratio_on_off=round(float(np.mean(rates['on']) / np.mean(rates['off'])), 4),
                   ratio_on_m_off=round(float(np.mean(rates['on_m']) / np.mean(rates['off'])), 4),
                   tracker_us_in_pipeline_median=round(float(np.median(inside)), 1),
                   tracker_us_in_pipeline=[round(v, 1) for v in inside], tracker_us_alone=round(alone, 1),
                   record_rows_last_step=on.d_rec_counts.download().reshape(-1).tolist(),
                   tracker_state={k: hdr[k] for k in STATE_KEYS[args.kind]})
        print(json.dumps(res), flush=True)
        results.append(res)
        for p in pipes.values():
            if p is not first:
                p.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
