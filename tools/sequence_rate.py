"""Pairs/s of one chain of keyframes driven through the pipeline as explicit pairs (run()) and as a sequence
(FramePairPipeline(sequence=True), push_frame()), in one process, runs alternating.

    python tools/sequence_rate.py [--keyframes 240] [--runs 3] [--modes f32,bf16] [--out profiles/sequence_mode_summary.md]

One synthetic sequence: keyframes synth.lidar_frame(seq, tau * j) / image_frame(seq, tau * j), resident in HBM before
timing; pair j is keyframes (j, j + 1), so both modes compute the same keyframes - 1 pairs and pair mode is the
yardstick (existing code, same machine, same process).  Modes: f32 (fp32 convs and heads, no look-ahead) and bf16
(bf16 convs and heads, with look-ahead).  Computed heads, 1 024 proposals, records into a caller's ring as a streaming
caller has them.  Per run: pairs/s over the whole chain (first call to the end of the drain), the host's
enqueue-to-enqueue time per step as percentiles (the host runs one step ahead of the GPU, so over a chain they are the
GPU's step times) and the host's own enqueue time per step.  The last pair's records of both modes are compared."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dodt_amd import config, device, synth  # noqa: E402
from dodt_amd.pipeline import FramePairPipeline, MAX_DET, REC_COLS  # noqa: E402

PCT = (('p01', 1), ('p50', 50), ('p90', 90), ('p99', 99))


def chain(pipe, keys, ahead, ctx):
    """All pairs of the chain through `pipe`; (seconds, per-step host times in ms, host enqueue ms per step)."""
    n = len(keys)

    def frame(j):
        return keys[j] if j < n else None

    def pair(j):
        return tuple([keys[j][i], keys[j + 1][i]] for i in range(3)) if j + 1 < n else None

    ctx.sync()
    stamps, busy = [], 0.0
    t0 = time.perf_counter()
    if pipe.sequence:
        pipe.push_frame(*frame(0), lookahead=frame(1) if ahead else None)
        stamps.append(time.perf_counter())
        for j in range(1, n):
            th = time.perf_counter()
            pipe.push_frame(*frame(j), lookahead=frame(j + 1) if ahead else None)
            stamps.append(time.perf_counter())
            busy += stamps[-1] - th
    else:
        stamps.append(t0)
        for j in range(n - 1):
            th = time.perf_counter()
            pipe.run(*pair(j), lookahead=pair(j + 1) if ahead else None)
            stamps.append(time.perf_counter())
            busy += stamps[-1] - th
    pipe.finish()
    ctx.sync()
    seconds = time.perf_counter() - t0
    if pipe.sequence:
        pipe.end_sequence()
    return seconds, np.diff(stamps) * 1e3, busy / (n - 1) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--keyframes', type=int, default=240)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--modes', default='f32,bf16')
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--proposals', type=int, default=1024)
    ap.add_argument('--tau', type=int, default=2)
    ap.add_argument('--seq', type=int, default=0)
    ap.add_argument('--out', default=None, help='markdown summary to write')
    args = ap.parse_args()
    if args.keyframes < 200:
        ap.error('at least 200 keyframes')
    cfg = config.PYRAMID_DODT
    ctx = device.default_context()
    hp = synth.head_params()
    keys = []
    for j in range(args.keyframes):
        p = synth.lidar_frame(args.seq, args.tau * j, args.points)
        keys.append((ctx.array(p), len(p), ctx.array(synth.image_frame(args.seq, args.tau * j))))
    n_pairs = args.keyframes - 1
    results, first = [], None
    for mode in args.modes.split(','):
        dt = 'bf16' if mode == 'bf16' else 'f32'
        ahead = mode == 'bf16'
        pipes, rings = {}, {}
        for label in ('pair', 'sequence'):
            pipes[label] = FramePairPipeline(ctx, cfg, **synth.pipeline_weights(cfg), n_points_max=args.points,
                                             rpn_nms_size=args.proposals, head_params=hp, conv_dtype=dt, head_dtype=dt,
                                             reuse_streams_of=first, sequence=label == 'sequence')
            first = first or pipes[label]
            rings[label] = (ctx.zeros((4, 1, 2, MAX_DET, REC_COLS), np.float32), ctx.zeros((4, 1, 2), np.int32))
            pipes[label].use_record_ring(*rings[label])
        runs = {'pair': [], 'sequence': []}
        for label in ('pair', 'sequence'):                       # warm-up: one chain each, not reported
            chain(pipes[label], keys[:40], ahead, ctx)
        for _ in range(args.runs):
            for label in ('pair', 'sequence'):
                seconds, step_ms, enqueue_ms = chain(pipes[label], keys, ahead, ctx)
                runs[label].append(dict(
                    pairs_per_s=round(n_pairs / seconds, 1), seconds=round(seconds, 3),
                    step_ms={q: round(float(np.percentile(step_ms[5:], p)), 3) for q, p in PCT},
                    host_enqueue_ms=round(enqueue_ms, 3)))
        same = all(np.array_equal(pipes['pair'].__dict__[n].download(), pipes['sequence'].__dict__[n].download())
                   for n in ('d_records', 'd_rec_counts'))
        rate = {label: [r['pairs_per_s'] for r in rs] for label, rs in runs.items()}
        res = dict(mode=mode, conv_dtype=dt, head_dtype=dt, lookahead=ahead, keyframes=args.keyframes, pairs=n_pairs,
                   points=args.points, proposals=args.proposals, runs=runs,
                   slowest=dict(pair=min(rate['pair']), sequence=min(rate['sequence'])),
                   sequence_not_below_pair=min(rate['sequence']) >= min(rate['pair']),
                   gain_of_medians=round(float(np.median(rate['sequence']) / np.median(rate['pair'])), 4),
                   gain_range=[round(min(rate['sequence']) / max(rate['pair']), 4),
                               round(max(rate['sequence']) / min(rate['pair']), 4)],
                   last_pair_records_equal=bool(same),
                   gflop_per_step=dict(pair=round(pipes['pair'].flops_per_step() / 1e9, 2),
                                       sequence=round(pipes['sequence'].flops_per_step() / 1e9, 2)))
        print(json.dumps(res), flush=True)
        results.append(res)
        for p in pipes.values():
            if p is not first:
                p.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(markdown(results, args))


def markdown(results, args):
    out = ['# Sequence mode against pair mode: one chain of keyframes, runs alternating', '',
           '`python tools/sequence_rate.py --keyframes %d --runs %d --modes %s`: %d keyframes of one synthetic sequence '
           '(%d points, %d proposals, computed heads, records into a ring), i.e. %d pairs per run; pair mode (`run()`, '
           'every inner keyframe handed over and computed twice) and sequence mode (`push_frame()`) alternate in one '
           'process.  pairs/s is over the whole chain including its drain; step times are the host\'s '
           'enqueue-to-enqueue times.' % (args.keyframes, args.runs, args.modes, args.keyframes, args.points,
                                          args.proposals, args.keyframes - 1), '']
    for r in results:
        out += ['## %s convs and heads%s' % (r['conv_dtype'], ', look-ahead' if r['lookahead'] else ''), '',
                '| run | mode | pairs/s | ms/step p01 | p50 | p90 | p99 | host_enqueue_ms / step |', '|---|---|---|---|---|---|---|---|']
        for i in range(len(r['runs']['pair'])):
            for label in ('pair', 'sequence'):
                x = r['runs'][label][i]
                out.append('| %d | %s | %.1f | %.3f | %.3f | %.3f | %.3f | %.3f |' % (
                    i + 1, label, x['pairs_per_s'], x['step_ms']['p01'], x['step_ms']['p50'], x['step_ms']['p90'],
                    x['step_ms']['p99'], x['host_enqueue_ms']))
        out += ['', 'Slowest run: pair %.1f, sequence %.1f pairs/s -- sequence mode\'s slowest run is %s pair mode\'s '
                'slowest.  Ratio of the medians %.3f; from sequence\'s slowest over pair\'s fastest to the reverse: '
                '%.3f .. %.3f.  Conv work per step: %.2f against %.2f GFLOP.  Last pair\'s records byte-equal: %s.' % (
                    r['slowest']['pair'], r['slowest']['sequence'],
                    'not below' if r['sequence_not_below_pair'] else '**BELOW**', r['gain_of_medians'],
                    r['gain_range'][0], r['gain_range'][1], r['gflop_per_step']['sequence'],
                    r['gflop_per_step']['pair'], r['last_pair_records_equal']), '']
    return '\n'.join(out)


if __name__ == '__main__':
    main()
