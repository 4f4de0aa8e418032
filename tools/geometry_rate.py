"""Pairs/s of the headline workload with the geometry given per step (run(..., calib=)), and what one rebuild of the BEV
skip tables costs when the union of the calibrations' supports grows.

    python tools/geometry_rate.py [--steps 400] [--runs 3] [--out profiles/per_sample_geometry_summary.md]
                                  [--parent-json FILE]
    python tools/geometry_rate.py --tree DIR --json FILE      # form (a) alone, on another (built) checkout

The workload of bench.py's defaults: fp32 convs and heads, computed heads, 120 000 points, 1 024 proposals, one pair per
step, no look-ahead, records into a caller's ring, three synthetic batches resident in HBM and taken in turn.  One
pipeline, one process, the forms alternating run by run:
  (a) no `calib` argument;
  (b) the constructor's calibration passed explicitly with every step;
  (c) two calibrations (and image sizes) alternating every step, after both have been seen;
and two controls that tell the mechanism from the samples -- a step under another camera is other work: another
frustum, another number of kept anchors --
  (b2) the second calibration alone, explicit with every step;
  (c0) two calibrations alternating that differ in the last bit of p2[0][0] alone (two values, the same work);
then, on the drained pipeline,
  (d) the milliseconds of the host call that brings a third calibration whose support grows the union -- its mask on
      the host, the stream synchronisation, every table freed and made again --, and the wall time of the step behind
      it (full tables) against a step with a calibration already seen.
--tree DIR measures (a) on the checkout at DIR (the parent commit's, for the yardstick: it has no `calib`), the same
way in a process of its own; --parent-json takes that run's numbers into the summary."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# KITTI object frames 000006 / 000000 (numbers only): the two other cameras of the bundled real clouds
OTHERS = [
    dict(p2=[[718.3351, 0.0, 600.3891, 44.50382], [0.0, 718.3351, 181.5122, -0.5951107], [0.0, 0.0, 1.0, 0.002616315]],
         r0_rect=[[0.9999478, 0.009791707, -0.002925305], [-0.009806939, 0.9999382, -0.005238719],
                  [0.002873828, 0.005267134, 0.999982]],
         tr_velo_to_cam=[[0.007755449, -0.9999694, -0.001014303, -0.007275538],
                         [0.002294056, 0.001032122, -0.9999968, -0.06324057],
                         [0.9999673, 0.007753097, 0.00230199, -0.2670414]], image_wh=(1238, 374)),
    dict(p2=[[707.0493, 0.0, 604.0814, 45.75831], [0.0, 707.0493, 180.5066, -0.3454157], [0.0, 0.0, 1.0, 0.004981016]],
         r0_rect=[[0.9999128, 0.01009263, -0.008511932], [-0.01012729, 0.9999406, -0.004037671],
                  [0.008470675, 0.004123522, 0.9999556]],
         tr_velo_to_cam=[[0.006927964, -0.9999722, -0.002757829, -0.02457729],
                         [-0.001162982, 0.002749836, -0.9999955, -0.06127237],
                         [0.9999753, 0.006931141, -0.001143899, -0.3321029]], image_wh=(1224, 370)),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--proposals', type=int, default=1024)
    ap.add_argument('--tree', default=None, help='another built checkout: measure form (a) alone on it')
    ap.add_argument('--json', default=None, help='write the result line here as well')
    ap.add_argument('--parent-json', default=None, help="a --tree run's result, for the summary")
    ap.add_argument('--out', default=None, help='markdown summary to write')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    from dodt_amd import config, device, synth
    from dodt_amd.pipeline import FramePairPipeline, MAX_DET, REC_COLS

    cfg = config.PYRAMID_DODT
    ctx = device.default_context()
    pipe = FramePairPipeline(ctx, cfg, **synth.pipeline_weights(cfg), n_points_max=args.points,
                             rpn_nms_size=args.proposals, head_params=synth.head_params())
    ring = (ctx.zeros((16, 1, 2, MAX_DET, REC_COLS), np.float32), ctx.zeros((16, 1, 2), np.int32))
    pipe.use_record_ring(*ring)
    forms = ['a']
    cals = [None]
    if not args.tree:
        forms += ['b', 'c', 'b2', 'c0']
        cals = [config.KITTI_CALIBRATION] + [config.Calibration(**o) for o in OTHERS]
        p2 = cals[0].p2.copy()
        p2[0, 0] = np.nextafter(p2[0, 0], 1e9)
        twin = cals[0]._replace(p2=p2)
    batches = []
    for i in range(3):
        pts = [synth.lidar_frame(i, f, args.points) for f in (2 * i, 2 * i + 2)]
        imgs = {}
        for c in cals:
            wh = synth.IMAGE_WH if c is None else c.image_wh
            imgs[wh] = [ctx.array(synth.image_frame(i, f, wh)) for f in (2 * i, 2 * i + 2)]
        batches.append(dict(pts=[ctx.array(p) for p in pts], n=[len(p) for p in pts], imgs=imgs))

    def step(calib, explicit):
        b = batches[pipe.step_idx % 3]
        wh = synth.IMAGE_WH if calib is None else calib.image_wh
        if explicit:
            pipe.run(b['pts'], b['n'], b['imgs'][wh], calib=calib)
        else:
            pipe.run(b['pts'], b['n'], b['imgs'][wh])

    kept = {}

    def chain(form, steps):
        ctx.sync()
        t0 = time.perf_counter()
        for i in range(steps):
            if form == 'a':
                step(None, False)
            elif form == 'b':
                step(cals[0], True)
            elif form == 'b2':
                step(cals[1], True)
            elif form == 'c0':
                step((cals[0], twin)[i % 2], True)
            else:
                step(cals[i % 2], True)
        pipe.finish()
        ctx.sync()
        seconds = time.perf_counter() - t0
        kept[form] = [int(v) for v in pipe.last_anchor_counts]     # (of the chain's last step)
        return steps / seconds

    for form in forms:                              # warm-up, not reported; (c) sees its second calibration here
        chain(form, 40)
    rates = {form: [] for form in forms}
    for _ in range(args.runs):
        for form in forms:
            rates[form].append(round(chain(form, args.steps), 1))
    res = dict(tree=args.tree or '.', steps=args.steps, runs=args.runs, points=args.points, proposals=args.proposals,
               pairs_per_s=rates, slowest={f: min(r) for f, r in rates.items()},
               spread={f: round(max(r) - min(r), 1) for f, r in rates.items()}, anchors_kept_last_step=kept)
    if not args.tree:
        res['bev_skipped_items'] = dict(seen_by_the_forms=int(pipe.bev_skipped_items))
        res['rebuilds_before_d'] = pipe.support.rebuilds

        def one_step(calib):                        # a whole step, enqueue to drained, in ms
            ctx.sync()
            t0 = time.perf_counter()
            step(calib, True)
            pipe.finish()
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3
        seen = [one_step(cals[1]) for _ in range(5)]
        g = pipe._geometry(cals[2])
        ctx.sync()
        t0 = time.perf_counter()
        pipe._grow_support([g])
        ctx.sync()
        rebuild_ms = (time.perf_counter() - t0) * 1e3
        first = one_step(cals[2])
        again = [one_step(cals[2]) for _ in range(5)]
        res['rebuild'] = dict(rebuild_ms=round(rebuild_ms, 2), rebuilds=pipe.support.rebuilds,
                              step_behind_it_ms=round(first, 2), step_seen_ms=round(float(np.median(seen)), 2),
                              step_third_seen_ms=round(float(np.median(again)), 2))
        res['bev_skipped_items']['three_calibrations'] = int(pipe.bev_skipped_items)
        if args.parent_json:
            with open(args.parent_json) as f:
                res['parent'] = json.loads(f.read())
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            f.write(line + '\n')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(markdown(res))
    pipe.close()


def markdown(r):
    out = ['# Per-sample geometry: rates with `calib=` and the cost of a skip-table rebuild', '',
           '`python tools/geometry_rate.py --steps %d --runs %d`: bench.py\'s default workload (fp32, computed heads, %d '
           'points, %d proposals, one pair per step, records into a ring), %d steps per run through `finish()`, the '
           'forms alternating run by run in one process.' % (r['steps'], r['runs'], r['points'], r['proposals'],
                                                             r['steps']), '',
           '| form | pairs/s per run | slowest | spread |', '|---|---|---|---|']
    names = dict(a='(a) no `calib`', b='(b) the constructor\'s calibration, explicit',
                 c='(c) two calibrations alternating', b2='(b2) control: the second calibration alone',
                 c0='(c0) control: two calibrations one bit apart, alternating')
    p = r.get('parent')
    if p:
        out.append('| parent commit, (a), own process | %s | %.1f | %.1f |' % (
            ', '.join('%.1f' % v for v in p['pairs_per_s']['a']), p['slowest']['a'], p['spread']['a']))
    for f in ('a', 'b', 'c', 'b2', 'c0'):
        out.append('| %s | %s | %.1f | %.1f |' % (names[f], ', '.join('%.1f' % v for v in r['pairs_per_s'][f]),
                                                  r['slowest'][f], r['spread'][f]))
    out += ['', 'Kept anchors of the last step of a run (frame 0, frame 1): %s.' % ', '.join(
        '%s %s' % (f, r['anchors_kept_last_step'][f]) for f in ('a', 'b', 'c', 'b2', 'c0')), '']
    if p:
        floor = p['slowest']['a'] - p['spread']['a']
        out += ['Yardstick: the parent\'s slowest run less its own run-to-run spread, %.1f pairs/s.  (a) %s, (b) %s.' % (
            floor, 'not below it' if r['slowest']['a'] >= floor else '**BELOW** it',
            'not below it' if r['slowest']['b'] >= floor else '**BELOW** it'), '']
    d = r['rebuild']
    out += ['## (d) one rebuild', '',
            'A third calibration whose support has cells outside the union of the first two: the host call that takes it '
            'in (its mask on the host, the stream synchronisation, every table freed and made again) took **%.2f ms**; the '
            'step behind it, on full tables, %.2f ms from enqueue to drained, against %.2f ms for a step of a calibration '
            'already seen and %.2f ms for the third one from then on.  Rebuilds so far: %d (one per calibration).  Items '
            'the BEV net skips per forward: %d under the union the forms above had seen, %d with the third.' % (
                d['rebuild_ms'], d['step_behind_it_ms'], d['step_seen_ms'], d['step_third_seen_ms'], d['rebuilds'],
                r['bev_skipped_items']['seen_by_the_forms'], r['bev_skipped_items']['three_calibrations']), '']
    return '\n'.join(out)


if __name__ == '__main__':
    main()
