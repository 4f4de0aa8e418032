"""What tests/test_gpu_multiclass_pipeline.py runs in its own process and, for the tail's unfused form
(DODT_PIPE_FUSED_TAIL=0, read when a pipeline is built), in a child process:

    python tests/_multiclass_pipeline.py <cls_out bias shift> <out.npz>

writes the records of the people configuration's single frame."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dodt_amd import config, synth  # noqa: E402
from dodt_amd.pipeline import MAX_DET, FramePairPipeline  # noqa: E402

PEOPLE = ('Pedestrian', 'Cyclist')
N_POINTS = 20000
RPN_NMS_SIZE = 256
SEQ = 21


def head_params(shift):
    """synth's seeded heads with three stage-2 classification columns; `shift` is added to the last column's bias."""
    hp = synth.head_params(n_classes=3)
    b = hp['avod']['cls_out']['b']
    hp['avod']['cls_out']['b'] = (b + np.array([0.0, 0.0, shift], np.float32)).astype(np.float32)
    return hp


def balancing_shift(logits):
    """The shift of column 2 under which the MAX_DET rows with the largest non-background logit split most evenly."""
    d = (logits[:, 1] - logits[:, 2]).astype(np.float64)
    best, best_err = 0.0, 2.0
    for s in np.quantile(d, np.linspace(0.02, 0.98, 49)):
        c2 = logits[:, 2] + s
        top = np.argsort(-np.maximum(logits[:, 1], c2), kind='stable')[:MAX_DET]
        err = abs(float(np.mean(c2[top] > logits[top, 1])) - 0.5)
        if err < best_err:
            best, best_err = float(s), err
    return best


def type_shares(rec, n):
    return np.bincount(rec[:n, 8].astype(np.int64), minlength=2) / max(n, 1)


def frame_inputs(seq=SEQ, frame=0):
    return synth.lidar_frame(seq, frame, N_POINTS), synth.image_frame(seq, frame)


def run_single_frame(ctx, shift, cfg=config.PYRAMID_PEOPLE, reuse=None):
    """One single frame through a pipeline of `cfg` that computes its heads.  -> (pipe, points)."""
    pipe = FramePairPipeline(ctx, cfg, rpn_nms_size=RPN_NMS_SIZE, head_params=head_params(shift),
                             reuse_streams_of=reuse, **synth.pipeline_weights(cfg))
    pts, img = frame_inputs()
    pipe.run([ctx.array(pts)], [len(pts)], [ctx.array(img)])
    pipe.finish()
    ctx.sync()
    return pipe, pts


def main():
    from dodt_amd import device
    shift, path = float(sys.argv[1]), sys.argv[2]
    ctx = device.default_context()
    pipe, _ = run_single_frame(ctx, shift)
    np.savez(path, records=pipe.d_records.download(), counts=pipe.d_rec_counts.download(),
             fused_tail=np.asarray(pipe.sched.fused_tail))
    pipe.close()


if __name__ == '__main__':
    main()
