"""What the validation loss costs: ocv_depth_metrics_fwd (metrics only) against ocv_depth_metrics_loss_fwd (metrics + loss pieces,
one pass over the ground truth) per call, alternating, three repeats each, at bs 1 / 2 / 16 NYU (240x320 -> 480x640) and bs 2 KITTI
(176x608 -> 352x1216) on smooth scenes (tests/loss_ref.py: the realistic case for the interval atomics -- neighbouring pixels fall
into the same interval between bin centres); then PipelinedValidation at bs 1 (four slots) with loss off / on, alternating.

    python tools/time_val_loss.py [--calls-only | --kernels]       (--kernels: a few calls per shape, for rocprofv3 --kernel-trace --stats)
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")

import loss_ref as lr                     # noqa: E402
from objcavit_amd import hip_ops          # noqa: E402

SHAPES = [("nyu bs 1", 1, (240, 320), (480, 640), 10.0, 1.0), ("nyu bs 2", 2, (240, 320), (480, 640), 10.0, 1.0),
          ("nyu bs 16", 16, (240, 320), (480, 640), 10.0, 1.0), ("kitti bs 2", 2, (176, 608), (352, 1216), 80.0, 0.05)]
REPEATS, CALLS = 3, 300


def inputs(B, hw, HW, dmax, sparse):
    gt = lr.scene(B, HW[0], HW[1], dmax, sparse, 5).cuda()
    pred = (torch.rand(B, 1, *hw) * 1.0 * dmax + 0.2).cuda()
    mirror = (torch.rand(B, 1, *hw) * 1.0 * dmax + 0.2).cuda()
    return pred, mirror, gt, lr.clustered_edges(B, 256, 0.001, dmax, 9).cuda()


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3          # us per call


def calls(kernels_only=False):
    for name, B, hw, HW, dmax, sparse in SHAPES:
        pred, mirror, gt, edges = inputs(B, hw, HW, dmax, sparse)
        metrics = lambda: hip_ops.depth_metrics(pred, gt, 0.001, dmax, pred_mirror=mirror)                       # noqa: E731
        fused = lambda: hip_ops.depth_metrics_loss(pred, gt, edges, 0.001, dmax, pred_mirror=mirror)             # noqa: E731
        for _ in range(5):
            r0, (r1, l1) = metrics(), fused()
        assert torch.equal(r0, r1)
        if kernels_only:
            for _ in range(20):
                metrics(), fused()
            torch.cuda.synchronize()
            continue
        t = {"metrics": [], "metrics+loss": []}
        for _ in range(REPEATS):
            t["metrics"].append(timed(metrics, CALLS))
            t["metrics+loss"].append(timed(fused, CALLS))
        a, b = sorted(t["metrics"]), sorted(t["metrics+loss"])
        print(f"{name:11s} depth_metrics {a[1]:7.1f} us ({a[0]:.1f} .. {a[2]:.1f})   depth_metrics_loss {b[1]:7.1f} us ({b[0]:.1f} .. {b[2]:.1f})"
              f"   + {b[1] - a[1]:.1f} us per call, {(b[1] - a[1]) / B:.1f} us per image", flush=True)


def pipeline():
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    from objcavit_amd.validation import PipelinedValidation
    H, W, N = 480, 640, 400
    args = make_args(language="clip")
    m = GraphBins(args, object_provider=SyntheticObjectProvider(32, "clip", seed=9)).eval()
    gen.load_into(m, 31, gen.PEAKY)
    m = m.cuda()
    imgs = [gen.randn(f"im{i}", (1, 3, H, W), 300 + i).cuda() for i in range(8)]
    gts = [lr.scene(1, H, W, 10.0, 1.0, i).cuda() for i in range(8)]
    pv = PipelinedValidation(m, args, imgs[0])

    def run(loss):
        pv.loss = loss
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(N):
            pv.submit(imgs[i % 8], gts[i % 8], first_image_id=i)
        rec = pv.collect()
        dt = time.perf_counter() - t0
        assert rec.shape == (N, 16 if loss else 10)
        return dt / N * 1e6                            # us per validated image

    run(False), run(True)
    t = {False: [], True: []}
    for _ in range(REPEATS):
        for loss in (False, True):
            t[loss].append(run(loss))
    a, b = sorted(t[False]), sorted(t[True])
    print(f"PipelinedValidation bs 1, 4 slots, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}, {N} steps: loss off {a[1]:.1f} us / image ({a[0]:.1f} .. {a[2]:.1f}; {1e6 / a[1]:.0f} img/s)   "
          f"loss on {b[1]:.1f} us / image ({b[0]:.1f} .. {b[2]:.1f}; {1e6 / b[1]:.0f} img/s)   + {b[1] - a[1]:.1f} us; spread of the "
          f"loss-off repeats {a[2] - a[0]:.1f} us", flush=True)


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    if "--kernels" in sys.argv:
        calls(kernels_only=True)
    else:
        calls()
        if "--calls-only" not in sys.argv:
            pipeline()
