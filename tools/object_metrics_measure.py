"""Measure the per-object / per-region depth error on one MI355X -> profiles/object_metrics.txt.

    python tools/object_metrics_measure.py [--out profiles/object_metrics.txt]

Two steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time of ocv_object_metrics_fwd at bs 16, 480 x 640 (prediction 240 x 320 with mirror, NYU range and Eigen
                crop): 32 boxes per image drawn as SyntheticObjectProvider draws them, and one whole-frame box per image (the
                imbalance case: one workgroup per box) -- the boxes alone and with the region pass --, beside the ``depth_metrics``
                launch timed in the same run and the plain torch formulation of the same tables on the device (resize, masks and
                masked means per box in a Python loop: what a user writes without this entry point); then bs 1 with 16 boxes (the
                pipeline's step)
  (b) pipeline  images per second of PipelinedPredictor at bs 1, four slots, with ground truth and 16 boxes per frame:
                ``object_metrics`` on against off, same process, same model, alternating, three repeats each
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 300), ("pipeline", 600))          # name, time limit in seconds
DMIN, DMAX, CROP = 1e-3, 10.0, (45, 471, 41, 601)


def _event_ms(fn, reps: int) -> float:
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):                                  # three windows, the fastest: other people's work shares the host
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def provider_boxes(B: int, n: int, H: int, W: int, seed: int = 42):
    """[B, n, 4] as SyntheticObjectProvider draws them: centres uniform in the image, sizes uniform in [8, W / 2] x [8, H / 2]."""
    import numpy as np
    import torch
    rs = np.random.RandomState(seed)
    boxes = np.stack([rs.uniform(0, W, (B, n)), rs.uniform(0, H, (B, n)), rs.uniform(8, W / 2, (B, n)), rs.uniform(8, H / 2, (B, n))], axis=-1)
    return torch.from_numpy(boxes.astype(np.float32))


def box_range(box, H: int, W: int):
    """(x0, x1, y0, y1) of a finite box on an H x W map by the centre rule (fp32 statements, shrink 1), or None."""
    import torch
    half = torch.tensor(0.5)
    lo = torch.ceil((box[:2] - half * box[2:4]) - 0.5).clamp(min=0.0)
    hi = torch.minimum(torch.ceil((box[:2] + half * box[2:4]) - 0.5).clamp(min=0.0), torch.tensor([float(W), float(H)]))
    lo = torch.minimum(lo, torch.tensor([float(W), float(H)]))
    x0, y0, x1, y1 = int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1])
    return (x0, x1, y0, y1) if x1 > x0 and y1 > y0 else None


def torch_tables(pred, mirror, gt, ranges):
    """The same tables in plain torch on the device: the validation step's statements, then masked means per box and per region.
    ``ranges``: per image a list of (x0, x1, y0, y1) pixel ranges, worked out on the host beforehand (not timed)."""
    import torch
    import torch.nn.functional as F
    p = 0.5 * (pred.clamp(DMIN, DMAX) + mirror.flip(3).clamp(DMIN, DMAX))
    p = F.interpolate(p, gt.shape[-2:], mode="bilinear", align_corners=True).nan_to_num(nan=DMIN, posinf=DMAX, neginf=DMAX)
    mask = (gt > DMIN) & (gt <= DMAX)
    ev = torch.zeros_like(mask)
    ev[:, :, CROP[0]:CROP[1], CROP[2]:CROP[3]] = True
    mask &= ev
    d = gt - p
    ratio = torch.maximum(gt / p, p / gt)
    terms = torch.stack([d.abs() / gt, d * d / gt, d * d, (gt.log() - p.log()) ** 2, (gt.log10() - p.log10()).abs(),
                         (ratio < 1.25).float(), (ratio < 1.25 ** 2).float(), (ratio < 1.25 ** 3).float(), torch.ones_like(gt), gt], 0)
    terms = torch.where(mask[:, 0], terms[:, :, 0], torch.zeros((), device=gt.device))      # [10, B, H, W], zero outside the mask
    B = gt.shape[0]
    rows, regions = [], []
    for b in range(B):
        union = torch.zeros_like(mask[b, 0])
        for x0, x1, y0, y1 in ranges[b]:
            rows.append(terms[:, b, y0:y1, x0:x1].double().sum((1, 2)))
            union[y0:y1, x0:x1] = True
        regions.append((terms[:, b] * union).double().sum((1, 2)))
        regions.append((terms[:, b] * ~union).double().sum((1, 2)))
    out = []
    for s in (torch.stack(rows), torch.stack(regions)):
        n = s[:, 8:9].clamp(min=1.0)
        r = s / n
        r[:, 2:4] = r[:, 2:4].sqrt()
        r[:, 8] = s[:, 8]
        out.append(r.float())
    return out


def step_kernel() -> None:
    import torch
    from objcavit_amd import hip_ops
    H, W = 480, 640
    g = torch.Generator().manual_seed(3)
    print("(a) ocv_object_metrics_fwd, gt 480x640, pred 240x320 + mirror, NYU range, Eigen crop; us per call")
    print(f"    {'case':<40} {'rows':>5} {'Mpixel':>7} {'boxes us':>9} {'+regions us':>12} {'depth_metrics us':>17} {'torch us':>10}")
    for name, B, n, whole in (("bs 16, 32 provider boxes", 16, 32, False), ("bs 16, one whole-frame box per image", 16, 1, True),
                              ("bs 1, 16 provider boxes (pipeline step)", 1, 16, False)):
        gt = (torch.rand(B, 1, H, W, generator=g) * 10.5 + 0.2).cuda()
        pred = (torch.rand(B, 1, H // 2, W // 2, generator=g) * 9.0 + 0.5).cuda()
        mirror = pred.flip(3).contiguous()
        boxes = torch.tensor([W / 2.0, H / 2.0, float(W), float(H)]).expand(B, 1, 4).contiguous() if whole else provider_boxes(B, n, H, W)
        xywh, counts = boxes.cuda(), torch.full((B,), n, dtype=torch.int32, device="cuda")
        table, _ = hip_ops.object_metrics(pred, gt, xywh, counts, DMIN, DMAX, crop=CROP, pred_mirror=mirror)
        pixels = float(table[..., 8].sum())
        alone = _event_ms(lambda: hip_ops.object_metrics(pred, gt, xywh, counts, DMIN, DMAX, crop=CROP, pred_mirror=mirror, regions=False, out=table), 50)
        both = _event_ms(lambda: hip_ops.object_metrics(pred, gt, xywh, counts, DMIN, DMAX, crop=CROP, pred_mirror=mirror, out=table), 50)
        image = _event_ms(lambda: hip_ops.depth_metrics(pred, gt, DMIN, DMAX, crop=CROP, pred_mirror=mirror), 50)
        ranges = [[px for px in (box_range(boxes[b, r], H, W) for r in range(n)) if px is not None] for b in range(B)]
        plain = _event_ms(lambda: torch_tables(pred, mirror, gt, ranges), 3)
        print(f"    {name:<40} {B * n:>5} {pixels / 1e6:>7.2f} {alone * 1e3:9.1f} {both * 1e3:12.1f} {image * 1e3:17.1f} {plain * 1e3:10.1f}")


def step_pipeline() -> None:
    import torch
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    from objcavit_amd.predict import PipelinedPredictor
    torch.set_grad_enabled(False)
    H, W, N, POOL, NBOX = 480, 640, 600, 8, 16
    args = make_args(strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    model = GraphBins(args, object_provider=SyntheticObjectProvider(32, "clip", seed=42)).eval()
    gen.load_into(model, 42, gen.PEAKY)
    model = model.cuda()
    g = torch.Generator().manual_seed(1)
    frames = [torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(POOL)]
    gts = [(torch.rand(1, 1, H, W, generator=g) * 10.5 + 0.2).cuda() for _ in range(POOL)]
    boxes = [(provider_boxes(1, NBOX, H, W, seed=i).cuda(), torch.full((1,), NBOX, dtype=torch.int32, device="cuda")) for i in range(POOL)]
    off = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",))
    on = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), object_metrics={})

    def run(pp):
        for i in range(N):
            pp.submit(frames[i % POOL], gts[i % POOL], first_image_id=i, boxes=boxes[i % POOL])
        return pp.collect()

    assert run(off)[0].object_metrics is None
    res = run(on)                                        # warm-up of both
    assert float(res[0].object_metrics.table[0, :, 8].sum()) > 0
    rates = {"object_metrics off": [], "object_metrics on, 16 boxes per frame": []}
    for _ in range(3):                                   # alternating repeats
        for name, pp in zip(rates, (off, on)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(b) PipelinedPredictor with ground truth, bs 1, four slots, flip-TTA, {H}x{W}, {N} steps per repeat, three alternating repeats, img/s")
    for name, r in rates.items():
        print(f"    {name:<40} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    a, b = (sum(r) / 3 for r in rates.values())
    print(f"    off - on = {a - b:.1f} img/s = {(1 / b - 1 / a) * 1e6:.1f} us per image; on / off = {b / a:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_metrics.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            print("object_metrics_measure: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        step_kernel() if a.step == "kernel" else step_pipeline()
        return 0
    text = ["per-object / per-region depth error on MI355X (tools/object_metrics_measure.py); event-timed calls after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"object_metrics_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
