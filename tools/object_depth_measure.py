"""Measure the per-object depth readout on one MI355X -> profiles/object_depth.txt.

    python tools/object_depth_measure.py [--out profiles/object_depth.txt]

Two steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time of ocv_object_depth_fwd at the bench shape (bs 16, 480 x 640, 32 boxes per image drawn as
                SyntheticObjectProvider draws them, default quantiles), beside the finalize launch timed in the same run and the
                design's traffic floor: 4 reads of the boxes' pixels (+ 1 of depth_std when given) / the copy bandwidth recorded in
                profiles/predict_path.txt (6281 GB/s: ingest of 16 frames with the mirrored half); then one whole-frame box per image
                (the imbalance case: one workgroup per box), bs 1 with 16 boxes (the pipeline's step), and an all-equal map
  (b) pipeline  images per second of PipelinedPredictor at bs 1, four slots, 16 boxes per frame: ``object_depth`` on against off,
                same process, same model, alternating, three repeats each; the allowed gap is the larger of the off runs' spread and
                the kernel's standalone time per step, which the parent hands on from (a) as --kernel-us
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 300), ("pipeline", 600))          # name, time limit in seconds
COPY_GBS = 6281.0                                      # profiles/predict_path.txt (a), 16 frames with the mirrored half


def _event_ms(fn, reps: int) -> float:
    import torch
    for _ in range(10):
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


def step_kernel() -> None:
    import torch
    from objcavit_amd import hip_ops
    H, W = 480, 640
    g = torch.Generator().manual_seed(3)
    print("(a) ocv_object_depth_fwd, 480x640, default quantiles (0.1, 0.5, 0.9); floor = passes x 4 B x pixels covered / 6281 GB/s")
    print(f"    {'case':<44} {'rows':>5} {'Mpixel':>7} {'largest':>8} {'us':>8} {'floor us':>9} {'finalize us':>12}")
    per_step = None
    for name, B, n, whole, with_std, smooth in (("bs 16, 32 provider boxes", 16, 32, False, False, True),
                                                ("bs 16, 32 provider boxes, + depth_std", 16, 32, False, True, True),
                                                ("bs 16, 32 provider boxes, noise map", 16, 32, False, False, False),
                                                ("bs 16, one whole-frame box per image", 16, 1, True, False, True),
                                                ("bs 1, one whole-frame box", 1, 1, True, False, True),
                                                ("bs 1, 16 provider boxes (pipeline step)", 1, 16, False, False, True),
                                                ("bs 1, 16 provider boxes, + depth_std", 1, 16, False, True, True)):
        pred = torch.rand(B, 1, H // 2, W // 2, generator=g).cuda() * 9.0 + 0.5
        if smooth:                                       # a depth-like map: a ramp + small noise (neighbours share their upper bits)
            pred = (torch.linspace(0.5, 9.5, W // 2).view(1, 1, 1, -1) + torch.linspace(0.0, 0.4, H // 2).view(1, 1, -1, 1)).cuda() + 0.01 * pred
            pred = pred.expand(B, 1, H // 2, W // 2).contiguous()
        mirror = pred.flip(3).contiguous()
        depth = hip_ops.depth_finalize(pred, 0.001, 10.0, (H, W), pred_mirror=mirror)["depth"]
        std = torch.rand(B, 1, H, W, generator=g).cuda() if with_std else None
        boxes = torch.tensor([W / 2.0, H / 2.0, float(W), float(H)]).expand(B, 1, 4).contiguous() if whole else provider_boxes(B, n, H, W)
        # pixels covered, by the kernel's own record (column 0)
        xywh, counts = boxes.cuda(), torch.full((B,), n, dtype=torch.int32, device="cuda")
        out = hip_ops.object_depth(depth, xywh, counts, depth_std=std)
        pixels, largest = float(out[..., 0].sum()), float(out[..., 0].max())
        ms = _event_ms(lambda: hip_ops.object_depth(depth, xywh, counts, depth_std=std, out=out), 100)
        fin = _event_ms(lambda: hip_ops.depth_finalize(pred, 0.001, 10.0, (H, W), pred_mirror=mirror, out={"depth": depth}), 100)
        floor = (5 if with_std else 4) * 4.0 * pixels / (COPY_GBS * 1e9) * 1e6
        print(f"    {name:<44} {B * n:>5} {pixels / 1e6:>7.2f} {int(largest):>8} {ms * 1e3:8.1f} {floor:9.1f} {fin * 1e3:12.1f}")
        if name.startswith("bs 1, 16 provider boxes (pipeline"):
            per_step = ms * 1e3
    print(f"    standalone time per pipeline step (bs 1, 16 boxes): {per_step:.1f} us")


def step_pipeline(kernel_us: float) -> None:
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
    boxes = [(provider_boxes(1, NBOX, H, W, seed=i).cuda(), torch.full((1,), NBOX, dtype=torch.int32, device="cuda")) for i in range(POOL)]
    off = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",))
    on = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), object_depth={})

    def run(pp, with_boxes):
        for i in range(N):
            pp.submit(frames[i % POOL], first_image_id=i, boxes=boxes[i % POOL] if with_boxes else None)
        return pp.collect()

    run(off, False)
    res = run(on, True)                                  # warm-up of both
    assert res[0].objects is not None and float(res[0].objects.table[0, :, 0].sum()) > 0
    rates = {"object_depth off": [], "object_depth on, 16 boxes per frame": []}
    for _ in range(3):                                   # alternating repeats
        for name, (pp, wb) in zip(rates, ((off, False), (on, True))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp, wb)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(b) PipelinedPredictor, bs 1, four slots, flip-TTA, {H}x{W}, {N} steps per repeat, three alternating repeats, img/s")
    for name, r in rates.items():
        print(f"    {name:<40} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    a, b = (sum(r) / 3 for r in rates.values())
    base = rates["object_depth off"]
    spread = max(base) - min(base)
    # the kernel's standalone time per step as a rate gap at the off runs' rate: 1 / (1 / a + t) against a
    kernel_gap = a - 1.0 / (1.0 / a + kernel_us * 1e-6) if kernel_us == kernel_us else float("nan")
    allowed = max(spread, kernel_gap) if kernel_gap == kernel_gap else spread
    print(f"    allowed gap: max(off runs' spread {spread:.1f} img/s, kernel's standalone {kernel_us:.1f} us per step = {kernel_gap:.1f} img/s at "
          f"the off rate) = {allowed:.1f} img/s")
    print(f"    measured gap: off - on = {a - b:.1f} img/s = {(1 / b - 1 / a) * 1e6:.1f} us per image; on / off = {b / a:.4f}; "
          f"{'within' if a - b <= allowed else 'OUTSIDE'} the allowed gap")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_depth.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--kernel-us", type=float, default=float("nan"), help="(b): the kernel's standalone time per step from (a)")
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            print("object_depth_measure: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        step_kernel() if a.step == "kernel" else step_pipeline(a.kernel_us)
        return 0
    text = ["per-object depth readout on MI355X (tools/object_depth_measure.py); event-timed launches after warm-up, fastest of three windows", ""]
    extra = []
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"object_depth_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
        m = re.search(r"standalone time per pipeline step.*?: ([0-9.]+) us", r.stdout)
        if m:
            extra = ["--kernel-us", m.group(1)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
