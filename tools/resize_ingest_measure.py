"""Measure the resize on ingest on one MI355X -> profiles/resize_ingest.txt.

    python tools/resize_ingest_measure.py [--out profiles/resize_ingest.txt]

Two steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time of ocv_frame_resize_ingest at bs 16: 1080 x 1920 -> 480 x 640 and 720 x 1280 -> 480 x 640, each with and
                without the mirrored half, and whole KITTI frames 375 x 1242 -> 352 x 1216, beside (i) the traffic floor -- the window's
                bytes read once plus 12 B (24 B with the mirror) written per output pixel, over the copy bandwidth recorded in
                profiles/predict_path.txt (6281 GB/s) -- and (ii) the plain torch formulation of the same output on the same device in
                the same run (permute, float, interpolate(antialias=True), normalise, flip, cat: what a user writes without this
                feature).  (ii) is the bar: the launch must not be slower.
  (b) pipeline  images per second of PipelinedPredictor at bs 1, four slots: 1080p frames with resize=(480, 640) against native 480 x 640
                frames, same process, same model, alternating, three repeats each
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 300), ("pipeline", 600))          # name, time limit in seconds
COPY_GBS = 6281.0                                      # profiles/predict_path.txt (a), 16 frames with the mirrored half
CASES = (((1080, 1920), (480, 640)), ((720, 1280), (480, 640)), ((375, 1242), (352, 1216)))


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


def torch_resize(frames, size, mean, std, factor, mirror):
    """The same output with torch ops (fp32 on the device: torch decides the taps in fp32, so it is close to, not equal to, ours)."""
    import torch
    import torch.nn.functional as F
    x = frames.permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=size, mode="bilinear", antialias=True, align_corners=False)
    x = (x / factor - mean) / std
    return torch.cat([x, x.flip(3)], 0) if mirror else x


def step_kernel() -> None:
    import torch
    from objcavit_amd import hip_ops
    from objcavit_amd.config import make_args
    from objcavit_amd.predict import IMAGENET_MEAN, IMAGENET_STD, normalisation_table
    B = 16
    g = torch.Generator().manual_seed(3)
    table = normalisation_table(make_args()).cuda()
    mean = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1).cuda()
    std = torch.tensor(IMAGENET_STD).view(1, 3, 1, 1).cuda()
    print(f"(a) ocv_frame_resize_ingest, bs {B}; floor = (window bytes + 12 / 24 B per output pixel) / {COPY_GBS:.0f} GB/s; torch = permute, "
          "float, interpolate(antialias=True), normalise, flip, cat")
    print(f"    {'case':<44} {'us':>8} {'floor us':>9} {'GB/s':>7} {'x floor':>8} {'torch us':>9} {'torch / ours':>13} {'max |ours - torch|':>19}")
    for (Hs, Ws), (H, W) in CASES:
        frames = torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=g).cuda()
        for mirror in (False, True):
            out = torch.empty(2 * B if mirror else B, 3, H, W, device="cuda")
            call = lambda: hip_ops.frame_resize_ingest(frames, table, (H, W), mirror_too=mirror, out=out)      # noqa: E731
            call()
            ref = torch_resize(frames, (H, W), mean, std, 255.0, mirror)
            dev = float((out - ref).abs().max())
            assert dev < 5e-3, f"the torch formulation and the kernel disagree by {dev}"
            ms = _event_ms(call, 100)
            tms = _event_ms(lambda: torch_resize(frames, (H, W), mean, std, 255.0, mirror), 10)
            bytes_ = 3.0 * B * Hs * Ws + (24.0 if mirror else 12.0) * B * H * W
            floor = bytes_ / (COPY_GBS * 1e9) * 1e6
            name = f"{Hs}x{Ws} -> {H}x{W}{', + mirror' if mirror else ''}"
            print(f"    {name:<44} {ms * 1e3:8.1f} {floor:9.1f} {bytes_ / (ms * 1e-3) / 1e9:7.0f} {ms * 1e3 / floor:8.2f} {tms * 1e3:9.1f} "
                  f"{tms / ms:13.1f} {dev:19.2e}")
            if tms < ms:
                print(f"    ^^^ SLOWER than the torch formulation ({ms * 1e3:.1f} against {tms * 1e3:.1f} us): the bar is missed")


def step_pipeline() -> None:
    import torch
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    from objcavit_amd.predict import PipelinedPredictor
    torch.set_grad_enabled(False)
    H, W, N, POOL = 480, 640, 600, 8
    args = make_args(strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    model = GraphBins(args, object_provider=SyntheticObjectProvider(32, "clip", seed=42)).eval()
    gen.load_into(model, 42, gen.PEAKY)
    model = model.cuda()
    g = torch.Generator().manual_seed(1)
    native = [torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(POOL)]
    hd = [torch.randint(0, 256, (1, 1080, 1920, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(POOL)]
    plain = PipelinedPredictor(model, args, native[0], slots=4, want=("depth",))
    resized = PipelinedPredictor(model, args, hd[0], slots=4, want=("depth",), resize=(H, W))

    def run(pp, frames):
        for i in range(N):
            pp.submit(frames[i % POOL], first_image_id=i)
        return pp.collect()

    run(plain, native)
    res = run(resized, hd)                               # warm-up of both
    assert tuple(res[0].depth.shape) == (1, 1, 1080, 1920)
    rates = {f"native {H}x{W} frames": [], f"1080x1920 frames, resize=({H}, {W})": []}
    for _ in range(3):                                   # alternating repeats
        for name, (pp, frames) in zip(rates, ((plain, native), (resized, hd))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp, frames)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(b) PipelinedPredictor, bs 1, four slots, flip-TTA, model {H}x{W}, {N} steps per repeat, three alternating repeats, img/s "
          "(with resize the final map is written at 1080x1920: 8.3 MB per image instead of 1.2 MB)")
    for name, r in rates.items():
        print(f"    {name:<40} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    a, b = (sum(r) / 3 for r in rates.values())
    print(f"    native - resized = {a - b:.1f} img/s = {(1 / b - 1 / a) * 1e6:.1f} us per image; resized / native = {b / a:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_ingest.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            print("resize_ingest_measure: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        step_kernel() if a.step == "kernel" else step_pipeline()
        return 0
    text = ["resize on ingest on MI355X (tools/resize_ingest_measure.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"resize_ingest_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
