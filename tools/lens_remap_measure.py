"""Measure the lens on ingest on one MI355X -> profiles/lens_remap.txt.

    python tools/lens_remap_measure.py [--out profiles/lens_remap.txt]

Two steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time at bs 16, with the mirrored half, through a moderate barrel map (one map for the batch):
                  480 x 640 from 480 x 640, rgb24 and nv12: the fused launch ocv_frame_remap_ingest_fwd beside
                    plain   ocv_frame_ingest_fwd / ocv_frame_ingest_format at the same output size -- the floor: the writes are identical
                    torch   what a user writes without the feature: [YCbCr -> RGB in float,] float frames, grid_sample (bilinear, zeros
                            padding, align_corners) with the same coordinates, normalise, flip, cat -- THE BAR: the launch must beat it
                  1080 x 1920 nv12 through lens + resize to 480 x 640: ocv_frames_remap_rgb24_fwd + ocv_frame_resize_ingest (the two
                    launches ``lens`` + ``resize`` takes) beside the plain ocv_frame_resize_ingest_format
                and the bytes each fused launch must move: 8 B of map + the frame read once + 24 B written per output pixel.
  (b) pipeline  images per second of PipelinedPredictor at bs 1, four slots, 480 x 640 RGB frames, with and without ``lens=``, same
                process, same model, alternating, three repeats each
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 300), ("pipeline", 420))           # name, time limit in seconds
B = 16


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


def barrel(Hs: int, Ws: int):
    """A moderate barrel (k1 = -0.25): the rectified window keeps the camera and the size; its corners come from about 8 % further in."""
    from objcavit_amd.lens import LensMap
    f = 0.8 * Ws
    return LensMap.brown((f, f, (Ws - 1) / 2, (Hs - 1) / 2), (-0.25, 0.06, 0.0005, -0.0003), (Hs, Ws))


def step_kernel() -> None:
    import torch
    import torch.nn.functional as F
    from objcavit_amd import hip_ops
    from objcavit_amd.config import make_args
    from objcavit_amd.pixel_formats import PixelFormat, PlanarFrames
    from objcavit_amd.predict import IMAGENET_MEAN, IMAGENET_STD, normalisation_table
    torch.set_grad_enabled(False)
    table = normalisation_table(make_args()).cuda()
    g = torch.Generator().manual_seed(3)
    nv = PixelFormat("nv12")
    mean = torch.tensor(IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device="cuda").view(1, 3, 1, 1)
    print(f"(a) bs {B}, with the mirrored half, one barrel map for the batch; us per call (HIP events, fastest of three windows)")

    def grid_of(lm, Hs, Ws):
        m = lm.map[0].double() / 256.0
        return torch.stack([m[..., 0] * 2 / (Ws - 1) - 1, m[..., 1] * 2 / (Hs - 1) - 1], -1).float().cuda().unsqueeze(0).expand(B, -1, -1, -1)

    def torch_rgb(frames, grid):
        x = F.grid_sample(frames.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        x = (x / 255.0 - mean) / std
        return torch.cat([x, x.flip(3)], 0)

    yuv_m = torch.tensor([[1.164383, 0.0, 1.596027], [1.164383, -0.391762, -0.812968], [1.164383, 2.017232, 0.0]], device="cuda")

    def torch_nv12(frames, grid):
        y, c = frames.planes
        c = c.repeat_interleave(2, 1).repeat_interleave(2, 2).float() - 128.0
        ycc = torch.cat([(y.float() - 16.0).unsqueeze(-1), c], -1)
        rgb = (ycc @ yuv_m.t()).round().clamp(0, 255)
        x = F.grid_sample(rgb.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        x = (x / 255.0 - mean) / std
        return torch.cat([x, x.flip(3)], 0)

    Hs, Ws = 480, 640
    lm = barrel(Hs, Ws)
    grid = grid_of(lm, Hs, Ws)
    rgb = torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=g).cuda()
    planar = PlanarFrames.from_buffer(torch.randint(0, 256, (B, Hs * 3 // 2, Ws), dtype=torch.uint8, generator=g).cuda(), "nv12", Hs, Ws)
    out = torch.empty((2 * B, 3, Hs, Ws), device="cuda")
    print(f"    map: {int(lm.valid.sum())} of {lm.valid.numel()} pixels have all four taps inside the frame")
    for name, frames, fmt, plain, tfn, src in (
            ("rgb24", rgb, None, lambda: hip_ops.frame_ingest(rgb, table, mirror_too=True, out=out), torch_rgb, 3.0),
            ("nv12", planar, nv, lambda: hip_ops.frame_ingest_format(planar, table, nv, mirror_too=True, out=out), torch_nv12, 1.5)):
        fused = _event_ms(lambda: hip_ops.frame_remap_ingest(frames, table, lm, fmt, mirror_too=True, out=out), 200) * 1e3
        floor = _event_ms(plain, 200) * 1e3
        tt = _event_ms(lambda: tfn(frames, grid), 20) * 1e3
        # the fused launch's result is what the torch formulation approximates (float weights against 8-bit ones): within 1.5 / 255 / std
        got = hip_ops.frame_remap_ingest(frames, table, lm, fmt, mirror_too=True)
        diff = float((got - tfn(frames, grid)).abs().max())
        mb = B * Hs * Ws * (8.0 / B + src + 24.0) / 1e6
        print(f"    {Hs}x{Ws} {name:<5}  fused lens launch {fused:8.1f}   plain ingest (floor) {floor:8.1f}   ratio {fused / floor:5.2f}   "
              f"torch grid_sample formulation {tt:9.1f}   torch / fused {tt / fused:6.1f}x   "
              f"bytes {mb:.1f} MB -> {mb / fused * 1e3:.0f} GB/s   max |fused - torch| {diff:.4f}")
    Hs, Ws, size = 1080, 1920, (480, 640)
    lm = barrel(Hs, Ws)
    planar = PlanarFrames.from_buffer(torch.randint(0, 256, (B, Hs * 3 // 2, Ws), dtype=torch.uint8, generator=g).cuda(), "nv12", Hs, Ws)
    rect = torch.empty((B, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
    taps = hip_ops.frame_resize_taps("cuda", Hs, Ws, *size)

    def two():
        hip_ops.frames_remap_rgb24(planar, lm, nv, out=rect)
        hip_ops.frame_resize_ingest(rect, table, size, mirror_too=True, out=out, taps=taps)

    first = _event_ms(lambda: hip_ops.frames_remap_rgb24(planar, lm, nv, out=rect), 50) * 1e3
    both = _event_ms(two, 50) * 1e3
    plain = _event_ms(lambda: hip_ops.frame_resize_ingest_format(planar, table, size, nv, mirror_too=True, out=out, taps=taps), 50) * 1e3
    print(f"    {Hs}x{Ws} nv12 -> lens + resize -> {size[0]}x{size[1]}:  rgb24 lens launch {first:8.1f}   both launches {both:8.1f}   "
          f"plain resize ingest {plain:8.1f}   ratio {both / plain:5.2f}")


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
    rgb = [torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(POOL)]
    p_plain = PipelinedPredictor(model, args, rgb[0], slots=4, want=("depth",))
    p_lens = PipelinedPredictor(model, args, rgb[0], slots=4, want=("depth",), lens=barrel(H, W))

    def run(pp):
        for i in range(N):
            pp.submit(rgb[i % POOL], first_image_id=i)
        return pp.collect()

    run(p_plain)
    run(p_lens)                                          # warm-up of both
    rates = {"without lens=": [], "with lens= (barrel)": []}
    for _ in range(3):                                   # alternating repeats
        for name, pp in zip(rates, (p_plain, p_lens)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(b) PipelinedPredictor, bs 1, four slots, flip-TTA, {H}x{W} RGB frames on the device, {N} steps per repeat, three alternating "
          "repeats, img/s")
    for name, r in rates.items():
        print(f"    {name:<22} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    a, b = (sum(r) / 3 for r in rates.values())
    print(f"    without - with = {a - b:.1f} img/s = {(1 / b - 1 / a) * 1e6:.1f} us per image; with / without = {b / a:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_remap.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            print("lens_remap_measure: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        step_kernel() if a.step == "kernel" else step_pipeline()
        return 0
    text = ["lens on ingest on MI355X (tools/lens_remap_measure.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"lens_remap_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
