"""Measure the pixel formats on ingest on one MI355X -> profiles/pixel_formats.txt.

    python tools/pixel_formats_measure.py [--out profiles/pixel_formats.txt]

Two steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time at bs 16 of the fused launch of every format -- ocv_frame_ingest_format at 480 x 640 native and
                ocv_frame_resize_ingest_format at 1080 x 1920 -> 480 x 640, each without and with the mirrored half -- beside
                  rgb24   the rgb24 launch of the same shape on RGB frames (recorded, not gated: what the conversion costs)
                  2-step  ocv_frames_to_rgb24 + the rgb24 launch (THE BAR: the fused launch must not lose to it)
                  torch   the plain torch formulation a user writes without this feature (nv12 / i420: plane views,
                          repeat_interleave, float matrix, round, clamp; packed: channel gather + contiguous; then permute, float,
                          [interpolate(antialias=True),] normalise, flip, cat)
                and the traffic floor: the window's source bytes read once + 12 B (24 B with the mirror) per output pixel over the copy
                bandwidth recorded in profiles/predict_path.txt (6281 GB/s).  Fused and 2-step alternate three times; a format LOSES
                when every fused run is slower than every 2-step run and the means differ by more than twice the run-to-run spread.
  (b) pipeline  images per second of PipelinedPredictor at bs 1, four slots: 1080p NV12 frames with resize=(480, 640) against 1080p RGB
                frames with the same resize, same process, same model, alternating, three repeats each
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 420), ("pipeline", 420))           # name, time limit in seconds
COPY_GBS = 6281.0                                      # profiles/predict_path.txt (a), 16 frames with the mirrored half
FORMATS = ("bgr24", "rgba32", "bgra32", "nv12", "i420")
SHAPES = (((480, 640), None), ((1080, 1920), (480, 640)))          # (frame size, model size or None = native)


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


def source_bytes(name: str, Hs: int, Ws: int) -> float:
    """Bytes of one frame of a format."""
    if name in ("nv12", "i420"):
        return Hs * Ws + 2.0 * ((Hs + 1) // 2) * ((Ws + 1) // 2)
    return Hs * Ws * (4.0 if name.endswith("32") else 3.0)


def make_frames(name: str, rgb):
    """Frames of a format that show (about) the picture of uint8 RGB frames [B, Hs, Ws, 3] on the device (even Hs, Ws)."""
    import torch
    from objcavit_amd.pixel_formats import PlanarFrames
    B, Hs, Ws, _ = rgb.shape
    if name == "rgb24":
        return rgb
    if name == "bgr24":
        return rgb.flip(3).contiguous()
    if name in ("rgba32", "bgra32"):
        x = rgb if name == "rgba32" else rgb.flip(3)
        return torch.cat([x, torch.full((B, Hs, Ws, 1), 255, dtype=torch.uint8, device=rgb.device)], 3).contiguous()
    buf = torch.randint(0, 256, (B, Hs * 3 // 2, Ws), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(rgb.device)
    return PlanarFrames.from_buffer(buf, name, Hs, Ws)


def torch_to_rgb(name: str, frames, fmt):
    """The plain torch formulation of frames -> float RGB [B, Hs, Ws, 3] with byte values."""
    import torch
    if name == "bgr24":
        return frames[..., [2, 1, 0]].contiguous()
    if name == "rgba32":
        return frames[..., :3].contiguous()
    if name == "bgra32":
        return frames[..., [2, 1, 0]].contiguous()
    Hs, Ws = frames.Hs, frames.Ws
    y = frames.planes[0].float()
    if name == "nv12":
        cb, cr = frames.planes[1][..., 0].float(), frames.planes[1][..., 1].float()
    else:
        cb, cr = frames.planes[1].float(), frames.planes[2].float()
    cb = cb.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :Hs, :Ws]
    cr = cr.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :Hs, :Ws]
    kr, kb = (0.299, 0.114) if fmt.matrix == "bt601" else (0.2126, 0.0722)
    kg = 1.0 - kr - kb
    y0, sy, sc = (16.0, 255.0 / 219.0, 255.0 / 224.0) if fmt.range == "limited" else (0.0, 1.0, 1.0)
    l = sy * (y - y0)
    cb, cr = sc * (cb - 128.0), sc * (cr - 128.0)
    rgb = torch.stack([l + 2 * (1 - kr) * cr, l - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr, l + 2 * (1 - kb) * cb], 3)
    return (rgb + 0.5).floor().clamp_(0, 255)


def torch_ingest(rgb, size, mean, std, mirror):
    import torch
    import torch.nn.functional as F
    x = rgb.permute(0, 3, 1, 2).float()
    if size is not None:
        x = F.interpolate(x, size=size, mode="bilinear", antialias=True, align_corners=False)
    x = (x / 255.0 - mean) / std
    return torch.cat([x, x.flip(3)], 0) if mirror else x


def step_kernel() -> None:
    import torch
    from objcavit_amd import hip_ops
    from objcavit_amd.config import make_args
    from objcavit_amd.pixel_formats import PixelFormat
    from objcavit_amd.predict import IMAGENET_MEAN, IMAGENET_STD, normalisation_table
    B = 16
    g = torch.Generator().manual_seed(3)
    table = normalisation_table(make_args()).cuda()
    mean = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1).cuda()
    std = torch.tensor(IMAGENET_STD).view(1, 3, 1, 1).cuda()
    print(f"(a) fused launch per format, bs {B}, us; rgb24 = the rgb24 launch of the same shape; 2-step = ocv_frames_to_rgb24 + the rgb24 launch "
          f"(the bar); torch = the plain torch formulation; floor = (source bytes + 12 / 24 B per output pixel) / {COPY_GBS:.0f} GB/s; fused and "
          "2-step: three alternating runs each, fastest of three windows per run")
    print(f"    {'case':<52} {'fused (3 runs)':>22} {'2-step (3 runs)':>22} {'rgb24':>7} {'torch':>8} {'floor':>6} {'x floor':>8} {'fused/rgb24':>12} "
          f"{'2-step/fused':>13} {'torch/fused':>12}  verdict")
    lost = {}
    for (Hs, Ws), size in SHAPES:
        H, W = size or (Hs, Ws)
        rgb = torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=g).cuda()
        for name in FORMATS:
            fmt = PixelFormat(name, "bt709", "limited")
            frames = make_frames(name, rgb)
            for mirror in (False, True):
                out = torch.empty(2 * B if mirror else B, 3, H, W, device="cuda")
                out2 = torch.empty_like(out)
                tmp = torch.empty(B, Hs, Ws, 3, dtype=torch.uint8, device="cuda")
                if size is None:
                    fused = lambda: hip_ops.frame_ingest_format(frames, table, fmt, mirror_too=mirror, out=out)            # noqa: E731
                    plain = lambda src=rgb, o=out2: hip_ops.frame_ingest(src, table, mirror_too=mirror, out=o)              # noqa: E731
                else:
                    fused = lambda: hip_ops.frame_resize_ingest_format(frames, table, size, fmt, mirror_too=mirror, out=out)  # noqa: E731
                    plain = lambda src=rgb, o=out2: hip_ops.frame_resize_ingest(src, table, size, mirror_too=mirror, out=o)   # noqa: E731

                def two_step():
                    hip_ops.frames_to_rgb24(frames, fmt, out=tmp)
                    return plain(tmp, out2)

                def torch_form():
                    return torch_ingest(torch_to_rgb(name, frames, fmt), size, mean, std, mirror)

                fused()
                two_step()
                assert torch.equal(out, out2), f"{name}: the fused launch and frames_to_rgb24 + the rgb24 launch disagree"
                dev = float((out - torch_form()).abs().max())
                assert dev < 0.05, f"{name}: the torch formulation and the kernel disagree by {dev}"
                f_ms, t_ms = [], []
                for _ in range(3):                      # alternating
                    f_ms.append(_event_ms(fused, 100))
                    t_ms.append(_event_ms(two_step, 100))
                p_ms = _event_ms(plain, 100)
                o_ms = _event_ms(torch_form, 10)
                bytes_ = B * source_bytes(name, Hs, Ws) + (24.0 if mirror else 12.0) * B * H * W
                floor = bytes_ / (COPY_GBS * 1e9) * 1e6
                fm, tm = sum(f_ms) / 3, sum(t_ms) / 3
                spread = max(max(f_ms) - min(f_ms), max(t_ms) - min(t_ms))
                loses = min(f_ms) > max(t_ms) and fm - tm > 2 * spread
                if loses:
                    lost.setdefault(name, []).append((Hs, Ws, H, W, mirror, fm * 1e3, tm * 1e3))
                case = f"{name} {Hs}x{Ws}{'' if size is None else f' -> {H}x{W}'}{', + mirror' if mirror else ''}"
                print(f"    {case:<52} {' '.join(f'{v * 1e3:6.1f}' for v in f_ms):>22} {' '.join(f'{v * 1e3:6.1f}' for v in t_ms):>22} "
                      f"{p_ms * 1e3:7.1f} {o_ms * 1e3:8.1f} {floor:6.1f} {fm * 1e3 / floor:8.2f} {fm / p_ms:12.2f} {tm / fm:13.2f} {o_ms / fm:12.1f}  "
                      f"{'LOSES to the 2-step' if loses else 'fused holds'}")
    print("    routing decision per format (a format that loses in any case goes through ocv_frames_to_rgb24 + the rgb24 launch):")
    for name in FORMATS:
        if name in lost:
            print(f"      {name}: LOSES -> 2-step; " + "; ".join(f"{a}x{b} -> {c}x{d}{' + mirror' if m else ''}: {x:.1f} against {y:.1f} us"
                                                                  for a, b, c, d, m, x, y in lost[name]))
        else:
            print(f"      {name}: fused launch")


def step_pipeline() -> None:
    import torch
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    from objcavit_amd.pixel_formats import PlanarFrames
    from objcavit_amd.predict import PipelinedPredictor
    torch.set_grad_enabled(False)
    H, W, N, POOL = 480, 640, 600, 8
    args = make_args(strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    model = GraphBins(args, object_provider=SyntheticObjectProvider(32, "clip", seed=42)).eval()
    gen.load_into(model, 42, gen.PEAKY)
    model = model.cuda()
    g = torch.Generator().manual_seed(1)
    rgb = [torch.randint(0, 256, (1, 1080, 1920, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(POOL)]
    nv = [PlanarFrames.from_buffer(torch.randint(0, 256, (1, 1620, 1920), dtype=torch.uint8, generator=g).cuda(), "nv12", 1080, 1920)
          for _ in range(POOL)]
    p_rgb = PipelinedPredictor(model, args, rgb[0], slots=4, want=("depth",), resize=(H, W))
    p_nv = PipelinedPredictor(model, args, nv[0], slots=4, want=("depth",), resize=(H, W), pixel_format="nv12")

    def run(pp, frames):
        for i in range(N):
            pp.submit(frames[i % POOL], first_image_id=i)
        return pp.collect()

    run(p_rgb, rgb)
    res = run(p_nv, nv)                                  # warm-up of both
    assert tuple(res[0].depth.shape) == (1, 1, 1080, 1920)
    rates = {f"1080x1920 RGB frames, resize=({H}, {W})": [], f"1080x1920 NV12 frames, resize=({H}, {W})": []}
    for _ in range(3):                                   # alternating repeats
        for name, (pp, frames) in zip(rates, ((p_rgb, rgb), (p_nv, nv))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp, frames)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(b) PipelinedPredictor, bs 1, four slots, flip-TTA, model {H}x{W}, {N} steps per repeat, three alternating repeats, img/s "
          "(frames already on the device: 6.2 MB per RGB frame, 3.1 MB per NV12 frame)")
    for name, r in rates.items():
        print(f"    {name:<44} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    a, b = (sum(r) / 3 for r in rates.values())
    print(f"    RGB - NV12 = {a - b:.1f} img/s = {(1 / b - 1 / a) * 1e6:.1f} us per image; NV12 / RGB = {b / a:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_formats.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            print("pixel_formats_measure: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        step_kernel() if a.step == "kernel" else step_pipeline()
        return 0
    text = ["pixel formats on ingest on MI355X (tools/pixel_formats_measure.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"pixel_formats_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
