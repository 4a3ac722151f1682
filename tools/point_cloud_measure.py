"""Measure the point-cloud output on one MI355X -> profiles/point_cloud.txt.

    python tools/point_cloud_measure.py [--out profiles/point_cloud.txt]

Two steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time of the launch pair of ocv_depth_unproject_fwd at the bench shape (bs 16, 480 x 640), stride 1 and (2, 2),
                all pixels kept and about half of them, with and without colour + confidence, beside the finalize launch timed in the
                same run, the design's traffic floor -- the map (and the confidence) read twice, 3 B of the frame read and 16 B (20 B with
                the pixel index) written per kept point, over the copy bandwidth recorded in profiles/predict_path.txt (6281 GB/s) -- and
                the plain torch formulation of the same output on the same device (mask, nonzero, gathers, arithmetic, stack: what a
                user writes without this feature; its count is read on the host)
  (b) pipeline  images per second of PipelinedPredictor at bs 1, four slots: ``point_cloud`` on against off, same process, same model,
                alternating, three repeats each
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


def torch_cloud(depth, K, stride, near, far, conf, min_conf, frames):
    """The same output with torch ops: (xyz [n, 3], rgb [n, 3] or None, alpha [n] or None, counts [B]) in the kernel's order."""
    import torch
    sy, sx = stride
    B, _, H, W = depth.shape
    z = depth[:, 0, ::sy, ::sx]
    m = torch.isfinite(z) & (z >= near) & (z <= far)
    c = None if conf is None else conf[:, 0, ::sy, ::sx]
    if c is not None:
        m = m & (c >= min_conf)
    b, yc, xc = m.nonzero(as_tuple=True)                # (the host reads the count here)
    y, x = yc * sy, xc * sx
    zz = z[b, yc, xc]
    xyz = torch.stack([(x.float() - K[b, 2]) / K[b, 0] * zz, (y.float() - K[b, 3]) / K[b, 1] * zz, zz], 1)
    rgb = None if frames is None else frames[b, y, x]
    alpha = None if c is None else torch.round(255.0 * c[b, yc, xc].clamp(0.0, 1.0)).to(torch.uint8)
    return xyz, rgb, alpha, m.flatten(1).sum(1)


def step_kernel() -> None:
    import torch
    from objcavit_amd import hip_ops
    H, W, B = 480, 640, 16
    g = torch.Generator().manual_seed(3)
    near, far = 0.5, 10.0
    pred = (torch.rand(B, 1, H // 2, W // 2, generator=g) * 9.0 + 0.75).cuda()
    mirror = pred.flip(3).contiguous()
    depth_all = hip_ops.depth_finalize(pred, 0.001, 10.0, (H, W), pred_mirror=mirror)["depth"]
    depth_half = torch.where(torch.rand(B, 1, H, W, generator=g).cuda() < 0.5, depth_all, torch.full_like(depth_all, 20.0))
    conf = torch.rand(B, 1, H, W, generator=g).cuda() * 0.5 + 0.5
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    K = torch.tensor([[518.8579, 518.8579, 319.5, 239.5]]).expand(B, 4).contiguous().cuda()
    fin = _event_ms(lambda: hip_ops.depth_finalize(pred, 0.001, 10.0, (H, W), pred_mirror=mirror, out={"depth": depth_all}), 100)
    print(f"(a) ocv_depth_unproject_fwd (count + write), bs {B}, {H}x{W}; floor = bytes / {COPY_GBS:.0f} GB/s; the finalize launch: {fin * 1e3:.1f} us")
    print(f"    {'case':<52} {'Mpoints':>8} {'us':>8} {'floor us':>9} {'GB/s':>7} {'torch us':>9} {'torch / ours':>13}")
    for stride in ((1, 1), (2, 2)):
        gh, gw = hip_ops.unproject_grid(H, W, stride)
        cap = gh * gw
        for kept, depth in (("all kept", depth_all), ("half kept", depth_half)):
            for extras in (False, True):
                cf, fr = (conf, frames) if extras else (None, None)
                out = {"points": torch.empty(B, cap, 4, device="cuda"), "counts": torch.empty(B, dtype=torch.int32, device="cuda"),
                       "total": torch.empty(B, dtype=torch.int32, device="cuda")}
                call = lambda: hip_ops.depth_unproject(depth, K, cap, stride=stride, near=near, far=far, confidence=cf,      # noqa: E731
                                                       min_confidence=0.25, frames=fr, out=out)
                call()
                n = int(out["total"].sum())
                xyz, rgb, alpha, counts = torch_cloud(depth, K, stride, near, far, cf, 0.25, fr)
                assert torch.equal(counts.to(torch.int32), out["counts"]) and xyz.shape[0] == n
                ours = torch.cat([out["points"][i, :int(c), :3] for i, c in enumerate(out["counts"].tolist())], 0)
                assert torch.allclose(ours, xyz, rtol=1e-5, atol=0), "the torch formulation and the kernel disagree"
                ms = _event_ms(call, 100)
                tms = _event_ms(lambda: torch_cloud(depth, K, stride, near, far, cf, 0.25, fr), 20)
                bytes_ = 2 * 4.0 * B * cap * (2 if extras else 1) + n * (16.0 + (3.0 if extras else 0.0))
                floor = bytes_ / (COPY_GBS * 1e9) * 1e6
                name = f"stride {stride}, {kept}{', + colour + confidence' if extras else ''}"
                print(f"    {name:<52} {n / 1e6:>8.2f} {ms * 1e3:8.1f} {floor:9.1f} {bytes_ / (ms * 1e-3) / 1e9:7.0f} {tms * 1e3:9.1f} {tms / ms:13.1f}")


def step_pipeline() -> None:
    import torch
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import PipelinedPredictor
    torch.set_grad_enabled(False)
    H, W, N, POOL = 480, 640, 600, 8
    args = make_args(strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    model = GraphBins(args, object_provider=SyntheticObjectProvider(32, "clip", seed=42)).eval()
    gen.load_into(model, 42, gen.PEAKY)
    model = model.cuda()
    g = torch.Generator().manual_seed(1)
    frames = [torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(POOL)]
    K = intrinsics_from_focal(518.8579, H, W).cuda()
    off = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",))
    on = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), point_cloud={})

    def run(pp, with_k):
        for i in range(N):
            pp.submit(frames[i % POOL], first_image_id=i, intrinsics=K if with_k else None)
        return pp.collect()

    run(off, False)
    res = run(on, True)                                  # warm-up of both
    assert res[0].points is not None
    kept = int(res[0].points.total[0])
    rates = {"point_cloud off": [], "point_cloud on (stride 1, colour)": []}
    for _ in range(3):                                   # alternating repeats
        for name, (pp, wk) in zip(rates, ((off, False), (on, True))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp, wk)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(b) PipelinedPredictor, bs 1, four slots, flip-TTA, {H}x{W}, {N} steps per repeat, three alternating repeats, img/s "
          f"({kept} of {H * W} pixels kept in the first frame)")
    for name, r in rates.items():
        print(f"    {name:<40} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    a, b = (sum(r) / 3 for r in rates.values())
    print(f"    off - on = {a - b:.1f} img/s = {(1 / b - 1 / a) * 1e6:.1f} us per image; on / off = {b / a:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_cloud.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            print("point_cloud_measure: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        step_kernel() if a.step == "kernel" else step_pipeline()
        return 0
    text = ["point-cloud output on MI355X (tools/point_cloud_measure.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"point_cloud_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
