"""Measure the surface normals on one MI355X -> profiles/normals.txt.

    python tools/normals_measure.py [--out profiles/normals.txt]

Two steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) angle     the largest angle between the kernel's normal and the fp64 statement (tests/normals_ref.py) over the maps of
                tests/test_hip_normals.py -- every shape of normals_ref.CASE_SHAPES and VECTOR_SHAPES, every radius, every choice of the bad camera --
                with the largest | |n| - 1 | and the largest byte difference of the picture: the figure the test's bar is 8 x of
  (b) kernel    HIP-event time of ocv_depth_normals_fwd at the bench shape (bs 16, 480 x 640, r = 2; also r = 1, 3, 4) with and without
                the picture and the mask, of ocv_normals_gather_fwd behind a stride-(2, 2) cloud, the traffic floor -- 4 B read and
                12 B (+ 3 B picture, + 1 B mask) written per pixel over the copy bandwidth recorded in profiles/predict_path.txt
                (6281 GB/s) -- and the plain torch formulation of the same output on the same device (conv2d with the ramp and box
                kernels, max_pool2d for the extremes, elementwise ops: what a user writes without this feature)
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("angle", 300), ("kernel", 300))              # name, time limit in seconds
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


def torch_normals(depth, K, r, near, far, edge):
    """The same outputs with torch ops on the device: (normals [B, 3, H, W], valid bool [B, H, W])."""
    import torch
    import torch.nn.functional as F
    B, _, H, W = depth.shape
    k = 2 * r + 1
    D = k * 2 * sum(i * i for i in range(1, r + 1))
    ramp = torch.arange(-r, r + 1, dtype=torch.float32, device=depth.device)
    wu = (ramp.view(1, k).expand(k, k) / D).reshape(1, 1, k, k).contiguous()
    wv = (ramp.view(k, 1).expand(k, k) / D).reshape(1, 1, k, k).contiguous()
    fin = torch.isfinite(depth)
    z = torch.where(fin, depth, torch.zeros_like(depth))
    zu, zv = F.conv2d(z, wu, padding=r), F.conv2d(z, wv, padding=r)
    hi = F.max_pool2d(torch.where(fin, depth, torch.full_like(depth, float("inf"))), k, stride=1, padding=r)
    lo = -F.max_pool2d(torch.where(fin, -depth, torch.full_like(depth, float("inf"))), k, stride=1, padding=r)
    t = edge * z
    valid = (lo >= near) & (hi <= far) & (hi - z <= t) & (z - lo <= t)
    valid[:, :, :r] = False
    valid[:, :, H - r:] = False
    valid[:, :, :, :r] = False
    valid[:, :, :, W - r:] = False
    x = torch.arange(W, dtype=torch.float32, device=depth.device).view(1, 1, 1, W)
    y = torch.arange(H, dtype=torch.float32, device=depth.device).view(1, 1, H, 1)
    fx, fy, cx, cy = (K[:, i].view(B, 1, 1, 1) for i in range(4))
    m = torch.cat([fx * zu, fy * zv, -(z + (x - cx) * zu + (y - cy) * zv)], 1)
    n = m * torch.rsqrt((m * m).sum(1, keepdim=True))
    return torch.where(valid, n, torch.zeros_like(n)), valid[:, 0]


def step_angle() -> None:
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import normals_ref as ref
    from objcavit_amd import hip_ops
    worst = {"angle": 0.0, "length": 0.0, "byte": 0}
    print("(a) largest deviation from the fp64 statement (tests/normals_ref.py) over the maps of tests/test_hip_normals.py")
    print(f"    {'map':<10} {'r':>2} {'valid':>7} {'max angle rad':>14} {'max ||n|-1|':>12} {'max byte diff':>14}")
    for H, W in ref.CASE_SHAPES + ref.VECTOR_SHAPES:
        for r in ref.RADII:
            row = {"angle": 0.0, "length": 0.0, "byte": 0}
            nvalid = 0
            for bad in (None, 0, 1, 2):
                depth, K = ref.case(H, W, bad_camera=bad)
                want = ref.normals(depth, K, r)
                got = hip_ops.depth_normals(depth.cuda(), K.cuda(), radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE,
                                            want=("normals", "rgb8", "valid"))
                n, v = got["normals"].cpu().double(), got["valid"].cpu().bool()
                assert torch.equal(v, want.valid), (H, W, r, bad, "validity differs")
                if not bool(v.any()):
                    continue
                nvalid += int(v.sum())
                row["angle"] = max(row["angle"], float(ref.angle(n, want.normals)[v].max()))
                row["length"] = max(row["length"], float((n.norm(dim=1) - 1).abs()[v].max()))
                row["byte"] = max(row["byte"], int((got["rgb8"].cpu().int() - want.rgb8.int()).abs().max()))
            print(f"    {f'{H}x{W}':<10} {r:>2} {nvalid:>7} {row['angle']:14.3e} {row['length']:12.3e} {row['byte']:>14}")
            worst = {k: max(worst[k], row[k]) for k in worst}
    print(f"    largest angle {worst['angle']:.3e} rad (x 8 = {8 * worst['angle']:.3e}), largest ||n| - 1| {worst['length']:.3e}, "
          f"largest byte difference {worst['byte']}")


def step_kernel() -> None:
    import torch
    from objcavit_amd import hip_ops
    H, W, B = 480, 640, 16
    g = torch.Generator().manual_seed(3)
    near, far, edge = 0.5, 10.0, 0.05
    pred = (2.5 * (1.0 + 0.02 * torch.randn(B, 1, H // 2, W // 2, generator=g))).cuda()
    depth = hip_ops.depth_finalize(pred, 0.001, 10.0, (H, W))["depth"]
    K = torch.tensor([[518.8579, 518.8579, 319.5, 239.5]]).expand(B, 4).contiguous().cuda()
    px = float(B * H * W)
    print(f"(b) ocv_depth_normals_fwd, bs {B}, {H}x{W}; floor = bytes / {COPY_GBS:.0f} GB/s (4 B read + 12 B normals + 3 B picture + 1 B mask "
          "per pixel)")
    print(f"    {'case':<40} {'valid':>6} {'us':>8} {'floor us':>9} {'GB/s':>7} {'of copy':>8} {'torch us':>9} {'torch / ours':>13}")
    for r, want in ((2, ("normals",)), (2, ("normals", "rgb8")), (2, ("normals", "rgb8", "valid")), (1, ("normals",)), (3, ("normals",)),
                    (4, ("normals",)), (4, ("normals", "rgb8", "valid"))):
        shapes = {"normals": ((B, 3, H, W), torch.float32), "rgb8": ((B, H, W, 3), torch.uint8), "valid": ((B, H, W), torch.uint8)}
        out = {n: torch.empty(shapes[n][0], dtype=shapes[n][1], device="cuda") for n in want}
        call = lambda: hip_ops.depth_normals(depth, K, radius=r, near=near, far=far, edge_ratio=edge, want=want, out=out)      # noqa: E731
        call()
        tn, tv = torch_normals(depth, K, r, near, far, edge)
        mask = hip_ops.depth_normals(depth, K, radius=r, near=near, far=far, edge_ratio=edge, want=("valid",))["valid"].bool()
        agree = float((mask == tv).float().mean())
        both = mask & tv
        dev = float((out["normals"] - tn).abs().amax(1)[both].max())
        assert agree > 0.999 and dev < 5e-3, ("the torch formulation and the kernel disagree", agree, dev)
        ms = _event_ms(call, 100)
        tms = _event_ms(lambda: torch_normals(depth, K, r, near, far, edge), 20)
        bytes_ = px * (4.0 + 12.0 + (3.0 if "rgb8" in want else 0.0) + (1.0 if "valid" in want else 0.0))
        floor = bytes_ / (COPY_GBS * 1e9) * 1e6
        gbs = bytes_ / (ms * 1e-3) / 1e9
        name = f"r = {r}, " + " + ".join(want)
        print(f"    {name:<40} {float(mask.float().mean()):6.2f} {ms * 1e3:8.1f} {floor:9.1f} {gbs:7.0f} {gbs / COPY_GBS:8.2f} {tms * 1e3:9.1f} "
              f"{tms / ms:13.1f}")
    # the gather behind a stride-(2, 2) cloud
    normals = hip_ops.depth_normals(depth, K, radius=2, near=near, far=far, edge_ratio=edge)["normals"]
    gh, gw = hip_ops.unproject_grid(H, W, (2, 2))
    cap = gh * gw
    cloud = hip_ops.depth_unproject(depth, K, cap, stride=(2, 2), near=near, far=far, want_pixel=True)
    out = torch.empty(B, cap, 4, device="cuda")
    call = lambda: hip_ops.normals_gather(normals, cloud["pixel"], cloud["counts"], out=out)      # noqa: E731
    call()
    n = int(cloud["counts"].sum())

    def torch_gather():
        flat = normals.flatten(2)
        idx = cloud["pixel"].long().clamp(0, H * W - 1).unsqueeze(1).expand(B, 3, cap)
        return torch.cat([flat.gather(2, idx).permute(0, 2, 1), torch.zeros(B, cap, 1, device="cuda")], 2)

    tg = torch_gather()
    assert torch.equal(tg[0, :int(cloud["counts"][0])], out[0, :int(cloud["counts"][0])])
    ms = _event_ms(call, 100)
    tms = _event_ms(torch_gather, 20)
    bytes_ = n * (4.0 + 12.0 + 16.0)                     # the index, three gathered floats, one record
    print(f"    ocv_normals_gather_fwd, stride (2, 2): {n / 1e6:.2f} Mpoints, {ms * 1e3:.1f} us, floor {bytes_ / (COPY_GBS * 1e9) * 1e6:.1f} us, "
          f"{bytes_ / (ms * 1e-3) / 1e9:.0f} GB/s; torch (gather + cat) {tms * 1e3:.1f} us = {tms / ms:.1f} x")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            print("normals_measure: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        step_angle() if a.step == "angle" else step_kernel()
        return 0
    text = ["surface normals on MI355X (tools/normals_measure.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"normals_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
