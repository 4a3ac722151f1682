"""Measure the ground plane on one MI355X -> profiles/ground_plane.txt.

    python tools/ground_plane_measure.py [--out profiles/ground_plane.txt]

Steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time of ocv_ground_plane_fwd's four launches together (hypotheses, consensus, moments, solve; replayed from a
                captured graph, so that the host's share of a call is not in the figure, and called eagerly beside it) at bs 16 and bs 1,
                480 x 640, T = 256, stride (1, 1) and (2, 2), on a GROUND-like scene (flat ground seen from 1.65 m with a slab obstacle:
                most hypotheses are valid) and on the WALL scene (a fronto-parallel wall at 4 m: the triples span vertical planes, few
                or no hypotheses are valid and the consensus loop skips them); beside them the same statement's consensus in plain torch on
                the same device -- the [T, 4] x [4, N] product, compare, sum a user would write -- whose counts are checked against the
                kernel's first
  (b) launches  the same call under ``rocprofv3 --kernel-trace --stats`` (this tool starts it; the program goes after ``--``): the
                average time of each of the four launches at bs 16
  (c) pipeline  PipelinedPredictor at bs 1 with four slots: no readout (what the parent commit runs), ``ground_grid`` alone, and
                ``ground_plane`` + ``ground_grid(pose="plane")`` twice -- with the default options, under which the synthetic model's maps
                (no road scene) hold no ground plane, so that most hypotheses are skipped and the moments launch returns at once: the
                CHEAP path; and with options so wide (triples from every row, 0.3 m + 10 %, any tilt below 1.5 rad) that the hypotheses
                are valid, every one is scored against every pixel and the moments are summed: the path a road scene takes, whether or
                not the refit then passes its checks --, alternating repeats.  What is printed beside the rates says which path ran
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 300), ("launches", 200), ("pipeline", 600))             # name, time limit in seconds
H, W, T = 480, 640, 256
NEAR, FAR = 0.5, 80.0
STRIDES = ((1, 1), (2, 2))

sys.path.insert(0, os.path.join(ROOT, "tools"))
from ground_grid_measure import _event_ms, _graph_ms, scenes  # noqa: E402


def torch_consensus(depth, K, hyp, stride, tol, rel_tol, near, far):
    """count [B, T] of the same statement with torch ops on the device: back-projection, one [T, 4] x [4, N] product per image, compare,
    sum.  ``hyp``: fp32 [B, T, 4] = n, h of the kernel's own hypotheses (NaN h: invalid), so that only the consensus is compared."""
    import torch
    B = depth.shape[0]
    z = depth[:, 0, ::stride[0], ::stride[1]]
    fx, fy, cx, cy = (K[:, i].view(B, 1, 1) for i in range(4))
    x = torch.arange(0, W, stride[1], dtype=torch.float32, device=z.device).view(1, 1, -1)
    y = torch.arange(0, H, stride[0], dtype=torch.float32, device=z.device).view(1, -1, 1)
    keep = (torch.isfinite(z) & (z >= near) & (z <= far)).reshape(B, 1, -1)
    P = torch.stack([((x - cx) / fx * z).reshape(B, -1), ((y - cy) / fy * z).reshape(B, -1), z.reshape(B, -1), torch.ones_like(z).reshape(B, -1)], 1)
    d = torch.bmm(torch.nan_to_num(hyp, nan=1e30), P)                                            # [B, T, N]
    thr = (tol + rel_tol * z).reshape(B, 1, -1)
    return ((d.abs() <= thr) & keep).sum(2, dtype=torch.int32)


def _setup(B, name, stride):
    import torch
    from objcavit_amd import _lib
    from objcavit_amd.ground_plane import plane_triples
    depth, K, pose = scenes(B)[name]
    triples = plane_triples(H, W, T).cuda()
    prior = pose.clone()
    prior[:, :] = torch.tensor([1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 1.5], dtype=torch.float32, device="cuda")      # a level camera 1.5 m up
    out = {"pose": torch.empty((B, 12), device="cuda"), "stats": torch.empty((B, 4), dtype=torch.int32, device="cuda")}
    ws = torch.empty(int(_lib.load().ocv_ground_plane_workspace_bytes(B, T)), dtype=torch.uint8, device="cuda")
    return depth, K, triples, prior, out, ws


def _call_of(B, name, stride):
    from objcavit_amd import hip_ops
    depth, K, triples, prior, out, ws = _setup(B, name, stride)
    call = lambda want=("pose", "stats"): hip_ops.ground_plane(depth, K, triples, prior, stride=stride, near=NEAR, far=FAR, out=out,      # noqa: E731
                                                               workspace=ws, want=want)
    return call, depth, K, out, ws


def step_kernel() -> None:
    import torch
    from objcavit_amd import hip_ops
    print(f"(a) ocv_ground_plane_fwd (hypotheses + consensus + moments + solve), {H}x{W}, T = {T} triples of the lower half; us = the four "
          "launches replayed from a captured graph, eager = hip_ops.ground_plane called in a loop (host-bound at bs 1); torch = "
          "back-projection, bmm([T, 4], [4, N]), compare, sum on the same device, eager, for the consensus alone")
    print(f"    {'scene':<8} {'bs':>3} {'stride':>7} {'valid':>6} {'best':>8} {'ok':>3} {'us':>8} {'eager us':>9} {'torch us':>9} {'torch / ours':>13}")
    for B in (16, 1):
        for name in ("ground", "wall"):
            for stride in STRIDES:
                call, depth, K, out, ws = _call_of(B, name, stride)
                got = call(("pose", "stats", "count"))
                count = got["count"].clone()
                stats = out["stats"].cpu()
                again = out["pose"].clone()
                call()
                assert torch.equal(out["pose"].view(torch.int32), again.view(torch.int32)), "two calls differ"
                hyp = hip_ops.ground_plane_workspace_views(ws, B, T)["hypotheses"][:, :T].clone()
                valid = int((hyp[0, :, 3] == hyp[0, :, 3]).sum())
                t = torch_consensus(depth, K, hyp, stride, 0.05, 0.01, NEAR, FAR)
                differ = int(((t - count).abs() > 0.01 * count + 8).sum())             # (torch's product rounds otherwise: border points)
                assert differ == 0, ("the torch formulation and the kernel disagree", differ)
                ms, eager = _graph_ms(call, 100), _event_ms(call, 100)
                tms = _event_ms(lambda: torch_consensus(depth, K, hyp, stride, 0.05, 0.01, NEAR, FAR), 10)
                print(f"    {name:<8} {B:>3} {str(stride):>7} {valid:>6} {int(stats[0, 1]):>8} {int(stats[0, 3]):>3} {ms * 1e3:8.1f} {eager * 1e3:9.1f} "
                      f"{tms * 1e3:9.1f} {tms / ms:13.1f}")


def step_traced() -> None:
    """What step (b) runs under the tracer: fifty calls per case at bs 16."""
    import torch
    for name in ("ground", "wall"):
        for stride in STRIDES:
            call = _call_of(16, name, stride)[0]
            for _ in range(50):
                call()
            torch.cuda.synchronize()


def step_launches() -> None:
    if shutil.which("rocprofv3") is None:
        print("(b) rocprofv3 is not on the path: the four launches are not timed one by one")
        return
    d = tempfile.mkdtemp(prefix="ground_plane_trace_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                            os.path.abspath(__file__), "--step", "traced"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:])
            raise SystemExit(r.returncode)
        files = glob.glob(os.path.join(d, "*", "*_kernel_stats.csv"))
        print(f"(b) the four launches one by one (rocprofv3 --kernel-trace --stats), bs 16, {H}x{W}, T = {T}, the ground and the wall scene at "
              "stride (1, 1) and (2, 2) mixed: 200 calls")
        print(f"    {'launch':<28} {'calls':>6} {'average us':>11} {'min us':>8} {'max us':>8}")
        for row in csv.DictReader(open(files[0])):
            if "plane_" in row["Name"]:
                short = row["Name"].split("plane_")[1].split("_kernel")[0]
                print(f"    {short:<28} {row['Calls']:>6} {float(row['AverageNs']) / 1e3:11.1f} {float(row['MinNs']) / 1e3:8.1f} {float(row['MaxNs']) / 1e3:8.1f}")
    finally:
        shutil.rmtree(d, ignore_errors=True)


def step_pipeline() -> None:
    import torch
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import PipelinedPredictor
    torch.set_grad_enabled(False)
    N, POOL = 600, 8
    args = make_args(strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    model = GraphBins(args, object_provider=SyntheticObjectProvider(32, "clip", seed=42)).eval()
    gen.load_into(model, 42, gen.PEAKY)
    model = model.cuda()
    g = torch.Generator().manual_seed(1)
    frames = [torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(POOL)]
    K = intrinsics_from_focal(518.8579, H, W).cuda()
    grid = dict(pitch=0.07, band=(-5.0, 5.0))
    wide = dict(rows=(0, H), tol=0.3, rel_tol=0.1, max_tilt=1.5, height_range=(-20.0, 20.0), min_inliers=32, height=1.2, pitch=0.3)
    posed = dict(grid, pose="plane")
    cases = {"no readout (the parent commit's path)": (PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",)), False),
             "ground_grid alone": (PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), ground_grid=grid), True),
             "plane (defaults) + grid": (PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), ground_plane={},
                                                                        ground_grid=posed), True),
             "plane (wide options) + grid": (PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), ground_plane=wide,
                                                                       ground_grid=posed), True)}

    def run(pp, with_k):
        for i in range(N):
            pp.submit(frames[i % POOL], first_image_id=i, intrinsics=K if with_k else None)
        return pp.collect()

    stats = {}
    for name, (pp, wk) in cases.items():                 # warm-up of all four
        res = run(pp, wk)
        if res[0].plane is not None:
            stats[name] = torch.cat([r.plane.stats for r in res[:POOL]], 0).cpu()
    assert len(stats) == 2 and res[0].ground is not None
    rates = {name: [] for name in cases}
    for _ in range(3):                                   # alternating repeats
        for name, (pp, wk) in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp, wk)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(c) PipelinedPredictor, bs 1, four slots, flip-TTA, {H}x{W}, {N} steps per repeat, three alternating repeats, img/s; the "
          f"synthetic model's maps are no road scene -- of the {POOL} frames, those with a best hypothesis / with an accepted refit, and "
          "the mean inlier count: " + "; ".join(f"{name}: {int((s[:, 0] >= 0).sum())} / {int(s[:, 3].sum())}, {float(s[:, 1].float().mean()):.0f}"
                                                for name, s in stats.items()))
    for name, r in rates.items():
        print(f"    {name:<42} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    base, grid_only, none_found, found = (sum(r) / 3 for r in rates.values())
    for what, v in (("defaults", none_found), ("wide options", found)):
        print(f"    {what}: the plane costs {(1 / v - 1 / grid_only) * 1e6:.1f} us per image on top of the grid; plane + grid / no readout = "
              f"{v / base:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_plane.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["traced"])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        sys.path.insert(0, ROOT)
        if a.step != "launches":
            import torch
            if not torch.cuda.is_available():
                print("ground_plane_measure: no GPU -- nothing is measured without one", file=sys.stderr)
                return 2
        {"kernel": step_kernel, "launches": step_launches, "traced": step_traced, "pipeline": step_pipeline}[a.step]()
        return 0
    text = ["ground plane on MI355X (tools/ground_plane_measure.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"ground_plane_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
