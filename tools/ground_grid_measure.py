"""Measure the ground grid on one MI355X -> profiles/ground_grid.txt.

    python tools/ground_grid_measure.py [--out profiles/ground_grid.txt]

Steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time of ocv_ground_grid_fwd's three launches together (clear, accumulate, finalize; replayed from a captured
                graph, so that the host's share of a call is not in the figure, and called eagerly beside it) at bs 16 and bs 1,
                480 x 640, the default grid (200 x 400 cells of 0.1 m), on a GROUND-like scene (flat ground seen from 1.65 m with a slab
                obstacle: neighbouring pixels of a row share a cell near the camera) and on the WALL scene (a fronto-parallel wall at
                4 m: every pixel column and runs of 13 pixels of a row fall into one cell) -- their ratio is the price of contention --,
                and on an image whose pose is not finite (the accumulate pass returns at once: what clear + finalize cost);
                beside them the plain torch formulation of the same outputs on the same device (``index_add_`` / ``scatter_reduce`` on the
                flattened cell index: what a user writes without this feature; its counts are checked against the kernel's first)
  (b) nomerge   the same launches from a diagnostic build whose accumulate pass has the on-chip merge compiled out, every kept point
                issuing its own set of global integer atomics (tools/build_variant.sh ground_grid_nomerge "-DOCV_GROUND_GRID_NO_MERGE"
                tools/diag/ground_grid_nomerge.patch; never shipped): the first figure here for integer atomics on this part
  (c) pipeline  PipelinedPredictor at bs 1 with four slots, ``ground_grid`` on against off, alternating repeats
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 300), ("nomerge", 200), ("pipeline", 400))              # name, time limit in seconds
VARIANT = os.path.join(ROOT, "objcavit_amd", "lib", "variants", "ground_grid_nomerge.so")
H, W = 480, 640
NEAR, FAR = 0.5, 80.0


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


def _graph_ms(fn, reps: int) -> float:
    """The launches of ``fn`` captured once and replayed: the device's time, without the host's share of a call (at bs 1 the three
    launches are shorter than the wrapper's argument checks)."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return _event_ms(graph.replay, reps)


def scenes(B: int):
    """{name: (depth [B, 1, H, W], K [B, 4], pose [B, 12])} on the device."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ground_grid_ref as ref
    from objcavit_amd.ground_grid import ground_pose
    from objcavit_amd.point_cloud import intrinsics_from_focal
    K = intrinsics_from_focal(518.8579, H, W)
    P = ref.pose_matrix(1.65, 0.07, -0.03)
    pose = ground_pose(1.65, 0.07, -0.03)
    ground = ref.ground_with_slab(H, W, K[0], P, forward=12.0, top=1.5)
    ground = torch.where(torch.isfinite(ground), ground, torch.full_like(ground, 1e4))
    wall = ref.wall(H, W, 4.0)
    out = {}
    for name, z, p in (("ground", ground, pose), ("wall", wall, pose), ("no pose", wall, pose * float("inf"))):
        out[name] = (z.view(1, 1, H, W).expand(B, 1, H, W).contiguous().cuda(), K.expand(B, 4).contiguous().cuda(),
                     p.expand(B, 12).contiguous().cuda())
    return out


def torch_grid(depth, K, pose, grid, band, obstacle_height, min_points, min_obstacle_points, near, far):
    """The same outputs with torch ops on the device (float atomics behind ``index_add_`` / ``scatter_reduce``)."""
    import torch
    x0, y0, cell, GX, GY = grid
    B = depth.shape[0]
    n = B * GX * GY
    z = depth[:, 0]
    fx, fy, cx, cy = (K[:, i].view(B, 1, 1) for i in range(4))
    p = pose.view(B, 3, 4, 1, 1)
    x = torch.arange(W, dtype=torch.float32, device=z.device).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float32, device=z.device).view(1, H, 1)
    X, Y = (x - cx) / fx * z, (y - cy) / fy * z
    g = [p[:, i, 0] * X + p[:, i, 1] * Y + p[:, i, 2] * z + p[:, i, 3] for i in range(3)]
    fxi, fyi = torch.floor((g[0] - x0) / cell), torch.floor((g[1] - y0) / cell)
    keep = torch.isfinite(z) & (z >= near) & (z <= far) & (fxi >= 0) & (fxi < GX) & (fyi >= 0) & (fyi < GY) & (g[2] >= band[0]) & (g[2] <= band[1])
    image = torch.arange(B, device=z.device).view(B, 1, 1) * (GX * GY)
    idx = (image + fyi.long() * GX + fxi.long())[keep]
    h = g[2][keep]
    count = torch.zeros(n, dtype=torch.int32, device=z.device).index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
    obstacle = torch.zeros(n, dtype=torch.int32, device=z.device).index_add_(0, idx, (h > obstacle_height).to(torch.int32))
    total = torch.zeros(n, dtype=torch.float32, device=z.device).index_add_(0, idx, h)
    h_min = torch.zeros(n, dtype=torch.float32, device=z.device).scatter_reduce_(0, idx, h, "amin", include_self=False)
    h_max = torch.zeros(n, dtype=torch.float32, device=z.device).scatter_reduce_(0, idx, h, "amax", include_self=False)
    h_mean = total / count.clamp_min(1)
    state = torch.where(count < min_points, 0, torch.where(obstacle >= min_obstacle_points, 2, 1)).to(torch.uint8).view(B, GY, GX)
    iy = torch.where(state == 2, torch.arange(GY, device=z.device).view(1, GY, 1), GY).amin(1)
    first = torch.where(iy < GY, y0 + iy.float() * cell, float("inf"))
    return count.view(B, GY, GX), obstacle.view(B, GY, GX), h_min.view(B, GY, GX), h_max.view(B, GY, GX), h_mean.view(B, GY, GX), state, first


def _launches(with_torch: bool) -> None:
    import torch
    from objcavit_amd import _lib, hip_ops
    from objcavit_amd.ground_grid import DEFAULTS, grid_of
    grid = grid_of()
    opts = dict(band=DEFAULTS["band"], obstacle_height=DEFAULTS["obstacle_height"], min_points=1, min_obstacle_points=3, near=NEAR, far=FAR)
    head = (f"    {'scene':<10} {'bs':>3} {'points':>9} {'cells':>7} {'us':>8} {'eager us':>9}" +
            (f" {'torch us':>9} {'torch / ours':>13}" if with_torch else ""))
    lib = _lib.load()
    print(head)
    for B in (16, 1):
        for name, (depth, K, pose) in scenes(B).items():
            dt = {"count": torch.int32, "obstacle": torch.int32, "state": torch.uint8}
            out = {n: torch.empty((B, grid[3]) if n == "first_occupied" else (B, grid[4], grid[3]), dtype=dt.get(n, torch.float32), device="cuda")
                   for n in hip_ops.GROUND_GRID_WANT}
            ws = torch.empty(int(lib.ocv_ground_grid_workspace_bytes(B, grid[3], grid[4])), dtype=torch.uint8, device="cuda")
            call = lambda: hip_ops.ground_grid(depth, K, pose, grid, out=out, workspace=ws, **opts)      # noqa: E731
            call()
            again = {n: t.clone() for n, t in out.items()}
            call()
            assert all(torch.equal(out[n].view(torch.uint8), again[n].view(torch.uint8)) for n in out), "two calls differ"
            points, cells = int(out["count"].sum()), int((out["count"] > 0).sum())
            ms, eager = _graph_ms(call, 100), _event_ms(call, 100)
            line = f"    {name:<10} {B:>3} {points:>9} {cells:>7} {ms * 1e3:8.1f} {eager * 1e3:9.1f}"
            if with_torch and name != "no pose":
                t = torch_grid(depth, K, pose, grid, opts["band"], opts["obstacle_height"], 1, 3, NEAR, FAR)
                differ = int((t[0] != out["count"]).sum())
                assert differ <= 1e-3 * max(cells, 1), ("the torch formulation and the kernel disagree", differ, cells)      # (torch fuses: a few border points)
                tms = _event_ms(lambda: torch_grid(depth, K, pose, grid, opts["band"], opts["obstacle_height"], 1, 3, NEAR, FAR), 10)
                line += f" {tms * 1e3:9.1f} {tms / ms:13.1f}"
            print(line)


def step_kernel() -> None:
    print(f"(a) ocv_ground_grid_fwd (clear + accumulate + finalize, every output), {H}x{W}, grid 200 x 400 cells of 0.1 m; us = the three "
          "launches replayed from a captured graph, eager = hip_ops.ground_grid called in a loop (host-bound at bs 1); torch = index_add_ / "
          "scatter_reduce on the flattened cell index, eager")
    _launches(True)


def step_nomerge() -> None:
    print("(b) the same from the diagnostic build WITHOUT the on-chip merge: every kept point issues its own global integer atomics")
    _launches(False)


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
    off = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",))
    on = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), ground_grid=dict(pitch=0.07, band=(-5.0, 5.0)))

    def run(pp, with_k):
        for i in range(N):
            pp.submit(frames[i % POOL], first_image_id=i, intrinsics=K if with_k else None)
        return pp.collect()

    run(off, False)
    res = run(on, True)                                  # warm-up of both
    assert res[0].ground is not None
    points = int(res[0].ground.count.sum())
    rates = {"ground_grid off": [], "ground_grid on (default grid, every output)": []}
    for _ in range(3):                                   # alternating repeats
        for name, (pp, wk) in zip(rates, ((off, False), (on, True))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp, wk)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(c) PipelinedPredictor, bs 1, four slots, flip-TTA, {H}x{W}, {N} steps per repeat, three alternating repeats, img/s "
          f"({points} points in the first frame's grid)")
    for name, r in rates.items():
        print(f"    {name:<46} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    a, b = (sum(r) / 3 for r in rates.values())
    print(f"    off - on = {a - b:.1f} img/s = {(1 / b - 1 / a) * 1e6:.1f} us per image; on / off = {b / a:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_grid.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            print("ground_grid_measure: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        {"kernel": step_kernel, "nomerge": step_nomerge, "pipeline": step_pipeline}[a.step]()
        return 0
    text = ["ground grid on MI355X (tools/ground_grid_measure.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        env = dict(os.environ)
        if name == "nomerge":
            if not os.path.exists(VARIANT):
                note = "(b) the diagnostic build without the on-chip merge is not there (tools/build_variant.sh, see this tool's text): not measured"
                print(note)
                text += [note, ""]
                continue
            env["OCV_LIB_PATH"] = VARIANT
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"ground_grid_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
