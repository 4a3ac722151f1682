"""Measure the obstacle list on one MI355X -> profiles/obstacles.txt.

    python tools/measure_obstacles.py [--out profiles/obstacles.txt]

Steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time of ocv_obstacles_fwd's launches together (every output, the label map included; replayed from a captured
                graph, and called eagerly beside it) at bs 16, 480 x 640 into the default grid (200 x 400 cells of 0.1 m), link 1 and 3,
                on the grids of tools/ground_grid_measure.py's GROUND-like scene and WALL (made by ocv_ground_grid_fwd itself) and on a
                full-grid SERPENTINE one cell wide: one component that winds through every tile, the worst case for the seam pass.
                Beside it what a user does today: ``state.cpu()`` (the copy and the synchronisation included), then per image
                ``scipy.ndimage.label`` with a 3 x 3 structure and ``find_objects`` -- at link 3 as well, since ``label`` takes no wider
                structure (its components then differ from ours; its cost does not) -- or, where scipy does not import, the flood fill of
                tests/obstacles_ref.py; the text says which.  At link 1 scipy's number of components is checked against ``total``.
  (b) merge     the same calls with the statistics pass's on-chip merge switched off (ocv_obstacles_set_dispatch: every occupied cell
                issues its own global integer atomics at its root): the difference of the two columns is the statistics pass's
  (c) pipeline  PipelinedPredictor at bs 1 with four slots, ``ground_grid`` + ``obstacles`` against ``ground_grid`` alone, alternating
                repeats
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
STEPS = (("kernel", 400), ("pipeline", 400))             # name, time limit in seconds
B, CAP = 16, 64


def _grids():
    """{scene: (state, count, obstacle, h_max) [B, GY, GX] on the device} and the grid's spec."""
    import torch
    import ground_grid_measure as gm
    import obstacles_ref as ref
    from objcavit_amd import hip_ops
    from objcavit_amd.ground_grid import DEFAULTS, grid_of
    spec = grid_of()
    out = {}
    names = ("state", "count", "obstacle", "h_max")
    for scene, (depth, K, pose) in gm.scenes(B).items():
        if scene == "no pose":
            continue
        g = hip_ops.ground_grid(depth, K, pose, spec, band=DEFAULTS["band"], obstacle_height=DEFAULTS["obstacle_height"], min_points=1,
                                min_obstacle_points=3, near=gm.NEAR, far=gm.FAR, want=names)
        out[scene] = tuple(g[n] for n in names)
    occ = ref.pattern("serpentine", spec[3], spec[4])[None].repeat(B, 0)
    out["serpentine"] = tuple(torch.from_numpy(a).cuda() for a in ref.grid_inputs(occ, seed=1))
    return out, spec


def _host_ms(state, reps: int = 3):
    """(ms, components of image 0, what ran): the copy to the host, then label + find_objects per image."""
    import numpy as np
    import torch
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    import obstacles_ref as ref
    best, n0 = float("inf"), 0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = state.cpu().numpy()                        # the copy and the synchronisation
        for b in range(host.shape[0]):
            if ndimage is not None:
                lab, n = ndimage.label(host[b] == 2, structure=np.ones((3, 3), dtype=bool))
                ndimage.find_objects(lab)
            else:
                n = len(np.unique(ref.roots_of(host[b] == 2, 1))) - 1
            n0 = n if b == 0 else n0
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, n0, "scipy" if ndimage is not None else "flood fill"


def step_kernel() -> None:
    import torch
    import ground_grid_measure as gm
    from objcavit_amd import _lib, hip_ops
    grids, spec = _grids()
    lib = _lib.load()
    ws = torch.empty(int(lib.ocv_obstacles_workspace_bytes(B, spec[3], spec[4])), dtype=torch.uint8, device="cuda")
    out = {"cells": torch.empty((B, CAP, 8), dtype=torch.int32, device="cuda"), "metres": torch.empty((B, CAP, 8), device="cuda"),
           "counts": torch.empty((B,), dtype=torch.int32, device="cuda"), "total": torch.empty((B,), dtype=torch.int32, device="cuda"),
           "labels": torch.empty((B, spec[4], spec[3]), dtype=torch.int32, device="cuda")}
    rows = []
    for link in (1, 3):
        for scene, (state, count, obstacle, h_max) in grids.items():
            call = lambda: hip_ops.obstacles(state, spec, count=count, obstacle=obstacle, h_max=h_max, link=link, capacity=CAP, out=out,    # noqa: E731
                                             workspace=ws)
            call()
            first = {n: t.clone() for n, t in out.items()}
            us, eager = gm._graph_ms(call, 50) * 1e3, gm._event_ms(call, 50) * 1e3
            occupied, total = int((state[0] == 2).sum()), int(out["total"][0])
            hip_ops.obstacles_set_dispatch(False)
            try:
                call()
                assert all(torch.equal(out[n].view(torch.int32), first[n].view(torch.int32)) for n in out), "the merge changes the bytes"
                plain = gm._graph_ms(call, 50) * 1e3
            finally:
                hip_ops.obstacles_set_dispatch(True)
            host, n0, what = _host_ms(state)
            assert link != 1 or what != "scipy" or n0 == total, ("scipy and the kernel disagree", n0, total)
            rows.append((scene, link, occupied, total, us, eager, plain, host * 1e3, what))
    print(f"(a) ocv_obstacles_fwd (every output, labels included: seven launches), bs {B}, grid {spec[3]} x {spec[4]} cells, capacity {CAP}; us = "
          "the launches replayed from a captured graph, eager = hip_ops.obstacles called in a loop; host = state.cpu() + per image "
          f"{rows[0][8]} label (3 x 3 structure) + find_objects, the copy and the synchronisation included, fastest of three; occupied / kept: "
          "cells and obstacles of image 0")
    print(f"    {'scene':<11} {'link':>4} {'occupied':>9} {'kept':>6} {'us':>8} {'eager us':>9} {'host us':>10} {'host / ours':>12}")
    for scene, link, occupied, total, us, eager, plain, host, what in rows:
        print(f"    {scene:<11} {link:>4} {occupied:>9} {total:>6} {us:8.1f} {eager:9.1f} {host:10.1f} {host / us:12.1f}")
    print()
    print("(b) the same calls without the statistics pass's on-chip merge (every occupied cell sends its own global atomics to its root); "
          "the bytes are the same")
    print(f"    {'scene':<11} {'link':>4} {'merged us':>10} {'unmerged us':>12} {'difference':>11}")
    for scene, link, occupied, total, us, eager, plain, host, what in rows:
        print(f"    {scene:<11} {link:>4} {us:10.1f} {plain:12.1f} {plain - us:11.1f}")


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
    ground = dict(pitch=0.07, band=(-5.0, 5.0))
    grid = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), ground_grid=ground)
    both = PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), ground_grid=ground, obstacles={})

    def run(pp):
        for i in range(N):
            pp.submit(frames[i % POOL], first_image_id=i, intrinsics=K)
        return pp.collect()

    run(grid)
    res = run(both)                                      # warm-up of both
    assert res[0].obstacles is not None
    kept, occupied = int(res[0].obstacles.total[0]), int((res[0].ground.state == 2).sum())
    rates = {"ground_grid alone": [], "ground_grid + obstacles (defaults)": []}
    for _ in range(3):                                   # alternating repeats
        for name, pp in zip(rates, (grid, both)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(c) PipelinedPredictor, bs 1, four slots, flip-TTA, {H}x{W}, {N} steps per repeat, three alternating repeats, img/s "
          f"({occupied} occupied cells, {kept} obstacles kept in the first frame's grid)")
    for name, r in rates.items():
        print(f"    {name:<46} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    a, b = (sum(r) / 3 for r in rates.values())
    print(f"    alone - with = {a - b:.1f} img/s = {(1 / b - 1 / a) * 1e6:.1f} us per image; with / alone = {b / a:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacles.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        import torch
        if not torch.cuda.is_available():
            print("measure_obstacles: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        {"kernel": step_kernel, "pipeline": step_pipeline}[a.step]()
        return 0
    text = ["obstacle list on MI355X (tools/measure_obstacles.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=dict(os.environ))
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"measure_obstacles: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
