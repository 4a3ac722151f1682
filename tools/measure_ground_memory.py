"""Measure the ground memory on one MI355X -> profiles/ground_memory.txt.

    python tools/measure_ground_memory.py [--out profiles/ground_memory.txt]

Steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) kernel    HIP-event time of ocv_ground_fuse_fwd's one launch (every output; replayed from a captured graph, and called eagerly
                beside it) at bs 16 and bs 1 on the default grid (200 x 400 cells of 0.1 m), for the identity and for a quarter turn with a
                6 m shift (the gather then walks the previous map column by column).  Beside it what a user would otherwise run -- the
                same statement with torch ops on the device: ``affine_grid`` / ``grid_sample(mode="nearest")`` of the previous evidence
                and height, then the element-wise update and the column scan (eager torch; its cells are not bit-equal to ours at cell
                edges, its cost is what is compared) -- and the floor no launch can beat: ONE device copy that moves the same number of
                bytes (11 read and 7 written per cell: a copy of 9).
  (b) pipeline  PipelinedPredictor at bs 1 with four slots: ``ground_grid`` alone, with ``ground_memory``, and with
                ``ground_memory=dict(obstacles=True)`` + ``obstacles`` against ``ground_grid`` + ``obstacles``; alternating repeats.  The
                fuse launch of a step waits for the previous step's on another stream: this is what that ordering costs.
"""
from __future__ import annotations

import argparse
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
STEPS = (("kernel", 300), ("pipeline", 500))             # name, time limit in seconds
OPTIONS = dict(free=2, occupied=4, decay=1, limit=32, free_at=4, occupied_at=6)


def torch_fuse(state, spec, motion, prev_e, h_max, prev_h, free, occupied, decay, limit, free_at, occupied_at):
    """Statement F with torch ops on the device: the warp by ``affine_grid`` / ``grid_sample(mode="nearest")`` in normalised coordinates."""
    import torch
    import torch.nn.functional as F
    x0, y0, cell, GX, GY = spec
    B = state.shape[0]
    Wm, Hm = GX * cell, GY * cell
    c, s, tx, ty = (motion[:, i] for i in range(4))
    theta = torch.stack([torch.stack([c, -s * Hm / Wm, c - s * Hm / Wm + 2 * (c * x0 - s * y0 + tx - x0) / Wm - 1], 1),
                         torch.stack([s * Wm / Hm, c, s * Wm / Hm + c + 2 * (s * x0 + c * y0 + ty - y0) / Hm - 1], 1)], 1)
    grid = F.affine_grid(theta, (B, 2, GY, GX), align_corners=False)
    both = F.grid_sample(torch.stack([prev_e.float(), prev_h], 1), grid, mode="nearest", padding_mode="zeros", align_corners=False)
    carried, q = both[:, 0], both[:, 1]
    faded = torch.sign(carried) * (carried.abs() - decay).clamp(min=0)
    hit = (state == 2).float() * occupied - (state == 1).float() * free
    evidence = (faded + hit).clamp(-limit, limit)
    fused = (evidence >= occupied_at).to(torch.uint8) * 2 + (evidence <= -free_at).to(torch.uint8)
    ninf = torch.full_like(h_max, float("-inf"))
    h = torch.maximum(torch.where(state == 2, h_max, ninf), torch.where(carried > 0, q, ninf))
    fused_h = torch.where((evidence > 0) & (h > float("-inf")), h, torch.zeros_like(h))
    occ = fused == 2
    first = torch.where(occ.any(1), y0 + occ.float().argmax(1).float() * cell, torch.full((B, GX), float("inf"), device=state.device))
    return evidence.to(torch.int16), fused, fused_h, first


def step_kernel() -> None:
    import numpy as np
    import torch
    import ground_grid_measure as gm
    import ground_memory_ref as ref
    from objcavit_amd import hip_ops
    from objcavit_amd.ground_grid import grid_of
    spec = grid_of()
    rspec = ref.Spec(*spec)
    motions = {"identity": ref.motion_of(), "yaw 90 + 6 m": ref.motion_of(0.0, 6.0, math.pi / 2)}
    rows = []
    for B in (16, 1):
        c = ref.case(rspec, B, seed=1)
        state, h_max, prev_e, prev_h = (torch.from_numpy(a).cuda() for a in (c.state, np.nan_to_num(c.h_max, nan=0.0, neginf=0.0), c.prev_evidence, c.prev_h))
        dtypes = {"evidence": torch.int16, "state": torch.uint8}
        out = {n: torch.empty((B, spec[3]) if n == "first_occupied" else (B, spec[4], spec[3]), dtype=dtypes.get(n, torch.float32), device="cuda")
               for n in hip_ops.GROUND_FUSE_WANT}
        n = B * spec[3] * spec[4]
        src, dst = torch.empty(9 * n, dtype=torch.uint8, device="cuda"), torch.empty(9 * n, dtype=torch.uint8, device="cuda")
        copy_us = gm._graph_ms(lambda: dst.copy_(src), 200) * 1e3
        for name, m in motions.items():
            motion = torch.from_numpy(np.repeat(m[None], B, 0)).cuda()
            call = lambda: hip_ops.ground_fuse(state, spec, motion, prev_evidence=prev_e, h_max=h_max, prev_h=prev_h, out=out, **OPTIONS)      # noqa: E731
            call()
            want = ref.fuse(c.state, rspec, motion.cpu().numpy(), c.prev_evidence, np.nan_to_num(c.h_max, nan=0.0, neginf=0.0), c.prev_h, **OPTIONS)
            assert all(ref.same_bytes(out[k].cpu().numpy(), getattr(want, k)) for k in ref.OUTPUTS), "the kernel and the statement disagree"
            us, eager = gm._graph_ms(call, 200) * 1e3, gm._event_ms(call, 200) * 1e3
            other = lambda: torch_fuse(state, spec, motion, prev_e, h_max, prev_h, **OPTIONS)      # noqa: E731
            t = other()
            differ = int((t[0] != out["evidence"]).sum())
            torch_us = gm._event_ms(other, 50) * 1e3
            rows.append((B, name, int(want.inside.sum()) // B, us, eager, torch_us, copy_us, differ))
    print(f"(a) ocv_ground_fuse_fwd (every output: one launch), grid {spec[3]} x {spec[4]} cells; us = the launch replayed from a captured "
          "graph, eager = hip_ops.ground_fuse called in a loop; torch = affine_grid + grid_sample(nearest) + the element-wise update + "
          "the column scan, eager on the device; copy = one device copy of 9 bytes per cell (the same traffic), replayed from a graph; "
          "carried = cells per image with a source inside; differ = cells of the batch whose evidence the torch formulation rounds "
          "into another source cell")
    print(f"    {'bs':>3} {'motion':<13} {'carried':>8} {'us':>8} {'eager us':>9} {'torch us':>9} {'torch / ours':>13} {'copy us':>8} {'ours / copy':>12} {'differ':>7}")
    for B, name, inside, us, eager, torch_us, copy_us, differ in rows:
        print(f"    {B:>3} {name:<13} {inside:>8} {us:8.1f} {eager:9.1f} {torch_us:9.1f} {torch_us / us:13.1f} {copy_us:8.1f} {us / copy_us:12.2f} {differ:>7}")


def step_pipeline() -> None:
    import torch
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.ground_memory import ego_motion
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
    egos = [ego_motion(0.01 * (i - 4), 0.4, 0.005 * (i - 4)).cuda() for i in range(POOL)]      # on the device already: the upload is the caller's
    ground = dict(pitch=0.07, band=(-5.0, 5.0))
    kinds = {"ground_grid alone": dict(), "ground_grid + ground_memory": dict(ground_memory={}),
             "ground_grid + obstacles": dict(obstacles={}),
             "ground_grid + ground_memory(obstacles=True) + obstacles": dict(obstacles={}, ground_memory=dict(obstacles=True))}
    pps = {name: PipelinedPredictor(model, args, frames[0], slots=4, want=("depth",), ground_grid=ground, **kw) for name, kw in kinds.items()}

    def run(pp):
        memory = pp.ends.memory is not None
        for i in range(N):
            pp.submit(frames[i % POOL], first_image_id=i, intrinsics=K, **(dict(ego_motion=egos[i % POOL]) if memory else {}))
        return pp.collect()

    last = {name: run(pp)[-1] for name, pp in pps.items()}                      # warm-up of all
    f = last["ground_grid + ground_memory"].ground_memory
    assert f is not None and last["ground_grid alone"].ground_memory is None
    occupied, frame = int((f.state == 2).sum()), int((last["ground_grid alone"].ground.state == 2).sum())
    rates = {name: [] for name in pps}
    for _ in range(3):                                   # alternating repeats
        for name, pp in pps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pp)
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"(b) PipelinedPredictor, bs 1, four slots, flip-TTA, {H}x{W}, {N} steps per repeat, three alternating repeats, img/s "
          f"({frame} occupied cells in the last frame's grid, {occupied} in the fused map after {N} steps)")
    for name, r in rates.items():
        print(f"    {name:<58} " + "  ".join(f"{v:7.1f}" for v in r) + f"   mean {sum(r) / 3:7.1f}  spread {max(r) - min(r):5.1f}")
    mean = {name: sum(r) / 3 for name, r in rates.items()}
    names = list(mean)
    for a, b in ((names[0], names[1]), (names[2], names[3])):
        print(f"    [{a}] - [{b}] = {mean[a] - mean[b]:.1f} img/s = {(1 / mean[b] - 1 / mean[a]) * 1e6:.1f} us per image; ratio {mean[b] / mean[a]:.4f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_memory.txt"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")          # before torch initialises HIP: four slots, four hardware queues
        import torch
        if not torch.cuda.is_available():
            print("measure_ground_memory: no GPU -- nothing is measured without one", file=sys.stderr)
            return 2
        {"kernel": step_kernel, "pipeline": step_pipeline}[a.step]()
        return 0
    text = ["ground memory on MI355X (tools/measure_ground_memory.py); event-timed launches after warm-up, fastest of three windows", ""]
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=dict(os.environ))
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"measure_ground_memory: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
