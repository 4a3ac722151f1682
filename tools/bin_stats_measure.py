"""Measure the bin head's per-pixel statistics on one MI355X -> profiles/bin_stats.txt.

    python tools/bin_stats_measure.py [--out profiles/bin_stats.txt] [--parent DIR] [--rounds 3]

Steps, each a child process of its own under its own time limit, chained: the run stops at the first step that fails (a step that
faulted the device is not followed by another launch).
  (a) accuracy  e32 / eHIP of var and pmax for every (shape, gain, route) and of the finalize launch: the figures
                tests/test_hip_bin_stats.py prints before it asserts (the test run IS the measurement: same inputs, same references)
  (b) head      the head launch at bs 16, 240 x 320 on the h2 route, depth alone against depth + var + pmax, on the benchmark's own maps
                (the model and input of bench.py's default configuration, through forward_until_head) and on a flat softmax (every
                bin tile kept); h2dense and split3 beside it
  (c) finalize  the finalize launch(es) at bs 16, 240 x 320 -> 480 x 640 with flip-TTA: the depth map alone, and with depth_std +
                confidence (a second launch)
  (d) off       statistics OFF: bench.py --gpus 1 at this tree and at a checkout of the parent commit (--parent DIR, library built
                there), alternating, ``--rounds`` times each: the bin_head event time and the JSON line's value, with both spreads.
                Without --parent the step is skipped and the file says so.
  (e) registers VGPRs / AGPRs / scratch / LDS of every instantiation of csrc/bin_head.hip and csrc/depth_finalize.hip from the
                compiler's kernel-resource-usage remarks (a device-only compile; needs hipcc, no GPU)
Kernel times: HIP events around a run of launches on one stream after warm-up, the fastest of three windows.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("accuracy", 420), ("head", 300), ("finalize", 120), ("registers", 300), ("off", 1100))     # name, time limit in seconds


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


def step_accuracy() -> None:
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_hip_bin_stats.py"), "-m", "gpu", "-s", "-q",
                        "-k", "bin_head_stats or finalize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    # printed result lines only (pytest -q puts its progress dots in front of them): "bin_stats 3x37x53 ...", "finalize_stats 5x7->..."
    lines = [m.group(1) for m in (re.match(r"^\.*\s*((?:bin_stats|finalize_stats) \d+x\d.*)$", ln) for ln in r.stdout.splitlines()) if m]
    print("(a) largest absolute error against float64 (tests/bin_stats_ref.py): e32 = the plain fp32 torch formulation on the CPU,")
    print("    eHIP = the kernel; bars: var eHIP <= 2 e32 + 8.5e-9 range^2 (8.5e-7 m^2 here), pmax eHIP <= 2 e32 + 8.5e-9 + 2^-23")
    for ln in lines:
        print("    " + ln.strip())
    print("    pytest: " + r.stdout.strip().splitlines()[-1])
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        sys.exit(r.returncode)


def step_head() -> None:
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from objcavit_amd import hip_ops
    torch.set_grad_enabled(False)
    wl = bench.Workload(2)
    model, _, _ = bench.build_model(torch.device("cuda"), wl)
    img = bench.synthetic_images(wl.batch, 1234, wl.H, wl.W).cuda()
    feat, queries, centers, _, _ = model.forward_until_head(img)
    conv = model.conv_out[0]
    w, b = conv.weight.detach(), conv.bias.detach()
    B, _, h, wd = feat.shape
    flat_feat = torch.randn(B, 128, h, wd, device="cuda").contiguous(memory_format=torch.channels_last)
    flat_q = 0.5 * torch.randn(B, 128, 128, device="cuda")
    print(f"(b) head launch (ocv_bin_head_folded_ws_fwd against ocv_bin_head_folded_stats_fwd with var + pmax), bs {B}, {h} x {wd}, us")
    print(f"    {'maps':>12} {'route':>8} {'depth':>9} {'+var+pmax':>10} {'ratio':>7}")
    for maps, (f, q, ww) in (("benchmark", (feat, queries, w)), ("flat", (flat_feat, flat_q, w * 0.02))):
        for route in ("h2", "h2dense", "split3"):
            os.environ["OCV_BINHEAD"] = route
            t = []
            for stats in (False, True):
                hip_ops.enable_timing(True)
                for _ in range(30):
                    hip_ops.bin_head(f, q, ww, b, centers, stats=stats)
                hip_ops.enable_timing(True)             # (reset: the 30 calls above were the warm-up)
                for _ in range(200):
                    hip_ops.bin_head(f, q, ww, b, centers, stats=stats)
                t.append(hip_ops.timing_results()["bin_head"][1] * 1e3)
                hip_ops.enable_timing(False)
            print(f"    {maps:>12} {route:>8} {t[0]:9.1f} {t[1]:10.1f} {t[1] / t[0]:7.2f}")
    os.environ.pop("OCV_BINHEAD", None)


def step_finalize() -> None:
    import torch
    sys.path.insert(0, ROOT)
    from objcavit_amd import hip_ops
    B, h, w, H, W = 16, 240, 320, 480, 640
    pred, mirror = torch.rand(B, 1, h, w, device="cuda") * 10.0, torch.rand(B, 1, h, w, device="cuda") * 10.0
    var, var_m = torch.rand(B, 1, h, w, device="cuda"), torch.rand(B, 1, h, w, device="cuda")
    pm, pm_m = torch.rand(B, 1, h, w, device="cuda"), torch.rand(B, 1, h, w, device="cuda")
    kw = dict(pred_mirror=mirror, var=var, pmax=pm, var_mirror=var_m, pmax_mirror=pm_m)
    print(f"(c) finalize at bs {B}, {h} x {w} -> {H} x {W}, flip-TTA, us per step (the two new maps come from a second launch)")
    for want in (("depth",), ("depth", "depth_std", "confidence"), ("depth_std", "confidence")):
        out = hip_ops.depth_finalize(pred, 0.001, 10.0, (H, W), want=want, **kw)
        ms = _event_ms(lambda: hip_ops.depth_finalize(pred, 0.001, 10.0, (H, W), want=want, out=out, **kw), 200)
        nbytes = (2 if want == ("depth",) else 6) * pred.numel() * 4 + sum(t.numel() * 4 for t in out.values())
        print(f"    {'+'.join(want):>32} {ms * 1e3:8.1f} us {nbytes / 1e6:8.2f} MB {nbytes / ms / 1e6:8.0f} GB/s")


def _bench_once(tree: str, steps: int, warmup: int):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tree)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(r.returncode)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    def find(o, key):
        if isinstance(o, dict):
            if key in o:
                return o[key]
            for v in o.values():
                f = find(v, key)
                if f is not None:
                    return f
        return None
    bh = find(line, "bin_head")
    ms = bh.get("ms", bh.get("mean_ms")) if isinstance(bh, dict) else bh
    return float(line["value"]), (None if ms is None else float(ms)), line.get("unit", "")


def step_off(parent: str, rounds: int) -> None:
    if not parent:
        print("(d) statistics off against the parent commit: NOT MEASURED (no --parent checkout given)")
        return
    res = {"parent": [], "this": []}
    unit = ""
    for _ in range(rounds):                               # alternating, same box, same session
        for name, tree in (("parent", parent), ("this", ROOT)):
            v, ms, unit = _bench_once(os.path.abspath(tree), 10, 3)
            res[name].append((v, ms))
    print(f"(d) statistics off: bench.py --gpus 1 --steps 10 --warmup 3, parent commit and this tree alternating, {rounds} runs each")
    for name, r in res.items():
        vals, mss = [a for a, _ in r], [b for _, b in r if b is not None]
        print(f"    {name:>7}  value ({unit}) " + " ".join(f"{v:9.3f}" for v in vals) + f"   spread {max(vals) - min(vals):.3f}")
        if mss:
            print(f"    {name:>7}  bin_head ms     " + " ".join(f"{v:9.4f}" for v in mss) + f"   spread {max(mss) - min(mss):.4f}")
    pv, tv = [a for a, _ in res["parent"]], [a for a, _ in res["this"]]
    print(f"    mean value: parent {sum(pv) / len(pv):.3f}, this {sum(tv) / len(tv):.3f}; difference {sum(tv) / len(tv) - sum(pv) / len(pv):+.3f} "
          f"against the parent's own spread of {max(pv) - min(pv):.3f}")


def step_registers() -> None:
    sys.path.insert(0, ROOT)
    from objcavit_amd import build
    print("(e) compiler's kernel-resource-usage remarks (gfx950, -O3): VGPRs / AGPRs / scratch bytes per lane / static LDS bytes")
    for src in ("bin_head.hip", "depth_finalize.hip"):
        r = subprocess.run([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast",
                            "--cuda-device-only", "-S", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(build.CSRC, src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout)
            sys.exit(r.returncode)
        cur = {}
        for ln in r.stdout.splitlines():
            m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\S+)", ln)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = {"name": subprocess.run(["c++filt", m.group(2)], stdout=subprocess.PIPE, text=True).stdout.strip() or m.group(2)}
            else:
                cur[m.group(1).split()[0]] = m.group(2)
                if m.group(1).startswith("LDS"):
                    name = re.sub(r"\(anonymous namespace\)::", "", cur["name"]).split("(")[0]
                    print(f"    {name:<58} {cur.get('VGPRs', '?'):>4} {cur.get('AGPRs', '?'):>4} {cur.get('ScratchSize', '?'):>4} {cur.get('LDS', '?'):>6}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin_stats.txt"))
    ap.add_argument("--parent", default="", help="a checkout of the parent commit with its library built (step d)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated subset of the steps")
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        if a.step not in ("registers",) and not (a.step == "off" and not a.parent):
            import torch
            if not torch.cuda.is_available():
                print("bin_stats_measure: no GPU -- nothing is measured without one", file=sys.stderr)
                return 2
        {"accuracy": step_accuracy, "head": step_head, "finalize": step_finalize, "registers": step_registers,
         "off": lambda: step_off(a.parent, a.rounds)}[a.step]()
        return 0
    only = [s for s in a.only.split(",") if s]
    text = ["per-pixel depth uncertainty from the bin head on MI355X (tools/bin_stats_measure.py); event-timed launches after warm-up", ""]
    for name, limit in STEPS:
        if only and name not in only:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(a.rounds)]
        if a.parent:
            cmd += ["--parent", a.parent]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"bin_stats_measure: step {name} failed with exit status {r.returncode}; stopping here", file=sys.stderr)
            return r.returncode
        print(r.stdout, end="", flush=True)
        text += [r.stdout.rstrip(), ""]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                      # after every step: what was measured survives a later step's failure
            f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
