#!/usr/bin/env python3
"""Benchmark of the ObjCAViT forward depth-inference hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

N = 1 runs in this process.  N > 1: if the process was started by a launcher (``python -m torch.distributed.run
--nproc-per-node N ... bench.py --gpus N``: RANK / LOCAL_RANK / WORLD_SIZE in the environment) it is one rank of the
job; otherwise THIS process becomes the launcher: it starts N fresh child processes (one rank per GPU, rendezvous on
127.0.0.1) BEFORE making any GPU call of its own -- a process that has touched the GPU is never re-exec'ed or forked
-- waits for them, and exits non-zero if any rank failed.

A "step" is one GraphBins.forward over one batch of synthetic input that is
already resident in HBM.  Default workload = BASELINE.json configs[2], the
configuration the metric ("images/sec (640x480, bs=16)") is quoted on:
ObjCAViT enet-b5 NYU, emb_dim 128, learned positional MLP, 32 objects per image
with random 512-d "CLIP" text features, batch 16 PER GPU (weak scaling: images
are independent units, sharded by rank, weights replicated, no collective in the
forward; the one collective is a single all-gather of per-image metric records
after the last step).  ``--config 1|3|4`` selects the other BASELINE configurations
(WORKLOADS below) -- same code, same JSON.  Seeded random weights, fp32 results.

A plain run sets up, warms up, times the K steps, writes the last step's outputs
(``--dump-outputs DIR``) and prints the result line; nothing else.  With
``--full``, behind the timed region: the same steps strictly one after the other
(``value_sequential``), and (N = 1; ``--no-extras`` skips them) >= 5 s of
pipelined steps (``sustained_images_per_s``), one eager pass for the per-kernel
table, the workload again with every contraction on exact-fp32 arithmetic
(``exact_fp32_images_per_s``, same process), the other BASELINE configurations
and small batches, and the CPU oracle (``--no-cpu-baseline`` skips it).

Rank 0 prints ONE JSON line (contract in the task statement) with extra objects:
"roofline" (dominant hand-written kernel, live HIP-event timing inside the timed
region) and, with ``--full``, "cpu_baseline" (the CPU oracle timed on the host
cores on a bounded sample, N = 1 only).

``--dump-outputs DIR``: what the timed path returned in its last step -- depth,
bin edges and the per-image metric records -- as DIR/<name>.npy (float32), at most
64 MB in all (a larger array is stored as a fixed, seeded sample of its
elements).  The inputs are seeded, so two builds run with the same arguments can
be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

# ROCm maps HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4: the first two streams a process creates get
# queues of their own, later ones share the last) and streams that share a queue run one after the other; the pipelined
# mode below needs its slot streams on queues of their own.  Must be set before the HIP runtime loads.
# Round 5: FOUR, not eight -- three slots + the default stream fit four queues (same pipelined rate: 1052 vs 1056 img/s), and only
# on <= 4 hardware queues may a lone batch's capture fork side streams (hip_ops.hw_queues_allow_forks: a forked graph replays 3x
# slower on 6+ queues; lone-batch rate 1010 vs 977 img/s at bs 16, 310 vs 294 at bs 1: profiles/r05_graph_shapes.txt).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
F32_MFMA_PEAK_TFLOPS = 157.3  # v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0  # v_mfma_f32_32x32x16_bf16 / _f16, dense: the same peak for both 2-byte types (the split convolutions issue 3 MFMAs per product)

E, NBINS = 128, 256

# BASELINE.json configs[1..4] as benchmark workloads (configs[0] is the reference's CPU-only case: a parity test, no
# bench line).  --config 2 -- the configuration the metric is quoted on -- is the default and the driver's line; the others
# are measured with the same code and committed as profiles/r03_configs.json.  Batch = the per-GPU shard of the config.
KITTI_GAINS = (("in_proj_weight", 2.0), ("conv_out", 1.0), ("conv3x3", 1.0), ("regressor.4", 3.0))    # tests/test_hip_configs.py
WORKLOADS = {
    1: dict(dataset="nyu", H=480, W=640, batch=8, n_obj=16, language="control_obj_zeros_512", kw=dict(strategy="learned"),
            gains="PEAKY", desc="ObjCAViT enet-b5 NYU 480x640, emb_dim=128, learned pos-MLP, 16 objs/img with ZERO features "
                                "(control_obj_zeros_512)"),
    2: dict(dataset="nyu", H=480, W=640, batch=16, n_obj=32, language="clip", kw=dict(strategy="learned"), gains="PEAKY",
            desc="ObjCAViT enet-b5 NYU 480x640, emb_dim=128, learned pos-MLP, 32 objs/img with random 512-d text features"),
    3: dict(dataset="kitti", H=352, W=1216, batch=8, n_obj=24, language="clip", kw=dict(strategy="learned_bbox_wh", use_2_saca=True),
            gains="KITTI", desc="ObjCAViT enet-b5 KITTI 352x1216 (KB crop), learned_bbox_wh pos-MLP, 2x SA/CA stack, 24 objs/img "
                                "with random 512-d text features (per-GPU shard of bs=32 over 4 GPUs)"),
    4: dict(dataset="nyu", H=480, W=640, batch=16, n_obj=64, language="clip", kw=dict(strategy="grid_random_roi_align"),
            gains="PEAKY", desc="ObjCAViT enet-b5 NYU 480x640, grid_random_roi_align positional table, 64 objs/img with random "
                                "512-d text features, hipGraph-captured (per-GPU shard of bs=128 over 8 GPUs)"),
}


class Workload:
    def __init__(self, idx, batch=None):
        c = WORKLOADS[idx]
        self.idx, self.dataset, self.H, self.W = idx, c["dataset"], c["H"], c["W"]
        self.batch = batch or c["batch"]
        self.n_obj, self.language, self.kw, self.desc = c["n_obj"], c["language"], dict(c["kw"]), c["desc"]
        self.gains_name = c["gains"]
        self.h, self.w = self.H // 2, self.W // 2
        self.P = self.h * self.w
        self.S = (self.h // 16) * (self.w // 16)
        self.max_depth = 80.0 if self.dataset == "kitti" else 10.0
        self.min_depth = 0.001
        self.stacks = 2 if self.kw.get("use_2_saca") else 1

    def gains(self):
        from objcavit_amd import synth as gen
        return gen.PEAKY if self.gains_name == "PEAKY" else KITTI_GAINS


def kernel_model(B, wl):
    """Algorithmic bytes / flops per LAUNCH of each hand-written entry point (SURVEY.md section 8d figures x B,
    weights counted once per launch).  bin_head flops are those of the folded association the kernel executes
    ((Wout.Q).feat: 2*256*128 per pixel + the per-image fold), not the reference's unfused 7.69 GFLOP/img."""
    S, P = wl.S, wl.P
    act = S * E * 4
    return {
        "bin_head": dict(bytes=B * (P * 128 * 4 + P * 4) + B * NBINS * 128 * 4,
                         flops=B * (2 * NBINS * 128 * P + 2 * NBINS * 128 * 128)),
        "patch_embed": dict(bytes=B * (P * 128 * 4 + act) + 128 * 128 * 256 * 4, flops=B * 2 * S * 128 * 128 * 256),
        # cross-attention #1 AS THE REFERENCE EXECUTES IT (Sk = S; modules/ObjCAViT.py:195-201): SURVEY 8d
        "mha_cross": dict(bytes=B * (3 * act + S) + 4 * E * E * 4 + 4 * E * 4,
                          flops=B * (4 * 2 * S * E * E + 2 * 2 * S * S * E)),
        # cross-attention #2 (use_2_saca only; :202-207): Q = K-source = padded objects [S, E], V = objects, no mask
        "mha_cross_full": dict(bytes=B * 3 * act + 4 * E * E * 4 + 4 * E * 4,
                               flops=B * (4 * 2 * S * E * E + 2 * 2 * S * S * E)),
        "encoder_layer": dict(bytes=B * 2 * act + (4 * E * E + 2 * E * 1024) * 4,
                              flops=B * (4 * 2 * S * E * E + 2 * 2 * S * S * E + 2 * 2 * S * E * 1024)),
        # the image-token stack: 4 layers in 9 launches (packed projection, then attention + layer tail per layer)
        "encoder_stack": dict(bytes=4 * (B * 2 * act + (4 * E * E + 2 * E * 1024) * 4),
                              flops=4 * B * (4 * 2 * S * E * E + 2 * 2 * S * S * E + 2 * 2 * S * E * 1024)),
        # the object-token stack (modules/ObjCAViT.py:184-190): the same four layers over n_obj tokens per image
        "encoder_stack_obj": dict(bytes=4 * (B * 2 * wl.n_obj * E * 4 + (4 * E * E + 2 * E * 1024) * 4),
                                  flops=4 * B * (4 * 2 * wl.n_obj * E * E + 2 * 2 * wl.n_obj * wl.n_obj * E + 2 * 2 * wl.n_obj * E * 1024)),
    }


def build_model(device, wl):
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    args = make_args(dataset=wl.dataset, language=wl.language, dimensions_train=[wl.H, wl.W], dimensions_test=[wl.H, wl.W], **wl.kw)
    model = GraphBins(args, object_provider=SyntheticObjectProvider(wl.n_obj, wl.language, seed=42)).eval()
    sd = gen.load_into(model, 42, wl.gains())
    return model.to(device), sd, args


def synthetic_images(B, seed, H, W):
    """image = (rand - mean) / std with ImageNet statistics (modules/GraphBinsLM.py:45,70-73), CPU generator."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=g)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return (x - mean) / std


# ---------------------------------------------------------------------------
# CPU baseline (SURVEY.md section 8d / BASELINE.md section 3)
# ---------------------------------------------------------------------------
def host_cpu_info():
    """Physical cores (unique (package, core) pairs of /proc/cpuinfo), the CPU model string, and what this process may
    actually use: its affinity mask and the cgroup CPU quota, if any."""
    model, pairs, phys, core = "unknown", set(), None, None
    try:
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
            elif k == "" and phys is not None and core is not None:
                pairs.add((phys, core))
                phys = core = None
        if phys is not None and core is not None:
            pairs.add((phys, core))
    except OSError:
        pass
    logical = os.cpu_count() or 1
    affinity = len(os.sched_getaffinity(0))
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    quota = float(txt[0]) / float(txt[1])
            elif float(txt[0]) > 0:
                quota = float(txt[0]) / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            break
        except (OSError, ValueError, IndexError):
            continue
    physical = len(pairs) or max(1, logical // 2)
    return dict(cpu_model=model, physical_cores=physical, logical_cpus=logical, affinity_cpus=affinity, cgroup_cpu_quota=quota)


def cpu_baseline(sd, img_cpu, feats, boxes, gpu_depth, wl, budget_s=60.0):
    """The oracle (CPU restatement pinned to the reference's own modules) on the host cores, as SURVEY.md section 8d
    states it: threads = physical cores of the box (capped by what this process may use: affinity mask / cgroup
    quota -- all of it reported), fp32, eval, same weights and inputs as the GPU run, 2 warm-ups + median of 5 at
    bs = 1 and at bs = 16 -- or, if 7 passes of bs = 16 do not fit ``budget_s`` seconds, at the largest batch that
    does (said in `sample`)."""
    import torch
    from oracle import restate
    info = host_cpu_info()
    threads = info["physical_cores"]
    if info["cgroup_cpu_quota"]:
        threads = min(threads, max(1, int(info["cgroup_cpu_quota"])))
    threads = max(1, min(threads, info["affinity_cpus"]))
    torch.set_num_threads(threads)

    def run(k):
        # use_2_saca couples images through the batch's Nmax only; every image has wl.n_obj objects here
        return restate.graphbins_forward(img_cpu[:k], [f.cpu() for f in feats[:k]], [b.cpu() for b in boxes[:k]], sd,
                                         wl.min_depth, wl.max_depth, **wl.kw)

    def med5(k):
        for _ in range(2):
            run(k)
        ts, depth = [], None
        for _ in range(5):
            t0 = time.perf_counter()
            depth, _ = run(k)
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[2], depth

    t1, depth1 = med5(1)
    nmax = img_cpu.shape[0]
    k = nmax
    while k > 1 and 7 * t1 * k > budget_s:            # cost is close to linear in the batch
        k //= 2
    tk, depthk = (t1, depth1) if k == 1 else med5(k)
    rel = ((gpu_depth[:k].cpu() - depthk).abs() / depthk)
    note = "" if k == nmax else f" (bs={nmax} does not fit {budget_s:.0f} s of CPU time at {t1:.2f} s per image: largest batch that does)"
    cb = dict(value=round(k / tk, 4), unit="images/s", cores=threads, kind="port", cpu_model=info["cpu_model"],
              physical_cores=info["physical_cores"], logical_cpus=info["logical_cpus"], affinity_cpus=info["affinity_cpus"],
              cgroup_cpu_quota=info["cgroup_cpu_quota"], bs1_images_per_s=round(1.0 / t1, 4), batch=k,
              sample=f"oracle/restate.graphbins_forward on the same workload ({wl.H}x{wl.W}, {wl.n_obj} objs/img), fp32, eval, "
                     f"{threads} torch threads; 2 warm-ups + median of 5: bs=1 {t1:.3f} s, bs={k} {tk:.3f} s{note}")
    return cb, float(rel.mean()), float(rel.max())


# ---------------------------------------------------------------------------
# per-kernel report and the roofline object
# ---------------------------------------------------------------------------
def kernel_report(timing, a, B, wl, split_f16=True):
    """{"roofline": ..., "kernels": ..., "convs": ...} from the HIP-event durations of the entry points
    (name -> (launches, mean ms)) and the algorithmic bytes / flops of ``kernel_model``.  ``split_f16``: the element type of
    the direct convolutions' two-term splits (fp16 pairs since round 4; bf16 pairs on the fallback / A-B route)."""
    km = kernel_model(B, wl)
    kernels, convs = {}, []
    for name, (cnt, ms) in timing.items():
        if name.startswith(("conv3x3|", "conv1x1|", "conv3x3w4|", "conv3x3p|")):
            k = 1 if name.startswith("conv1x1") else 3
            packed = name.startswith("conv3x3p|")                    # packed taps: K = the nine taps' real 8-channel granules (round 6)
            # Winograd launches (the timing name says so): F(4x4,3x3) = 36 multiplies per 16 outputs on two-term fp16 splits; direct = 9 per output
            wino = 4 if name.startswith("conv3x3w4|") else 0
            per_out = {0: 1.0, 4: 36.0 / 144.0}[wino]
            mfma_dtype = "f16" if (wino == 4 or split_f16) else "bf16"
            b_, h_, w_, ci, co = (int(v) for v in name.split("|")[1].split(","))
            m_ = b_ * h_ * w_
            flops = 2.0 * m_ * co * ci * k * k                      # algorithmic (fp32-equivalent, direct-form) FLOPs
            # 2-byte matrix-core FLOPs the launch(es) actually issue (3 MFMAs per product) over the K the kernel walks: every tap padded
            # to a multiple of 32 channels (tap-major), or ceil(9 ceil(Cin / 8) / 4) steps of 32 (packed taps)
            k_walked = ((9 * ((ci + 7) // 8) + 3) // 4 * 32) if packed else k * k * ((ci + 31) // 32 * 32)
            issued = 3 * 2.0 * m_ * co * k_walked * per_out
            byts = m_ * ci * 4 + m_ * co * 4 + k * k * co * ci * 4   # read input once, write output once, weights
            form = "direct, packed taps" if packed else {0: "direct", 4: "winograd F(4x4,3x3), 3 launches"}[wino]
            convs.append(dict(shape=f"B{b_} {h_}x{w_} {ci}->{co} k{k}", form=form, mfma_dtype=mfma_dtype,
                              launches_per_step=cnt / a.steps, ms=round(ms, 4),
                              alg_GFLOP=round(flops / 1e9, 1), alg_MB=round(byts / 1e6, 1),
                              alg_TFLOPs=round(flops / (ms * 1e-3) / 1e12, 1),
                              issued_mfma_TFLOPs=round(issued / (ms * 1e-3) / 1e12, 1),
                              frac_mfma_algorithmic=round(flops / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
                              frac_mfma_issued=round(issued / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
                              k_walked=k_walked, k_real=k * k * ci,
                              GBps=round(byts / (ms * 1e-3) / 1e9, 1)))
            continue
        if name.startswith("tap_interp|"):
            b_, h_, w_, co = (int(v) for v in name.split("|")[1].split(","))
            m_ = b_ * h_ * w_
            byts = m_ * co * 4 * (9 / 4 + 1 + 1)        # tap products at ~1/4 of the pixels, skip part, output (hl32 = 4 B too)
            convs.append(dict(shape=f"B{b_} {h_}x{w_} ->{co}", form="tap interpolation + skip part + bias + LeakyReLU + split "
                              "(third launch of a low-resolution first convolution)", launches_per_step=cnt / a.steps,
                              ms=round(ms, 4), alg_MB=round(byts / 1e6, 1), GBps=round(byts / (ms * 1e-3) / 1e9, 1)))
            continue
        if name not in km:
            continue
        gbs = km[name]["bytes"] / (ms * 1e-3) / 1e9
        tfs = km[name]["flops"] / (ms * 1e-3) / 1e12
        kernels[name] = dict(launches_per_step=cnt / a.steps, ms=round(ms, 4), alg_MB=round(km[name]["bytes"] / 1e6, 3),
                             alg_GFLOP=round(km[name]["flops"] / 1e9, 3), GBps=round(gbs, 1), TFLOPs=round(tfs, 2),
                             frac_hbm=round(gbs / HBM_PEAK_GBS, 4), frac_mfma_f32=round(tfs / F32_MFMA_PEAK_TFLOPS, 4),
                             total_ms_per_step=round(ms * cnt / a.steps, 4))
    # SelfAttnCrossAttn.forward as a whole (modules/ObjCAViT.py:167-213): object stack + image stack + cross-attention #1 -- 9 + 9 + 1
    # launches of a few hundred workgroups each; what the SUM of their event times is against the bytes the three move
    tail = [n for n in ("encoder_stack_obj", "encoder_stack", "mha_cross") if n in kernels]
    if len(tail) == 3:
        ms = sum(kernels[n]["total_ms_per_step"] for n in tail)
        byts, fl = sum(km[n]["bytes"] for n in tail), sum(km[n]["flops"] for n in tail)
        kernels["sa_ca_tail"] = dict(parts=tail, ms=round(ms, 4), alg_MB=round(byts / 1e6, 3), alg_GFLOP=round(fl / 1e9, 3),
                                     GBps=round(byts / (ms * 1e-3) / 1e9, 1), TFLOPs=round(fl / (ms * 1e-3) / 1e12, 2),
                                     frac_hbm=round(byts / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                     frac_mfma_f32=round(fl / (ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4), total_ms_per_step=round(ms, 4),
                                     note="latency-bound chain of 19 launches (one image's tokens fit a few workgroups): neither roof applies; "
                                          "under three batches in flight it runs beside the other slots' convolutions")
    dom = max((k for k in kernels if k != "sa_ca_tail"), key=lambda k: kernels[k]["ms"]) if kernels else None     # longest single launch
    roofline = None
    traffic_all = {}
    tpath = os.path.join(ROOT, "profiles", "roofline_traffic.json")
    if os.path.exists(tpath):
        traffic_all = json.load(open(tpath))
    # the roofline launch is a FIXED one -- the eager islands of the graph replay, the direct 128 -> 128 convolution at
    # half resolution (three launches per step -- two of them islands: the heads' conv3x3 stays in the graph, beside the token
    # chain (hip_ops.head_overlap_enabled) --, the longest single launches of the step since the first convolution of
    # every decoder stage runs at the low resolution; profiles/roofline_traffic.json holds the PMC traffic of this launch)
    island_shape = f"B{B} {wl.h}x{wl.w} 128->128 k3"
    direct = [c for c in convs if c["form"] == "direct" and " k3" in c["shape"]]
    conv_dom = next((c for c in direct if c["shape"] == island_shape), None) or (max(direct, key=lambda c: c["ms"]) if direct else None)
    if conv_dom and (dom is None or max(c["ms"] for c in convs) > kernels[dom]["ms"]):
        # dominant hand-written kernel = the split-bf16 implicit-GEMM convolution (conv_split_dma_kernel): matrix-pipe
        # bound (AI >> ridge).  `achieved` = ALGORITHMIC flops / duration (the task's definition); the kernel issues
        # three bf16 MFMAs per algorithmic product, so the matrix pipe's own utilisation is 3x that (frac_issued).
        roofline = dict(kernel="conv_split_dma_kernel " + conv_dom["shape"], bound="mfma",
                        achieved=conv_dom["alg_TFLOPs"], peak=BF16_MFMA_PEAK_TFLOPS, unit="TFLOP/s",
                        frac=conv_dom["frac_mfma_algorithmic"],
                        traffic=traffic_all.get("conv3x3") if (wl.idx == 2 and B == 16) else None,
                        traffic_source=("profiles/roofline_traffic.json: 2 x FETCH_SIZE + WRITE_SIZE of this launch from separate rocprofv3 "
                                        "--pmc passes of this command (tools/profile_round.sh), committed -- NOT measured in this run"
                                        if (wl.idx == 2 and B == 16) else "no PMC pass committed for this workload"),
                        frac_algorithmic=conv_dom["frac_mfma_algorithmic"], frac_issued=conv_dom["frac_mfma_issued"],
                        issued_mfma_TFLOPs=conv_dom["issued_mfma_TFLOPs"], mfma_dtype=conv_dom["mfma_dtype"],
                        x_over_fp32_mfma_peak=round(conv_dom["alg_TFLOPs"] / F32_MFMA_PEAK_TFLOPS, 2),
                        ms=conv_dom["ms"], alg_GFLOP=conv_dom["alg_GFLOP"], alg_MB=conv_dom["alg_MB"],
                        note="achieved / frac = algorithmic fp32-equivalent FLOPs (2*M*N*K*9) per launch over the dense 2-byte "
                             "MFMA peak (2.5 PF for bf16 and for fp16); the two-term split issues 3 MFMAs per product "
                             "(frac_issued = matrix-pipe utilisation); x_over_fp32_mfma_peak = the same rate over the 157.3 TF "
                             "fp32-MFMA peak the reference's arithmetic would be priced on.  The launch runs at the package "
                             "power cap (rocm-smi: 1385-1397 W of 1400 W, sclk 2.02-2.08 GHz; tools/power_probe_conv.sh): "
                             "`peak` assumes 2.4 GHz; fp16 pairs (round 4: 2^-22 products instead of 2^-17) draw more power "
                             "per MFMA than bf16 pairs and run ~4 % slower under that cap (same box: 0.940 vs 0.902 ms)")
    elif dom:
        k = kernels[dom]
        # fp32 contraction kernels sit above the ridge point (157.3 TF / 8 TB/s = 19.7 flop/B): matrix-pipe bound
        ai = km[dom]["flops"] / km[dom]["bytes"]
        if ai > F32_MFMA_PEAK_TFLOPS * 1e12 / (HBM_PEAK_GBS * 1e9):
            roofline = dict(kernel=dom, bound="mfma", achieved=k["TFLOPs"], peak=F32_MFMA_PEAK_TFLOPS, unit="TFLOP/s",
                            frac=k["frac_mfma_f32"], traffic=traffic_all.get(dom), hbm_GBps=k["GBps"], hbm_frac=k["frac_hbm"])
        else:
            roofline = dict(kernel=dom, bound="hbm", achieved=k["GBps"], peak=HBM_PEAK_GBS, unit="GB/s",
                            frac=k["frac_hbm"], traffic=traffic_all.get(dom))
    return {"roofline": roofline, "kernels": kernels, "convs": convs}


_T0 = time.perf_counter()


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


# ---------------------------------------------------------------------------
# launcher: N fresh rank processes, started before this process touches the GPU
# ---------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n, argv):
    """Start ``n`` ranks of this script as child processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their
    environment), wait for all of them; the first failure ends the others (their exact PIDs) and becomes the exit
    code.  The parent has imported neither torch nor the HIP library at this point."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OCV_BENCH_LAUNCHER="self")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    live = set(range(n))
    while live and rc == 0:
        for r in sorted(live):
            code = procs[r].poll()
            if code is not None:
                live.discard(r)
                if code != 0:
                    rc = code
                    print(f"[bench] rank {r} exited with code {code}", file=sys.stderr, flush=True)
        if live and rc == 0:
            time.sleep(0.2)
    for r in live:                                    # a rank failed: end the others
        procs[r].terminate()
    for r in live:
        try:
            procs[r].wait(timeout=30)
        except subprocess.TimeoutExpired:
            procs[r].kill()
    return rc


class StubWorkload:
    """--stub-cpu: the launcher / sharding / gather plumbing on CPU ranks over gloo (tests/test_bench_launch.py).
    NOT the hot path and not a fallback for it: no model, no kernel, the JSON says data = "stub"."""

    def __init__(self, B):
        import torch
        self.B = B
        self.w = torch.arange(1, 4, dtype=torch.float32).view(1, 3, 1, 1)

    def step(self, img, first_id):
        import torch
        depth = (img[:, :, ::2, ::2] * self.w).sum(1, keepdim=True).abs() + 1.0
        rec = torch.zeros(self.B, 10)
        rec[:, 0] = depth.mean(dim=(1, 2, 3))
        rec[:, 8] = 1.0
        rec[:, 9] = torch.arange(first_id, first_id + self.B, dtype=torch.float32)
        return depth, rec


EXACT_ENV = {"OCV_CONV": "exact", "OCV_PW": "fp32", "OCV_TOKENS": "fp32", "OCV_BINHEAD": "exact", "OCV_PATCH_EMBED": "exact", "OCV_ATTN_FORM": "fp32"}


def exact_fp32_pass(device, wl, img, gt, box, B, default_depth, steps=10):
    """The same workload with EVERY contraction on exact-fp32 arithmetic (v_mfma_f32_32x32x2_f32 / FMA), in this process,
    after the timed region: a second model instance with the same seeded weights is built while EXACT_ENV is set (the
    routes are chosen when a module's weight caches are folded), dispatched eagerly, one step after the other.
    -> (images/s, depth of the last step, max relative difference to the default route's depth)."""
    import torch
    from objcavit_amd import hip_ops
    saved = {k: os.environ.get(k) for k in EXACT_ENV}
    os.environ.update(EXACT_ENV)
    try:
        model, _, _ = build_model(device, wl)
        for _ in range(2):
            out = model(img)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            out = model(img)
            hip_ops.depth_metrics(out.depth_pred, gt, wl.min_depth, wl.max_depth, crop=box, first_image_id=i * B)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        depth = out.depth_pred.clone()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    rel = float(((depth - default_depth).abs() / depth).max())
    del model
    return steps * B / dt, depth, rel


DUMP_BUDGET_BYTES = 64 * 1000 * 1000


def dump_outputs(dirname, arrays, seed=1234):
    """Write each array of ``arrays`` (name -> tensor) as ``dirname/<name>.npy``: float32, float64 kept as float64.  The
    smallest arrays are written whole; an array larger than its share of DUMP_BUDGET_BYTES is written as a sample of its
    flattened elements at fixed, seeded positions (the same positions for the same shape on every run).  -> {name: note}."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    cpu = {k: v.detach().cpu().numpy() for k, v in arrays.items() if v is not None}
    cpu = {k: v.astype(np.float64 if v.dtype == np.float64 else np.float32) for k, v in cpu.items()}
    left, notes = DUMP_BUDGET_BYTES, {}
    for i, (name, x) in enumerate(sorted(cpu.items(), key=lambda kv: kv[1].nbytes)):
        share = left // (len(cpu) - i) - 256               # (room for the .npy header)
        if x.nbytes > share:
            k = share // x.itemsize
            idx = np.sort(np.random.default_rng(seed).choice(x.size, size=k, replace=False))
            notes[name] = f"{k} of {x.size} elements of {list(x.shape)} (seeded sample, seed {seed})"
            x = x.reshape(-1)[idx]
        else:
            notes[name] = f"{list(x.shape)} whole"
        np.save(os.path.join(dirname, name + ".npy"), x)
        left -= x.nbytes + 256
    return notes


def cpu_share() -> int:
    """CPUs this job may really use: the affinity mask, capped by the cgroup CPU quota (v2 cpu.max / v1 cfs quota) when there is one."""
    n = len(os.sched_getaffinity(0))
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(float(q) / float(p))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except (OSError, ValueError):
            pass
    return n


def side_leg(device, wl, model, nslot, seconds, seed=42):
    """One more workload behind the timed region, on the driver's clock too: ``wl`` captured as ``nslot``
    hipGraph slots (1 = a lone-batch capture with its side streams, one step strictly after the other), run for ~``seconds``.
    Every step = forward + the fused metric kernel, as in the timed region.  -> dict for the JSON line."""
    import torch
    from objcavit_amd import hip_ops
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.validation import crop_box
    B = wl.batch
    img = synthetic_images(B, seed, wl.H, wl.W).to(device)
    gt = (torch.rand(B, 1, wl.H, wl.W, generator=torch.Generator().manual_seed(7)) * (0.9 * wl.max_depth) + 0.05 * wl.max_depth).to(device)
    box = crop_box(model.args, wl.H, wl.W)
    t_build = time.perf_counter()
    model(img)                                               # calibrating first call of this model / shape
    sts = hip_ops.independent_streams(nslot, device) if nslot > 1 else [None]      # (slots on hardware queues of their own: checked)
    slots = [GraphedGraphBins(model, img, in_flight=nslot, stream=sts[k]) for k in range(nslot)]
    t_build = time.perf_counter() - t_build

    flags = []                                               # every step's taken range-guard word (device, 4 bytes each): read once, below

    def step(k):
        g = slots[k % nslot]
        with torch.cuda.stream(g.stream):
            out = g(img)
            flags.append(g.last_flag)
            hip_ops.depth_metrics(out.depth_pred, gt, wl.min_depth, wl.max_depth, crop=box, first_image_id=0)

    for k in range(2 * nslot):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(nslot):
        step(k)
    torch.cuda.synchronize()
    per_round = max(nslot, int(0.2 / max((time.perf_counter() - t0) / nslot, 1e-4)) // nslot * nslot)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for k in range(per_round):
            step(k)
        torch.cuda.synchronize()
        n += per_round
    dt = time.perf_counter() - t0
    taken = [f for f in flags if f is not None]               # ALL steps of the leg, not the last replay of each slot
    tripped = int(torch.cat(taken).ne(0).sum()) if taken else 0
    nodes = [sum(x for x in g.segment_nodes if x) for g in slots][0]
    forks = sum(t.get("forks", 0) for t in slots[0].segment_topology)      # side-stream forks inside the captured forward (0 = single chain)
    del slots
    torch.cuda.empty_cache()
    return {"images_per_s": round(n * B / dt, 1), "ms_per_step": round(dt / n * 1e3, 3), "batch": B, "inflight": nslot, "steps": n,
            "seconds": round(dt, 2), "graph_nodes": nodes, "graph_forks": forks, "capture_s": round(t_build, 2), "fp16_range_guard_tripped": tripped,
            "workload": f"BASELINE configs[{wl.idx}] {wl.H}x{wl.W}, {wl.n_obj} objs/img, {wl.kw}"}


def pipelined_validation_leg(device, wl, model, nslot, seconds, seed=42):
    """The reference's validation loop as the product serves it: ``validation.PipelinedValidation`` -- one step =
    the ``wl.batch`` images AND their mirrors as one joint forward (modules/GraphBinsLM.py:159,173) + the fused metric kernel, ``nslot``
    steps in flight, records collected per round -- for ~``seconds`` on the driver's clock.  ``images_per_s`` counts VALIDATED images
    (each costs two forwards: ``forwards_per_s``).  -> dict for the JSON line."""
    import torch
    from objcavit_amd import hip_ops
    from objcavit_amd.validation import PipelinedValidation
    B = wl.batch
    img = synthetic_images(B, seed, wl.H, wl.W).to(device)
    gt = (torch.rand(B, 1, wl.H, wl.W, generator=torch.Generator().manual_seed(7)) * (0.9 * wl.max_depth) + 0.05 * wl.max_depth).to(device)
    t_build = time.perf_counter()
    model(torch.cat([img, img.flip(dims=[3])], 0))           # calibrating first call at the joint shape
    pv = PipelinedValidation(model, model.args, img, slots=nslot)
    t_build = time.perf_counter() - t_build
    for k in range(2 * nslot):
        pv.submit(img, gt, first_image_id=k * B)
    pv.collect()
    t0 = time.perf_counter()
    for k in range(nslot):
        pv.submit(img, gt, first_image_id=k * B)
    pv.collect()
    per_round = max(nslot, int(0.2 / max((time.perf_counter() - t0) / nslot, 1e-4)) // nslot * nslot)
    n, rows, t0 = 0, 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for k in range(per_round):
            pv.submit(img, gt, first_image_id=(n + k) * B)
        rows += int(pv.collect().shape[0])                   # one synchronisation + one host read of the round's range-guard words
        n += per_round
    dt = time.perf_counter() - t0
    nodes = sum(x for x in pv.graphs[0].segment_nodes if x)
    out = {"images_per_s": round(n * B / dt, 1), "forwards_per_s": round(2 * n * B / dt, 1), "ms_per_step": round(dt / n * 1e3, 3),
           "batch": B, "slots": nslot, "steps": n, "records": rows, "seconds": round(dt, 2), "graph_nodes_joint_2b": nodes,
           "capture_s": round(t_build, 2), "steps_rerun_on_bf16_pairs": pv.rerun_steps,
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "unset (runtime default 4)"),
           "hw_queue_note": hip_ops.ROUTE_REPORT.get("PipelinedValidation"),
           "workload": f"PipelinedValidation(slots={nslot}): image + mirror per step, BASELINE configs[{wl.idx}] {wl.H}x{wl.W}, {wl.n_obj} objs/img"}
    del pv
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=2, choices=sorted(WORKLOADS),
                    help="BASELINE.json configs[i] as the workload; 2 (default) is the configuration the metric is quoted on")
    ap.add_argument("--batch", type=int, default=None, help="images per GPU per step (default: the config's per-GPU batch)")
    ap.add_argument("--full", action="store_true",
                    help="behind the timed region, also measure everything that is not the headline figure: the sequential rate, "
                         "the sustained rate, the per-kernel eager pass, the exact-fp32 route, the other configurations and "
                         "batches, the CPU baseline (default: set up, warm up, time the steps, print the result line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last step as DIR/<name>.npy (float32, <= 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-budget", type=float, default=60.0, help="seconds of CPU time the cpu_baseline leg may spend on its batched passes")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full without the legs behind the timed region (sustained run, exact-fp32 route, per-kernel eager pass, "
                         "other configurations)")
    ap.add_argument("--sustain-seconds", type=float, default=5.0, help="length of the sustained-rate leg after the timed region (--full)")
    ap.add_argument("--eager", action="store_true",
                    help="dispatch every launch eagerly instead of replaying the forward as a hipGraph (default: graph "
                         "segments + the roofline convolution and the bin head as eager, event-timed launches)")
    ap.add_argument("--inflight", type=int, default=3,
                    help="batches in flight per GPU: one hipGraph instance (own static input, own scratch) per slot, each "
                         "replayed on its own stream, slots taking the steps round-robin, so that the latency-bound launches "
                         "of one batch (token path, squeeze-excite, late 1x1 layers) run under the compute-bound ones of "
                         "another.  1 = strictly one step after the other")
    ap.add_argument("--leg-seconds", type=float, default=1.0,
                    help="length of each leg of configs_all / small_batch behind the timed region (--full, N = 1, skipped by --no-extras)")
    ap.add_argument("--stub-cpu", action="store_true", help=argparse.SUPPRESS)   # plumbing test only (gloo, no model)
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a.gpus, sys.argv[1:]))     # before any GPU call (and before torch is imported) here

    import torch
    import torch.distributed as dist
    from objcavit_amd import dp
    dev_type = "cpu" if a.stub_cpu else "cuda"
    if int(os.environ.get("WORLD_SIZE", "1")) != a.gpus:      # before the rendezvous: a wrong count must fail, not hang
        sys.exit(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={os.environ.get('WORLD_SIZE')} ranks")
    rank, local, world = dp.init_from_env(dev_type)
    device = torch.device("cpu") if a.stub_cpu else torch.device("cuda", local)
    torch.set_grad_enabled(False)
    if world > 1:
        # N ranks share the host: the seeded weight generator and torch's CPU copies (model build, before the first GPU call) would
        # otherwise run N x (all logical CPUs) threads on the job's CPU share -- 8 x 128 threads on a 16-CPU quota
        torch.set_num_threads(max(1, cpu_share() // world))
    launcher = "none (single process)" if world == 1 else \
        ("bench.py spawned the ranks itself" if os.environ.get("OCV_BENCH_LAUNCHER") == "self" else "external (torch.distributed.run)")

    wl = Workload(a.config, a.batch)
    B, H, W = wl.batch, wl.H, wl.W
    img_cpu = synthetic_images(B, 42 + rank, H, W)
    img = img_cpu.to(device)

    def barrier():
        if world > 1:
            dist.barrier()
        if not a.stub_cpu:
            torch.cuda.synchronize()

    launch_mode = "eager"
    island = f"conv3x3|{B},{wl.h},{wl.w},128,128"
    gt = box = None
    last_out = [None]                                  # the model output of the latest step (GPU path)
    if a.stub_cpu:
        # the slot bookkeeping of the pipelined mode (slots take the steps round-robin after the first ROOFLINE_STEPS) without a GPU
        work = [StubWorkload(B) for _ in range(max(1, a.inflight))]
        launch_mode = "stub"

        def step(first_id, slot=0):
            return work[slot].step(img, first_id)
    else:
        from objcavit_amd import hip_ops
        from objcavit_amd.validation import crop_box
        log(f"building model (config {wl.idx}, world={world}, cpus={len(os.sched_getaffinity(0))}, torch threads={torch.get_num_threads()})")
        model, sd, args = build_model(device, wl)
        log("model on device")
        # synthetic ground truth at the dataset's full resolution; metrics as the reference's validation step computes
        # them (metrics/MetricsPreprocess.py: resize the prediction to the ground truth, Eigen / Garg crop) -- one fused kernel
        gt = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(7 + rank)) * (0.9 * wl.max_depth) + 0.05 * wl.max_depth).to(device)
        box = crop_box(args, H, W)
        run = model
        slots, streams = [model], [torch.cuda.current_stream(device)]
        if not a.eager:
            from objcavit_amd.graph import GraphedGraphBins
            try:
                # capture = part of warm-up; each slot clones img as its graph's static input.  The longest launches of the
                # step -- the three direct 128 -> 128 3x3 convolutions at half resolution (second convolution of the last
                # decoder stage, the decoder's conv3, the heads' conv3x3) -- stay outside the graph as eager islands so that
                # they are timed live (with several batches in flight no side stream is forked, so the heads' convolution
                # can be an island too: the log line below lists all three).
                n = max(1, a.inflight)
                # (only slot 0 carries the islands: the event-timed steps run on it; the other slots replay the forward as a
                #  caller captures it, whole)
                # slot streams that do not share a hardware queue -- checked, not assumed (hip_ops.independent_streams: the runtime's
                # dealing of its GPU_MAX_HW_QUEUES queues put two of four consecutive streams on one: profiles/r06_stream_queues.txt)
                sts = hip_ops.independent_streams(n, device) if n > 1 else [None]
                slots = [GraphedGraphBins(model, img, eager_ops=(island,) if k == 0 else (), in_flight=n, stream=sts[k]) for k in range(n)]
                # a slot is replayed on the stream it was captured on: creating further streams can put two slots on
                # the same hardware queue (ROCm maps streams round-robin onto GPU_MAX_HW_QUEUES = 4 queues), which
                # serialises them -- measured: 781 instead of 840 img/s with the same code, depending on creation order
                streams = [g.stream for g in slots]
                run = slots[0]
                launch_mode = (f"hipGraph replay in {len(run.segments) - len(run.islands)} segments + {len(run.islands) + 1} eager, "
                               "event-timed launches (roofline convolutions, bin head) per step on slot 0"
                               + (f", the whole forward as captured on the other slots; {n} batches in flight (one graph instance + stream per slot, steps round-robin; the first "
                                  f"ROOFLINE_STEPS steps of the timed region run alone, which is where the event timings come from)"
                                  if n > 1 else ""))
                log(f"forward captured into {len(run.segments) - len(run.islands)} hipGraph segments x {n} slots "
                    f"({run.empty_segments_dropped} empty dropped), eager islands: {run.islands}")
            except Exception as e:                          # noqa: BLE001 -- reported in the JSON, never hidden
                launch_mode = f"eager (capture failed: {type(e).__name__}: {e})"
                log(f"hipGraph capture failed ({type(e).__name__}: {e}); falling back to eager dispatch")
                a.eager, run, slots, streams = True, model, [model], [torch.cuda.current_stream(device)]
                torch.cuda.synchronize()

        step_flags = []                                    # every step's taken range-guard word (device, 4 bytes): read once behind the timed region

        def step(first_id, slot=0):
            with torch.cuda.stream(streams[slot]):
                out = slots[slot](img)
                step_flags.append(getattr(slots[slot], "last_flag", None))
                last_out[0] = out                          # (--dump-outputs: the bin edges travel with the depth)
                return out.depth_pred, hip_ops.depth_metrics(out.depth_pred, gt, wl.min_depth, wl.max_depth, crop=box,
                                                             first_image_id=first_id)

    nslot = len(work) if a.stub_cpu else len(slots)
    slot_steps = [0] * nslot
    for i in range(a.warmup):
        for k in range(nslot):
            step(0, k)                                 # also warms the metric kernel (lazy code loading)
        barrier() if world == 1 else (None if a.stub_cpu else torch.cuda.synchronize())
        log(f"warm-up step {i} done")
    if world > 1:
        # warm-up of the job's ONE collective, same shape as the timed one: the first all-gather of a communicator sets up its
        # own channels (the barrier's all-reduce does not), which must not land inside a timed region of a few hundred ms
        warm = torch.zeros(a.steps * B, len(dp.RECORD_FIELDS), dtype=torch.float32, device=device if not a.stub_cpu else "cpu")
        warm[:, dp.RECORD_FIELDS.index("image_id")] = torch.arange(a.steps * B, dtype=torch.float32, device=warm.device) + rank * a.steps * B
        dp.gather_records(warm, world, n_total=world * a.steps * B)
    barrier()
    startup_s = time.perf_counter() - _T0              # process start -> model built, captured, warmed (per rank; min / max in the JSON)

    # With several batches in flight the first ROOFLINE_STEPS steps of the timed region run ALONE on slot 0 (the other
    # slots wait for them): their event pairs are the live kernel timings of the JSON; the remaining steps are pipelined
    # and carry no events (a launch bracketed on one stream while another stream shares the chip would time the sharing).
    ROOFLINE_STEPS = 1                                 # one step = three event-timed launches of the roofline convolution + one bin head
                                                       # (rounds 3 - 5 took two of twenty: every step that runs alone is 5 % slower than
                                                       # a pipelined one, and `value` is the whole timed region)
    if not a.stub_cpu:
        hip_ops.enable_timing(True)
    records = []
    depth = None
    t0 = time.perf_counter()
    for s_ in range(a.steps):
        first_id = (s_ * world + rank) * B
        if nslot == 1:
            slot = 0
        else:
            if s_ == ROOFLINE_STEPS and not a.stub_cpu:
                hip_ops.pause_timing(True)
                ev = torch.cuda.Event()
                ev.record(streams[0])
                for st_ in streams[1:]:
                    st_.wait_event(ev)
            slot = 0 if s_ < ROOFLINE_STEPS else s_ % nslot
        depth, rec = step(first_id, slot)
        slot_steps[slot] += 1
        records.append(rec)
    t_issue = time.perf_counter() - t0                 # host time to ISSUE the K steps (<< the steps' GPU time: not host-bound)
    if not a.stub_cpu:
        torch.cuda.synchronize()
        hip_ops.pause_timing(False)
    t_local = time.perf_counter() - t0                 # this rank's own steps (reported as per-rank min / max)
    table = dp.gather_records(torch.cat(records, 0), world, n_total=world * a.steps * B)      # the one collective of the job
    barrier()
    dt = time.perf_counter() - t0
    dumped = None
    if a.dump_outputs:
        # the last timed step's outputs, before anything behind the timed region replays the slots (this rank's shard)
        sfx = f"_rank{rank}" if world > 1 else ""
        outs = {"depth_pred" + sfx: depth, "metric_records" + sfx: records[-1]}
        if last_out[0] is not None:
            outs["bin_edges" + sfx] = last_out[0].bin_edges
        dumped = dump_outputs(a.dump_outputs, outs)
        log(f"outputs of the last timed step written to {a.dump_outputs}: {dumped}")
    timing = {}
    step_latency_ms = sequential_ips = sustained_ips = sustained_s = None
    exact = None
    if not a.stub_cpu:
        timing = hip_ops.timing_results()          # graph mode: only the eager islands + bin head carry events here
        # fp16 range guard: every replay took its word into the slot's last_flag on the device (one one-thread launch per step inside
        # the timed region); read here, behind it.  A tripped synthetic batch would mean the timed steps need the bf16 re-run.
        # EVERY timed step's word (take() zeroes the sticky flag per replay: the slots' last words alone would miss earlier trips)
        taken = [f for f in step_flags[-a.steps:] if f is not None]
        guard_tripped = int(torch.cat(taken).ne(0).sum()) if taken else 0
        del step_flags[:]
        log(f"timed region done: {dt / a.steps * 1e3:.1f} ms/step")
        default_depth = depth.clone()              # slot outputs are overwritten by the legs below
        if not a.eager:
            # launches inside the graph segments carry no events: their durations come from one eager pass right after
            # the timed region; the eager islands (roofline convolution, bin head) keep their LIVE measurements
            timed_steps = a.steps if nslot == 1 else ROOFLINE_STEPS
            live = {k: (v[0] / timed_steps * a.steps, v[1]) for k, v in timing.items()}
            hip_ops.enable_timing(False)
            if not a.full:
                timing = {}
            else:
                # one batch at a time: what a caller with a single forward in flight gets -- a capture of its own, made the way
                # such a caller makes it (in_flight = 1: the lone-batch side streams on where the hardware-queue count allows), on slot 0's stream
                seq_step = lambda: step(0, 0)
                if nslot > 1:
                    from objcavit_amd.graph import GraphedGraphBins
                    lone = GraphedGraphBins(model, img, in_flight=1)

                    def seq_step():
                        with torch.cuda.stream(lone.stream):
                            out = lone(img)
                            return out.depth_pred, hip_ops.depth_metrics(out.depth_pred, gt, wl.min_depth, wl.max_depth, crop=box, first_image_id=0)
                    for _ in range(2):
                        seq_step()
                    torch.cuda.synchronize()
                t1 = time.perf_counter()
                seq_step()
                torch.cuda.synchronize()
                step_latency_ms = (time.perf_counter() - t1) * 1e3          # one batch alone, submit -> metrics record
                nseq = max(4, a.steps)                                       # reference: the same steps strictly one after the other
                t1 = time.perf_counter()
                for _ in range(nseq):
                    seq_step()
                torch.cuda.synchronize()
                sequential_ips = nseq * B / (time.perf_counter() - t1)
                if nslot > 1:
                    del lone
                if not a.no_extras:
                    # sustained rate: the timed region above is a fraction of a second on a cold part; here the same pipelined
                    # steps run for >= sustain_seconds (the chip settles at its power-capped clock: profiles/r02_power_probe.txt)
                    per_round = max(nslot, int(0.25 / max(dt / a.steps, 1e-4)) // nslot * nslot)
                    t1 = time.perf_counter()
                    n_sus = 0
                    while time.perf_counter() - t1 < a.sustain_seconds:
                        for k in range(per_round):
                            step(0, k % nslot)
                        torch.cuda.synchronize()
                        n_sus += per_round
                    sustained_s = time.perf_counter() - t1
                    sustained_ips = n_sus * B / sustained_s
                    log(f"sustained leg: {n_sus} steps in {sustained_s:.2f} s = {sustained_ips:.1f} img/s")
                    # per-kernel table: one stream (a launch bracketed while a side stream shares the chip would time the sharing)
                    saved = {"OCV_FORKS": os.environ.get("OCV_FORKS")}
                    os.environ["OCV_FORKS"] = "0"
                    try:
                        for _ in range(2):
                            model(img)                       # (scratch of the one-stream order: allocated outside the timed pass)
                        torch.cuda.synchronize()
                        hip_ops.enable_timing(True)
                        for _ in range(3):
                            model(img)
                    finally:
                        for k, v in saved.items():
                            if v is None:
                                os.environ.pop(k, None)
                            else:
                                os.environ[k] = v
                    extra = hip_ops.timing_results()
                    timing = {k: (v[0] / 3 * a.steps, v[1]) for k, v in extra.items()}
                else:
                    timing = {}
            timing.update(live)
        hip_ops.enable_timing(False)
        if a.full and world == 1 and not a.no_extras:
            log("exact-fp32 route ...")
            ips, exact_depth, rel = exact_fp32_pass(device, wl, img, gt, box, B, default_depth)
            exact = dict(images_per_s=round(ips, 1), depth=exact_depth, max_rel_vs_default_route=rel)
            log(f"exact-fp32 route: {ips:.1f} img/s, max rel vs default route {rel:.2e}")
        legs = None
        if a.full and world == 1 and not a.no_extras and not a.eager and a.config == 2 and a.batch is None:
            # Every other BASELINE configuration and the reference's own batch sizes, on the driver's clock:
            # configs[1] / [3] / [4] with this run's --inflight, configs[2] at bs 1 and bs 2 (= image + mirror) one step at a time
            # and at bs 16 one step at a time.  ~leg-seconds each + a capture; slots of the timed region are released first.
            del slots, run
            torch.cuda.empty_cache()
            legs = {"configs_all": {}, "small_batch": {}}
            for c in (1, 3, 4):
                wl_c = Workload(c)
                if c == 1:                                    # same network as configs[2]: other objects only
                    from objcavit_amd.modules.GraphBins import SyntheticObjectProvider
                    m_c, keep = model, model.object_provider
                    model.object_provider = SyntheticObjectProvider(wl_c.n_obj, wl_c.language, seed=42)
                else:
                    m_c, keep = build_model(device, wl_c)[0], None
                legs["configs_all"][f"configs[{c}]"] = side_leg(device, wl_c, m_c, max(1, a.inflight), a.leg_seconds)
                if keep is not None:
                    model.object_provider = keep
                else:
                    del m_c
                    torch.cuda.empty_cache()
                log(f"configs[{c}]: {legs['configs_all'][f'configs[{c}]']['images_per_s']} img/s")
            # the reference's do_final_upscale models (51 of its 108 params files; modules/GraphBins.py:45, modules/AdaBins.py:43): features,
            # tokens and depth at FULL resolution -- configs[2] with that one switch, same objects, same weights' seed
            wl_f = Workload(2)
            wl_f.kw = dict(wl_f.kw, do_final_upscale=True)
            m_f = build_model(device, wl_f)[0]
            legs["configs_all"]["configs[2] + do_final_upscale"] = side_leg(device, wl_f, m_f, max(1, a.inflight), a.leg_seconds)
            log(f"configs[2] + do_final_upscale: {legs['configs_all']['configs[2] + do_final_upscale']['images_per_s']} img/s")
            del m_f
            torch.cuda.empty_cache()
            for b in (1, 2, 16):
                legs["small_batch"][f"bs{b}_one_at_a_time"] = side_leg(device, Workload(2, b), model, 1, a.leg_seconds)
                log(f"configs[2] bs {b} one at a time: {legs['small_batch'][f'bs{b}_one_at_a_time']['images_per_s']} img/s")
            # ... and with four steps in flight, the form that hides the launch latency of the reference's bs-1 loop: plain forwards
            # (bs 1 / bs 2 = image + mirror, four graph slots), then the product's own driver of that loop, PipelinedValidation
            for b in (1, 2):
                legs["small_batch"][f"bs{b}_inflight4"] = side_leg(device, Workload(2, b), model, 4, a.leg_seconds)
                log(f"configs[2] bs {b}, four in flight: {legs['small_batch'][f'bs{b}_inflight4']['images_per_s']} img/s")
            legs["small_batch"]["pipelined_validation_bs1_slots4"] = pipelined_validation_leg(device, Workload(2, 1), model, 4, a.leg_seconds)
            log(f"PipelinedValidation bs 1 (image + mirror per step), four slots: "
                f"{legs['small_batch']['pipelined_validation_bs1_slots4']['images_per_s']} validated img/s")
        depth = default_depth

    # max over ranks of the job time; ranks RCCL / gloo actually saw; per-rank rates
    ranks_seen, rank_rates, rank_startup = 1, [a.steps * B / t_local], [startup_s]
    if world > 1:
        st = torch.zeros(world, dtype=torch.float64, device=device)
        dist.all_gather_into_tensor(st, torch.tensor([startup_s], dtype=torch.float64, device=device))
        rank_startup = st.tolist()
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        ones = torch.ones(1, dtype=torch.float64, device=device)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)
        ranks_seen = int(ones.item())
        rates = torch.zeros(world, dtype=torch.float64, device=device)
        dist.all_gather_into_tensor(rates, torch.tensor([a.steps * B / t_local], dtype=torch.float64, device=device))
        rank_rates = rates.tolist()

    if rank == 0:
        ids = table[:, dp.RECORD_FIELDS.index("image_id")].cpu().long().tolist()
        assert table.shape[0] == world * a.steps * B and sorted(ids) == list(range(world * a.steps * B)), "gathered table incomplete"
        assert ranks_seen == world
        value = round(world * a.steps * B / dt, 3)
        inflight_note = f"{nslot} batches of {B} in flight per GPU" if nslot > 1 else "one batch at a time"
        res = {
            "metric": f"images/sec ({W}x{H}, bs={B}) forward depth inference, {inflight_note}; AbsRel vs CPU ref",
            "value": value, "unit": "images/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "full": a.full,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "stub" if a.stub_cpu else "f32 (fp16 / bf16 split contractions)",
            "data": "stub" if a.stub_cpu else "synthetic",
            # like-for-like with round 1 and with a caller that submits one batch at a time: value_sequential;
            # `value` is the timed region as the driver clocks it (= value_pipelined when inflight > 1)
            "value_pipelined": value if nslot > 1 else None,
            "value_sequential": (None if sequential_ips is None else round(sequential_ips * world, 1)) if nslot > 1 else value,
            "sustained_images_per_s": None if sustained_ips is None else round(sustained_ips * world, 1),
            "sustained_seconds": None if sustained_s is None else round(sustained_s, 2),
            "launch": launch_mode.replace("ROOFLINE_STEPS", str(ROOFLINE_STEPS)), "inflight": nslot, "launcher": launcher,
            "slot_steps": slot_steps,                 # timed steps each slot of THIS rank served (first ROOFLINE_STEPS on slot 0, then round-robin)
            # host threads per rank: the main thread issues every launch (one Python thread per process, captures serialised by
            # graph._CAPTURE_LOCK); torch's intra-op pool is not used by the hot path (no CPU tensor math in a step) -- a rank
            # needs ONE busy CPU while it issues and idles in synchronize(); 8 ranks fit the 16-CPU quota of the driver's box
            "host_threads": {"issuing": 1, "torch_intra_op": torch.get_num_threads(), "cpus_allowed": len(os.sched_getaffinity(0))},
            "ranks_seen": ranks_seen, "host_issue_ms_per_step": round(t_issue / a.steps * 1e3, 3),
            "step_latency_ms": None if step_latency_ms is None else round(step_latency_ms, 3),
            "sequential_images_per_s_this_rank": None if sequential_ips is None else round(sequential_ips, 1),
            "per_rank_images_per_s": {"min": round(min(rank_rates), 2), "max": round(max(rank_rates), 2)},
            # process start -> ready for the timed region (imports, rendezvous, seeded weights, capture, warm-up), per rank
            "per_rank_startup_s": {"min": round(min(rank_startup), 2), "max": round(max(rank_startup), 2)},
            "config": {"workload": f"BASELINE configs[{wl.idx}]: {wl.desc}, bs={B} per GPU; seeded random weights with the "
                                   f"parity tests' gains on attention / bin-head layers (gen.{'PEAKY' if wl.gains_name == 'PEAKY' else 'KITTI_GAINS'}: "
                                   "a non-degenerate bin softmax, SURVEY Q12) -- no trained checkpoint exists offline",
                       "baseline_config": wl.idx, "global_batch": world * B, "image": [H, W], "objects_per_image": wl.n_obj,
                       "tokens": wl.S, "sa_ca_stacks": wl.stacks, "parallelism": f"dp{world}",
                       # the like-for-like rates travel inside `config` too (the driver's parsed line keeps it): `value` is
                       # `inflight` batches overlapped on the chip, value_sequential one batch after the other
                       "inflight": nslot, "value_pipelined": value if nslot > 1 else None,
                       "value_sequential": (None if sequential_ips is None else round(sequential_ips * world, 1)) if nslot > 1 else value},
            "metrics_gathered": dp.summarise(table),
        }
        if dumped is not None:
            res["outputs_dumped"] = {"dir": a.dump_outputs, "arrays": dumped}
        if not a.stub_cpu:
            res["dtype_note"] = ("fp32 results; the decoder's / heads' 3x3, tap-GEMM and 16x16-patch convolutions run as two-term FP16 splits "
                                 "(round 4: hi*hi + hi*lo + lo*hi on v_mfma_*_f16, fp32 accumulate, product error <= 2^-22; weights scaled per "
                                 "output channel by a power of two, activations range-checked on the first batch, bf16 pairs as the REPORTED "
                                 "fallback: conv_split); the encoder's 1x1 convolutions as two-term bf16 splits (2^-17); the first convolution "
                                 "of every decoder stage at the low resolution = an exact re-association; the 30x40 and 60x80 second convolutions in Winograd "
                                 "F(4x4,3x3) form with fp32 transforms, per-tile scaled two-term fp16 products, same parity bar); layer 0's projection of each transformer stack as a "
                                 "three-term bf16 split (six products, dropped terms <= 2^-24: fp32-faithful); the layers' projections and "
                                 "feed-forward blocks, the attention cores (QK^T, PV), the image <- object cross-attention and the bin head as a two-term fp16 split with a "
                                 "scaled low term (x = hi + 2^-11 lo', three v_mfma_*_f16 per product block: 22-bit products = the error of "
                                 "an fp32 FMA chain); depthwise and squeeze-excite on exact fp32 FMA.  exact_fp32_* = the same workload with "
                                 "every contraction on exact-fp32 arithmetic (" + " ".join(f"{k}={v}" for k, v in EXACT_ENV.items()) + ")")
            from objcavit_amd import hip_ops as _ops
            dec = model.dense_feature_extractor.decoder
            fmode = dec.__dict__.get("_f16_modes", {}).get(dec._wkey())
            split_f16 = bool(fmode[1]) if fmode else _ops.conv_split_f16()
            res["conv_split"] = {"pairs": "fp16" if split_f16 else "bf16",
                                 # the decoder measured its activations' range on its first eager batch (host syncs, that call only)
                                 "fp16_range_first_batch": (fmode[2] if fmode and len(fmode) > 2 else None),
                                 "route_report": dict(_ops.ROUTE_REPORT),
                                 # sticky device word ORed by every fp16-pair producer, taken per replay (hip_ops.RangeGuard)
                                 "fp16_range_guard_tripped_steps": guard_tripped}
            res.update(kernel_report(timing, a, B, wl, split_f16))
            if legs is not None:
                res.update(legs)
            if exact is not None:
                res["exact_fp32_images_per_s"] = exact["images_per_s"]
                res["exact_fp32_max_rel_vs_default_route"] = exact["max_rel_vs_default_route"]
            if a.full and world == 1 and not a.no_cpu_baseline:
                feats, boxes, _ = model.object_provider(img)
                log("cpu baseline ...")
                cb, absrel, maxrel = cpu_baseline(sd, img_cpu, feats, boxes, depth, wl, budget_s=a.cpu_budget)
                res["cpu_baseline"] = cb
                res["abs_rel_vs_cpu"] = absrel
                res["max_rel_vs_cpu"] = maxrel
                res["speedup_vs_cpu"] = round(res["value"] / cb["value"], 1)
                if res["value_sequential"]:
                    res["speedup_vs_cpu_sequential"] = round(res["value_sequential"] / cb["value"], 1)
                if exact is not None:
                    from oracle import restate
                    ref, _ = restate.graphbins_forward(img_cpu[:1], [feats[0].cpu()], [boxes[0].cpu()], sd, wl.min_depth, wl.max_depth, **wl.kw)
                    res["exact_fp32_max_rel_vs_cpu"] = float(((exact["depth"][:1].cpu() - ref).abs() / ref).max())
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
