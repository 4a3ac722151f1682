"""Throughput of the EfficientNet-B1 / V2-S / V2-M models and of the strided 3x3 kernel (not bench.py).

    python tools/bench_encoders.py models      images/s of B1, V2-S, V2-M AdaBins and V2-M GraphBins, 480 x 640, bs 16 and bs 1
                                               (eager forward, HIP events, seeded weights; JSON line per case)
    python tools/bench_encoders.py kernels     ocv_conv3x3_nhwc_strided_fwd at stride 2 and 1 beside the stride-1 kernel
                                               (ocv_conv_nhwc_fwd) at the same widths, bs 16: ms, algorithmic TF/s, strided /
                                               stride-1 time per FLOP
    python tools/bench_encoders.py trace       two V2-M GraphBins bs-16 forwards (run under rocprofv3 --kernel-trace --stats);
                                               the encoder window is bracketed by two one-element add kernels
Every line printed is JSON (``{"kind": ...}``)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import gen           # noqa: E402
from objcavit_amd import hip_ops                      # noqa: E402
from objcavit_amd.config import make_args            # noqa: E402

torch.set_grad_enabled(False)
H, W = 480, 640


def _model(kind, enc):
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    if kind == "adabins":
        m = AdaBins(make_args(model="adabins", encoder_name=enc, dimensions_train=[H, W], dimensions_test=[H, W]))
    else:
        args = make_args(strategy="learned", language="clip", encoder_name=enc, dimensions_train=[H, W], dimensions_test=[H, W])
        m = GraphBins(args, object_provider=SyntheticObjectProvider(32, "clip", seed=3))
    gen.load_into(m.eval(), 7, gen.PEAKY)
    return m.cuda()


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def models():
    for kind, enc in (("adabins", "efficientnet-b1"), ("adabins", "efficientnet-v2-s"), ("adabins", "efficientnet-v2-m"),
                      ("graphbins", "efficientnet-v2-m"), ("adabins", "efficientnet-b5")):
        m = _model(kind, enc)
        for B in (16, 1):
            img = gen.randn("img", (B, 3, H, W), 1).cuda()
            ms = _time(lambda: m(img), 10 if B == 16 else 30)
            enc_ms = _time(lambda: m.dense_feature_extractor.encoder(img), 10 if B == 16 else 30)
            print(json.dumps(dict(kind="model", model=kind, encoder=enc, batch=B, ms=round(ms, 3), images_per_s=round(B * 1e3 / ms, 1),
                                  encoder_ms=round(enc_ms, 3))), flush=True)
        del m
        torch.cuda.empty_cache()


# (Cin, Cout, H, W of the INPUT): the Fused-MBConv 3x3 layers of V2-S / V2-M at 480 x 640
KERNEL_SHAPES = ((24, 24, 240, 320), (24, 96, 240, 320), (48, 192, 120, 160), (64, 256, 60, 80), (80, 320, 60, 80))


def kernels(B=16, reps=50):
    cl = torch.channels_last
    for cin, cout, h, w in KERNEL_SHAPES:
        x = torch.randn(B, cin, h, w, device="cuda").contiguous(memory_format=cl)
        wt = torch.randn(cout, cin, 3, 3, device="cuda") / np.sqrt(9 * cin)
        bias = torch.zeros(cout, device="cuda")
        hi, lo = hip_ops.prep_conv_weight(wt)
        rows = []
        for tag, fn, ho, wo in (
                ("stride1_igemm", lambda: hip_ops.conv_nhwc(x, None, hi, lo, bias, 3, hip_ops.ACT_SILU), h, w),
                ("strided_s1", lambda: hip_ops.conv3x3_strided(x, hi, lo, bias, 1, (1, 1), hip_ops.ACT_SILU), h, w),
                ("strided_s2", lambda: hip_ops.conv3x3_strided(x, hi, lo, bias, 2, (1, 1), hip_ops.ACT_SILU), h // 2, w // 2)):
            ms = _time(fn, reps)
            flop = 2.0 * B * ho * wo * cout * cin * 9
            issued = 2.0 * B * ho * wo * (-(-cout // 128) * 128) * (-(-cin // 32) * 32) * 9 * 3      # MFMA work the tiles issue
            rows.append(dict(form=tag, ms=round(ms, 4), alg_TFLOPs=round(flop / ms / 1e9, 1), ns_per_MFLOP=round(ms * 1e6 / (flop / 1e6), 3),
                             issued_frac_useful=round(flop * 3 / issued, 3)))
        base = rows[0]["ns_per_MFLOP"]
        for r in rows:
            r["per_flop_vs_stride1_igemm"] = round(r["ns_per_MFLOP"] / base, 3)
        print(json.dumps(dict(kind="conv3x3", batch=B, cin=cin, cout=cout, h=h, w=w, forms=rows)), flush=True)


def trace():
    m = _model("graphbins", "efficientnet-v2-m")
    img = gen.randn("img", (16, 3, H, W), 1).cuda()
    mark = torch.zeros(1, device="cuda")
    m(img)                                           # warm-up: weight folding, workspace
    torch.cuda.synchronize()
    for _ in range(2):
        mark.add_(1)                                 # encoder window opens (one elementwise kernel)
        m.dense_feature_extractor.encoder(img)
        mark.add_(1)                                 # closes
        m(img)
    torch.cuda.synchronize()
    print(json.dumps(dict(kind="trace", note="encoder windows bracketed by elementwise add kernels")), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "models"
    if what == "kernels" and len(sys.argv) > 2:
        kernels(reps=int(sys.argv[2]))                # few repetitions: under rocprofv3 --pmc
    else:
        {"models": models, "kernels": kernels, "trace": trace}[what]()
