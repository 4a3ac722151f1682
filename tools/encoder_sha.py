"""SHA-1 of every output of the MBConv / encoder family (csrc/stem.hip, depthwise.hip, encoder_nhwc.hip, pointwise_split.hip,
pointwise_hl.hip, depthwise_se.hip, se_gate.hip, mbconv_fused.hip) on fixed seeded operands, one line per case, so that two library
builds (OCV_LIB_PATH) can be compared bit for bit from their logs -- run once per build, in a process of its own:

    python tools/encoder_sha.py > new.log;  OCV_LIB_PATH=objcavit_amd/lib/variants/parent.so python tools/encoder_sha.py > parent.log

Cases: the encoder rows of tests/test_hip_memory_bounds.py (the smallest shapes at which these kernels can go wrong) -- the 1 x 1
convolutions on PW_SHAPES as exact fp32, split (gate + residual, with the split copy, SiLU), through the first-ABI entry points and
under every pinned pointwise_hl tile; split-K across workgroups; the depthwise kernels on DW_SHAPES x k {3, 5} x stride {1, 2},
plain (NCHW and NHWC) and with the squeeze-excite gate under both dispatch modes; depthwise -> gate folded into per-image packed
weights -> project (the packed weights included); fused expand + depthwise; channel mean + gate from the mean (R 2, 6 and 24); the stem -- and
ocv_se_gate_partials_fwd on each side of its dispatch, fed from a (2, C, 33, 47) depthwise: one launch (C 96, R 8), two because
of R (96, 65), two because of C (1540, 8), and one row group per pooling pass (4096, 4).  The last line is a SHA-1 over all the others.
"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from objcavit_amd import hip_ops as ops

lib = ops._lib.load()
CL = torch.channels_last
lines = []


def rnd(seed, shape, scale=1.0):
    return scale * torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def cl(seed, shape, scale=1.0):
    return rnd(seed, shape, scale).contiguous(memory_format=CL)


def sha(t):
    if t is None:
        return "-" * 12
    t = (t.hl if hasattr(t, "hl") else t).contiguous()
    return hashlib.sha1(t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().tobytes()).hexdigest()[:12]


def note(name, *outs):
    torch.cuda.synchronize()
    lines.append(f"{name:<72s} " + " ".join(sha(o) for o in outs))
    print(lines[-1], flush=True)


def ok(rc):
    assert rc == 0, lib.ocv_last_error().decode(errors="replace")


def st():
    return torch.cuda.current_stream().cuda_stream


def se_params(C, R, seed=20):
    return (rnd(seed, (R, C), C ** -0.5), rnd(seed + 1, (R,), 0.3), rnd(seed + 2, (C, R), R ** -0.5).t().contiguous(), rnd(seed + 3, (C,), 0.3))


# ---- 1 x 1 convolutions
for shape in [(3, 5, 7, 40, 24), (3, 5, 7, 240, 40)]:
    B, H, W, Cin, Cout = shape
    x, w, b = cl(1, (B, Cin, H, W)), rnd(2, (Cout, Cin), Cin ** -0.5), rnd(3, (Cout,), 0.2)
    g, r = torch.sigmoid(rnd(4, (B, Cin))), cl(5, (B, Cout, H, W))
    sw = ops.SplitWeight(w)
    note(f"pointwise_nhwc|fp32|{shape}", ops.pointwise_nhwc(x, w, b, 0, gate=g, residual=r))
    note(f"pointwise_nhwc|split|{shape}", ops.pointwise_nhwc(x, sw, b, 0, gate=g, residual=r),
         *ops.pointwise_nhwc(x, sw, b, 0, gate=g, residual=r, out_split=True), ops.pointwise_nhwc(x, sw, b, 3))
    M = B * H * W
    y = torch.full((B, Cout, H, W), float("nan"), device="cuda").contiguous(memory_format=CL)
    ok(lib.ocv_pointwise_conv_nhwc_split_fwd(x.data_ptr(), g.data_ptr(), H * W, sw.packed.data_ptr(), b.data_ptr(), r.data_ptr(),
                                             y.data_ptr(), M, Cin, Cout, 0, st()))
    y2 = torch.full((B, Cout, H, W), float("nan"), device="cuda").contiguous(memory_format=CL)
    ys = ops.SplitAct.empty(B, Cout, H, W, "cuda")
    ok(lib.ocv_pointwise_conv_nhwc_split_hl_fwd(x.data_ptr(), g.data_ptr(), H * W, sw.packed.data_ptr(), b.data_ptr(), r.data_ptr(),
                                                y2.data_ptr(), ys.hl.data_ptr(), M, Cin, Cout, 0, st()))
    note(f"pointwise_nhwc|first-ABI entry points|{shape}", y, y2, ys)
    xs = ops.split_act(x)
    for cfg in [(0, 0), (1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2)]:
        ok(lib.ocv_pointwise_hl_set_dispatch(*cfg))
        try:
            both = ops.pointwise_hl(xs, sw, b, 0, residual=r, out_fp32=True, out_split=True)
            only = ops.pointwise_hl(xs, sw, b, 3, out_fp32=False, out_split=True)
        finally:
            ok(lib.ocv_pointwise_hl_set_dispatch(0, 0))
        note(f"pointwise_hl|{shape}|cfg{cfg}", *both, only)

B, H, W, Cin, Cout = 1, 5, 7, 1040, 40
assert lib.ocv_pointwise_split_workspace_bytes(B * H * W, Cin, Cout) > 0
x, sw, b = cl(1, (B, Cin, H, W)), ops.SplitWeight(rnd(2, (Cout, Cin), Cin ** -0.5)), rnd(3, (Cout,), 0.2)
note("pointwise_nhwc|split-K across workgroups", ops.pointwise_nhwc(x, sw, b, 0, gate=torch.sigmoid(rnd(4, (B, Cin))), residual=cl(5, (B, Cout, H, W))),
     ops.pointwise_nhwc(x, sw, b, 3))

# ---- depthwise, plain and with the squeeze-excite gate
for shape in [(3, 12, 33, 47), (1, 4, 1, 1)]:
    B, C, H, W = shape
    R = max(1, C // 3)
    for k in (3, 5):
        x, w, b = rnd(1, shape), rnd(2, (C, 1, k, k), 0.3), rnd(3, (C,), 0.2)
        xc, wkc = x.contiguous(memory_format=CL), w.flatten(1).t().contiguous()
        for s in (1, 2):
            note(f"depthwise|{shape}|k{k}s{s}", ops.depthwise_conv_same(x, w, b, s, 3), ops.depthwise_nhwc_same(xc, wkc, b, k, s, 3))
            for mode in (1, 2):
                ok(lib.ocv_depthwise_set_dispatch(mode))
                try:
                    out = ops.depthwise_se_gate(xc, wkc, b, k, s, *se_params(C, R))
                finally:
                    ok(lib.ocv_depthwise_set_dispatch(0))
                note(f"depthwise_se_gate|{shape}|k{k}s{s}|{'window' if mode == 1 else 'lds-rows'}", *out)

k, s, B, C, H, W, R, N = 5, 2, 2, 96, 13, 17, 4, 24
args = (cl(1, (B, C, H, W)), rnd(2, (k * k, C), 0.3), rnd(3, (C,), 0.2), k, s, *se_params(C, R))
y32, g32 = ops.depthwise_se_gate(*args)
ys, wg, gate = ops.depthwise_se_gate_weights(*args, rnd(8, (N, C), C ** -0.5), want_gate=True)
Ho, Wo = y32.shape[2:]
note("depthwise_hl_gate_weights_project", y32, g32, ys, gate, wg.packed,
     *ops.pointwise_hl(ys, wg, rnd(9, (N,), 0.2), 0, residual=cl(10, (B, N, Ho, Wo)), out_fp32=True, out_split=True))

# ---- fused expand + depthwise
B, H, W, Cin, mid = 2, 17, 23, 24, 144
x, we, be = cl(1, (B, Cin, H, W)), ops.SplitWeight(rnd(2, (mid, Cin), Cin ** -0.5)), rnd(3, (mid,), 0.3)
for k in (3, 5):
    for s in (1, 2):
        note(f"expand_depthwise_fused|k{k}s{s}", *ops.expand_depthwise_se_gate(x, we, be, rnd(4, (k * k, mid), 0.3), rnd(5, (mid,), 0.2), k, s,
                                                                               *se_params(mid, Cin // 4)))

# ---- channel mean and the gate from it
for (B, C, H, W, R) in [(1, 8, 1, 3, 2), (2, 144, 60, 80, 6), (2, 64, 5, 7, 24)]:      # R 24: the gate dot's 16-wide loop and its tail
    x = cl(1, (B, C, H, W))
    note(f"channel_mean_and_se_gate|{(B, C, H, W, R)}", ops.channel_mean_nhwc(x), ops.se_gate(x, *se_params(C, R)))

# ---- stem
note("stem_conv_same", ops.stem_conv_same(rnd(1, (1, 3, 33, 47)), rnd(2, (48, 3, 3, 3), 0.3), rnd(3, (48,), 0.2), 2, 3))

# ---- ocv_se_gate_partials_fwd on each side of its dispatch
for tag, C, R in (("one launch", 96, 8), ("two launches because of R", 96, 65), ("two launches because of C", 1540, 8), ("one row group per pass", 4096, 4)):
    y, g = ops.depthwise_se_gate(cl(1, (2, C, 33, 47)), rnd(2, (9, C), 0.3), rnd(3, (C,), 0.2), 3, 1, *se_params(C, R))
    note(f"se_gate_partials|{tag}|C{C} R{R}|{lib.ocv_depthwise_sum_tiles(2, C, 33, 47, 3, 1)} partial rows", y, g)

print(f"{len(lines)} cases  sha1 of all lines {hashlib.sha1(chr(10).join(lines).encode()).hexdigest()}  [{os.environ.get('OCV_LIB_PATH', 'product build')}]")
