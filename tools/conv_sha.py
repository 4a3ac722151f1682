"""SHA-1 of every output of the split-operand convolution family (csrc/conv_igemm.hip, conv_dma.hip, conv_winograd.hip and the
split patch embedding of patch_embed.hip) on fixed operands, one line per case, so that two library builds (OCV_LIB_PATH) can be
compared bit for bit from their logs -- run once per build, in a process of its own:

    python tools/conv_sha.py > new.log;  OCV_LIB_PATH=objcavit_amd/lib/variants/parent.so python tools/conv_sha.py > parent.log

Cases: the convolution rows of tests/test_hip_memory_bounds.py (dense k 1 and 3, halo forced, split-K, packed taps, Winograd,
strided, split patch embedding), the six shapes of tests/test_hip_conv_halo.py under both dispatch modes, and the ragged
element-wise row of tests/test_hip_kernels.py; each as bf16 and fp16 pairs, "plain" (no bias, activation, residual: fp32 output
alone) and "full" (scale, bias, LeakyReLU, residual where the entry point takes one, fp32 and split output).  The last line is a
SHA-1 over all the others.
"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from objcavit_amd import hip_ops as ops

lib = ops._lib.load()
CL = torch.channels_last
LEAKY = ops.ACT_LEAKY_RELU
lines = []


def rnd(seed, shape, scale=1.0):
    return scale * torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def sha(t):
    if t is None:
        return "-" * 12
    t = t.hl if hasattr(t, "hl") else t
    t = t.contiguous()
    return hashlib.sha1(t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().tobytes()).hexdigest()[:12]


def note(name, *outs):
    torch.cuda.synchronize()
    lines.append(f"{name:<64s} " + " ".join(sha(o) for o in outs))
    print(lines[-1], flush=True)


def p(t):
    return None if t is None else t.data_ptr()


def dense(tag, B, H, W, Cin, Cout, k, f16, full, mode=0, packed=False, ws=False):
    """ocv_conv_nhwc_split_x_fwd / ocv_conv3x3_split_packed_taps_fwd through the C ABI (the wrappers pass no residual)."""
    x = ops.split_act(rnd(1, (B, Cin, H, W)).contiguous(memory_format=CL), f16=f16)
    w = rnd(2, (Cout, Cin, k, k), 1.0 / (k * Cin ** 0.5))
    prep = (ops.prep_conv_weight_packed_taps if packed else ops.prep_conv_weight)(w, f16=f16)
    osc = prep[2] if f16 else (torch.exp2(torch.arange(Cout, device="cuda") % 3 - 1.0).float() if full else None)
    bias, res = (rnd(3, (Cout,), 0.3), rnd(4, (B, H, W, Cout))) if full else (None, None)
    y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    ys = ops.SplitAct.empty(B, Cout, H, W, "cuda", f16=f16) if full else None
    if ys is not None:
        ys.hl.view(torch.int16).fill_(0x7E7E)
    st = torch.cuda.current_stream().cuda_stream
    head = (x.hl.data_ptr(), Cin, prep[0].data_ptr(), prep[1].data_ptr(), p(osc), int(f16), p(bias), p(res), y.data_ptr(),
            None if ys is None else ys.hl.data_ptr(), B, H, W, Cout)
    assert lib.ocv_conv3x3_set_dispatch(mode) == 0
    try:
        if packed:
            rc = lib.ocv_conv3x3_split_packed_taps_fwd(*head, LEAKY if full else 0, st)
        else:
            nws = int(lib.ocv_conv_nhwc_split_workspace_bytes(B, H, W, Cin, Cout, k)) if ws else 0
            assert bool(nws) == ws
            wsb = torch.empty(max(nws, 4) // 4, device="cuda") if ws else None
            rc = lib.ocv_conv_nhwc_split_x_fwd(*head, k, LEAKY if full else 0, p(wsb), nws, st)
    finally:
        lib.ocv_conv3x3_set_dispatch(0)
    assert rc == 0, lib.ocv_last_error().decode(errors="replace")
    kern = ("-", "ring", "halo")[lib.ocv_conv3x3_last_kernel()] if k == 3 and not packed else "-"
    note(f"{tag}|{(B, H, W, Cin, Cout)}|k{k}|{'f16' if f16 else 'bf16'}|{'full' if full else 'plain'}|{kern}", y, ys)


for f16 in (False, True):
    for full in (False, True):
        for shape in [(1, 9, 33, 40, 72), (3, 5, 7, 32, 40)]:
            for k in (1, 3):
                dense("dense", *shape, k, f16, full, mode=1)
                # the fp32-input kernel on the same sizes: one source, and the virtual concat where Cin > 32
                B, H, W, Cin, Cout = shape
                x = rnd(1, (B, Cin, H, W)).contiguous(memory_format=CL)
                hi, lo = ops.prep_conv_weight(rnd(2, (Cout, Cin, k, k), 1.0 / (k * Cin ** 0.5)))
                two = full and Cin > 32
                y = ops.conv_nhwc(x[:, :32].contiguous(memory_format=CL) if two else x, x[:, 32:].contiguous(memory_format=CL) if two else None,
                                  hi, lo, rnd(3, (Cout,), 0.3) if full else None, k, LEAKY if full else 0,
                                  residual=rnd(4, (B, Cout, H, W)).contiguous(memory_format=CL) if full else None)
                note(f"igemm|{shape}|k{k}|{'full' if full else 'plain'}", y)
        dense("halo-forced", 2, 16, 64, 40, 136, 3, f16, full, mode=2)
        dense("split-K", 1, 45, 183, 456, 1032, 3, f16, full, ws=True)
        dense("packed-taps", 1, 9, 33, 40, 72, 3, f16, full, packed=True)
        dense("ragged-elementwise", 1, 9, 33, 40, 12, 1, f16, full, mode=1)
        dense("ragged-elementwise", 1, 9, 33, 40, 12, 3, f16, full, mode=1)
        for shape in [(1, 8, 32, 32, 128), (1, 16, 64, 64, 128), (2, 8, 32, 96, 128), (2, 8, 32, 40, 8), (1, 16, 64, 32, 12), (2, 16, 64, 64, 136)]:
            for mode in (1, 2):
                dense(f"halo-test-mode{mode}", *shape, 3, f16, full, mode=mode)
        # Winograd F(4x4, 3x3): the split input's element type is f16; the transformed filters are always fp16 pairs
        B, H, W, Cin, Cout = 1, 7, 9, 40, 72
        xs = ops.split_act(rnd(1, (B, Cin, H, W)).contiguous(memory_format=CL), f16=f16)
        u_hi, u_lo, fs, cs = ops.prep_winograd43_weight(rnd(2, (Cout, Cin, 3, 3), 1.0 / (3 * Cin ** 0.5)))
        got = ops.conv3x3_winograd43_split(xs, u_hi, u_lo, fs, rnd(3, (Cout,), 0.3) if full else None, LEAKY if full else 0,
                                           out_fp32=True, out_split=full, cscale=cs)
        note(f"winograd43|{(B, H, W, Cin, Cout)}|{'f16' if f16 else 'bf16'}|{'full' if full else 'plain'}", *(got if full else (got,)))
        # split patch embedding
        for (B, C, h, w, E) in [(1, 64, 37, 53, 40), (3, 32, 48, 50, 128)]:
            prep = ops.prep_patch_embed_weight(rnd(2, (E, C, 16, 16), 1.0 / (16 * C ** 0.5)), f16)
            xs = ops.split_act(rnd(1, (B, C, h, w)).contiguous(memory_format=CL), f16=f16)
            y = ops.patch_embed_split(xs, prep[0], prep[1], rnd(3, (E,), 0.1) if full else None,
                                      rnd(4, ((h // 16) * (w // 16), E)) if full else None, oscale=prep[2] if f16 else None)
            note(f"patch_embed_split|{(B, C, h, w, E)}|{'f16' if f16 else 'bf16'}|{'full' if full else 'plain'}", y)

# the strided fp32-input kernel at 17 x 23 (bf16 pairs only: it splits its input itself)
for full in (False, True):
    for stride in (1, 2):
        B, cin, cout, H, W = 3, 24, 40, 17, 23
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        hi, lo = ops.prep_conv_weight(rnd(2, (cout, cin, 3, 3), 1.0 / (3 * cin ** 0.5)))
        y = ops.conv3x3_strided(rnd(1, (B, cin, H, W)).contiguous(memory_format=CL), hi, lo, rnd(3, (cout,), 0.1) if full else None, stride,
                                (1, 1), ops.ACT_SILU if full else 0,
                                residual=rnd(4, (B, cout, Ho, Wo)).contiguous(memory_format=CL) if full else None, out_hw=(Ho, Wo))
        note(f"strided|s{stride}|{'full' if full else 'plain'}", y)

print(f"{len(lines)} cases  sha1 of all lines {hashlib.sha1(chr(10).join(lines).encode()).hexdigest()}  [{os.environ.get('OCV_LIB_PATH', 'product build')}]")
