"""-m gpu: no launch writes or reads beside its operands -- every ``hip_ops`` entry point under the guarded-allocation harness
of tests/mem_guard.py.

(a) ROWS: one row per operation, at the smallest shapes where its tiling is ragged.  Inputs and weights are guarded copies,
    outputs and workspaces are guarded by the harness (exact size, poisoned).  A row asserts: no guard breached, no 32-bit
    word of an output left unwritten (hl32 pad channels zero), no device pointer handed to the library that lies outside a
    guarded payload, and the result within the family's own tolerance of the family's own float64 / reference statement
    (the constants and helpers are imported from the family's test).
(b) whole eager forwards of AdaBins / GraphBins under the harness: no breach, finite, bit-equal to the forward outside it.
(c) accounting: every ``*_fwd`` entry point of ``_lib.PROTOTYPES`` ran in (a), but for the few named in ``EXEMPT``.

Where the issue's wish and a kernel's contract differ: the halo-staged 3 x 3 kernel takes whole 8 x 32 patches only
(ocv_conv3x3_halo_supported), so its row is 16 x 64; dense split-K starts at more than 256 tiles of 256 x 128 and 128 K steps
(conv_ksplit), so its row is the smallest such shape with H, W no multiples of 4 and a ragged channel tile; the fused
expand + depthwise has one kernel, so "the LDS-rows kernel" is the depthwise one (ocv_depthwise_set_dispatch(2))."""
import contextlib
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen
import mem_guard
from decoder_shadow import BF16_TOL, EXACT_TOL, WINO_TOL
from oracle import restate
from test_hip_encoders import KERNEL_TOL
from test_hip_fp16_route import F16_TOL
from test_hip_kernels import SPLIT_TOL, TOL, _attn_ref, _encoder_sd, _same_pad
from util import branch_dev, max_rel, rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CL = torch.channels_last
DEV = "cuda"
ROWS = {}            # name -> (function, guard bytes)
RAN = {}             # name -> the ocv_* calls the row made
TRIED = set()        # rows that were started in this process, passed or not
PAIR_TOL = {False: 1e-5, True: 3e-7}      # split copy against its fp32 twin: bf16 pairs (test_hip_kernels.py), fp16 pairs (test_hip_fp16_route.py)


def rnd(key, shape, seed=0, scale=1.0):
    return gen.randn(key, shape, seed, scale)


def row(name, guard_bytes=mem_guard.DEFAULT_GUARD_BYTES):
    def deco(fn):
        assert name not in ROWS, name
        ROWS[name] = (fn, guard_bytes)
        return fn
    return deco


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Ctx:
    """What a row works with: ``put`` / ``cl`` make guarded device copies of inputs and weights, ``out`` names the outputs."""

    def __init__(self, g):
        from objcavit_amd import _lib, hip_ops
        self.g, self.ops, self.lib = g, hip_ops, _lib.load()          # (the recorder's proxy: record_calls came first)
        self.outputs, self.splits = [], []

    def put(self, t):
        return None if t is None else self.g.copy(t)

    def cl(self, t):
        return None if t is None else self.g.copy(t.contiguous(memory_format=CL))

    def weights(self, *ts):
        return tuple(self.put(t) for t in ts)

    def split(self, x, f16=False):
        """fp32 NCHW host tensor -> guarded SplitAct (the resize kernel at scale 1: a guarded launch of its own)."""
        s = self.ops.split_act(self.cl(x), f16=f16)
        self.out(s)
        return s

    def out(self, *ts):
        for t in ts:
            if t is None:
                continue
            if isinstance(t, self.ops.SplitAct):
                self.splits.append(t)
                self.outputs.append(t.hl)
            else:
                self.outputs.append(t)

    def stream(self):
        return torch.cuda.current_stream().cuda_stream


def _pads_zero(sa):
    B, H, W, c2 = sa.hl.shape
    Cp = c2 // 2
    if Cp == sa.C:
        return True
    blocks = sa.hl.view(B, H, W, Cp // 32, 2, 32).permute(0, 1, 2, 4, 3, 5).reshape(B, H, W, 2, Cp)
    return not bool(blocks[..., sa.C:].any())


def run_row(name):
    fn, guard_bytes = ROWS[name]
    TRIED.add(name)
    if name.startswith("bin_head"):
        _bin_case()                                  # shared inputs and float64 references: made once, outside the harness
    try:
        with mem_guard.guarded("cuda", guard_bytes=guard_bytes) as g:
            g.record_calls()
            c = Ctx(g)
            fn(c)
            torch.cuda.synchronize()
            g.check()
            for t in c.outputs:
                left = g.never_written(t)
                assert left == 0, f"{name}: {left} word(s) of an output {tuple(t.shape)} {t.dtype} were never written"
            for s in c.splits:
                assert _pads_zero(s), f"{name}: pad channels of a split output are not zero"
            assert not g.stray, f"{name}: pointers outside every guarded payload: {g.stray[:6]}"
            assert g.calls, name
            RAN[name] = list(g.calls)
    except RuntimeError as e:                      # a device fault ends the session: nothing more is launched on a faulted GPU
        if "HIP error" in str(e) or "illegal memory" in str(e) or "hipError" in str(e):
            pytest.exit(f"GPU fault in row {name}: {e}", returncode=3)
        raise


def act_ref(ref, act):
    return [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref), torch.sigmoid(ref)][act]


# =====================================================================================================================
# dense convolutions
# =====================================================================================================================
CONV_SHAPES = [(1, 9, 33, 40, 72),      # one row and one column past an 8 x 32 patch, Cp padding, Cout no multiple of 32 / 128
               (3, 5, 7, 32, 40)]       # M = 105: less than one tile


def _conv_case(B, H, W, Cin, Cout, k, act, on_gpu=False):
    x = rnd("x", (B, Cin, H, W), 1)
    w, b = rnd("w", (Cout, Cin, k, k), 3, 1 / math.sqrt(Cin * k * k)), rnd("b", (Cout,), 4, 0.2)
    if on_gpu:
        ref = F.conv2d(x.cuda().double(), w.cuda().double(), b.cuda().double(), padding=k // 2)
        ref = act_ref(ref, act).cpu()
    else:
        ref = act_ref(F.conv2d(x.double(), w.double(), b.double(), padding=k // 2), act)
    return x, w, b, ref


def _unpack(got, out_fp32, out_split):
    if out_fp32 and out_split:
        return got
    return (got, None) if out_fp32 else (None, got)


def _check_conv_outputs(c, y, ys, ref, tol, f16):
    if y is not None:
        assert y.is_contiguous(memory_format=CL) and rel_dev(y, ref) < tol, rel_dev(y, ref)
    if ys is not None:
        assert ys.f16 == f16
        if y is not None:
            assert rel_dev(ys.float(), y) < PAIR_TOL[f16]
        else:
            assert rel_dev(ys.float(), ref) < tol, rel_dev(ys.float(), ref)
    c.out(y, ys)


for _shape in CONV_SHAPES:
    for _k in (1, 3):
        def _conv_nhwc_row(c, shape=_shape, k=_k):
            B, H, W, Cin, Cout = shape
            x, w, b, ref = _conv_case(B, H, W, Cin, Cout, k, 2)
            res = rnd("res", tuple(ref.shape), 5)
            hi, lo = c.weights(*c.ops.prep_conv_weight(w.cuda()))
            two = Cin > 32                                           # two sources, the virtual concat: C1 must be whole 32-blocks
            y = c.ops.conv_nhwc(c.cl(x[:, :32]) if two else c.cl(x), c.cl(x[:, 32:]) if two else None, hi, lo, c.put(b), k, 2,
                                residual=c.cl(res))
            assert rel_dev(y, ref + res) < SPLIT_TOL
            y1 = c.ops.conv_nhwc(c.cl(x), None, hi, lo, None, k, 0)
            assert rel_dev(y1, F.conv2d(x.double(), w.double(), padding=k // 2)) < SPLIT_TOL
            c.out(y, y1)
        row(f"conv_nhwc|{_shape}|k{_k}")(_conv_nhwc_row)

        for _f16 in (False, True):
            for _outs in ((True, False), (False, True), (True, True)):
                def _conv_split_row(c, shape=_shape, k=_k, f16=_f16, outs=_outs):
                    B, H, W, Cin, Cout = shape
                    x, w, b, ref = _conv_case(B, H, W, Cin, Cout, k, 2)
                    xs = c.split(x, f16)
                    prep = c.weights(*c.ops.prep_conv_weight(w.cuda(), f16=f16))
                    got = c.ops.conv_nhwc_split(xs, prep[0], prep[1], c.put(b), k, 2, out_fp32=outs[0], out_split=outs[1],
                                                oscale=prep[2] if f16 else None)
                    if k == 3:
                        assert c.lib.ocv_conv3x3_last_kernel() == 1                  # the tap ring (conv_split_dma_kernel)
                    y, ys = _unpack(got, *outs)
                    _check_conv_outputs(c, y, ys, ref, F16_TOL if f16 else SPLIT_TOL, f16)
                row(f"conv_nhwc_split|{_shape}|k{_k}|{'f16' if _f16 else 'bf16'}|{'y' * _outs[0]}{'s' * _outs[1]}")(_conv_split_row)


for _f16 in (False, True):
    def _conv_halo_row(c, f16=_f16):
        """conv_halo_dma_kernel, forced (automatic dispatch keeps it for two full-size layers): B 2, two patch rows and columns,
        Cp = 64 with pad channels, a ragged second channel tile.  Reference and bars as test_hip_conv_halo.py."""
        B, H, W, Cin, Cout = 2, 16, 64, 40, 136
        assert c.lib.ocv_conv3x3_halo_supported(B, H, W, Cin, Cout) == 1
        x, w, b, _ = _conv_case(B, H, W, Cin, Cout, 3, 2)
        xs = c.split(x, f16)
        prep = c.weights(*c.ops.prep_conv_weight(w.cuda(), f16=f16))
        assert c.lib.ocv_conv3x3_set_dispatch(2) == 0
        try:
            y, ys = c.ops.conv_nhwc_split(xs, prep[0], prep[1], c.put(b), 3, 2, out_fp32=True, out_split=True,
                                          oscale=prep[2] if f16 else None)
            assert c.lib.ocv_conv3x3_last_kernel() == 2
        finally:
            c.lib.ocv_conv3x3_set_dispatch(0)
        ref = F.leaky_relu(F.conv2d(xs.float().double().cpu(), w.double(), b.double(), padding=1), 0.01)
        assert max(branch_dev(y, ref)) < (F16_TOL if f16 else BF16_TOL)
        assert rel_dev(ys.float(), y) < PAIR_TOL[f16]
        c.out(y, ys)
    row(f"conv_nhwc_split|halo|{'f16' if _f16 else 'bf16'}")(_conv_halo_row)


@row("conv_nhwc_split|split-K", guard_bytes=8 << 20)     # rows of 1032 fp32 channels: 256 x 1032 x 4 B = 1.01 MiB per tile row block
def _conv_splitk_row(c):
    B, H, W, Cin, Cout = 1, 45, 183, 456, 1032
    nws = c.lib.ocv_conv_nhwc_split_workspace_bytes(B, H, W, Cin, Cout, 3)
    assert nws == 2 * B * H * W * Cout * 4                            # two K halves of fp32 partial sums + the finish pass
    x, w, b, ref = _conv_case(B, H, W, Cin, Cout, 3, 2, on_gpu=True)
    xs = c.split(x, True)
    hi, lo, osc = c.weights(*c.ops.prep_conv_weight(w.cuda(), f16=True))
    y, ys = c.ops.conv_nhwc_split(xs, hi, lo, c.put(b), 3, 2, out_fp32=True, out_split=True, oscale=osc)
    assert c.lib.ocv_conv3x3_last_kernel() == 1
    _check_conv_outputs(c, y, ys, ref, F16_TOL, True)


for _f16 in (False, True):
    def _packed_taps_row(c, f16=_f16):
        B, H, W, Cin, Cout = CONV_SHAPES[0]
        assert c.ops.packed_taps_pay(Cin)
        x, w, b, ref = _conv_case(B, H, W, Cin, Cout, 3, 2)
        xs = c.split(x, f16)
        prep = c.weights(*c.ops.prep_conv_weight_packed_taps(w.cuda(), f16=f16))
        y, ys = c.ops.conv3x3_split_packed_taps(xs, prep[0], prep[1], c.put(b), 2, out_fp32=True, out_split=True,
                                                oscale=prep[2] if f16 else None)
        assert rel_dev(y, ref) < SPLIT_TOL and rel_dev(ys.float(), y) < (1e-6 if f16 else 1e-5)      # test_conv3x3_packed_taps
        c.out(y, ys)
    row(f"conv3x3_packed_taps|{'f16' if _f16 else 'bf16'}")(_packed_taps_row)


for _shape in [(1, 7, 9, 40, 72), (1, 5, 7, 1056, 40)]:              # ragged everything / Cp > 1024: the two-round input transform
    for _f16 in (False, True):
        def _winograd_row(c, shape=_shape, f16=_f16):
            B, H, W, Cin, Cout = shape
            x, w, b, ref = _conv_case(B, H, W, Cin, Cout, 3, 2)
            xs = c.split(x, f16)
            u_hi, u_lo, fs, cs = c.weights(*c.ops.prep_winograd43_weight(w.cuda()))
            assert c.lib.ocv_conv3x3_winograd43_workspace_bytes(B, H, W, Cin, Cout) > 0
            y, ys = c.ops.conv3x3_winograd43_split(xs, u_hi, u_lo, fs, c.put(b), 2, out_fp32=True, out_split=True, cscale=cs)
            _check_conv_outputs(c, y, ys, ref, WINO_TOL if f16 else SPLIT_TOL, f16)
        row(f"conv3x3_winograd43|{_shape}|{'f16' if _f16 else 'bf16'}")(_winograd_row)


for _pad in ("sym", "same"):
    for _res in (False, True):
        def _strided_row(c, pad=_pad, res=_res):
            """test_strided_conv3x3_vs_fp64 at stride 2 on an odd 17 x 23 map, three images."""
            B, cin, cout, H, W, stride = 3, 24, 40, 17, 23, 2
            x, w, b = rnd("x", (B, cin, H, W), 1), rnd("w", (cout, cin, 3, 3), 2, 1 / math.sqrt(9 * cin)), rnd("b", (cout,), 3, 0.1)
            if pad == "sym":
                pt, pl = 1, 1
                Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
            else:
                Ho, Wo = -(-H // stride), -(-W // stride)
                pt, pl = max((Ho - 1) * stride + 3 - H, 0) // 2, max((Wo - 1) * stride + 3 - W, 0) // 2
            pb, pr = (Ho - 1) * stride + 3 - H - pt, (Wo - 1) * stride + 3 - W - pl
            ref = F.silu(F.conv2d(F.pad(x.double(), (pl, pr, pt, pb)), w.double(), b.double(), stride=stride))
            r = rnd("r", (B, cout, Ho, Wo), 4) if res else None
            if res:
                ref = ref + r.double()
            hi, lo = c.weights(*c.ops.prep_conv_weight(w.cuda()))
            y = c.ops.conv3x3_strided(c.cl(x), hi, lo, c.put(b), stride, (pt, pl), c.ops.ACT_SILU, residual=c.cl(r), out_hw=(Ho, Wo))
            assert tuple(y.shape) == tuple(ref.shape) and rel_dev(y, ref) < KERNEL_TOL
            c.out(y)
        row(f"conv3x3_strided|{_pad}|{'res' if _res else 'plain'}")(_strided_row)


@row("conv_nhwc_exact")
def _conv_exact_row(c):
    B, H, W, C1, C2, Cout, k = 2, 13, 17, 40, 3, 72, 3
    x1, x2 = rnd("x1", (B, C1, H, W), 1), rnd("x2", (B, C2, H, W), 2)
    w, b = rnd("w", (Cout, C1 + C2, k, k), 3, 1 / math.sqrt((C1 + C2) * k * k)), rnd("b", (Cout,), 4, 0.2)
    res = rnd("r", (B, Cout, H, W), 5)
    ref = F.leaky_relu(F.conv2d(torch.cat([x1, x2], 1).double(), w.double(), b.double(), padding=1), 0.01) + res
    wt = c.put(w.permute(2, 3, 0, 1).reshape(k * k, Cout, C1 + C2).contiguous())
    y = c.ops.conv_nhwc_exact(c.cl(x1), c.cl(x2), wt, c.put(b), k, 2, residual=c.cl(res))
    assert rel_dev(y, ref) < EXACT_TOL
    c.out(y)


@row("conv3x3_few_channels")
def _few_channels_row(c):
    B, C, H, W, Cout = 2, 3, 33, 47, 128
    x, w = rnd("x", (B, C, H, W), 1), rnd("w", (Cout, C, 3, 3), 2, 0.4)
    y = c.ops.conv3x3_few_channels(c.put(x), c.put(w.permute(2, 3, 1, 0).reshape(9, C, Cout).contiguous()))
    assert rel_dev(y, F.conv2d(x.double(), w.double(), padding=1)) < EXACT_TOL        # test_conv3x3_few_channels: 2e-6
    c.out(y)


@row("stem_conv_same")
def _stem_row(c):
    B, Cin, H, W, Cout, stride = 1, 3, 33, 47, 48, 2
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 3, 3), 2, 0.3), rnd("b", (Cout,), 3, 0.2)
    y = c.ops.stem_conv_same(c.put(x), c.put(w), c.put(b), stride, 3)
    assert rel_dev(y, F.silu(F.conv2d(_same_pad(x, 3, stride), w, b, stride=stride))) < TOL
    c.out(y)


@row("conv_nhwc_split|first-ABI entry points")
def _conv_legacy_row(c):
    """ocv_conv_nhwc_split_fwd / ocv_conv_nhwc_split_ws_fwd: the bf16-pair forms an ABI 3 caller still links against."""
    B, H, W, Cin, Cout = CONV_SHAPES[0]
    x, w, b, ref = _conv_case(B, H, W, Cin, Cout, 3, 2)
    xs = c.split(x, False)
    hi, lo = c.weights(*c.ops.prep_conv_weight(w.cuda()))
    bg = c.put(b)
    for ws_form in (False, True):
        y = torch.empty(B, Cout, H, W, dtype=torch.float32, device=DEV, memory_format=CL)
        ys = c.ops.SplitAct.empty(B, Cout, H, W, DEV)
        args = (xs.hl.data_ptr(), Cin, hi.data_ptr(), lo.data_ptr(), bg.data_ptr(), None, y.data_ptr(), ys.hl.data_ptr(), B, H, W, Cout, 3, 2)
        rc = c.lib.ocv_conv_nhwc_split_ws_fwd(*args, None, 0, c.stream()) if ws_form else c.lib.ocv_conv_nhwc_split_fwd(*args, c.stream())
        assert rc == 0, c.lib.ocv_last_error()
        _check_conv_outputs(c, y, ys, ref, SPLIT_TOL, False)


# =====================================================================================================================
# resize + concat + split: one shape per kernel (test_upsample_concat_split), both pair types
# =====================================================================================================================
UPSAMPLE_SHAPES = [(3, 5, 7, 11, 13, 8, 4), (2, 9, 11, 17, 21, 16, 8), (1, 20, 24, 11, 13, 8, 8), (1, 9, 11, 19, 23, 128, 8),
                   (2, 8, 10, 16, 20, 1096, 0), (1, 1, 1, 5, 7, 64, 0)]


def _upsample_ref(x, skip, H, W):
    ref = F.interpolate(x, size=[H, W], mode="bilinear", align_corners=True)
    return ref if skip is None else torch.cat([ref, skip], 1)


for _shape in UPSAMPLE_SHAPES:
    for _f16 in (False, True):
        def _upsample_row(c, shape=_shape, f16=_f16):
            B, h, w, H, W, C1, C2 = shape
            x = rnd("x", (B, C1, h, w), 1)
            skip = rnd("s", (B, C2, H, W), 2) if C2 else None
            got = c.ops.upsample_concat_split(c.cl(x), c.cl(skip), (H, W), f16=f16)
            assert got.hl.dtype == (torch.float16 if f16 else torch.bfloat16) and tuple(got.shape) == (B, C1 + C2, H, W)
            # test_upsample_concat_split (bf16 pairs: 1e-5) / test_split_producers_write_fp16_pairs (2e-6)
            assert rel_dev(got.float(), _upsample_ref(x, skip, H, W)) < (2e-6 if f16 else 1e-5)
            c.out(got)
        row(f"upsample_concat_split|{_shape}|{'f16' if _f16 else 'bf16'}")(_upsample_row)


@row("upsample_concat_split|first-ABI entry point")
def _upsample_legacy_row(c):
    B, h, w, H, W, C1, C2 = UPSAMPLE_SHAPES[1]
    x, skip = rnd("x", (B, C1, h, w), 1), rnd("s", (B, C2, H, W), 2)
    xg, sg = c.cl(x), c.cl(skip)
    out = c.ops.SplitAct.empty(B, C1 + C2, H, W, DEV)
    rc = c.lib.ocv_upsample_concat_split_fwd(xg.data_ptr(), h, w, C1, sg.data_ptr(), C2, out.hl.data_ptr(), B, H, W, c.stream())
    assert rc == 0, c.lib.ocv_last_error()
    assert rel_dev(out.float(), _upsample_ref(x, skip, H, W)) < 1e-5
    c.out(out)


# =====================================================================================================================
# tap interpolation
# =====================================================================================================================
TAP_SHAPES = [(1, 5, 7, 11, 13, 8), (1, 17, 22, 30, 40, 72), (1, 1, 1, 7, 9, 40)]


def _tap_ref(z, s, b, H, W, Cout, act):
    """test_tap_interp_combine's definition in fp64."""
    ref = torch.zeros(z.shape[0], Cout, H, W, dtype=torch.float64)
    if s is not None:
        ref = ref + s.double()
    if b is not None:
        ref = ref + b.double().view(1, -1, 1, 1)
    for t in range(9):
        up = F.interpolate(z[:, t * Cout:(t + 1) * Cout].double(), size=(H, W), mode="bilinear", align_corners=True)
        dy, dx = t // 3 - 1, t % 3 - 1
        ref = ref + F.pad(up, (1, 1, 1, 1))[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return act_ref(ref, act)


for _shape in TAP_SHAPES:
    for _border in (False, True):
        for _f16 in (False, True):
            def _tap_row(c, shape=_shape, bordered=_border, f16=_f16):
                B, h, w, H, W, Cout = shape
                z = rnd("z", (B, 9 * Cout, h, w), 1)
                s, b = rnd("s", (B, Cout, H, W), 2), rnd("b", (Cout,), 3, 0.3)
                border = rnd("c", (9 * Cout,), 4) if bordered else None
                full = z
                if bordered:                                        # the grid the bordered form stands for, materialised
                    full = border.view(1, -1, 1, 1).expand(B, 9 * Cout, h + 2, w + 2).clone()
                    full[:, :, 1:-1, 1:-1] = z
                assert c.ops.tap_interp_supported(full.shape[2], full.shape[3], H, W, Cout)
                y, ys = c.ops.tap_interp_combine(c.cl(z), c.cl(s), c.put(b), (H, W), 2, out_fp32=True, out_split=True,
                                                 border=c.put(border), split_f16=f16)
                assert rel_dev(y, _tap_ref(full, s, b, H, W, Cout, 2)) < TOL
                assert rel_dev(ys.float(), y) < PAIR_TOL[f16]
                y2 = c.ops.tap_interp_combine(c.cl(z), None, None, (H, W), 0, border=c.put(border))
                assert rel_dev(y2, _tap_ref(full, None, None, H, W, Cout, 0)) < TOL
                c.out(y, ys, y2)
            row(f"tap_interp_combine|{_shape}|{'bordered' if _border else 'plain'}|{'f16' if _f16 else 'bf16'}")(_tap_row)


@row("tap_interp_combine|first-ABI entry point")
def _tap_legacy_row(c):
    B, h, w, H, W, Cout = TAP_SHAPES[1]
    z, s, b = rnd("z", (B, 9 * Cout, h, w), 1), rnd("s", (B, Cout, H, W), 2), rnd("b", (Cout,), 3, 0.3)
    zg, sg, bg = c.cl(z), c.cl(s), c.put(b)
    y = torch.empty(B, Cout, H, W, dtype=torch.float32, device=DEV, memory_format=CL)
    ys = c.ops.SplitAct.empty(B, Cout, H, W, DEV)
    rc = c.lib.ocv_tap_interp_combine_fwd(zg.data_ptr(), h, w, 0, None, sg.data_ptr(), bg.data_ptr(), y.data_ptr(), ys.hl.data_ptr(),
                                          B, H, W, Cout, 2, c.stream())
    assert rc == 0, c.lib.ocv_last_error()
    assert rel_dev(y, _tap_ref(z, s, b, H, W, Cout, 2)) < TOL and rel_dev(ys.float(), y) < PAIR_TOL[False]
    c.out(y, ys)


for _shape in [(1, 5, 7, 11, 13, 8, 8, 8), (1, 17, 22, 30, 40, 96, 16, 72), (1, 1, 1, 7, 9, 40, 0, 40)]:
    for _f16 in (False, True):
        def _lowres_row(c, shape=_shape, f16=_f16):
            """test_upsampled_conv_at_low_resolution / test_lowres_first_convolution_on_fp16_pairs: tap GEMM + skip-part 3 x 3 + tap
            interpolation against conv3x3(cat(interpolate(x), skip)) in fp64."""
            B, h, w, H, W, C1, C2, Cout = shape
            x = rnd("x", (B, C1, h, w), 1)
            skip = rnd("k", (B, C2, H, W), 2) if C2 else None
            wt, b = rnd("w", (Cout, C1 + C2, 3, 3), 3, 1 / math.sqrt((C1 + C2) * 9)), rnd("b", (Cout,), 4, 0.2)
            up = F.interpolate(x.double(), size=(H, W), mode="bilinear", align_corners=True)
            ref = F.leaky_relu(F.conv2d(up if skip is None else torch.cat([up, skip.double()], 1), wt.double(), b.double(), padding=1), 0.01)
            wa = wt.cuda()[:, :C1].permute(2, 3, 0, 1).reshape(9 * Cout, C1, 1, 1)
            a = c.weights(*c.ops.prep_conv_weight(wa, f16=f16))
            z = c.ops.conv_nhwc_split(c.split(x, f16), a[0], a[1], None, 1, 0, oscale=a[2] if f16 else None)
            s = None
            if skip is not None:
                p = c.weights(*c.ops.prep_conv_weight(wt.cuda()[:, C1:].contiguous(), f16=f16))
                s = c.ops.conv_nhwc_split(c.split(skip, f16), p[0], p[1], None, 3, 0, oscale=p[2] if f16 else None)
            y, ys = c.ops.tap_interp_combine(z, s, c.put(b), (H, W), 2, out_fp32=True, out_split=True, split_f16=f16)
            assert rel_dev(y, ref) < (F16_TOL if f16 else SPLIT_TOL) and rel_dev(ys.float(), y) < PAIR_TOL[f16]
            c.out(z, s, y, ys)
        row(f"upsampled_conv_at_low_resolution|{_shape}|{'f16' if _f16 else 'bf16'}")(_lowres_row)


# =====================================================================================================================
# 1 x 1 convolutions of the encoder
# =====================================================================================================================
PW_SHAPES = [(3, 5, 7, 40, 24), (3, 5, 7, 240, 40)]


def _pw_case(B, H, W, Cin, Cout, act, gate=True, res=True):
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 1, 1), 2, 1 / math.sqrt(Cin)), rnd("b", (Cout,), 3, 0.2)
    g = torch.sigmoid(rnd("g", (B, Cin), 4)) if gate else None
    r = rnd("r", (B, Cout, H, W), 5) if res else None
    xin = x if g is None else x * g[:, :, None, None]
    ref = act_ref(F.conv2d(xin.double(), w.double(), b.double()), act)
    return x, w, b, g, r, (ref if r is None else ref + r)


def _split_weight(c, w):
    sw = c.ops.SplitWeight(w.cuda())
    sw.packed = c.put(sw.packed)
    return sw


for _shape in PW_SHAPES:
    def _pw_fp32_row(c, shape=_shape):
        x, w, b, g, r, ref = _pw_case(*shape, 0)
        y = c.ops.pointwise_nhwc(c.cl(x), c.put(w), c.put(b), 0, gate=c.put(g), residual=c.cl(r))
        assert rel_dev(y, ref) < TOL
        c.out(y)
    row(f"pointwise_nhwc|fp32|{_shape}")(_pw_fp32_row)

    def _pw_split_row(c, shape=_shape):
        x, w, b, g, r, ref = _pw_case(*shape, 0)
        sw = _split_weight(c, w)
        y = c.ops.pointwise_nhwc(c.cl(x), sw, c.put(b), 0, gate=c.put(g), residual=c.cl(r))
        assert rel_dev(y, ref) < SPLIT_TOL
        y2, ys = c.ops.pointwise_nhwc(c.cl(x), sw, c.put(b), 0, gate=c.put(g), residual=c.cl(r), out_split=True)
        assert rel_dev(y2, ref) < SPLIT_TOL
        hi = y2.to(torch.bfloat16)                                   # test_pointwise_nhwc_split_also_writes_the_split_copy
        assert torch.equal(ys.hi.contiguous(), hi) and torch.equal(ys.lo.contiguous(), (y2 - hi.float()).to(torch.bfloat16))
        x3, w3, b3, _, _, ref3 = _pw_case(*shape, 3, gate=False, res=False)
        y3 = c.ops.pointwise_nhwc(c.cl(x3), sw, c.put(b3), 3)
        assert rel_dev(y3, ref3) < SPLIT_TOL
        c.out(y, y2, ys, y3)
    row(f"pointwise_nhwc|split|{_shape}")(_pw_split_row)

    def _pw_legacy_row(c, shape=_shape):
        """ocv_pointwise_conv_nhwc_split_fwd / ocv_pointwise_conv_nhwc_split_hl_fwd (no workspace argument)."""
        B, H, W, Cin, Cout = shape
        x, w, b, g, r, ref = _pw_case(*shape, 0)
        sw = _split_weight(c, w)
        xg, bg, gg, rg = c.cl(x), c.put(b), c.put(g), c.cl(r)
        M = B * H * W
        y = torch.empty(B, Cout, H, W, dtype=torch.float32, device=DEV, memory_format=CL)
        rc = c.lib.ocv_pointwise_conv_nhwc_split_fwd(xg.data_ptr(), gg.data_ptr(), H * W, sw.packed.data_ptr(), bg.data_ptr(), rg.data_ptr(),
                                                     y.data_ptr(), M, Cin, Cout, 0, c.stream())
        assert rc == 0, c.lib.ocv_last_error()
        y2 = torch.empty(B, Cout, H, W, dtype=torch.float32, device=DEV, memory_format=CL)
        ys = c.ops.SplitAct.empty(B, Cout, H, W, DEV)
        rc = c.lib.ocv_pointwise_conv_nhwc_split_hl_fwd(xg.data_ptr(), gg.data_ptr(), H * W, sw.packed.data_ptr(), bg.data_ptr(), rg.data_ptr(),
                                                        y2.data_ptr(), ys.hl.data_ptr(), M, Cin, Cout, 0, c.stream())
        assert rc == 0, c.lib.ocv_last_error()
        assert rel_dev(y, ref) < SPLIT_TOL and rel_dev(y2, ref) < SPLIT_TOL and rel_dev(ys.float(), ref) < SPLIT_TOL
        c.out(y, y2, ys)
    row(f"pointwise_nhwc|first-ABI entry points|{_shape}")(_pw_legacy_row)

    for _cfg in [(0, 0), (1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2)]:        # test_pointwise_hl's pinned wavefront tiles
        def _pw_hl_row(c, shape=_shape, cfg=_cfg):
            B, H, W, Cin, Cout = shape
            x, w, b, _, r, _ = _pw_case(*shape, 0, gate=False)
            xs = c.split(x)
            ref = F.conv2d(x.double(), w.double(), b.double()) + r
            sw = _split_weight(c, w)
            assert c.lib.ocv_pointwise_hl_set_dispatch(*cfg) == 0
            try:
                y, ys = c.ops.pointwise_hl(xs, sw, c.put(b), 0, residual=c.cl(r), out_fp32=True, out_split=True)
                only = c.ops.pointwise_hl(xs, sw, c.put(b), 0, residual=c.cl(r), out_fp32=False, out_split=True)
            finally:
                c.lib.ocv_pointwise_hl_set_dispatch(0, 0)
            assert rel_dev(y, ref) < SPLIT_TOL and rel_dev(ys.float(), ref) < SPLIT_TOL and rel_dev(only.float(), ref) < SPLIT_TOL
            c.out(y, ys, only)
        row(f"pointwise_hl|{_shape}|cfg{_cfg}")(_pw_hl_row)


@row("pointwise_nhwc|split-K across workgroups")
def _pw_splitk_row(c):
    """The smallest M x K the scratch query gives slices to: 35 rows (one ragged 32-row tile more), K = 1040, 40 channels."""
    B, H, W, Cin, Cout = 1, 5, 7, 1040, 40
    assert c.lib.ocv_pointwise_split_workspace_bytes(B * H * W, Cin, Cout) > 0
    for act, gate, res in ((0, True, True), (3, False, False)):
        x, w, b, g, r, ref = _pw_case(B, H, W, Cin, Cout, act, gate, res)
        y = c.ops.pointwise_nhwc(c.cl(x), _split_weight(c, w), c.put(b), act, gate=c.put(g), residual=c.cl(r))
        assert rel_dev(y, ref) < SPLIT_TOL
        c.out(y)
    assert "ocv_pointwise_conv_nhwc_split_ws_fwd" in c.g.calls


# =====================================================================================================================
# depthwise, squeeze-excite, fused expand + depthwise
# =====================================================================================================================
DW_SHAPES = [(3, 12, 33, 47), (1, 4, 1, 1)]


def _dw_case(B, C, H, W, k, R=None):
    x, w, b = rnd("x", (B, C, H, W), 1), rnd("w", (C, 1, k, k), 2, 0.3), rnd("b", (C,), 3, 0.2)
    if R is None:
        return x, w, b
    w1, b1 = rnd("w1", (R, C), 4, 1 / math.sqrt(C)), rnd("b1", (R,), 5, 0.3)
    w2, b2 = rnd("w2", (C, R), 6, 1 / math.sqrt(R)), rnd("b2", (C,), 7, 0.3)
    return x, w, b, w1, b1, w2, b2


def _gate_ref(d, w1, b1, w2, b2):
    return torch.sigmoid(F.silu(d.mean((2, 3)) @ w1.T + b1) @ w2.T + b2)


for _shape in DW_SHAPES:
    for _k, _s in [(3, 1), (3, 2), (5, 1), (5, 2)]:
        def _dw_row(c, shape=_shape, k=_k, s=_s):
            B, C, H, W = shape
            x, w, b = _dw_case(B, C, H, W, k)
            ref = F.silu(F.conv2d(_same_pad(x, k, s), w, b, stride=s, groups=C))
            y = c.ops.depthwise_conv_same(c.put(x), c.put(w), c.put(b), s, 3)                       # NCHW
            assert y.shape == ref.shape and rel_dev(y, ref) < TOL
            y2 = c.ops.depthwise_nhwc_same(c.cl(x), c.put(w.flatten(1).t().contiguous()), c.put(b), k, s, 3)
            assert y2.shape == ref.shape and rel_dev(y2, ref) < TOL
            c.out(y, y2)
        row(f"depthwise|{_shape}|k{_k}s{_s}")(_dw_row)

        for _mode in (1, 2):                                         # register window / LDS rows wherever supported
            def _dw_se_row(c, shape=_shape, k=_k, s=_s, mode=_mode):
                B, C, H, W = shape
                R = max(1, C // 3)
                x, w, b, w1, b1, w2, b2 = _dw_case(B, C, H, W, k, R)
                ref = F.silu(F.conv2d(_same_pad(x, k, s), w, b, stride=s, groups=C))
                assert c.lib.ocv_depthwise_set_dispatch(mode) == 0
                try:
                    y, g = c.ops.depthwise_se_gate(c.cl(x), c.put(w.flatten(1).t().contiguous()), c.put(b), k, s,
                                                   c.put(w1), c.put(b1), c.put(w2.t().contiguous()), c.put(b2))
                finally:
                    c.lib.ocv_depthwise_set_dispatch(0)
                assert rel_dev(y, ref) < TOL and rel_dev(g, _gate_ref(ref, w1, b1, w2, b2)) < TOL
                c.out(y, g)
            row(f"depthwise_se_gate|{_shape}|k{_k}s{_s}|{'window' if _mode == 1 else 'lds-rows'}")(_dw_se_row)


@row("depthwise_hl_gate_weights_project")
def _dw_hl_row(c):
    """test_depthwise_hl_gate_weights_project's smallest case: 5 x 5 stride 2 on 13 x 17, 96 channels, 24 out."""
    k, s, B, C, H, W, R, N = 5, 2, 2, 96, 13, 17, 4, 24
    x, w, b, w1, b1, w2, b2 = _dw_case(B, C, H, W, k, R)
    wp, bp = rnd("wp", (N, C), 8, 1 / math.sqrt(C)), rnd("bp", (N,), 9, 0.2)
    d = F.silu(F.conv2d(_same_pad(x, k, s), w, b, stride=s, groups=C)).double()
    gref = torch.sigmoid(F.silu(d.mean((2, 3)) @ w1.double().T + b1.double()) @ w2.double().T + b2.double())
    res = rnd("r", (B, N, d.shape[2], d.shape[3]), 10)
    ref = F.conv2d(d * gref[:, :, None, None], wp.double()[:, :, None, None], bp.double()) + res
    args = (c.cl(x), c.put(w.flatten(1).t().contiguous()), c.put(b), k, s, c.put(w1), c.put(b1), c.put(w2.t().contiguous()), c.put(b2))
    y_fp32, g_fp32 = c.ops.depthwise_se_gate(*args)
    ys, wg, gate = c.ops.depthwise_se_gate_weights(*args, c.put(wp), want_gate=True)
    hi = y_fp32.to(torch.bfloat16)                                 # the split output is the split of the fp32 kernel's, bit for bit
    assert torch.equal(ys.hi.contiguous(), hi) and torch.equal(ys.lo.contiguous(), (y_fp32 - hi.float()).to(torch.bfloat16))
    assert torch.equal(gate, g_fp32) and rel_dev(gate, gref) < TOL and rel_dev(y_fp32, d) < TOL
    c.out(y_fp32, g_fp32)
    out, outs = c.ops.pointwise_hl(ys, wg, c.put(bp), 0, residual=c.cl(res), out_fp32=True, out_split=True)
    assert rel_dev(out, ref) < SPLIT_TOL and rel_dev(outs.float(), ref) < SPLIT_TOL
    c.out(ys, gate, out, outs)
    # the per-image packed weights: every element of every image's matrix is written (the pad rows / columns as zero)
    c.out(wg.packed)


for _k, _s in [(3, 1), (3, 2), (5, 1), (5, 2)]:
    def _expand_dw_row(c, k=_k, s=_s):
        B, H, W, Cin, mid = 2, 17, 23, 24, 144
        R = Cin // 4
        x = rnd("x", (B, Cin, H, W), 1)
        we, be = rnd("we", (mid, Cin), 2, 1 / math.sqrt(Cin)), rnd("be", (mid,), 3, 0.3)
        wd, bd = rnd("wd", (mid, 1, k, k), 4, 0.3), rnd("bd", (mid,), 5, 0.2)
        w1, b1 = rnd("w1", (R, mid), 6, 1 / math.sqrt(mid)), rnd("b1", (R,), 7, 0.3)
        w2, b2 = rnd("w2", (mid, R), 8, 1 / math.sqrt(R)), rnd("b2", (mid,), 9, 0.3)
        e = F.silu(F.conv2d(x.double(), we.double()[:, :, None, None], be.double())).float()
        ref = F.silu(F.conv2d(_same_pad(e, k, s), wd, bd, stride=s, groups=mid))
        y, g = c.ops.expand_depthwise_se_gate(c.cl(x), _split_weight(c, we), c.put(be), c.put(wd.flatten(1).t().contiguous()), c.put(bd), k, s,
                                              c.put(w1), c.put(b1), c.put(w2.t().contiguous()), c.put(b2))
        assert rel_dev(y, ref) < SPLIT_TOL and rel_dev(g, _gate_ref(ref, w1, b1, w2, b2)) < SPLIT_TOL
        c.out(y, g)
    row(f"expand_depthwise_fused|k{_k}s{_s}")(_expand_dw_row)


for _shape in [(1, 8, 1, 3, 2), (2, 144, 60, 80, 6)]:               # one split / 16 splits of the pixel axis per image
    def _mean_row(c, shape=_shape):
        B, C, H, W, R = shape
        x = rnd("x", (B, C, H, W), 1)
        w1, b1 = rnd("w1", (R, C), 2, 1 / math.sqrt(C)), rnd("b1", (R,), 3, 0.3)
        w2, b2 = rnd("w2", (C, R), 4, 1 / math.sqrt(R)), rnd("b2", (C,), 5, 0.3)
        xg = c.cl(x)
        m = c.ops.channel_mean_nhwc(xg)
        assert rel_dev(m, x.mean((2, 3))) < TOL
        g = c.ops.se_gate(xg, c.put(w1), c.put(b1), c.put(w2.t().contiguous()), c.put(b2))
        assert rel_dev(g, torch.sigmoid(F.silu(x.mean((2, 3)) @ w1.T + b1) @ w2.T + b2)) < TOL
        c.out(m, g)
    row(f"channel_mean_and_se_gate|{_shape}")(_mean_row)


# =====================================================================================================================
# tokens and heads
# =====================================================================================================================
for _M, _N, _K in [(37, 64, 24), (1, 32, 8)]:
    def _linear_row(c, M=_M, N=_N, K=_K):
        x, w, b = rnd("x", (M, K), 1), rnd("w", (N, K), 2, 1 / math.sqrt(K)), rnd("b", (N,), 3, 0.1)
        ref = F.leaky_relu(x.double() @ w.double().T + b.double(), 0.01)
        y = c.ops.linear(c.put(x), c.put(w), c.put(b), 2)
        sw = c.ops.SplitWeight3(c.put(w))                            # packs on the device: ocv_pack_split3_fwd, guarded too
        y3 = c.ops.linear_split3(c.put(x), sw, c.put(b), 2)
        assert rel_dev(y, ref) < TOL and rel_dev(y3, ref) < TOL
        c.out(y, y3, sw.packed)
    row(f"linear+linear_split3|{(_M, _N, _K)}")(_linear_row)


@row("linear_residual_layernorm|(45,128)")
def _lrl_row(c):
    M, K = 45, 128
    a, w, b = rnd("a", (M, K), 1), rnd("w", (128, K), 2, 1 / math.sqrt(K)), rnd("b", (128,), 3)
    res, g, be = rnd("r", (M, 128), 4), 1 + 0.1 * rnd("g", (128,), 5), rnd("be", (128,), 6)
    ref = restate.layer_norm(res + a @ w.T + b, g, be)
    mask = (torch.arange(M) % 3 == 1)
    dev = [c.put(t) for t in (a, w, b, res, g, be)]
    y = c.ops.linear_residual_layernorm(*dev)
    ym = c.ops.linear_residual_layernorm(*dev, zero_row_mask=c.put(mask.to(torch.uint8)))
    assert rel_dev(y, ref) < TOL and rel_dev(ym, ref.masked_fill(mask[:, None], 0.0)) < TOL
    # the split3 form of the same unit has no wrapper: straight through the C ABI
    sw = c.ops.SplitWeight3(dev[1])
    y3 = torch.empty(M, 128, dtype=torch.float32, device=DEV)
    rc = c.lib.ocv_linear_residual_layernorm_split3_fwd(dev[0].data_ptr(), K, sw.packed.data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), 128,
                                                        dev[4].data_ptr(), dev[5].data_ptr(), 1e-5, None, y3.data_ptr(), 128, M, 128, K, c.stream())
    assert rc == 0, c.lib.ocv_last_error()
    assert rel_dev(y3, ref) < TOL
    c.out(y, ym, y3)


for _M, _FF in [(33, 256), (45, 1024)]:
    def _ffn_row(c, M=_M, FF=_FF):
        x = rnd("x", (M, 128), 1)
        w1, b1 = rnd("w1", (FF, 128), 2, 1 / math.sqrt(128)), rnd("b1", (FF,), 3, 0.1)
        w2, b2 = rnd("w2", (128, FF), 4, 1 / math.sqrt(FF)), rnd("b2", (128,), 5, 0.1)
        g, be = 1 + 0.1 * rnd("g", (128,), 6), rnd("be", (128,), 7)
        ref = restate.layer_norm((x.double() + torch.relu(x.double() @ w1.double().T + b1.double()) @ w2.double().T + b2.double()).float(), g, be)
        mask = (torch.arange(M) % 4 == 2)
        xg, w1g, b1g, w2g, b2g, gg, bg = (c.put(t) for t in (x, w1, b1, w2, b2, g, be))
        mg = c.put(mask.to(torch.uint8))
        y = c.ops.ffn_residual_layernorm(xg, w1g, b1g, w2g, b2g, gg, bg)
        ym = c.ops.ffn_residual_layernorm(xg, w1g, b1g, w2g, b2g, gg, bg, zero_row_mask=mg)
        p1, p2 = c.ops.SplitWeight3(w1g), c.ops.SplitWeight3(w2g)
        y3 = c.ops.ffn_residual_layernorm_split3(xg, p1, b1g, p2, b2g, gg, bg)
        y3m = c.ops.ffn_residual_layernorm_split3(xg, p1, b1g, p2, b2g, gg, bg, zero_row_mask=mg)
        masked = ref.masked_fill(mask[:, None], 0.0)
        assert rel_dev(y, ref) < TOL and rel_dev(y3, ref) < TOL and rel_dev(ym, masked) < TOL and rel_dev(y3m, masked) < TOL
        c.out(y, ym, y3, y3m)
    row(f"ffn_residual_layernorm|both forms|{(_M, _FF)}")(_ffn_row)


@row("layernorm|(17,96)")
def _layernorm_row(c):
    x, r = rnd("x", (17, 96), 1, 3.0), rnd("r", (17, 96), 2)
    g, b = 1 + 0.1 * rnd("g", (96,), 3), rnd("b", (96,), 4)
    y = c.ops.layernorm(c.put(x), c.put(g), c.put(b), 1e-5, c.put(r))
    y2 = c.ops.layernorm(c.put(x), c.put(g), c.put(b))
    assert rel_dev(y, restate.layer_norm(x + r, g, b)) < TOL and rel_dev(y2, restate.layer_norm(x, g, b)) < TOL
    c.out(y, y2)


for _form in ("h2", "fp32"):
    def _attention_row(c, form=_form):
        B, Sq, Sk = 3, 129, 77
        q, k, v = rnd("q", (B, Sq, 128), 1, 1.5), rnd("k", (B, Sk, 128), 2, 1.5), rnd("v", (B, Sk, 128), 3)
        n_valid = torch.tensor([max(1, (Sk * (b + 1)) // (B + 1)) for b in range(B)])
        mask = torch.arange(Sk)[None, :] >= n_valid[:, None]
        with env(OCV_ATTN_FORM=form):
            got = c.ops.attention_core(c.put(q), c.put(k), c.put(v), c.put(mask), 4)
            plain = c.ops.attention_core(c.put(q), c.put(k), c.put(v), None, 4)
        c.ops.attention_form_sync()                                   # back to the environment's form
        assert rel_dev(got, _attn_ref(q, k, v, mask, 4)) < TOL and rel_dev(plain, _attn_ref(q, k, v, None, 4)) < TOL
        c.out(got, plain)
    row(f"attention_core|{_form}|(3,129,77)")(_attention_row)


def _mha_case(B, Sq, Sk, counts):
    E = 128
    qs, ks, vs = rnd("qs", (B, Sq, E), 1), rnd("ks", (B, Sk, E), 2), rnd("vs", (B, Sk, E), 3)
    iw, ib = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    mask = None if counts is None else torch.arange(Sk)[None, :] >= torch.tensor(counts)[:, None]
    return (qs, ks, vs, iw, ib, ow, ob, mask), restate.multi_head_attention(qs, ks, vs, iw, ib, ow, ob, mask)


def _mha_check(got, ref, counts):
    got = got.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan) and bool(nan.any()) == bool(counts and 0 in counts)
    assert rel_dev(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(ref), ref)) < TOL


for _tokens in ("h2", "split3", "fp32"):
    def _mha_few_row(c, tokens=_tokens):
        """test_mha_split3's (45, 300, [5, 0], 5): at most 32 live keys, an image without one (NaN rows as torch)."""
        counts = [5, 0]
        args, ref = _mha_case(2, 45, 300, counts)
        dev = [c.put(t) for t in args]
        with env(OCV_TOKENS=tokens):
            got = c.ops.mha(*dev, kv_limit=5, packed={} if tokens != "fp32" else None)
        _mha_check(got, ref, counts)
        c.out(got)
        want = {"h2": "ocv_mha_few_keys_h2_fwd", "split3": "ocv_mha_split3_fwd", "fp32": "ocv_mha_fwd"}[tokens]
        assert want in c.g.calls, c.g.calls
    row(f"mha|few keys, a zero count|{_tokens}")(_mha_few_row)

    def _mha_row(c, tokens=_tokens):
        counts = [45, 17, 1]
        args, ref = _mha_case(3, 33, 45, counts)
        dev = [c.put(t) for t in args]
        with env(OCV_TOKENS=tokens):
            got = c.ops.mha(*dev, packed={} if tokens != "fp32" else None)
        _mha_check(got, ref, counts)
        c.out(got)
    row(f"mha|(3,33,45) masked|{_tokens}")(_mha_row)


def _guard_module(c, m):
    """A module's parameters as guarded device tensors."""
    m = m.cuda()
    for p in m.parameters():
        p.data = c.put(p.data)
    return m


for _mode in ("h2", "split3", "fp32"):
    def _stack_row(c, mode=_mode):
        """test_transformer_encoder_stack (3, 40, [40, 7, 1]) at its 5e-5; fp32: four ocv_encoder_layer_fwd calls."""
        from objcavit_amd.modules.layers import HipEncoderStack
        B, S, counts = 3, 40, [40, 7, 1]
        enc, sd = _encoder_sd(11)
        x = rnd("x", (B, S, 128), 12)
        mask = torch.arange(S)[None, :] >= torch.tensor(counts)[:, None]
        ref = restate.transformer_encoder(x, sd, "", mask)
        stack = HipEncoderStack(_guard_module(c, enc))
        mg = c.put(mask)
        with env(OCV_TOKENS=mode):
            got = stack(c.put(x), mg)
        assert rel_dev(got, ref) < 5e-5
        assert float(got[mg].abs().max()) == 0.0
        c.out(got)
        assert ("ocv_encoder_layer_fwd" if mode == "fp32" else "ocv_encoder_stack_fwd") in c.g.calls
    row(f"transformer_encoder_stack|{_mode}")(_stack_row)


def _patch_case(B, C, h, w, E, pos_mode):
    x = rnd("x", (B, C, h, w), 1)
    wt, b = rnd("w", (E, C, 16, 16), 2, 1 / math.sqrt(C * 256)), rnd("b", (E,), 3, 0.1)
    S = (h // 16) * (w // 16)
    pos = {"none": None, "shared": rnd("p", (S, E), 4), "batched": rnd("p", (B, S, E), 4)}[pos_mode]
    ref = F.conv2d(x.double(), wt.double(), b.double(), stride=16).flatten(2).permute(0, 2, 1)
    return x, wt, b, pos, (ref if pos is None else ref + pos.double())


@row("patch_embed|(3,37,53)")
def _patch_embed_row(c):
    x, wt, b, pos, ref = _patch_case(3, 128, 37, 53, 128, "batched")
    y = c.ops.patch_embed(c.put(x), c.put(wt), c.put(b), c.put(pos))
    y2 = c.ops.patch_embed(c.cl(x), c.cl(wt), c.put(b), c.put(pos))           # channels_last map and weight
    assert rel_dev(y, ref) < TOL and rel_dev(y2, ref) < TOL
    c.out(y, y2)


for _shape in [(1, 64, 37, 53, 40), (1, 32, 16, 16, 40), (3, 32, 48, 50, 128)]:     # ragged (B = 1) / the smallest / three images
    for _f16 in (False, True):
        def _patch_split_row(c, shape=_shape, f16=_f16):
            B, C, h, w, E = shape
            x, wt, b, pos, ref = _patch_case(B, C, h, w, E, "shared")
            assert c.ops.patch_embed_split_supported(B, C, h, w, E)
            prep = c.weights(*c.ops.prep_patch_embed_weight(wt.cuda(), f16))
            y = c.ops.patch_embed_split(c.split(x, f16), prep[0], prep[1], c.put(b), c.put(pos), oscale=prep[2] if f16 else None)
            assert rel_dev(y, ref) < (F16_TOL if f16 else SPLIT_TOL)
            c.out(y)
        row(f"patch_embed_split|{_shape}|{'f16' if _f16 else 'bf16'}")(_patch_split_row)


@row("pixel_dot|(3,37,53)")
def _pixel_dot_row(c):
    feat, q = rnd("f", (3, 128, 37, 53), 1), rnd("q", (3, 300, 128), 2)
    ref = restate.pixel_wise_dot_product(feat, q[:, 1:129, :])
    qg = c.put(q)[:, 1:129, :]
    y, y2 = c.ops.pixel_dot(c.put(feat), qg), c.ops.pixel_dot(c.cl(feat), qg)
    assert rel_dev(y, ref) < TOL and rel_dev(y2, ref) < TOL
    c.out(y, y2)


def _bin_case():
    import test_hip_bin_stats as tbs
    return tbs, tbs._case((5, 37, 53), "stress")


for _route in ("nchw", "nhwc_exact", "h2", "h2dense", "split3", "bf16_pairs"):
    def _bin_head_row(c, route=_route):
        """test_bin_head's depth bar (1e-4 max-rel) and test_bin_head_stats's bars, B = 5 on a ragged 37 x 53 map."""
        tbs, case = _bin_case()
        feat = case["feat"] if route == "nchw" else case["feat"].contiguous(memory_format=CL)
        args = (c.put(feat), c.put(case["q"])[:, 1:129, :], c.put(case["wout"]), c.put(case["bout"]), c.put(case["centers"]))
        envs = {"OCV_BINHEAD": route} if route in ("h2", "h2dense", "split3") else {"OCV_BINHEAD": "h2"}
        scope = c.ops.bf16_pairs() if route == "bf16_pairs" else contextlib.nullcontext()
        with env(**envs), scope:
            plain = c.ops.bin_head(*args, exact=route == "nhwc_exact")
            depth, var, pmax = c.ops.bin_head(*args, exact=route == "nhwc_exact", stats=True)
        d64, var64, pmax64 = case["ref64"]
        assert torch.equal(depth, plain) and max_rel(depth, d64) < 1e-4
        e_var, e_pmax = float((var.cpu().double() - var64).abs().max()), float((pmax.cpu().double() - pmax64).abs().max())
        assert e_var <= 2.0 * case["e32_var"] + tbs.SKIP * tbs.SPAN2 and e_pmax <= 2.0 * case["e32_pmax"] + tbs.SKIP + tbs.ULP1
        c.out(plain, depth, var, pmax)
    row(f"bin_head|{_route}")(_bin_head_row)


@row("bin_head|one-call and folded entry points")
def _bin_head_legacy_row(c):
    """ocv_bin_head_fwd (fold + head in one call) and ocv_bin_head_folded_fwd (no partials argument): the exact-fp32 layouts."""
    tbs, case = _bin_case()
    B, Cc, h, w = case["feat"].shape
    d64 = case["ref64"][0]
    q = c.put(case["q"])[:, 1:129, :]
    w2, bout, centers = c.put(case["wout"].reshape(256, 128)), c.put(case["bout"]), c.put(case["centers"])
    nb = c.lib.ocv_bin_head_workspace_bytes(B, 256, Cc)
    for cl, feat in ((0, c.put(case["feat"])), (1, c.put(case["feat"].contiguous(memory_format=CL)))):
        ws = c.ops.workspace(nb, feat.device, "bin_head")
        depth = torch.empty(B, 1, h, w, dtype=torch.float32, device=DEV)
        rc = c.lib.ocv_bin_head_fwd(feat.data_ptr(), cl, q.data_ptr(), q.stride(0), q.stride(1), w2.data_ptr(), bout.data_ptr(), centers.data_ptr(),
                                    depth.data_ptr(), B, Cc, 128, 256, h * w, ws.data_ptr(), ws.numel(), c.stream())
        assert rc == 0, c.lib.ocv_last_error()
        ws2 = c.ops.workspace(nb, feat.device, "bin_head")
        wf = ws2.view(torch.float32)
        assert c.lib.ocv_bin_head_fold_fwd(q.data_ptr(), q.stride(0), q.stride(1), w2.data_ptr(), wf.data_ptr(), B, Cc, 128, 256, c.stream()) == 0
        depth2 = torch.empty(B, 1, h, w, dtype=torch.float32, device=DEV)
        rc = c.lib.ocv_bin_head_folded_fwd(feat.data_ptr(), cl, wf.data_ptr(), bout.data_ptr(), centers.data_ptr(), depth2.data_ptr(), B, Cc, 256,
                                           h * w, c.stream())
        assert rc == 0, c.lib.ocv_last_error()
        assert max_rel(depth, d64) < 1e-4 and max_rel(depth2, d64) < 1e-4
        c.out(depth, depth2)


for _norm in ("linear", "sigmoid"):
    def _regressor_row(c, norm=_norm):
        B, E, H1, H2, n = 3, 64, 100, 36, 80
        tok = rnd("tok", (B, 7, E), 1)
        par = [rnd("w1", (H1, E), 2, 1 / math.sqrt(E)), rnd("b1", (H1,), 3, 0.2), rnd("w2", (H2, H1), 4, 1 / math.sqrt(H1)), rnd("b2", (H2,), 5, 0.2),
               rnd("w3", (n, H2), 6, 2 / math.sqrt(H2)), rnd("b3", (n,), 7, 0.2)]
        head = c.put(tok)[:, 0, :]
        w, e, ce = c.ops.regressor_bins(head, *[c.put(t) for t in par], norm, 0.001, 10.0)
        y = F.leaky_relu(tok[:, 0, :].double() @ par[0].double().T + par[1].double(), 0.01)
        y = F.leaky_relu(y @ par[2].double().T + par[3].double(), 0.01)
        y = y @ par[4].double().T + par[5].double()
        raw = y.float()
        y = torch.relu(y) + 0.1 if norm == "linear" else torch.sigmoid(y)
        wr = y / y.sum(1, keepdim=True)
        er = torch.cumsum(F.pad((10.0 - 0.001) * wr, (1, 0), value=0.001), 1)
        cr = 0.5 * (er[:, :-1] + er[:, 1:])
        assert rel_dev(w, wr.float()) < 2e-6 and rel_dev(e, er.float()) < 2e-6 and rel_dev(ce, cr.float()) < 2e-6      # test_regressor_bins_one_launch
        w2, e2, c2 = c.ops.bin_edges(c.put(raw), norm, 0.001, 10.0)
        assert rel_dev(w2, wr.float()) < 2e-6 and rel_dev(e2, er.float()) < 2e-6 and rel_dev(c2, cr.float()) < 2e-6
        c.out(w, e, ce, w2, e2, c2)
    row(f"regressor_bins+bin_edges|{_norm}")(_regressor_row)


@row("pos_grid_sample|(2,1,7)")
def _pos_row(c):
    """test_pos_grid_sample_vs_oracle's smallest grid: centre mode (a strided column slice, then with the addend), RoI mode, image tokens."""
    gh, gw, E = 2, 1, 7
    fh, fw, patch, seed = gh * 16, gw * 16, 16, 11 * gh + gw
    table = gen.uniform("tab", (gh * gw + 3, E), seed)
    H, W, n = 2 * fh, 2 * fw, 50
    rs = np.random.RandomState(seed)
    xywh = torch.from_numpy(np.stack([rs.uniform(-0.2 * W, 1.3 * W, n), rs.uniform(-0.2 * H, 1.3 * H, n),
                                      rs.uniform(0.5, 1.5 * W, n), rs.uniform(0.5, 1.5 * H, n)], 1).astype(np.float32))
    xywh[0] = -1.0
    add = rnd("add", (n, E), seed)
    tg, xg = c.put(table), c.put(xywh)
    ref = restate.grid_random_pos_emb(table, xywh[:, 0:2], (fh, fw), patch, "centre", "obj")
    a = c.ops.pos_grid_sample(tg, gh, gw, xg[:, 0:2], c.ops.POS_CENTRE_OBJ, fh * 2.0, fw * 2.0)
    b = c.ops.pos_grid_sample(tg, gh, gw, xg, c.ops.POS_CENTRE_OBJ, fh * 2.0, fw * 2.0, addend=c.put(add))
    assert float((a.cpu() - ref).abs().max()) < 1e-5 and float((b.cpu() - (ref + add)).abs().max()) < 1e-5
    ref = restate.grid_random_pos_emb(table, xywh, (fh, fw), patch, "roi_align", "obj")
    r = c.ops.pos_grid_sample(tg, gh, gw, xg, c.ops.POS_ROI, 1.0 / 32.0)
    assert torch.equal(torch.isnan(r.cpu()), torch.isnan(ref)) and float((r.cpu().nan_to_num(-7.0) - ref.nan_to_num(-7.0)).abs().max()) < 1e-5
    pc = restate.patch_coords(2, gh, gw, patch)
    S = gh * gw
    ref = restate.grid_random_pos_emb(table, pc[..., 0:2], (fh, fw), patch, "centre", "img")
    i = c.ops.pos_grid_sample(tg, gh, gw, c.put(pc.reshape(2 * S, 4)), c.ops.POS_CENTRE_IMG, gh, gw, rows_per_image=S)
    assert float((i.cpu().view(2, S, E) - ref).abs().max()) < 1e-5
    c.out(a, b, r, i)


@row("object pads|a zero count")
def _object_pad_row(c):
    """test_object_pad_kernels_vs_reference_formulation with an image without objects: it keeps ONE live key, the PAD row
    (test_object_pad_stray_counts_keep_one_defined_key)."""
    PAD, counts, cap, S, E = 0.0001, [0, 3, 5], 5, 20, 128
    B = len(counts)
    tok = torch.full((B, cap, E), float("nan"))
    for i, n in enumerate(counts):
        tok[i, :n] = rnd(f"o{i}", (n, E), 5)
    cnt = c.put(torch.tensor(counts, dtype=torch.int32))
    out, mask = c.ops.object_tokens_pad(c.put(tok), cnt, PAD)
    live = torch.tensor([max(n, 1) for n in counts])
    want = torch.where((torch.arange(cap)[None] < torch.tensor(counts)[:, None])[:, :, None], tok, torch.full_like(tok, PAD))
    assert torch.equal(out.cpu(), want) and torch.equal(mask.cpu().bool(), torch.arange(cap)[None] >= live[:, None])
    enc = rnd("enc", (B, cap, E), 6)
    keys, kpm = c.ops.object_front_pad(c.put(enc), cnt, S, PAD)
    n = max(counts)
    r_keys = F.pad(enc[:, :n], (0, 0, S - n, 0), value=PAD)
    r_mask = F.pad(torch.arange(n)[None] >= live[:, None], (0, S - n), value=True)
    assert torch.equal(keys[1:].cpu(), r_keys[1:]) and torch.equal(kpm.cpu().bool(), r_mask)
    assert bool((keys[0, :S - n] == PAD).all())
    c.out(out, mask, keys, kpm)


@row("object_frontend|a zero count")
def _object_frontend_row(c):
    """test_dense_class_table_equals_index_select: seven images, the last without a detection (served the <UNK> row)."""
    import test_hip_object_frontend as tof
    golden = tof._Golden()
    table = rnd("dense", (tof.NCLS, 512), 8)
    dets = golden.dets(capacity=16)
    xywh, cls, counts = c.put(dets.xywh), c.put(dets.cls), c.put(dets.counts)
    f, x, cn, rows, keys, flags = c.ops.object_frontend(xywh, cls, counts, class_table=c.put(table))
    live = torch.arange(16, device=DEV)[None, :] < counts[:, None]
    want = table.cuda().index_select(0, cls.long().flatten()).view(7, 16, 512) * live[:, :, None]
    want_x = xywh * live[:, :, None]
    want_x[6, 0] = -1.0
    assert torch.equal(f, want) and torch.equal(x, want_x) and cn.tolist() == [12, 3, 13, 2, 1, 2, 1] and int(flags.max()) == 0
    assert torch.equal(rows, torch.where(live, cls, torch.full_like(cls, -1)))
    c.out(f, x, cn, rows, keys.view(torch.int64), flags)


@row("range_flag_take")
def _range_flag_row(c):
    guard = c.ops.RangeGuard(torch.device(DEV))
    guard.flag.fill_(1)
    taken = guard.take()
    assert c.ops.RangeGuard.tripped(taken) and int(guard.flag.item()) == 0
    c.out(taken)


# =====================================================================================================================
# frames in, maps out, metrics
# =====================================================================================================================
@row("frame_ingest|(2,37,53) window, mirror")
def _frame_ingest_row(c):
    import predict_ref
    from objcavit_amd.config import make_args
    from objcavit_amd.predict import normalisation_table
    args = make_args()
    top, left, H, W = 4, 5, 31, 45
    f = torch.randint(0, 256, (2, 37, 53, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(11))
    ref = predict_ref.frames_to_input(f, args, top, left, H, W)
    table = c.put(normalisation_table(args))
    got = c.ops.frame_ingest(c.put(f), table, top, left, (H, W), mirror_too=True)
    assert torch.equal(got[:2].cpu(), ref) and torch.equal(got[2:].cpu(), ref.flip(3))
    one = c.ops.frame_ingest(c.put(f), table, top, left, (H, W))
    assert torch.equal(one.cpu(), ref)
    c.out(got, one)


@row("depth_ingest|(2,37,53) window")
def _depth_ingest_row(c):
    import predict_ref
    d = torch.from_numpy(torch.randint(0, 65536, (2, 37, 53), generator=torch.Generator().manual_seed(3)).numpy().astype(np.uint16))
    got = c.ops.depth_ingest(c.put(d), 1000.0, 4, 5, (31, 45))
    whole = c.ops.depth_ingest(c.put(d), 256.0)
    assert torch.equal(got.cpu(), predict_ref.depth_to_metres(d, 1000.0, 4, 5, 31, 45))
    assert torch.equal(whole.cpu(), predict_ref.depth_to_metres(d, 256.0, 0, 0, 37, 53))
    c.out(got, whole)


for _mirror in (False, True):
    def _finalize_row(c, with_mirror=_mirror):
        """test_depth_finalize_vs_float64_and_its_integer_forms at 17 x 23 -> 45 x 61."""
        import predict_ref
        from test_hip_predict import _pred
        B, h, w, H, W, dmin, dmax = 2, 17, 23, 45, 61, 0.001, 10.0
        pred = _pred("p", B, h, w, dmin, dmax, 1)
        mirror = _pred("m", B, h, w, dmin, dmax, 2) if with_mirror else None
        table = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
        res = c.ops.depth_finalize(c.put(pred), dmin, dmax, (H, W), pred_mirror=c.put(mirror), want=("depth", "depth_u16", "rgb8"),
                                   u16_scale=1000.0, colormap=c.put(table), vmin=dmin, vmax=dmax)
        d = res["depth"]
        assert rel_dev(d, predict_ref.final_depth(pred, mirror, dmin, dmax, H, W, torch.float64)) < TOL
        assert torch.equal(res["depth_u16"].cpu().to(torch.int32), predict_ref.to_u16(d[:, 0], 1000.0))
        assert torch.equal(res["rgb8"].cpu(), predict_ref.to_rgb8(d[:, 0], table, dmin, dmax))
        c.out(d, res["depth_u16"], res["rgb8"])
    row(f"depth_finalize|{'mirror' if _mirror else 'plain'}")(_finalize_row)

    def _finalize_stats_row(c, mirror=_mirror):
        """test_depth_finalize_stats at 17 x 23 -> 45 x 61."""
        import bin_stats_ref
        import test_hip_bin_stats as tbs
        B, h, w, H, W = 2, 17, 23, 45, 61
        d, var, pmax = tbs._maps(7, B, h, w)
        dm, varm, pmaxm = tbs._maps(8, B, h, w) if mirror else (None, None, None)
        std64, conf64, _, _ = bin_stats_ref.full_stats(d, var, pmax, dm, varm, pmaxm, (H, W))
        std32, conf32, _, _ = bin_stats_ref.full_stats(d, var, pmax, dm, varm, pmaxm, (H, W), dtype=torch.float32)
        got = c.ops.depth_finalize(c.put(d), tbs.DMIN, tbs.DMAX, (H, W), want=("depth", "depth_std", "confidence"), pred_mirror=c.put(dm),
                                   var=c.put(var), pmax=c.put(pmax), var_mirror=c.put(varm), pmax_mirror=c.put(pmaxm))
        for name, r64, r32 in (("depth_std", std64, std32), ("confidence", conf64, conf32)):
            e32 = float((r32.double() - r64).abs().max())
            err = (got[name].cpu().double() - r64).abs()
            assert bool((err <= 2.0 * e32 + 2.0 * tbs.ULP1 * r64.abs()).all()), (name, float(err.max()), e32)
        c.out(got["depth"], got["depth_std"], got["confidence"])
    row(f"depth_finalize|stats|{'mirror' if _mirror else 'plain'}")(_finalize_stats_row)


@row("depth_metrics+depth_metrics_loss|(3,11,13->37,29)")
def _metrics_row(c):
    """test_depth_metrics_vs_oracle and test_depth_metrics_loss_vs_loss_ref at their (3, 11, 13, 37, 29, mirror) case."""
    import loss_ref as lr
    from oracle import validation_ref as vr
    from test_hip_val_loss import field_devs
    B, h, w, H, W = 3, 11, 13, 37, 29
    g = torch.Generator().manual_seed(B * 1000 + H)
    gt = torch.rand(B, 1, H, W, generator=g) * 12.0 - 1.0
    pa = torch.rand(B, 1, h, w, generator=g) * 11.0 + 0.1
    pb = torch.rand(B, 1, h, w, generator=g) * 11.0 + 0.1
    pa[0, 0, 1, 1] = float("nan")
    gt[1] = -1.0
    ref = vr.per_image_records(pa, gt, 0.001, 10.0, depth_pred_mirror=pb, first_image_id=3)
    got = c.ops.depth_metrics(c.put(pa), c.put(gt), 0.001, 10.0, pred_mirror=c.put(pb), first_image_id=3)
    assert torch.equal(got[:, 8:].cpu(), ref[:, 8:]) and rel_dev(got[:, :8], ref[:, :8]) < TOL
    g = torch.Generator().manual_seed(B * 1000 + H)
    gt = torch.rand(B, 1, H, W, generator=g) * 12.0 - 1.0
    pa = torch.rand(B, 1, h, w, generator=g) * 4.0 + 0.1
    pb = torch.rand(B, 1, h, w, generator=g) * 4.0 + 0.1
    gt[1] = -1.0
    edges = lr.clustered_edges(B, 256, 0.001, 10.0, H)
    box = (H // 4, H - H // 8, W // 8, W)
    rec, lrec = c.ops.depth_metrics_loss(c.put(pa), c.put(gt), c.put(edges), 0.001, 10.0, crop=box, pred_mirror=c.put(pb), first_image_id=3)
    devs = field_devs(lrec, lr.loss_records(pa, pb, gt, edges, 0.001, 10.0, first_image_id=3), "guarded")
    assert max(devs.values()) < TOL, devs
    rec2 = c.ops.depth_metrics(c.put(pa), c.put(gt), 0.001, 10.0, crop=box, pred_mirror=c.put(pb), first_image_id=3)
    assert torch.equal(rec, rec2)
    c.out(got, rec, lrec, rec2)


@row("object_depth")
def _object_depth_row(c):
    import object_depth_ref as odr
    from test_hip_object_depth import _check
    q = (0.1, 0.5, 0.9)
    depth, std = odr.case_map("uniform"), odr.case_map("uniform", seed=2)
    name = sorted(odr.BOX_SETS)[0]
    xywh4, counts = odr.case_boxes(name, 4)
    xywh6, _ = odr.case_boxes(name, 6)
    dg, sg, cg = c.put(depth), c.put(std), c.put(counts)
    for shrink in (1.0, 0.3):
        want = odr.object_depth(depth, xywh4, counts, std, q, shrink)
        got = c.ops.object_depth(dg, c.put(xywh4), cg, depth_std=sg, quantiles=q, shrink=shrink)
        _check(got, want, 3, (name, shrink))
        strided = c.ops.object_depth(dg, c.put(xywh6)[:, :, :4], cg, depth_std=sg, quantiles=q, shrink=shrink)
        assert torch.equal(strided.view(torch.int32), got.view(torch.int32))
        c.out(got, strided)


@row("object_metrics")
def _object_metrics_row(c):
    import object_depth_ref as odr
    import object_metrics_ref as omr
    from test_hip_object_metrics import _check
    pred, mirror, gt = omr.case_maps(seed=1)
    name = sorted(odr.BOX_SETS)[0]
    xywh6, counts = odr.case_boxes(name, 6)
    box = omr.GARG_STYLE(odr.CASE_H, odr.CASE_W)
    for shrink, crop in ((1.0, None), (0.3, box)):
        want_b, want_r = omr.object_metrics(pred, gt, xywh6[..., :4], counts, crop=crop, pred_mirror=mirror, shrink=shrink)
        boxes, regions = c.ops.object_metrics(c.put(pred), c.put(gt), c.put(xywh6), c.put(counts), omr.MIN_DEPTH, omr.MAX_DEPTH, crop=crop,
                                              pred_mirror=c.put(mirror), shrink=shrink)
        _check(boxes, want_b, (name, shrink, "boxes"))
        _check(regions, want_r, (name, shrink, "regions"))
        alone, none = c.ops.object_metrics(c.put(pred), c.put(gt), c.put(xywh6), c.put(counts), omr.MIN_DEPTH, omr.MAX_DEPTH, crop=crop,
                                           pred_mirror=c.put(mirror), shrink=shrink, regions=False)
        assert none is None and torch.equal(alone.view(torch.int32), boxes.view(torch.int32))
        c.out(boxes, regions, alone)


for _stride in [(1, 1), (2, 3)]:
    def _unproject_row(c, stride=_stride):
        """test_points_equal_the_reference / test_every_combination_...: B 3, 61 x 83, capacity above and below the totals; the rows at or
        beyond counts[b] are documented as NOT written: they must still hold the harness's pattern."""
        import point_cloud_ref as pcr
        depth, K = pcr.case_depth("random_half"), pcr.case_intrinsics()
        conf, frames = pcr.case_confidence(), pcr.case_frames(1, pcr.CASE_B, pcr.CASE_H, pcr.CASE_W)
        want = pcr.unproject(depth, K, stride, pcr.NEAR, pcr.FAR, confidence=conf, min_confidence=0.25, frames=frames)
        totals = [w.records.shape[0] for w in want]
        dg, kg, cg, fg = c.put(depth), c.put(K), c.put(conf), c.put(frames)
        for cap in (max(totals) + 5, max(1, max(totals) // 2)):
            got = c.ops.depth_unproject(dg, kg, cap, stride=stride, near=pcr.NEAR, far=pcr.FAR, confidence=cg, min_confidence=0.25, frames=fg,
                                        want_pixel=True)
            points, pixel = got["points"].cpu(), got["pixel"].cpu()
            assert got["total"].tolist() == totals and got["counts"].tolist() == [min(t, cap) for t in totals]
            for b, w in enumerate(want):
                k = min(totals[b], cap)
                assert torch.equal(points[b, :k].view(torch.int32), w.records[:k].view(torch.int32)) and torch.equal(pixel[b, :k], w.pixel[:k])
                assert bool((points[b, k:].view(torch.int32) == mem_guard._PATTERN_I32).all()) and bool((pixel[b, k:] == mem_guard._PATTERN_I32).all())
            c.out(got["total"], got["counts"])
    row(f"depth_unproject|stride{_stride}")(_unproject_row)


# =====================================================================================================================
# the harness itself on the device (tests/test_mem_guard_host.py has the rest, on CPU tensors)
# =====================================================================================================================
def test_harness_sees_stray_stores_and_unwritten_words_on_the_device():
    """No project kernel: torch writes one element behind, and one in front of, a guarded device tensor."""
    with pytest.raises(mem_guard.Breach) as ei:
        with mem_guard.guarded("cuda") as g:
            t = torch.empty(3, 5, dtype=torch.float32, device="cuda")
            h = torch.empty(2, 64, dtype=torch.bfloat16, device=torch.device("cuda", torch.cuda.current_device()))
            assert g.never_written(t) == 15 and g.never_written(h) == 64
            t.zero_()
            h[0].zero_()
            assert g.never_written(t) == 0 and g.never_written(h) == 32
            g.check()
            torch.as_strided(t, (1,), (1,), t.storage_offset() + 15).fill_(1.0)
            torch.as_strided(h, (1,), (1,), h.storage_offset() - 1).fill_(0.0)
    msg = str(ei.value)
    assert "trailing guard of torch.empty (3, 5) torch.float32" in msg and "first at payload offset 60, last at 63 " in msg
    assert "leading guard of torch.empty (2, 64) torch.bfloat16" in msg and "first at payload offset -2, last at -1 " in msg
    assert torch.empty(2, device="cuda").data_ptr() % 256 == 0            # restored: torch's own allocation


# =====================================================================================================================
# (a) the table, (c) the accounting
# =====================================================================================================================
@pytest.mark.parametrize("name", list(ROWS))
def test_row(name):
    run_row(name)


EXEMPT = {
    "ocv_layer_tail_split3_fwd": "no Python caller; the same launch runs inside ocv_encoder_stack_fwd's guarded rows (split3); alone, tests/"
                                 "test_hip_token_units.py puts 32 sentinel rows behind its outputs",
    "ocv_layer_tail_h2_fwd": "as above (the OCV_TOKENS=h2 stack row)",
    "ocv_layer_tail_h2_ws_fwd": "as above: the form the h2 stack takes at few tokens, on a part of the stack's own workspace",
}
_NEVER_EXEMPT = ("conv", "pointwise", "depthwise", "se_gate", "channel_mean", "mbconv", "upsample", "tap")


def test_every_fwd_entry_point_ran_guarded():
    from objcavit_amd import _lib
    for name in ROWS:                                                 # (a -k selection, or another worker, ran fewer: run the rest)
        if name not in TRIED:
            run_row(name)
    failed = sorted(TRIED - set(RAN))
    assert not failed, f"rows that did not pass: {failed}"
    table = {n for n in _lib.PROTOTYPES if n.endswith("_fwd")}
    assert len(EXEMPT) <= 8
    unknown = set(EXEMPT) - table
    assert not unknown, f"EXEMPT names that are no entry points: {sorted(unknown)}"
    assert not [n for n in EXEMPT if any(k in n for k in _NEVER_EXEMPT)]
    called = set().union(*RAN.values())
    missing = table - called - set(EXEMPT)
    assert not missing, f"entry points that never ran under the harness: {sorted(missing)}"
    both = set(EXEMPT) & called
    assert not both, f"exempt, yet called by a row: {sorted(both)}"
    print(f"{len(ROWS)} rows, {len(table & called)} of {len(table)} *_fwd entry points guarded, {len(EXEMPT)} exempt")


# =====================================================================================================================
# (b) whole forwards, eager
# =====================================================================================================================
FWD_H, FWD_W = 192, 208          # the smallest size an end-to-end test runs (test_final_upscale_models_end_to_end_vs_oracle)
ENCODERS = ["efficientnet-b5", "efficientnet-b1", "efficientnet-v2-s"]
ROUTES = ["default", "bf16_pairs", "exact"]
FORWARDS = [(m, e, r, 2) for m in ("adabins", "graphbins") for e in ENCODERS for r in ROUTES] + \
           [(m, "efficientnet-b5", "default", 3) for m in ("adabins", "graphbins")]
# kernels that legitimately cannot repeat their bits from one run to the next: none known (the suite asserts run-to-run and
# replay-to-eager equality: test_two_batches_in_flight_give_the_same_bits, test_graph_replay_with_eager_island_equals_eager_dispatch)
NOT_BITWISE = {}


_MODELS = {}


def _forward_model(model, enc, exact, seed=64):
    """Built once per (model, encoder, exact route): the prepared weights are cached per route where they are made."""
    key = (model, enc, exact)
    if key not in _MODELS:
        _MODELS[key] = _build_model(model, enc, seed)
    return _MODELS[key]


def _build_model(model, enc, seed):
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.GraphBins import GraphBins
    from objcavit_amd.objects import TableObjectProvider
    args = make_args(model=model, encoder_name=enc, do_final_upscale=True, language="clip", dimensions_train=[FWD_H, FWD_W],
                     dimensions_test=[FWD_H, FWD_W])
    if model == "adabins":
        m = AdaBins(args).eval()
    else:                                                             # ragged detections, one image without any
        table = rnd("table", (40, 512), seed, 10.0 / np.sqrt(512)).cuda()
        cls = [torch.tensor([3, 17, 17, 39, 0]), None, torch.tensor([8])]
        xywh = [gen.boxes("b0", 5, seed, FWD_H, FWD_W), None, gen.boxes("b2", 1, seed, FWD_H, FWD_W)]
        prov = TableObjectProvider(lambda image: ([None if b is None else b.to(image.device) for b in xywh[:image.shape[0]]],
                                                  cls[:image.shape[0]]), class_table=table)
        m = GraphBins(args, object_provider=prov).eval()
    gen.load_into(m, seed, gen.PEAKY)
    return m.cuda()


@pytest.mark.parametrize("model,enc,route,B", FORWARDS)
def test_forward_under_the_harness(model, enc, route, B):
    from objcavit_amd import hip_ops
    envs = {"OCV_CONV": "exact", "OCV_PW": "fp32"} if route == "exact" else {}
    scope = hip_ops.bf16_pairs if route == "bf16_pairs" else contextlib.nullcontext
    img = rnd("img", (B, 3, FWD_H, FWD_W), 64).cuda()
    try:
        with env(**envs):
            m = _forward_model(model, enc, route == "exact")
            with scope():
                m(img)                                                # the model's first batch: weight caches, the fp16 pairs' calibration
                ref = m(img).depth_pred.clone()
            with mem_guard.guarded("cuda") as g:
                g.record_calls()
                with scope():
                    out = m(g.copy(img))
                depth = out.depth_pred
                torch.cuda.synchronize()
                g.check()
                assert g.never_written(depth) == 0
                print(f"{model} {enc} {route} B={B}: {len(g.calls)} calls, {len(g.arenas)} guarded allocations, "
                      f"{len(g.stray)} pointers outside them (module parameters and prepared weights)")
                assert bool(torch.isfinite(depth).all())
                key = (model, enc, route)
                if key in NOT_BITWISE:
                    assert max_rel(depth, ref) < 1e-3, NOT_BITWISE[key]
                else:
                    assert torch.equal(depth, ref)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory" in str(e) or "hipError" in str(e):
            pytest.exit(f"GPU fault in forward {model} {enc} {route}: {e}", returncode=3)
        raise
