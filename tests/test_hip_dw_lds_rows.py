"""The 5 x 5 depthwise kernel that stages its input rows once through LDS (dw_rows_kernel, csrc/depthwise_se.hip) against
the register-window kernel it replaces (dw_slide_kernel), switched by ocv_depthwise_set_dispatch in one process: the
outputs are bit-identical, both agree with the fp32 CPU formulation of tests/test_hip_kernels.py::test_depthwise_se_gate
to its tolerance, and a second call repeats the first bit for bit.  Shapes sit where the staging can go wrong: one quad
that is all halo, images smaller than the kernel, odd sizes and the asymmetric TF-SAME padding of stride 2, a width one
past a tile multiple, a ragged last channel chunk, many chunks with a tile smaller than its halo, the stage-5 row."""
import math

import pytest
import torch
import torch.nn.functional as F

import gen
from util import rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 2e-5          # tests/test_hip_kernels.py: fp32 kernels vs fp32 CPU, accumulation-order noise only
K = 5
REGISTER_WINDOW, LDS_ROWS = 1, 2

SHAPES = [(1, 4, 1, 1), (1, 8, 3, 2), (2, 12, 33, 47), (2, 144, 30, 41), (2, 1056, 9, 11), (1, 3072, 4, 5), (3, 64, 17, 40)]
HL_SHAPES = [(2, 1056, 9, 11), (3, 64, 17, 40)]


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


class dispatch:
    """``with dispatch(lib, mode):`` -- the mode holds for the size query and the launch inside, automatic afterwards."""

    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        assert self.lib.ocv_depthwise_set_dispatch(self.mode) == 0

    def __exit__(self, *exc):
        self.lib.ocv_depthwise_set_dispatch(0)
        return False


def _params(B, C, H, W):
    """The inputs of test_depthwise_se_gate (same generator keys, seeds and scales)."""
    R = max(1, C // 24)
    x, w, b = gen.randn("x", (B, C, H, W), 1), gen.randn("w", (C, 1, K, K), 2, 0.3), gen.randn("b", (C,), 3, 0.2)
    w1, b1 = gen.randn("w1", (R, C), 4, 1 / math.sqrt(C)), gen.randn("b1", (R,), 5, 0.3)
    w2, b2 = gen.randn("w2", (C, R), 6, 1 / math.sqrt(R)), gen.randn("b2", (C,), 7, 0.3)
    return x, w, b, w1, b1, w2, b2


def _same_pad(x, k, s):
    ih, iw = x.shape[-2:]
    ph = max((math.ceil(ih / s) - 1) * s + k - ih, 0)
    pw = max((math.ceil(iw / s) - 1) * s + k - iw, 0)
    return F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))


def _reference(x, w, b, w1, b1, w2, b2, s, padding=None):
    xp = _same_pad(x, K, s) if padding is None else F.pad(x, (padding[1], padding[1], padding[0], padding[0]))
    ref = F.silu(F.conv2d(xp, w, b, stride=s, groups=x.shape[1]))
    return ref, torch.sigmoid(F.silu(ref.mean((2, 3)) @ w1.T + b1) @ w2.T + b2)


def _device_args(x, w, b, w1, b1, w2, b2, s):
    return (x.cuda().contiguous(memory_format=torch.channels_last), w.cuda().flatten(1).t().contiguous(), b.cuda(), K, s,
            w1.cuda(), b1.cuda(), w2.cuda().t().contiguous(), b2.cuda())


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_lds_rows_equal_register_window(ops, B, C, H, W, s):
    lib = ops._lib.load()
    p = _params(B, C, H, W)
    ref, gref = _reference(*p, s)
    args = _device_args(*p, s)
    try:
        with dispatch(lib, REGISTER_WINDOW):
            y1, g1 = ops.depthwise_se_gate(*args)
        with dispatch(lib, LDS_ROWS):
            y2, g2 = ops.depthwise_se_gate(*args)
            y3, g3 = ops.depthwise_se_gate(*args)
    finally:
        lib.ocv_depthwise_set_dispatch(0)
    print(f"rel_dev y {rel_dev(y2, ref):.3g} gate {rel_dev(g2, gref):.3g} (register window: {rel_dev(y1, ref):.3g} {rel_dev(g1, gref):.3g})")
    assert y2.shape == ref.shape and y2.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y2, y1)
    assert rel_dev(y2, ref) < TOL and rel_dev(g2, gref) < TOL
    assert rel_dev(y1, ref) < TOL and rel_dev(g1, gref) < TOL
    assert torch.equal(y3, y2) and torch.equal(g3, g2)        # fixed-order pooling sums


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("B,C,H,W", HL_SHAPES)
def test_lds_rows_hl32_equal_register_window(ops, B, C, H, W, s):
    """The hl32 split output (C a multiple of 32), written where it is produced."""
    lib = ops._lib.load()
    p = _params(B, C, H, W)
    ref, gref = _reference(*p, s)
    args = _device_args(*p, s)
    wp = gen.randn("wp", (16, C), 8, 1 / math.sqrt(C)).cuda()
    try:
        with dispatch(lib, REGISTER_WINDOW):
            ys1, _, g1 = ops.depthwise_se_gate_weights(*args, wp, want_gate=True)
        with dispatch(lib, LDS_ROWS):
            ys2, _, g2 = ops.depthwise_se_gate_weights(*args, wp, want_gate=True)
            y2, _ = ops.depthwise_se_gate(*args)
            ys3, _, g3 = ops.depthwise_se_gate_weights(*args, wp, want_gate=True)
    finally:
        lib.ocv_depthwise_set_dispatch(0)
    assert torch.equal(ys2.hl.view(torch.int16), ys1.hl.view(torch.int16))
    hi = y2.to(torch.bfloat16)                                 # the split of the fp32 output, bit for bit
    assert torch.equal(ys2.hi.contiguous(), hi) and torch.equal(ys2.lo.contiguous(), (y2 - hi.float()).to(torch.bfloat16))
    assert rel_dev(y2, ref) < TOL and rel_dev(g2, gref) < TOL and rel_dev(g1, gref) < TOL
    assert torch.equal(ys3.hl.view(torch.int16), ys2.hl.view(torch.int16)) and torch.equal(g3, g2)


@pytest.mark.parametrize("s", [1, 2])
def test_lds_rows_explicit_padding(ops, s):
    """padding = (pad_t, pad_l), symmetric: the form of the V2 encoders."""
    lib = ops._lib.load()
    p = _params(2, 12, 33, 47)
    ref, gref = _reference(*p, s, padding=(2, 2))
    args = _device_args(*p, s)
    try:
        with dispatch(lib, REGISTER_WINDOW):
            y1, g1 = ops.depthwise_se_gate(*args, padding=(2, 2))
        with dispatch(lib, LDS_ROWS):
            y2, g2 = ops.depthwise_se_gate(*args, padding=(2, 2))
            y3, g3 = ops.depthwise_se_gate(*args, padding=(2, 2))
    finally:
        lib.ocv_depthwise_set_dispatch(0)
    assert y2.shape == ref.shape and torch.equal(y2, y1)
    assert rel_dev(y2, ref) < TOL and rel_dev(g2, gref) < TOL
    assert torch.equal(y3, y2) and torch.equal(g3, g2)


def test_lds_rows_write_every_partial(ops):
    """Every partial row of every channel is written: a workspace full of NaN leaves a finite, correct gate."""
    lib = ops._lib.load()
    p = _params(2, 144, 30, 41)
    ref, gref = _reference(*p, 1)
    args = _device_args(*p, 1)
    try:
        with dispatch(lib, LDS_ROWS):
            ops.depthwise_se_gate(*args)                       # sizes the workspace
            torch.cuda.synchronize()
            tiles = lib.ocv_depthwise_sum_tiles(2, 144, 30, 41, K, 1)
            ops.workspace(2 * tiles * 144 * 4, args[0].device, "dw_part").fill_(0xFF)      # all-ones words: NaN
            y, g = ops.depthwise_se_gate(*args)
    finally:
        lib.ocv_depthwise_set_dispatch(0)
    assert torch.isfinite(g).all() and rel_dev(g, gref) < TOL and rel_dev(y, ref) < TOL


def test_lds_rows_pass_inf_and_nan(ops):
    """An inf and a NaN input pixel reach the output (padded taps are multiplications by zero, never selects of the
    product), identically under both kernels."""
    lib = ops._lib.load()
    x, *rest = _params(2, 12, 33, 47)
    x = x.clone()
    x[0, 3, 0, 0] = float("inf")
    x[1, 7, 20, 46] = float("nan")
    args = _device_args(x, *rest, 1)
    try:
        with dispatch(lib, REGISTER_WINDOW):
            y1, _ = ops.depthwise_se_gate(*args)
        with dispatch(lib, LDS_ROWS):
            y2, _ = ops.depthwise_se_gate(*args)
    finally:
        lib.ocv_depthwise_set_dispatch(0)
    assert torch.isinf(y2[0, 3]).any() and torch.isnan(y2[1, 7]).any()
    assert torch.isfinite(y2[0, :3]).all() and torch.isfinite(y2[1, 8:]).all()        # and nowhere but in their channel
    assert torch.equal(_bits(y2), _bits(y1))


def test_dispatch_setter_rejects_unknown_modes(ops):
    lib = ops._lib.load()
    try:
        assert lib.ocv_depthwise_set_dispatch(3) == -1 and lib.ocv_depthwise_set_dispatch(-1) == -1
        for mode in (1, 2, 0):
            assert lib.ocv_depthwise_set_dispatch(mode) == 0
    finally:
        lib.ocv_depthwise_set_dispatch(0)
