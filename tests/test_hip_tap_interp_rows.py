"""-m gpu: the row form of tap_interp_kernel (csrc/tap_interp.hip: x interpolation once per source row and output column,
a block of consecutive output rows per thread) against the fp64 definition that test_hip_kernels.test_tap_interp_combine
uses, at that file's TOL, on the smallest shapes at which the row logic can go wrong.  The split outputs are compared with
the fp32 one at what their formats hold: 1e-5 for bf16 pairs (test_tap_interp_combine's bar), 3e-7 ~ 2^-22 for fp16 pairs
(test_hip_fp16_route's bar)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import gen
from util import rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 2e-5          # test_hip_kernels.TOL: fp32 kernels vs fp64, accumulation-order noise only
CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def rnd(key, shape, seed=0, scale=1.0):
    return gen.randn(key, shape, seed, scale)


def cl(t):
    return t.cuda().contiguous(memory_format=CL)


def activate(v, act):
    return [v, torch.relu(v), F.leaky_relu(v, 0.01), F.silu(v)][act]


def definition(z, s, b, H, W, act):
    """fp64: nine bilinear (align_corners) up-samplings of the tap products, each shifted by its tap with zero padding,
    + skip part + bias, activation."""
    Cout = z.shape[1] // 9
    ref = torch.zeros(z.shape[0], Cout, H, W, dtype=torch.float64)
    if s is not None:
        ref = ref + s.double()
    if b is not None:
        ref = ref + b.double().view(1, -1, 1, 1)
    for t in range(9):
        up = F.interpolate(z[:, t * Cout:(t + 1) * Cout].double(), size=(H, W), mode="bilinear", align_corners=True)
        dy, dx = t // 3 - 1, t % 3 - 1
        ref = ref + F.pad(up, (1, 1, 1, 1))[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return activate(ref, act)


@functools.lru_cache(maxsize=None)
def case(B, h, w, H, W, Cout):
    """Inputs and the pre-activation fp64 definition of one shape, computed once and shared (never modified)."""
    z = rnd("z", (B, 9 * Cout, h, w), 1)
    s, b = rnd("s", (B, Cout, H, W), 2), rnd("b", (Cout,), 3, 0.3)
    return z, s, b, definition(z, s, b, H, W, 0)


def check_all_outputs(ops, z, s, b, H, W, act, ref, border=None):
    """fp32 + bf16 pairs in one launch, fp16 pairs alone in another; returns the fp32 result."""
    y, ys = ops.tap_interp_combine(z, s, b, (H, W), act, out_fp32=True, out_split=True, border=border)
    assert y.is_contiguous(memory_format=CL) and rel_dev(y, ref) < TOL
    assert not ys.f16 and rel_dev(ys.float(), y) < 1e-5
    yh = ops.tap_interp_combine(z, s, b, (H, W), act, out_fp32=False, out_split=True, border=border, split_f16=True)
    assert yh.f16 and rel_dev(yh.float(), y) < 3e-7
    return y


SHAPES = [(2, 8, 9, 16, 19, 36),        # the row block meets the largest source-row count of a 2x up-sampling; W and Cout tails
          (1, 17, 22, 30, 40, 72),      # sh = 0.552: one source row more per block than at 2x
          (1, 13, 40, 22, 76, 64),      # sh = 0.571
          (1, 12, 12, 16, 16, 32),      # sh = 0.733, near the upper end of what is accepted
          (1, 1, 1, 8, 16, 32),         # a single source pixel: every y1 = y0 and x1 = x0 clamp
          (1, 2, 3, 9, 23, 40),         # > 3x
          (1, 5, 7, 11, 13, 8),         # H smaller than one tile
          (3, 5, 7, 17, 13, 32)]        # H one row more than a tile: a row block that is mostly outside the image


@pytest.mark.parametrize("B,h,w,H,W,Cout", SHAPES)
def test_rows_against_definition(ops, B, h, w, H, W, Cout):
    assert ops.tap_interp_supported(h, w, H, W, Cout)
    z, s, b, pre = case(B, h, w, H, W, Cout)
    check_all_outputs(ops, cl(z), cl(s), b.cuda(), H, W, 2, activate(pre, 2))


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_rows_every_activation(ops, act):
    B, h, w, H, W, Cout = SHAPES[0]
    z, s, b, pre = case(B, h, w, H, W, Cout)
    check_all_outputs(ops, cl(z), cl(s), b.cuda(), H, W, act, activate(pre, act))


def test_rows_without_skip_and_bias(ops):
    B, h, w, H, W, Cout = SHAPES[1]
    z = case(B, h, w, H, W, Cout)[0]
    check_all_outputs(ops, cl(z), None, None, H, W, 0, definition(z, None, None, H, W, 0))


def test_rows_bordered_grid(ops):
    """zpad = 1: z holds the interior of an (h+2) x (w+2) source whose border ring is one constant vector: the definition on
    the materialised grid, and bit for bit what the plain form gives on it."""
    B, h, w, H, W, Cout, act = 2, 6, 9, 17, 23, 96, 1
    z, border = rnd("z", (B, 9 * Cout, h, w), 1), rnd("c", (9 * Cout,), 2)
    s, b = rnd("s", (B, Cout, H, W), 3), rnd("b", (Cout,), 4, 0.3)
    full = border.view(1, -1, 1, 1).expand(B, 9 * Cout, h + 2, w + 2).clone()
    full[:, :, 1:-1, 1:-1] = z
    assert ops.tap_interp_supported(h + 2, w + 2, H, W, Cout)
    ref = definition(full, s, b, H, W, act)
    got = check_all_outputs(ops, cl(z), cl(s), b.cuda(), H, W, act, ref, border=border.cuda())
    want = ops.tap_interp_combine(cl(full), cl(s), b.cuda(), (H, W), act)
    assert torch.equal(got, want)


def test_rows_repeatable_and_batch_independent(ops):
    B, h, w, H, W, Cout = 4, 8, 9, 16, 19, 36
    z, s, b = cl(rnd("z", (B, 9 * Cout, h, w), 5)), cl(rnd("s", (B, Cout, H, W), 6)), rnd("b", (Cout,), 7, 0.3).cuda()
    run = lambda zz, ss: ops.tap_interp_combine(zz, ss, b, (H, W), 2, out_fp32=True, out_split=True)
    y, ys = run(z, s)
    y2, ys2 = run(z, s)
    assert torch.equal(y, y2) and torch.equal(ys.hl, ys2.hl)
    for half in (slice(0, 2), slice(2, 4)):
        yh, ysh = run(z[half].contiguous(memory_format=CL), s[half].contiguous(memory_format=CL))
        assert torch.equal(yh, y[half]) and torch.equal(ysh.hl, ys.hl[half])
