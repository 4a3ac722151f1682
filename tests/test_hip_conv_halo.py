"""The halo-staged dense 3 x 3 kernel (conv_halo_dma_kernel, csrc/conv_dma.hip: one 8 x 32 pixel patch per workgroup, the
(8 + 2) x (32 + 2) halo patch of a 32-channel chunk staged once) against the tap ring it stands beside (conv_split_dma_kernel),
switched by ocv_conv3x3_set_dispatch in one process on the same operands: same products, same accumulation order, so the fp32
output and the hl32 split output are compared with torch.equal.  Shapes are the smallest at which the staging can go wrong:

    B 1,  8 x 32    every halo side outside the image (a single patch)
    B 1, 16 x 64    halos inside the image in both directions
    B 2,  8 x 32    the second image's top halo is zeros, not the first image's last row
    Cin 32 / 64 / 96    one A buffer / the double-buffer swap / the weights' ring wraps while A swaps
    Cin 40              Cp = 64 with zero pad channels
    Cout 8 / 128 / 136  the element-wise epilogue (Cout % 8 != 0 never takes it: 8 is a partial N tile; 12 does) / one full
                        N tile / a ragged second N tile

each with nothing but the fp32 output and with bias, oscale, LeakyReLU, residual and the split output together, as bf16 and as
fp16 pairs; one shape against the float64 definition with the bars tests/decoder_shadow.py applies to this kernel; the
forced-mode error, automatic dispatch on an unsupported shape and on the two layers it gives to the halo kernel, and a captured launch
replayed in a fresh child process.  ocv_conv3x3_last_kernel tells which kernel a run launched: every case asserts it."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import gen
from decoder_shadow import BF16_TOL, F16_TOL
from util import branch_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HERE = os.path.dirname(os.path.abspath(__file__))
AUTO, RING, HALO = 0, 1, 2
ACT_NONE, ACT_LEAKY_RELU = 0, 2

# (B, H, W, Cin, Cout)
SHAPES = [(1, 8, 32, 32, 128), (1, 16, 64, 64, 128), (2, 8, 32, 96, 128), (2, 8, 32, 40, 8), (1, 16, 64, 32, 12),
          (2, 16, 64, 64, 136)]


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    assert hip_ops.ACT_LEAKY_RELU == ACT_LEAKY_RELU
    return hip_ops


class Case:
    """Operands of one convolution on the device; ``run(mode)`` -> (y fp32 NHWC storage or None, split output bits or None)."""

    def __init__(self, ops, B, H, W, Cin, Cout, f16, full, seed=0):
        self.ops, self.lib = ops, ops._lib.load()
        self.dims, self.f16, self.full = (B, H, W, Cin, Cout), f16, full
        self.x32 = gen.randn("x", (B, Cin, H, W), 11 + seed).cuda().contiguous(memory_format=torch.channels_last)
        self.w32 = gen.randn("w", (Cout, Cin, 3, 3), 12 + seed, 1.0 / (3.0 * Cin ** 0.5))
        self.x = ops.split_act(self.x32, f16=f16)
        prep = ops.prep_conv_weight(self.w32.cuda(), f16=f16)
        self.w_hi, self.w_lo = prep[0], prep[1]
        self.oscale = prep[2] if f16 else (torch.exp2(torch.arange(Cout) % 3 - 1.0).float().cuda() if full else None)
        self.bias = gen.randn("b", (Cout,), 13 + seed, 0.3).cuda() if full else None
        self.res = gen.randn("r", (B, H, W, Cout), 14 + seed).cuda() if full else None
        self.act = ACT_LEAKY_RELU if full else ACT_NONE

    def run(self, mode, expect_rc=0):
        B, H, W, Cin, Cout = self.dims
        y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
        ys = self.ops.SplitAct.empty(B, Cout, H, W, "cuda", f16=self.f16) if self.full else None
        if ys is not None:
            ys.hl.view(torch.int16).fill_(0x7E7E)
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        assert self.lib.ocv_conv3x3_set_dispatch(mode) == 0
        try:
            rc = self.lib.ocv_conv_nhwc_split_x_fwd(self.x.hl.data_ptr(), Cin, self.w_hi.data_ptr(), self.w_lo.data_ptr(), p(self.oscale),
                                                    int(self.f16), p(self.bias), p(self.res), y.data_ptr(), None if ys is None else ys.hl.data_ptr(),
                                                    B, H, W, Cout, 3, self.act, None, 0, torch.cuda.current_stream().cuda_stream)
        finally:
            self.lib.ocv_conv3x3_set_dispatch(AUTO)
        assert rc == expect_rc, self.lib.ocv_last_error().decode(errors="replace")
        self.kernel = self.lib.ocv_conv3x3_last_kernel() if rc == 0 else None      # 1 = tap ring, 2 = halo-staged
        torch.cuda.synchronize()
        return y, None if ys is None else ys.hl.view(torch.int16).clone()

    def reference(self):
        """The float64 definition on the operands the kernel read: x = hi + lo of the split input, the fp32 weights."""
        hi, lo = self.x.parts()
        x = hi.double().cpu() + lo.double().cpu()
        y = F.conv2d(x, self.w32.double(), None if self.bias is None else self.bias.double().cpu(), padding=1)
        if self.act == ACT_LEAKY_RELU:
            y = F.leaky_relu(y, 0.01)
        if self.res is not None:
            y = y + self.res.double().cpu().permute(0, 3, 1, 2)
        return y


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_halo_equals_ring(ops, B, H, W, Cin, Cout, f16, full):
    assert ops._lib.load().ocv_conv3x3_halo_supported(B, H, W, Cin, Cout) == 1
    c = Case(ops, B, H, W, Cin, Cout, f16, full)
    y1, s1 = c.run(RING)
    assert c.kernel == RING
    y2, s2 = c.run(HALO)
    assert c.kernel == HALO                                      # mode 2 really launched conv_halo_dma_kernel
    y3, s3 = c.run(HALO)
    assert not torch.isnan(y1).any() and not torch.isnan(y2).any()
    assert torch.equal(y2, y1)
    assert torch.equal(y3, y2)                                   # two runs of the same case: bit-equal
    if full:
        assert torch.equal(s2, s1) and torch.equal(s3, s2)
        assert not (s2 == 0x7E7E).all()


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
def test_halo_against_float64(ops, f16):
    """Bars: tests/decoder_shadow.py (F16_TOL for fp16 pairs, BF16_TOL for bf16 pairs), per image as a share of max |ref|.  The
    oscale of the bf16 case is left out here: it is not part of the definition (the fp16 weights carry theirs)."""
    c = Case(ops, 2, 16, 64, 64, 128, f16, True, seed=5)
    if not f16:
        c.oscale = None
    y, _ = c.run(HALO)
    devs = branch_dev(y.permute(0, 3, 1, 2), c.reference())
    bar = F16_TOL if f16 else BF16_TOL
    print(f"halo vs float64 ({'fp16' if f16 else 'bf16'} pairs): {max(devs):.3g} (bar {bar:.1e})")
    assert max(devs) < bar


def test_forced_halo_fails_on_an_unsupported_shape(ops):
    lib = ops._lib.load()
    assert lib.ocv_conv3x3_halo_supported(1, 8, 40, 32, 128) == 0
    c = Case(ops, 1, 8, 40, 32, 128, True, True)
    y, _ = c.run(HALO, expect_rc=-1)
    assert b"halo" in lib.ocv_last_error() and torch.isnan(y).all()          # an error, nothing launched, no fall-back


def test_automatic_on_an_unsupported_shape_equals_ring(ops):
    c = Case(ops, 1, 8, 40, 32, 128, True, True)
    y1, s1 = c.run(RING)
    y0, s0 = c.run(AUTO)
    assert c.kernel == RING
    assert not torch.isnan(y0).any() and torch.equal(y0, y1) and torch.equal(s0, s1)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 240, 320, 128, 128), (2, 120, 160, 256, 256)])
def test_automatic_runs_the_halo_kernel_on_the_layers_it_won(ops, B, H, W, Cin, Cout):
    """The two layers automatic dispatch gives to the halo kernel (keyed on H, W, Cin, Cout; profiles/conv_halo.txt), at a small
    batch; every other shape of this file stays on the ring under automatic."""
    c = Case(ops, B, H, W, Cin, Cout, True, True)
    y1, s1 = c.run(RING)
    y0, s0 = c.run(AUTO)
    assert c.kernel == HALO
    assert not torch.isnan(y0).any() and torch.equal(y0, y1) and torch.equal(s0, s1)
    small = Case(ops, 1, 16, 64, 64, 128, True, False)
    small.run(AUTO)
    assert small.kernel == RING


def test_dispatch_setter_rejects_unknown_modes(ops):
    lib = ops._lib.load()
    try:
        assert lib.ocv_conv3x3_set_dispatch(3) == -1 and lib.ocv_conv3x3_set_dispatch(-1) == -1
        for mode in (RING, HALO, AUTO):
            assert lib.ocv_conv3x3_set_dispatch(mode) == 0
    finally:
        lib.ocv_conv3x3_set_dispatch(AUTO)


def test_captured_halo_launch_replays_on_new_inputs():
    """In a fresh child process (tests/conv_halo_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "conv_halo_graph_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
