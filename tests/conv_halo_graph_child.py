"""Child process of tests/test_hip_conv_halo.py: a ``torch.cuda.graph`` that holds ONLY one halo-staged 3 x 3 convolution
(ocv_conv3x3_set_dispatch(2): the pad-channel clear of the split output and the convolution launch, one linear chain), replayed
after the input was overwritten in place, against the tap ring run eagerly on the same operands.  Started fresh so that the HIP
runtime reads GPU_MAX_HW_QUEUES=4 (what tests/conftest.py sets for the suite) at ITS start.  Prints OK when both replays are
bit-equal to the ring."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

from objcavit_amd import hip_ops, synth  # noqa: E402

B, H, W, CIN, COUT = 2, 16, 64, 64, 136
RING, HALO = 1, 2


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    lib = hip_ops._lib.load()
    x32 = synth.randn("x", (B, CIN, H, W), 21).cuda().contiguous(memory_format=torch.channels_last)
    x = hip_ops.split_act(x32, f16=True)
    w_hi, w_lo, oscale = hip_ops.prep_conv_weight(synth.randn("w", (COUT, CIN, 3, 3), 22, 0.05).cuda(), f16=True)
    bias = synth.randn("b", (COUT,), 23, 0.3).cuda()
    y = torch.empty(B, H, W, COUT, device="cuda")
    ys = hip_ops.SplitAct.empty(B, COUT, H, W, "cuda", f16=True)

    def call(mode, y_, ys_):
        assert lib.ocv_conv3x3_set_dispatch(mode) == 0
        try:
            rc = lib.ocv_conv_nhwc_split_x_fwd(x.hl.data_ptr(), CIN, w_hi.data_ptr(), w_lo.data_ptr(), oscale.data_ptr(), 1, bias.data_ptr(), None,
                                               y_.data_ptr(), ys_.hl.data_ptr(), B, H, W, COUT, 3, hip_ops.ACT_LEAKY_RELU, None, 0,
                                               torch.cuda.current_stream().cuda_stream)
        finally:
            lib.ocv_conv3x3_set_dispatch(0)
        assert rc == 0, lib.ocv_last_error().decode(errors="replace")

    def ring():
        y1, ys1 = torch.empty_like(y), hip_ops.SplitAct.empty(B, COUT, H, W, "cuda", f16=True)
        call(RING, y1, ys1)
        torch.cuda.synchronize()
        return y1, ys1.hl.view(torch.int16)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(HALO, y, ys)                                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(HALO, y, ys)
    y.fill_(float("nan"))
    ys.hl.view(torch.int16).fill_(0x7E7E)
    graph.replay()
    torch.cuda.synchronize()
    y1, s1 = ring()
    assert torch.equal(y, y1) and torch.equal(ys.hl.view(torch.int16), s1), "replay on the captured input"
    first = y.clone()
    x.hl.copy_(hip_ops.split_act(synth.randn("x", (B, CIN, H, W), 24).cuda().contiguous(memory_format=torch.channels_last), f16=True).hl)
    y.fill_(float("nan"))
    ys.hl.view(torch.int16).fill_(0x7E7E)
    graph.replay()
    torch.cuda.synchronize()
    y1, s1 = ring()
    assert not torch.isnan(y).any() and not torch.equal(y, first), "replay on the new input: every element written"
    assert torch.equal(y, y1) and torch.equal(ys.hl.view(torch.int16), s1), "replay on the new input"
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
