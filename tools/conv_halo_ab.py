"""The five dense 3 x 3 launches of one bs-16 480 x 640 step (four 128 -> 128 at 240 x 320, one 256 -> 256 at 120 x 160; fp16 pairs,
bias + LeakyReLU, split output) under both kernels of csrc/conv_dma.hip, switched by ocv_conv3x3_set_dispatch in one process
(1 = tap ring, conv_split_dma_kernel; 2 = halo-staged, conv_halo_dma_kernel; 0 = automatic): time per launch (20 launches after
3), the sum over the five, and a SHA-1 of the output bytes, so that two library builds (OCV_LIB_PATH: a parent build exports the
setter as a no-op and runs the ring under every mode) can be compared bit for bit from their logs.

    python tools/conv_halo_ab.py [MODE ...]     # default: 1 2; under a profiler give ONE mode and read the launches off its output
    OCV_AB_BATCH=8 python tools/conv_halo_ab.py # the same layers at another batch size
"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from objcavit_amd import hip_ops
# (launches per step, B, H, W, Cin, Cout)
NB = int(os.environ.get("OCV_AB_BATCH", "16"))
SH = [(4, NB, 240, 320, 128, 128), (1, NB, 120, 160, 256, 256)]
modes = [int(a) for a in sys.argv[1:]] or [1, 2]
lib = hip_ops._lib.load()
g = torch.Generator(device="cuda").manual_seed(7)
tot = {m: 0.0 for m in modes}
for (n, B, H, W, Cin, Cout) in SH:
    x = hip_ops.split_act(torch.randn(B, Cin, H, W, device="cuda", generator=g).contiguous(memory_format=torch.channels_last), f16=True)
    w_hi, w_lo, osc = hip_ops.prep_conv_weight(torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / (3 * Cin ** 0.5), f16=True)
    bias = 0.2 * torch.randn(Cout, device="cuda", generator=g)
    y = torch.empty(B, H, W, Cout, device="cuda")
    ys = hip_ops.SplitAct.empty(B, Cout, H, W, "cuda", f16=True)
    st = torch.cuda.current_stream().cuda_stream
    fn = lambda: hip_ops._lib.check(lib.ocv_conv_nhwc_split_x_fwd(x.hl.data_ptr(), Cin, w_hi.data_ptr(), w_lo.data_ptr(), osc.data_ptr(), 1,
                                                                  bias.data_ptr(), None, y.data_ptr(), ys.hl.data_ptr(), B, H, W, Cout, 3,
                                                                  hip_ops.ACT_LEAKY_RELU, None, 0, st), "conv3x3")
    for m in modes:
        assert lib.ocv_conv3x3_set_dispatch(m) == 0
        y.zero_(); ys.hl.zero_()
        for _ in range(3): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20): fn()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        tot[m] += n * ms
        hsh = hashlib.sha1(y.cpu().numpy().tobytes()).hexdigest()[:12]
        ssh = hashlib.sha1(ys.hl.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:12]
        print(f"mode {m}  {n} x B{B} {H}x{W} {Cin}->{Cout}: {1e3 * ms:7.1f} us  sha1 y {hsh} split {ssh}  kernel {('-', 'ring', 'halo')[lib.ocv_conv3x3_last_kernel()]}")
lib.ocv_conv3x3_set_dispatch(0)
for m in modes:
    print(f"mode {m}  sum over the 5 launches {tot[m]:.3f} ms  [{os.environ.get('OCV_LIB_PATH', 'product build')}]")
