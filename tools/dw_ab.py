"""The k = 5 depthwise launches of one bs-16 EfficientNet-B5 step under both kernels of csrc/depthwise_se.hip, switched by
ocv_depthwise_set_dispatch in one process (1 = register window, dw_slide_kernel; 2 = input rows staged through LDS,
dw_rows_kernel): time per launch (20 launches after 3, the depthwise launch alone), the sum over the 21 launches of a
step, and a SHA-1 of the output bytes, so that two library builds (OCV_LIB_PATH) can be compared bit for bit from their logs.

    python tools/dw_ab.py [MODE ...]        # default: 1 2; under a profiler give ONE mode and read the launches off its trace
"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from objcavit_amd import hip_ops
# (launches per step, B, C, H, W, stride)
SH = [(4, 16, 384, 60, 80, 1), (6, 16, 1056, 30, 40, 1), (1, 16, 768, 30, 40, 1), (8, 16, 1824, 15, 20, 1),
      (1, 16, 240, 120, 160, 2), (1, 16, 1056, 30, 40, 2)]
K = 5
modes = [int(a) for a in sys.argv[1:]] or [1, 2]
lib = hip_ops._lib.load()
cl = torch.channels_last
g = torch.Generator(device="cuda").manual_seed(5)
tot = {m: 0.0 for m in modes}
for (n, B, C, H, W, s) in SH:
    R = C // 24
    x = torch.randn(B, C, H, W, device="cuda", generator=g).contiguous(memory_format=cl)
    w = (0.3 * torch.randn(K * K, C, device="cuda", generator=g)).contiguous()
    b = 0.2 * torch.randn(C, device="cuda", generator=g)
    se = (torch.randn(R, C, device="cuda", generator=g) / C ** 0.5, torch.randn(R, device="cuda", generator=g),
          torch.randn(R, C, device="cuda", generator=g) / R ** 0.5, torch.randn(C, device="cuda", generator=g))
    Ho, Wo = -(-H // s), -(-W // s)
    pt, pl = max((Ho - 1) * s + K - H, 0) // 2, max((Wo - 1) * s + K - W, 0) // 2
    out = torch.empty(B, C, Ho, Wo, device="cuda").contiguous(memory_format=cl)
    st = torch.cuda.current_stream().cuda_stream
    for m in modes:
        assert lib.ocv_depthwise_set_dispatch(m) == 0
        y, gate = hip_ops.depthwise_se_gate(x, w, b, K, s, *se)
        hsh = hashlib.sha1(y.cpu().numpy().tobytes()).hexdigest()[:12]
        gsh = hashlib.sha1(gate.cpu().numpy().tobytes()).hexdigest()[:12]
        part = torch.empty(B * lib.ocv_depthwise_sum_tiles(B, C, Ho, Wo, K, s) * C, device="cuda")
        fn = lambda: hip_ops._lib.check(lib.ocv_depthwise_conv_nhwc_sum_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(),
                                                                            part.data_ptr(), B, C, H, W, K, s, pt, pl, Ho, Wo, st), "depthwise")
        for _ in range(3): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20): fn()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        tot[m] += n * ms
        print(f"mode {m}  {n} x B{B} C{C} {H}x{W} s{s}: {1e3 * ms:7.1f} us  sha1 y {hsh} gate {gsh}  equal-to-launch {torch.equal(out, y)}")
lib.ocv_depthwise_set_dispatch(0)
for m in modes:
    print(f"mode {m}  sum over the 21 launches {tot[m]:.3f} ms  [{os.environ.get('OCV_LIB_PATH', 'product build')}]")
