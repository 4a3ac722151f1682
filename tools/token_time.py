"""Time of the token-path kernels a refactor changed, one process per library build (OCV_LIB_PATH): the encoder stack under
OCV_TOKENS=split3 (layer_tail3_kernel) at bs 16 x 300 image tokens and bs 16 x 32 object tokens, and the split3 few-key
cross-attention (xattn_kv3_kernel + xattn_main3_kernel) at bs 16 and bs 512 x 300 queries; microseconds per call, 20 calls after 3 warm-ups.

    python tools/token_time.py;  OCV_LIB_PATH=objcavit_amd/lib/variants/parent.so python tools/token_time.py
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["OCV_TOKENS"] = "split3"
import torch
from objcavit_amd import hip_ops as ops


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


torch.manual_seed(0)
layers = [torch.nn.TransformerEncoderLayer(128, 4, 1024, dropout=0.0, batch_first=True).cuda().eval() for _ in range(4)]
caches = [{} for _ in layers]
params = [ops.layer_params(m, c) for m, c in zip(layers, caches)]
mh = torch.nn.MultiheadAttention(128, 4, batch_first=True).cuda().eval()
w = [t.detach() for t in (mh.in_proj_weight, mh.in_proj_bias, mh.out_proj.weight, mh.out_proj.bias)]
res = []
for S in (300, 32):
    x = torch.randn(16, S, 128, device="cuda")
    res.append(f"stack_split3_16x{S} {timed(lambda: ops.encoder_stack(x, [p[0] for p in params])):.2f}")
q, k = torch.randn(16, 300, 128, device="cuda"), torch.randn(16, 32, 128, device="cuda")
mask = (torch.arange(32, device="cuda")[None, :] >= 20).expand(16, 32).contiguous()
cache = {}
res.append(f"mha_few_split3_16x300 {timed(lambda: ops.mha(q, k, k, *w, mask, 4, 20, packed=cache)):.2f}")
q, k = torch.randn(512, 300, 128, device="cuda"), torch.randn(512, 32, 128, device="cuda")          # (the GPU, not the host, sets this one's time)
mask = (torch.arange(32, device="cuda")[None, :] >= 20).expand(512, 32).contiguous()
res.append(f"mha_few_split3_512x300 {timed(lambda: ops.mha(q, k, k, *w, mask, 4, 20, packed=cache)):.2f}")
print("us/call  " + "  ".join(res) + f"  [{os.environ.get('OCV_LIB_PATH', 'product build')}]")
