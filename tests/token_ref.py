"""Plain restatements of the token path's units (the four-layer stacks' layer tails, the packed projection, the attention
core, nn.MultiheadAttention), written against torch's documented formulas and nothing else in this repository
(independent of oracle/restate.py).  Every function computes in the dtype of its activation inputs -- float64 tensors give
the reference, float32 tensors the "same formula in float32" that the GPU tests take their bars from -- and casts the
parameters it is handed to that dtype.

A layer's parameters travel as the state_dict of an nn.TransformerEncoderLayer (keys ``self_attn.in_proj_weight`` ...
``norm2.bias``); ``matmul`` is the product used for every ``a @ w.T`` (default: torch's), so that ``h2_matmul`` can stand in
for it and isolate the operand rounding of the two-term fp16 kernels.
"""
import math

import torch


def plain_matmul(a, w):
    """a [.., K] @ w [N, K]^T in a's dtype."""
    return a @ w.to(a.dtype).t()


def split_h2(v):
    """The two-term fp16 split of csrc/token_tile.hpp (split_h2) as float64 tensors: hi = fp16(v), lo' = fp16((v - hi) 2^11), so that
    v ~ hi + 2^-11 lo' to 22 significant bits.  The kernels split fp32 values: v is rounded to float32 first."""
    v32 = v.to(torch.float32)
    hi = v32.to(torch.float16)
    lo = ((v32 - hi.to(torch.float32)) * 2048.0).to(torch.float16)       # (exact in float32, as on the device)
    return hi.to(torch.float64), lo.to(torch.float64)


def h2_matmul(a, w):
    """a @ w^T with both operands as two-term fp16 splits and the three products the kernels keep, summed in float64:
    hi.hi + 2^-11 (hi.lo' + lo'.hi).  Only the operands are rounded; returns float64."""
    ah, al = split_h2(a)
    wh, wl = split_h2(w)
    return ah @ wh.t() + (ah @ wl.t() + al @ wh.t()) * (2.0 ** -11)


def layernorm(x, gamma, beta, eps=1e-5):
    """nn.LayerNorm over the last dim: biased variance."""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + eps) * gamma.to(x.dtype) + beta.to(x.dtype)


def tail(ctx, x, p, eps=1e-5, matmul=plain_matmul):
    """Everything of a post-norm nn.TransformerEncoderLayer (eval, relu) behind the attention core, per token:
        x1 = LN1(x + ctx Wo^T + bo);  x2 = LN2(x1 + W2 relu(W1 x1 + b1) + b2)
    ctx / x [M, 128]; p: the layer's state_dict.  Returns (x1, x2) in the dtype of ``x``."""
    t = x.dtype
    ctx = ctx.to(t)
    a = matmul(ctx, p["self_attn.out_proj.weight"]).to(t) + p["self_attn.out_proj.bias"].to(t)
    x1 = layernorm(x + a, p["norm1.weight"], p["norm1.bias"], eps)
    h = torch.relu(matmul(x1, p["linear1.weight"]).to(t) + p["linear1.bias"].to(t))
    f = matmul(h, p["linear2.weight"]).to(t) + p["linear2.bias"].to(t)
    x2 = layernorm(x1 + f, p["norm2.weight"], p["norm2.bias"], eps)
    return x1, x2


def qkv(x2, w, b, matmul=plain_matmul):
    """The packed q | k | v projection: x2 [.., 128] -> [.., 384] with in_proj_weight [384, 128] / in_proj_bias."""
    return matmul(x2, w).to(x2.dtype) + b.to(x2.dtype)


def _heads(t, heads):
    B, S, E = t.shape
    return t.reshape(B, S, heads, E // heads).permute(0, 2, 1, 3)


def _core(q, k, v, mask, heads):
    """softmax(q k^T / sqrt(d) + mask) v per head; q [B, Sq, E], k / v [B, Sk, E]; mask bool [B, Sk], True = ignore the key.
    An image whose keys are all masked yields NaN rows (softmax over -inf only), as torch does."""
    B, Sq, E = q.shape
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(E // heads)
    if mask is not None:
        s = s.masked_fill(mask.to(torch.bool)[:, None, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)                                  # (-inf) - (-inf) = NaN for a row without a live key
    pr = e / e.sum(-1, keepdim=True)
    return (pr @ vh).permute(0, 2, 1, 3).reshape(B, Sq, E)


def attention(qkv_packed, mask, heads=4):
    """Self-attention core on the packed [B, S, 3E] projection a tail (or layer 0's linear) wrote -> ctx [B, S, E]."""
    E = qkv_packed.shape[-1] // 3
    return _core(qkv_packed[..., :E], qkv_packed[..., E:2 * E], qkv_packed[..., 2 * E:], mask, heads)


def mha(q_src, k_src, v_src, in_w, in_b, out_w, out_b, mask=None, heads=4):
    """nn.MultiheadAttention(E, heads, batch_first=True)(q_src, k_src, v_src, key_padding_mask=mask, need_weights=False)[0]."""
    t = q_src.dtype
    E = q_src.shape[-1]
    in_w, in_b = in_w.to(t), in_b.to(t)
    q = q_src @ in_w[:E].t() + in_b[:E]
    k = k_src.to(t) @ in_w[E:2 * E].t() + in_b[E:2 * E]
    v = v_src.to(t) @ in_w[2 * E:].t() + in_b[2 * E:]
    return _core(q, k, v, mask, heads) @ out_w.to(t).t() + out_b.to(t)


def encoder_layer(x, p, mask=None, heads=4, eps=1e-5):
    """One whole layer on x [B, S, E] from the units above (what the host test anchors against torch's layer)."""
    B, S, E = x.shape
    ctx = attention(qkv(x, p["self_attn.in_proj_weight"], p["self_attn.in_proj_bias"]), mask, heads)
    return tail(ctx.reshape(B * S, E), x.reshape(B * S, E), p, eps)[1].reshape(B, S, E)
