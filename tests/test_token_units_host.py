"""CPU: the references of tests/test_hip_token_units.py, and the rule its bars follow.

1. tests/token_ref.py restates the token path's units in plain torch.  Each restatement is anchored here against
   torch's own nn.TransformerEncoderLayer / nn.MultiheadAttention in float64, to 1e-12 of max |ref|: unmasked, a masked
   batch, and an image without a live key (NaN rows in the same places).
2. The GPU test allows a two-term fp16 kernel ``4 x max(d32, 2e-7)``, d32 = the deviation of the same formula in float32.  That
   margin assumes the operand rounding of the two-term form costs less than float32's own rounding.  Shown here on the inputs
   the GPU cases use: dh2 (the unit in float64 with every product through ``token_ref.h2_matmul``) < d32, for x2 and for
   qkv_next.  Measured over the cases below (FF = 1024 at M = 33 / 769 / 1793, layers 0 and 2; FF = 128 .. 768 at M = 33):
       x2        d32 2.0e-7 .. 3.7e-7    dh2 0.6e-7 .. 0.9e-7
       qkv_next  d32 3.7e-7 .. 7.9e-7    dh2 1.0e-7 .. 1.4e-7
   (qkv_next here = the tail and the projection chained, each form against the float64 chain.)
"""
import pytest
import torch
import torch.nn as nn

import token_cases as tc
import token_ref as tr
from util import rel_dev

ANCHOR = 1e-12


@pytest.fixture(scope="module")
def enc():
    return tc.encoder()


def _z(t, nan):
    return torch.where(nan, torch.zeros_like(t), t)


@pytest.mark.parametrize("B,S,counts", [(2, 37, None), (3, 40, [40, 7, 1])])
@pytest.mark.parametrize("l", [0, 2])
def test_layer_from_units_equals_torch_layer_in_float64(enc, B, S, counts, l):
    """qkv() -> attention() -> tail() chained = nn.TransformerEncoderLayer.double() (its op-by-op path: gradients enabled, so
    that torch does not take the fused inference path that rewrites padded rows), with and without a key-padding mask."""
    layer = enc.layers[l]
    x = tc.gen.randn("x", (B, S, 128), 5 + l).double()
    mask = None if counts is None else tc.key_mask(counts, S)
    ref_layer = nn.TransformerEncoderLayer(128, 4, 1024, batch_first=True).eval()
    ref_layer.load_state_dict(layer.state_dict())
    ref_layer = ref_layer.double()
    with torch.enable_grad():
        ref = ref_layer(x, src_key_padding_mask=mask).detach()
    got = tr.encoder_layer(x, tc.params(layer), mask)
    assert got.dtype == torch.float64 and not bool(torch.isnan(ref).any())
    assert rel_dev(got, ref) < ANCHOR


@pytest.mark.parametrize("Sq,Sk,counts", [(37, 37, None), (40, 33, [33, 7, 1]), (5, 12, [12, 0, 3])])
def test_mha_and_attention_equal_torch_multihead_attention_in_float64(enc, Sq, Sk, counts):
    """mha(), and attention() on qkv()'s packed projection (self-attention cases), = nn.MultiheadAttention.double(); an image
    without a live key gives NaN in exactly the rows torch gives it."""
    B = 3 if counts else 2
    sa = enc.layers[1].self_attn
    ref_m = nn.MultiheadAttention(128, 4, batch_first=True).eval()
    ref_m.load_state_dict(sa.state_dict())
    ref_m = ref_m.double()
    qs, ks, vs = (tc.gen.randn(n, (B, s, 128), 9).double() for n, s in (("qs", Sq), ("ks", Sk), ("vs", Sk)))
    if Sq == Sk:
        ks = vs = qs
    mask = None if counts is None else tc.key_mask(counts, Sk)
    with torch.enable_grad():                  # need_weights=True: torch's op-by-op softmax (NaN without a live key, what the kernels
        ref = ref_m(qs, ks, vs, key_padding_mask=mask, need_weights=True)[0].detach()    # restate; recent fused routes write 0 there)
    w =(sa.in_proj_weight.detach(), sa.in_proj_bias.detach(), sa.out_proj.weight.detach(), sa.out_proj.bias.detach())
    got = tr.mha(qs, ks, vs, *w, mask)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert bool(nan.any()) == bool(counts and 0 in counts)
    if counts and 0 in counts:
        assert bool(nan[counts.index(0)].all()) and not bool(nan[[i for i, c in enumerate(counts) if c]].any())
    assert rel_dev(_z(got, nan), _z(ref, nan)) < ANCHOR
    if Sq == Sk:
        ctx = tr.attention(tr.qkv(qs, w[0], w[1]), mask)
        via = ctx @ w[2].double().t() + w[3].double()
        assert rel_dev(via, ref) < ANCHOR


def test_attention_on_an_image_without_live_keys_is_nan_there_only():
    packed = tc.gen.randn("qkv", (3, 6, 384), 3).double()
    mask = tc.key_mask([6, 0, 2], 6)
    got = tr.attention(packed, mask)
    assert bool(torch.isnan(got[1]).all()) and not bool(torch.isnan(got[[0, 2]]).any())


def test_h2_matmul_carries_22_bits_and_float32_inputs_keep_their_dtype():
    a, w = tc.gen.randn("a", (33, 128), 1), tc.gen.randn("w", (64, 128), 2, 0.1)
    exact = a.double() @ w.double().t()
    scale = float((a.double().abs() @ w.double().abs().t()).max())
    assert float((tr.h2_matmul(a, w) - exact).abs().max()) < 3 * 2.0 ** -22 * scale      # two operands at 2^-22 each, + the dropped lo.lo
    hi, lo = tr.split_h2(a)
    assert float((hi + lo * 2.0 ** -11 - a.double()).abs().max()) <= 2.0 ** -22 * float(a.abs().max())
    p = tc.params(tc.encoder().layers[0])
    x1, x2 = tr.tail(a, a, p)
    assert x1.dtype == torch.float32 and x2.dtype == torch.float32 and tr.qkv(x2, w.repeat(6, 1), torch.zeros(384)).dtype == torch.float32


@pytest.mark.parametrize("M,FF,l", [(33, 1024, 0), (33, 1024, 2), (769, 1024, 0), (769, 1024, 2), (1793, 1024, 0), (1793, 1024, 2)] +
                         [(33, FF, 0) for FF in (128, 256, 384, 512, 640, 768)])
def test_two_term_operand_rounding_costs_less_than_float32_rounding(enc, M, FF, l):
    """dh2 < d32 for x2 and for qkv_next (module docstring, 2.) on the GPU cases' own inputs: the margin of 4 the GPU test
    gives the two-term fp16 kernels = operand rounding (<= d32, here) + float32 accumulation in another order (~ d32), times two."""
    p = tc.params(tc.layer_module(enc, l, FF))
    nxt = tc.params(enc.layers[l + 1])
    wq, bq = nxt["self_attn.in_proj_weight"], nxt["self_attn.in_proj_bias"]
    ctx, x = tc.tail_inputs(M, tc.tail_seed(M, FF, l))
    x2_64 = tr.tail(ctx.double(), x.double(), p)[1]
    x2_32 = tr.tail(ctx, x, p)[1]
    x2_h2 = tr.tail(ctx.double(), x.double(), p, matmul=tr.h2_matmul)[1]
    q_64, q_32, q_h2 = tr.qkv(x2_64, wq, bq), tr.qkv(x2_32, wq, bq), tr.qkv(x2_h2, wq, bq, matmul=tr.h2_matmul)
    assert x2_32.dtype == torch.float32 and q_32.dtype == torch.float32 and x2_h2.dtype == torch.float64
    d32_x, dh2_x = rel_dev(x2_32, x2_64), rel_dev(x2_h2, x2_64)
    d32_q, dh2_q = rel_dev(q_32, q_64), rel_dev(q_h2, q_64)
    print(f"M={M} FF={FF} l={l}: x2 d32 {d32_x:.2e} dh2 {dh2_x:.2e} | qkv_next d32 {d32_q:.2e} dh2 {dh2_q:.2e}")
    assert 0 < dh2_x < d32_x and 0 < dh2_q < d32_q
