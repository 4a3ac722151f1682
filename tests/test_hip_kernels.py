"""-m gpu: every HIP kernel, called through the C ABI (objcavit_amd.hip_ops ->
ctypes -> libobjcavit_hip.so), against the CPU oracle on the same seeded
inputs.  All arithmetic is fp32; tolerances are stated per test (relative to
the largest reference magnitude unless noted)."""
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen
from oracle import restate
from util import rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 2e-5          # fp32 kernels vs fp32 CPU: accumulation-order noise only


def dev(t):
    return t.cuda()


def rnd(key, shape, seed=0, scale=1.0):
    return gen.randn(key, shape, seed, scale)


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------ linear
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (5, 32, 2), (37, 64, 4), (300, 128, 128), (4800, 384, 128),
                                   (77, 1024, 128), (130, 128, 1024), (33, 256, 513), (16, 130, 66)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear(ops, M, N, K, act):
    x, w, b = rnd("x", (M, K), 1), rnd("w", (N, K), 2, 1 / math.sqrt(K)), rnd("b", (N,), 3)
    ref = x @ w.T + b
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01)][act]
    got = ops.linear(dev(x), dev(w), dev(b), act)
    assert rel_dev(got, ref) < TOL


def test_linear_no_bias_and_batched_leading_dims(ops):
    x, w = rnd("x", (3, 7, 64), 4), rnd("w", (48, 64), 5)
    assert rel_dev(ops.linear(dev(x), dev(w)), x @ w.T) < TOL


@pytest.mark.parametrize("M,K", [(1, 128), (45, 128), (300, 1024), (4800, 128)])
def test_linear_residual_layernorm(ops, M, K):
    a, w, b = rnd("a", (M, K), 1), rnd("w", (128, K), 2, 1 / math.sqrt(K)), rnd("b", (128,), 3)
    res, g, be = rnd("r", (M, 128), 4), 1 + 0.1 * rnd("g", (128,), 5), rnd("be", (128,), 6)
    ref = restate.layer_norm(res + a @ w.T + b, g, be)
    got = ops.linear_residual_layernorm(dev(a), dev(w), dev(b), dev(res), dev(g), dev(be))
    assert rel_dev(got, ref) < TOL
    mask = (torch.arange(M) % 3 == 1)
    got = ops.linear_residual_layernorm(dev(a), dev(w), dev(b), dev(res), dev(g), dev(be),
                                        zero_row_mask=dev(mask.to(torch.uint8)))
    assert rel_dev(got, ref.masked_fill(mask[:, None], 0.0)) < TOL
    assert float(got[dev(mask)].abs().max()) == 0.0 if mask.any() else True


@pytest.mark.parametrize("M,FF", [(1, 128), (45, 1024), (300, 1024), (4800, 1024), (33, 256)])
def test_ffn_residual_layernorm_fused(ops, M, FF):
    x = rnd("x", (M, 128), 1)
    w1, b1 = rnd("w1", (FF, 128), 2, 1 / math.sqrt(128)), rnd("b1", (FF,), 3, 0.1)
    w2, b2 = rnd("w2", (128, FF), 4, 1 / math.sqrt(FF)), rnd("b2", (128,), 5, 0.1)
    g, be = 1 + 0.1 * rnd("g", (128,), 6), rnd("be", (128,), 7)
    ref = restate.layer_norm(x + torch.relu(x @ w1.T + b1) @ w2.T + b2, g, be)
    got = ops.ffn_residual_layernorm(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(g), dev(be))
    assert rel_dev(got, ref) < TOL
    mask = (torch.arange(M) % 4 == 2)
    got = ops.ffn_residual_layernorm(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(g), dev(be),
                                     zero_row_mask=dev(mask.to(torch.uint8)))
    assert rel_dev(got, ref.masked_fill(mask[:, None], 0.0)) < TOL


# ------------------------------------------------------------------ three-term bf16 split ("split3") token kernels
@pytest.mark.parametrize("M,N,K", [(1, 32, 8), (37, 64, 24), (300, 128, 128), (4800, 384, 128), (77, 1024, 128),
                                   (130, 128, 1024), (33, 256, 520), (16, 130, 72), (512, 200, 512)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_split3(ops, M, N, K, act):
    """ocv_linear_split3_fwd against an fp64 reference AT THE EXACT KERNEL'S TOLERANCE (fp32 accumulation noise): the
    three-term split is fp32-faithful, unlike the two-term split of the convolutions."""
    x, w, b = rnd("x", (M, K), 1), rnd("w", (N, K), 2, 1 / math.sqrt(K)), rnd("b", (N,), 3, 0.1)
    ref = x.double() @ w.double().T + b.double()
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01)][act]
    sw = ops.SplitWeight3(dev(w))
    assert sw.packed.numel() == ops._lib.load().ocv_split3_packed_elems(N, K)
    got = ops.linear_split3(dev(x), sw, dev(b), act)
    assert rel_dev(got, ref) < TOL
    exact = ops.linear(dev(x), dev(w), dev(b), act)
    e3, ex = rel_dev(got, ref), rel_dev(exact, ref)
    assert e3 <= 3.0 * ex + 1e-7, (e3, ex)                  # as good as the exact-fp32 MFMA kernel


def test_split3_keeps_fp32_range_and_24_bits(ops):
    """Operands spanning 12 decades and values that differ in their last mantissa bits only."""
    x = rnd("x", (64, 128), 1) * torch.logspace(-6, 6, 128).view(1, 128)
    w = rnd("w", (96, 128), 2, 0.05) / torch.logspace(-6, 6, 128).view(1, 128)
    got = ops.linear_split3(dev(x), ops.SplitWeight3(dev(w)))
    assert rel_dev(got, x.double() @ w.double().T) < TOL
    a = torch.full((32, 16), 1.0) + torch.arange(16).float() * 2.0 ** -23          # 1 + j ulp
    eye = torch.eye(16)
    got = ops.linear_split3(dev(a), ops.SplitWeight3(dev(eye)))
    assert torch.equal(got.cpu(), a)                                              # every mantissa bit survives


@pytest.mark.parametrize("M,FF", [(1, 128), (37, 1024), (512, 1024), (4800, 1024), (300, 256)])
def test_ffn_residual_layernorm_split3(ops, M, FF):
    x = rnd("x", (M, 128), 1)
    w1, b1 = rnd("w1", (FF, 128), 2, 1 / math.sqrt(128)), rnd("b1", (FF,), 3, 0.1)
    w2, b2 = rnd("w2", (128, FF), 4, 1 / math.sqrt(FF)), rnd("b2", (128,), 5, 0.1)
    g, be = 1 + 0.1 * rnd("g", (128,), 6), rnd("be", (128,), 7)
    ref = restate.layer_norm((x.double() + torch.relu(x.double() @ w1.double().T + b1.double()) @ w2.double().T + b2.double()).float(),
                             g, be)
    p1, p2 = ops.SplitWeight3(dev(w1)), ops.SplitWeight3(dev(w2))
    got = ops.ffn_residual_layernorm_split3(dev(x), p1, dev(b1), p2, dev(b2), dev(g), dev(be))
    assert rel_dev(got, ref) < TOL
    assert torch.equal(got, ops.ffn_residual_layernorm_split3(dev(x), p1, dev(b1), p2, dev(b2), dev(g), dev(be)))
    mask = (torch.arange(M) % 4 == 2)
    got = ops.ffn_residual_layernorm_split3(dev(x), p1, dev(b1), p2, dev(b2), dev(g), dev(be),
                                            zero_row_mask=dev(mask.to(torch.uint8)))
    assert rel_dev(got, ref.masked_fill(mask[:, None], 0.0)) < TOL


@pytest.mark.parametrize("rows,E", [(1, 128), (301, 128), (17, 96), (9, 300)])
def test_layernorm(ops, rows, E):
    x, r = rnd("x", (rows, E), 1, 3.0), rnd("r", (rows, E), 2)
    g, b = 1 + 0.1 * rnd("g", (E,), 3), rnd("b", (E,), 4)
    assert rel_dev(ops.layernorm(dev(x), dev(g), dev(b), 1e-5, dev(r)), restate.layer_norm(x + r, g, b)) < TOL
    assert rel_dev(ops.layernorm(dev(x), dev(g), dev(b)), restate.layer_norm(x, g, b)) < TOL


# ------------------------------------------------------------------ attention
def _attn_ref(q, k, v, mask, H):
    B, Sq, E = q.shape
    d = E // H
    qh = q.view(B, Sq, H, d).permute(0, 2, 1, 3)
    kh = k.view(B, -1, H, d).permute(0, 2, 1, 3)
    vh = v.view(B, -1, H, d).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(d)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ vh).permute(0, 2, 1, 3).reshape(B, Sq, E)


@pytest.mark.parametrize("B,Sq,Sk", [(1, 1, 1), (2, 132, 132), (2, 300, 300), (1, 418, 418), (3, 129, 77),
                                     (1, 40, 1200), (2, 300, 513)])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", ["h2", "fp32"])
def test_attention_core(ops, monkeypatch, B, Sq, Sk, masked, form):
    """softmax(q k^T / sqrt(d) + mask) v per head: both contractions as two-term fp16 splits (form h2, the default:
    attention_h2_kernel) or on exact fp32 MFMA (OCV_ATTN_FORM=fp32) -- one and several LDS chunks of keys, ragged tiles."""
    monkeypatch.setenv("OCV_ATTN_FORM", form)
    q, k, v = rnd("q", (B, Sq, 128), 1, 1.5), rnd("k", (B, Sk, 128), 2, 1.5), rnd("v", (B, Sk, 128), 3)
    mask = None
    if masked:
        n_valid = torch.tensor([max(1, (Sk * (b + 1)) // (B + 1)) for b in range(B)])
        mask = torch.arange(Sk)[None, :] >= n_valid[:, None]
    got = ops.attention_core(dev(q), dev(k), dev(v), None if mask is None else dev(mask), 4)
    assert rel_dev(got, _attn_ref(q, k, v, mask, 4)) < TOL


def test_attention_core_strided_packed_qkv(ops):
    """q/k/v as views of one packed [B, S, 3E] projection (what the encoder layer passes)."""
    B, S = 2, 150
    qkv = rnd("qkv", (B, S, 384), 7)
    g = dev(qkv)
    got = ops.attention_core(g[..., 0:128], g[..., 128:256], g[..., 256:384], None, 4)
    assert rel_dev(got, _attn_ref(qkv[..., :128].contiguous(), qkv[..., 128:256].contiguous(),
                                  qkv[..., 256:].contiguous(), None, 4)) < TOL


@pytest.mark.parametrize("form", ["h2", "fp32"])
def test_attention_online_softmax_rescale_is_exercised(ops, monkeypatch, form):
    monkeypatch.setenv("OCV_ATTN_FORM", form)
    """A spike in a late key tile forces the running max to jump after earlier tiles were accumulated."""
    B, S = 1, 320
    q, k, v = rnd("q", (B, S, 128), 1), rnd("k", (B, S, 128), 2), rnd("v", (B, S, 128), 3)
    k[0, 300] = q[0, 5] * 8.0
    k[0, 10] = q[0, 200] * 6.0
    got = ops.attention_core(dev(q), dev(k), dev(v), None, 4)
    assert rel_dev(got, _attn_ref(q, k, v, None, 4)) < TOL


@pytest.mark.parametrize("form", ["h2", "fp32"])
def test_attention_fully_masked_row_is_nan_like_torch(ops, monkeypatch, form):
    monkeypatch.setenv("OCV_ATTN_FORM", form)
    q, k, v = rnd("q", (1, 4, 128), 1), rnd("k", (1, 40, 128), 2), rnd("v", (1, 40, 128), 3)
    mask = torch.ones(1, 40, dtype=torch.bool)
    got = ops.attention_core(dev(q), dev(k), dev(v), dev(mask), 4)
    assert bool(torch.isnan(got).all())


@pytest.mark.parametrize("Sq,Sk,masked", [(132, 132, True), (300, 300, True), (64, 300, False)])
def test_mha_module(ops, Sq, Sk, masked):
    B, E = 2, 128
    qs, ks, vs = rnd("qs", (B, Sq, E), 1), rnd("ks", (B, Sk, E), 2), rnd("vs", (B, Sk, E), 3)
    iw, ib = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    mask = (torch.arange(Sk)[None, :] >= torch.tensor([[Sk // 3], [Sk]])) if masked else None
    ref = restate.multi_head_attention(qs, ks, vs, iw, ib, ow, ob, mask)
    got = ops.mha(dev(qs), dev(ks), dev(vs), dev(iw), dev(ib), dev(ow), dev(ob), None if mask is None else dev(mask))
    assert rel_dev(got, ref) < TOL


@pytest.mark.parametrize("counts", [[16, 5], [1, 1], [100, 3], [32] * 4])
def test_mha_kv_limit_skips_only_masked_keys(ops, counts):
    """Cross-attention #1 layout: keys >= Nmax are all masked; kv_limit = Nmax must not change the result."""
    B, S, E = len(counts), 132, 128
    qs, ks = rnd("qs", (B, S, E), 1), rnd("ks", (B, S, E), 2)
    iw, ib = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    mask = torch.arange(S)[None, :] >= torch.tensor(counts)[:, None]
    ref = restate.multi_head_attention(qs, ks, qs, iw, ib, ow, ob, mask)
    args = (dev(qs), dev(ks), dev(qs), dev(iw), dev(ib), dev(ow), dev(ob), dev(mask))
    full = ops.mha(*args)
    lim = ops.mha(*args, kv_limit=max(counts))
    assert rel_dev(full, ref) < TOL and rel_dev(lim, ref) < TOL


@pytest.mark.parametrize("Sq,counts", [(300, [32, 7, 1]), (45, [5, 0]), (32, [32]), (1, [3, 3])])
def test_mha_fused_few_keys(ops, Sq, counts):
    """kv_limit <= 32 takes the single-launch kernel (projections + attention + output projection): ragged query
    tiles, a batch row without any live key (NaN rows, as torch), V taken from a different tensor than K."""
    B, Sk, E = len(counts), 300, 128
    qs, ks, vs = rnd("qs", (B, Sq, E), 1), rnd("ks", (B, Sk, E), 2), rnd("vs", (B, Sk, E), 3)
    iw, ib = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    mask = torch.arange(Sk)[None, :] >= torch.tensor(counts)[:, None]
    ref = restate.multi_head_attention(qs, ks, vs, iw, ib, ow, ob, mask)
    got = ops.mha(dev(qs), dev(ks), dev(vs), dev(iw), dev(ib), dev(ow), dev(ob), dev(mask), kv_limit=max(max(counts), 1)).cpu()
    nan_ref = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan_ref)
    assert nan_ref.any() == (0 in counts)
    assert rel_dev(torch.where(nan_ref, torch.zeros_like(got), got), torch.where(nan_ref, torch.zeros_like(ref), ref)) < TOL
    full = ops.mha(dev(qs), dev(ks), dev(vs), dev(iw), dev(ib), dev(ow), dev(ob), dev(mask)).cpu()      # five-launch path
    assert rel_dev(torch.where(nan_ref, torch.zeros_like(got), got), torch.where(nan_ref, torch.zeros_like(full), full)) < TOL


@pytest.mark.parametrize("form", ["h2", "split3"])
@pytest.mark.parametrize("Sq,Sk,counts,kv", [(300, 300, [32, 7, 1], 32), (45, 300, [5, 0], 5), (32, 40, [32], 32), (1, 132, [3, 3], 3),
                                            (418, 418, [24] * 8, 24), (132, 132, [100, 3], 100), (77, 50, None, 0), (300, 1200, [1200, 640], 0),
                                            (300, 300, [(7 * i) % 33 for i in range(40)], 32), (64, 20, None, 0), (70, 32, [32, 31], 0)])
def test_mha_split3(ops, monkeypatch, Sq, Sk, counts, kv, form):
    """hip_ops.mha on packed split weights.  <= 32 live keys: K / V projected once per image + the fused per-tile launch, as
    two-term fp16 splits throughout (form h2, ocv_mha_few_keys_h2_fwd) or three-term bf16 projections + exact-fp32 scores (form
    split3, ocv_mha_split3_fwd): ragged tiles, an image without a live key -> NaN rows as torch, V from another tensor than K,
    KITTI's S = 418, 40 images with 0..32 objects, Sk <= 32 without a mask or a kv_limit; more keys / no mask: split3 linears
    around the attention kernel (multi-chunk Sk) under either form.  Against the oracle at the kernels' tolerance and against
    the exact-fp32 route."""
    B, E = (len(counts) if counts else 2), 128
    qs, ks, vs = rnd("qs", (B, Sq, E), 1), rnd("ks", (B, Sk, E), 2), rnd("vs", (B, Sk, E), 3)
    iw, ib = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    mask = None if counts is None else torch.arange(Sk)[None, :] >= torch.tensor(counts)[:, None]
    ref = restate.multi_head_attention(qs, ks, vs, iw, ib, ow, ob, mask)
    args = (dev(qs), dev(ks), dev(vs), dev(iw), dev(ib), dev(ow), dev(ob), None if mask is None else dev(mask))
    cache = {}
    monkeypatch.setenv("OCV_TOKENS", form)                      # (the few-key cross-attention follows the token mode)
    got = ops.mha(*args, kv_limit=kv, packed=cache).cpu()
    few = (kv if 0 < kv < Sk else Sk) <= 32
    assert set(cache) == ({"in_proj_h2", "out_proj_h2"} if few and form == "h2" else {"in_proj_p3", "out_proj_p3"})
    again = ops.mha(*args, kv_limit=kv, packed=cache).cpu()
    exact = ops.mha(*args, kv_limit=kv).cpu()
    nan_ref = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan_ref) and bool(nan_ref.any()) == bool(counts and 0 in counts)
    z = lambda t: torch.where(nan_ref, torch.zeros_like(t), t)          # noqa: E731
    assert rel_dev(z(got), z(ref)) < TOL and rel_dev(z(got), z(exact)) < TOL
    assert torch.equal(z(got), z(again))
    # (sub-tile count of the fused kernels: automatic here = one; two from 2048 64-query workgroups on: test_mha_few_keys_large_launch)


@pytest.mark.parametrize("form", ["h2", "split3"])
def test_mha_few_keys_large_launch(ops, monkeypatch, form):
    """Enough 64-query workgroups (>= 2048) for the two-sub-tile form of the fused few-key kernels: 420 images x 300 queries
    (a ragged last sub-tile: 300 = 4 x 64 + 44), 0..32 objects per image, every image checked against the exact-fp32 route and
    a sample of them against the oracle."""
    B, Sq, Sk, E = 420, 300, 40, 128
    counts = [(11 * i) % 33 for i in range(B)]
    qs, ks, vs = rnd("qs", (B, Sq, E), 21), rnd("ks", (B, Sk, E), 22), rnd("vs", (B, Sk, E), 23)
    iw, ib = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    mask = torch.arange(Sk)[None, :] >= torch.tensor(counts)[:, None]
    args = (dev(qs), dev(ks), dev(vs), dev(iw), dev(ib), dev(ow), dev(ob), dev(mask))
    monkeypatch.setenv("OCV_TOKENS", form)                      # (the few-key cross-attention follows the token mode)
    got = ops.mha(*args, kv_limit=32, packed={}).cpu()
    exact = ops.mha(*args, kv_limit=32).cpu()
    nan = torch.isnan(exact)
    assert torch.equal(torch.isnan(got), nan) and bool(nan[0].all()) and not bool(nan[1].any())
    z = lambda t: torch.where(nan, torch.zeros_like(t), t)              # noqa: E731
    assert rel_dev(z(got), z(exact)) < TOL
    pick = [1, 2, 4, 32, 34, 419]                                       # images with at least one live key (11 i mod 33 != 0)
    ref = restate.multi_head_attention(qs[pick], ks[pick], vs[pick], iw, ib, ow, ob, mask[pick])
    assert rel_dev(got[pick], ref) < TOL


def test_mha_few_keys_h2_random_shapes(ops):
    """Seeded sweep of the fused few-key form over ragged shapes: 1..9 images, 1..200 queries, 1..32 live keys of 1..90 key rows
    (kv_limit given or not, mask given or not when every key row is live), V from K's tensor or another -- against the exact-fp32
    route at the kernels' tolerance, NaN rows (an image without a live key) in the same places."""
    import random
    rng = random.Random(1234)
    E = 128
    iw, ib = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    par = (dev(iw), dev(ib), dev(ow), dev(ob))
    for case in range(40):
        B, Sq = rng.randint(1, 9), rng.choice([1, 2, 31, 32, 33, 63, 64, 65, 100, 200])
        live_max = rng.randint(1, 32)
        Sk = rng.choice([live_max, live_max, rng.randint(live_max, 90)])
        counts = [rng.randint(0 if B > 1 else 1, live_max) for _ in range(B)]
        counts[rng.randrange(B)] = live_max
        dense = Sk == live_max and all(c == live_max for c in counts) and rng.random() < 0.5
        qs, ks = rnd("q", (B, Sq, E), 100 + case), rnd("k", (B, Sk, E), 200 + case)
        vs = ks if rng.random() < 0.5 else rnd("v", (B, Sk, E), 300 + case)
        mask = None if dense else torch.arange(Sk)[None, :] >= torch.tensor(counts)[:, None]
        kv = 0 if (dense or (Sk <= 32 and rng.random() < 0.5)) else live_max
        args = (dev(qs), dev(ks), dev(vs)) + par + (None if mask is None else dev(mask),)
        cache = {}
        got = ops.mha(*args, kv_limit=kv, packed=cache).cpu()
        assert set(cache) == {"in_proj_h2", "out_proj_h2"}, (case, B, Sq, Sk, counts, kv)
        exact = ops.mha(*args, kv_limit=kv).cpu()
        nan = torch.isnan(exact)
        assert torch.equal(torch.isnan(got), nan), (case, B, Sq, Sk, counts, kv)
        assert bool(nan.any()) == (mask is not None and 0 in counts)
        z = lambda t: torch.where(nan, torch.zeros_like(t), t)          # noqa: E731
        assert rel_dev(z(got), z(exact)) < TOL, (case, B, Sq, Sk, counts, kv)


def test_mha_few_keys_h2_one_launch_equals_two_launches(ops):
    """Small calls (every query tile's workgroup resident at once) run as ONE launch whose tiles project K / V themselves; larger
    ones as the K / V launch + the tiles.  Same MFMAs on the same operands in the same order: the two forms agree BIT FOR BIT,
    ragged object counts, an image without a live key (NaN rows) and a separate value tensor included."""
    from objcavit_amd import _lib
    lib = _lib.load()
    E = 128
    iw, ib = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    par = (dev(iw), dev(ib), dev(ow), dev(ob))
    try:
        for case, (B, Sq, Sk, live) in enumerate([(16, 300, 16, 16), (2, 300, 16, 16), (5, 77, 40, 32), (1, 1, 1, 1), (32, 300, 24, 20)]):
            counts = [(live - (7 * i) % (live + 1)) for i in range(B)]
            counts[0] = live
            qs, ks, vs = rnd("q", (B, Sq, E), 10 + case), rnd("k", (B, Sk, E), 20 + case), rnd("v", (B, Sk, E), 30 + case)
            mask = torch.arange(Sk)[None, :] >= torch.tensor(counts)[:, None]
            args = (dev(qs), dev(ks), dev(vs if case % 2 else ks)) + par + (dev(mask),)
            outs = []
            for limit in (1 << 30, 0):                                  # one launch whatever the size / always two launches
                assert lib.ocv_mha_few_keys_h2_set_dispatch(limit) == 0
                outs.append(ops.mha(*args, kv_limit=live if live < Sk else 0, packed={}).cpu())
            nan = torch.isnan(outs[0])
            assert torch.equal(nan, torch.isnan(outs[1])) and bool(nan.any()) == (0 in counts), (case, counts)
            assert torch.equal(torch.nan_to_num(outs[0]), torch.nan_to_num(outs[1])), (case, B, Sq, Sk)
    finally:
        lib.ocv_mha_few_keys_h2_set_dispatch(-1)


@pytest.mark.parametrize("scale", [1e-4, 1e-2, 1.0, 300.0])
def test_two_term_fp16_kernels_hold_their_relative_error_at_any_magnitude(ops, scale):
    """The scaled low term keeps the two-term fp16 split out of fp16's subnormals and v_mfma_f32_32x32x16_f16 honours the
    subnormal HIGH terms of tiny operands (tools/diag/mfma_f16_denorm.hip): the self-attention core and the few-key cross-attention
    keep the kernels' tolerance when every token is scaled by 1e-4 ... 300 (the projections' outputs scale with it; the attention
    logits are kept O(1) by scaling the other operand back)."""
    B, S, E = 2, 96, 128
    q, k, v = rnd("q", (B, S, E), 1) * scale, rnd("k", (B, S, E), 2) / scale, rnd("v", (B, S, E), 3) * scale
    got = ops.attention_core(dev(q), dev(k), dev(v), None, 4)
    assert rel_dev(got, _attn_ref(q, k, v, None, 4)) < TOL
    qs, ks, vs = rnd("qs", (B, 70, E), 11) * scale, rnd("ks", (B, 24, E), 12) * scale, rnd("vs", (B, 24, E), 13) * scale
    iw = rnd("iw", (3 * E, E), 4, 2 / math.sqrt(E))
    iw[:2 * E] /= scale                                                   # q and k projections back to O(1): logits O(1 .. 10)
    ib, ow, ob = rnd("ib", (3 * E,), 5, 0.1), rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1) * scale
    ib[2 * E:] *= scale
    mask = torch.arange(24)[None, :] >= torch.tensor([24, 5])[:, None]
    ref = restate.multi_head_attention(qs, ks, vs, iw, ib, ow, ob, mask)
    cache = {}
    got = ops.mha(dev(qs), dev(ks), dev(vs), dev(iw), dev(ib), dev(ow), dev(ob), dev(mask), kv_limit=24, packed=cache).cpu()
    assert set(cache) == {"in_proj_h2", "out_proj_h2"}
    assert rel_dev(got, ref) < TOL


def test_two_term_fp16_kernels_turn_out_of_range_operands_into_non_finite_rows(ops):
    """fp16's range is the documented limit of the h2 forms: a token beyond +-65504 must come out LOUD (inf / NaN in the rows it
    feeds), never as a finite wrong number; the split3 / exact forms take the same input in their stride."""
    import os
    B, S, E = 1, 40, 128
    q, k, v = rnd("q", (B, S, E), 1), rnd("k", (B, S, E), 2), rnd("v", (B, S, E), 3)
    v[0, 7, 5] = 1.0e6                                                    # one value element beyond fp16
    got = ops.attention_core(dev(q), dev(k), dev(v), None, 4).cpu()
    assert not bool(torch.isfinite(got[0, :, 5]).all())                   # every query attends key 7 a little: column 5 of head 0
    assert bool(torch.isfinite(got[0, :, 40:]).all())                     # other heads untouched
    os.environ["OCV_ATTN_FORM"] = "fp32"
    try:
        exact = ops.attention_core(dev(q), dev(k), dev(v), None, 4).cpu()
    finally:
        del os.environ["OCV_ATTN_FORM"]
    assert bool(torch.isfinite(exact).all()) and rel_dev(exact, _attn_ref(q, k, v, None, 4)) < TOL


def test_split_h2_pack_layout_saturation_and_product_precision(ops):
    """ocv_pack_split_h2_fwd: the documented operand-order layout on a ragged [70, 40] matrix (zero padding to 32 rows / 16
    columns), saturation at fp16's range instead of inf, and what the two-term split is for: hi hi + 2^-11 (hi lo' + lo' hi)
    reproduces an fp64 product to ~3e-7 of its largest element where a two-term bf16 split gives ~5e-6."""
    N, K = 70, 40
    w = rnd("w", (N, K), 31, 0.3)
    w[3, 5], w[4, 6], w[5, 7] = 1.0e6, -3.0e5, 65504.0
    sw = ops.SplitWeightH2(dev(w))
    nsteps, ntiles = (K + 15) // 16, (N + 31) // 32
    pk = sw.packed.cpu().view(ntiles, nsteps, 2, 64, 8)
    wp = torch.zeros(ntiles * 32, nsteps * 16)
    wp[:N, :K] = w.clamp(-65504.0, 65504.0)
    hi = wp.half()
    lo = ((wp - hi.float()) * 2048.0).half()
    for part, t in ((0, hi), (1, lo)):
        exp = t.view(ntiles, 32, nsteps, 2, 8).permute(0, 2, 3, 1, 4).reshape(ntiles, nsteps, 64, 8)      # lane = 32 * half + row
        assert torch.equal(pk[:, :, part], exp)
    assert bool(torch.isfinite(pk.float()).all())
    x, v = rnd("x", (64, 128), 32).double(), rnd("v", (128, 128), 33, 0.1).double()
    ref = x @ v.T

    def h2(a):
        a = a.float()
        h = a.half()
        return h.double(), ((a - h.float()) * 2048.0).half().double()

    def bf2(a):
        a = a.float()
        h = a.bfloat16()
        return h.double(), (a - h.float()).bfloat16().double()
    (xh, xl), (vh, vl) = h2(x), h2(v)
    got = xh @ vh.T + (xh @ vl.T + xl @ vh.T) / 2048.0
    (bh, bl), (ch, cl) = bf2(x), bf2(v)
    two = bh @ ch.T + bh @ cl.T + bl @ ch.T
    e_h2, e_b2 = float((got - ref).abs().max() / ref.abs().max()), float((two - ref).abs().max() / ref.abs().max())
    assert e_h2 < 6e-7 and e_b2 > 4 * e_h2, (e_h2, e_b2)


def test_mha_few_keys_h2_on_large_tokens(ops):
    """Tokens of magnitude ~100 (far above this model's, far below fp16's 65504): the scaled low term keeps the two-term fp16
    split at fp32's relative error whatever the magnitude."""
    B, Sq, Sk, E = 3, 100, 32, 128
    qs, ks, vs = rnd("qs", (B, Sq, E), 41) * 100.0, rnd("ks", (B, Sk, E), 42) * 100.0, rnd("vs", (B, Sk, E), 43) * 100.0
    iw, ib = rnd("iw", (3 * E, E), 4, 0.02 / math.sqrt(E)), rnd("ib", (3 * E,), 5, 0.1)       # logits stay O(1 .. 10)
    ow, ob = rnd("ow", (E, E), 6, 1 / math.sqrt(E)), rnd("ob", (E,), 7, 0.1)
    mask = torch.arange(Sk)[None, :] >= torch.tensor([32, 9, 1])[:, None]
    ref = restate.multi_head_attention(qs, ks, vs, iw, ib, ow, ob, mask)
    got = ops.mha(dev(qs), dev(ks), dev(vs), dev(iw), dev(ib), dev(ow), dev(ob), dev(mask), kv_limit=32, packed={}).cpu()
    assert rel_dev(got, ref) < TOL


def _encoder_sd(seed, prefix="layers."):
    import torch.nn as nn
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(128, 4, 1024, batch_first=True), 4, enable_nested_tensor=False).eval()
    sd = gen.load_into(enc, seed, gen.PEAKY)
    return enc, sd


@pytest.mark.parametrize("mode", ["h2", "split3"])
@pytest.mark.parametrize("B,S,counts", [(2, 132, None), (1, 300, None), (3, 40, [40, 7, 1]), (16, 32, [32] * 16), (2, 1200, None), (4, 418, None)])
def test_transformer_encoder_stack(ops, monkeypatch, B, S, counts, mode):
    """nn.TransformerEncoder (4 post-norm layers) in 1 + 2 L launches: the layer tails as two-term fp16 splits (OCV_TOKENS=h2, the
    default: csrc/token_h2.hip) or as three-term bf16 splits (split3), against the oracle and against the exact-fp32 route."""
    monkeypatch.setenv("OCV_TOKENS", mode)
    from objcavit_amd.modules.layers import HipEncoderStack
    enc, sd = _encoder_sd(11)
    x = rnd("x", (B, S, 128), 12)
    mask = None if counts is None else (torch.arange(S)[None, :] >= torch.tensor(counts)[:, None])
    ref = restate.transformer_encoder(x, sd, "", mask)
    stack = HipEncoderStack(enc.cuda())
    got = stack(dev(x), None if mask is None else dev(mask))          # default: three-term-split projections / FFN
    assert rel_dev(got, ref) < 5e-5
    if mask is not None and bool(mask.any()):
        assert float(got[dev(mask)].abs().max()) == 0.0
    import os
    os.environ["OCV_TOKENS"] = "fp32"                                  # the exact-fp32 MFMA route: same answer to rounding
    try:
        exact = stack(dev(x), None if mask is None else dev(mask))
    finally:
        del os.environ["OCV_TOKENS"]
    assert rel_dev(exact, ref) < 5e-5
    ok = ~dev(mask) if mask is not None else torch.ones(B, S, dtype=torch.bool, device="cuda")
    assert rel_dev(got[ok], exact[ok]) < 2e-5


def test_layer_tails_share_their_feed_forward_out_over_workgroups_repeatably(ops):
    """Few tokens: a row block's eight feed-forward chunks go to 8 (up to 24 row blocks) or 4 (up to 56) workgroups and the LAST one to
    arrive finishes the layer (csrc/token_h2.hip; agent-scope ticket, tickets cleared once per stack call and left zero by every tail).
    Thirty back-to-back stacks per shape -- 192 / 188 workgroups per tail launch, every ticket used 4 x 30 times -- give the same bits
    every time, and the oracle's values."""
    from objcavit_amd.modules.layers import HipEncoderStack
    enc, sd = _encoder_sd(21)
    stack = HipEncoderStack(enc.cuda())
    lib = ops._lib.load()
    for B, S, G in ((4, 192, 8), (4, 370, 4), (1, 32, 8), (5, 418, 1)):      # (the stack shares out only for batches of up to 4 sequences)
        assert lib.ocv_layer_tail_h2_groups(B * S, 1024) == G
        assert (lib.ocv_layer_tail_h2_workspace_bytes(B * S, 1024) > 0) == (G > 1)
        x = rnd("x", (B, S, 128), 30 + B)
        ref = restate.transformer_encoder(x, sd, "", None)
        xd = dev(x)
        first = stack(xd).clone()
        assert rel_dev(first, ref) < 5e-5, (B, S)
        for _ in range(30):
            assert torch.equal(stack(xd), first), (B, S)


def test_encoder_layer_params_truncated_struct_reads_missing_fields_as_null(ops):
    """ABI 2: a caller built against a header without the packed-weight fields passes struct_size = size field + 12
    pointers; whatever lies behind that in memory is NOT read (here: poison pointers), the layer runs on the exact-fp32
    route and equals the full struct with the *_p3 fields NULL, bit for bit."""
    import ctypes as C
    from objcavit_amd import _lib
    enc, sd = _encoder_sd(13)
    layer = enc.cuda().layers[0]
    x = dev(rnd("x", (2, 40, 128), 14))
    full, keep = ops.layer_params(layer, None)
    ref = ops.encoder_layer(x, full)
    trunc, keep2 = ops.layer_params(layer, None)
    trunc.struct_size = 8 * 13
    for f in ("in_proj_p3", "out_proj_p3", "linear1_p3", "linear2_p3"):
        setattr(trunc, f, 0xdead0000)
    got = ops.encoder_layer(x, trunc)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert rel_dev(got, restate.encoder_layer(x.cpu(), sd, "layers.0.")) < 5e-5


# ------------------------------------------------------------------ patch embedding
@pytest.mark.parametrize("B,h,w,pos_mode", [(1, 16, 16, "none"), (2, 176, 192, "shared"), (1, 240, 320, "batched"),
                                            (3, 48, 80, "shared"), (1, 176, 608, "shared"), (2, 50, 70, "batched")])
def test_patch_embed(ops, B, h, w, pos_mode):
    C, E = 128, 128
    x = rnd("x", (B, C, h, w), 1)
    wt, b = rnd("w", (E, C, 16, 16), 2, 1 / math.sqrt(C * 256)), rnd("b", (E,), 3, 0.1)
    S = (h // 16) * (w // 16)
    pos = {"none": None, "shared": rnd("p", (S, E), 4), "batched": rnd("p", (B, S, E), 4)}[pos_mode]
    ref = F.conv2d(x, wt, b, stride=16).flatten(2).permute(0, 2, 1)
    if pos is not None:
        ref = ref + pos
    got = ops.patch_embed(dev(x), dev(wt), dev(b), None if pos is None else dev(pos))
    assert rel_dev(got, ref) < TOL


@pytest.mark.parametrize("B,C,h,w,E,pos_mode", [(2, 128, 64, 96, 128, "shared"), (16, 128, 240, 320, 128, "shared"),
                                                (1, 64, 37, 53, 40, "none"), (3, 32, 48, 50, 128, "batched"),
                                                (2, 128, 176, 608, 128, "shared"), (1, 128, 240, 320, 128, "shared"),
                                                (2, 128, 240, 320, 128, "batched")])
def test_patch_embed_split(ops, B, C, h, w, E, pos_mode):
    """ocv_patch_embed_split_fwd (16 split-bf16 GEMMs over the hl32 map in one launch + fixed-order sum) against the
    convolution in fp64, at the split-bf16 convolutions' bar; ragged widths / heights (B = 1), KITTI's half-resolution map;
    the validation loop's batches of 1 and 2 (K cut in 4 parts per patch row: 64 slabs); and bitwise repeatable."""
    x = rnd("x", (B, C, h, w), 1)
    wt, b = rnd("w", (E, C, 16, 16), 2, 1 / math.sqrt(C * 256)), rnd("b", (E,), 3, 0.1)
    S = (h // 16) * (w // 16)
    pos = {"none": None, "shared": rnd("p", (S, E), 4), "batched": rnd("p", (B, S, E), 4)}[pos_mode]
    ref = F.conv2d(x.double(), wt.double(), b.double(), stride=16).flatten(2).permute(0, 2, 1)
    if pos is not None:
        ref = ref + pos.double()
    xs = ops.split_act(dev(x).contiguous(memory_format=torch.channels_last))
    hi, lo = ops.prep_patch_embed_weight(dev(wt))
    assert ops.patch_embed_split_supported(B, C, h, w, E)
    got = ops.patch_embed_split(xs, hi, lo, dev(b), None if pos is None else dev(pos))
    assert got.shape == (B, S, E) and rel_dev(got, ref) < SPLIT_TOL
    assert torch.equal(got, ops.patch_embed_split(xs, hi, lo, dev(b), None if pos is None else dev(pos)))
    if (C, E) == (128, 128):                                  # the exact-fp32 kernel is built for the model's 128 -> 128
        exact = ops.patch_embed(dev(x), dev(wt), dev(b), None if pos is None else dev(pos))
        assert rel_dev(got, exact) < SPLIT_TOL


def test_patch_embed_split_seeded_shape_sweep(ops):
    """The patch embedding's K axis is cut in a modelled number of pieces that depends on the batch and the map (1 ... 64 pieces, each
    piece crossing patch-row boundaries wherever the cut falls): a seeded sweep over batches and map sizes, fp16 and bf16 pairs,
    against the convolution in fp64; every call bitwise repeatable."""
    rng = random.Random(1234)
    for _ in range(14):
        B = rng.choice((1, 1, 2, 3, 5, 8, 12))
        h, w = 16 * rng.randint(1, 9), 16 * rng.randint(1, 12)
        C, E = rng.choice(((128, 128), (64, 128), (32, 40), (96, 64)))
        f16 = rng.random() < 0.6
        x = rnd("x", (B, C, h, w), rng.randint(0, 999))
        wt, b = rnd("w", (E, C, 16, 16), rng.randint(0, 999), 1 / math.sqrt(C * 256)), rnd("b", (E,), 3, 0.1)
        pos = rnd("p", ((h // 16) * (w // 16), E), 4)
        ref = F.conv2d(x.double(), wt.double(), b.double(), stride=16).flatten(2).permute(0, 2, 1) + pos.double()
        xs = ops.split_act(dev(x).contiguous(memory_format=torch.channels_last), f16)
        prep = ops.prep_patch_embed_weight(dev(wt), f16)
        call = lambda: ops.patch_embed_split(xs, prep[0], prep[1], dev(b), dev(pos), oscale=prep[2] if f16 else None)
        got = call()
        assert rel_dev(got, ref) < SPLIT_TOL, (B, C, h, w, E, f16)
        assert torch.equal(got, call()), (B, C, h, w, E, f16)


def test_patch_embed_split_rejects_what_it_cannot_address(ops):
    assert not ops.patch_embed_split_supported(2, 128, 40, 64, 128)       # two images, height not a multiple of 16
    assert not ops.patch_embed_split_supported(1, 24, 64, 64, 128)        # channels not whole hi|lo blocks
    xs = ops.split_act(dev(rnd("x", (2, 128, 40, 64), 1)).contiguous(memory_format=torch.channels_last))
    hi, lo = ops.prep_patch_embed_weight(dev(rnd("w", (128, 128, 16, 16), 2, 0.01)))
    with pytest.raises(ValueError):
        ops.patch_embed_split(xs, hi, lo, None, None)


def test_patch_embed_is_deterministic(ops):
    x, wt, b = dev(rnd("x", (4, 128, 96, 128), 1)), dev(rnd("w", (128, 128, 16, 16), 2, 0.01)), dev(rnd("b", (128,), 3))
    a = ops.patch_embed(x, wt, b, None).clone()
    for _ in range(3):
        assert torch.equal(a, ops.patch_embed(x, wt, b, None))      # fixed-order split-K reduction, no atomics


# ------------------------------------------------------------------ pixel-wise dot / bin head
@pytest.mark.parametrize("B,h,w", [(1, 8, 16), (2, 176, 192), (1, 240, 320), (3, 37, 53)])
def test_pixel_dot(ops, B, h, w):
    feat, q = rnd("f", (B, 128, h, w), 1), rnd("q", (B, 300, 128), 2)
    queries = q[:, 1:129, :]
    ref = restate.pixel_wise_dot_product(feat, queries)
    got = ops.pixel_dot(dev(feat), dev(q)[:, 1:129, :])
    assert rel_dev(got, ref) < TOL


@pytest.mark.parametrize("B,h,w", [(1, 8, 16), (2, 176, 192), (1, 240, 320), (5, 37, 53)])
def test_bin_head(ops, B, h, w):
    feat, q = rnd("f", (B, 128, h, w), 1), rnd("q", (B, 300, 128), 2, 0.5)
    wout, bout = rnd("wo", (256, 128, 1, 1), 3, 6 / math.sqrt(128)), rnd("bo", (256,), 4, 0.5)
    widths = torch.rand(B, 256, generator=torch.Generator().manual_seed(5)) + 0.1
    widths = widths / widths.sum(1, keepdim=True)
    queries = q[:, 1:129, :]
    ram = restate.pixel_wise_dot_product(feat, queries)
    ref_depth, ref_edges = restate.bin_head(widths, ram, wout, bout, 0.001, 10.0)
    from objcavit_amd.modules.AdaBins import bin_edges_and_centers
    edges, centers = bin_edges_and_centers(dev(widths), 0.001, 10.0)
    got = ops.bin_head(dev(feat), dev(q)[:, 1:129, :], dev(wout), dev(bout), centers)
    assert rel_dev(edges, ref_edges) < 1e-6
    # north-star tolerance is 1e-3 relative on depth; fp32 end to end gives far better
    assert float(((got.cpu() - ref_depth).abs() / ref_depth).max()) < 1e-4
    assert float(ref_depth.max() - ref_depth.min()) > 0.5      # the softmax is not trivially flat


# ------------------------------------------------------------------ channels_last (NHWC) operands
@pytest.mark.parametrize("B,h,w", [(2, 176, 192), (1, 240, 320), (3, 48, 80)])
def test_patch_embed_channels_last(ops, B, h, w):
    x = rnd("x", (B, 128, h, w), 1)
    wt, b = rnd("w", (128, 128, 16, 16), 2, 1 / math.sqrt(128 * 256)), rnd("b", (128,), 3, 0.1)
    S = (h // 16) * (w // 16)
    pos = rnd("p", (S, 128), 4)
    ref = F.conv2d(x, wt, b, stride=16).flatten(2).permute(0, 2, 1) + pos
    xg = dev(x).contiguous(memory_format=torch.channels_last)
    assert not xg.is_contiguous()
    got = ops.patch_embed(xg, dev(wt), dev(b), dev(pos))
    assert rel_dev(got, ref) < TOL
    # a channels_last weight parameter is consumed in place
    got2 = ops.patch_embed(xg, dev(wt).contiguous(memory_format=torch.channels_last), dev(b), dev(pos))
    assert torch.equal(got, got2)


@pytest.mark.parametrize("B,h,w", [(2, 176, 192), (1, 240, 320), (3, 37, 53)])
def test_pixel_dot_and_bin_head_channels_last(ops, monkeypatch, B, h, w):
    from objcavit_amd.modules.AdaBins import bin_edges_and_centers
    feat, q = rnd("f", (B, 128, h, w), 1), rnd("q", (B, 300, 128), 2, 0.5)
    wout, bout = rnd("wo", (256, 128, 1, 1), 3, 6 / math.sqrt(128)), rnd("bo", (256,), 4, 0.5)
    widths = torch.rand(B, 256, generator=torch.Generator().manual_seed(5)) + 0.1
    widths = widths / widths.sum(1, keepdim=True)
    fg = dev(feat).contiguous(memory_format=torch.channels_last)
    qg = dev(q)[:, 1:129, :]
    ram = restate.pixel_wise_dot_product(feat, q[:, 1:129, :])
    got_ram = ops.pixel_dot(fg, qg)
    assert got_ram.is_contiguous() and rel_dev(got_ram, ram) < TOL
    ref_depth, _ = restate.bin_head(widths, ram, wout, bout, 0.001, 10.0)
    _, centers = bin_edges_and_centers(dev(widths), 0.001, 10.0)
    # NHWC: the two faithful split forms -- two-term fp16 with a scaled low term, all 256 bins per workgroup (the default), and
    # three-term bf16 in two bin halves + merge -- are both held to the exact kernel's error: against an fp64 evaluation of the
    # same folded logits (this input is the stress case: logit gain 6, near-one-hot softmax over 256 bins) within 2x of
    # the exact v_mfma_f32_32x32x2_f32 kernel
    d64, _ = restate.bin_head(widths.double(), restate.pixel_wise_dot_product(feat.double(), q[:, 1:129, :].double()),
                              wout.double(), bout.double(), 0.001, 10.0)
    exact = ops.bin_head(fg, qg, dev(wout), dev(bout), centers, exact=True)
    ex = float(((exact.cpu().double() - d64).abs() / d64).max())
    for mode in ("split3", "h2dense", "h2"):
        monkeypatch.setenv("OCV_BINHEAD", mode)
        got = ops.bin_head(fg, qg, dev(wout), dev(bout), centers)
        assert float(((got.cpu() - ref_depth).abs() / ref_depth).max()) < 1e-4, mode
        e3 = float(((got.cpu().double() - d64).abs() / d64).max())
        assert e3 < 1e-4 and e3 <= 2.0 * ex + 2e-6, (mode, e3, ex)
        assert torch.equal(got, ops.bin_head(fg, qg, dev(wout), dev(bout), centers))
    monkeypatch.delenv("OCV_BINHEAD")
    assert torch.equal(got, ops.bin_head(fg, qg, dev(wout), dev(bout), centers))          # h2 is the default
    # NCHW and NHWC paths agree to rounding
    got_nchw = ops.bin_head(dev(feat), qg, dev(wout), dev(bout), centers)
    assert float(((got - got_nchw).abs() / got_nchw).max()) < 1e-4      # different K order inside the MFMA chains
    # inside hip_ops.bf16_pairs() -- the fp16 range guard's fallback route -- the head takes the form with fp32's range (split3)
    monkeypatch.setenv("OCV_BINHEAD", "split3")
    want = ops.bin_head(fg, qg, dev(wout), dev(bout), centers)
    monkeypatch.delenv("OCV_BINHEAD")
    with ops.bf16_pairs():
        assert torch.equal(ops.bin_head(fg, qg, dev(wout), dev(bout), centers), want)
    big = (fg * 1e6).contiguous(memory_format=torch.channels_last)       # a map far beyond fp16's range, queries scaled the other way
    with ops.bf16_pairs():
        far = ops.bin_head(big, qg / 1e6, dev(wout), dev(bout), centers)
    assert bool(torch.isfinite(far).all()) and float(((far - want).abs() / want).max()) < 1e-4


@pytest.mark.parametrize("B,C,H,W,Cout,layout", [(2, 3, 33, 47, 128, "nchw"), (1, 3, 480, 640, 128, "nchw"), (2, 4, 16, 17, 8, "nhwc"),
                                                (1, 1, 1, 1, 4, "nchw"), (3, 2, 5, 9, 260, "nhwc"), (2, 3, 20, 8, 132, "view")])
def test_conv3x3_few_channels(ops, B, C, H, W, Cout, layout):
    """ocv_conv3x3_few_channels_fwd (the skip part of the last decoder stage of do_final_upscale models: the skip tensor is the
    image): exact fp32, zero padding, any dense layout of the image read through its strides (NCHW, channels_last, a channel
    slice of a wider tensor), ragged tiles (8-pixel column groups, 16-row blocks, 128-channel blocks)."""
    x, w = rnd("x", (B, C, H, W), 1), rnd("w", (Cout, C, 3, 3), 2, 0.4)
    ref = F.conv2d(x.double(), w.double(), padding=1).float()
    xg = dev(x)
    if layout == "nhwc":
        xg = xg.contiguous(memory_format=torch.channels_last)
    elif layout == "view":
        wide = torch.zeros(B, C + 2, H, W, device="cuda")
        wide[:, 1:1 + C] = xg
        xg = wide[:, 1:1 + C]
        assert not xg.is_contiguous()
    got = ops.conv3x3_few_channels(xg, dev(w).permute(2, 3, 1, 0).reshape(9, C, Cout).contiguous())
    assert got.shape == (B, Cout, H, W) and got.is_contiguous(memory_format=torch.channels_last)
    assert rel_dev(got, ref) < 2e-6


@pytest.mark.parametrize("scale", [1e-3, 64.0])
def test_bin_head_h2_on_scaled_maps(ops, monkeypatch, scale):
    """The two-term fp16 bin head on a map scaled down / up with the queries scaled the other way (same logits): depth as for the
    unscaled pair, to the exact kernel's noise -- tiny map values (subnormal fp16 high terms) lose nothing."""
    from objcavit_amd.modules.AdaBins import bin_edges_and_centers
    B, h, w = 2, 30, 40
    feat, q = rnd("f", (B, 128, h, w), 1), rnd("q", (B, 128, 128), 2, 0.5)
    wout, bout = rnd("wo", (256, 128, 1, 1), 3, 2 / math.sqrt(128)), rnd("bo", (256,), 4, 0.5)
    widths = torch.rand(B, 256, generator=torch.Generator().manual_seed(5)) + 0.1
    widths = widths / widths.sum(1, keepdim=True)
    _, centers = bin_edges_and_centers(dev(widths), 0.001, 10.0)
    fg = dev(feat).contiguous(memory_format=torch.channels_last)
    monkeypatch.setenv("OCV_BINHEAD", "exact")
    ref = ops.bin_head(fg, dev(q), dev(wout), dev(bout), centers)
    monkeypatch.setenv("OCV_BINHEAD", "h2")
    got = ops.bin_head((fg * scale).contiguous(memory_format=torch.channels_last), dev(q) / scale, dev(wout), dev(bout), centers)
    assert float(((got - ref).abs() / ref).max()) < 5e-5


@pytest.mark.parametrize("norm", ["linear", "sigmoid"])
@pytest.mark.parametrize("B,E,H1,H2,n", [(16, 128, 256, 256, 256), (1, 128, 256, 256, 256), (3, 64, 100, 36, 80), (2, 128, 256, 256, 1000)])
def test_regressor_bins_one_launch(ops, norm, B, E, H1, H2, n):
    """ocv_regressor_bins_fwd (the bin regressor's three layers + normalisation + edges + centres in one launch, one workgroup per
    image) against the reference's formulation in fp64 (modules/miniViT.py:33-42, AdaBins.py:79-83) and against the launches it
    replaces (three ocv_linear_fwd + ocv_bin_edges_fwd); the head rows are a strided view of a token tensor, as in the model."""
    tok = rnd("tok", (B, 7, E), 1)
    par = [rnd("w1", (H1, E), 2, 1 / math.sqrt(E)), rnd("b1", (H1,), 3, 0.2), rnd("w2", (H2, H1), 4, 1 / math.sqrt(H1)), rnd("b2", (H2,), 5, 0.2),
           rnd("w3", (n, H2), 6, 2 / math.sqrt(H2)), rnd("b3", (n,), 7, 0.2)]
    head = dev(tok)[:, 0, :]
    assert not head.is_contiguous() or B == 1
    w, e, c = ops.regressor_bins(head, *[dev(t) for t in par], norm, 0.001, 10.0)
    x = tok[:, 0, :].double()
    y = F.leaky_relu(x @ par[0].double().T + par[1].double(), 0.01)
    y = F.leaky_relu(y @ par[2].double().T + par[3].double(), 0.01)
    y = y @ par[4].double().T + par[5].double()
    y = torch.relu(y) + 0.1 if norm == "linear" else torch.sigmoid(y)
    wr = y / y.sum(1, keepdim=True)
    er = torch.cumsum(F.pad((10.0 - 0.001) * wr, (1, 0), value=0.001), 1)
    cr = 0.5 * (er[:, :-1] + er[:, 1:])
    assert rel_dev(w, wr.float()) < 2e-6 and rel_dev(e, er.float()) < 2e-6 and rel_dev(c, cr.float()) < 2e-6
    g = [dev(t) for t in par]
    y3 = ops.linear(ops.linear(ops.linear(head.contiguous(), g[0], g[1], ops.ACT_LEAKY_RELU), g[2], g[3], ops.ACT_LEAKY_RELU), g[4], g[5],
                    ops.ACT_NONE)
    w3, e3, c3 = ops.bin_edges(y3, norm, 0.001, 10.0)
    assert rel_dev(w, w3.cpu()) < 2e-6 and rel_dev(e, e3.cpu()) < 2e-6 and rel_dev(c, c3.cpu()) < 2e-6
    assert torch.equal(w, ops.regressor_bins(head, *g, norm, 0.001, 10.0)[0])


@pytest.mark.parametrize("gain", [0.02, 0.6, 6.0, 40.0])
def test_bin_head_two_level_logits_against_every_tile_in_full(ops, monkeypatch, gain):
    """The default bin head forms every bin coarsely and only the 32-bin tiles near a pixel's maximum in full (csrc/bin_head.hip).
    Flat softmaxes (small logit gain): every tile is kept; peaked ones (gain 6, 40): most are dropped, and the dropped bins weigh
    <= 224 e^-24.  What differs from the one-level kernel is the path of the online softmax's running maximum, i.e. rounding: the
    two-level depth is held to the same bound as every faithful form -- against an fp64 evaluation of the same folded logits,
    within 2x of the exact-fp32 MFMA kernel's own error (tools/exp_binhead_two_level.py prints the three side by side).  A NaN /
    inf / beyond-fp16 map value reaches its pixel's depth in both kernels alike (a non-finite pixel keeps every tile), and its
    neighbours in the same 32-pixel group stay as they were."""
    from objcavit_amd.modules.AdaBins import bin_edges_and_centers
    B, h, w = 2, 37, 53                                                  # ragged: the last 32-pixel groups are partly beyond the map
    feat, q = rnd("f", (B, 128, h, w), 11), rnd("q", (B, 128, 128), 12, 0.5)
    wout, bout = rnd("wo", (256, 128, 1, 1), 13, gain / math.sqrt(128)), rnd("bo", (256,), 14, 0.5)
    widths = torch.rand(B, 256, generator=torch.Generator().manual_seed(15)) + 0.1
    widths = widths / widths.sum(1, keepdim=True)
    _, centers = bin_edges_and_centers(dev(widths), 0.001, 10.0)
    fg = dev(feat).contiguous(memory_format=torch.channels_last)
    run = lambda m, f=fg: (monkeypatch.setenv("OCV_BINHEAD", m), ops.bin_head(f, dev(q), dev(wout), dev(bout), centers))[1]   # noqa: E731
    dense, two, exact = run("h2dense"), run("h2"), run("exact")
    d64, _ = restate.bin_head(widths.double(), restate.pixel_wise_dot_product(feat.double(), q.double()), wout.double(), bout.double(),
                              0.001, 10.0)
    err = lambda t: float(((t.cpu().double() - d64).abs() / d64).max())   # noqa: E731
    ex = err(exact)
    assert err(two) <= 2.0 * ex + 2e-6 and err(dense) <= 2.0 * ex + 2e-6, (err(two), err(dense), ex)
    assert float(((two - dense).abs() / dense).max()) <= 2.0 * ex + 2e-6
    bad = fg.clone()
    bad[0, 5, 3, 7] = float("nan")
    bad[1, 9, 20, 40] = float("inf")
    bad[1, 100, 36, 52] = 1e6                                            # beyond fp16: hi = inf
    d2, t2 = run("h2dense", bad), run("h2", bad)
    for (b, y, x) in ((0, 3, 7), (1, 20, 40), (1, 36, 52)):
        assert not bool(torch.isfinite(d2[b, 0, y, x])) and not bool(torch.isfinite(t2[b, 0, y, x]))
    ok = torch.isfinite(d2)
    assert torch.equal(ok, torch.isfinite(t2)) and int((~ok).sum()) == 3
    assert float(((t2[ok] - d2[ok]).abs() / d2[ok]).max()) <= 2.0 * ex + 2e-6


# ------------------------------------------------------------------ depthwise convolution
def _same_pad(x, k, s):
    ih, iw = x.shape[-2:]
    ph = max((math.ceil(ih / s) - 1) * s + k - ih, 0)
    pw = max((math.ceil(iw / s) - 1) * s + k - iw, 0)
    return F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("B,C,H,W", [(2, 48, 240, 320), (1, 7, 15, 20), (3, 5, 33, 47), (1, 3, 1, 1), (2, 16, 30, 40)])
@pytest.mark.parametrize("act", [0, 3])
def test_depthwise_conv_same(ops, k, s, B, C, H, W, act):
    x, w, b = rnd("x", (B, C, H, W), 1), rnd("w", (C, 1, k, k), 2, 0.3), rnd("b", (C,), 3, 0.2)
    ref = F.conv2d(_same_pad(x, k, s), w, b, stride=s, groups=C)
    if act == 3:
        ref = F.silu(ref)
    got = ops.depthwise_conv_same(dev(x), dev(w), dev(b), s, act)
    assert got.shape == ref.shape
    assert rel_dev(got, ref) < TOL


# ------------------------------------------------------------------ split-bf16 implicit-GEMM convolution
SPLIT_TOL = 2e-5     # hi+lo carries 16 bits, 3 of 4 partial products kept: ~1e-6 measured, bound stated in the kernel


@pytest.mark.parametrize("B,H,W,C1,C2,Cout,k,act", [
    (2, 30, 40, 64, 24, 128, 3, 2),       # concat, Cin = 88 (not a multiple of 32)
    (1, 17, 23, 32, 0, 40, 3, 0),         # ragged M, Cout < tile
    (3, 16, 16, 128, 0, 128, 3, 0),       # conv3x3 of the heads
    (1, 240, 320, 128, 0, 128, 3, 0),     # full NYU head size
    (2, 15, 20, 256, 176, 256, 3, 2),     # decoder-like
    (2, 9, 11, 96, 0, 200, 1, 3),         # 1x1 + SiLU, two N tiles
    (1, 5, 7, 4, 0, 8, 3, 1),             # tiny
])
def test_conv_nhwc_split_bf16(ops, B, H, W, C1, C2, Cout, k, act):
    x1 = rnd("x1", (B, C1, H, W), 1)
    x2 = rnd("x2", (B, C2, H, W), 2) if C2 else None
    w, b = rnd("w", (Cout, C1 + C2, k, k), 3, 1 / math.sqrt((C1 + C2) * k * k)), rnd("b", (Cout,), 4, 0.2)
    xin = x1 if x2 is None else torch.cat([x1, x2], 1)
    ref = F.conv2d(xin.double(), w.double(), b.double(), padding=k // 2).float()
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act]
    hi, lo = ops.prep_conv_weight(dev(w))
    cl = torch.channels_last
    got = ops.conv_nhwc(dev(x1).contiguous(memory_format=cl), None if x2 is None else dev(x2).contiguous(memory_format=cl),
                        hi, lo, dev(b), k, act)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=cl)
    assert rel_dev(got, ref) < SPLIT_TOL
    res = rnd("res", tuple(ref.shape), 5)
    got = ops.conv_nhwc(dev(x1), None if x2 is None else dev(x2), hi, lo, dev(b), k, act, residual=dev(res))
    assert rel_dev(got, ref + res) < SPLIT_TOL


def test_conv_nhwc_split_bf16_error_is_small_for_large_dynamic_range(ops):
    """Operands spanning 6 decades: the split representation keeps fp32's exponent range (unlike fp16)."""
    x = rnd("x", (1, 64, 12, 12), 1) * torch.logspace(-3, 3, 64).view(1, 64, 1, 1)
    w = rnd("w", (32, 64, 3, 3), 2, 0.05) / torch.logspace(-3, 3, 64).view(1, 64, 1, 1)
    ref = F.conv2d(x.double(), w.double(), None, padding=1).float()
    hi, lo = ops.prep_conv_weight(dev(w))
    got = ops.conv_nhwc(dev(x), None, hi, lo, None, 3)
    assert rel_dev(got, ref) < SPLIT_TOL


# ------------------------------------------------------------------ NHWC encoder blocks
@pytest.mark.parametrize("B,H,W,Cin,Cout,act,use_gate,use_res", [
    (2, 30, 40, 24, 144, 3, False, False),      # expand + SiLU
    (2, 30, 40, 144, 24, 0, True, True),        # project with SE gate + skip (Cout <= 32 -> 128-row tiles)
    (1, 15, 20, 512, 2048, 0, False, False),    # conv_head
    (3, 7, 9, 240, 40, 0, True, False),         # Cout <= 64 tile
    (1, 5, 5, 3072, 512, 0, True, True),        # K > one chunk
    (2, 4, 4, 48, 200, 4, False, False),        # sigmoid, ragged N
])
def test_pointwise_nhwc(ops, B, H, W, Cin, Cout, act, use_gate, use_res):
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 1, 1), 2, 1 / math.sqrt(Cin)), rnd("b", (Cout,), 3, 0.2)
    gate = torch.sigmoid(rnd("g", (B, Cin), 4)) if use_gate else None
    res = rnd("r", (B, Cout, H, W), 5) if use_res else None
    xin = x if gate is None else x * gate[:, :, None, None]
    ref = F.conv2d(xin, w, b)
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref), torch.sigmoid(ref)][act]
    if res is not None:
        ref = ref + res
    cl = torch.channels_last
    got = ops.pointwise_nhwc(dev(x).contiguous(memory_format=cl), dev(w), dev(b), act,
                             gate=None if gate is None else dev(gate),
                             residual=None if res is None else dev(res).contiguous(memory_format=cl))
    assert got.shape == ref.shape and got.is_contiguous(memory_format=cl)
    assert rel_dev(got, ref) < TOL


@pytest.mark.parametrize("B,H,W,Cin,Cout,act,use_gate,use_res", [
    (2, 60, 80, 24, 144, 3, False, False),      # Cin <= 32, Kp = 32 > Cin
    (2, 60, 80, 48, 24, 0, True, False),        # Cin <= 64, gate, one ragged channel tile
    (1, 64, 80, 40, 240, 3, False, False),      # Cin % 16 == 8
    (3, 40, 40, 128, 768, 3, False, False),     # Cin = 128, 24 channel tiles
    (2, 33, 67, 64, 200, 4, True, True),        # ragged M and N, sigmoid
    (2, 30, 40, 144, 24, 0, True, True),        # <= 32 channels
    (1, 8, 8, 512, 24, 0, True, True),          # long K, few channels
    (3, 7, 9, 240, 40, 0, True, False),         # <= 64 channels, ragged rows
    (1, 15, 20, 1824, 304, 0, True, True),      # two K groups, K not a multiple of the slab, ragged channel block
    (1, 5, 5, 3072, 512, 0, True, True),        # two K groups
    (1, 15, 20, 512, 2048, 0, False, False),    # conv_head
    (3, 7, 9, 40, 72, 3, False, False),         # Cin % 16 == 8, small M
    (2, 4, 4, 136, 200, 4, False, False),       # Kp = 144, sigmoid, ragged N
    (2, 30, 40, 176, 1056, 3, False, False),    # stage-5 expand
    (4, 120, 160, 240, 40, 0, True, True),      # many rows
])
def test_pointwise_nhwc_split(ops, B, H, W, Cin, Cout, act, use_gate, use_res):
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 1, 1), 2, 1 / math.sqrt(Cin)), rnd("b", (Cout,), 3, 0.2)
    gate = torch.sigmoid(rnd("g", (B, Cin), 4)) if use_gate else None
    res = rnd("r", (B, Cout, H, W), 5) if use_res else None
    xin = x if gate is None else x * gate[:, :, None, None]
    ref = F.conv2d(xin, w, b)
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref), torch.sigmoid(ref)][act]
    if res is not None:
        ref = ref + res
    cl = torch.channels_last
    sw = ops.SplitWeight(dev(w))
    assert sw.kp == (Cin + 15) // 16 * 16 and sw.packed.numel() == ops._lib.load().ocv_pointwise_packed_weight_elems(Cin, Cout)
    xg = dev(x).contiguous(memory_format=cl)
    kw = dict(gate=None if gate is None else dev(gate), residual=None if res is None else dev(res).contiguous(memory_format=cl))
    got = ops.pointwise_nhwc(xg, sw, dev(b), act, **kw)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=cl)
    assert rel_dev(got, ref) < SPLIT_TOL
    assert torch.equal(got, ops.pointwise_nhwc(xg, sw, dev(b), act, **kw))      # fixed-order K-group reduction


@pytest.mark.parametrize("cfg", [(3, 4, 1), (3, 4, 2), (3, 2, 1), (3, 2, 2), (3, 4, 4), (3, 2, 4)])      # (.., 4): four K groups, round 4
@pytest.mark.parametrize("B,H,W,Cin,Cout,act,use_gate,use_res", [
    (2, 30, 40, 176, 1056, 3, False, False),    # stage-5 expand: 11 K steps, 33 channel tiles
    (2, 30, 40, 1056, 176, 0, True, True),      # stage-5 project: ragged channel block, rows spanning two images per tile
    (1, 15, 20, 1824, 304, 0, True, True),      # 300 rows, K = 114 steps
    (2, 9, 11, 136, 200, 4, False, True),       # Kp = 144, 198 rows, ragged everything, sigmoid
    (1, 4, 5, 128, 102, 1, False, True),        # N % 4 != 0: the per-element store path
])
def test_pointwise_nhwc_split_pinned_tile_shapes(ops, cfg, B, H, W, Cin, Cout, act, use_gate, use_res):
    """Every shape of the 32-row tile kernel (2 | 4 wavefronts across channels x 1 | 2 | 4 K groups), pinned through
    ocv_pointwise_split_set_dispatch instead of left to the automatic choice, on late-stage layer shapes and ragged
    M / N / K; the automatic dispatch must agree with each of them to fp32 summation order."""
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 1, 1), 2, 1 / math.sqrt(Cin)), rnd("b", (Cout,), 3, 0.2)
    gate = torch.sigmoid(rnd("g", (B, Cin), 4)) if use_gate else None
    res = rnd("r", (B, Cout, H, W), 5) if use_res else None
    xin = x if gate is None else x * gate[:, :, None, None]
    ref = F.conv2d(xin.double(), w.double(), b.double())
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref), torch.sigmoid(ref)][act]
    if res is not None:
        ref = ref + res
    cl = torch.channels_last
    sw = ops.SplitWeight(dev(w))
    xg = dev(x).contiguous(memory_format=cl)
    kw = dict(gate=None if gate is None else dev(gate), residual=None if res is None else dev(res).contiguous(memory_format=cl))
    lib = ops._lib.load()
    try:
        assert lib.ocv_pointwise_split_set_dispatch(*cfg) == 0
        got = ops.pointwise_nhwc(xg, sw, dev(b), act, **kw)
        again = ops.pointwise_nhwc(xg, sw, dev(b), act, **kw)
    finally:
        lib.ocv_pointwise_split_set_dispatch(0, 0, 0)
    assert rel_dev(got, ref) < SPLIT_TOL and torch.equal(got, again)
    assert rel_dev(ops.pointwise_nhwc(xg, sw, dev(b), act, **kw), got) < SPLIT_TOL
    assert lib.ocv_pointwise_split_set_dispatch(9, 0, 0) == -1


@pytest.mark.parametrize("B,H,W,Cin,Cout,act,use_gate,use_res,split", [
    (1, 15, 20, 3072, 512, 0, True, True, True),      # stage-7 project at the reference's batch: 10 x 4 tiles, K = 3072 -> 6 slices
    (2, 15, 20, 1824, 304, 0, True, True, True),      # stage-6 project of an image + mirror pair: 19 x 3 tiles -> 4 slices
    (1, 15, 20, 1824, 304, 3, False, False, True),    # SiLU in the finish pass
    (1, 9, 11, 1040, 102, 0, True, True, False),      # N % 4 != 0: never split
    (4, 15, 20, 1824, 304, 0, True, True, True),      # 114 tiles -> 2 slices
    (8, 15, 20, 1824, 304, 0, True, True, False),     # 225 tiles: the chip is busy enough, no split
])
def test_pointwise_nhwc_split_k_across_workgroups(ops, B, H, W, Cin, Cout, act, use_gate, use_res, split):
    """Round 4: a tiny batch's late 1x1 layers share the K slabs of a tile out over several workgroups (raw partial tiles in the
    caller's scratch + a fixed-order finish pass with bias / activation / residual): against fp64, bitwise reproducible, and the
    scratch query says where it applies.
    The deterministic form of this check -- every operand and workspace between poisoned guards -- is tests/test_hip_memory_bounds.py."""
    lib = ops._lib.load()
    assert (lib.ocv_pointwise_split_workspace_bytes(B * H * W, Cin, Cout) > 0) == split
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 1, 1), 2, 1 / math.sqrt(Cin)), rnd("b", (Cout,), 3, 0.2)
    gate = torch.sigmoid(rnd("g", (B, Cin), 4)) if use_gate else None
    res = rnd("r", (B, Cout, H, W), 5) if use_res else None
    xin = x if gate is None else x * gate[:, :, None, None]
    ref = F.conv2d(xin.double(), w.double(), b.double())
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref), torch.sigmoid(ref)][act]
    if res is not None:
        ref = ref + res
    cl = torch.channels_last
    sw = ops.SplitWeight(dev(w))
    xg = dev(x).contiguous(memory_format=cl)
    kw = dict(gate=None if gate is None else dev(gate), residual=None if res is None else dev(res).contiguous(memory_format=cl))
    poison = [torch.full((1 << 22,), float("nan"), device="cuda") for _ in range(4)]
    del poison                                                  # the scratch comes out of NaN-filled memory
    got = ops.pointwise_nhwc(xg, sw, dev(b), act, **kw)
    assert rel_dev(got, ref) < SPLIT_TOL and torch.equal(got, ops.pointwise_nhwc(xg, sw, dev(b), act, **kw))


@pytest.mark.parametrize("B,H,W,Cin,Cout,gate", [(16, 120, 160, 40, 240, False), (16, 240, 320, 48, 24, True), (16, 120, 160, 240, 40, True)])
def test_pointwise_nhwc_split_many_rows(ops, B, H, W, Cin, Cout, gate):
    """Full-size stage-1/2 shapes: these take the rows (Cin <= 128) / stream (<= 32 channels) / tile kernels."""
    x = torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(1))
    w, b = rnd("w", (Cout, Cin, 1, 1), 2, 1 / math.sqrt(Cin)), rnd("b", (Cout,), 3, 0.2)
    g = torch.sigmoid(rnd("g", (B, Cin), 4)) if gate else None
    ref = F.conv2d(x if g is None else x * g[:, :, None, None], w, b)
    got = ops.pointwise_nhwc(dev(x).contiguous(memory_format=torch.channels_last), ops.SplitWeight(dev(w)), dev(b), 0,
                             gate=None if g is None else dev(g))
    assert rel_dev(got, ref) < SPLIT_TOL


def test_pointwise_nhwc_split_keeps_fp32_range(ops):
    """Channels spanning 6 decades: the split form keeps fp32's exponent range and ~16 mantissa bits."""
    x = rnd("x", (2, 64, 12, 12), 1) * torch.logspace(-3, 3, 64).view(1, 64, 1, 1)
    w = rnd("w", (96, 64, 1, 1), 2, 0.05) / torch.logspace(-3, 3, 64).view(1, 64, 1, 1)
    ref = F.conv2d(x.double(), w.double()).float()
    got = ops.pointwise_nhwc(dev(x).contiguous(memory_format=torch.channels_last), ops.SplitWeight(dev(w)), None, 0)
    assert rel_dev(got, ref) < SPLIT_TOL


def _to_split_act(ops, x):
    """fp32 [B, C, H, W] -> SplitAct on the GPU (the resize kernel at scale 1), plus the value it holds (hi + lo)."""
    s = ops.split_act(dev(x).contiguous(memory_format=torch.channels_last))
    return s, s.float().cpu()


@pytest.mark.parametrize("cfg", [(0, 0), (1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2)])
@pytest.mark.parametrize("B,H,W,Cin,Cout,act,use_res,outs", [
    (2, 30, 40, 176, 1056, 3, False, "f"),      # stage-5 expand: K = 11 steps (3 slabs, last one short), 33 channel blocks
    (2, 15, 20, 304, 1824, 3, False, "f"),      # stage-6 expand: Cp = 320 (5 hl32 blocks: half a slab at the end)
    (1, 15, 20, 512, 3072, 3, False, "fs"),     # stage-7 expand, both outputs
    (2, 30, 40, 1056, 176, 0, True, "fs"),      # project: ragged channel block (176 = 5.5 x 32), pad channels of the split copy
    (3, 7, 9, 128, 304, 0, True, "s"),          # 63 rows per image, split output only (Cpo = 320)
    (2, 9, 11, 136, 200, 4, True, "f"),         # Kp = 144 (Cin % 16 == 8), ragged everything, sigmoid
    (1, 4, 5, 64, 36, 1, False, "f"),           # one slab, N = 36 (not a multiple of 8), ReLU
])
def test_pointwise_hl(ops, cfg, B, H, W, Cin, Cout, act, use_res, outs):
    """ocv_pointwise_hl_fwd (pre-split rows by LDS-DMA) on every wavefront tile shape, pinned through
    ocv_pointwise_hl_set_dispatch, against float64 of the same contraction; ragged M / N / K; fp32 and / or split output."""
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 1, 1), 2, 1 / math.sqrt(Cin)), rnd("b", (Cout,), 3, 0.2)
    res = rnd("r", (B, Cout, H, W), 5) if use_res else None
    xs, _ = _to_split_act(ops, x)
    ref = F.conv2d(x.double(), w.double(), b.double())
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref), torch.sigmoid(ref)][act]
    if res is not None:
        ref = ref + res
    cl = torch.channels_last
    sw = ops.SplitWeight(dev(w))
    kw = dict(residual=None if res is None else dev(res).contiguous(memory_format=cl), out_fp32="f" in outs, out_split="s" in outs)
    lib = ops._lib.load()
    try:
        assert lib.ocv_pointwise_hl_set_dispatch(*cfg) == 0
        got = ops.pointwise_hl(xs, sw, dev(b), act, **kw)
        again = ops.pointwise_hl(xs, sw, dev(b), act, **kw)
    finally:
        lib.ocv_pointwise_hl_set_dispatch(0, 0)
    y, ys = (got if outs == "fs" else (got, None)) if "f" in outs else (None, got)
    y2, ys2 = (again if outs == "fs" else (again, None)) if "f" in outs else (None, again)
    if y is not None:
        assert y.shape == ref.shape and y.is_contiguous(memory_format=cl)
        assert rel_dev(y, ref) < SPLIT_TOL and torch.equal(y, y2)
    if ys is not None:
        assert tuple(ys.shape) == tuple(ref.shape) and ys.hl.shape[-1] == 2 * ((Cout + 31) // 32 * 32)
        assert rel_dev(ys.float(), ref) < SPLIT_TOL and torch.equal(ys.hl, ys2.hl)
        if y is not None:                                              # the split copy is the split of the fp32 result
            hi = y.to(torch.bfloat16)
            assert torch.equal(ys.hi.contiguous(), hi) and torch.equal(ys.lo.contiguous(), (y - hi.float()).to(torch.bfloat16))
        pad = ys.hl.view(B, H, W, -1, 2, 32)[..., Cout // 32:, :, :].reshape(B, H, W, -1) if Cout % 32 else None
        if pad is not None:                                            # pad channels of the last block are written as zero
            blk = ys.hl.view(B, H, W, -1, 2, 32)[:, :, :, Cout // 32]
            assert float(blk[..., Cout % 32:].float().abs().max()) == 0.0
    assert lib.ocv_pointwise_hl_set_dispatch(3, 1) == -1


@pytest.mark.parametrize("cfg", [(0, 0), (1, 1), (2, 2), (4, 1)])
@pytest.mark.parametrize("k,s,B,C,H,W,R,N", [(5, 1, 2, 1056, 30, 40, 44, 176), (3, 1, 3, 768, 9, 11, 32, 128),
                                             (5, 2, 2, 96, 13, 17, 4, 24), (3, 2, 16, 384, 15, 20, 16, 128)])
def test_depthwise_hl_gate_weights_project(ops, monkeypatch, cfg, k, s, B, C, H, W, R, N):
    """The late-stage MBConv tail on the pre-split route: depthwise + SiLU written ONCE in the hl32 layout, the
    squeeze-excite gate folded into per-image packed project weights (ocv_se_gate_weights_fwd), the project 1x1 on the
    LDS-DMA kernel with tiles that never span images -- against the definition (gate applied to the rows) in float64, and
    piece by piece against the fp32-row kernels."""
    x, w, b = rnd("x", (B, C, H, W), 1), rnd("w", (C, 1, k, k), 2, 0.3), rnd("b", (C,), 3, 0.2)
    w1, b1 = rnd("w1", (R, C), 4, 1 / math.sqrt(C)), rnd("b1", (R,), 5, 0.3)
    w2, b2 = rnd("w2", (C, R), 6, 1 / math.sqrt(R)), rnd("b2", (C,), 7, 0.3)
    wp, bp = rnd("wp", (N, C), 8, 1 / math.sqrt(C)), rnd("bp", (N,), 9, 0.2)
    d = F.silu(F.conv2d(_same_pad(x, k, s), w, b, stride=s, groups=C)).double()
    gref = torch.sigmoid(F.silu(d.mean((2, 3)) @ w1.double().T + b1.double()) @ w2.double().T + b2.double())
    res = rnd("r", (B, N, d.shape[2], d.shape[3]), 10)
    ref = F.conv2d(d * gref[:, :, None, None], wp.double()[:, :, None, None], bp.double()) + res
    args = (dev(x).contiguous(memory_format=torch.channels_last), dev(w).flatten(1).t().contiguous(), dev(b), k, s,
            dev(w1), dev(b1), dev(w2).t().contiguous(), dev(b2))
    y_fp32, g_fp32 = ops.depthwise_se_gate(*args)
    ys, wg, gate = ops.depthwise_se_gate_weights(*args, dev(wp), want_gate=True)
    # the split output is the split of the fp32 kernel's output, bit for bit; the gate equals the two-launch gate
    hi = y_fp32.to(torch.bfloat16)
    assert torch.equal(ys.hi.contiguous(), hi) and torch.equal(ys.lo.contiguous(), (y_fp32 - hi.float()).to(torch.bfloat16))
    assert torch.equal(gate, g_fp32) and rel_dev(gate, gref) < TOL
    # per-image packed weights = SplitWeight of W * diag(gate[b]), bit for bit
    for i in (0, B - 1):
        one = ops.SplitWeight(dev(wp) * gate[i][None, :])
        assert torch.equal(wg.packed[i * wg.img_elems: i * wg.img_elems + one.packed.numel()], one.packed)
    lib = ops._lib.load()
    try:
        assert lib.ocv_pointwise_hl_set_dispatch(*cfg) == 0
        out, outs = ops.pointwise_hl(ys, wg, dev(bp), 0, residual=dev(res).contiguous(memory_format=torch.channels_last),
                                     out_fp32=True, out_split=N % 8 == 0) if N % 8 == 0 else \
            (ops.pointwise_hl(ys, wg, dev(bp), 0, residual=dev(res).contiguous(memory_format=torch.channels_last)), None)
    finally:
        lib.ocv_pointwise_hl_set_dispatch(0, 0)
    assert rel_dev(out, ref) < SPLIT_TOL
    if outs is not None:
        assert rel_dev(outs.float(), ref) < SPLIT_TOL
    # and the round-2 route (gate multiplied into fp32 rows by the consumer) agrees to the split tolerance
    old = ops.pointwise_nhwc(y_fp32, ops.SplitWeight(dev(wp)), dev(bp), 0, gate=g_fp32,
                             residual=dev(res).contiguous(memory_format=torch.channels_last))
    assert rel_dev(out, old) < SPLIT_TOL


def test_pointwise_nhwc_split_also_writes_the_split_copy(ops):
    """ocv_pointwise_conv_nhwc_split_hl_fwd: the fp32-row kernel leaves the hl32 copy of its result for an LDS-DMA consumer.
    (Eight images: 225 tiles -- a launch of fewer than 128 tiles without the split copy takes the split-K form, another summation order.)"""
    B, H, W, Cin, Cout = 8, 15, 20, 1824, 304
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 1, 1), 2, 1 / math.sqrt(Cin)), rnd("b", (Cout,), 3, 0.2)
    g = torch.sigmoid(rnd("g", (B, Cin), 4))
    res = dev(rnd("r", (B, Cout, H, W), 5)).contiguous(memory_format=torch.channels_last)
    xg = dev(x).contiguous(memory_format=torch.channels_last)
    sw = ops.SplitWeight(dev(w))
    y0 = ops.pointwise_nhwc(xg, sw, dev(b), 0, gate=dev(g), residual=res)
    y, ys = ops.pointwise_nhwc(xg, sw, dev(b), 0, gate=dev(g), residual=res, out_split=True)
    assert torch.equal(y, y0)
    hi = y.to(torch.bfloat16)
    assert torch.equal(ys.hi.contiguous(), hi) and torch.equal(ys.lo.contiguous(), (y - hi.float()).to(torch.bfloat16))
    blk = ys.hl.view(B, H, W, -1, 2, 32)[:, :, :, Cout // 32]
    assert float(blk[..., Cout % 32:].float().abs().max()) == 0.0          # 304 = 9.5 blocks: the pad half-block is zero


@pytest.mark.parametrize("B,Cin,H,W,Cout,stride,act", [
    (2, 3, 96, 128, 48, 2, 3),       # the B5 stem shape family: SAME padding 0/1 (even sizes)
    (1, 3, 33, 47, 48, 2, 3),        # odd sizes: padding 1/1, ragged last pixel tile
    (3, 3, 17, 20, 24, 1, 0),        # stride 1, symmetric padding, <= 32 channels, no activation
    (2, 1, 9, 9, 64, 2, 1),          # single input plane, 64 channels, ReLU
    (1, 2, 5, 4, 7, 3, 2),           # stride 3, ragged channel tile, LeakyReLU
])
def test_stem_conv_same(ops, B, Cin, H, W, Cout, stride, act):
    x, w, b = rnd("x", (B, Cin, H, W), 1), rnd("w", (Cout, Cin, 3, 3), 2, 0.3), rnd("b", (Cout,), 3, 0.2)
    ref = F.conv2d(_same_pad(x, 3, stride), w, b, stride=stride)
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act]
    got = ops.stem_conv_same(dev(x), dev(w), dev(b), stride, act)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert rel_dev(got, ref) < TOL


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("B,C,H,W", [(2, 48, 60, 80), (1, 8, 15, 20), (3, 12, 33, 47), (1, 4, 1, 1), (2, 144, 30, 41)])
def test_depthwise_nhwc_same(ops, k, s, B, C, H, W):
    x, w, b = rnd("x", (B, C, H, W), 1), rnd("w", (C, 1, k, k), 2, 0.3), rnd("b", (C,), 3, 0.2)
    ref = F.silu(F.conv2d(_same_pad(x, k, s), w, b, stride=s, groups=C))
    wt = dev(w).flatten(1).t().contiguous()
    got = ops.depthwise_nhwc_same(dev(x).contiguous(memory_format=torch.channels_last), wt, dev(b), k, s, 3)
    assert got.shape == ref.shape and rel_dev(got, ref) < TOL


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("B,C,H,W,R", [(2, 48, 60, 80, 12), (1, 8, 15, 20, 2), (3, 12, 33, 47, 4), (1, 4, 1, 1, 1),
                                       (2, 144, 30, 41, 6), (2, 1056, 9, 11, 44), (1, 3072, 4, 5, 128), (16, 240, 30, 40, 10)])
def test_depthwise_se_gate(ops, k, s, B, C, H, W, R):
    x, w, b = rnd("x", (B, C, H, W), 1), rnd("w", (C, 1, k, k), 2, 0.3), rnd("b", (C,), 3, 0.2)
    w1, b1 = rnd("w1", (R, C), 4, 1 / math.sqrt(C)), rnd("b1", (R,), 5, 0.3)
    w2, b2 = rnd("w2", (C, R), 6, 1 / math.sqrt(R)), rnd("b2", (C,), 7, 0.3)
    ref = F.silu(F.conv2d(_same_pad(x, k, s), w, b, stride=s, groups=C))
    gref = torch.sigmoid(F.silu(ref.mean((2, 3)) @ w1.T + b1) @ w2.T + b2)
    args = (dev(x).contiguous(memory_format=torch.channels_last), dev(w).flatten(1).t().contiguous(), dev(b), k, s,
            dev(w1), dev(b1), dev(w2).t().contiguous(), dev(b2))
    y, g = ops.depthwise_se_gate(*args)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last) and rel_dev(y, ref) < TOL
    assert g.shape == gref.shape and rel_dev(g, gref) < TOL
    y2, g2 = ops.depthwise_se_gate(*args)
    assert torch.equal(y, y2) and torch.equal(g, g2)        # fixed-order pooling sums


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("B,H,W,Cin,mid", [(2, 17, 23, 24, 144), (1, 30, 40, 40, 240), (2, 33, 47, 64, 384), (1, 8, 32, 40, 48),
                                           (1, 3, 2, 24, 36), (3, 64, 70, 32, 100)])
def test_expand_depthwise_fused(ops, k, s, B, H, W, Cin, mid):
    """Fused expand 1x1 + depthwise (+ squeeze-excite gate) against the fp32 formulation and against the two-launch
    path: image sizes that are not multiples of the 8 x 32 / 8 x 16 tiles, channel counts that do not fill the last
    32-channel chunk, images smaller than one tile, asymmetric 'SAME' padding at stride 2."""
    R = max(1, Cin // 4)
    x = rnd("x", (B, Cin, H, W), 1)
    we, be = rnd("we", (mid, Cin), 2, 1 / math.sqrt(Cin)), rnd("be", (mid,), 3, 0.3)
    wd, bd = rnd("wd", (mid, 1, k, k), 4, 0.3), rnd("bd", (mid,), 5, 0.2)
    w1, b1 = rnd("w1", (R, mid), 6, 1 / math.sqrt(mid)), rnd("b1", (R,), 7, 0.3)
    w2, b2 = rnd("w2", (mid, R), 8, 1 / math.sqrt(R)), rnd("b2", (mid,), 9, 0.3)
    e = F.silu(F.conv2d(x.double(), we.double()[:, :, None, None], be.double())).float()
    ref = F.silu(F.conv2d(_same_pad(e, k, s), wd, bd, stride=s, groups=mid))
    gref = torch.sigmoid(F.silu(ref.mean((2, 3)) @ w1.T + b1) @ w2.T + b2)
    xg = dev(x).contiguous(memory_format=torch.channels_last)
    wsp = ops.SplitWeight(dev(we))
    se = (dev(w1), dev(b1), dev(w2).t().contiguous(), dev(b2))
    wdk = dev(wd).flatten(1).t().contiguous()
    y, g = ops.expand_depthwise_se_gate(xg, wsp, dev(be), wdk, dev(bd), k, s, *se)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert rel_dev(y, ref) < SPLIT_TOL and rel_dev(g, gref) < SPLIT_TOL
    y2, g2 = ops.depthwise_se_gate(ops.pointwise_nhwc(xg, wsp, dev(be), ops.ACT_SILU), wdk, dev(bd), k, s, *se)
    assert rel_dev(y, y2) < 1e-5 and rel_dev(g, g2) < 1e-5
    y3, g3 = ops.expand_depthwise_se_gate(xg, wsp, dev(be), wdk, dev(bd), k, s, *se)
    assert torch.equal(y, y3) and torch.equal(g, g3)        # fixed-order pooling sums


@pytest.mark.parametrize("B,C,H,W,R", [(16, 144, 120, 160, 6), (2, 48, 240, 320, 12), (3, 3072, 15, 20, 128), (1, 8, 1, 3, 2)])
def test_channel_mean_and_se_gate(ops, B, C, H, W, R):
    x = rnd("x", (B, C, H, W), 1)
    xg = dev(x).contiguous(memory_format=torch.channels_last)
    assert rel_dev(ops.channel_mean_nhwc(xg), x.mean((2, 3))) < TOL
    w1, b1 = rnd("w1", (R, C), 2, 1 / math.sqrt(C)), rnd("b1", (R,), 3, 0.3)
    w2, b2 = rnd("w2", (C, R), 4, 1 / math.sqrt(R)), rnd("b2", (C,), 5, 0.3)
    ref = torch.sigmoid(F.silu(x.mean((2, 3)) @ w1.T + b1) @ w2.T + b2)
    assert rel_dev(ops.se_gate(xg, dev(w1), dev(b1), dev(w2).t().contiguous(), dev(b2)), ref) < TOL
    # deterministic two-stage reduction
    assert torch.equal(ops.channel_mean_nhwc(xg), ops.channel_mean_nhwc(xg))


def test_conv_nhwc_does_not_depend_on_stale_memory(ops):
    """Regression: an earlier pipeline read load-destination registers before the loads had landed and only looked
    right when registers / LDS / recycled allocations happened to hold the same data.  Poison the caching allocator
    with NaN, then require the FIRST run on freshly recycled memory to be correct.
    The deterministic form of this check -- every operand and workspace between poisoned guards -- is tests/test_hip_memory_bounds.py."""
    B, H, W, C1, C2, Cout = 4, 120, 160, 256, 24, 128
    cl = torch.channels_last
    x1, x2 = dev(rnd("x1", (B, C1, H, W), 1)).contiguous(memory_format=cl), dev(rnd("x2", (B, C2, H, W), 2)).contiguous(memory_format=cl)
    w, b = dev(rnd("w", (Cout, C1 + C2, 3, 3), 3, 0.02)), dev(rnd("b", (Cout,), 4, 0.2))
    hi, lo = ops.prep_conv_weight(w)
    ref = F.leaky_relu(F.conv2d(torch.cat([x1, x2], 1), w, b, padding=1), 0.01)
    for _ in range(2):
        poison = torch.full((1 << 30,), float("nan"), device="cuda")      # 4 GiB of NaN back into the allocator
        del poison
        y = ops.conv_nhwc(x1, x2, hi, lo, b, 3, 2)
        assert bool(torch.isfinite(y).all())
        assert rel_dev(y, ref) < 1e-4


# ------------------------------------------------------------------ split activations between convolutions
@pytest.mark.parametrize("B,h,w,H,W,C1,C2", [(2, 17, 22, 30, 40, 64, 24), (1, 30, 40, 60, 80, 32, 0), (3, 5, 7, 11, 13, 8, 4),
                                             (1, 120, 160, 240, 320, 16, 8),
                                             (2, 9, 11, 17, 21, 16, 8),      # odd output size: ragged 2 x 2 blocks
                                             (1, 7, 9, 7, 9, 8, 0),          # identity resize through the 2 x 2 kernel
                                             (1, 20, 24, 11, 13, 8, 8),      # shrinking: the per-pixel octet kernel
                                             (1, 1, 1, 6, 5, 40, 16),        # one source pixel
                                             (2, 8, 10, 16, 20, 1096, 0),    # 137 octets per pixel: 192-thread blocks
                                             (2, 15, 20, 30, 40, 64, 24),    # >= 2x and C1 % 64 == 0: the LDS-tiled kernel
                                             (1, 9, 11, 19, 23, 128, 8),     # ... ragged 16 x 32 tiles, two resize chunks
                                             (1, 1, 1, 5, 7, 64, 0),         # ... one source pixel, no skip tensor
                                             (1, 40, 50, 97, 131, 64, 40)])  # ... several tiles per image, 2.4x / 2.6x
def test_upsample_concat_split(ops, B, h, w, H, W, C1, C2):
    x = rnd("x", (B, C1, h, w), 1)
    skip = rnd("s", (B, C2, H, W), 2) if C2 else None
    ref = F.interpolate(x, size=[H, W], mode="bilinear", align_corners=True)
    if skip is not None:
        ref = torch.cat([ref, skip], 1)
    got = ops.upsample_concat_split(dev(x), None if skip is None else dev(skip), (H, W))
    Cp = (C1 + C2 + 31) // 32 * 32
    assert got.hl.dtype == torch.bfloat16 and tuple(got.hl.shape) == (B, H, W, 2 * Cp) and got.hl.is_contiguous()
    assert tuple(got.shape) == (B, C1 + C2, H, W)
    blocks = got.hl.view(B, H, W, Cp // 32, 2, 32).permute(0, 1, 2, 4, 3, 5).reshape(B, H, W, 2, Cp)
    assert not bool(blocks[..., C1 + C2:].any())       # pad channels of the last 32-block are zero
    assert rel_dev(got.float(), ref) < 1e-5            # hi + lo carries 16 bits: 2^-17 relative per element
    assert rel_dev(got.hi.float(), ref) < 5e-3         # hi alone is plain bf16


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,act", [(2, 30, 40, 88, 128, 3, 2), (1, 17, 23, 32, 40, 3, 0), (1, 60, 80, 256, 256, 3, 2),
                                                  (2, 9, 11, 96, 200, 1, 3)])
def test_conv_nhwc_split_in_and_out(ops, B, H, W, Cin, Cout, k, act):
    x = rnd("x", (B, Cin, H, W), 1)
    w, b = rnd("w", (Cout, Cin, k, k), 3, 1 / math.sqrt(Cin * k * k)), rnd("b", (Cout,), 4, 0.2)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=k // 2).float()
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act]
    hi, lo = ops.prep_conv_weight(dev(w))
    xs = ops.upsample_concat_split(dev(x), None, (H, W))          # identity resize = plain split
    y, ys = ops.conv_nhwc_split(xs, hi, lo, dev(b), k, act, out_fp32=True, out_split=True)
    assert rel_dev(y, ref) < SPLIT_TOL
    assert rel_dev(ys.float(), y) < 1e-5
    y2 = ops.conv_nhwc_split(xs, hi, lo, dev(b), k, act, out_fp32=True, out_split=False)
    assert torch.equal(y, y2)
    if Cout % 32:
        # pad channels of the last 32-block read as zero (ocv_zero_async: a launch, so that the same holds in a graph replay)
        Cp = (Cout + 31) // 32 * 32
        pads = lambda t: t.hl.view(B, H, W, Cp // 32, 2, 32).permute(0, 1, 2, 4, 3, 5).reshape(B, H, W, 2, Cp)[..., Cout:]
        assert not bool(pads(ys).any())
        torch.cuda.synchronize()
        g, st, bg = torch.cuda.CUDAGraph(), torch.cuda.Stream(), dev(b)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            poison = torch.full_like(ys.hl, 7.0)                 # the replay's output lands where this was: pads start dirty
            del poison
            with torch.cuda.graph(g, stream=st):
                _, ys_g = ops.conv_nhwc_split(xs, hi, lo, bg, k, act, out_fp32=True, out_split=True)
        ys_g.hl.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ys_g.hl, ys.hl)
    # and it agrees with the fp32-input kernel to rounding
    y3 = ops.conv_nhwc(dev(x), None, hi, lo, dev(b), k, act)
    assert rel_dev(y, y3) < 1e-5


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("k", [1, 3])
def test_conv_nhwc_split_ragged_tile_elementwise_split_out(ops, k, f16):
    """The tap ring's element-wise epilogue (Cout % 8 != 0; conv_store_elems, csrc/conv_tile.hpp) on a ragged last tile
    (M = 297 = 256 + 41 rows) with everything it can do at once: per-channel scale, bias, LeakyReLU, residual, the fp32 and
    the split output.  Against float64 on the operands the kernel read (x = hi + lo of the split input) at the decoder's
    bars; the split copy is the pair of the fp32 result, its pad channels zero, and rows past M are not written."""
    from decoder_shadow import BF16_TOL, F16_TOL
    B, H, W, Cin, Cout = 1, 9, 33, 40, 12
    lib = ops._lib.load()
    x32 = dev(rnd("x", (B, Cin, H, W), 21)).contiguous(memory_format=torch.channels_last)
    w32 = rnd("w", (Cout, Cin, k, k), 22, 1 / math.sqrt(Cin * k * k))
    bias, res = dev(rnd("b", (Cout,), 23, 0.3)), dev(rnd("r", (B, H, W, Cout), 24))
    xs = ops.split_act(x32, f16=f16)
    w_hi, w_lo, osc = (ops.prep_conv_weight(dev(w32), f16=f16) + (None,))[:3]
    M = B * H * W
    ybuf = torch.full((M + 256, Cout), float("nan"), device="cuda")          # room for a whole second tile behind the result
    ys = ops.SplitAct.empty(B, Cout, H, W, "cuda", f16=f16)
    ys.hl.view(torch.int16).fill_(0x7E7E)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    rc = lib.ocv_conv_nhwc_split_x_fwd(xs.hl.data_ptr(), Cin, w_hi.data_ptr(), w_lo.data_ptr(), p(osc), int(f16), p(bias), p(res),
                                       ybuf.data_ptr(), ys.hl.data_ptr(), B, H, W, Cout, k, ops.ACT_LEAKY_RELU, None, 0,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ocv_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    assert torch.isnan(ybuf[M:]).all()                                       # the ragged tile's 215 missing rows
    y = ybuf[:M].view(B, H, W, Cout).permute(0, 3, 1, 2)
    hi, lo = xs.parts()
    ref = F.leaky_relu(F.conv2d(hi.double().cpu() + lo.double().cpu(), w32.double(), bias.double().cpu(), padding=k // 2), 0.01)
    ref = ref + res.double().cpu().permute(0, 3, 1, 2)
    err, bar = rel_dev(y.cpu().double(), ref), F16_TOL if f16 else BF16_TOL
    print(f"ragged element-wise split-out k={k} {'fp16' if f16 else 'bf16'} pairs: {err:.3g} (bar {bar:.1e})")
    assert err < bar
    assert rel_dev(ys.float(), y) < (1e-6 if f16 else 1e-5)                  # a 22- / 16-bit pair of the fp32 result
    pads = ys.hl.view(B, H, W, 1, 2, 32)[..., Cout:]
    assert not bool(pads.view(torch.int16).any())


@pytest.mark.parametrize("B,H,W,Cin,Cout,act", [
    (2, 30, 40, 96, 64, 2),        # H not a multiple of 4 (last tile row half outside), LeakyReLU
    (1, 7, 9, 40, 72, 0),          # odd H and W, Cin % 32 != 0, Cout % 32 != 0
    (3, 1, 1, 32, 8, 1),           # a single pixel: every tap but the centre is padding
    (1, 4, 4, 8, 16, 3),           # one tile, SiLU
    (1, 16, 20, 1024, 512, 2),     # long K: 32 channel chunks per position
    (2, 13, 16, 300, 136, 2),      # ragged everything
    (16, 30, 40, 1024, 1024, 2),   # the decoder's 30 x 40 stage at full size (1280 tiles per position, 36 GEMMs of K = 1024)
])
def test_conv3x3_winograd43_split(ops, B, H, W, Cin, Cout, act):
    """ocv_conv3x3_winograd43_split_fwd (F(4x4, 3x3): input transform, 36 batched two-term-fp16 GEMMs on filters scaled out of
    fp16's subnormals, output transform) against an fp64 convolution at the SAME bar as the direct kernel (2e-5 of max |y|),
    and against the direct kernel itself.
    The deterministic form of this check -- every operand and workspace between poisoned guards -- is tests/test_hip_memory_bounds.py."""
    x = rnd("x", (B, Cin, H, W), 1)
    w, b = rnd("w", (Cout, Cin, 3, 3), 3, 1 / math.sqrt(Cin * 9)), rnd("b", (Cout,), 4, 0.2)
    if B * H * W * Cout > 4e6:                                  # the full-size case: reference on the GPU in fp64
        ref = F.conv2d(dev(x).double(), dev(w).double(), dev(b).double(), padding=1).cpu()
    else:
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act]
    u_hi, u_lo, fs, cs = ops.prep_winograd43_weight(dev(w))
    assert tuple(u_hi.shape) == (36, Cout, (Cin + 31) // 32 * 32) and u_hi.dtype == torch.float16 and fs.numel() == 36
    assert cs.numel() == (Cin + 31) // 32 * 32 and bool((torch.log2(cs) == torch.round(torch.log2(cs))).all())     # powers of two
    assert float(u_hi.float().abs().amax()) < 1024.0 and bool(torch.isfinite(u_lo.float()).all())
    xs = ops.upsample_concat_split(dev(x), None, (H, W))
    poison = [torch.full((1 << 22,), float("nan"), device="cuda") for _ in range(8)]
    del poison                                                  # workspace and outputs come out of NaN-filled memory
    y, ys = ops.conv3x3_winograd43_split(xs, u_hi, u_lo, fs, dev(b), act, out_fp32=True, out_split=True, cscale=cs)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert rel_dev(y, ref) < SPLIT_TOL
    assert rel_dev(ys.float(), y) < 1e-5
    Cpo = (Cout + 31) // 32 * 32
    blocks = ys.hl.view(B, H, W, Cpo // 32, 2, 32).permute(0, 1, 2, 4, 3, 5).reshape(B, H, W, 2, Cpo)
    assert not bool(blocks[..., Cout:].any())                  # pad channels of the split output are zero
    y2 = ops.conv3x3_winograd43_split(xs, u_hi, u_lo, fs, dev(b), act, out_fp32=True, out_split=False, cscale=cs)
    assert torch.equal(y, y2)
    hi, lo = ops.prep_conv_weight(dev(w))
    direct = ops.conv_nhwc_split(xs, hi, lo, dev(b), 3, act)
    assert rel_dev(y, direct) < SPLIT_TOL


def test_conv3x3_winograd43_random_shapes(ops):
    """Seeded sweep of the F(4x4, 3x3) form over ragged shapes (1..3 images, 1..23 rows / columns, 4..132 input channels, 8..200
    output channels, every activation) against an fp64 convolution."""
    import random
    rng = random.Random(4343)
    for case in range(16):
        B, H, W = rng.randint(1, 3), rng.randint(1, 23), rng.randint(1, 23)
        Cin, Cout, act = rng.choice([4, 8, 12, 28, 32, 36, 64, 132]), 8 * rng.randint(1, 25), rng.randint(0, 3)     # (the splitter takes channel quads)
        x = rnd("x", (B, Cin, H, W), 500 + case)
        w, b = rnd("w", (Cout, Cin, 3, 3), 600 + case, 1 / math.sqrt(Cin * 9)), rnd("b", (Cout,), 700 + case, 0.2)
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
        ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act]
        u_hi, u_lo, fs, cs = ops.prep_winograd43_weight(dev(w))
        xs = ops.upsample_concat_split(dev(x), None, (H, W))
        y = ops.conv3x3_winograd43_split(xs, u_hi, u_lo, fs, dev(b), act, cscale=cs)
        assert rel_dev(y, ref) < SPLIT_TOL, (case, B, H, W, Cin, Cout, act)


@pytest.mark.parametrize("Cin", [64, 1024, 1056])     # tiles sharing a workgroup / one tile per workgroup / the two-round path (Cp > 1024)
def test_conv3x3_winograd43_keeps_fp32_range(ops, Cin):
    """the F(4x4, 3x3) form's transformed input is up to 49x the activation with an UNSCALED fp16 low term.  Its input
    transform now scales every tile by a power of two from the tile's own largest input and every channel by a static power of two
    from the filters' columns, so the result keeps SPLIT_TOL at every magnitude fp32 activations take -- x * 1e-4 (was 3e-4 of
    max |y|: low terms in fp16's subnormals), x * 1e3, x * 1e6 (was NaN: overflow from ~1.3e3 on), per-channel scales spanning
    2^-10 ... 2^10 against inverse weights (was 3e-4), tiles of very different magnitude side by side -- and that an inf / NaN
    activation comes out non-finite (loud), never clipped."""
    B, H, W, Cout = 2, 12, 13, 32
    x0 = rnd("x", (B, Cin, H, W), 11)
    w0 = rnd("w", (Cout, Cin, 3, 3), 12, 1 / math.sqrt(Cin * 9))
    span = torch.logspace(-3, 3, Cin).view(1, Cin, 1, 1)
    ramp = torch.logspace(-4, 4, W).view(1, 1, 1, W)                       # neighbouring tiles differ by orders of magnitude
    cases = [("unit", x0, w0), ("x 1e-4", x0 * 1e-4, w0), ("x 1e3", x0 * 1e3, w0), ("x 1e6", x0 * 1e6, w0),
             ("per-channel 1e-3 .. 1e3 against inverse weights", x0 * span, w0 / span), ("per-channel activations only", x0 * span, w0),
             ("column ramp 1e-4 .. 1e4", x0 * ramp, w0)]
    for name, x, w in cases:
        ref = F.conv2d(x.double(), w.double(), padding=1)
        u_hi, u_lo, fs, cs = ops.prep_winograd43_weight(dev(w))
        assert bool(torch.isfinite(u_hi.float()).all()) and float(u_hi.float().abs().amax()) < 1024.0
        xs = ops.upsample_concat_split(dev(x), None, (H, W))
        y = ops.conv3x3_winograd43_split(xs, u_hi, u_lo, fs, None, 0, cscale=cs)
        assert bool(torch.isfinite(y).all()), name
        if name.startswith("column ramp"):                                  # error relative to each column's own magnitude
            err = ((y.cpu().double() - ref).abs().amax(dim=(0, 1, 2)) / ref.abs().amax(dim=(0, 1, 2))).max()
            assert float(err) < 4 * SPLIT_TOL, (name, float(err))         # a tile holds four columns: 10x steps inside it
        else:
            assert rel_dev(y, ref) < SPLIT_TOL, (name, rel_dev(y, ref))
    for bad in (float("inf"), float("nan")):
        x = x0.clone()
        x[0, 3, 5, 6] = bad
        u_hi, u_lo, fs, cs = ops.prep_winograd43_weight(dev(w0))
        y = ops.conv3x3_winograd43_split(ops.upsample_concat_split(dev(x), None, (H, W)), u_hi, u_lo, fs, None, 0, cscale=cs)
        assert not bool(torch.isfinite(y[0, :, 4:7, 5:8]).all())           # loud where the bad value enters
        assert bool(torch.isfinite(y[1]).all())                            # and nowhere else: the other image is untouched


def test_winograd_dispatch_policy(ops):
    """hip_ops.winograd_pays: F(4x4, 3x3) takes the decoder's 30 x 40 and 60 x 80 second convolutions, nothing shallower or larger."""
    assert ops.winograd_pays(16, 30, 40, 2224, 1024) and ops.winograd_pays(16, 30, 40, 1024, 1024)
    assert ops.winograd_pays(16, 60, 80, 512, 512) and not ops.winograd_pays(16, 120, 160, 256, 256)
    assert not ops.winograd_pays(16, 240, 320, 280, 128) and not ops.winograd_pays(16, 30, 40, 1024, 36)


@pytest.mark.parametrize("B,H,W,C1,C2,Cout,k,act", [
    (2, 13, 17, 40, 0, 72, 3, 2),        # ragged rows / channels
    (1, 9, 11, 128, 3, 128, 3, 2),       # the final_upscale stage's 131 input channels (virtual concat with the image)
    (1, 7, 5, 5, 0, 3, 5, 0),            # 5 x 5, tiny odd channel counts
    (2, 6, 6, 32, 16, 33, 1, 3),         # 1 x 1, concat, SiLU
    (1, 30, 40, 256, 0, 128, 3, 1),      # several K chunks, ReLU
])
def test_conv_nhwc_exact(ops, B, H, W, C1, C2, Cout, k, act):
    """ocv_conv_nhwc_exact_fwd: the hand-written exact-fp32 implicit GEMM (OCV_CONV=exact and shapes the split-bf16
    kernels do not take) against an fp64 convolution, at fp32 accumulation-order noise."""
    x1 = rnd("x1", (B, C1, H, W), 1)
    x2 = rnd("x2", (B, C2, H, W), 2) if C2 else None
    w, b = rnd("w", (Cout, C1 + C2, k, k), 3, 1 / math.sqrt((C1 + C2) * k * k)), rnd("b", (Cout,), 4, 0.2)
    res = rnd("r", (B, Cout, H, W), 5)
    xin = x1 if x2 is None else torch.cat([x1, x2], 1)
    ref = F.conv2d(xin.double(), w.double(), b.double(), padding=k // 2)
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act] + res
    wt = dev(w).permute(2, 3, 0, 1).reshape(k * k, Cout, C1 + C2).contiguous()
    cl = torch.channels_last
    got = ops.conv_nhwc_exact(dev(x1).contiguous(memory_format=cl), None if x2 is None else dev(x2).contiguous(memory_format=cl),
                              wt, dev(b), k, act, residual=dev(res).contiguous(memory_format=cl))
    assert got.is_contiguous(memory_format=cl) and rel_dev(got, ref) < 2e-6


@pytest.mark.parametrize("B,h,w,H,W,Cout,act", [(2, 15, 20, 30, 40, 64, 2), (1, 17, 22, 30, 40, 72, 0), (1, 5, 7, 11, 13, 8, 3),
                                                (3, 30, 40, 60, 80, 32, 2), (1, 2, 3, 9, 23, 40, 1),
                                                (1, 13, 40, 22, 76, 64, 2), (2, 11, 38, 22, 76, 32, 2),      # KITTI's first stages
                                                (1, 4, 5, 13, 17, 36, 0), (1, 1, 1, 8, 16, 32, 2)])           # > 3x, a single source pixel
def test_tap_interp_combine(ops, B, h, w, H, W, Cout, act):
    """ocv_tap_interp_combine_fwd against its definition in fp64: nine bilinear (align_corners) up-samplings of the tap
    products, each shifted by its tap with zero padding, + skip part + bias, activation; fp32 and split outputs."""
    z = rnd("z", (B, 9 * Cout, h, w), 1)
    s, b = rnd("s", (B, Cout, H, W), 2), rnd("b", (Cout,), 3, 0.3)
    ref = s.double() + b.double().view(1, -1, 1, 1)
    for t in range(9):
        up = F.interpolate(z[:, t * Cout:(t + 1) * Cout].double(), size=(H, W), mode="bilinear", align_corners=True)
        dy, dx = t // 3 - 1, t % 3 - 1
        ref = ref + F.pad(up, (1, 1, 1, 1))[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act]
    cl = torch.channels_last
    assert ops.tap_interp_supported(h, w, H, W, Cout)
    y, ys = ops.tap_interp_combine(dev(z).contiguous(memory_format=cl), dev(s).contiguous(memory_format=cl), dev(b), (H, W), act,
                                   out_fp32=True, out_split=True)
    assert y.is_contiguous(memory_format=cl) and rel_dev(y, ref) < TOL
    assert rel_dev(ys.float(), y) < 1e-5
    y2 = ops.tap_interp_combine(dev(z).contiguous(memory_format=cl), None, None, (H, W), 0)
    ref2 = sum(F.pad(F.interpolate(z[:, t * Cout:(t + 1) * Cout].double(), size=(H, W), mode="bilinear", align_corners=True),
                     (1, 1, 1, 1))[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9))
    assert rel_dev(y2, ref2) < TOL
    assert not ops.tap_interp_supported(64, 64, 32, 32, Cout)          # a down-scaling: the footprint does not fit


@pytest.mark.parametrize("B,h,w,H,W,Cout,act", [(2, 15, 20, 30, 40, 64, 2), (1, 3, 4, 11, 13, 8, 0), (1, 1, 1, 7, 9, 40, 2),
                                                (2, 6, 9, 17, 23, 96, 1)])
def test_tap_interp_combine_bordered_grid(ops, B, h, w, H, W, Cout, act):
    """zpad = 1: z stores the h x w interior of an (h+2) x (w+2) resize source whose border ring holds one constant vector
    (Decoder.conv2's padding=1 on a 1x1 convolution): equals the plain form on the materialised grid, bit for bit."""
    cl = torch.channels_last
    z = dev(rnd("z", (B, 9 * Cout, h, w), 1)).contiguous(memory_format=cl)
    border = dev(rnd("c", (9 * Cout,), 2))
    s, b = dev(rnd("s", (B, Cout, H, W), 3)).contiguous(memory_format=cl), dev(rnd("b", (Cout,), 4, 0.3))
    full = border.view(1, -1, 1, 1).expand(B, 9 * Cout, h + 2, w + 2).contiguous(memory_format=cl).clone()
    full[:, :, 1:-1, 1:-1] = z
    want = ops.tap_interp_combine(full.contiguous(memory_format=cl), s, b, (H, W), act)
    got, gs = ops.tap_interp_combine(z, s, b, (H, W), act, out_fp32=True, out_split=True, border=border)
    assert torch.equal(got, want)
    assert rel_dev(gs.float(), got) < 1e-5
    with pytest.raises(ValueError):
        ops.tap_interp_combine(z, s, b, (H, W), act, border=border[:-1])


@pytest.mark.parametrize("B,h,w,H,W,C1,C2,Cout", [(2, 15, 20, 30, 40, 64, 24, 64), (1, 17, 22, 30, 40, 96, 16, 72),
                                                  (1, 30, 40, 60, 80, 128, 0, 32), (2, 8, 9, 16, 19, 32, 40, 128)])
def test_upsampled_conv_at_low_resolution(ops, B, h, w, H, W, C1, C2, Cout):
    """The whole first convolution of an UpSampleWithSkip stage in its low-resolution form -- 1x1 GEMM with the nine taps
    stacked, 3x3 convolution over the skip channels, tap interpolation + bias + LeakyReLU -- against the reference's
    literal form in fp64: conv3x3(cat(interpolate(x), skip)), at the direct split-bf16 kernel's bar."""
    x = rnd("x", (B, C1, h, w), 1)
    skip = rnd("k", (B, C2, H, W), 2) if C2 else None
    wt, b = rnd("w", (Cout, C1 + C2, 3, 3), 3, 1 / math.sqrt((C1 + C2) * 9)), rnd("b", (Cout,), 4, 0.2)
    up = F.interpolate(x.double(), size=(H, W), mode="bilinear", align_corners=True)
    cat = up if skip is None else torch.cat([up, skip.double()], 1)
    ref = F.leaky_relu(F.conv2d(cat, wt.double(), b.double(), padding=1), 0.01)
    cl = torch.channels_last
    wa = dev(wt)[:, :C1].permute(2, 3, 0, 1).reshape(9 * Cout, C1, 1, 1)
    a_hi, a_lo = ops.prep_conv_weight(wa)
    z = ops.conv_nhwc_split(ops.split_act(dev(x).contiguous(memory_format=cl)), a_hi, a_lo, None, 1, 0)
    s = None
    if skip is not None:
        s_hi, s_lo = ops.prep_conv_weight(dev(wt)[:, C1:].contiguous())
        s = ops.conv_nhwc_split(ops.split_act(dev(skip).contiguous(memory_format=cl)), s_hi, s_lo, None, 3, 0)
    y = ops.tap_interp_combine(z, s, dev(b), (H, W), 2)
    assert rel_dev(y, ref) < SPLIT_TOL
    # and it agrees with the direct path (resize + concat + split, then the 3x3 kernel) to the same bar
    hi, lo = ops.prep_conv_weight(dev(wt))
    direct = ops.conv_nhwc_split(ops.upsample_concat_split(dev(x).contiguous(memory_format=cl),
                                                           None if skip is None else dev(skip).contiguous(memory_format=cl), (H, W)),
                                 hi, lo, dev(b), 3, 2)
    assert rel_dev(y, direct) < SPLIT_TOL


@pytest.mark.parametrize("out_fp32,out_split", [(True, False), (False, True), (True, True)])
def test_conv_nhwc_split_k_halves(ops, out_fp32, out_split):
    """300 tiles on 256 CUs: the launcher halves the channel chunks between two workgroups per tile (fp32 partial
    sums in a workspace) and a finish pass adds them, applies bias + LeakyReLU and writes fp32 and / or split output.
    Checked against the fp32-input kernel (no split-K) and torch's convolution on the GPU."""
    B, H, W, Cin, Cout, k, act = 4, 60, 80, 464, 512, 3, 2
    from objcavit_amd import _lib
    assert _lib.load().ocv_conv_nhwc_split_workspace_bytes(B, H, W, Cin, Cout, k) == 2 * B * H * W * Cout * 4
    assert _lib.load().ocv_conv_nhwc_split_workspace_bytes(16, 60, 80, 1088, 512, 3) == 0       # 1200 tiles: no split
    x = dev(rnd("x", (B, Cin, H, W), 1)).contiguous(memory_format=torch.channels_last)
    w, b = dev(rnd("w", (Cout, Cin, k, k), 3, 1 / math.sqrt(Cin * k * k))), dev(rnd("b", (Cout,), 4, 0.2))
    hi, lo = ops.prep_conv_weight(w)
    xs = ops.upsample_concat_split(x, None, (H, W))
    got = ops.conv_nhwc_split(xs, hi, lo, b, k, act, out_fp32=out_fp32, out_split=out_split)
    outs = got if isinstance(got, tuple) else (got,)
    y3 = ops.conv_nhwc(x, None, hi, lo, b, k, act)                      # fp32-input kernel, one workgroup per tile
    ref = F.leaky_relu(F.conv2d(x, w, b, padding=1), 0.01)
    for o in outs:
        v = o.float() if isinstance(o, ops.SplitAct) else o
        assert rel_dev(v, y3) < 1e-5 and rel_dev(v, ref) < 2e-4
    again = ops.conv_nhwc_split(xs, hi, lo, b, k, act, out_fp32=out_fp32, out_split=out_split)
    a0 = again[0] if isinstance(again, tuple) else again
    g0 = outs[0]
    assert torch.equal(a0.hl if isinstance(a0, ops.SplitAct) else a0, g0.hl if isinstance(g0, ops.SplitAct) else g0)


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,act", [
    (3, 150, 154, 40, 96, 3, 2),        # 271 row tiles x 1: more tiles than CUs, ragged rows
    (3, 150, 154, 32, 136, 3, 0),       # 542 tiles, two channel tiles (second ragged), tile count not a multiple of 8
    (2, 240, 320, 24, 16, 3, 2),        # 600 tiles, Cout % 8 == 0 but < one tile; one K chunk only (9 steps)
    (1, 300, 301, 8, 12, 1, 0),         # 353 tiles, 1x1 (ONE K step per tile), Cout % 8 != 0: element-wise epilogue
])
def test_conv_nhwc_split_many_tiles(ops, B, H, W, Cin, Cout, k, act):
    """More output tiles than CUs (several rounds of workgroups, tile counts that are not multiples of 8 for the XCD
    map, single-K-step tiles, ragged rows / channels) against an fp64 convolution and the fp32-input kernel."""
    x = rnd("x", (B, Cin, H, W), 1)
    w, b = rnd("w", (Cout, Cin, k, k), 3, 1 / math.sqrt(Cin * k * k)), rnd("b", (Cout,), 4, 0.2)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=k // 2).float()
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act]
    hi, lo = ops.prep_conv_weight(dev(w))
    xs = ops.upsample_concat_split(dev(x), None, (H, W))
    y, ys = ops.conv_nhwc_split(xs, hi, lo, dev(b), k, act, out_fp32=True, out_split=True)
    assert rel_dev(y, ref) < SPLIT_TOL
    assert rel_dev(ys.float(), y) < 1e-5
    assert torch.equal(y, ops.conv_nhwc_split(xs, hi, lo, dev(b), k, act, out_fp32=True, out_split=False))
    y3 = ops.conv_nhwc(dev(x), None, hi, lo, dev(b), k, act)        # fp32-input kernel
    assert rel_dev(y, y3) < 1e-5


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("B,H,W,Cin,Cout,act", [
    (2, 30, 40, 24, 128, 0),           # 27 granules = 7 K steps (the last one: 3 real granules + 1 of padding); a skip part's shape
    (1, 61, 83, 40, 256, 2),           # 45 granules = 12 steps, granules of one step from two taps; ragged rows, two channel tiles
    (3, 9, 11, 8, 40, 3),              # one granule per tap: a step holds FOUR taps; Cout % 32 != 0 with a split copy
    (1, 17, 23, 176, 72, 1),           # 22 granules per tap (198 -> 50 steps): granule index / 22 up to 199
    (2, 1, 1, 16, 16, 0),              # a single pixel: every tap but the centre is padding
])
def test_conv3x3_packed_taps(ops, f16, B, H, W, Cin, Cout, act):
    """Round 6: ocv_conv3x3_split_packed_taps_fwd -- the 3x3 implicit GEMM with the nine taps' real 8-channel granules laid end to end
    along K (no zero pad channels per tap) -- against an fp64 convolution at the tap-major kernel's bar and against the tap-major
    kernel itself (same products, another summation order)."""
    x = rnd("x", (B, Cin, H, W), 1)
    w, b = rnd("w", (Cout, Cin, 3, 3), 3, 1 / math.sqrt(Cin * 9)), rnd("b", (Cout,), 4, 0.2)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).float()
    ref = [ref, torch.relu(ref), F.leaky_relu(ref, 0.01), F.silu(ref)][act]
    xs = ops.upsample_concat_split(dev(x), None, (H, W), f16=f16)
    prep = ops.prep_conv_weight_packed_taps(dev(w), f16=f16)
    hi, lo, osc = (prep + (None,))[:3]
    Kp = (9 * (Cin // 8) + 3) // 4 * 32
    assert tuple(hi.shape) == (1, Cout, Kp) and ops._lib.load().ocv_conv3x3_packed_taps_k(Cin) == Kp
    y, ys = ops.conv3x3_split_packed_taps(xs, hi, lo, dev(b), act, out_fp32=True, out_split=True, oscale=osc)
    assert rel_dev(y, ref) < SPLIT_TOL
    assert rel_dev(ys.float(), y) < (1e-6 if f16 else 1e-5)
    d = ops.prep_conv_weight(dev(w), f16=f16)
    yd = ops.conv_nhwc_split(xs, d[0], d[1], dev(b), 3, act, out_fp32=True, oscale=(d + (None,))[2])
    assert rel_dev(y, yd) < 2e-6
    assert torch.equal(y, ops.conv3x3_split_packed_taps(xs, hi, lo, dev(b), act, out_fp32=True, oscale=osc))      # deterministic
    if Cout % 32:
        Cp = (Cout + 31) // 32 * 32
        pads = ys.hl.view(B, H, W, Cp // 32, 2, 32).permute(0, 1, 2, 4, 3, 5).reshape(B, H, W, 2, Cp)[..., Cout:]
        assert not bool(pads.any())
    with pytest.raises(ValueError):
        ops.conv3x3_split_packed_taps(xs, d[0], d[1], dev(b), act)                      # tap-major weights are not packed-tap weights
    assert ops.packed_taps_pay(24) and ops.packed_taps_pay(40) and not ops.packed_taps_pay(64) and not ops.packed_taps_pay(176)
    assert not ops.packed_taps_pay(128) and not ops.packed_taps_pay(12)


# ------------------------------------------------------------------ positional-embedding samplers
def test_pos_grid_sample_roi_vs_hand_computed_boxes(ops):
    """ocv_pos_grid_sample_fwd, RoI mode, against the hand-computed boxes of tests/roi_cases.py (box inside one cell,
    spanning cells, clipped at 0, beyond the grid, adaptive counts; no extent -> NaN) -- independent of the oracle."""
    import roi_cases as rc
    table = dev(rc.grid_table())
    boxes = dev(torch.tensor([c[1] for c in rc.CASES]))
    want = torch.tensor([c[2] for c in rc.CASES], dtype=torch.float64)
    got = ops.pos_grid_sample(table, rc.GH, rc.GW, boxes, ops.POS_ROI, rc.SCALE)
    assert float((got.cpu().double() - want).abs().max()) < 1e-6, (got, want)
    nan = ops.pos_grid_sample(table, rc.GH, rc.GW, dev(torch.tensor(rc.NAN_BOXES)), ops.POS_ROI, rc.SCALE)
    assert bool(torch.isnan(nan).all())
    # huge and non-finite boxes terminate (bounded sample window) and give finite values / NaN
    wild = dev(torch.tensor([[64.0, 48.0, 3e6, 3e6], [64.0, 48.0, 1e30, 16.0], [float("nan"), 48.0, 16.0, 16.0],
                             [64.0, 48.0, float("inf"), 16.0]]))
    w = ops.pos_grid_sample(table, rc.GH, rc.GW, wild, ops.POS_ROI, rc.SCALE).cpu()
    ind = rc.vectorised_expected(rc.grid_table().numpy(), rc.GH, rc.GW, wild[:1].cpu().numpy(), rc.SCALE)[0]   # ~46877^2 samples
    assert bool(torch.isfinite(w[0]).all()) and float(np.abs(w[0].double().numpy() / ind - 1).max()) < 1e-3
    assert bool(torch.isnan(w[1:]).all())


@pytest.mark.parametrize("gh,gw,E", [(15, 20, 128), (11, 38, 128), (3, 5, 40), (2, 1, 7)])
def test_pos_grid_sample_vs_oracle(ops, gh, gw, E):
    """All four (mode, coordinate space) combinations of GridRandomPositionalEmbeddings.forward against the oracle's
    literal restatement (grid_sample pinned by torch and the G3 fixture; ps_roi_align by tests/roi_cases.py), plus
    the fused addend and a column-slice (strided) coordinate operand."""
    import roi_cases as rc
    fh, fw, patch, seed = gh * 16, gw * 16, 16, 11 * gh + gw
    table = gen.uniform("tab", (gh * gw + 3, E), seed)                      # table longer than the grid (:81)
    H, W = 2 * fh, 2 * fw
    n = 50
    rs = np.random.RandomState(seed)
    xywh = torch.from_numpy(np.stack([rs.uniform(-0.2 * W, 1.3 * W, n), rs.uniform(-0.2 * H, 1.3 * H, n),
                                      rs.uniform(0.5, 1.5 * W, n), rs.uniform(0.5, 1.5 * H, n)], 1).astype(np.float32))
    xywh[0] = -1.0                                                          # the reference's "no detections" box (:313)
    add = rnd("add", (n, E), seed)
    # objects, centre
    ref = restate.grid_random_pos_emb(table, xywh[:, 0:2], (fh, fw), patch, "centre", "obj")
    got = ops.pos_grid_sample(dev(table), gh, gw, dev(xywh)[:, 0:2], ops.POS_CENTRE_OBJ, fh * 2.0, fw * 2.0)
    assert float((got.cpu() - ref).abs().max()) < 1e-5
    got = ops.pos_grid_sample(dev(table), gh, gw, dev(xywh), ops.POS_CENTRE_OBJ, fh * 2.0, fw * 2.0, addend=dev(add))
    assert float((got.cpu() - (ref + add)).abs().max()) < 1e-5
    # objects, roi_align (box 0 has no extent: NaN on both sides)
    ref = restate.grid_random_pos_emb(table, xywh, (fh, fw), patch, "roi_align", "obj")
    got = ops.pos_grid_sample(dev(table), gh, gw, dev(xywh), ops.POS_ROI, 1.0 / 32.0).cpu()
    assert bool(torch.isnan(ref[0]).all()) and bool(torch.isnan(got[0]).all())
    assert torch.equal(torch.isnan(got), torch.isnan(ref))                  # boxes entirely left of / above the image too
    assert float((got.nan_to_num(-7.0) - ref.nan_to_num(-7.0)).abs().max()) < 1e-5
    ind = torch.from_numpy(rc.vectorised_expected(table.numpy(), gh, gw, xywh.numpy(), 1 / 32))
    assert torch.equal(torch.isnan(ind), torch.isnan(got))
    assert float((got.double().nan_to_num(-7.0) - ind.nan_to_num(-7.0)).abs().max()) < 1e-5
    # image tokens (patch centres / sizes in feature-map pixels), both modes, B = 2
    pc = restate.patch_coords(2, gh, gw, patch)
    S = gh * gw
    ref = restate.grid_random_pos_emb(table, pc[..., 0:2], (fh, fw), patch, "centre", "img")
    got = ops.pos_grid_sample(dev(table), gh, gw, dev(pc).reshape(2 * S, 4), ops.POS_CENTRE_IMG, gh, gw, rows_per_image=S)
    assert float((got.cpu().view(2, S, E) - ref).abs().max()) < 1e-5
    ref = restate.grid_random_pos_emb(table, pc, (fh, fw), patch, "roi_align", "img")
    got = ops.pos_grid_sample(dev(table), gh, gw, dev(pc).reshape(2 * S, 4), ops.POS_ROI, 1.0 / patch)
    assert float((got.cpu().view(2, S, E) - ref).abs().max()) < 1e-5


def test_pos_grid_sample_rejects_bad_operands(ops):
    t = dev(torch.zeros(12, 8))
    with pytest.raises(ValueError):
        ops.pos_grid_sample(t, 4, 4, dev(torch.zeros(3, 4)), ops.POS_ROI, 1.0)          # grid larger than the table
    with pytest.raises(ValueError):
        ops.pos_grid_sample(t, 3, 4, dev(torch.zeros(3, 2)), ops.POS_ROI, 1.0)          # boxes need 4 columns
    with pytest.raises(Exception):
        ops.pos_grid_sample(t, 3, 4, torch.zeros(3, 4), ops.POS_ROI, 1.0)               # CPU tensor
    assert tuple(ops.pos_grid_sample(t, 3, 4, dev(torch.zeros(0, 4)), ops.POS_ROI, 1.0).shape) == (0, 8)
