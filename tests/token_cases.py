"""The seeded weights and inputs of the token-unit tests, shared by the host test (which supports the bars on exactly these
inputs) and the GPU test (which applies them): tests/test_token_units_host.py, tests/test_hip_token_units.py."""
import math

import torch
import torch.nn as nn

import gen

ENC_SEED = 11


def encoder(seed=ENC_SEED):
    """The four-layer stack of the product (E = 128, H = 4, FF = 1024) with seeded weights, peaky attention."""
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(128, 4, 1024, batch_first=True), 4, enable_nested_tensor=False).eval()
    gen.load_into(enc, seed, gen.PEAKY)
    return enc


def layer_module(enc, l, FF=1024):
    """Layer ``l`` of ``enc``; FF != 1024: the same layer with a feed-forward block of FF hidden units, linear1 / linear2 from
    gen.randn at scales 1 / sqrt(128) and 1 / sqrt(FF) (linear2.bias is the layer's own)."""
    if FF == 1024:
        return enc.layers[l]
    lay = nn.TransformerEncoderLayer(128, 4, FF, batch_first=True).eval()
    sd = {k: v.clone() for k, v in enc.layers[l].state_dict().items() if not k.startswith("linear1") and k != "linear2.weight"}
    sd["linear1.weight"] = gen.randn("linear1.weight", (FF, 128), FF + l, 1.0 / math.sqrt(128))
    sd["linear1.bias"] = gen.randn("linear1.bias", (FF,), FF + l, 0.1)
    sd["linear2.weight"] = gen.randn("linear2.weight", (128, FF), FF + l, 1.0 / math.sqrt(FF))
    lay.load_state_dict(sd, strict=True)
    return lay


def params(layer):
    """A layer's state_dict as detached CPU float32 tensors (what tests/token_ref.py takes)."""
    return {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}


def tail_inputs(M, seed):
    """(ctx, x) [M, 128] of a tail case: the layer's input and an attention output of the magnitude a softmax average has."""
    return gen.randn("ctx", (M, 128), seed + 10, 0.7), gen.randn("x", (M, 128), seed)


def tail_seed(M, FF, l):
    return M + FF // 128 + l


def expected_groups(M, FF):
    """The few-token rule of include/objcavit_hip.h, restated: 8 workgroups per row block up to 24 row blocks, 4 up to 56, else
    1; halved until it divides the number of 128-unit feed-forward chunks."""
    nblk, nchunk = (M + 31) // 32, FF // 128
    G = 8 if nblk <= 24 else 4 if nblk <= 56 else 1
    while G > 1 and nchunk % G:
        G //= 2
    return G


def key_mask(counts, S):
    """bool [B, S], True = padding (key j >= counts[b])."""
    return torch.arange(S)[None, :] >= torch.tensor(counts)[:, None]
