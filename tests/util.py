"""Shared helpers for the tests (fixtures loading, comparisons)."""
import json
import os

import numpy as np
import torch

import gen  # tests/golden/gen.py (on sys.path via conftest)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, {k: z[k] for k in z.files if k != "meta"}


def gains_of(meta):
    return [tuple(g) for g in meta.get("gains", [])]


def rel_dev(a, b):
    """max |a-b| / max |b| (both converted to float64 CPU tensors)."""
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def max_rel(a, b):
    """max elementwise |a-b| / |b| (for strictly positive b such as depth)."""
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float(((a - b).abs() / b.abs()).max())


def state_dict_from(meta_shapes, seed, gains=()):
    return gen.fill({k: tuple(v) for k, v in meta_shapes.items()}, seed, gains)


def golden_sample_dev(x, z, t, images=None):
    """(sampled deviation, moment deviation) of a [B, C, H, W] tensor ``x`` (NCHW or channels_last, CPU or GPU) against the
    stored tensor ``t`` of a sampled fixture (G8: ``<t>_idx`` (n, c, h, w), ``<t>_val``, per (image, channel) ``<t>_mean`` /
    ``<t>_rms``), both as max |difference| / ``<t>_absmax`` -- normalised like rel_dev on the whole tensor.  ``images``: the
    fixture's image indices that x's batch entries hold, in order (x a subset of the batch); None: x is the whole batch."""
    idx = torch.from_numpy(z[t + "_idx"].astype(np.int64))
    mean, rms = torch.from_numpy(z[t + "_mean"]).double(), torch.from_numpy(z[t + "_rms"]).double()
    val = torch.from_numpy(z[t + "_val"]).double()
    if images is not None:
        pos = torch.full((mean.shape[0],), -1, dtype=torch.int64)
        pos[torch.as_tensor(list(images))] = torch.arange(len(images))
        sel = pos[idx[:, 0]] >= 0
        idx, val = idx[sel], val[sel]
        idx[:, 0] = pos[idx[:, 0]]
        mean, rms = mean[list(images)], rms[list(images)]
    assert tuple(x.shape[:2]) == tuple(mean.shape), (tuple(x.shape), tuple(mean.shape))
    n, c, h, w = idx.to(x.device).unbind(1)
    got = x[n, c, h, w].double().cpu()
    xd = x.detach().double()
    got_mean, got_rms = xd.mean((2, 3)).cpu(), xd.pow(2).mean((2, 3)).sqrt().cpu()
    den = float(z[t + "_absmax"])
    samp = float((got - val).abs().max()) / den
    mom = max(float((got_mean - mean).abs().max()), float((got_rms - rms).abs().max())) / den
    return samp, mom


def branch_dev(y, ref, x=None):
    """Per image (dim 0) of a block's output ``y`` against its float64 reference ``ref``: max |y - ref| / max |ref - x| for a
    residual block with input ``x`` -- relative to the residual branch rather than the stream it is added to -- and
    max |y - ref| / max |ref| without ``x``.  Returns a list of floats, one per image."""
    y = torch.as_tensor(y).detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    den = ref if x is None else ref - torch.as_tensor(x).detach().cpu().double()
    num = (y - ref).flatten(1).abs().amax(1)
    return (num / (den.flatten(1).abs().amax(1) + 1e-30)).tolist()
