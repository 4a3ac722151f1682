"""Reference statements of the bin head's per-pixel statistics, in torch on the CPU, float64 unless told
otherwise.  ``head_stats`` forms the full softmax; ``full_stats`` forms the mixture at full resolution by an explicit loop over taps."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def head_stats(feat: torch.Tensor, queries: torch.Tensor, wout: torch.Tensor, bout: torch.Tensor, centers: torch.Tensor,
               dtype=torch.float64) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """modules/GraphBins.py:109-119 (pixel-wise dot product, conv_out = 1x1 convolution + softmax, centre-weighted sum) plus
    var = sum_k p_k (c_k - d)^2 and pmax = max_k p_k.  feat [B, C, h, w], queries [B, Q, C], wout [n, Q(, 1, 1)], bout [n],
    centers [B, n] -> (d, var, pmax), each [B, 1, h, w]."""
    f, q, c = feat.detach().cpu().to(dtype), queries.detach().cpu().to(dtype), centers.detach().cpu().to(dtype)
    B, C, h, w = f.shape
    ram = torch.einsum("ncp,nqc->nqp", f.reshape(B, C, h * w), q).reshape(B, q.shape[1], h, w)
    n = wout.shape[0]
    p = torch.softmax(F.conv2d(ram, wout.detach().cpu().to(dtype).reshape(n, -1, 1, 1), bout.detach().cpu().to(dtype)), dim=1)
    c = c.view(B, n, 1, 1)
    d = torch.sum(p * c, dim=1, keepdim=True)
    var = torch.sum(p * (c - d) ** 2, dim=1, keepdim=True)
    return d, var, p.amax(dim=1, keepdim=True)


def head_stats_fp32(feat, queries, wout, bout, centers, min_depth: float, max_depth: float):
    """What a user of the reference would write in plain fp32 torch: out = softmax(conv_out(ram)), d = sum out c, and the variance as
    the second moment about the middle of the depth range minus the squared mean offset.  -> (d, var, pmax) fp32."""
    f, q, c = feat.detach().cpu().float(), queries.detach().cpu().float(), centers.detach().cpu().float()
    B, C, h, w = f.shape
    ram = torch.einsum("ncp,nqc->nqp", f.reshape(B, C, h * w), q).reshape(B, q.shape[1], h, w)
    n = wout.shape[0]
    out = torch.softmax(F.conv2d(ram, wout.detach().cpu().float().reshape(n, -1, 1, 1), bout.detach().cpu().float()), dim=1)
    c = c.view(B, n, 1, 1)
    c0 = torch.tensor(0.5 * (min_depth + max_depth), dtype=torch.float32)
    d = torch.sum(out * c, dim=1, keepdim=True)
    var = torch.sum(out * (c - c0) ** 2, dim=1, keepdim=True) - (d - c0) ** 2
    return d, var, out.max(dim=1, keepdim=True).values


def tap_coefficients(n_in: int, n_out: int, dtype=torch.float64):
    """ATen upsample_bilinear2d, align_corners=True, along one axis (the coefficients tests/predict_ref.py's F.interpolate uses):
    -> (i0, i1, l0, l1), source = l0 * in[i0] + l1 * in[i1]."""
    scale = torch.tensor(float(n_in - 1), dtype=dtype) / torch.tensor(float(n_out - 1), dtype=dtype) if n_out > 1 else torch.zeros((), dtype=dtype)
    src = scale * torch.arange(n_out, dtype=dtype)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = src - i0.to(dtype)
    return i0, i1, 1.0 - l1, l1


def full_stats(d: torch.Tensor, var: torch.Tensor, pmax: torch.Tensor, d_m: Optional[torch.Tensor], var_m: Optional[torch.Tensor],
               pmax_m: Optional[torch.Tensor], size: Tuple[int, int], dtype=torch.float64, span: Optional[float] = None):
    """The mixture of the source distributions at every output pixel of ``size`` = (H, W): weights = the bilinear align_corners
    weights, halved over the map and the un-mirrored mirror map when ``d_m`` is given.  m = sum w_t d_t (unclamped),
    var_full = sum w_t (var_t + (d_t - m)^2), confidence = sum w_t pmax_t, by an explicit loop over the taps (zero-weight taps
    included: 0 * NaN = NaN, as ATen's resize has it).  -> (depth_std, confidence, var_full, m), each [B, 1, H, W]; with ``span`` a NaN
    becomes span (depth_std) / 0 (confidence)."""
    H, W = int(size[0]), int(size[1])
    srcs = [(d.cpu().to(dtype), var.cpu().to(dtype), pmax.cpu().to(dtype))]
    if d_m is not None:
        srcs.append(tuple(t.cpu().to(dtype).flip(3) for t in (d_m, var_m, pmax_m)))
    share = torch.tensor(1.0 / len(srcs), dtype=dtype)
    h, w = srcs[0][0].shape[2:]
    taps = []                                                   # (weight [H, W], d, var, pmax at the tap, each [B, 1, H, W])
    if (h, w) == (H, W):                                        # ATen's identity short-cut: the pixel itself
        for s in srcs:
            taps.append((share.expand(H, W),) + s)
    else:
        y0, y1, ly0, ly1 = tap_coefficients(h, H, dtype)
        x0, x1, lx0, lx1 = tap_coefficients(w, W, dtype)
        for iy, wy in ((y0, ly0), (y1, ly1)):
            for ix, wx in ((x0, lx0), (x1, lx1)):
                wt = wy[:, None] * wx[None, :]
                for s in srcs:
                    taps.append((wt * share,) + tuple(t[:, :, iy][:, :, :, ix] for t in s))
    m = sum(wt * dd for wt, dd, _, _ in taps)
    var_full = sum(wt * (vv + (dd - m) ** 2) for wt, dd, vv, _ in taps)
    conf = sum(wt * pp for wt, _, _, pp in taps)
    std = torch.sqrt(var_full)
    if span is not None:
        std = torch.where(torch.isnan(std), torch.tensor(span, dtype=dtype), std)
        conf = torch.where(torch.isnan(conf), torch.zeros((), dtype=dtype), conf)
    return std, conf, var_full, m
