"""The per-object / per-region metric record (include/objcavit_hip.h: ocv_object_metrics_fwd) as a CPU statement, COMPOSED from pieces
that are pinned elsewhere: the per-pixel value and the sums are oracle/validation_ref.py's (``tta_average``, ``metrics_preprocess``,
``pixel_sums``, ``finish`` -- held to the reference project's own classes by tests/test_oracle_golden.py), the pixels of a box are
tests/object_depth_ref.py's ``box_pixels`` (held to a brute-force loop by tests/test_object_depth_host.py).  There is no counterpart in
the reference project; this file IS the definition the kernels are held to.  ``brute_force`` is the segmentation from first principles (a
Python loop over every pixel, the centre rule in exact comparisons, ``math.fsum``); tests/test_object_metrics_host.py holds the two
against each other.  The file also makes the inputs the host and the GPU tests share."""
import math

import torch
import torch.nn.functional as F

import object_depth_ref as odr
from oracle import validation_ref as vr

FIELDS = 10          # the eight metrics, n_valid, gt_mean
MIN_DEPTH, MAX_DEPTH = 1e-3, 10.0
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
BAND = 1e-5          # relative guard band round the delta thresholds (see ``guard``)


def pixel_value(pred, gt, min_depth, max_depth, pred_mirror=None, crop=None):
    """(the resized, fixed prediction fp32 [B, 1, H, W]; the valid mask bool [B, 1, H, W]) -- the validation step's own statements;
    ``crop`` = (y0, y1, x0, x1) is applied here (the oracle's crop takes dataset flags, this one any box)."""
    p = vr.tta_average(pred, pred_mirror, min_depth, max_depth) if pred_mirror is not None else torch.clamp(pred, min=min_depth, max=max_depth)
    p, mask = vr.metrics_preprocess(p, gt, min_depth, max_depth)
    if crop is not None:
        ev = torch.zeros(gt.shape[2:], dtype=torch.bool)
        ev[crop[0]:crop[1], crop[2]:crop[3]] = True
        mask = mask & ev
    return p, mask


def record(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """One float64 row from the [H, W] maps p, g over the pixels of the bool map m: all zero when m is empty."""
    out = torch.zeros(FIELDS, dtype=torch.float64)
    if not bool(m.any()):
        return out
    f = vr.finish(vr.pixel_sums(p[m], g[m]))
    out[:8] = torch.tensor([f[k] for k in vr.METRICS], dtype=torch.float64)
    out[8] = float(m.sum())
    out[9] = g[m].double().mean()
    return out


def box_masks(xywh, counts, b: int, H: int, W: int, shrink: float):
    """Per row of image b its pixels as a bool [H, W] map, or None (a row at or beyond the count, an empty box)."""
    out = []
    for r in range(int(xywh.shape[1])):
        px = odr.box_pixels(xywh[b, r], H, W, shrink) if r < int(counts[b]) else None
        if px is None:
            out.append(None)
            continue
        m = torch.zeros(H, W, dtype=torch.bool)
        m[px[2]:px[3], px[0]:px[1]] = True
        out.append(m)
    return out


def object_metrics(pred, gt, xywh, counts, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, crop=None, pred_mirror=None, shrink=1.0):
    """-> (boxes float64 [B, cap, 10], regions float64 [B, 2, 10]), all on the host."""
    pred, gt, xywh = pred.detach().cpu().float(), gt.detach().cpu().float(), xywh.detach().cpu().float()
    pred_mirror = None if pred_mirror is None else pred_mirror.detach().cpu().float()
    p, mask = pixel_value(pred, gt, min_depth, max_depth, pred_mirror, crop)
    B, _, H, W = gt.shape
    cap = int(xywh.shape[1])
    boxes = torch.zeros(B, cap, FIELDS, dtype=torch.float64)
    regions = torch.zeros(B, 2, FIELDS, dtype=torch.float64)
    for b in range(B):
        union = torch.zeros(H, W, dtype=torch.bool)
        for r, m in enumerate(box_masks(xywh, counts, b, H, W, shrink)):
            if m is None:
                continue
            boxes[b, r] = record(p[b, 0], gt[b, 0], m & mask[b, 0])
            union |= m
        regions[b, 0] = record(p[b, 0], gt[b, 0], union & mask[b, 0])
        regions[b, 1] = record(p[b, 0], gt[b, 0], ~union & mask[b, 0])
    return boxes, regions


def recombine(rows: torch.Tensor) -> torch.Tensor:
    """[..., K, 10] float64 rows -> [..., 10]: the record of the union of K DISJOINT pixel sets (n-weighted, RMSEs through their squares)."""
    rows = rows.double()
    n = rows[..., 8:9]
    tot = n.sum(-2).clamp(min=1.0)
    v = rows.clone()
    v[..., 2:4] = v[..., 2:4] ** 2
    out = (v * n).sum(-2) / tot
    out[..., 2:4] = out[..., 2:4].sqrt()
    out[..., 8] = n.sum(-2)[..., 0]
    return out


def delta_counts(rows: torch.Tensor) -> torch.Tensor:
    """delta_k * n_valid of [..., 10] rows as exact integers (float64): a mean of 0 / 1 values times its count."""
    rows = rows.detach().cpu().double()
    return torch.round(rows[..., 5:8] * rows[..., 8:9])


def brute_force(p, g, valid, box, shrink: float = 1.0):
    """(row of 10 Python floats over the box's valid pixels, bool [H, W] map of the box's pixels): every pixel of the [H, W] maps tested
    by the centre rule in exact (double on fp32 operands) comparisons against the fp32 edges; ``box`` None: no pixel."""
    H, W = g.shape
    inside = torch.zeros(H, W, dtype=torch.bool)
    if box is None:
        return [0.0] * FIELDS, inside
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))             # noqa: E731
    cx, cy, w, h = (f32(float(v)) for v in box[:4])
    half = f32(0.5 * float(shrink))
    hw, hh = f32(half * w), f32(half * h)
    xl, xh, yl, yh = f32(cx - hw), f32(cx + hw), f32(cy - hh), f32(cy + hh)
    if not all(math.isfinite(e) for e in (xl, xh, yl, yh)):
        return [0.0] * FIELDS, inside
    for y in range(H):
        for x in range(W):
            inside[y, x] = xl <= x + 0.5 < xh and yl <= y + 0.5 < yh
    return brute_record(p, g, valid & inside), inside


def brute_record(p, g, m):
    """The record over the pixels of m from Python floats: every term in double, ``math.fsum``."""
    t = [[] for _ in range(9)]
    for y, x in m.nonzero().tolist():
        a, e = float(p[y, x]), float(g[y, x])
        ratio = max(e / a, a / e)
        for i, v in enumerate((abs(e - a) / e, (e - a) ** 2 / e, (e - a) ** 2, (math.log(e) - math.log(a)) ** 2,
                               abs(math.log10(e) - math.log10(a)), float(ratio < 1.25), float(ratio < 1.25 ** 2), float(ratio < 1.25 ** 3), e)):
            t[i].append(v)
    n = len(t[0])
    if n == 0:
        return [0.0] * FIELDS
    s = [math.fsum(v) / n for v in t]
    return [s[0], s[1], math.sqrt(s[2]), math.sqrt(s[3]), s[4], s[5], s[6], s[7], float(n), s[8]]


# ---------------------------------------------------------------------------
# the inputs the host and the GPU tests share
# ---------------------------------------------------------------------------
def in_band(p, gt, mask) -> torch.Tensor:
    """bool map of the VALID pixels whose float64 ratio max(gt / p, p / gt) lies within ``BAND`` (relative) of a delta threshold: there
    the kernel's fp32 value of p -- a few roundings (four taps, an average, a division: a few x 6e-8) away from the reference's -- could
    land on the other side, and a one-pixel box would read 0 instead of 1."""
    g, q = gt.double(), p.double()
    ratio = torch.maximum(g / q, q / g)
    near = torch.zeros_like(mask)
    for t in THRESHOLDS:
        near |= (ratio / t - 1.0).abs() < BAND
    return near & mask


def guard(pred, gt, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, pred_mirror=None) -> torch.Tensor:
    """gt with every valid pixel inside the guard band scaled by 1.001 until none is left (gt has the full resolution, so every pixel
    is independent of the others; p does not depend on gt)."""
    gt = gt.clone()
    for _ in range(20):
        p, mask = pixel_value(pred, gt, min_depth, max_depth, pred_mirror)
        near = in_band(p, gt, mask)
        if not bool(near.any()):
            return gt
        gt[near] *= 1.001
    raise AssertionError("guard band not empty after 20 rounds")


def band_size(pred, gt, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, pred_mirror=None) -> int:
    p, mask = pixel_value(pred, gt, min_depth, max_depth, pred_mirror)
    return int(in_band(p, gt, mask).sum())


def case_maps(B=3, H=odr.CASE_H, W=odr.CASE_W, h=19, w=27, mirror=True, seed=0, special=False, dead_image=None):
    """(pred [B, 1, h, w], pred_mirror or None, gt [B, 1, H, W]): gt in (0.5, 11) with ~ 5 % zeros (about one pixel in seven is invalid),
    the prediction a noisy resize of it with values on both sides of the depth range (the clamp), the mirrored output a noisy mirror of
    the prediction.  ``special``: a NaN and a +inf tap in pred (and a NaN in the mirror); ``dead_image``: that image's gt is all zero.
    gt is guarded (``guard``)."""
    g = torch.Generator().manual_seed(4000 + seed)
    gt = torch.rand(B, 1, H, W, generator=g) * 10.5 + 0.5
    gt[torch.rand(B, 1, H, W, generator=g) < 0.05] = 0.0
    base = gt if (h, w) == (H, W) else F.interpolate(gt, (h, w), mode="bilinear", align_corners=True)
    pred = base * (1.0 + 0.3 * torch.randn(B, 1, h, w, generator=g)) + 0.05
    pred_mirror = (pred * (1.0 + 0.05 * torch.randn(B, 1, h, w, generator=g))).flip(3).contiguous() if mirror else None
    if special:
        pred[0, 0, h // 3, w // 3] = float("nan")
        pred[min(1, B - 1), 0, h // 2, w // 2] = float("inf")
        if mirror:
            pred_mirror[B - 1, 0, h // 4, w // 4] = float("nan")
    if dead_image is not None:
        gt[dead_image] = 0.0
    return pred, pred_mirror, guard(pred, gt, pred_mirror=pred_mirror)


def random_boxes(B, cap, counts, H, W, seed=0):
    """(xywh [B, cap, 4], counts int32 [B]): seeded boxes over and a little beyond the map, every row filled (rows beyond a count too)."""
    g = torch.Generator().manual_seed(5000 + seed)
    c = torch.rand(B, cap, 2, generator=g) * torch.tensor([W + 16.0, H + 16.0]) - 8.0
    s = torch.rand(B, cap, 2, generator=g) * torch.tensor([W / 3.0, H / 3.0]) + 0.5
    return torch.cat([c, s], 2), torch.tensor(counts, dtype=torch.int32)


GARG_STYLE = lambda H, W: (int(0.40810811 * H), int(0.99189189 * H), int(0.03594771 * W), int(0.96405229 * W))     # noqa: E731
NYU_EIGEN = (45, 471, 41, 601)
