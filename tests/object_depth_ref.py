"""The per-object depth record (include/objcavit_hip.h: ocv_object_depth_fwd) as a plain torch CPU statement: fp32 box edges in the
stated order, ``torch.sort`` for the order statistics, float64 sums.  There is no counterpart in the reference project; this file IS the
definition the kernel is held to.  ``brute_force`` is the same record from first principles (a Python loop over every pixel of the map,
membership by the centre rule in exact arithmetic on the fp32 operands, ``sorted``): tests/test_object_depth_host.py holds the two
against each other."""
import math

import torch

FIELDS = 5          # n, min, max, mean, std_mean


def _edges(c: torch.Tensor, size: torch.Tensor, half: torch.Tensor, limit: int):
    """(lo, hi) of the pixel range along one axis, or None for an empty range.  0-d fp32 tensors: every statement rounds to fp32."""
    hs = half * size
    lo = torch.ceil((c - hs) - 0.5)
    hi = torch.ceil((c + hs) - 0.5)
    if not (bool(torch.isfinite(lo)) and bool(torch.isfinite(hi))):
        return None
    lo = int(lo.clamp(0.0, float(limit)))
    hi = int(hi.clamp(0.0, float(limit)))
    return (lo, hi) if hi > lo else None


def box_pixels(box: torch.Tensor, H: int, W: int, shrink: float = 1.0):
    """(x0, x1, y0, y1) of a box (cx, cy, w, h, ...) on an H x W map, or None."""
    box = box.to(torch.float32)
    half = torch.tensor(0.5 * float(shrink), dtype=torch.float32)          # rounded once, on the host
    xs = _edges(box[0], box[2], half, W)
    ys = _edges(box[1], box[3], half, H)
    return None if xs is None or ys is None else xs + ys


def record(values: torch.Tensor, std_values, quantiles) -> torch.Tensor:
    """One row from the box's pixels (any shape, fp32) and the matching ``depth_std`` pixels (or None)."""
    out = torch.zeros(FIELDS + len(quantiles), dtype=torch.float32)
    values = values.reshape(-1)
    keep = ~torch.isnan(values)
    v = torch.sort(values[keep]).values
    n = int(v.numel())
    if n == 0:
        return out
    out[0] = float(n)
    out[1], out[2] = v[0], v[n - 1]
    out[3] = (v.to(torch.float64).sum() / n).to(torch.float32)
    if std_values is not None:
        out[4] = (std_values.reshape(-1)[keep].to(torch.float64).sum() / n).to(torch.float32)
    for i, q in enumerate(quantiles):
        out[FIELDS + i] = v[min(int(math.floor(float(q) * float(n - 1))), n - 1)]
    return out


def object_depth(depth: torch.Tensor, xywh: torch.Tensor, counts, depth_std=None, quantiles=(0.1, 0.5, 0.9), shrink: float = 1.0) -> torch.Tensor:
    """depth [B, 1, H, W], xywh [B, cap, >= 4], counts [B] -> [B, cap, 5 + Q], all on the host."""
    depth, xywh = depth.detach().cpu().float(), xywh.detach().cpu().float()
    depth_std = None if depth_std is None else depth_std.detach().cpu().float()
    B, _, H, W = depth.shape
    cap = xywh.shape[1]
    out = torch.zeros(B, cap, FIELDS + len(quantiles), dtype=torch.float32)
    for b in range(B):
        for r in range(min(int(counts[b]), cap)):
            px = box_pixels(xywh[b, r], H, W, shrink)
            if px is None:
                continue
            x0, x1, y0, y1 = px
            out[b, r] = record(depth[b, 0, y0:y1, x0:x1], None if depth_std is None else depth_std[b, 0, y0:y1, x0:x1], quantiles)
    return out


def brute_force(depth: torch.Tensor, box, quantiles=(0.1, 0.5, 0.9), shrink: float = 1.0, depth_std=None):
    """One row as a list of Python floats: every pixel of the [H, W] map tested by the centre rule, in exact (double on fp32 operands)
    comparisons against the fp32 edges cx -+ half * size."""
    H, W = depth.shape
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))             # noqa: E731
    cx, cy, w, h = (f32(float(v)) for v in box[:4])
    half = f32(0.5 * float(shrink))
    hw, hh = f32(half * w), f32(half * h)
    xl, xh, yl, yh = f32(cx - hw), f32(cx + hw), f32(cy - hh), f32(cy + hh)
    row = [0.0] * (FIELDS + len(quantiles))
    if not all(math.isfinite(e) for e in (xl, xh, yl, yh)):
        return row
    vals, stds = [], []
    for y in range(H):
        for x in range(W):
            if xl <= x + 0.5 < xh and yl <= y + 0.5 < yh:
                v = float(depth[y, x])
                if v == v:
                    vals.append(v)
                    stds.append(0.0 if depth_std is None else float(depth_std[y, x]))
    n = len(vals)
    if n == 0:
        return row
    vals = sorted(vals)
    total = lambda vs: sum(vs) if any(math.isinf(v) or v != v for v in vs) else math.fsum(vs)      # noqa: E731  (fsum refuses inf - inf)
    row[0:5] = [float(n), vals[0], vals[-1], f32(total(vals) / n), f32(total(stds) / n)]
    for i, q in enumerate(quantiles):
        row[FIELDS + i] = vals[min(int(math.floor(q * (n - 1))), n - 1)]
    return row


# ---------------------------------------------------------------------------
# the inputs the host and the GPU tests share
# ---------------------------------------------------------------------------
CASE_H, CASE_W, CASE_COUNTS = 37, 53, (6, 1, 3)
_NAN, _INF = float("nan"), float("inf")
_SPARE = (10.0, 7.0, 2.0, 2.0)          # a valid box in every row at or beyond an image's count: it must come out all zero
BOX_SETS = {
    # whole map; one pixel; edges exactly on pixel centres (lower edge in, upper edge out): 1 and 4 pixels; 15 pixels; 1 pixel at the
    # corner | a 1e30-wide box | an infinite width, a box over the corner, an odd box in the middle
    "inside": [[(26.5, 18.5, 53.0, 37.0), (20.5, 11.5, 1.0, 1.0), (10.0, 7.0, 1.0, 1.0), (10.0, 7.0, 2.0, 2.0), (10.3, 7.7, 4.6, 3.2),
                (0.2, 0.2, 1.0, 1.0)],
               [(26.0, 18.0, 1e30, 10.0)],
               [(5.0, 5.0, _INF, 3.0), (0.0, 0.0, 7.0, 5.0), (26.5, 18.5, 20.25, 11.75)]],
    # over the left, right, top and bottom border; fully outside; the <UNK> box | zero size | NaN and +inf coordinates, 1e30 x 1e30
    "borders": [[(-2.0, 10.0, 10.0, 6.0), (52.0, 10.0, 8.0, 6.0), (20.0, -1.0, 6.0, 8.0), (20.0, 36.0, 6.0, 9.0), (100.0, 100.0, 5.0, 5.0),
                 (-1.0, -1.0, -1.0, -1.0)],
                [(10.0, 10.0, 0.0, 0.0)],
                [(_NAN, 5.0, 3.0, 3.0), (_INF, 5.0, 3.0, 3.0), (3.0, 4.0, 1e30, 1e30)]],
    # n = 1, 2, 3, 4 (the lower median), a column of 5, a row of 40 | a 9 x 9 block | 2 x 3, 3 x 2, 30 x 30
    "small": [[(20.5, 11.5, 1.0, 1.0), (21.0, 11.5, 2.0, 1.0), (21.5, 11.5, 3.0, 1.0), (31.0, 21.0, 2.0, 2.0), (3.5, 10.5, 1.0, 5.0),
               (25.0, 30.5, 40.0, 1.0)],
              [(30.5, 20.5, 9.0, 9.0)],
              [(41.0, 5.5, 2.0, 3.0), (41.5, 9.0, 3.0, 2.0), (26.0, 18.0, 30.0, 30.0)]],
}
VALUE_KINDS = ("uniform", "three_values", "constant", "byte0", "byte1", "byte2", "byte3", "special")


def case_boxes(name: str, width: int = 4):
    """(xywh [3, 6, width], counts int32 [3]) of a box set; columns beyond the fourth hold a large number that must not be read as a box."""
    xywh = torch.full((len(CASE_COUNTS), max(CASE_COUNTS), width), 1000.0)
    xywh[:, :, :4] = torch.tensor(_SPARE)
    for b, rows in enumerate(BOX_SETS[name]):
        assert len(rows) == CASE_COUNTS[b]
        xywh[b, :len(rows), :4] = torch.tensor(rows)
    return xywh, torch.tensor(CASE_COUNTS, dtype=torch.int32)


def case_map(kind: str, B: int = 3, H: int = CASE_H, W: int = CASE_W, seed: int = 0) -> torch.Tensor:
    """fp32 [B, 1, H, W].  three_values: ties across every radix digit; constant; byteN: the values differ ONLY in byte N of their bit
    pattern, so radix pass 3 - N alone decides (byte3: positive finite values only); special: negative values, +-0, +-inf and NaN
    pixels, and NaN over the pixels (20..22, 11) -- the n = 1, 2, 3 boxes of the "small" set and the one-pixel box of "inside"."""
    g = torch.Generator().manual_seed(1000 + seed)
    shape = (B, 1, H, W)
    if kind == "uniform":
        return torch.rand(shape, generator=g) * 9.9 + 0.1
    if kind == "three_values":
        return torch.tensor([0.75, 2.5, 2.5000002])[torch.randint(0, 3, shape, generator=g)]
    if kind == "constant":
        return torch.full(shape, 3.1400001)
    if kind.startswith("byte"):
        n = int(kind[4])
        r = torch.randint(1 if n == 3 else 0, 127 if n == 3 else 256, shape, generator=g, dtype=torch.int32)      # (byte3: no denormals)
        base = 0x40490FDB & ~(0xFF << (8 * n))
        return (r * (1 << (8 * n)) + base).view(torch.float32)
    if kind == "special":
        m = torch.rand(shape, generator=g) * 20.0 - 10.0
        pick = torch.randint(0, 40, shape, generator=g)
        for code, v in enumerate((0.0, -0.0, _NAN)):
            m[pick == code] = v
        m[:, :, 30:, 40:][pick[:, :, 30:, 40:] == 3] = _INF          # +inf only in the lower right corner, -inf only in the upper right
        m[:, :, :6, 40:][pick[:, :, :6, 40:] == 3] = -_INF
        m[:, :, 11, 20:23] = _NAN
        m[:, :, 33, 45], m[:, :, 2, 45] = _INF, -_INF                  # both in every image: the whole map's sum is inf - inf
        return m
    raise ValueError(kind)


def within_one_ulp(got: torch.Tensor, want: torch.Tensor) -> bool:
    """fp32 ``got`` against the fp32 rounding ``want`` of a float64 reference: equal, both NaN, or finite and at most one unit in the
    last place apart (as ordered integers of the bit patterns: adjacent floats differ by one)."""
    got, want = got.detach().cpu().float().reshape(-1), want.detach().cpu().float().reshape(-1)
    both_nan = torch.isnan(got) & torch.isnan(want)
    key = lambda t: torch.where(t.view(torch.int32) < 0, -(t.view(torch.int32) & 0x7FFFFFFF), t.view(torch.int32)).to(torch.int64)   # noqa: E731
    near = torch.isfinite(got) & torch.isfinite(want) & ((key(got) - key(want)).abs() <= 1)
    return bool((both_nan | near | (got == want)).all())
