"""Statement L of the lens on ingest (include/objcavit_hip.h, csrc/frame_remap.hip, objcavit_amd/lens.py), in numpy integers on the host,
and the two lens models restated in float64 from their formulas.  Nothing here imports the package.

    map    int32 [M, Hw, Ww, 2], M = 1 or B; entry (X, Y) of rectified pixel (u, v): its source coordinate in 1/256 pixel of the whole frame
           X = floor(xs * 256 + 0.5), clamped to [-256, Ws * 256] (Y: [-256, Hs * 256]), NaN -> -256
    taps   x0 = X >> 8, wx = X & 255, y0 = Y >> 8, wy = Y & 255; (x0, y0) (x0 + 1, y0) (x0, y0 + 1) (x0 + 1, y0 + 1);
           outside 0 <= x < Ws, 0 <= y < Hs: R = G = B = 0; inside: the pixel's R, G, B in the frames' format (tests/pixel_format_ref.py)
    byte   ((256 - wx)(256 - wy) v00 + wx (256 - wy) v10 + (256 - wx) wy v01 + wx wy v11 + 32768) >> 16
    fused  table[c][byte] at (b, c, v, u); the mirror at (b + mirror, c, v, Ww - 1 - u)
"""
import math

import numpy as np

import pixel_format_ref

ONE = 256


def quantise(xs, ys, Hs, Ws):
    """float64 coordinates -> int32 [..., 2], element by element in Python floats."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    out = np.empty(xs.shape + (2,), dtype=np.int32)
    for idx in np.ndindex(xs.shape):
        for k, (c, n) in enumerate(((xs[idx], Ws), (ys[idx], Hs))):
            if math.isnan(c):
                q = -ONE
            elif math.isinf(c):
                q = -ONE if c < 0 else n * ONE
            else:
                q = min(max(math.floor(c * ONE + 0.5), -ONE), n * ONE)
            out[idx + (k,)] = q
    return out


def taps_inside(m, Hs, Ws):
    """int64 [..., Hw, Ww]: how many of the four taps of every entry lie inside the frame."""
    m = np.asarray(m).astype(np.int64)
    x0, y0 = m[..., 0] >> 8, m[..., 1] >> 8
    n = np.zeros(x0.shape, dtype=np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            n += ((x0 + dx >= 0) & (x0 + dx < Ws) & (y0 + dy >= 0) & (y0 + dy < Hs))
    return n


def remap_rgb(rgb, m):
    """uint8 RGB frames [B, Hs, Ws, 3] (the frames' pixels by their format's fetch) through ``m`` int32 [M, Hw, Ww, 2] -> uint8 [B, Hw, Ww, 3]."""
    rgb = np.asarray(rgb).astype(np.int64)
    m = np.asarray(m).astype(np.int64)
    B, Hs, Ws, _ = rgb.shape
    if m.shape[0] == 1:
        m = np.broadcast_to(m, (B,) + m.shape[1:])
    assert m.shape[0] == B and m.shape[3] == 2
    X, Y = m[..., 0], m[..., 1]
    x0, wx, y0, wy = X >> 8, X & 255, Y >> 8, Y & 255
    bi = np.arange(B).reshape(B, 1, 1)
    acc = np.zeros(X.shape + (3,), dtype=np.int64)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        x, y = x0 + dx, y0 + dy
        inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
        v = rgb[bi, np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)] * inside[..., None]
        w = (wx if dx else ONE - wx) * (wy if dy else ONE - wy)
        acc += w[..., None] * v
    assert int(acc.max(initial=0)) + 32768 <= 255 * 65536 + 32768
    return ((acc + 32768) >> 16).astype(np.uint8)


def rectified_rgb(frames, fmt, m):
    """Frames of any format (as ``pixel_format_ref.rgb_of`` takes them) -> the rectified window uint8 [B, Hw, Ww, 3]."""
    planes = [pixel_format_ref._np(p) for p in frames] if isinstance(frames, (list, tuple)) else pixel_format_ref._np(frames)
    y = planes[0] if isinstance(planes, list) else planes
    Hs, Ws = y.shape[1], y.shape[2]
    return remap_rgb(pixel_format_ref.rgb_of(planes, fmt, 0, 0, Hs, Ws), m)


def ingest(rgb_window, table, mirror):
    """uint8 [B, Hw, Ww, 3] -> fp32 [B or 2B, 3, Hw, Ww]: table[c][byte], the mirrored batch behind."""
    table = np.asarray(table, dtype=np.float32)
    out = np.stack([table[c][rgb_window[..., c]] for c in range(3)], 1)
    return np.concatenate([out, out[..., ::-1]], 0) if mirror else out


def remap_ingest(frames, fmt, m, table, mirror=False):
    return ingest(rectified_rgb(frames, fmt, m), table, mirror)


# --------------------------------------------------------------------------- the lens models, pixel by pixel in Python floats (float64)
def _ray(u, v, new_K, R):
    fx, fy, cx, cy = new_K
    x, y = (u - cx) / fx, (v - cy) / fy
    if R is not None:
        X = R[0][0] * x + R[1][0] * y + R[2][0]
        Y = R[0][1] * x + R[1][1] * y + R[2][1]
        W = R[0][2] * x + R[1][2] * y + R[2][2]
        if not W > 0.0:
            return float("nan"), float("nan")
        x, y = X / W, Y / W
    return x, y


def brown_point(x, y, K, dist):
    """The ideal ray (x, y) -> the distorted pixel of the rational Brown-Conrady model."""
    fx, fy, cx, cy = K
    k1, k2, p1, p2, k3, k4, k5, k6 = list(dist) + [0.0] * (8 - len(dist))
    r2 = x * x + y * y
    s = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * s + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * s + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def fisheye_point(x, y, K, dist4):
    """The ideal ray (x, y) -> the distorted pixel of the Kannala-Brandt model."""
    fx, fy, cx, cy = K
    r = math.sqrt(x * x + y * y)
    if r == 0.0:
        return cx, cy
    th = math.atan(r)
    thd = th * (1 + dist4[0] * th ** 2 + dist4[1] * th ** 4 + dist4[2] * th ** 6 + dist4[3] * th ** 8)
    return fx * (thd / r) * x + cx, fy * (thd / r) * y + cy


def model_coordinates(point, K, dist, window_size, new_K=None, R=None):
    """float64 (xs, ys) [Hw, Ww] of ``point`` = brown_point / fisheye_point over the rectified window."""
    Hw, Ww = window_size
    new_K = K if new_K is None else new_K
    xs, ys = np.empty((Hw, Ww)), np.empty((Hw, Ww))
    for v in range(Hw):
        for u in range(Ww):
            x, y = _ray(float(u), float(v), new_K, R)
            xs[v, u], ys[v, u] = (float("nan"), float("nan")) if math.isnan(x) else point(x, y, K, dist)
    return xs, ys
