"""Lens on ingest: the map from the rectified window to a distorted source frame (Statement L, include/objcavit_hip.h).

The predict path reads every metre out of an ideal pinhole camera; a real lens bends the frame first.  A ``LensMap`` says, for every
pixel (u, v) of the RECTIFIED window, where in the source frame it comes from -- decided HERE, on the host, in float64, for any lens
model -- and quantises that coordinate to 1/256 pixel.  ``hip_ops.frame_remap_ingest`` / ``hip_ops.frames_remap_rgb24`` apply the map on
the device in integer arithmetic (csrc/frame_remap.hip), and ``Predictor(lens=...)`` / ``PipelinedPredictor(lens=...)`` ingest through it.

    map entry (X, Y) = floor(xs * 256 + 0.5), floor(ys * 256 + 0.5)      float64; pixel centres at integer indices; coordinates of the
    clamped to [-256, Ws * 256] x [-256, Hs * 256], NaN -> -256           WHOLE source frame

A clamped entry has all of its taps outside the frame (x0 = -1 with weight 0 on tap 0, or x0 = Ws): the pixel is black.  Builders:
``from_coordinates`` (maps made elsewhere), ``brown`` (rational Brown-Conrady, OpenCV's coefficient order), ``fisheye``
(Kannala-Brandt), ``identity`` (a plain crop).  Making a map needs no GPU.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

FRACTION_BITS = 8
ONE = 1 << FRACTION_BITS             # 256 map units per source pixel
OUTSIDE = -ONE                       # the sentinel of a coordinate left of / above the frame, and of NaN
_F64 = torch.float64


def quantise(xs: torch.Tensor, ys: torch.Tensor, source_size: Tuple[int, int]) -> torch.Tensor:
    """float64 source coordinates [..., Hw, Ww] -> the int32 entries [..., Hw, Ww, 2] of Statement L."""
    Hs, Ws = int(source_size[0]), int(source_size[1])
    out = []
    for c, n in ((xs, Ws), (ys, Hs)):
        q = torch.floor(c.to(_F64) * ONE + 0.5)
        q = torch.where(torch.isnan(q), torch.full_like(q, float(OUTSIDE)), q).clamp_(float(OUTSIDE), float(n * ONE))
        out.append(q.to(torch.int32))
    return torch.stack(out, -1).contiguous()


def taps_inside(map_i32: torch.Tensor, source_size: Tuple[int, int]) -> torch.Tensor:
    """uint8 [..., Hw, Ww]: 1 where all four taps of the entry lie inside the frame."""
    Hs, Ws = int(source_size[0]), int(source_size[1])
    x0, y0 = map_i32[..., 0] >> FRACTION_BITS, map_i32[..., 1] >> FRACTION_BITS
    return ((x0 >= 0) & (x0 + 1 < Ws) & (y0 >= 0) & (y0 + 1 < Hs)).to(torch.uint8)


def _k4(K, what: str) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) of a 4-vector or a 3 x 3 camera matrix."""
    k = torch.as_tensor(K, dtype=_F64).cpu()
    if tuple(k.shape) == (3, 3):
        k = torch.stack([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if tuple(k.shape) != (4,):
        raise ValueError(f"{what}: expected (fx, fy, cx, cy) or a 3 x 3 matrix, got {tuple(k.shape)}")
    fx, fy, cx, cy = (float(v) for v in k)
    if not (fx > 0.0 and fy > 0.0):
        raise ValueError(f"{what}: focal lengths must be positive, got {fx}, {fy}")
    return fx, fy, cx, cy


def _rays(K, source_size, window_size, new_K, R, who: str):
    """(x, y of the ideal ray through every rectified pixel -- NaN behind the camera --, the sizes, new_K)."""
    Hs, Ws = int(source_size[0]), int(source_size[1])
    Hw, Ww = (Hs, Ws) if window_size is None else (int(window_size[0]), int(window_size[1]))
    if min(Hs, Ws, Hw, Ww) < 1:
        raise ValueError(f"{who}: sizes must be >= 1, got source {Hs} x {Ws}, window {Hw} x {Ww}")
    k = _k4(K, f"{who}: K")
    nk = k if new_K is None else _k4(new_K, f"{who}: new_K")
    x = ((torch.arange(Ww, dtype=_F64) - nk[2]) / nk[0]).view(1, Ww).expand(Hw, Ww)
    y = ((torch.arange(Hw, dtype=_F64) - nk[3]) / nk[1]).view(Hw, 1).expand(Hw, Ww)
    if R is not None:
        r = torch.as_tensor(R, dtype=_F64).cpu()
        if tuple(r.shape) != (3, 3):
            raise ValueError(f"{who}: R must be 3 x 3, got {tuple(r.shape)}")
        # a ray of the rectified camera, back in the real camera's frame: R^T (x, y, 1)
        X = r[0, 0] * x + r[1, 0] * y + r[2, 0]
        Y = r[0, 1] * x + r[1, 1] * y + r[2, 1]
        Wd = r[0, 2] * x + r[1, 2] * y + r[2, 2]
        nan = torch.full_like(Wd, float("nan"))
        x, y = torch.where(Wd > 0.0, X / Wd, nan), torch.where(Wd > 0.0, Y / Wd, nan)
    return x, y, k, (Hs, Ws), nk


class LensMap:
    """The fixed-point map of one camera (M = 1) or of a batch's cameras (M = B).

    ``map``: int32 [M, Hw, Ww, 2] on the host (Statement L's entries); ``source_size`` = (Hs, Ws) of the distorted frames;
    ``window_size`` = (Hw, Ww) of the rectified window; ``new_K`` = (fx, fy, cx, cy) of the rectified window in ITS pixels (None when
    the builder was not told); ``valid``: uint8 [M, Hw, Ww], 1 where all four taps lie inside the frame (the other pixels blend in the
    black border -- the mask is handed out, nothing reads it).  ``on(device)``: the device copy, uploaded when first asked for and kept."""

    def __init__(self, map_i32: torch.Tensor, source_size: Tuple[int, int], new_K=None):
        if not isinstance(map_i32, torch.Tensor) or map_i32.dtype != torch.int32:
            raise TypeError("LensMap: the map is an int32 tensor (LensMap.from_coordinates quantises float coordinates)")
        if map_i32.dim() == 3:
            map_i32 = map_i32.unsqueeze(0)
        if map_i32.dim() != 4 or map_i32.shape[3] != 2 or min(map_i32.shape[:3]) < 1:
            raise ValueError(f"LensMap: expected int32 [M, Hw, Ww, 2] (or [Hw, Ww, 2]), got {tuple(map_i32.shape)}")
        Hs, Ws = int(source_size[0]), int(source_size[1])
        if Hs < 1 or Ws < 1:
            raise ValueError(f"LensMap: bad source size {tuple(source_size)}")
        self.map = map_i32.cpu().contiguous()
        self.source_size = (Hs, Ws)
        self.window_size = (int(self.map.shape[1]), int(self.map.shape[2]))
        self.new_K = None if new_K is None else _k4(new_K, "LensMap: new_K")
        self.valid = taps_inside(self.map, self.source_size)
        self._dev = {}

    @property
    def M(self) -> int:
        return int(self.map.shape[0])

    def __repr__(self) -> str:
        return f"LensMap(M={self.M}, source={self.source_size}, window={self.window_size}, new_K={self.new_K})"

    def on(self, device) -> torch.Tensor:
        """The map on ``device`` (a ROCm GPU): uploaded on the current stream when first asked for there, then kept -- it outlives every
        step that reads it."""
        from ._lib import HipLibraryError
        device = torch.device(device)
        if device.type != "cuda":
            raise HipLibraryError(f"LensMap.on: {device} is no ROCm GPU (there is no CPU fallback)")
        key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = self.map.to(device)
        return t

    # ------------------------------------------------------------------ builders
    @classmethod
    def from_coordinates(cls, xs, ys, source_size: Tuple[int, int], new_K=None) -> "LensMap":
        """Source coordinates from any model (e.g. maps exported from another library): ``xs`` / ``ys`` [Hw, Ww] or [M, Hw, Ww], the
        column / row in the source frame of every rectified pixel, pixel centres at integer indices.  Only the quantisation of
        Statement L happens here."""
        xs, ys = torch.as_tensor(xs).to(_F64).cpu(), torch.as_tensor(ys).to(_F64).cpu()
        if xs.shape != ys.shape or xs.dim() not in (2, 3):
            raise ValueError(f"LensMap.from_coordinates: xs / ys must share a shape [Hw, Ww] or [M, Hw, Ww], got {tuple(xs.shape)} / {tuple(ys.shape)}")
        return cls(quantise(xs, ys, source_size), source_size, new_K)

    @classmethod
    def identity(cls, source_size: Tuple[int, int], top: int = 0, left: int = 0, window_size: Optional[Tuple[int, int]] = None,
                 new_K=None) -> "LensMap":
        """The window at (top, left) as it is: X = 256 (left + u), Y = 256 (top + v)."""
        Hs, Ws = int(source_size[0]), int(source_size[1])
        Hw, Ww = (Hs - int(top), Ws - int(left)) if window_size is None else (int(window_size[0]), int(window_size[1]))
        if Hw < 1 or Ww < 1:
            raise ValueError(f"LensMap.identity: bad window {Hw} x {Ww}")
        xs = (torch.arange(Ww, dtype=_F64) + int(left)).view(1, Ww).expand(Hw, Ww)
        ys = (torch.arange(Hw, dtype=_F64) + int(top)).view(Hw, 1).expand(Hw, Ww)
        return cls(quantise(xs, ys, (Hs, Ws)), (Hs, Ws), new_K)

    @classmethod
    def brown(cls, K, dist: Sequence[float], source_size: Tuple[int, int], window_size: Optional[Tuple[int, int]] = None, new_K=None,
              R=None) -> "LensMap":
        """The rational Brown-Conrady model.  ``K``: (fx, fy, cx, cy) or 3 x 3, of the distorted frames; ``dist`` = (k1, k2, p1, p2[, k3[,
        k4, k5, k6]]); ``R``: an optional 3 x 3 rectifying rotation (real camera -> rectified camera); ``new_K``: the rectified window's
        camera (default ``K``); ``window_size`` (default the source size).  With (x, y) the ideal ray of rectified pixel (u, v)
        (x = (u - cx') / fx', y = (v - cy') / fy', turned by R^T) and r2 = x^2 + y^2:
            s = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
            xd = x s + 2 p1 x y + p2 (r2 + 2 x^2)        yd = y s + p1 (r2 + 2 y^2) + 2 p2 x y
            xs = fx xd + cx                              ys = fy yd + cy"""
        d = [float(v) for v in dist]
        if len(d) not in (4, 5, 8):
            raise ValueError(f"LensMap.brown: dist = (k1, k2, p1, p2[, k3[, k4, k5, k6]]), got {len(d)} coefficients")
        k1, k2, p1, p2, k3, k4, k5, k6 = d + [0.0] * (8 - len(d))
        x, y, (fx, fy, cx, cy), src, nk = _rays(K, source_size, window_size, new_K, R, "LensMap.brown")
        r2 = x * x + y * y
        s = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
        xd = x * s + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * s + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        return cls(quantise(fx * xd + cx, fy * yd + cy, src), src, nk)

    @classmethod
    def fisheye(cls, K, dist4: Sequence[float], source_size: Tuple[int, int], window_size: Optional[Tuple[int, int]] = None, new_K=None,
                R=None) -> "LensMap":
        """Kannala-Brandt.  Arguments as ``brown`` takes them, ``dist4`` = (k1, k2, k3, k4).  With r = sqrt(x^2 + y^2), theta = atan(r):
            theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)
            xs = fx (theta_d / r) x + cx        ys = fy (theta_d / r) y + cy        (r = 0: the principal point)"""
        d = [float(v) for v in dist4]
        if len(d) != 4:
            raise ValueError(f"LensMap.fisheye: dist4 = (k1, k2, k3, k4), got {len(d)} coefficients")
        x, y, (fx, fy, cx, cy), src, nk = _rays(K, source_size, window_size, new_K, R, "LensMap.fisheye")
        r = torch.sqrt(x * x + y * y)
        th = torch.atan(r)
        t2 = th * th
        thd = th * (1.0 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3]))))
        scale = torch.where(r > 0.0, thd / r, torch.ones_like(r))
        scale = torch.where(torch.isnan(r), r, scale)
        return cls(quantise(fx * scale * x + cx, fy * scale * y + cy, src), src, nk)


__all__ = ["LensMap", "quantise", "taps_inside", "FRACTION_BITS", "ONE", "OUTSIDE"]
