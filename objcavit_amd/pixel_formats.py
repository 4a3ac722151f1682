"""Pixel formats on ingest: the layouts decoders and capture APIs deliver, and Statement P, the YCbCr -> RGB
conversion of the 4:2:0 formats -- in integers, from five tables the HOST makes here in float64 and rounds once.  The kernels
(csrc/pixel_fetch.hpp) decide no coefficient, as they decide no normalisation constant (``predict.normalisation_table``) and no tap
(``hip_ops.resize_taps``).

    name              planes
    rgb24, bgr24      one, uint8 [B, Hs, Ws, 3]
    rgba32, bgra32    one, uint8 [B, Hs, Ws, 4], alpha ignored
    nv12              Y [B, Hs, Ws]; CbCr [B, ceil(Hs / 2), ceil(Ws / 2), 2]
    i420              Y [B, Hs, Ws]; Cb [B, ceil(Hs / 2), ceil(Ws / 2)]; Cr likewise

Statement P.  Kr, Kb of the matrix (bt601: 0.299, 0.114; bt709: 0.2126, 0.0722), Kg = 1 - Kr - Kb; y0, sy, sc of the range (limited:
16, 255 / 219, 255 / 224; full: 0, 1, 1); for v = 0 .. 255

    T0[v] = rint(2^16 sy (v - y0)) + 2^15
    T1[v] = rint(2^16 sc 2 (1 - Kr) (v - 128))                 Cr -> R
    T2[v] = rint(2^16 sc (-2 Kb (1 - Kb) / Kg) (v - 128))      Cb -> G
    T3[v] = rint(2^16 sc (-2 Kr (1 - Kr) / Kg) (v - 128))      Cr -> G
    T4[v] = rint(2^16 sc 2 (1 - Kb) (v - 128))                 Cb -> B
    R = clamp((T0[Y] + T1[Cr]) >> 16)   G = clamp((T0[Y] + T2[Cb] + T3[Cr]) >> 16)   B = clamp((T0[Y] + T4[Cb]) >> 16)

with ``>>`` the arithmetic shift and clamp to 0 .. 255.  Pixel (x, y) takes the chroma sample (x >> 1, y >> 1): replication.  Sited
(interpolated) chroma, 10-bit surfaces (P010) and 4:2:2 / 4:4:4 are not served.  Needs no GPU.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

# include/objcavit_hip.h: OCV_PIXFMT_*
FORMAT_IDS = {"rgb24": 0, "bgr24": 1, "rgba32": 2, "bgra32": 3, "nv12": 4, "i420": 5}
PLANAR = ("nv12", "i420")
_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
_RANGES = {"limited": (16.0, 255.0 / 219.0, 255.0 / 224.0), "full": (0.0, 1.0, 1.0)}


def yuv_tables(matrix: str = "bt601", range: str = "limited") -> torch.Tensor:
    """int32 [5, 256] on the host: T0 .. T4 of Statement P for ``matrix`` ("bt601" / "bt709") and ``range`` ("limited" / "full"),
    evaluated in float64 and rounded once (ties to even; no product here lands on a tie that matters: the tests hold every entry to an
    independent restatement)."""
    if matrix not in _MATRICES:
        raise ValueError(f"yuv_tables: matrix must be one of {sorted(_MATRICES)}, got {matrix!r}")
    if range not in _RANGES:
        raise ValueError(f"yuv_tables: range must be one of {sorted(_RANGES)}, got {range!r}")
    kr, kb = _MATRICES[matrix]
    kg = 1.0 - kr - kb
    y0, sy, sc = _RANGES[range]
    v = torch.arange(256, dtype=torch.float64)
    one = 65536.0
    rows = [torch.round(one * sy * (v - y0)) + 32768.0,
            torch.round(one * sc * (2.0 * (1.0 - kr)) * (v - 128.0)),
            torch.round(one * sc * (-2.0 * kb * (1.0 - kb) / kg) * (v - 128.0)),
            torch.round(one * sc * (-2.0 * kr * (1.0 - kr) / kg) * (v - 128.0)),
            torch.round(one * sc * (2.0 * (1.0 - kb)) * (v - 128.0))]
    return torch.stack(rows, 0).to(torch.int32)


class PixelFormat:
    """``PixelFormat(name, matrix="bt601", range="limited")``: a layout of the table above and, for the 4:2:0 formats, which tables
    Statement P uses (packed formats ignore ``matrix`` and ``range``).  Hashable; ``PixelFormat.of(x)`` takes a PixelFormat, a name or
    None (= rgb24)."""

    __slots__ = ("name", "matrix", "range")

    def __init__(self, name: str, matrix: str = "bt601", range: str = "limited"):
        if name not in FORMAT_IDS:
            raise ValueError(f"PixelFormat: name must be one of {sorted(FORMAT_IDS)}, got {name!r}")
        if matrix not in _MATRICES or range not in _RANGES:
            raise ValueError(f"PixelFormat: matrix must be one of {sorted(_MATRICES)} and range one of {sorted(_RANGES)}, got "
                             f"{matrix!r}, {range!r}")
        object.__setattr__(self, "name", name)
        object.__setattr__(self, "matrix", matrix)
        object.__setattr__(self, "range", range)

    def __setattr__(self, key, value):
        raise AttributeError("PixelFormat is immutable")

    @staticmethod
    def of(fmt: Union["PixelFormat", str, None]) -> "PixelFormat":
        if fmt is None:
            return PixelFormat("rgb24")
        return fmt if isinstance(fmt, PixelFormat) else PixelFormat(fmt)

    @property
    def id(self) -> int:
        return FORMAT_IDS[self.name]

    @property
    def planar(self) -> bool:
        return self.name in PLANAR

    @property
    def channels(self) -> int:
        """Bytes per pixel of a packed format's one plane (0 for the 4:2:0 formats)."""
        return 0 if self.planar else (4 if self.name in ("rgba32", "bgra32") else 3)

    def tables(self) -> torch.Tensor:
        return yuv_tables(self.matrix, self.range)

    def _key(self):
        return (self.name, self.matrix, self.range) if self.planar else (self.name,)

    def __eq__(self, other):
        return isinstance(other, PixelFormat) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"PixelFormat({self.name!r}, {self.matrix!r}, {self.range!r})" if self.planar else f"PixelFormat({self.name!r})"


def chroma_size(Hs: int, Ws: int) -> Tuple[int, int]:
    """(rows, columns) of the chroma samples of an Hs x Ws 4:2:0 frame: ceil(Hs / 2) x ceil(Ws / 2)."""
    return (int(Hs) + 1) // 2, (int(Ws) + 1) // 2


class PlanarFrames:
    """``PlanarFrames(name, planes, Hs, Ws)``: a batch of 4:2:0 frames as its planes -- uint8 tensors on one device, each dense within
    a row; rows and frames may be strided and the planes may be views into one allocation, at any alignment.

        nv12    planes = (Y [B, Hs, Ws], CbCr [B, Hc, Wc, 2])           Hc, Wc = ceil(Hs / 2), ceil(Ws / 2)
        i420    planes = (Y [B, Hs, Ws], Cb [B, Hc, Wc], Cr [B, Hc, Wc])

    A chroma plane may be larger than Hc x Wc (it is read up to there).  Planes without the batch axis are one frame (B = 1).
    ``shape`` = (B, Hs, Ws) and ``device`` are what the predict path reads of a frame batch; ``planes`` is the tuple of tensors (what a
    pipeline holds and marks with ``record_stream``)."""

    def __init__(self, name: str, planes: Sequence[torch.Tensor], Hs: int, Ws: int):
        if name not in PLANAR:
            raise ValueError(f"PlanarFrames: name must be one of {PLANAR}, got {name!r}")
        planes = tuple(planes)
        want = 2 if name == "nv12" else 3
        if len(planes) != want:
            raise ValueError(f"PlanarFrames: {name} has {want} planes, got {len(planes)}")
        Hs, Ws = int(Hs), int(Ws)
        if Hs < 1 or Ws < 1:
            raise ValueError(f"PlanarFrames: bad frame size {Hs} x {Ws}")
        Hc, Wc = chroma_size(Hs, Ws)
        dims = [3] + ([4] if name == "nv12" else [3, 3])
        fixed = []
        for i, (p, d) in enumerate(zip(planes, dims)):
            if not isinstance(p, torch.Tensor) or p.dtype != torch.uint8:
                raise TypeError(f"PlanarFrames: plane {i} must be a uint8 tensor")
            if p.dim() == d - 1:
                p = p.unsqueeze(0)
            if p.dim() != d:
                raise ValueError(f"PlanarFrames: plane {i} of {name} has {d - 1} axes (+ the batch axis), got {tuple(p.shape)}")
            fixed.append(p)
        B = int(fixed[0].shape[0])
        if B < 1:
            raise ValueError("PlanarFrames: empty batch")
        for i, p in enumerate(fixed):
            rows, cols = (Hs, Ws) if i == 0 else (Hc, Wc)
            if int(p.shape[0]) != B:
                raise ValueError(f"PlanarFrames: plane {i} holds {int(p.shape[0])} frame(s), plane 0 holds {B}")
            if p.device != fixed[0].device:
                raise ValueError(f"PlanarFrames: plane {i} is on {p.device}, plane 0 on {fixed[0].device}")
            if i == 0 and (int(p.shape[1]), int(p.shape[2])) != (Hs, Ws):
                raise ValueError(f"PlanarFrames: the Y plane must be [B, {Hs}, {Ws}], got {tuple(p.shape)}")
            if int(p.shape[1]) < rows or int(p.shape[2]) < cols:
                raise ValueError(f"PlanarFrames: plane {i} must hold at least {rows} x {cols} samples, got {tuple(p.shape)}")
            if p.dim() == 4 and int(p.shape[3]) != 2:
                raise ValueError(f"PlanarFrames: the CbCr plane must be [B, {Hc}, {Wc}, 2], got {tuple(p.shape)}")
            st = p.stride()
            inner = 2 if p.dim() == 4 else 1
            if (p.dim() == 4 and st[3] != 1) or (int(p.shape[2]) > 1 and st[2] != inner):
                raise ValueError(f"PlanarFrames: the samples of a row of plane {i} must be dense (strides {st})")
            row_bytes = cols * inner
            if (int(p.shape[1]) > 1 and st[1] < row_bytes) or (B > 1 and st[0] < (rows - 1) * (st[1] if int(p.shape[1]) > 1 else row_bytes) + row_bytes):
                raise ValueError(f"PlanarFrames: overlapping rows / frames in plane {i} (strides {st})")
        self.name, self.planes, self.Hs, self.Ws = name, tuple(fixed), Hs, Ws

    @classmethod
    def from_buffer(cls, buf: torch.Tensor, name: str, Hs: int, Ws: int) -> "PlanarFrames":
        """The usual contiguous single-buffer form: ``buf`` uint8 [B, Hs * 3 / 2, Ws] (or one frame [Hs * 3 / 2, Ws]) whose frames
        are dense -- the Y plane, then the CbCr rows (nv12) or the Cb plane and the Cr plane (i420).  Even Hs and Ws.  The planes are
        views: nothing is copied."""
        Hs, Ws = int(Hs), int(Ws)
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8:
            raise TypeError("PlanarFrames.from_buffer: expected a uint8 tensor")
        if buf.dim() == 2:
            buf = buf.unsqueeze(0)
        if Hs < 2 or Ws < 2 or Hs % 2 or Ws % 2:
            raise ValueError(f"PlanarFrames.from_buffer: Hs and Ws must be even, got {Hs} x {Ws} (pass explicit planes for odd sizes)")
        if buf.dim() != 3 or tuple(buf.shape[1:]) != (Hs * 3 // 2, Ws) or buf.stride(2) != 1 or buf.stride(1) != Ws:
            raise ValueError(f"PlanarFrames.from_buffer: expected [B, {Hs * 3 // 2}, {Ws}] with dense frames, got {tuple(buf.shape)} "
                             f"(strides {buf.stride()})")
        B, fs, off = int(buf.shape[0]), int(buf.stride(0)), int(buf.storage_offset())
        Hc, Wc = Hs // 2, Ws // 2
        y = buf[:, :Hs, :]
        if name == "nv12":
            planes = (y, torch.as_strided(buf, (B, Hc, Wc, 2), (fs, Ws, 2, 1), off + Hs * Ws))
        elif name == "i420":
            planes = (y, torch.as_strided(buf, (B, Hc, Wc), (fs, Wc, 1), off + Hs * Ws),
                      torch.as_strided(buf, (B, Hc, Wc), (fs, Wc, 1), off + Hs * Ws + Hc * Wc))
        else:
            raise ValueError(f"PlanarFrames.from_buffer: name must be one of {PLANAR}, got {name!r}")
        return cls(name, planes, Hs, Ws)

    @property
    def shape(self) -> Tuple[int, int, int]:
        return (int(self.planes[0].shape[0]), self.Hs, self.Ws)

    @property
    def device(self) -> torch.device:
        return self.planes[0].device

    def __len__(self) -> int:
        return self.shape[0]

    def __getitem__(self, index) -> "PlanarFrames":
        """A sub-batch (a slice, or an int -> one frame, still batched)."""
        if isinstance(index, int):
            index = slice(index, index + 1) if index != -1 else slice(-1, None)
        if not isinstance(index, slice):
            raise TypeError("PlanarFrames: index with an int or a slice of the batch axis")
        return PlanarFrames(self.name, tuple(p[index] for p in self.planes), self.Hs, self.Ws)

    def to(self, device) -> "PlanarFrames":
        """The planes copied to ``device`` (each on its own: views into one buffer become separate tensors)."""
        return PlanarFrames(self.name, tuple(p.to(device) for p in self.planes), self.Hs, self.Ws)

    def __repr__(self):
        return f"PlanarFrames({self.name!r}, B={self.shape[0]}, {self.Hs} x {self.Ws}, device={self.device})"


def plane_strides(p: torch.Tensor) -> Tuple[int, int]:
    """(frame stride, row stride) in bytes of one uint8 plane [B, rows, cols(, k)] as the C entry points take them: a one-row plane's row
    stride and a one-frame batch's frame stride are the dense ones."""
    rows = int(p.shape[1])
    row_bytes = int(p.shape[2]) * (int(p.shape[3]) if p.dim() == 4 else 1)
    row = int(p.stride(1)) if rows > 1 else row_bytes
    frame = int(p.stride(0)) if int(p.shape[0]) > 1 else rows * row
    return frame, row


__all__ = ["FORMAT_IDS", "PLANAR", "yuv_tables", "PixelFormat", "PlanarFrames", "chroma_size", "plane_strides"]
