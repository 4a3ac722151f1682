"""hip_ops frames: the two ends of the predict path -- decoded uint8 / uint16 frames in (csrc/frame_ingest.hip; a window of any size
resized to the model's on the way in: csrc/frame_resize.hip), full-resolution depth
maps out (csrc/depth_finalize.hip), and what is read out of the final map behind them: per-box statistics (csrc/object_depth.hip), the
point cloud (csrc/point_cloud.hip), the surface normals (csrc/surface_normals.hip), the bird's-eye occupancy grid (csrc/ground_grid.hip) and, against ground truth, the depth error per box and per region (csrc/object_metrics.hip).  Same rules as every wrapper: operands are checked on the host, CPU tensors raise
``HipLibraryError``, one launch on the current stream, ``out=`` writes straight into a buffer the caller owns (a captured graph's
static input)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import check
from ..pixel_formats import PixelFormat, PlanarFrames, plane_strides
from ._core import _ptr, _req, _stream, timed


def _frames_view(frames: torch.Tensor, name: str, dtype, channels: int) -> Tuple[int, int, int, int, int]:
    """(B, Hs, Ws, frame stride, row stride in elements) of a decoded-frame tensor [B, Hs, Ws(, 3)] whose pixels are dense within a row;
    rows and frames may be strided (a view into a larger buffer)."""
    _req(frames, name, dtype, contiguous=False)
    want = 4 if channels == 3 else 3
    if frames.dim() != want or (channels == 3 and frames.shape[3] != 3):
        raise ValueError(f"{name}: expected {'[B, Hs, Ws, 3] (HWC)' if channels == 3 else '[B, Hs, Ws]'}, got {tuple(frames.shape)}")
    B, Hs, Ws = (int(s) for s in frames.shape[:3])
    if B < 1 or Hs < 1 or Ws < 1:
        raise ValueError(f"{name}: empty frames {tuple(frames.shape)}")
    st = frames.stride()
    if (channels == 3 and (st[3] != 1 or st[2] != 3)) or (channels == 1 and st[2] != 1):
        raise ValueError(f"{name}: the pixels of a row must be dense (strides {st})")
    row = int(st[1]) if Hs > 1 else Ws * channels
    frame = int(st[0]) if B > 1 else Hs * row
    if row < Ws * channels or frame < (Hs - 1) * row + Ws * channels:
        raise ValueError(f"{name}: overlapping rows / frames (strides {st})")
    return B, Hs, Ws, frame, row


def _window(Hs: int, Ws: int, top: int, left: int, size: Optional[Tuple[int, int]], name: str) -> Tuple[int, int]:
    H, W = (Hs - top, Ws - left) if size is None else (int(size[0]), int(size[1]))
    if top < 0 or left < 0 or H < 1 or W < 1 or top + H > Hs or left + W > Ws:
        raise ValueError(f"{name}: crop window {H} x {W} at ({top}, {left}) does not fit a {Hs} x {Ws} frame")
    return H, W


def _out_slice(out: Optional[torch.Tensor], shape: Tuple[int, ...], dtype, device, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _req(out, f"{name}: out", dtype)
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{name}: out must be {tuple(shape)}, got {tuple(out.shape)}")
    return out


def frame_ingest(frames_u8: torch.Tensor, table: torch.Tensor, top: int = 0, left: int = 0, size: Optional[Tuple[int, int]] = None,
                 mirror_too: bool = False, out: Optional[torch.Tensor] = None, out_index: int = 0) -> torch.Tensor:
    """uint8 frames [B, Hs, Ws, 3] (rows / frames may be strided) -> fp32 NCHW: the ``size`` = (H, W) window at (top, left), every
    channel value looked up in ``table`` (fp32 [3, 256] on the device: ``predict.normalisation_table``).  ``mirror_too``: the result
    has a second half, the first flipped along W -- the [batch | mirrored batch] input of the validation step's joint forward.
    ``out``: write into this tensor ([N, 3, H, W], N >= B, or N = 2 * (images) with ``mirror_too``) at images ``out_index`` ..
    ``out_index + B`` (and N / 2 + the same for the mirrors): a captured graph's static input, or one batch tensor filled by one launch
    per differently sized frame.  -> the tensor written."""
    lib = _lib.load()
    B, Hs, Ws, frame, row = _frames_view(frames_u8, "frames_u8", torch.uint8, 3)
    _req(table, "table")
    if tuple(table.shape) != (3, 256):
        raise ValueError(f"frame_ingest: table must be [3, 256], got {tuple(table.shape)}")
    H, W = _window(Hs, Ws, int(top), int(left), size, "frame_ingest")
    if out is None:
        out = torch.empty((2 * B if mirror_too else B, 3, H, W), dtype=torch.float32, device=frames_u8.device)
        out_index = 0
    else:
        _req(out, "frame_ingest: out")
        if out.dim() != 4 or tuple(out.shape[1:]) != (3, H, W):
            raise ValueError(f"frame_ingest: out must be [N, 3, {H}, {W}], got {tuple(out.shape)}")
    N = int(out.shape[0])
    half = N // 2 if mirror_too else N
    if (mirror_too and N % 2) or out_index < 0 or out_index + B > half:
        raise ValueError(f"frame_ingest: {B} image(s) at index {out_index} do not fit out {tuple(out.shape)}"
                         f"{' (first half: the second takes the mirrors)' if mirror_too else ''}")
    plane = 3 * H * W
    with timed("frame_ingest"):
        check(lib.ocv_frame_ingest_fwd(frames_u8.data_ptr(), frame, row, Hs, Ws, int(top), int(left), table.data_ptr(),
                                       out.data_ptr() + 4 * plane * int(out_index), B, H, W, 1 if mirror_too else 0, half * plane,
                                       _stream()), "ocv_frame_ingest_fwd")
    return out


FRAME_RESIZE_MAX_RATIO = 8        # include/objcavit_hip.h: OCV_FRAME_RESIZE_MAX_RATIO, source pixels per output pixel along an axis
_TAPS = {}                        # (device type, index, Hw, Ww, H, W) -> the device copy of the two tap tables
_TAPS_KEPT = 64                   # sizes kept: a source of ever-changing window sizes must not grow the cache without bound


def resize_taps(n_in: int, n_out: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The tap table of one axis of the antialiased resize ``n_in -> n_out`` (the separable triangle filter with half-pixel centres:
    torch's ``interpolate(mode="bilinear", antialias=True, align_corners=False)`` in float64; enlarging, plain bilinear) ->
    (start int32 [n_out], weight fp32 [n_out, K]) on the HOST.  All in float64: s = n_in / n_out, support = max(s, 1); output i has its
    centre at c = s (i + 0.5) and the taps j = lo .. hi - 1 with lo = max(0, int(c - support + 0.5)), hi = min(n_in, int(c + support +
    0.5)) (int truncates) and w_j = max(0, 1 - |(j - c + 0.5) / support|) divided by their sum; the weights are rounded to fp32 ONCE.
    K is the largest tap count; shorter rows are padded with weight 0.  Where a tap falls is decided here and nowhere else: torch's own
    fp32 path decides it in fp32 and puts a tap on the other side at ratios just above 1 (375 -> 352: 4e-4 off).  Needs no GPU."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_taps: sizes must be >= 1, got {n_in} -> {n_out}")
    s = n_in / n_out
    support = max(s, 1.0)
    inv = 1.0 / support
    c = s * (torch.arange(n_out, dtype=torch.float64) + 0.5)
    lo = (c - support + 0.5).trunc().clamp_(min=0).to(torch.int64)
    hi = (c + support + 0.5).trunc().clamp_(max=n_in).to(torch.int64)
    K = int((hi - lo).max())
    j = lo.view(-1, 1) + torch.arange(K, dtype=torch.int64).view(1, -1)
    w = (1.0 - ((j.to(torch.float64) - c.view(-1, 1) + 0.5) * inv).abs()).clamp_(min=0.0)
    w = torch.where(j < hi.view(-1, 1), w, torch.zeros((), dtype=torch.float64))
    w = w / w.sum(1, keepdim=True)
    return lo.to(torch.int32), w.to(torch.float32)


def frame_resize_supported(Hw: int, Ww: int, H: int, W: int) -> bool:
    """Whether ``frame_resize_ingest`` takes an Hw x Ww window to H x W: it shrinks by at most ``FRAME_RESIZE_MAX_RATIO`` along either
    axis (any enlargement is served).  Asked of the library (ocv_frame_resize_supported), no launch, no GPU."""
    return bool(_lib.load().ocv_frame_resize_supported(int(Hw), int(Ww), int(H), int(W)))


def frame_resize_taps(device, Hw: int, Ww: int, H: int, W: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ystart, yweight, xstart, xweight) of ``Hw x Ww -> H x W`` on ``device``: ``resize_taps`` of both axes, uploaded on the current
    stream when the size is first seen there and kept (the ``taps`` argument of ``frame_resize_ingest``)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HipLibraryError(f"frame_resize_taps: {device} is no ROCm GPU (there is no CPU fallback)")
    index = torch.cuda.current_device() if device.index is None else device.index
    key = (device.type, index, int(Hw), int(Ww), int(H), int(W))
    taps = _TAPS.get(key)
    if taps is None:
        if len(_TAPS) >= _TAPS_KEPT:
            _TAPS.clear()
        taps = _TAPS[key] = tuple(t.to(device) for t in resize_taps(Hw, H) + resize_taps(Ww, W))
    return taps


def frame_resize_ingest(frames_u8: torch.Tensor, table: torch.Tensor, size: Tuple[int, int], top: int = 0, left: int = 0,
                        window: Optional[Tuple[int, int]] = None, mirror_too: bool = False, out: Optional[torch.Tensor] = None,
                        out_index: int = 0, taps: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
    """``frame_ingest`` for a window of any size: the ``window`` = (Hw, Ww) pixels at (top, left) of uint8 frames [B, Hs, Ws, 3]
    (default: the rest of the frame) -> fp32 NCHW at ``size`` = (H, W), the model's, through the antialiased resize of ``resize_taps``
    applied to the ``table`` values (already normalised).  ``mirror_too``, ``out``, ``out_index``: as ``frame_ingest`` takes them; the
    mirrored half holds the same values flipped along W.  ``taps``: ``frame_resize_taps``' four device tensors for this window and size
    (default: made on first use and cached per device and size).  A window that shrinks by more than ``FRAME_RESIZE_MAX_RATIO`` along an
    axis raises ``ValueError`` before any launch.  One launch (ocv_frame_resize_ingest) on the current stream; within (Ky + Kx + 4) 2^-24
    max|table| of the float64 statement; a window of ``size`` is bit-equal to ``frame_ingest``.  -> the tensor written."""
    lib = _lib.load()
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise ValueError(f"frame_resize_ingest: bad output size {tuple(size)}")
    if isinstance(frames_u8, torch.Tensor) and frames_u8.dim() == 4:          # the ratio is judged first: it needs no device
        Hw, Ww = _window(int(frames_u8.shape[1]), int(frames_u8.shape[2]), int(top), int(left), window, "frame_resize_ingest")
        if not frame_resize_supported(Hw, Ww, H, W):
            raise ValueError(f"frame_resize_ingest: a {Hw} x {Ww} window to {H} x {W} shrinks by more than {FRAME_RESIZE_MAX_RATIO} "
                             "along an axis, the most one launch takes (the filter is never truncated): resize in two steps")
    B, Hs, Ws, frame, row = _frames_view(frames_u8, "frames_u8", torch.uint8, 3)
    _req(table, "table")
    if tuple(table.shape) != (3, 256):
        raise ValueError(f"frame_resize_ingest: table must be [3, 256], got {tuple(table.shape)}")
    Hw, Ww = _window(Hs, Ws, int(top), int(left), window, "frame_resize_ingest")
    if taps is None:
        taps = frame_resize_taps(frames_u8.device, Hw, Ww, H, W)
    if len(taps) != 4:
        raise ValueError("frame_resize_ingest: taps = (ystart, yweight, xstart, xweight)")
    ys, yw, xs, xw = taps
    for name, st, wt, n in (("y", ys, yw, H), ("x", xs, xw, W)):
        _req(st, f"taps: {name}start", torch.int32)
        _req(wt, f"taps: {name}weight")
        if tuple(st.shape) != (n,) or wt.dim() != 2 or wt.shape[0] != n or wt.shape[1] < 1:
            raise ValueError(f"frame_resize_ingest: taps of the {name} axis must be int32 [{n}] and fp32 [{n}, K], got "
                             f"{tuple(st.shape)} / {tuple(wt.shape)}")
    if out is None:
        out = torch.empty((2 * B if mirror_too else B, 3, H, W), dtype=torch.float32, device=frames_u8.device)
        out_index = 0
    else:
        _req(out, "frame_resize_ingest: out")
        if out.dim() != 4 or tuple(out.shape[1:]) != (3, H, W):
            raise ValueError(f"frame_resize_ingest: out must be [N, 3, {H}, {W}], got {tuple(out.shape)}")
    N = int(out.shape[0])
    half = N // 2 if mirror_too else N
    if (mirror_too and N % 2) or out_index < 0 or out_index + B > half:
        raise ValueError(f"frame_resize_ingest: {B} image(s) at index {out_index} do not fit out {tuple(out.shape)}"
                         f"{' (first half: the second takes the mirrors)' if mirror_too else ''}")
    plane = 3 * H * W
    with timed("frame_resize_ingest"):
        check(lib.ocv_frame_resize_ingest(frames_u8.data_ptr(), frame, row, Hs, Ws, int(top), int(left), Hw, Ww, table.data_ptr(),
                                          ys.data_ptr(), yw.data_ptr(), int(yw.shape[1]), xs.data_ptr(), xw.data_ptr(), int(xw.shape[1]),
                                          out.data_ptr() + 4 * plane * int(out_index), B, H, W, 1 if mirror_too else 0, half * plane,
                                          _stream()), "ocv_frame_resize_ingest")
    return out


_YUV = {}                         # (device type, index, matrix, range) -> the device copy of ``pixel_formats.yuv_tables``


def frame_yuv_tables(device, pixel_format) -> Optional[torch.Tensor]:
    """The int32 [5, 256] tables of Statement P of a 4:2:0 ``pixel_format`` on ``device`` (``pixel_formats.yuv_tables``), uploaded on
    the current stream when first used there and kept; None for a packed format."""
    fmt = PixelFormat.of(pixel_format)
    if not fmt.planar:
        return None
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HipLibraryError(f"frame_yuv_tables: {device} is no ROCm GPU (there is no CPU fallback)")
    index = torch.cuda.current_device() if device.index is None else device.index
    key = (device.type, index, fmt.matrix, fmt.range)
    t = _YUV.get(key)
    if t is None:
        t = _YUV[key] = fmt.tables().to(device)
    return t


def _yuv_on(device, fmt: PixelFormat, given: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if not fmt.planar:
        return None
    if given is None:
        return frame_yuv_tables(device, fmt)
    _req(given, "yuv_tables", torch.int32)
    if tuple(given.shape) != (5, 256):
        raise ValueError(f"yuv_tables must be int32 [5, 256], got {tuple(given.shape)}")
    return given


def _source(frames, fmt: PixelFormat, who: str):
    """(B, Hs, Ws, device, the nine plane arguments of a ``*_format`` entry point) of a frame batch in ``fmt``: a ``PlanarFrames`` for the
    4:2:0 formats, a uint8 tensor [B, Hs, Ws, 3 | 4] (rows / frames may be strided) for the packed ones."""
    if fmt.planar:
        if not isinstance(frames, PlanarFrames) or frames.name != fmt.name:
            raise TypeError(f"{who}: {fmt.name} frames are a PlanarFrames({fmt.name!r}, ...), got "
                            f"{frames if isinstance(frames, PlanarFrames) else type(frames).__name__}")
        args = []
        for i, p in enumerate(frames.planes):
            _req(p, f"{who}: plane {i}", torch.uint8, contiguous=False)
            args += [p.data_ptr(), *plane_strides(p)]
        args += [None, 0, 0] * (3 - len(frames.planes))
        B, Hs, Ws = frames.shape
        return B, Hs, Ws, frames.device, args
    ch = fmt.channels
    _req(frames, f"{who}: frames", torch.uint8, contiguous=False)
    if frames.dim() != 4 or frames.shape[3] != ch:
        raise ValueError(f"{who}: {fmt.name} frames are [B, Hs, Ws, {ch}], got {tuple(frames.shape)}")
    B, Hs, Ws = (int(s) for s in frames.shape[:3])
    if B < 1 or Hs < 1 or Ws < 1:
        raise ValueError(f"{who}: empty frames {tuple(frames.shape)}")
    st = frames.stride()
    if st[3] != 1 or st[2] != ch:
        raise ValueError(f"{who}: the pixels of a row must be dense (strides {st})")
    row = int(st[1]) if Hs > 1 else Ws * ch
    frame = int(st[0]) if B > 1 else Hs * row
    if row < Ws * ch or frame < (Hs - 1) * row + Ws * ch:
        raise ValueError(f"{who}: overlapping rows / frames (strides {st})")
    return B, Hs, Ws, frames.device, [frames.data_ptr(), frame, row, None, 0, 0, None, 0, 0]


def _ingest_out(out, out_index: int, B: int, H: int, W: int, mirror_too: bool, device, who: str):
    """The ``out`` / ``out_index`` rules of ``frame_ingest`` -> (out, out_index, images per half)."""
    if out is None:
        out = torch.empty((2 * B if mirror_too else B, 3, H, W), dtype=torch.float32, device=device)
        out_index = 0
    else:
        _req(out, f"{who}: out")
        if out.dim() != 4 or tuple(out.shape[1:]) != (3, H, W):
            raise ValueError(f"{who}: out must be [N, 3, {H}, {W}], got {tuple(out.shape)}")
    N = int(out.shape[0])
    half = N // 2 if mirror_too else N
    if (mirror_too and N % 2) or out_index < 0 or out_index + B > half:
        raise ValueError(f"{who}: {B} image(s) at index {out_index} do not fit out {tuple(out.shape)}"
                         f"{' (first half: the second takes the mirrors)' if mirror_too else ''}")
    return out, int(out_index), half


def frame_ingest_format(frames, table: torch.Tensor, pixel_format, top: int = 0, left: int = 0, size: Optional[Tuple[int, int]] = None,
                        mirror_too: bool = False, out: Optional[torch.Tensor] = None, out_index: int = 0,
                        yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``frame_ingest`` for frames of any ``pixel_format`` (a ``PixelFormat`` or a name): a uint8 tensor [B, Hs, Ws, 3 | 4] for the
    packed formats, a ``PlanarFrames`` for nv12 / i420, whose pixels become R, G, B bytes by Statement P (``pixel_formats``) inside the
    launch.  Every other argument as ``frame_ingest`` takes it; bit-equal to ``frame_ingest`` on the converted frames.  One launch
    (ocv_frame_ingest_format) on the current stream; a 4:2:0 format's tables are uploaded on it when first used
    (``frame_yuv_tables``), or passed as ``yuv_tables`` (the int32 [5, 256] device tensor of the format's matrix and range)."""
    lib = _lib.load()
    fmt = PixelFormat.of(pixel_format)
    B, Hs, Ws, device, planes = _source(frames, fmt, "frame_ingest_format")
    _req(table, "table")
    if tuple(table.shape) != (3, 256):
        raise ValueError(f"frame_ingest_format: table must be [3, 256], got {tuple(table.shape)}")
    H, W = _window(Hs, Ws, int(top), int(left), size, "frame_ingest_format")
    out, out_index, half = _ingest_out(out, out_index, B, H, W, mirror_too, device, "frame_ingest_format")
    yuv = _yuv_on(device, fmt, yuv_tables)
    plane = 3 * H * W
    with timed("frame_ingest_format"):
        check(lib.ocv_frame_ingest_format(fmt.id, *planes, _ptr(yuv), Hs, Ws, int(top), int(left), table.data_ptr(),
                                          out.data_ptr() + 4 * plane * out_index, B, H, W, 1 if mirror_too else 0, half * plane,
                                          _stream()), "ocv_frame_ingest_format")
    return out


def frame_resize_ingest_format(frames, table: torch.Tensor, size: Tuple[int, int], pixel_format, top: int = 0, left: int = 0,
                               window: Optional[Tuple[int, int]] = None, mirror_too: bool = False, out: Optional[torch.Tensor] = None,
                               out_index: int = 0, taps: Optional[Sequence[torch.Tensor]] = None,
                               yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``frame_resize_ingest`` for frames of any ``pixel_format`` (as ``frame_ingest_format`` takes them): the conversion happens
    while the window's pixels are staged, the two tap passes are ``frame_resize_ingest``'s -- bit-equal to it on the converted frames.
    One launch (ocv_frame_resize_ingest_format) on the current stream."""
    lib = _lib.load()
    fmt = PixelFormat.of(pixel_format)
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise ValueError(f"frame_resize_ingest_format: bad output size {tuple(size)}")
    B, Hs, Ws, device, planes = _source(frames, fmt, "frame_resize_ingest_format")
    Hw, Ww = _window(Hs, Ws, int(top), int(left), window, "frame_resize_ingest_format")
    if not frame_resize_supported(Hw, Ww, H, W):
        raise ValueError(f"frame_resize_ingest_format: a {Hw} x {Ww} window to {H} x {W} shrinks by more than {FRAME_RESIZE_MAX_RATIO} "
                         "along an axis, the most one launch takes (the filter is never truncated): resize in two steps")
    _req(table, "table")
    if tuple(table.shape) != (3, 256):
        raise ValueError(f"frame_resize_ingest_format: table must be [3, 256], got {tuple(table.shape)}")
    if taps is None:
        taps = frame_resize_taps(device, Hw, Ww, H, W)
    if len(taps) != 4:
        raise ValueError("frame_resize_ingest_format: taps = (ystart, yweight, xstart, xweight)")
    ys, yw, xs, xw = taps
    for name, st, wt, n in (("y", ys, yw, H), ("x", xs, xw, W)):
        _req(st, f"taps: {name}start", torch.int32)
        _req(wt, f"taps: {name}weight")
        if tuple(st.shape) != (n,) or wt.dim() != 2 or wt.shape[0] != n or wt.shape[1] < 1:
            raise ValueError(f"frame_resize_ingest_format: taps of the {name} axis must be int32 [{n}] and fp32 [{n}, K], got "
                             f"{tuple(st.shape)} / {tuple(wt.shape)}")
    out, out_index, half = _ingest_out(out, out_index, B, H, W, mirror_too, device, "frame_resize_ingest_format")
    yuv = _yuv_on(device, fmt, yuv_tables)
    plane = 3 * H * W
    with timed("frame_resize_ingest_format"):
        check(lib.ocv_frame_resize_ingest_format(fmt.id, *planes, _ptr(yuv), Hs, Ws, int(top), int(left), Hw, Ww, table.data_ptr(),
                                                 ys.data_ptr(), yw.data_ptr(), int(yw.shape[1]), xs.data_ptr(), xw.data_ptr(),
                                                 int(xw.shape[1]), out.data_ptr() + 4 * plane * out_index, B, H, W,
                                                 1 if mirror_too else 0, half * plane, _stream()), "ocv_frame_resize_ingest_format")
    return out


def frames_to_rgb24(frames, pixel_format, top: int = 0, left: int = 0, size: Optional[Tuple[int, int]] = None,
                    out: Optional[torch.Tensor] = None, yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ``size`` = (Hw, Ww) window at (top, left) (default: the rest of the frame) of frames of any ``pixel_format`` (as
    ``frame_ingest_format`` takes them) -> packed RGB uint8 [B, Hw, Ww, 3]: Statement P for the 4:2:0 formats, the bytes re-ordered for
    the packed ones.  ``out``: a contiguous uint8 [B, Hw, Ww, 3] to write.  One launch (ocv_frames_to_rgb24) on the current stream,
    every output byte written."""
    lib = _lib.load()
    fmt = PixelFormat.of(pixel_format)
    B, Hs, Ws, device, planes = _source(frames, fmt, "frames_to_rgb24")
    Hw, Ww = _window(Hs, Ws, int(top), int(left), size, "frames_to_rgb24")
    out = _out_slice(out, (B, Hw, Ww, 3), torch.uint8, device, "frames_to_rgb24")
    yuv = _yuv_on(device, fmt, yuv_tables)
    with timed("frames_to_rgb24"):
        check(lib.ocv_frames_to_rgb24(fmt.id, *planes, _ptr(yuv), Hs, Ws, int(top), int(left), out.data_ptr(), B, Hw, Ww, _stream()),
              "ocv_frames_to_rgb24")
    return out


def depth_ingest(depth_u16: torch.Tensor, factor: float, top: int = 0, left: int = 0, size: Optional[Tuple[int, int]] = None,
                 out: Optional[torch.Tensor] = None, out_index: int = 0) -> torch.Tensor:
    """uint16 ground-truth depth [B, Hs, Ws] (as in the 16-bit PNGs) -> fp32 metres [B, 1, H, W] = float(v) / ``factor`` over the same
    window arguments as ``frame_ingest`` (modules/Preprocess.py:45-65; 1000 for NYU, 256 for KITTI)."""
    lib = _lib.load()
    B, Hs, Ws, frame, row = _frames_view(depth_u16, "depth_u16", torch.uint16, 1)
    H, W = _window(Hs, Ws, int(top), int(left), size, "depth_ingest")
    if not float(factor) > 0.0:
        raise ValueError("depth_ingest: factor must be positive")
    if out is None:
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=depth_u16.device)
        out_index = 0
    else:
        _req(out, "depth_ingest: out")
        if out.dim() != 4 or tuple(out.shape[1:]) != (1, H, W) or out_index < 0 or out_index + B > out.shape[0]:
            raise ValueError(f"depth_ingest: out must be [N >= {out_index + B}, 1, {H}, {W}], got {tuple(out.shape)}")
    with timed("depth_ingest"):
        check(lib.ocv_depth_ingest_fwd(depth_u16.data_ptr(), frame, row, Hs, Ws, int(top), int(left), float(factor),
                                       out.data_ptr() + 4 * H * W * int(out_index), B, H, W, _stream()), "ocv_depth_ingest_fwd")
    return out


def colormap_scale(vmin: float, vmax: float) -> float:
    """256 / (vmax - vmin) in fp32, as ``depth_finalize`` hands it to the kernel."""
    lo, hi = torch.tensor(float(vmin), dtype=torch.float32), torch.tensor(float(vmax), dtype=torch.float32)
    if not bool(hi > lo):
        raise ValueError("colour range: vmax must be above vmin")
    return float(torch.tensor(256.0, dtype=torch.float32) / (hi - lo))


def depth_finalize(pred: torch.Tensor, min_depth: float, max_depth: float, size: Tuple[int, int],
                   pred_mirror: Optional[torch.Tensor] = None, want: Tuple[str, ...] = ("depth",), u16_scale: float = 1000.0,
                   colormap: Optional[torch.Tensor] = None, vmin: Optional[float] = None, vmax: Optional[float] = None,
                   out: Optional[dict] = None, var: Optional[torch.Tensor] = None, pmax: Optional[torch.Tensor] = None,
                   var_mirror: Optional[torch.Tensor] = None, pmax_mirror: Optional[torch.Tensor] = None) -> dict:
    """The model's depth_pred [B, 1, h, w] (+ ``pred_mirror``, the output for the mirrored image, still mirrored) -> the final map at
    ``size`` = (H, W): flip-TTA average of the clamped maps (or the clamped map), bilinear align_corners resize, nan -> min_depth,
    +-inf -> max_depth -- the map ``depth_metrics`` evaluates, materialised.  ``want``: any of "depth" (fp32 [B, 1, H, W]),
    "depth_u16" ([B, H, W] = min(65535, rint(depth * u16_scale))), "rgb8" ([B, H, W, 3] through ``colormap``, uint8 [256, 3] on the
    device, over [vmin, vmax]; default the depth range), and -- from the bin head's statistics ``var`` / ``pmax`` (``bin_head(...,
    stats=True)``; with ``pred_mirror`` also ``var_mirror`` / ``pmax_mirror``, still mirrored) -- "depth_std" and "confidence" (fp32
    [B, 1, H, W]): standard deviation and peak probability of the MIXTURE of the source distributions under the same bilinear (and
    TTA) weights, m = sum w_t d_t on the unclamped maps, std = sqrt(sum w_t (var_t + (d_t - m)^2)), confidence = sum w_t pmax_t;
    nan -> max_depth - min_depth / 0.  They come from a second launch (ocv_depth_finalize_stats_fwd); the first three outputs are
    what they are without them.  ``out``: {name: tensor} to write into.  -> {name: tensor}."""
    lib = _lib.load()
    _req(pred, "pred")
    if pred.dim() != 4 or pred.shape[1] != 1:
        raise ValueError("depth_finalize: expected pred [B, 1, h, w]")
    if pred_mirror is not None:
        _req(pred_mirror, "pred_mirror")
        if pred_mirror.shape != pred.shape:
            raise ValueError("depth_finalize: pred_mirror must have pred's shape")
    want = tuple(want)
    bad = set(want) - {"depth", "depth_u16", "rgb8", "depth_std", "confidence"}
    if bad or not want:
        raise ValueError(f"depth_finalize: want must name some of 'depth', 'depth_u16', 'rgb8', 'depth_std', 'confidence' (got {want})")
    for name, need, t, tm in (("depth_std", "var", var, var_mirror), ("confidence", "pmax", pmax, pmax_mirror)):
        if name not in want:
            continue
        if t is None or (pred_mirror is not None and tm is None):
            raise ValueError(f"depth_finalize: '{name}' needs {need}{' and ' + need + '_mirror' if pred_mirror is not None else ''} "
                             "(hip_ops.bin_head(..., stats=True))")
        for nm, x in ((need, t), (need + "_mirror", tm if pred_mirror is not None else None)):
            if x is not None:
                _req(x, nm)
                if x.shape != pred.shape:
                    raise ValueError(f"depth_finalize: {nm} must have pred's shape")
    B, _, h, w = (int(s) for s in pred.shape)
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise ValueError("depth_finalize: bad output size")
    out = dict(out or {})
    res = {}
    if "depth" in want:
        res["depth"] = _out_slice(out.get("depth"), (B, 1, H, W), torch.float32, pred.device, "depth_finalize")
    if "depth_u16" in want:
        res["depth_u16"] = _out_slice(out.get("depth_u16"), (B, H, W), torch.uint16, pred.device, "depth_finalize")
    scale = 0.0
    lo = float(min_depth) if vmin is None else float(vmin)
    if "rgb8" in want:
        if colormap is None:
            raise ValueError("depth_finalize: 'rgb8' needs a colormap (uint8 [256, 3] on the device: predict.colormap_table)")
        _req(colormap, "colormap", torch.uint8)
        if tuple(colormap.shape) != (256, 3):
            raise ValueError(f"depth_finalize: colormap must be [256, 3], got {tuple(colormap.shape)}")
        scale = colormap_scale(lo, float(max_depth) if vmax is None else float(vmax))
        res["rgb8"] = _out_slice(out.get("rgb8"), (B, H, W, 3), torch.uint8, pred.device, "depth_finalize")
    if "depth_std" in want or "confidence" in want:
        sd = _out_slice(out.get("depth_std"), (B, 1, H, W), torch.float32, pred.device, "depth_finalize") if "depth_std" in want else None
        cf = _out_slice(out.get("confidence"), (B, 1, H, W), torch.float32, pred.device, "depth_finalize") if "confidence" in want else None
        tta = pred_mirror is not None
        with timed("depth_finalize_stats"):
            check(lib.ocv_depth_finalize_stats_fwd(pred.data_ptr(), _ptr(pred_mirror), _ptr(var) if sd is not None else None,
                                                   _ptr(var_mirror) if sd is not None and tta else None,
                                                   _ptr(pmax) if cf is not None else None,
                                                   _ptr(pmax_mirror) if cf is not None and tta else None, h, w, float(min_depth),
                                                   float(max_depth), H, W, _ptr(sd), _ptr(cf), B, _stream()), "ocv_depth_finalize_stats_fwd")
        if sd is not None:
            res["depth_std"] = sd
        if cf is not None:
            res["confidence"] = cf
    if not res.keys() - {"depth_std", "confidence"}:
        return res
    with timed("depth_finalize"):
        check(lib.ocv_depth_finalize_fwd(pred.data_ptr(), _ptr(pred_mirror), h, w, float(min_depth), float(max_depth), H, W,
                                         _ptr(res.get("depth")), _ptr(res.get("depth_u16")), float(u16_scale), _ptr(res.get("rgb8")),
                                         _ptr(colormap) if "rgb8" in want else None, lo, scale, B, _stream()), "ocv_depth_finalize_fwd")
    return res


OBJECT_DEPTH_COLUMNS = 5          # n, min, max, mean, std_mean in front of the quantiles


def object_depth(depth: torch.Tensor, xywh: torch.Tensor, counts: torch.Tensor, depth_std: Optional[torch.Tensor] = None,
                 quantiles: Sequence[float] = (0.1, 0.5, 0.9), shrink: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depth statistics per detection box: ``depth`` fp32 [B, 1, H, W] (the final map), ``xywh`` fp32 [B, cap, k >= 4] = centre x,
    centre y, width, height in the map's pixels (rows may be wider than 4 and strided: ``PaddedObjects.xywh``), ``counts`` int32 [B] on
    the device -> fp32 [B, cap, 5 + Q]: n, min, max, mean, std_mean, then v[floor(q * (n - 1))] per quantile, v the sorted non-NaN
    pixels whose centres lie inside the box (its central ``shrink`` part).  min, max and the quantiles are elements of the map; the
    means are float64 sums rounded once; std_mean is the mean of ``depth_std`` (same shape as ``depth``) over the same pixels, 0
    without it.  Rows at or beyond ``counts[b]`` and boxes without a valid pixel are all zero (n = 0).  One launch
    (ocv_object_depth_fwd), the counts are read on the device only."""
    lib = _lib.load()
    _req(depth, "depth")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"object_depth: expected depth [B, 1, H, W], got {tuple(depth.shape)}")
    B, _, H, W = (int(s) for s in depth.shape)
    if depth_std is not None:
        _req(depth_std, "depth_std")
        if depth_std.shape != depth.shape:
            raise ValueError("object_depth: depth_std must have depth's shape")
    _req(xywh, "xywh", contiguous=False)
    if xywh.dim() != 3 or xywh.shape[0] != B or xywh.shape[1] < 1 or xywh.shape[2] < 4:
        raise ValueError(f"object_depth: expected xywh [{B}, cap >= 1, k >= 4], got {tuple(xywh.shape)}")
    cap = int(xywh.shape[1])
    st = xywh.stride()
    row = int(st[1]) if cap > 1 else max(int(st[1]), 4)
    if st[2] != 1 or row < 4 or (B > 1 and st[0] != cap * row):
        raise ValueError(f"object_depth: xywh rows must be dense and evenly spaced over the batch (strides {st})")
    _req(counts, "counts", torch.int32)
    if tuple(counts.shape) != (B,):
        raise ValueError(f"object_depth: counts must be int32 [{B}], got {tuple(counts.shape)}")
    q = tuple(float(v) for v in quantiles)
    if not 1 <= len(q) <= 8 or not all(0.0 <= v <= 1.0 for v in q):
        raise ValueError(f"object_depth: 1 to 8 quantiles in [0, 1], got {q}")
    shrink = float(shrink)
    if not 0.0 < shrink <= 1.0 or C.c_float(0.5 * shrink).value <= 0.0:
        raise ValueError(f"object_depth: shrink must be in (0, 1], got {shrink}")
    out = _out_slice(out, (B, cap, OBJECT_DEPTH_COLUMNS + len(q)), torch.float32, depth.device, "object_depth")
    with timed("object_depth"):
        check(lib.ocv_object_depth_fwd(depth.data_ptr(), _ptr(depth_std), xywh.data_ptr(), row, counts.data_ptr(), B, cap, H, W,
                                       0.5 * shrink, (C.c_double * len(q))(*q), len(q), out.data_ptr(), _stream()),
              "ocv_object_depth_fwd")
    return out


OBJECT_METRICS_COLUMNS = 10       # abs_rel, sq_rel, rmse, rmse_log, log10, delta1, delta2, delta3, n_valid, gt_mean
OBJECT_METRICS_MAX_BOXES = 1024   # include/objcavit_hip.h: OCV_OBJECT_METRICS_MAX_BOXES, boxes per image the region pass takes


def object_metrics(pred: torch.Tensor, gt: torch.Tensor, xywh: torch.Tensor, counts: torch.Tensor, min_depth: float, max_depth: float,
                   crop: Optional[Tuple[int, int, int, int]] = None, pred_mirror: Optional[torch.Tensor] = None, shrink: float = 1.0,
                   regions: bool = True, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Depth error per detection box and over objects against background: ``pred`` [B, 1, h, w], ``gt`` [B, 1, H, W], depth range,
    ``crop`` = (y0, y1, x0, x1) and ``pred_mirror`` as ``depth_metrics`` takes them; ``xywh`` fp32 [B, cap, k >= 4] (rows may be strided),
    ``counts`` int32 [B] on the device and ``shrink`` as ``object_depth`` takes them, in pixels of the ground truth's grid ->
    (boxes fp32 [B, cap, 10], regions fp32 [B, 2, 10] or None without ``regions``).  A record is the eight metrics of ``depth_metrics``
    over a set of valid pixels, then n_valid and the float64 mean of gt: per box over the box's valid pixels (all zero for rows at or
    beyond ``counts[b]``, empty boxes and boxes without a valid pixel), regions[:, 0] over the valid pixels under any of the image's
    boxes, regions[:, 1] over those under none -- their n_valid add up to ``depth_metrics``' exactly.  ``out``: a [B, cap, 10] table to
    write the boxes into.  One launch for the boxes, two for the regions (ocv_object_metrics_fwd), the counts are read on the device
    only; with ``regions`` at most ``OBJECT_METRICS_MAX_BOXES`` rows per image."""
    lib = _lib.load()
    _req(pred, "pred"); _req(gt, "gt")
    if pred.dim() != 4 or gt.dim() != 4 or pred.shape[1] != 1 or gt.shape[1] != 1 or pred.shape[0] != gt.shape[0]:
        raise ValueError("object_metrics: expected pred [B,1,h,w] and gt [B,1,H,W]")
    if pred_mirror is not None:
        _req(pred_mirror, "pred_mirror")
        if pred_mirror.shape != pred.shape:
            raise ValueError("object_metrics: pred_mirror must have pred's shape")
    B, _, h, w = (int(v) for v in pred.shape)
    H, W = (int(v) for v in gt.shape[2:])
    _req(xywh, "xywh", contiguous=False)
    if xywh.dim() != 3 or xywh.shape[0] != B or xywh.shape[1] < 1 or xywh.shape[2] < 4:
        raise ValueError(f"object_metrics: expected xywh [{B}, cap >= 1, k >= 4], got {tuple(xywh.shape)}")
    cap = int(xywh.shape[1])
    st = xywh.stride()
    row = int(st[1]) if cap > 1 else max(int(st[1]), 4)
    if st[2] != 1 or row < 4 or (B > 1 and st[0] != cap * row):
        raise ValueError(f"object_metrics: xywh rows must be dense and evenly spaced over the batch (strides {st})")
    _req(counts, "counts", torch.int32)
    if tuple(counts.shape) != (B,):
        raise ValueError(f"object_metrics: counts must be int32 [{B}], got {tuple(counts.shape)}")
    shrink = float(shrink)
    if not 0.0 < shrink <= 1.0 or C.c_float(0.5 * shrink).value <= 0.0:
        raise ValueError(f"object_metrics: shrink must be in (0, 1], got {shrink}")
    if regions and cap > OBJECT_METRICS_MAX_BOXES:
        raise ValueError(f"object_metrics: {cap} box rows per image; the region pass takes at most {OBJECT_METRICS_MAX_BOXES} "
                         "(regions=False gives the boxes alone)")
    y0, y1, x0, x1 = crop if crop is not None else (0, H, 0, W)
    out = _out_slice(out, (B, cap, OBJECT_METRICS_COLUMNS), torch.float32, pred.device, "object_metrics")
    reg = ws = None
    if regions:
        from ._core import workspace as _workspace
        reg = torch.empty((B, 2, OBJECT_METRICS_COLUMNS), dtype=torch.float32, device=pred.device)
        ws = _workspace(int(lib.ocv_object_metrics_workspace_bytes(B, H, W)), pred.device, "object_metrics")
    with timed("object_metrics"):
        check(lib.ocv_object_metrics_fwd(pred.data_ptr(), _ptr(pred_mirror), h, w, gt.data_ptr(), H, W, float(min_depth), float(max_depth),
                                         int(y0), int(y1), int(x0), int(x1), xywh.data_ptr(), row, counts.data_ptr(), B, cap,
                                         0.5 * shrink, out.data_ptr(), _ptr(reg), _ptr(ws), 0 if ws is None else int(ws.numel()),
                                         _stream()), "ocv_object_metrics_fwd")
    return out, reg


UNPROJECT_TILE = 2048             # include/objcavit_hip.h: OCV_UNPROJECT_TILE, candidates of the strided grid per workgroup


def unproject_grid(H: int, W: int, stride: Tuple[int, int] = (1, 1)) -> Tuple[int, int]:
    """(rows, columns) of the strided pixel grid of an H x W map: the pixels with y % sy == 0 and x % sx == 0."""
    sy, sx = int(stride[0]), int(stride[1])
    if sy < 1 or sx < 1:
        raise ValueError(f"depth_unproject: stride must be >= 1, got {tuple(stride)}")
    return -(-int(H) // sy), -(-int(W) // sx)


def depth_unproject(depth: torch.Tensor, K: torch.Tensor, capacity: int, stride: Tuple[int, int] = (1, 1), near: float = 0.0,
                    far: float = float("inf"), confidence: Optional[torch.Tensor] = None, min_confidence: float = 0.0,
                    depth_std: Optional[torch.Tensor] = None, max_std: float = float("inf"), frames: Optional[torch.Tensor] = None,
                    top: int = 0, left: int = 0, want_pixel: bool = False, out: Optional[dict] = None,
                    workspace: Optional[torch.Tensor] = None, image_index: int = 0) -> dict:
    """The final map as 3-D points in the camera frame: ``depth`` fp32 [B, 1, H, W], ``K`` fp32 [B, 4] on the device = fx, fy, cx, cy in
    pixels of the map's grid (OpenCV convention: index (x, y) is the pixel's centre) -> {"points": fp32 [B, capacity, 4], "counts": int32
    [B], "total": int32 [B]} (+ "pixel": int32 [B, capacity] = y * W + x with ``want_pixel``).  A pixel is kept iff it lies on the
    ``stride`` = (sy, sx) grid, its depth z is finite with near <= z <= far, ``confidence`` >= min_confidence and ``depth_std`` <= max_std
    where those maps (depth's shape) are given (NaN fails), and the image's fx, fy are finite and > 0, cx, cy finite.  Kept pixels are
    numbered in row-major order; point i is a 16-byte record: X = ((x - cx) / fx) * z, Y = ((y - cy) / fy) * z, Z = z (fp32, every
    operation rounded on its own), then the bytes R, G, B of ``frames[b, top + y, left + x]`` (uint8 [B, Hs, Ws, 3], rows / frames may be
    strided as ``frame_ingest`` takes them; 0 without frames) and rint(255 * clamp(confidence, 0, 1)) (255 without the map).
    total = the number of kept pixels, counts = min(total, capacity): the first ``capacity`` points are written.  ROWS AT OR BEYOND
    counts[b] ARE NOT WRITTEN: they hold whatever the buffer held (a new tensor: uninitialised memory) -- read ``points[b, :counts[b]]``.
    ``out``: {name: tensor} of caller-owned buffers [N, ...] with N >= image_index + B; the B images are written at ``image_index``
    (one batch filled by one call per differently sized frame) and the dict returned holds the whole buffers.  ``workspace``: a uint8
    device tensor of at least ``ocv_depth_unproject_workspace_bytes`` (default: the stream's workspace store).  Two launches
    (ocv_depth_unproject_fwd) on the current stream, nothing read on the host: capturable with ``out`` and a warmed-up workspace."""
    lib = _lib.load()
    _req(depth, "depth")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"depth_unproject: expected depth [B, 1, H, W], got {tuple(depth.shape)}")
    B, _, H, W = (int(s) for s in depth.shape)
    _req(K, "K")
    if tuple(K.shape) != (B, 4):
        raise ValueError(f"depth_unproject: K must be fp32 [{B}, 4] = fx, fy, cx, cy, got {tuple(K.shape)}")
    for name, t in (("confidence", confidence), ("depth_std", depth_std)):
        if t is not None:
            _req(t, name)
            if t.shape != depth.shape:
                raise ValueError(f"depth_unproject: {name} must have depth's shape")
    sy, sx = int(stride[0]), int(stride[1])
    unproject_grid(H, W, (sy, sx))
    cap = int(capacity)
    if cap < 1:
        raise ValueError(f"depth_unproject: capacity must be >= 1, got {capacity}")
    if not float(near) <= float(far):
        raise ValueError(f"depth_unproject: near = {near} must be <= far = {far}")
    fs = rs = Hs = Ws = 0
    if frames is not None:
        Bf, Hs, Ws, fs, rs = _frames_view(frames, "frames", torch.uint8, 3)
        if Bf != B:
            raise ValueError(f"depth_unproject: {Bf} frame(s) for {B} map(s)")
        _window(Hs, Ws, int(top), int(left), (H, W), "depth_unproject")
    out = dict(out or {})
    names = ("points", "counts", "total") + (("pixel",) if want_pixel else ())
    shapes = {"points": (cap, 4), "counts": (), "total": (), "pixel": (cap,)}
    N, index = B, int(image_index)
    if out:
        given = out.get("points")
        if not isinstance(given, torch.Tensor) or given.dim() != 3:
            raise ValueError("depth_unproject: out needs 'points' [N, capacity, 4]")
        N = int(given.shape[0])
        if index < 0 or index + B > N:
            raise ValueError(f"depth_unproject: {B} image(s) at index {index} do not fit buffers of {N}")
    else:
        index = 0
    res = {}
    for name in names:
        dtype = torch.float32 if name == "points" else torch.int32
        if out and name not in out:
            raise ValueError(f"depth_unproject: out has no '{name}' (it needs {names})")
        res[name] = _out_slice(out.get(name), (N,) + shapes[name], dtype, depth.device, "depth_unproject")
    need = int(lib.ocv_depth_unproject_workspace_bytes(B, H, W, sy, sx))
    if workspace is None:
        from ._core import workspace as _workspace
        workspace = _workspace(need, depth.device, "depth_unproject")
    else:
        _req(workspace, "workspace", torch.uint8)
    with timed("depth_unproject"):
        check(lib.ocv_depth_unproject_fwd(depth.data_ptr(), K.data_ptr(), _ptr(confidence), _ptr(depth_std), _ptr(frames), fs, rs, Hs, Ws,
                                          int(top), int(left), B, H, W, sy, sx, float(near), float(far), float(min_confidence),
                                          float(max_std), cap, res["points"].data_ptr() + 16 * cap * index,
                                          res["pixel"].data_ptr() + 4 * cap * index if want_pixel else None,
                                          res["counts"].data_ptr() + 4 * index, res["total"].data_ptr() + 4 * index,
                                          workspace.data_ptr(), int(workspace.numel()), _stream()), "ocv_depth_unproject_fwd")
    return res


NORMALS_WANT = ("normals", "rgb8", "valid")
NORMALS_MAX_RADIUS = 4            # include/objcavit_hip.h, Statement N: the window is (2r + 1)^2, r in 1..4


def depth_normals(depth: torch.Tensor, K: torch.Tensor, radius: int = 2, near: float = 0.0, far: float = float("inf"),
                  edge_ratio: float = 0.05, want: Tuple[str, ...] = ("normals",), out: Optional[dict] = None, image_index: int = 0) -> dict:
    """Surface normals of the final map (Statement N of include/objcavit_hip.h): ``depth`` fp32 [B, 1, H, W], ``K`` fp32 [B, 4] on the
    device = fx, fy, cx, cy in pixels of the map's grid (index (x, y) is the pixel's centre) -> {"normals": fp32 [B, 3, H, W], "rgb8":
    uint8 [B, H, W, 3] = rint(127.5 n + 127.5), "valid": uint8 [B, H, W]}, those that ``want`` names.  A pixel is valid iff its
    (2 radius + 1)^2 window lies inside the map, every depth in it is finite with near <= z <= far, the window's largest and smallest
    depth are within ``edge_ratio`` * z of the centre's z (no depth discontinuity), and the image's fx, fy are finite and > 0, cx, cy
    finite.  There the normal is m / |m|, m = (fx zu, fy zv, -(z + (x - cx) zu + (y - cy) zv)) with zu, zv the least-squares plane
    slopes of the window: the unit normal of the back-projected surface, pointing at the camera.  Invalid pixels are all zero in every
    output; every element is written.  ``out``: {name: tensor} of caller-owned buffers [N, ...] with N >= image_index + B; the B images
    are written at ``image_index`` and the dict returned holds the whole buffers.  One launch (ocv_depth_normals_fwd) on the current
    stream, nothing read on the host: capturable with ``out``."""
    lib = _lib.load()
    _req(depth, "depth")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"depth_normals: expected depth [B, 1, H, W], got {tuple(depth.shape)}")
    B, _, H, W = (int(s) for s in depth.shape)
    _req(K, "K")
    if tuple(K.shape) != (B, 4):
        raise ValueError(f"depth_normals: K must be fp32 [{B}, 4] = fx, fy, cx, cy, got {tuple(K.shape)}")
    r = int(radius)
    if not 1 <= r <= NORMALS_MAX_RADIUS or r != radius:
        raise ValueError(f"depth_normals: radius must be an integer in 1..{NORMALS_MAX_RADIUS}, got {radius}")
    if not float(near) <= float(far):
        raise ValueError(f"depth_normals: near = {near} must be <= far = {far}")
    if not C.c_float(float(edge_ratio)).value > 0.0:
        raise ValueError(f"depth_normals: edge_ratio must be > 0, got {edge_ratio}")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or set(want) - set(NORMALS_WANT):
        raise ValueError(f"depth_normals: want must name some of {NORMALS_WANT} (got {want})")
    out = dict(out or {})
    shapes = {"normals": (3, H, W), "rgb8": (H, W, 3), "valid": (H, W)}
    N, index = B, int(image_index)
    if out:
        missing = [n for n in want if n not in out]
        if missing:
            raise ValueError(f"depth_normals: out has no {missing} (it needs {want})")
        N = int(out[want[0]].shape[0]) if out[want[0]].dim() else 0
        if index < 0 or index + B > N:
            raise ValueError(f"depth_normals: {B} image(s) at index {index} do not fit buffers of {N}")
    else:
        index = 0
    res = {n: _out_slice(out.get(n), (N,) + shapes[n], torch.float32 if n == "normals" else torch.uint8, depth.device, "depth_normals")
           for n in NORMALS_WANT if n in want}
    at = {n: t.data_ptr() + index * H * W * (12 if n == "normals" else 3 if n == "rgb8" else 1) for n, t in res.items()}
    with timed("depth_normals"):
        check(lib.ocv_depth_normals_fwd(depth.data_ptr(), K.data_ptr(), H, W, r, float(near), float(far), float(edge_ratio),
                                        at.get("normals"), at.get("rgb8"), at.get("valid"), B, _stream()), "ocv_depth_normals_fwd")
    return res


def normals_gather(normals: torch.Tensor, pixel: torch.Tensor, counts: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A normal for every point of a cloud: ``normals`` fp32 [B, 3, H, W] (``depth_normals``), ``pixel`` int32 [B, cap] and ``counts``
    int32 [B] (``depth_unproject(..., want_pixel=True)``, on the device) -> fp32 [B, cap, 4]: row i of image b = (nx, ny, nz, 0) of the
    pixel ``pixel[b, i]`` = y * W + x, for i < counts[b].  ROWS AT OR BEYOND counts[b] ARE NOT WRITTEN (the cloud's rule).  One launch
    (ocv_normals_gather_fwd), the counts are read on the device only."""
    lib = _lib.load()
    _req(normals, "normals")
    if normals.dim() != 4 or normals.shape[1] != 3:
        raise ValueError(f"normals_gather: expected normals [B, 3, H, W], got {tuple(normals.shape)}")
    B, _, H, W = (int(s) for s in normals.shape)
    _req(pixel, "pixel", torch.int32)
    if pixel.dim() != 2 or int(pixel.shape[0]) != B or int(pixel.shape[1]) < 1:
        raise ValueError(f"normals_gather: pixel must be int32 [{B}, cap >= 1], got {tuple(pixel.shape)}")
    cap = int(pixel.shape[1])
    _req(counts, "counts", torch.int32)
    if tuple(counts.shape) != (B,):
        raise ValueError(f"normals_gather: counts must be int32 [{B}], got {tuple(counts.shape)}")
    out = _out_slice(out, (B, cap, 4), torch.float32, normals.device, "normals_gather")
    with timed("normals_gather"):
        check(lib.ocv_normals_gather_fwd(normals.data_ptr(), pixel.data_ptr(), counts.data_ptr(), H, W, cap, out.data_ptr(), B, _stream()),
              "ocv_normals_gather_fwd")
    return out


GROUND_GRID_WANT = ("count", "obstacle", "h_min", "h_max", "h_mean", "state", "first_occupied")
GROUND_GRID_TILE = 1024           # include/objcavit_hip.h: OCV_GROUND_GRID_TILE, candidates of the strided grid per workgroup
GROUND_GRID_MAX_HEIGHT = 1000.0   # Statement G: the band's edges are of magnitude at most 1000 (a point's height in 1 / 1024 m fits 2^20)


def ground_grid(depth: torch.Tensor, K: torch.Tensor, pose: torch.Tensor, grid: Tuple[float, float, float, int, int],
                band: Tuple[float, float] = (-0.5, 2.5), obstacle_height: float = 0.3, min_points: int = 1, min_obstacle_points: int = 3,
                stride: Tuple[int, int] = (1, 1), near: float = 0.0, far: float = float("inf"), confidence: Optional[torch.Tensor] = None,
                min_confidence: float = 0.0, depth_std: Optional[torch.Tensor] = None, max_std: float = float("inf"),
                want: Tuple[str, ...] = GROUND_GRID_WANT, out: Optional[dict] = None, workspace: Optional[torch.Tensor] = None,
                image_index: int = 0) -> dict:
    """The final map as a bird's-eye occupancy grid (Statement G of include/objcavit_hip.h): ``depth`` fp32 [B, 1, H, W], ``K`` fp32
    [B, 4] on the device as ``depth_unproject`` takes it, ``pose`` fp32 [B, 12] on the device = a row-major 3 x 4 [R | t] from the camera
    frame (x right, y down, z forward) to the ground frame (row 0 lateral, row 1 forward, row 2 height), ``grid`` = (x0, y0, cell, GX,
    GY): GX x GY cells of ``cell`` metres from the corner (x0, y0), lateral x forward.  A pixel is a point iff ``depth_unproject`` would
    keep it (``stride``, ``near`` / ``far``, ``confidence`` / ``depth_std`` with their thresholds, a usable camera) and its image's pose
    is finite; the point's ground coordinates g = R P + t are fp32, every operation rounded on its own; it belongs to cell
    (floor((g_1 - y0) / cell), floor((g_0 - x0) / cell)) if that lies in the grid and ``band[0]`` <= g_2 <= ``band[1]``.  ->
    {"count", "obstacle" (points above ``obstacle_height``): int32 [B, GY, GX]; "h_min", "h_max", "h_mean": fp32 [B, GY, GX], 0 in an
    empty cell; "state": uint8 [B, GY, GX], 0 = unknown (count < min_points), 2 = occupied (obstacle >= min_obstacle_points), 1 = free;
    "first_occupied": fp32 [B, GX], the forward distance y0 + iy * cell of the nearest occupied cell of a lateral column, +inf without
    one}, those that ``want`` names; every element is written.  ``out``: {name: tensor} of caller-owned buffers [N, ...] with N >=
    image_index + B; the B images are written at ``image_index`` and the dict returned holds the whole buffers.  ``workspace``: a uint8
    device tensor of at least ``ocv_ground_grid_workspace_bytes`` (default: the stream's workspace store).  Three launches
    (ocv_ground_grid_fwd) on the current stream, integer atomics only (two calls give the same bytes), nothing read on the host:
    capturable with ``out`` and a warmed-up workspace."""
    lib = _lib.load()
    _req(depth, "depth")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"ground_grid: expected depth [B, 1, H, W], got {tuple(depth.shape)}")
    B, _, H, W = (int(s) for s in depth.shape)
    _req(K, "K")
    if tuple(K.shape) != (B, 4):
        raise ValueError(f"ground_grid: K must be fp32 [{B}, 4] = fx, fy, cx, cy, got {tuple(K.shape)}")
    _req(pose, "pose")
    if tuple(pose.shape) != (B, 12):
        raise ValueError(f"ground_grid: pose must be fp32 [{B}, 12] = a row-major 3 x 4 [R | t], got {tuple(pose.shape)}")
    for name, t in (("confidence", confidence), ("depth_std", depth_std)):
        if t is not None:
            _req(t, name)
            if t.shape != depth.shape:
                raise ValueError(f"ground_grid: {name} must have depth's shape")
    sy, sx = int(stride[0]), int(stride[1])
    unproject_grid(H, W, (sy, sx))
    if not float(near) <= float(far):
        raise ValueError(f"ground_grid: near = {near} must be <= far = {far}")
    if len(tuple(grid)) != 5:
        raise ValueError(f"ground_grid: grid must be (x0, y0, cell, GX, GY), got {grid}")
    x0, y0, cell = (C.c_float(float(v)).value for v in tuple(grid)[:3])
    GX, GY = int(grid[3]), int(grid[4])
    if GX != grid[3] or GY != grid[4] or GX < 1 or GY < 1:
        raise ValueError(f"ground_grid: GX, GY must be integers >= 1, got {grid[3]}, {grid[4]}")
    if not (0.0 < cell < float("inf")) or not abs(x0) < float("inf") or not abs(y0) < float("inf"):
        raise ValueError(f"ground_grid: cell must be > 0 and finite and the origin finite, got {tuple(grid)[:3]}")
    lo, hi = (C.c_float(float(v)).value for v in band)
    if not lo <= hi or not abs(lo) <= GROUND_GRID_MAX_HEIGHT or not abs(hi) <= GROUND_GRID_MAX_HEIGHT:
        raise ValueError(f"ground_grid: band must be (lo, hi) with lo <= hi, both within +-{GROUND_GRID_MAX_HEIGHT}, got {tuple(band)}")
    if float(obstacle_height) != float(obstacle_height):
        raise ValueError("ground_grid: obstacle_height is NaN")
    if int(min_points) != min_points or int(min_obstacle_points) != min_obstacle_points or min_points < 1 or min_obstacle_points < 1:
        raise ValueError(f"ground_grid: min_points and min_obstacle_points must be integers >= 1, got {min_points}, {min_obstacle_points}")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or set(want) - set(GROUND_GRID_WANT):
        raise ValueError(f"ground_grid: want must name some of {GROUND_GRID_WANT} (got {want})")
    out = dict(out or {})
    N, index = B, int(image_index)
    if out:
        missing = [n for n in want if n not in out]
        if missing:
            raise ValueError(f"ground_grid: out has no {missing} (it needs {want})")
        N = int(out[want[0]].shape[0]) if out[want[0]].dim() else 0
        if index < 0 or index + B > N:
            raise ValueError(f"ground_grid: {B} image(s) at index {index} do not fit buffers of {N}")
    else:
        index = 0
    dtypes = {"count": torch.int32, "obstacle": torch.int32, "state": torch.uint8}
    res = {n: _out_slice(out.get(n), (N, GX) if n == "first_occupied" else (N, GY, GX), dtypes.get(n, torch.float32), depth.device,
                         "ground_grid") for n in GROUND_GRID_WANT if n in want}
    at = {n: t.data_ptr() + index * t.element_size() * (GX if n == "first_occupied" else GX * GY) for n, t in res.items()}
    need = int(lib.ocv_ground_grid_workspace_bytes(B, GX, GY))
    if need == 0:
        raise ValueError(f"ground_grid: a grid of {B} x {GY} x {GX} cells is too large (B * GX * GY below 2^31, GX and GY at most 2^24)")
    if workspace is None:
        from ._core import workspace as _workspace
        workspace = _workspace(need, depth.device, "ground_grid")
    else:
        _req(workspace, "workspace", torch.uint8)
    with timed("ground_grid"):
        check(lib.ocv_ground_grid_fwd(depth.data_ptr(), K.data_ptr(), pose.data_ptr(), _ptr(confidence), _ptr(depth_std), B, H, W, sy, sx,
                                      float(near), float(far), float(min_confidence), float(max_std), x0, y0, cell, GX, GY, lo, hi,
                                      float(obstacle_height), int(min_points), int(min_obstacle_points), at.get("count"), at.get("obstacle"),
                                      at.get("h_min"), at.get("h_max"), at.get("h_mean"), at.get("state"), at.get("first_occupied"),
                                      workspace.data_ptr(), int(workspace.numel()), _stream()), "ocv_ground_grid_fwd")
    return res


__all__ = ["frame_ingest", "frame_ingest_format", "frame_resize_ingest_format", "frames_to_rgb24", "frame_yuv_tables", "resize_taps", "frame_resize_supported", "frame_resize_taps", "frame_resize_ingest", "FRAME_RESIZE_MAX_RATIO",
           "depth_ingest", "depth_finalize", "colormap_scale", "object_depth", "OBJECT_DEPTH_COLUMNS", "object_metrics",
           "OBJECT_METRICS_COLUMNS", "OBJECT_METRICS_MAX_BOXES", "depth_unproject",
           "unproject_grid", "UNPROJECT_TILE", "depth_normals", "normals_gather", "NORMALS_WANT", "NORMALS_MAX_RADIUS",
           "ground_grid", "GROUND_GRID_WANT", "GROUND_GRID_TILE", "GROUND_GRID_MAX_HEIGHT"]
