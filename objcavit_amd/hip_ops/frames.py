"""hip_ops frames: the two ends of the predict path -- decoded uint8 / uint16 frames in (csrc/frame_ingest.hip; a window of any size
resized to the model's on the way in: csrc/frame_resize.hip; the rectified window of distorted frames: csrc/frame_remap.hip), full-resolution depth maps out (csrc/depth_finalize.hip).  What is read
out of the final map behind them is ``readouts``.  Same rules as every wrapper: operands are checked on the host, CPU tensors raise
``HipLibraryError``, one launch on the current stream, ``out=`` writes straight into a buffer the caller owns (a captured graph's
static input).  The four ingest wrappers are fronts of one function, ``_ingest``."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import check
from ..lens import LensMap
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
    return _ingest(frames_u8, table, None, top, left, size, None, mirror_too, out, out_index)


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
    return _ingest(frames_u8, table, None, top, left, window, size, mirror_too, out, out_index, taps)


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


def _ratio_checked(Hw: int, Ww: int, H: int, W: int, who: str) -> None:
    if not frame_resize_supported(Hw, Ww, H, W):
        raise ValueError(f"{who}: a {Hw} x {Ww} window to {H} x {W} shrinks by more than {FRAME_RESIZE_MAX_RATIO} "
                         "along an axis, the most one launch takes (the filter is never truncated): resize in two steps")


def _ingest(frames, table: torch.Tensor, fmt: Optional[PixelFormat], top: int, left: int, window: Optional[Tuple[int, int]],
            size: Optional[Tuple[int, int]], mirror_too: bool, out: Optional[torch.Tensor], out_index: int,
            taps: Optional[Sequence[torch.Tensor]] = None, yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What the four ingest wrappers are fronts of: the ``window`` = (Hw, Ww) at (top, left) (None: the rest of the frame) of frames in
    ``fmt`` (None: packed RGB through the rgb24 entry points) -> fp32 NCHW at ``size`` (None: the window's own, no resize).  The source
    view, the window, the resize ratio, the table, the taps, the ``out`` / ``out_index`` / mirror-half rule and the choice among the four
    entry points; every text carries the name of the wrapper that stands for the case."""
    lib = _lib.load()
    who = f"frame{'_resize' if size is not None else ''}_ingest{'_format' if fmt is not None else ''}"
    top, left = int(top), int(left)
    if size is not None:
        H, W = int(size[0]), int(size[1])
        if H < 1 or W < 1:
            raise ValueError(f"{who}: bad output size {tuple(size)}")
    if fmt is None:
        if size is not None and isinstance(frames, torch.Tensor) and frames.dim() == 4:     # the ratio is judged first: it needs no device
            _ratio_checked(*_window(int(frames.shape[1]), int(frames.shape[2]), top, left, window, who), H, W, who)
        B, Hs, Ws, frame, row = _frames_view(frames, "frames_u8", torch.uint8, 3)
        device, source = frames.device, [frames.data_ptr(), frame, row]
    else:
        B, Hs, Ws, device, planes = _source(frames, fmt, who)
    Hw, Ww = _window(Hs, Ws, top, left, window, who)
    if size is None:
        H, W = Hw, Ww
    elif fmt is not None:
        _ratio_checked(Hw, Ww, H, W, who)
    _req(table, "table")
    if tuple(table.shape) != (3, 256):
        raise ValueError(f"{who}: table must be [3, 256], got {tuple(table.shape)}")
    resize = []
    if size is not None:
        if taps is None:
            taps = frame_resize_taps(device, Hw, Ww, H, W)
        if len(taps) != 4:
            raise ValueError(f"{who}: taps = (ystart, yweight, xstart, xweight)")
        ys, yw, xs, xw = taps
        for name, st, wt, n in (("y", ys, yw, H), ("x", xs, xw, W)):
            _req(st, f"taps: {name}start", torch.int32)
            _req(wt, f"taps: {name}weight")
            if tuple(st.shape) != (n,) or wt.dim() != 2 or wt.shape[0] != n or wt.shape[1] < 1:
                raise ValueError(f"{who}: taps of the {name} axis must be int32 [{n}] and fp32 [{n}, K], got "
                                 f"{tuple(st.shape)} / {tuple(wt.shape)}")
        resize = [ys.data_ptr(), yw.data_ptr(), int(yw.shape[1]), xs.data_ptr(), xw.data_ptr(), int(xw.shape[1])]
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
    if fmt is not None:
        source = [fmt.id, *planes, _ptr(_yuv_on(device, fmt, yuv_tables))]
    entry = ("ocv_frame_ingest_fwd" if size is None else "ocv_frame_resize_ingest") if fmt is None else f"ocv_{who}"
    plane = 3 * H * W
    with timed(who):
        check(getattr(lib, entry)(*source, Hs, Ws, top, left, *((Hw, Ww) if size is not None else ()), table.data_ptr(), *resize,
                                  out.data_ptr() + 4 * plane * int(out_index), B, H, W, 1 if mirror_too else 0, half * plane,
                                  _stream()), entry)
    return out


def frame_window_ingest(frames, table: torch.Tensor, top: int = 0, left: int = 0, window: Optional[Tuple[int, int]] = None,
                        size: Optional[Tuple[int, int]] = None, pixel_format=None, mirror_too: bool = False,
                        out: Optional[torch.Tensor] = None, out_index: int = 0, taps: Optional[Sequence[torch.Tensor]] = None,
                        yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The four ingest wrappers in one call: ``size`` None is ``frame_ingest`` of the ``window``, else ``frame_resize_ingest`` of it to
    ``size``; ``pixel_format`` None reads packed RGB through those two, else through their ``*_format`` forms.  The same launch with the
    same arguments as the wrapper it stands for, whose name its errors carry."""
    fmt = None if pixel_format is None else PixelFormat.of(pixel_format)
    return _ingest(frames, table, fmt, top, left, window, size, mirror_too, out, out_index, taps, yuv_tables)


def frame_ingest_format(frames, table: torch.Tensor, pixel_format, top: int = 0, left: int = 0, size: Optional[Tuple[int, int]] = None,
                        mirror_too: bool = False, out: Optional[torch.Tensor] = None, out_index: int = 0,
                        yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``frame_ingest`` for frames of any ``pixel_format`` (a ``PixelFormat`` or a name): a uint8 tensor [B, Hs, Ws, 3 | 4] for the
    packed formats, a ``PlanarFrames`` for nv12 / i420, whose pixels become R, G, B bytes by Statement P (``pixel_formats``) inside the
    launch.  Every other argument as ``frame_ingest`` takes it; bit-equal to ``frame_ingest`` on the converted frames.  One launch
    (ocv_frame_ingest_format) on the current stream; a 4:2:0 format's tables are uploaded on it when first used
    (``frame_yuv_tables``), or passed as ``yuv_tables`` (the int32 [5, 256] device tensor of the format's matrix and range)."""
    return _ingest(frames, table, PixelFormat.of(pixel_format), top, left, size, None, mirror_too, out, out_index, None, yuv_tables)


def frame_resize_ingest_format(frames, table: torch.Tensor, size: Tuple[int, int], pixel_format, top: int = 0, left: int = 0,
                               window: Optional[Tuple[int, int]] = None, mirror_too: bool = False, out: Optional[torch.Tensor] = None,
                               out_index: int = 0, taps: Optional[Sequence[torch.Tensor]] = None,
                               yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``frame_resize_ingest`` for frames of any ``pixel_format`` (as ``frame_ingest_format`` takes them): the conversion happens
    while the window's pixels are staged, the two tap passes are ``frame_resize_ingest``'s -- bit-equal to it on the converted frames.
    One launch (ocv_frame_resize_ingest_format) on the current stream."""
    return _ingest(frames, table, PixelFormat.of(pixel_format), top, left, window, size, mirror_too, out, out_index, taps, yuv_tables)


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


def _lens_on(lens_map, device, B: int, Hs: int, Ws: int, who: str) -> torch.Tensor:
    """The device map of a ``lens.LensMap`` (uploaded when first used on ``device``, then kept), or an int32 device tensor [M, Hw, Ww, 2]
    of Statement L's entries as it is; M = 1 or B, and a ``LensMap``'s source size must be the frames'."""
    if isinstance(lens_map, LensMap):
        if lens_map.source_size != (Hs, Ws):
            raise ValueError(f"{who}: the lens map was made for {lens_map.source_size[0]} x {lens_map.source_size[1]} frames, got {Hs} x {Ws}")
        m = lens_map.on(device)
    else:
        m = lens_map
        _req(m, f"{who}: lens_map", torch.int32)
        if m.dim() != 4 or m.shape[3] != 2 or min(m.shape[:3]) < 1:
            raise ValueError(f"{who}: lens_map must be a LensMap or int32 [M, Hw, Ww, 2], got {tuple(m.shape)}")
    if int(m.shape[0]) not in (1, B):
        raise ValueError(f"{who}: {int(m.shape[0])} maps for {B} frame(s): one map for the batch or one per frame")
    return m


def frame_remap_ingest(frames, table: torch.Tensor, lens_map, pixel_format=None, mirror_too: bool = False,
                       out: Optional[torch.Tensor] = None, out_index: int = 0, yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``frame_ingest_format`` through a lens: the rectified window of DISTORTED frames of any ``pixel_format`` (None: rgb24; frames as
    ``frame_ingest_format`` takes them) -> fp32 NCHW [B, 3, Hw, Ww], every channel value the ``table`` entry of the byte Statement L
    (include/objcavit_hip.h, ``objcavit_amd.lens``) gathers for the pixel: four taps of the source frame in the format's own fetch,
    8-bit weights, integer arithmetic, a black border.  ``lens_map``: a ``LensMap`` made for the frames' size (its device copy is
    uploaded on the current stream when first used, then kept) or an int32 device tensor [M, Hw, Ww, 2], M = 1 or B.  ``mirror_too``,
    ``out``, ``out_index``: as ``frame_ingest`` takes them.  One launch (ocv_frame_remap_ingest_fwd) on the current stream; bit-equal to
    ``frame_ingest`` of ``frames_remap_rgb24``'s bytes, and with ``LensMap.identity`` to ``frame_ingest_format`` of that window."""
    lib = _lib.load()
    who = "frame_remap_ingest"
    fmt = PixelFormat.of(pixel_format)
    B, Hs, Ws, device, planes = _source(frames, fmt, who)
    m = _lens_on(lens_map, device, B, Hs, Ws, who)
    Hw, Ww = int(m.shape[1]), int(m.shape[2])
    _req(table, "table")
    if tuple(table.shape) != (3, 256):
        raise ValueError(f"{who}: table must be [3, 256], got {tuple(table.shape)}")
    if out is None:
        out = torch.empty((2 * B if mirror_too else B, 3, Hw, Ww), dtype=torch.float32, device=device)
        out_index = 0
    else:
        _req(out, f"{who}: out")
        if out.dim() != 4 or tuple(out.shape[1:]) != (3, Hw, Ww):
            raise ValueError(f"{who}: out must be [N, 3, {Hw}, {Ww}], got {tuple(out.shape)}")
    N = int(out.shape[0])
    half = N // 2 if mirror_too else N
    if (mirror_too and N % 2) or out_index < 0 or out_index + B > half:
        raise ValueError(f"{who}: {B} image(s) at index {out_index} do not fit out {tuple(out.shape)}"
                         f"{' (first half: the second takes the mirrors)' if mirror_too else ''}")
    plane = 3 * Hw * Ww
    with timed(who):
        check(lib.ocv_frame_remap_ingest_fwd(fmt.id, *planes, _ptr(_yuv_on(device, fmt, yuv_tables)), Hs, Ws, m.data_ptr(), int(m.shape[0]),
                                             Hw, Ww, table.data_ptr(), out.data_ptr() + 4 * plane * int(out_index), B,
                                             1 if mirror_too else 0, half * plane, _stream()), "ocv_frame_remap_ingest_fwd")
    return out


def frames_remap_rgb24(frames, lens_map, pixel_format=None, out: Optional[torch.Tensor] = None,
                       yuv_tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rectified window of distorted frames (as ``frame_remap_ingest`` takes them, through the same ``lens_map``) -> packed RGB uint8
    [B, Hw, Ww, 3]: the bytes of Statement L themselves.  ``out``: a contiguous uint8 [B, Hw, Ww, 3] to write.  One launch
    (ocv_frames_remap_rgb24_fwd) on the current stream, every output byte written."""
    lib = _lib.load()
    who = "frames_remap_rgb24"
    fmt = PixelFormat.of(pixel_format)
    B, Hs, Ws, device, planes = _source(frames, fmt, who)
    m = _lens_on(lens_map, device, B, Hs, Ws, who)
    Hw, Ww = int(m.shape[1]), int(m.shape[2])
    out = _out_slice(out, (B, Hw, Ww, 3), torch.uint8, device, who)
    with timed(who):
        check(lib.ocv_frames_remap_rgb24_fwd(fmt.id, *planes, _ptr(_yuv_on(device, fmt, yuv_tables)), Hs, Ws, m.data_ptr(), int(m.shape[0]),
                                             Hw, Ww, out.data_ptr(), B, _stream()), "ocv_frames_remap_rgb24_fwd")
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


__all__ = ["frame_ingest", "frame_ingest_format", "frame_resize_ingest_format", "frame_window_ingest", "frames_to_rgb24", "frame_yuv_tables",
           "frame_remap_ingest", "frames_remap_rgb24",
           "resize_taps", "frame_resize_supported", "frame_resize_taps", "frame_resize_ingest", "FRAME_RESIZE_MAX_RATIO", "depth_ingest",
           "depth_finalize", "colormap_scale"]
