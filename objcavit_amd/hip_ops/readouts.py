"""hip_ops readouts: what is read out of the predict path's final map (``frames.depth_finalize``) behind it -- per-box statistics
(csrc/object_depth.hip), the point cloud (csrc/point_cloud.hip), the surface normals (csrc/surface_normals.hip), the bird's-eye occupancy
grid (csrc/ground_grid.hip), that grid fused over time (csrc/ground_fuse.hip), the obstacles its occupied cells form
(csrc/obstacles.hip), the ground plane that poses it
(csrc/ground_plane.hip) and, against ground truth, the depth error per box
and per region (csrc/object_metrics.hip).  Same rules as every wrapper: operands are checked on the host, CPU tensors raise
``HipLibraryError``, launches on the current stream, ``out=`` writes straight into buffers the caller owns.  The checks the wrappers
share are the four helpers in front of them."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import check
from ._core import _ptr, _req, _stream, timed
from .frames import _frames_view, _out_slice, _window


def _map_and_K(depth: torch.Tensor, K: Optional[torch.Tensor], who: str) -> Tuple[int, int, int]:
    """(B, H, W) of the final map ``depth`` fp32 [B, 1, H, W]; ``K`` (where the readout takes one) must be fp32 [B, 4]."""
    _req(depth, "depth")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"{who}: expected depth [B, 1, H, W], got {tuple(depth.shape)}")
    B, _, H, W = (int(s) for s in depth.shape)
    if K is not None:
        _req(K, "K")
        if tuple(K.shape) != (B, 4):
            raise ValueError(f"{who}: K must be fp32 [{B}, 4] = fx, fy, cx, cy, got {tuple(K.shape)}")
    return B, H, W


def _like_depth(depth: torch.Tensor, who: str, **maps) -> None:
    """The maps beside the final one (``confidence`` / ``depth_std``), where given, have its shape."""
    for name, t in maps.items():
        if t is not None:
            _req(t, name)
            if t.shape != depth.shape:
                raise ValueError(f"{who}: {name} must have depth's shape")


def _boxes(xywh: torch.Tensor, counts: torch.Tensor, shrink: float, B: int, who: str) -> Tuple[int, int, float]:
    """(cap, row stride in elements, shrink) of the boxes ``xywh`` fp32 [B, cap, k >= 4] (rows may be strided) / ``counts`` int32 [B]."""
    _req(xywh, "xywh", contiguous=False)
    if xywh.dim() != 3 or xywh.shape[0] != B or xywh.shape[1] < 1 or xywh.shape[2] < 4:
        raise ValueError(f"{who}: expected xywh [{B}, cap >= 1, k >= 4], got {tuple(xywh.shape)}")
    cap = int(xywh.shape[1])
    st = xywh.stride()
    row = int(st[1]) if cap > 1 else max(int(st[1]), 4)
    if st[2] != 1 or row < 4 or (B > 1 and st[0] != cap * row):
        raise ValueError(f"{who}: xywh rows must be dense and evenly spaced over the batch (strides {st})")
    _req(counts, "counts", torch.int32)
    if tuple(counts.shape) != (B,):
        raise ValueError(f"{who}: counts must be int32 [{B}], got {tuple(counts.shape)}")
    shrink = float(shrink)
    if not 0.0 < shrink <= 1.0 or C.c_float(0.5 * shrink).value <= 0.0:
        raise ValueError(f"{who}: shrink must be in (0, 1], got {shrink}")
    return cap, row, shrink


def _image_buffers(out: Optional[dict], want: Tuple[str, ...], shapes: dict, B: int, image_index: int, device, who: str):
    """The ``out=`` rule of the per-image readouts.  ``want``: the names asked for; ``shapes``: {name: (shape of one image, dtype)} in the
    order of the result.  Without ``out`` every buffer is made for the B images ([B, ...]) and written from image 0; with it every name
    wanted must be there, N is the first one's, and the B images at ``image_index`` must fit.  -> ({name: the whole buffer}, {name: the
    address of image ``image_index`` in it})."""
    out = dict(out or {})
    N, index = B, int(image_index)
    if out:
        missing = [n for n in want if n not in out]
        if missing:
            raise ValueError(f"{who}: out has no {missing} (it needs {want})")
        N = int(out[want[0]].shape[0]) if out[want[0]].dim() else 0
        if index < 0 or index + B > N:
            raise ValueError(f"{who}: {B} image(s) at index {index} do not fit buffers of {N}")
    else:
        index = 0
    res = {n: _out_slice(out.get(n), (N,) + tuple(shape), dtype, device, who) for n, (shape, dtype) in shapes.items() if n in want}
    return res, {n: t.data_ptr() + index * t.element_size() * math.prod(shapes[n][0]) for n, t in res.items()}


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
    B, H, W = _map_and_K(depth, None, "object_depth")
    _like_depth(depth, "object_depth", depth_std=depth_std)
    q = tuple(float(v) for v in quantiles)
    if not 1 <= len(q) <= 8 or not all(0.0 <= v <= 1.0 for v in q):
        raise ValueError(f"object_depth: 1 to 8 quantiles in [0, 1], got {q}")
    cap, row, shrink = _boxes(xywh, counts, shrink, B, "object_depth")
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
    cap, row, shrink = _boxes(xywh, counts, shrink, B, "object_metrics")
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
    B, H, W = _map_and_K(depth, K, "depth_unproject")
    _like_depth(depth, "depth_unproject", confidence=confidence, depth_std=depth_std)
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
    names = ("points", "counts", "total") + (("pixel",) if want_pixel else ())
    if out and not (isinstance(out.get("points"), torch.Tensor) and out["points"].dim() == 3):     # this one names its first buffer
        raise ValueError("depth_unproject: out needs 'points' [N, capacity, 4]")
    for name in names if out else ():
        if name not in out:
            raise ValueError(f"depth_unproject: out has no '{name}' (it needs {names})")
    shapes = {"points": ((cap, 4), torch.float32), "counts": ((), torch.int32), "total": ((), torch.int32), "pixel": ((cap,), torch.int32)}
    res, at = _image_buffers(out, names, shapes, B, image_index, depth.device, "depth_unproject")
    need = int(lib.ocv_depth_unproject_workspace_bytes(B, H, W, sy, sx))
    if workspace is None:
        from ._core import workspace as _workspace
        workspace = _workspace(need, depth.device, "depth_unproject")
    else:
        _req(workspace, "workspace", torch.uint8)
    with timed("depth_unproject"):
        check(lib.ocv_depth_unproject_fwd(depth.data_ptr(), K.data_ptr(), _ptr(confidence), _ptr(depth_std), _ptr(frames), fs, rs, Hs, Ws,
                                          int(top), int(left), B, H, W, sy, sx, float(near), float(far), float(min_confidence),
                                          float(max_std), cap, at["points"], at.get("pixel"), at["counts"], at["total"],
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
    B, H, W = _map_and_K(depth, K, "depth_normals")
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
    shapes = {"normals": ((3, H, W), torch.float32), "rgb8": ((H, W, 3), torch.uint8), "valid": ((H, W), torch.uint8)}
    res, at = _image_buffers(out, want, shapes, B, image_index, depth.device, "depth_normals")
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
    B, H, W = _map_and_K(depth, K, "ground_grid")
    _req(pose, "pose")
    if tuple(pose.shape) != (B, 12):
        raise ValueError(f"ground_grid: pose must be fp32 [{B}, 12] = a row-major 3 x 4 [R | t], got {tuple(pose.shape)}")
    _like_depth(depth, "ground_grid", confidence=confidence, depth_std=depth_std)
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
    dtypes = {"count": torch.int32, "obstacle": torch.int32, "state": torch.uint8}
    shapes = {n: ((GX,) if n == "first_occupied" else (GY, GX), dtypes.get(n, torch.float32)) for n in GROUND_GRID_WANT}
    res, at = _image_buffers(out, want, shapes, B, image_index, depth.device, "ground_grid")
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


OBSTACLES_WANT = ("cells", "metres", "counts", "total", "labels")
OBSTACLES_TILE = 32               # include/objcavit_hip.h: OCV_OBSTACLES_TILE, the union-find runs in LDS per tile of 32 x 32 cells
OBSTACLES_MAX_LINK = 3            # Statement O: link in 1..3
OBSTACLES_COLUMNS = 8             # columns of a row of "cells" / "metres"


def obstacles(state: torch.Tensor, spec: Tuple[float, float, float, int, int], count: Optional[torch.Tensor] = None,
              obstacle: Optional[torch.Tensor] = None, h_max: Optional[torch.Tensor] = None, link: int = 1, min_cells: int = 1,
              min_obstacle_points: int = 0, capacity: int = 64, want: Tuple[str, ...] = OBSTACLES_WANT, out: Optional[dict] = None,
              workspace: Optional[torch.Tensor] = None, image_index: int = 0) -> dict:
    """The occupied cells of a ground grid grouped into obstacles (Statement O of include/objcavit_hip.h): ``state`` uint8 [B, GY, GX]
    and, where given, ``count`` / ``obstacle`` int32 and ``h_max`` fp32 of that shape -- ``ground_grid``'s outputs, on the device --,
    ``spec`` = the grid's (x0, y0, cell, GX, GY).  Occupied cells (state 2) within ``link`` (1..3) cells of each other along both axes
    belong to one component; a component of at least ``min_cells`` cells and ``min_obstacle_points`` obstacle points is kept, and the
    kept ones are ranked by their smallest iy * GX + ix: nearest first, ties left to right.  -> {"cells": int32 [B, capacity, 8] = ix_min,
    ix_max, iy_min, iy_max, n, points, obstacle_points, root; "metres": fp32 [B, capacity, 8] = x_min, x_max, y_min, y_max, x_mean, y_mean,
    h_max, fill; "counts", "total": int32 [B], total = the number kept, counts = min(total, capacity); "labels": int32 [B, GY, GX] = -1
    where the cell is not occupied, its component's rank where that is kept and below ``capacity``, -2 otherwise}, those that ``want``
    names; rows at or beyond counts[b] are all zero; every element is written.  ``out``: {name: tensor} of caller-owned buffers [N, ...]
    with N >= image_index + B; the B images are written at ``image_index`` and the dict returned holds the whole buffers.
    ``workspace``: a uint8 device tensor of at least ``ocv_obstacles_workspace_bytes`` (default: the stream's workspace store).  At most
    seven launches (ocv_obstacles_fwd) on the current stream, integer atomics only (two calls give the same bytes), nothing read on the
    host: capturable with ``out`` and a warmed-up workspace."""
    lib = _lib.load()
    _req(state, "state", torch.uint8)
    if state.dim() != 3:
        raise ValueError(f"obstacles: expected state uint8 [B, GY, GX], got {tuple(state.shape)}")
    B, GY, GX = (int(v) for v in state.shape)
    if len(tuple(spec)) != 5:
        raise ValueError(f"obstacles: spec must be the grid's (x0, y0, cell, GX, GY), got {spec}")
    x0, y0, cell = (C.c_float(float(v)).value for v in tuple(spec)[:3])
    if (int(spec[3]), int(spec[4])) != (GX, GY) or GX < 1 or GY < 1 or B < 1:
        raise ValueError(f"obstacles: state {tuple(state.shape)} is not [B >= 1, GY, GX] of the grid {tuple(spec)}")
    if not (0.0 < cell < float("inf")) or not abs(x0) < float("inf") or not abs(y0) < float("inf"):
        raise ValueError(f"obstacles: cell must be > 0 and finite and the origin finite, got {tuple(spec)[:3]}")
    for name, t, dtype in (("count", count, torch.int32), ("obstacle", obstacle, torch.int32), ("h_max", h_max, torch.float32)):
        if t is not None:
            _req(t, name, dtype)
            if t.shape != state.shape:
                raise ValueError(f"obstacles: {name} must have state's shape")
    for name, v, lo in (("link", link, 1), ("min_cells", min_cells, 1), ("min_obstacle_points", min_obstacle_points, 0), ("capacity", capacity, 1)):
        if isinstance(v, bool) or int(v) != v or int(v) < lo:
            raise ValueError(f"obstacles: {name} must be an integer >= {lo}, got {v}")
    if int(link) > OBSTACLES_MAX_LINK:
        raise ValueError(f"obstacles: link must be in 1..{OBSTACLES_MAX_LINK}, got {link}")
    cap = int(capacity)
    if B * cap * OBSTACLES_COLUMNS >= 1 << 31:
        raise ValueError(f"obstacles: {B} x {cap} rows are too many (B * capacity * 8 below 2^31)")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or set(want) - set(OBSTACLES_WANT):
        raise ValueError(f"obstacles: want must name some of {OBSTACLES_WANT} (got {want})")
    shapes = {"cells": ((cap, OBSTACLES_COLUMNS), torch.int32), "metres": ((cap, OBSTACLES_COLUMNS), torch.float32),
              "counts": ((), torch.int32), "total": ((), torch.int32), "labels": ((GY, GX), torch.int32)}
    res, at = _image_buffers(out, want, shapes, B, image_index, state.device, "obstacles")
    need = int(lib.ocv_obstacles_workspace_bytes(B, GX, GY))
    if need == 0:
        raise ValueError(f"obstacles: a grid of {B} x {GY} x {GX} cells is too large (B * GX * GY below 2^31, GX and GY at most 2^24)")
    if workspace is None:
        from ._core import workspace as _workspace
        workspace = _workspace(need, state.device, "obstacles")
    else:
        _req(workspace, "workspace", torch.uint8)
    with timed("obstacles"):
        check(lib.ocv_obstacles_fwd(state.data_ptr(), _ptr(count), _ptr(obstacle), _ptr(h_max), B, GX, GY, x0, y0, cell, int(link),
                                    int(min_cells), int(min_obstacle_points), cap, at.get("cells"), at.get("metres"), at.get("labels"),
                                    at.get("counts"), at.get("total"), workspace.data_ptr(), int(workspace.numel()), _stream()),
              "ocv_obstacles_fwd")
    return res


def obstacles_set_dispatch(on_chip_merge: bool = True) -> None:
    """The statistics pass of ``obstacles`` with (default) or without its on-chip merge: the same bytes either way; the A/B of
    tools/measure_obstacles.py."""
    check(_lib.load().ocv_obstacles_set_dispatch(1 if on_chip_merge else 0), "ocv_obstacles_set_dispatch")


GROUND_FUSE_WANT = ("evidence", "state", "h_max", "first_occupied")
GROUND_FUSE_TILE = 16             # include/objcavit_hip.h: OCV_GROUND_FUSE_TILE, a workgroup fuses a tile of 16 x 16 cells
GROUND_FUSE_MAX = 16383           # Statement F: the largest value of each integer option (sums of two stay inside an int16's range)


def ground_fuse(state: torch.Tensor, spec: Tuple[float, float, float, int, int], motion: torch.Tensor,
                prev_evidence: Optional[torch.Tensor] = None, h_max: Optional[torch.Tensor] = None, prev_h: Optional[torch.Tensor] = None,
                free: int = 2, occupied: int = 4, decay: int = 1, limit: int = 32, free_at: int = 4, occupied_at: int = 6,
                want: Tuple[str, ...] = GROUND_FUSE_WANT, out: Optional[dict] = None, image_index: int = 0) -> dict:
    """One step of the ground memory (Statement F of include/objcavit_hip.h): ``state`` uint8 [B, GY, GX] and, where given, ``h_max`` fp32
    of that shape -- this step's ``ground_grid`` outputs, on the device --, ``spec`` = the grid's (x0, y0, cell, GX, GY), ``motion`` fp32
    [B, 4] on the device = (cos, sin, tx, ty): a point at p in this step's ground frame was at R p + t in the previous step's
    (``objcavit_amd.ground_memory.ego_motion``); ``prev_evidence`` int16 / ``prev_h`` fp32 [B, GY, GX]: the "evidence" / "h_max" the
    previous step returned (None: nothing yet).  Every cell carries the evidence of the previous map's cell its centre was in (the nearest
    one; none outside the grid, or when its image's motion is not finite: that image forgets), faded towards 0 by ``decay``, adds
    +``occupied`` where this step's state is 2 and -``free`` where it is 1, and is clamped to +-``limit``.  -> {"evidence": int16
    [B, GY, GX]; "state": uint8 [B, GY, GX], 2 where evidence >= ``occupied_at``, 1 where evidence <= -``free_at``, else 0; "h_max": fp32
    [B, GY, GX], the larger of this step's h_max (where its state is 2) and the carried one (where the carried evidence is positive), 0
    where the evidence is not positive; "first_occupied": fp32 [B, GX] of the fused state, as the grid's}, those that ``want`` names;
    every element is written.  ``out``: {name: tensor} of caller-owned buffers [N, ...] with N >= image_index + B; the B images are
    written at ``image_index`` and the dict returned holds the whole buffers.  No output may overlap an input (the warp is a gather: it
    cannot run in place).  One launch (ocv_ground_fuse_fwd) on the current stream, no workspace, no atomics (two calls give the same
    bytes), nothing read on the host: capturable with ``out``."""
    lib = _lib.load()
    _req(state, "state", torch.uint8)
    if state.dim() != 3:
        raise ValueError(f"ground_fuse: expected state uint8 [B, GY, GX], got {tuple(state.shape)}")
    B, GY, GX = (int(v) for v in state.shape)
    if len(tuple(spec)) != 5:
        raise ValueError(f"ground_fuse: spec must be the grid's (x0, y0, cell, GX, GY), got {spec}")
    x0, y0, cell = (C.c_float(float(v)).value for v in tuple(spec)[:3])
    if (int(spec[3]), int(spec[4])) != (GX, GY) or GX < 1 or GY < 1 or B < 1:
        raise ValueError(f"ground_fuse: state {tuple(state.shape)} is not [B >= 1, GY, GX] of the grid {tuple(spec)}")
    if not (0.0 < cell < float("inf")) or not abs(x0) < float("inf") or not abs(y0) < float("inf"):
        raise ValueError(f"ground_fuse: cell must be > 0 and finite and the origin finite, got {tuple(spec)[:3]}")
    if B * GX * GY >= 1 << 31 or GX > 1 << 24 or GY > 1 << 24:
        raise ValueError(f"ground_fuse: a grid of {B} x {GY} x {GX} cells is too large (B * GX * GY below 2^31, GX and GY at most 2^24)")
    _req(motion, "motion")
    if tuple(motion.shape) != (B, 4):
        raise ValueError(f"ground_fuse: motion must be fp32 [{B}, 4] = cos, sin, tx, ty, got {tuple(motion.shape)}")
    for name, t, dtype in (("prev_evidence", prev_evidence, torch.int16), ("h_max", h_max, torch.float32), ("prev_h", prev_h, torch.float32)):
        if t is not None:
            _req(t, name, dtype)
            if t.shape != state.shape:
                raise ValueError(f"ground_fuse: {name} must have state's shape")
    for name, v, lo in (("free", free, 0), ("occupied", occupied, 0), ("decay", decay, 0), ("limit", limit, 1), ("free_at", free_at, 1),
                        ("occupied_at", occupied_at, 1)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= GROUND_FUSE_MAX:
            raise ValueError(f"ground_fuse: {name} must be an integer in {lo}..{GROUND_FUSE_MAX}, got {v}")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or set(want) - set(GROUND_FUSE_WANT):
        raise ValueError(f"ground_fuse: want must name some of {GROUND_FUSE_WANT} (got {want})")
    dtypes = {"evidence": torch.int16, "state": torch.uint8}
    shapes = {n: ((GX,) if n == "first_occupied" else (GY, GX), dtypes.get(n, torch.float32)) for n in GROUND_FUSE_WANT}
    res, at = _image_buffers(out, want, shapes, B, image_index, state.device, "ground_fuse")
    with timed("ground_fuse"):
        check(lib.ocv_ground_fuse_fwd(state.data_ptr(), _ptr(h_max), _ptr(prev_evidence), _ptr(prev_h), motion.data_ptr(), B, GX, GY, x0, y0,
                                      cell, int(free), int(occupied), int(decay), int(limit), int(free_at), int(occupied_at),
                                      at.get("evidence"), at.get("state"), at.get("h_max"), at.get("first_occupied"), _stream()),
              "ocv_ground_fuse_fwd")
    return res


GROUND_PLANE_WANT = ("pose", "stats", "count", "moments")
GROUND_PLANE_TILE = 1024              # include/objcavit_hip.h: OCV_GROUND_PLANE_TILE, candidates of the strided grid per workgroup
GROUND_PLANE_MAX_HYPOTHESES = 1024    # OCV_GROUND_PLANE_MAX_HYPOTHESES
GROUND_PLANE_BATCH = 8                # OCV_GROUND_PLANE_BATCH: the workspace pads the hypotheses to a multiple of it
GROUND_PLANE_MAX_CANDIDATES = 1 << 22  # Statement E: candidates per image (every moment then converts to float64 without rounding)
GROUND_PLANE_MOMENTS = ("N", "Sx", "Sy", "Sz", "Sxx", "Sxz", "Szz", "Sxy", "Szy")


def ground_plane(depth: torch.Tensor, K: torch.Tensor, triples: torch.Tensor, prior: torch.Tensor, tol: float = 0.05, rel_tol: float = 0.01,
                 height_range: Tuple[float, float] = (0.5, 4.0), cos_tilt: float = math.cos(0.35), min_cross: float = 1e-3,
                 min_inliers: int = 64, stride: Tuple[int, int] = (1, 1), near: float = 0.0, far: float = float("inf"),
                 confidence: Optional[torch.Tensor] = None, min_confidence: float = 0.0, depth_std: Optional[torch.Tensor] = None,
                 max_std: float = float("inf"), want: Tuple[str, ...] = ("pose", "stats"), out: Optional[dict] = None,
                 workspace: Optional[torch.Tensor] = None, image_index: int = 0) -> dict:
    """The ground plane of the final map as a camera pose (Statement E of include/objcavit_hip.h): ``depth`` fp32 [B, 1, H, W], ``K`` fp32
    [B, 4] on the device as ``ground_grid`` takes it, ``triples`` int32 [T, 3] on the device (1 <= T <= 1024 pixel triples y * W + x, one
    table for the batch: ``objcavit_amd.ground_plane.plane_triples``), ``prior`` fp32 [B, 12] on the device = a ``ground_pose``-style
    [R | t] whose row 2 is the expected up direction and which is the fallback output.  Every triple whose pixels are kept (``near`` /
    ``far``, ``confidence`` / ``depth_std`` with their thresholds, a usable camera; not the stride) spans a plane (n, h); it is a valid
    hypothesis if the triple is not degenerate (``min_cross``), n is within ``cos_tilt`` of the prior's up and h within ``height_range``.
    Each is scored by the number of candidates -- the kept pixels of the ``stride`` grid, ``ground_grid``'s points -- within ``tol`` +
    ``rel_tol`` * Z of it; the best one with at least ``min_inliers`` is refitted once from the integer moments of its inliers.  ->
    {"pose": fp32 [B, 12], the refitted plane as [right, 0; forward, 0; up, height] or the prior's bytes; "stats": int32 [B, 4] = best
    hypothesis (-1: none), its count, the refit's points, ok}, and with ``want`` naming them {"count": int32 [B, T], "moments": int64
    [B, 9] = ``GROUND_PLANE_MOMENTS``}: VIEWS of the workspace, valid until it is used again.  Every element is written.  ``out``:
    {"pose", "stats"} of caller-owned buffers [N, ...] with N >= image_index + B; the B images are written at ``image_index`` and the
    dict returned holds the whole buffers.  ``workspace``: a uint8 device tensor of at least ``ocv_ground_plane_workspace_bytes``
    (default: the stream's workspace store).  Four launches (ocv_ground_plane_fwd) on the current stream, integer atomics only (two calls
    give the same bytes), nothing read on the host: capturable with ``out`` and a warmed-up workspace."""
    lib = _lib.load()
    B, H, W = _map_and_K(depth, K, "ground_plane")
    _req(triples, "triples", torch.int32)
    if triples.dim() != 2 or int(triples.shape[1]) != 3 or not 1 <= int(triples.shape[0]) <= GROUND_PLANE_MAX_HYPOTHESES:
        raise ValueError(f"ground_plane: triples must be int32 [T, 3] with 1 <= T <= {GROUND_PLANE_MAX_HYPOTHESES}, got {tuple(triples.shape)}")
    T = int(triples.shape[0])
    _req(prior, "prior")
    if tuple(prior.shape) != (B, 12):
        raise ValueError(f"ground_plane: prior must be fp32 [{B}, 12] = a row-major 3 x 4 [R | t], got {tuple(prior.shape)}")
    _like_depth(depth, "ground_plane", confidence=confidence, depth_std=depth_std)
    sy, sx = int(stride[0]), int(stride[1])
    gh, gw = unproject_grid(H, W, (sy, sx))
    if gh * gw > GROUND_PLANE_MAX_CANDIDATES:
        raise ValueError(f"ground_plane: {gh * gw} candidates per image, at most {GROUND_PLANE_MAX_CANDIDATES} (raise the stride)")
    if not float(near) <= float(far):
        raise ValueError(f"ground_plane: near = {near} must be <= far = {far}")
    tol, rel_tol, cos_tilt, min_cross = (C.c_float(float(v)).value for v in (tol, rel_tol, cos_tilt, min_cross))
    if not 0.0 <= tol < float("inf") or not 0.0 <= rel_tol < float("inf"):
        raise ValueError(f"ground_plane: tol and rel_tol must be >= 0 and finite, got {tol}, {rel_tol}")
    if len(tuple(height_range)) != 2:
        raise ValueError(f"ground_plane: height_range must be (lo, hi), got {height_range}")
    h_lo, h_hi = (C.c_float(float(v)).value for v in height_range)
    if not h_lo <= h_hi:
        raise ValueError(f"ground_plane: height_range must be (lo, hi) with lo <= hi, got {tuple(height_range)}")
    if not 0.0 < cos_tilt <= 1.0:
        raise ValueError(f"ground_plane: cos_tilt must be in (0, 1], got {cos_tilt}")
    if not min_cross > 0.0:
        raise ValueError(f"ground_plane: min_cross must be > 0, got {min_cross}")
    if isinstance(min_inliers, bool) or int(min_inliers) != min_inliers or int(min_inliers) < 3:
        raise ValueError(f"ground_plane: min_inliers must be an integer >= 3, got {min_inliers}")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or set(want) - set(GROUND_PLANE_WANT):
        raise ValueError(f"ground_plane: want must name some of {GROUND_PLANE_WANT} (got {want})")
    shapes = {"pose": ((12,), torch.float32), "stats": ((4,), torch.int32)}
    res, at = _image_buffers(out, ("pose", "stats"), shapes, B, image_index, depth.device, "ground_plane")
    need = int(lib.ocv_ground_plane_workspace_bytes(B, T))
    if need == 0:
        raise ValueError(f"ground_plane: a batch of {B} with {T} hypotheses is too large")
    if workspace is None:
        from ._core import workspace as _workspace
        workspace = _workspace(need, depth.device, "ground_plane")
    else:
        _req(workspace, "workspace", torch.uint8)
    with timed("ground_plane"):
        check(lib.ocv_ground_plane_fwd(depth.data_ptr(), K.data_ptr(), triples.data_ptr(), prior.data_ptr(), _ptr(confidence), _ptr(depth_std),
                                       B, H, W, T, sy, sx, float(near), float(far), float(min_confidence), float(max_std), tol, rel_tol,
                                       h_lo, h_hi, cos_tilt, min_cross, int(min_inliers), at["pose"], at["stats"], workspace.data_ptr(),
                                       int(workspace.numel()), _stream()), "ocv_ground_plane_fwd")
    res = {n: t for n, t in res.items() if n in want}
    views = ground_plane_workspace_views(workspace, B, T)
    res.update({n: views[n] for n in ("moments", "count") if n in want})
    return res


def ground_plane_workspace_views(workspace: torch.Tensor, B: int, T: int) -> dict:
    """{"hypotheses": fp32 [B, Tp, 4], "moments": int64 [B, 9], "count": int32 [B, T]}: views of a ``ground_plane`` workspace (uint8,
    16-byte aligned) by the layout Statement E documents in include/objcavit_hip.h -- the ONE place on the Python side that knows it;
    Tp = T rounded up to ``GROUND_PLANE_BATCH`` (a padding hypothesis is 0, 0, 0, NaN)."""
    if workspace.dtype != torch.uint8 or workspace.dim() != 1 or workspace.data_ptr() % 16:
        raise ValueError("ground_plane: the workspace must be a flat uint8 tensor that starts 16-byte aligned")
    Tp = -(-int(T) // GROUND_PLANE_BATCH) * GROUND_PLANE_BATCH
    a, b = 16 * B * Tp, 16 * B * Tp + 72 * B
    if workspace.numel() < b + 4 * B * T:
        raise ValueError(f"ground_plane: a workspace of {workspace.numel()} bytes does not hold {B} image(s) x {T} hypotheses")
    return {"hypotheses": workspace[:a].view(torch.float32).view(B, Tp, 4), "moments": workspace[a:b].view(torch.int64).view(B, 9),
            "count": workspace[b:b + 4 * B * T].view(torch.int32).view(B, T)}


__all__ = ["ground_plane", "ground_plane_workspace_views", "GROUND_PLANE_BATCH", "GROUND_PLANE_WANT", "GROUND_PLANE_TILE", "GROUND_PLANE_MAX_HYPOTHESES", "GROUND_PLANE_MAX_CANDIDATES",
           "GROUND_PLANE_MOMENTS", "object_depth", "OBJECT_DEPTH_COLUMNS", "object_metrics", "OBJECT_METRICS_COLUMNS", "OBJECT_METRICS_MAX_BOXES", "depth_unproject",
           "unproject_grid", "UNPROJECT_TILE", "depth_normals", "normals_gather", "NORMALS_WANT", "NORMALS_MAX_RADIUS",
           "ground_grid", "GROUND_GRID_WANT", "GROUND_GRID_TILE", "GROUND_GRID_MAX_HEIGHT", "obstacles", "obstacles_set_dispatch", "OBSTACLES_WANT",
           "OBSTACLES_TILE", "OBSTACLES_MAX_LINK", "OBSTACLES_COLUMNS", "ground_fuse", "GROUND_FUSE_WANT", "GROUND_FUSE_TILE", "GROUND_FUSE_MAX"]
