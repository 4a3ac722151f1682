"""Frames in, depth out: the reference's predict mode around the model (row N5 of DESIGN.md section 6b), on the device.

``Predictor(model, args)(frames_u8)`` takes DECODED frames -- uint8 HWC, as an image decoder returns them -- and does what the
reference does between a file and its saved results (modules/GraphBinsLM.py:285-421): / image_norm_factor, KITTI benchmark crop,
ImageNet normalisation (modules/Preprocess.py:68-111, GraphBinsLM.py:45,443) in ONE launch that also writes the mirrored batch
(csrc/frame_ingest.hip); the same joint 2B-image forward as ``ValidationStep``; then the final map -- clamp, un-mirror, average,
bilinear align_corners resize to the input size, nan / inf fix (GraphBinsLM.py:159-183, metrics/MetricsPreprocess.py:17-24) -- written
out in one more launch as fp32 metres, as the datasets' 16-bit PNG values and as a colour-mapped picture (csrc/depth_finalize.hip).
With ground truth the existing metric launch adds the per-image records of a validation step.  ``flip_tta=False`` is the
reference's own predict step, which uses no test-time augmentation (GraphBinsLM.py:295-301).  ``PipelinedPredictor`` keeps several
such steps in flight on captured graphs: it and ``PipelinedValidation`` are the two subclasses of ``validation._SlotPipeline``, which
owns the slots, their streams and the range-guard handling; the pair forward is ``validation._forward_pair`` for both steps.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import hip_ops
from ._lib import HipLibraryError
from .lens import LensMap
from .object_depth import DEFAULT_QUANTILES, ObjectDepths, object_depths, pad_boxes
from .object_metrics import ObjectMetrics, object_metrics as _object_metrics
from .pixel_formats import PixelFormat, PlanarFrames
from .point_cloud import PointCloud
from .surface_normals import DEFAULT_EDGE_RATIO, DEFAULT_RADIUS, SurfaceNormals
from .ground_grid import DEFAULTS as _GROUND_DEFAULTS, GroundGrid, grid_of as _grid_of, ground_pose as _ground_pose
from .obstacles import DEFAULTS as _OBSTACLE_DEFAULTS, GRID_INPUTS as _OBSTACLE_INPUTS, Obstacles
from .ground_memory import (OPTIONS as _MEMORY_OPTIONS, FusedGrid, check_want as _memory_want, ego_motion as _ego_motion,
                            options_of as _memory_integers)
from .ground_plane import DEFAULTS as _PLANE_DEFAULTS, GroundPlane, cos_of_tilt as _cos_of_tilt, plane_triples as _plane_triples
from .validation import _SlotPipeline, _call, _depth_range, _empty_records, _forward_pair, _joint, _records, _split

IMAGENET_MEAN = (0.485, 0.456, 0.406)          # modules/GraphBinsLM.py:45
IMAGENET_STD = (0.229, 0.224, 0.225)
KB_CROP = (352, 1216)                          # modules/Preprocess.py:104-107
_DEPTH_FACTOR = {"nyu": 1000.0, "kitti": 256.0}     # params/basicParams.yaml depth_norm_factor of the two dataset blocks
WANT = ("depth", "depth_u16", "rgb8", "depth_std", "confidence")
STATS_WANT = ("depth_std", "confidence")       # the outputs that need the model's ``bin_stats``

PredictResult = namedtuple("PredictResult", ["depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence"],
                           defaults=(None, None))

Frames = Union[torch.Tensor, PlanarFrames, Sequence[Union[torch.Tensor, PlanarFrames]]]


def _dataset(args):
    return args[args.basic.dataset]


def normalisation_table(args) -> torch.Tensor:
    """fp32 [3, 256] on the host: table[c][v] = ((v / image_norm_factor) - mean[c]) / std[c], the reference's own fp32 statements in
    their order (modules/Preprocess.py:85-87: float32 array /= factor; torchvision Normalize: sub mean, div std, both fp32 tensors)
    evaluated for every value a uint8 channel can take."""
    factor = float(_dataset(args).get("image_norm_factor", 255.0))
    v = torch.arange(256, dtype=torch.float32)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).view(3, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).view(3, 1)
    return ((v / factor).view(1, 256) - mean) / std


def depth_factor(args) -> float:
    """uint16 ground-truth units per metre (modules/Preprocess.py:59-64): the dataset block's ``depth_norm_factor``, else the
    reference's constants (1000 NYU, 256 KITTI)."""
    return float(_dataset(args).get("depth_norm_factor", _DEPTH_FACTOR[args.basic.dataset]))


def kb_crop_origin(Hs: int, Ws: int) -> Tuple[int, int]:
    """(top, left) of the 352 x 1216 KITTI benchmark crop of an Hs x Ws frame (modules/Preprocess.py:104-105)."""
    if Hs < KB_CROP[0] or Ws < KB_CROP[1]:
        raise ValueError(f"the KITTI benchmark crop needs frames of at least {KB_CROP[0]} x {KB_CROP[1]}, got {Hs} x {Ws}")
    return int(Hs - KB_CROP[0]), int((Ws - KB_CROP[1]) / 2)


def colormap_table(name: str = "inferno_r") -> torch.Tensor:
    """uint8 [256, 3] on the host: the 256 RGB rows of a matplotlib colormap (imported here, lazily: nothing else needs matplotlib).
    A reversed map (``inferno_r``) is its base table read backwards."""
    import matplotlib
    import numpy as np
    lut = matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3]
    return torch.from_numpy(np.ascontiguousarray(lut)).to(torch.uint8)


def _options(keyword: str, given, keys: Tuple[str, ...], spelt: Optional[str] = None) -> dict:
    """A copy of a predictor keyword's dict; a key outside ``keys`` is refused (``spelt``: how the text lists them, default the tuple)."""
    opts = dict(given)
    bad = set(opts) - set(keys)
    if bad:
        raise ValueError(f"{keyword}: unknown option(s) {sorted(bad)}; expected some of {spelt or keys}")
    return opts


def _stride_of(opts: dict) -> Tuple[int, int]:
    """The ``stride`` option, (sy, sx) or one int, as the (sy, sx) ``hip_ops.unproject_grid`` accepts."""
    stride = opts.get("stride", (1, 1))
    stride = (int(stride), int(stride)) if isinstance(stride, int) else (int(stride[0]), int(stride[1]))
    hip_ops.unproject_grid(1, 1, stride)
    return stride


def _pixel_filter(keyword: str, opts: dict, min_depth: float, max_depth: float, uncertainty: bool = True) -> dict:
    """The options that say which pixels count: ``near`` / ``far`` (default the dataset's depth range) and, with ``uncertainty``,
    ``min_confidence`` / ``max_std`` (default: no filter)."""
    out = {"near": float(opts.get("near", min_depth)), "far": float(opts.get("far", max_depth))}
    if uncertainty:
        out.update(min_confidence=float(opts.get("min_confidence", 0.0)), max_std=float(opts.get("max_std", float("inf"))))
    if not out["near"] <= out["far"]:
        raise ValueError(f"{keyword}: near = {out['near']} must be <= far = {out['far']}")
    return out


def _readout_options(object_depth) -> Optional[dict]:
    """The ``object_depth`` keyword of both predictors: None (no readout) or a dict with some of ``quantiles`` / ``shrink``."""
    if object_depth is None:
        return None
    opts = _options("object_depth", object_depth, ("quantiles", "shrink"), "'quantiles', 'shrink'")
    return {"quantiles": tuple(opts.get("quantiles", DEFAULT_QUANTILES)), "shrink": float(opts.get("shrink", 1.0))}


def _metric_options(object_metrics) -> Optional[dict]:
    """The ``object_metrics`` keyword of both predictors: None (no per-object error) or a dict with some of ``shrink`` / ``regions``."""
    if object_metrics is None:
        return None
    opts = _options("object_metrics", object_metrics, ("shrink", "regions"), "'shrink', 'regions'")
    return {"shrink": float(opts.get("shrink", 1.0)), "regions": bool(opts.get("regions", True))}


_CLOUD_KEYS = ("stride", "near", "far", "min_confidence", "max_std", "capacity", "colour", "pixel", "normals")
_NORMAL_KEYS = ("radius", "edge_ratio", "near", "far", "picture", "valid")
_GROUND_KEYS = ("cell", "x_range", "y_range", "height", "pitch", "roll", "band", "obstacle_height", "min_points", "min_obstacle_points",
                "stride", "near", "far", "min_confidence", "max_std", "want", "pose")
_PLANE_KEYS = ("hypotheses", "rows", "seed", "tol", "rel_tol", "max_tilt", "height_range", "min_cross", "min_inliers", "height", "pitch",
               "roll", "stride", "near", "far", "min_confidence", "max_std")


def _cloud_options(point_cloud, min_depth: float, max_depth: float) -> Optional[dict]:
    """The ``point_cloud`` keyword of both predictors: None (no cloud) or a dict with some of ``_CLOUD_KEYS``.  Defaults: every pixel
    (stride (1, 1)) within the dataset's depth range, no uncertainty filter, capacity = the strided grid's size (None here: the map's
    size is known at the call), the frame's colour in every record, no pixel index, no normal per point."""
    if point_cloud is None:
        return None
    opts = _options("point_cloud", point_cloud, _CLOUD_KEYS)
    stride = _stride_of(opts)
    cap = opts.get("capacity")
    if cap is not None and int(cap) < 1:
        raise ValueError(f"point_cloud: capacity must be >= 1, got {cap}")
    return {"stride": stride, **_pixel_filter("point_cloud", opts, min_depth, max_depth), "capacity": None if cap is None else int(cap),
            "colour": bool(opts.get("colour", True)), "pixel": bool(opts.get("pixel", False))}


def _cloud_normals(point_cloud) -> bool:
    """The ``normals`` option of the ``point_cloud`` keyword (kept beside the cloud's own options, which are what they were)."""
    return point_cloud is not None and bool(dict(point_cloud).get("normals", False))


def _normal_options(surface_normals, cloud_normals: bool, min_depth: float, max_depth: float) -> Optional[dict]:
    """The ``surface_normals`` keyword of both predictors: None (no normals -- unless the cloud's ``normals=True`` asks for them, which
    implies the defaults) or a dict with some of ``_NORMAL_KEYS``.  Defaults: radius 2, edge_ratio 0.05, the dataset's depth range,
    neither the picture nor the mask."""
    if surface_normals is None:
        if not cloud_normals:
            return None
        surface_normals = {}
    opts = _options("surface_normals", surface_normals, _NORMAL_KEYS)
    radius = opts.get("radius", DEFAULT_RADIUS)
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= hip_ops.NORMALS_MAX_RADIUS:
        raise ValueError(f"surface_normals: radius must be an integer in 1..{hip_ops.NORMALS_MAX_RADIUS}, got {radius}")
    out = {"radius": int(radius), "edge_ratio": float(opts.get("edge_ratio", DEFAULT_EDGE_RATIO)),
           "picture": bool(opts.get("picture", False)), "valid": bool(opts.get("valid", False))}
    if not out["edge_ratio"] > 0.0:
        raise ValueError(f"surface_normals: edge_ratio must be > 0, got {out['edge_ratio']}")
    return {**out, **_pixel_filter("surface_normals", opts, min_depth, max_depth, uncertainty=False)}


def _plane_options(ground_plane, min_depth: float, max_depth: float) -> Optional[dict]:
    """The ``ground_plane`` keyword of both predictors: None (no estimate) or a dict with some of ``_PLANE_KEYS``.  Defaults: 256
    hypotheses drawn with seed 0 from the map's lower half, inliers within 0.05 m + 1 % of their depth, planes within 0.35 rad of the
    prior's up and 0.5 .. 4 m below the camera, at least 64 inliers; the prior a level camera 1.65 m above the ground; every pixel within
    the dataset's depth range, no uncertainty filter.  -> the options with ``cos_tilt`` and ``prior`` = the prior pose, fp32 [1, 12] on
    the host (the table of triples is made per map size, at the call)."""
    if ground_plane is None:
        return None
    opts = _options("ground_plane", ground_plane, _PLANE_KEYS)
    d = _PLANE_DEFAULTS
    T = opts.get("hypotheses", d["hypotheses"])
    if isinstance(T, bool) or int(T) != T or not 1 <= int(T) <= hip_ops.GROUND_PLANE_MAX_HYPOTHESES:
        raise ValueError(f"ground_plane: hypotheses must be an integer in 1..{hip_ops.GROUND_PLANE_MAX_HYPOTHESES}, got {T}")
    rows = opts.get("rows", d["rows"])
    if rows is not None and (len(tuple(rows)) != 2 or not 0 <= int(rows[0]) < int(rows[1])):
        raise ValueError(f"ground_plane: rows must be (first, end) with 0 <= first < end, got {rows}")
    tol, rel_tol, min_cross = (float(opts.get(n, d[n])) for n in ("tol", "rel_tol", "min_cross"))
    if not 0.0 <= tol < float("inf") or not 0.0 <= rel_tol < float("inf"):
        raise ValueError(f"ground_plane: tol and rel_tol must be >= 0 and finite, got {tol}, {rel_tol}")
    if not min_cross > 0.0:
        raise ValueError(f"ground_plane: min_cross must be > 0, got {min_cross}")
    hr = tuple(float(v) for v in opts.get("height_range", d["height_range"]))
    if len(hr) != 2 or not hr[0] <= hr[1]:
        raise ValueError(f"ground_plane: height_range must be (lo, hi) with lo <= hi, got {opts.get('height_range')}")
    n = opts.get("min_inliers", d["min_inliers"])
    if isinstance(n, bool) or int(n) != n or int(n) < 3:
        raise ValueError(f"ground_plane: min_inliers must be an integer >= 3, got {n}")
    angles = [float(opts.get(name, d[name])) for name in ("height", "pitch", "roll")]
    if not all(math.isfinite(v) for v in angles):
        raise ValueError(f"ground_plane: height, pitch and roll must be finite, got {angles}")
    out = {"hypotheses": int(T), "rows": None if rows is None else (int(rows[0]), int(rows[1])), "seed": int(opts.get("seed", d["seed"])),
           "tol": tol, "rel_tol": rel_tol, "cos_tilt": _cos_of_tilt(opts.get("max_tilt", d["max_tilt"])), "height_range": hr,
           "min_cross": min_cross, "min_inliers": int(n), "prior": _ground_pose(*angles), "stride": _stride_of(opts)}
    return {**out, **_pixel_filter("ground_plane", opts, min_depth, max_depth)}


def _ground_options(ground_grid, min_depth: float, max_depth: float, plane: bool = False) -> Optional[dict]:
    """The ``ground_grid`` keyword of both predictors: None (no grid) or a dict with some of ``_GROUND_KEYS``.  Defaults: cells of 0.1 m
    over 20 m x 40 m in front of a level camera 1.65 m above the ground, the band -0.5 .. 2.5 m, obstacles above 0.3 m, a cell known
    from one point on and occupied from three obstacle points on; every pixel within the dataset's depth range, no uncertainty filter,
    every output.  ``pose``: None (the keyword's ``height`` / ``pitch`` / ``roll``) or "plane": the pose the ``ground_plane`` keyword
    (``plane``: whether it is given; without it "plane" is refused) estimates in the same step.  -> the options with ``grid`` = (x0, y0,
    cell, GX, GY), ``pose`` = the keyword's pose, fp32 [1, 12] on the host, and ``pose_from`` = None or "plane"."""
    if ground_grid is None:
        return None
    opts = _options("ground_grid", ground_grid, _GROUND_KEYS)
    pose_from = opts.get("pose")
    if pose_from not in (None, "plane"):
        raise ValueError(f"ground_grid: pose must be None (the keyword's height / pitch / roll) or 'plane', got {pose_from!r}")
    if pose_from == "plane" and not plane:
        raise ValueError("ground_grid: pose='plane' needs the ground_plane= keyword beside it (ground_plane={} takes the defaults)")
    d = _GROUND_DEFAULTS
    stride = _stride_of(opts)
    band = tuple(float(v) for v in opts.get("band", d["band"]))
    limit = hip_ops.GROUND_GRID_MAX_HEIGHT
    if len(band) != 2 or not band[0] <= band[1] or not abs(band[0]) <= limit or not abs(band[1]) <= limit:
        raise ValueError(f"ground_grid: band must be (lo, hi) with lo <= hi, both within +-{limit}, got {opts.get('band')}")
    counts = {}
    for name in ("min_points", "min_obstacle_points"):
        v = opts.get(name, d[name])
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise ValueError(f"ground_grid: {name} must be an integer >= 1, got {v}")
        counts[name] = int(v)
    want = opts.get("want", hip_ops.GROUND_GRID_WANT)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or set(want) - set(hip_ops.GROUND_GRID_WANT):
        raise ValueError(f"ground_grid: want must name some of {hip_ops.GROUND_GRID_WANT} (got {want})")
    angles = [float(opts.get(name, d[name])) for name in ("height", "pitch", "roll")]
    if not all(math.isfinite(v) for v in angles):
        raise ValueError(f"ground_grid: height, pitch and roll must be finite, got {angles}")
    out = {"grid": _grid_of(opts.get("cell", d["cell"]), opts.get("x_range", d["x_range"]), opts.get("y_range", d["y_range"])),
           "pose": _ground_pose(*angles), "band": band, "obstacle_height": float(opts.get("obstacle_height", d["obstacle_height"])),
           "stride": stride, "want": tuple(n for n in hip_ops.GROUND_GRID_WANT if n in want), "pose_from": pose_from, **counts}
    if out["obstacle_height"] != out["obstacle_height"]:
        raise ValueError("ground_grid: obstacle_height is NaN")
    return {**out, **_pixel_filter("ground_grid", opts, min_depth, max_depth)}


_OBSTACLE_KEYS = ("link", "min_cells", "min_obstacle_points", "capacity", "labels")


def _obstacle_options(obstacles, ground: bool) -> Optional[dict]:
    """The ``obstacles`` keyword of both predictors: None (no list) or a dict with some of ``_OBSTACLE_KEYS``.  Defaults: 8-connectivity
    (link 1), obstacles of at least two cells, no threshold on their obstacle points, 64 rows per image, no label map.  It reads the grid
    of the same step (``ground``: whether the ``ground_grid`` keyword is given; without it the keyword is refused)."""
    if obstacles is None:
        return None
    opts = _options("obstacles", obstacles, _OBSTACLE_KEYS)
    if not ground:
        raise ValueError("obstacles: the list is made from the grid of the same step -- it needs the ground_grid= keyword beside it "
                         "(ground_grid={} takes the defaults)")
    out = {}
    for name, lo in (("link", 1), ("min_cells", 1), ("min_obstacle_points", 0), ("capacity", 1)):
        v = opts.get(name, _OBSTACLE_DEFAULTS[name])
        if isinstance(v, bool) or int(v) != v or int(v) < lo:
            raise ValueError(f"obstacles: {name} must be an integer >= {lo}, got {v}")
        out[name] = int(v)
    if out["link"] > hip_ops.OBSTACLES_MAX_LINK:
        raise ValueError(f"obstacles: link must be in 1..{hip_ops.OBSTACLES_MAX_LINK}, got {out['link']}")
    out["labels"] = bool(opts.get("labels", _OBSTACLE_DEFAULTS["labels"]))
    return out


_MEMORY_KEYS = _MEMORY_OPTIONS + ("obstacles", "want")


def _memory_options(ground_memory, ground: bool) -> Optional[dict]:
    """The ``ground_memory`` keyword of both predictors: None (no memory) or a dict with some of ``_MEMORY_KEYS``.  Defaults: those of
    ``objcavit_amd.ground_memory`` (free 2, occupied 4, decay 1, limit 32, free_at 4, occupied_at 6), every output, and the obstacle list
    (where the ``obstacles`` keyword asks for one) made from the frame's grid as without the memory; ``obstacles=True`` makes it from the
    FUSED map instead.  It reads the grid of the same step (``ground``: whether the ``ground_grid`` keyword is given; without it the
    keyword is refused)."""
    if ground_memory is None:
        return None
    opts = _options("ground_memory", ground_memory, _MEMORY_KEYS)
    if not ground:
        raise ValueError("ground_memory: the memory fuses the grid of every step -- it needs the ground_grid= keyword beside it "
                         "(ground_grid={} takes the defaults)")
    return {**_memory_integers(opts), "obstacles": bool(opts.get("obstacles", False)),
            "want": _memory_want(opts.get("want", hip_ops.GROUND_FUSE_WANT))}


def _cloud_want(cloud: Optional[dict]) -> Tuple[str, ...]:
    """The maps a point cloud's (or a ground grid's) filters read beyond "depth": they are made for it (and ``bin_stats`` turned on)
    even when ``want`` leaves them out."""
    if cloud is None:
        return ()
    return (("confidence",) if cloud["min_confidence"] > 0.0 else ()) + (("depth_std",) if cloud["max_std"] < float("inf") else ())


def _filter_maps(maps: dict, o: dict) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(the "confidence" map, the "depth_std" map) of a step, each only if the readout's own threshold reads it."""
    return (maps.get("confidence") if o["min_confidence"] > 0.0 else None), (maps.get("depth_std") if o["max_std"] < float("inf") else None)


def _per_frame(ends: "_Ends", step: "_Step", device, conf: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None):
    """What a readout that takes intrinsics needs per entry of ``step.frames`` (a list of differently sized frames has an origin -- hence a
    principal point -- per frame): (the frames, their slice of the batch, top, left of their window, K of the slice shifted by that
    origin -- ``point_cloud.shift_intrinsics``'s statement, the offsets cached on the device --, the slices of ``conf`` / ``std`` or None)."""
    i = 0
    for f in step.frames:
        s = slice(i, i + int(f.shape[0]))
        top, left = ends.origin_of(f)
        yield f, s, top, left, step.K[s] - ends._shift(device, top, left), None if conf is None else conf[s], None if std is None else std[s]
        i = s.stop


# The outputs behind the final map.  Each is run by one function (ends, step, made) -> its result, on the current stream; ``made`` holds
# the step's final ``maps``, the names the caller ``asked`` for, the model's ``pred`` / ``mirror`` maps and the ground truth ``depth_gt``,
# and under its attribute name the result of every readout that ran in front.
def _run_errors(ends, step, made) -> ObjectMetrics:
    """The depth error per box / region, right behind the metric launch, from the tensors that launch reads."""
    return _object_metrics(made["pred"], made["depth_gt"], step.boxes, ends.args, pred_mirror=made["mirror"], **ends.errors)


def _run_objects(ends, step, made) -> ObjectDepths:
    """The per-object readout of the final map; ``std_mean`` is filled when the caller's ``want`` names "depth_std"."""
    maps = made["maps"]
    return object_depths(maps["depth"], step.boxes, depth_std=maps.get("depth_std") if "depth_std" in made["asked"] else None, **ends.readout)


def _run_cloud(ends, step, made) -> PointCloud:
    """The point cloud of a step's final map: one launch pair per entry of ``step.frames`` into one set of buffers.  With a
    ``pixel_format`` other than rgb24 the colour is read from the window's RGB24 copy, made by one more launch in front
    (``hip_ops.frames_to_rgb24``): bytes 12 - 14 of a record are Statement P's R, G, B.  The pixel index is made for the cloud's
    ``normals=True`` even when ``pixel`` was not asked for; it is then left in ``made["pixel"]`` and not handed out with the cloud."""
    c, maps = ends.cloud, made["maps"]
    depth = maps["depth"]
    B, _, H, W = (int(v) for v in depth.shape)
    gh, gw = hip_ops.unproject_grid(H, W, c["stride"])
    cap = gh * gw if c["capacity"] is None else c["capacity"]
    dev = depth.device
    bufs = {"points": torch.empty((B, cap, 4), dtype=torch.float32, device=dev),
            "counts": torch.empty((B,), dtype=torch.int32, device=dev), "total": torch.empty((B,), dtype=torch.int32, device=dev)}
    want_pixel = c["pixel"] or ends.cloud_normals
    if want_pixel:
        bufs["pixel"] = torch.empty((B, cap), dtype=torch.int32, device=dev)
    recolour = c["colour"] and (ends.lens is not None or (ends.fmt is not None and ends.fmt.name != "rgb24"))
    n = 0
    # byte 15 of a record is the confidence whenever that map is made, whatever the threshold
    for f, s, top, left, K, conf, std in _per_frame(ends, step, dev, maps.get("confidence"), _filter_maps(maps, c)[1]):
        colour, ctop, cleft = (f if c["colour"] else None), top, left
        if recolour:
            colour, ctop, cleft = ends.rgb24_of(step.frames, n, top, left, (H, W)), 0, 0
        n += 1
        hip_ops.depth_unproject(depth[s], K, cap, stride=c["stride"], near=c["near"], far=c["far"], confidence=conf,
                                min_confidence=c["min_confidence"], depth_std=std, max_std=c["max_std"], frames=colour, top=ctop,
                                left=cleft, want_pixel=want_pixel, out=bufs, image_index=s.start)
    made["pixel"] = bufs.get("pixel")
    return PointCloud(bufs["points"], bufs["counts"], bufs["total"], bufs.get("pixel") if c["pixel"] else None)


def _run_normals(ends, step, made) -> SurfaceNormals:
    """The surface normals of a step's final map (Statement N, objcavit_amd/surface_normals.py): one launch per entry of ``step.frames``
    into one set of buffers; they read the final map only, so the frames' sizes, ``resize`` and ``pixel_format`` do not matter.  With the
    cloud's ``normals=True`` one more launch gathers a normal per point of the cloud through its pixel index."""
    o, depth = ends.normals, made["maps"]["depth"]
    B, _, H, W = (int(v) for v in depth.shape)
    dev = depth.device
    want = ("normals",) + (("rgb8",) if o["picture"] else ()) + (("valid",) if o["valid"] else ())
    shapes = {"normals": ((B, 3, H, W), torch.float32), "rgb8": ((B, H, W, 3), torch.uint8), "valid": ((B, H, W), torch.uint8)}
    bufs = {n: torch.empty(shapes[n][0], dtype=shapes[n][1], device=dev) for n in want}
    for _, s, _, _, K, _, _ in _per_frame(ends, step, dev):
        hip_ops.depth_normals(depth[s], K, radius=o["radius"], near=o["near"], far=o["far"], edge_ratio=o["edge_ratio"], want=want,
                              out=bufs, image_index=s.start)
    points, cloud = None, made.get("points")
    if cloud is not None and ends.cloud_normals:
        points = hip_ops.normals_gather(bufs["normals"], made["pixel"], cloud.counts)
    return SurfaceNormals(bufs["normals"], bufs.get("rgb8"), bufs.get("valid"), points)


def _run_plane(ends, step, made) -> GroundPlane:
    """The ground plane of a step's final map (Statement E, objcavit_amd/ground_plane.py): one call (four launches) per entry of
    ``step.frames`` into one pair of buffers.  The table of triples (per map size) and the prior (per batch size) are made once per
    device and kept."""
    o, maps = ends.plane, made["maps"]
    depth = maps["depth"]
    B, _, H, W = (int(v) for v in depth.shape)
    dev = depth.device
    ent = ends._on(dev, False)
    tkey, pkey = ("plane_triples", H, W), ("plane_prior", B)
    if tkey not in ent:
        ent[tkey] = _plane_triples(H, W, o["hypotheses"], o["rows"], o["seed"]).to(dev)
    if pkey not in ent:
        ent[pkey] = o["prior"].expand(B, 12).contiguous().to(dev)
    triples, prior = ent[tkey], ent[pkey]
    bufs = {"pose": torch.empty((B, 12), dtype=torch.float32, device=dev), "stats": torch.empty((B, 4), dtype=torch.int32, device=dev)}
    for _, s, _, _, K, conf, std in _per_frame(ends, step, dev, *_filter_maps(maps, o)):
        hip_ops.ground_plane(depth[s], K, triples, prior[s], tol=o["tol"], rel_tol=o["rel_tol"], height_range=o["height_range"],
                             cos_tilt=o["cos_tilt"], min_cross=o["min_cross"], min_inliers=o["min_inliers"], stride=o["stride"],
                             near=o["near"], far=o["far"], confidence=conf, min_confidence=o["min_confidence"], depth_std=std,
                             max_std=o["max_std"], out=bufs, image_index=s.start)
    return GroundPlane(bufs["pose"], bufs["stats"])


def _run_ground(ends, step, made) -> GroundGrid:
    """The bird's-eye occupancy grid of a step's final map (Statement G, objcavit_amd/ground_grid.py): one call (three launches) per
    entry of ``step.frames`` into one set of buffers, posed by ``step.pose`` ([B, 12], ``camera_pose=``) or, without it, by the pose the
    ``ground_plane`` readout has just estimated (``pose="plane"``: its device tensor, read by the grid's launches behind it on the same
    stream) or by the keyword's pose for every image (uploaded once per device)."""
    o, maps = ends.ground, made["maps"]
    depth, pose = maps["depth"], step.pose
    B = int(depth.shape[0])
    dev = depth.device
    x0, y0, cell, GX, GY = o["grid"]
    if pose is None and o["pose_from"] == "plane":
        pose = made["plane"].pose
    if pose is None:
        ent = ends._on(dev, False)
        key = ("ground_pose", B)
        if key not in ent:
            ent[key] = o["pose"].expand(B, 12).contiguous().to(dev)
        pose = ent[key]
    dtypes = {"count": torch.int32, "obstacle": torch.int32, "state": torch.uint8}
    # the obstacle list reads state, count, obstacle and h_max, the memory state and h_max: they are made for them even when the grid's
    # ``want`` leaves them out (and are then not handed out) -- the ``_cloud_want`` rule
    extra = (_OBSTACLE_INPUTS if ends.obstacles is not None else ()) + (("state", "h_max") if ends.memory is not None else ())
    make = tuple(n for n in hip_ops.GROUND_GRID_WANT if n in o["want"] or n in extra)
    bufs = {n: torch.empty((B, GX) if n == "first_occupied" else (B, GY, GX), dtype=dtypes.get(n, torch.float32), device=dev)
            for n in make}
    for _, s, _, _, K, conf, std in _per_frame(ends, step, dev, *_filter_maps(maps, o)):
        hip_ops.ground_grid(depth[s], K, pose[s], o["grid"], band=o["band"], obstacle_height=o["obstacle_height"],
                            min_points=o["min_points"], min_obstacle_points=o["min_obstacle_points"], stride=o["stride"], near=o["near"],
                            far=o["far"], confidence=conf, min_confidence=o["min_confidence"], depth_std=std, max_std=o["max_std"],
                            want=make, out=bufs, image_index=s.start)
    made["ground_buffers"] = bufs
    return GroundGrid(*(bufs.get(n) if n in o["want"] else None for n in hip_ops.GROUND_GRID_WANT), x0=x0, y0=y0, cell=cell)


def _run_memory(ends, step, made) -> FusedGrid:
    """The ground memory's step (Statement F, objcavit_amd/ground_memory.py): one launch for the batch behind the grid's, on the grid's
    ``state`` and ``h_max``, the evidence and fused ``h_max`` of the PREVIOUS step (``ends._memory``) and the step's motion; the outputs
    are fresh tensors, and the memory then holds this step's.  The previous step may have run on another stream (a pipeline's slots):
    the current stream waits for the event that step recorded behind its launch, this step records its own, and the previous step's
    tensors are recorded for the current stream.  Only this launch is ordered; everything in front of it overlaps as before.
    A step that runs a SECOND time (``PipelinedPredictor.collect`` re-runs a step whose fp16 range guard tripped, after the steps
    behind it have run) is fused again from the previous evidence and motion it had read the first time -- kept in ``step.memory`` --
    and does not advance the memory: its own ``FusedGrid`` is the re-run's, but THE STEPS BEHIND IT HAVE FUSED ITS FIRST MAP."""
    o, g, rec = ends.memory, made["ground_buffers"], step.memory
    state = g["state"]
    B, dev = int(state.shape[0]), state.device
    x0, y0, cell, GX, GY = ends.ground["grid"]
    again = "prev" in rec
    if not again:
        if rec["reset"]:
            ends._memory = None
        rec["prev"] = ends._memory                           # None, or (evidence, h_max, the event behind the launch that wrote them)
    prev = rec["prev"]
    motion = rec["motion"]
    if motion is None:
        ent = ends._on(dev, False)
        key = ("ego_identity", B)
        if key not in ent:
            ent[key] = _ego_motion().expand(B, 4).contiguous().to(dev)
        motion = ent[key]
    cur = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
    if prev is not None and tuple(prev[0].shape) != tuple(state.shape):
        raise ValueError(f"ground_memory: the batch changed from {int(prev[0].shape[0])} to {B} stream(s) (pass reset=True)")
    if prev is not None and not again and prev[2] is not None and cur is not None:
        cur.wait_event(prev[2])
    make = tuple(n for n in hip_ops.GROUND_FUSE_WANT if n in o["want"] or n in ("evidence", "h_max") or (o["obstacles"] and n == "state"))
    res = hip_ops.ground_fuse(state, (x0, y0, cell, GX, GY), motion, prev_evidence=None if prev is None else prev[0], h_max=g["h_max"],
                              prev_h=None if prev is None else prev[1], want=make, **{n: o[n] for n in _MEMORY_OPTIONS})
    if not again:
        event = None
        if cur is not None:
            event = torch.cuda.Event()
            event.record(cur)
            for t in (prev or ())[:2]:
                t.record_stream(cur)                         # made on the previous step's stream, read by this launch on this one
        ends._memory = (res["evidence"], res["h_max"], event)
    made["memory_buffers"] = res
    return FusedGrid(*(res[n] if n in o["want"] else None for n in hip_ops.GROUND_FUSE_WANT), x0=x0, y0=y0, cell=cell)


def _run_obstacles(ends, step, made) -> Obstacles:
    """The obstacle list of a step's grid (Statement O, objcavit_amd/obstacles.py): one call (at most seven launches) for the batch, on
    the grid's own buffers behind its launches on the same stream -- the grid's cells are per image whatever the frames' sizes.  With
    ``ground_memory=dict(obstacles=True)`` it reads the FUSED ``state`` and ``h_max`` of the step instead (``count`` / ``obstacle`` null:
    the rows' point counts are 0)."""
    o, g = ends.obstacles, made["ground_buffers"]
    if ends.memory is not None and ends.memory["obstacles"]:
        f = made["memory_buffers"]
        g = {"state": f["state"], "count": None, "obstacle": None, "h_max": f["h_max"]}
    x0, y0, cell, GX, GY = ends.ground["grid"]
    want = tuple(n for n in hip_ops.OBSTACLES_WANT if n != "labels" or o["labels"])
    res = hip_ops.obstacles(g["state"], (x0, y0, cell, GX, GY), count=g["count"], obstacle=g["obstacle"], h_max=g["h_max"], link=o["link"],
                            min_cells=o["min_cells"], min_obstacle_points=o["min_obstacle_points"], capacity=o["capacity"], want=want)
    return Obstacles(*(res.get(n) for n in hip_ops.OBSTACLES_WANT), x0=x0, y0=y0, cell=cell)


# One entry per output behind the final map, IN THE ORDER OF THEIR LAUNCHES.  keyword: the predictors' keyword; attr: the attribute of the
# result that holds the output (None when it did not run); options: the attribute of ``_Ends`` that holds the parsed keyword; parse:
# (the predictors' readout keywords, min_depth, max_depth) -> those options or None; maps: options -> the final maps it reads, which are
# made for it even when ``want`` leaves them out; needs: the fields of the step record it cannot run without; run: above; streamed: which
# of its result's tensors are made on a pipeline slot's stream and read by the caller on another, so that ``submit`` must
# ``record_stream`` them -- the per-object readout's table is NOT among them, as it never was.
_Readout = namedtuple("_Readout", ["keyword", "attr", "options", "parse", "maps", "needs", "run", "streamed"])
READOUTS = (
    _Readout("object_metrics", "object_metrics", "errors", lambda kw, lo, hi: _metric_options(kw["object_metrics"]),
             lambda o: (), ("depth_gt", "boxes"), _run_errors, slice(2)),
    _Readout("object_depth", "objects", "readout", lambda kw, lo, hi: _readout_options(kw["object_depth"]),
             lambda o: ("depth",), ("boxes",), _run_objects, slice(0)),
    _Readout("point_cloud", "points", "cloud", lambda kw, lo, hi: _cloud_options(kw["point_cloud"], lo, hi),
             lambda o: ("depth",) + _cloud_want(o), ("K",), _run_cloud, slice(None)),
    _Readout("surface_normals", "normals", "normals",
             lambda kw, lo, hi: _normal_options(kw["surface_normals"], _cloud_normals(kw["point_cloud"]), lo, hi),
             lambda o: ("depth",), ("K",), _run_normals, slice(None)),
    _Readout("ground_plane", "plane", "plane", lambda kw, lo, hi: _plane_options(kw["ground_plane"], lo, hi),
             lambda o: ("depth",) + _cloud_want(o), ("K",), _run_plane, slice(None)),
    _Readout("ground_grid", "ground", "ground", lambda kw, lo, hi: _ground_options(kw["ground_grid"], lo, hi, kw["ground_plane"] is not None),
             lambda o: ("depth",) + _cloud_want(o), ("K",), _run_ground, slice(None)),
)
# The readouts of a READOUT: they read no final map but the buffers of an entry above, of the same step on the same stream, and run
# behind all of READOUTS in this order.  ``obstacles`` reads the grid's and is refused without the ``ground_grid`` keyword.
DERIVED_READOUTS = (
    _Readout("obstacles", "obstacles", "obstacles", lambda kw, lo, hi: _obstacle_options(kw["obstacles"], kw["ground_grid"] is not None),
             lambda o: (), ("K",), _run_obstacles, slice(5)),
)
ALL_READOUTS = READOUTS + DERIVED_READOUTS
# The readouts that carry state from one step to the next.  They run behind READOUTS and IN FRONT OF DERIVED_READOUTS (the obstacle list
# may read the fused map), so they have a table of their own: ``ALL_READOUTS`` ends with the grid and its list, as it did.
# ``ground_memory`` reads the grid's buffers of the same step and the memory of the previous one (``_Ends._memory``).
TEMPORAL_READOUTS = (
    _Readout("ground_memory", "ground_memory", "memory", lambda kw, lo, hi: _memory_options(kw["ground_memory"], kw["ground_grid"] is not None),
             lambda o: (), ("K",), _run_memory, slice(4)),
)
RUN_ORDER = READOUTS + TEMPORAL_READOUTS + DERIVED_READOUTS          # every readout, in the order of their launches
for _r in RUN_ORDER:
    setattr(PredictResult, _r.attr, None)          # an ATTRIBUTE, not a field: ``PredictResult``'s fields are what they were


class _ObjectsResult(PredictResult):
    """A ``PredictResult`` -- same fields, same tuple -- whose attributes named in ``READOUTS`` (``objects`` / ``points`` /
    ``object_metrics`` / ``normals`` / ``plane`` / ``ground``) or in ``DERIVED_READOUTS`` (``obstacles``) hold the step's ``ObjectDepths`` /
    ``PointCloud`` / ``ObjectMetrics`` / ``SurfaceNormals`` / ``GroundPlane`` / ``GroundGrid`` / ``Obstacles``, and ``ground_memory``
    (``TEMPORAL_READOUTS``) the step's ``FusedGrid``; each is a keyword of its own and survives ``_replace``."""

    def __new__(cls, *fields, **kw):
        made = {r.attr: kw.pop(r.attr, None) for r in RUN_ORDER}
        self = super().__new__(cls, *fields, **kw)
        self.__dict__.update(made)
        return self

    def _replace(self, **kw):
        return _ObjectsResult(*PredictResult(*self)._replace(**kw), **{r.attr: getattr(self, r.attr) for r in RUN_ORDER})


class _Step(namedtuple("_Step", ["depth_gt", "boxes", "K", "frames", "pose", "size", "memory"], defaults=(None,))):
    """The inputs of one step beside the forward's (``_Ends.step``): the ground truth as the caller gave it, the boxes as (xywh, counts),
    the intrinsics of the source frames [B, 4] and the camera poses [B, 12] on the device (each None when absent or when no keyword
    reads it), the frame batches and the step's final size; ``memory``: None without the ``ground_memory`` keyword, else the step's
    part of it -- {"motion": fp32 [B, 4] on the device or None (the identity), "reset": bool} and, once the step has run, "prev": what
    it read of the previous step (``_run_memory``), so that a re-run reads the same.  ``PipelinedPredictor`` hands it through its slot
    pipeline in the place of the ground truth."""
    __slots__ = ()

    def held(self) -> List[torch.Tensor]:
        """The tensors among them that a pipeline slot's launches read (the frames' own are held with the ingest's)."""
        gt = [self.depth_gt] if isinstance(self.depth_gt, torch.Tensor) else list(self.depth_gt or [])
        return gt + list(self.boxes or ()) + [t for t in (self.K, self.pose, (self.memory or {}).get("motion")) if t is not None]


def _window(args, Hs: int, Ws: int, crop) -> Tuple[int, int, int, int]:
    """(top, left, H, W): ``crop`` as given, else the dataset's rule -- the KITTI benchmark crop with ``do_kb_crop``, else the frame."""
    if crop is not None:
        top, left, H, W = (int(c) for c in crop)
        return top, left, H, W
    if _dataset(args).get("do_kb_crop", False):
        return kb_crop_origin(Hs, Ws) + KB_CROP
    return 0, 0, Hs, Ws


def _model_size(resize) -> Optional[Tuple[int, int]]:
    """The ``resize`` keyword of both predictors: None (the window is the model's input, as it is) or the model's (H, W)."""
    if resize is None:
        return None
    H, W = (int(v) for v in resize)
    if H < 1 or W < 1:
        raise ValueError(f"resize: the model's (H, W) must be >= 1, got {tuple(resize)}")
    return H, W


def fit_window(Hs: int, Ws: int, H: int, W: int) -> Tuple[int, int, int, int]:
    """(top, left, Hw, Ww): the largest centred window of an Hs x Ws frame with the aspect ratio of the model's H x W -- the ``crop`` to
    pass beside ``resize=(H, W)``.  Integer arithmetic: the frame's full height with Ww = floor(Hs * W / H) when the frame is at least as
    wide as the model's shape (Ws * H >= Hs * W), else its full width with Hw = floor(Ws * H / W); the cut side is ROUNDED DOWN (the
    window never leaves the frame; its ratio is off by less than one pixel of that side) and never below 1; top / left =
    floor(margin / 2), so an odd margin leaves the extra pixel at the bottom / right."""
    Hs, Ws, H, W = int(Hs), int(Ws), int(H), int(W)
    if min(Hs, Ws, H, W) < 1:
        raise ValueError(f"fit_window: sizes must be >= 1, got {Hs} x {Ws} -> {H} x {W}")
    if Ws * H >= Hs * W:
        Hw, Ww = Hs, max(1, Hs * W // H)
    else:
        Hw, Ww = max(1, Ws * H // W), Ws
    return (Hs - Hw) // 2, (Ws - Ww) // 2, Hw, Ww


def boxes_to_model(xywh, window_size: Tuple[int, int], model_size: Tuple[int, int]):
    """Detector boxes (centre x, centre y, width, height, ...) in pixels of the WINDOW -> pixels of the model's input, for the model's
    object provider under ``resize``: cx, w times W / Ww and cy, h times H / Hw; columns beyond the fourth and the <UNK> box
    (-1, -1, -1, -1) pass through unchanged.  ``xywh``: a tensor [..., >= 4] (-> a new tensor), or a list of such tensors / None (-> a
    list, None kept).  The boxes of ``boxes=`` (readout, object metrics) are NOT scaled: the final map has the window's size."""
    if xywh is None:
        return None
    if not isinstance(xywh, torch.Tensor):
        return [boxes_to_model(b, window_size, model_size) for b in xywh]
    if xywh.dim() < 1 or xywh.shape[-1] < 4:
        raise ValueError(f"boxes_to_model: expected [..., >= 4] boxes, got {tuple(xywh.shape)}")
    (Hw, Ww), (H, W) = (int(v) for v in window_size), (int(v) for v in model_size)
    scale = torch.ones(xywh.shape[-1], dtype=torch.float64)
    scale[0] = scale[2] = W / Ww
    scale[1] = scale[3] = H / Hw
    out = xywh * scale.to(device=xywh.device, dtype=xywh.dtype)
    unk = (xywh[..., :4] == -1).all(-1, keepdim=True)
    return torch.where(unk, xywh, out)


def _frame_list(frames: Frames, what: str, dims: int) -> List[torch.Tensor]:
    """A batch tensor, or a list of single frames of varying size, as a list of [b, ...] batch tensors."""
    if isinstance(frames, torch.Tensor):
        if frames.dim() != dims:
            raise ValueError(f"{what}: expected a [B, Hs, Ws{', 3' if dims == 4 else ''}] tensor or a list of single frames, got {tuple(frames.shape)}")
        return [frames]
    out = []
    for f in frames:
        if not isinstance(f, torch.Tensor) or f.dim() != dims - 1:
            raise ValueError(f"{what}: a list holds single frames [Hs, Ws{', 3' if dims == 4 else ''}]")
        out.append(f.unsqueeze(0))
    if not out:
        raise ValueError(f"{what}: empty list")
    return out


def _frames_of(frames: Frames, what: str, fmt: Optional[PixelFormat]) -> list:
    """``_frame_list`` for the ``pixel_format`` keyword: without it (None) today's packed RGB frames; a packed format takes tensors
    [B, Hs, Ws, 3 | 4] (or a list of single frames [Hs, Ws, 3 | 4]); a 4:2:0 format takes a ``PlanarFrames`` or a list of them (each a
    frame, or a batch, of its own size)."""
    if fmt is None:
        return _frame_list(frames, what, 4)
    if not fmt.planar:
        out = _frame_list(frames, what, 4)
        for f in out:
            if int(f.shape[3]) != fmt.channels:
                raise ValueError(f"{what}: {fmt.name} frames have {fmt.channels} bytes per pixel, got {tuple(f.shape)}")
        return out
    out = [frames] if isinstance(frames, PlanarFrames) else list(frames)
    if not out:
        raise ValueError(f"{what}: empty list")
    for f in out:
        if not isinstance(f, PlanarFrames) or f.name != fmt.name:
            raise ValueError(f"{what}: {fmt.name} frames are a PlanarFrames({fmt.name!r}, ...) or a list of them, got "
                             f"{f if isinstance(f, PlanarFrames) else type(f).__name__}")
    return out


def _tensors_of(frames: list) -> List[torch.Tensor]:
    """Every tensor a list of frame batches is made of: the frames themselves, or the planes of ``PlanarFrames``."""
    return [t for f in frames for t in (f.planes if isinstance(f, PlanarFrames) else (f,))]


class _Ends:
    """What both predictors share: the device tables and the two ends around a forward."""

    def __init__(self, args, *, flip_tta: bool = True, loss: bool = False, colormap=None, vmin=None, vmax=None, u16_scale=None, crop=None,
                 resize=None, pixel_format=None, lens=None, **readouts):
        """The predictors' keywords, by keyword; ``readouts``: those named in ``ALL_READOUTS``."""
        self.args, self.flip_tta, self.loss, self.crop = args, flip_tta, loss, crop
        self.fmt = None if pixel_format is None else PixelFormat.of(pixel_format)      # None: rgb24 through the rgb24 calls
        self.resize = _model_size(resize)
        if lens is not None and not isinstance(lens, LensMap):
            raise TypeError(f"lens: expected a LensMap (objcavit_amd.lens), got {type(lens).__name__}")
        if lens is not None and crop is not None:
            raise ValueError("lens: the map's window is the window -- crop= cannot be given beside lens= (build the map for the window wanted)")
        self.lens = lens
        self._rect = (None, None)                    # (the frame list last ingested through the lens with ``resize``, its RGB24 copies)
        self.min_depth, self.max_depth = _depth_range(args)
        given = {r.keyword: readouts.pop(r.keyword, None) for r in RUN_ORDER}
        if readouts:
            raise TypeError(f"_Ends: unknown keyword(s) {sorted(readouts)}")
        for r in RUN_ORDER:                          # .errors, .readout, .cloud, .normals, .plane, .ground, .memory, .obstacles: the parsed keyword or None
            setattr(self, r.options, r.parse(given, self.min_depth, self.max_depth))
        self.cloud_normals = _cloud_normals(given["point_cloud"])          # a normal per point of the cloud
        self.readouts = tuple((r, r.maps(getattr(self, r.options))) for r in RUN_ORDER if getattr(self, r.options) is not None)
        self._memory = None                          # ``ground_memory``: (evidence, h_max, event) of the newest step, None before the first
        self.vmin = self.min_depth if vmin is None else float(vmin)
        self.vmax = self.max_depth if vmax is None else float(vmax)
        self.u16_scale = depth_factor(args) if u16_scale is None else float(u16_scale)
        self._table_host = normalisation_table(args)
        self._colormap_host = colormap
        self._dev = {}

    def _on(self, device: torch.device, want_cmap: bool):
        key = (device.type, device.index)
        ent = self._dev.get(key)
        if ent is None:
            ent = self._dev[key] = {"table": self._table_host.to(device)}
        if want_cmap and "cmap" not in ent:
            cm = self._colormap_host
            if cm is None or isinstance(cm, str):
                cm = colormap_table(cm or "inferno_r")
            ent["cmap"] = cm.to(device=device, dtype=torch.uint8).contiguous()
        return ent

    def origin_of(self, f) -> Tuple[int, int]:
        """(top, left) of a frame batch's window in the pixels its intrinsics are given in: under ``lens`` the rectified window itself."""
        if self.lens is not None:
            return 0, 0
        return _window(self.args, int(f.shape[1]), int(f.shape[2]), self.crop)[:2]

    def window_of(self, frames: List[torch.Tensor]) -> Tuple[int, int]:
        if self.lens is not None:
            for f in frames:
                if (int(f.shape[1]), int(f.shape[2])) != self.lens.source_size:
                    raise ValueError(f"lens: the map was made for {self.lens.source_size[0]} x {self.lens.source_size[1]} frames, got "
                                     f"{int(f.shape[1])} x {int(f.shape[2])}")
            return self.lens.window_size
        sizes = {_window(self.args, int(f.shape[1]), int(f.shape[2]), self.crop)[2:] for f in frames}
        if len(sizes) != 1:
            raise ValueError(f"frames of one batch must crop to one size, got {sorted(sizes)}")
        return sizes.pop()

    def model_size(self, frames: List[torch.Tensor]) -> Tuple[int, int]:
        """The size the model sees: ``resize``, else the window's."""
        return self.window_of(frames) if self.resize is None else self.resize

    def taps_of(self, frames: List[torch.Tensor]):
        """With ``resize``: the device tap tables of the step's window size, uploaded on the current stream when the size is first seen
        on that device and kept (``hip_ops.frame_resize_taps``); None without."""
        if self.resize is None:
            return None
        Hw, Ww = self.window_of(frames)
        if not hip_ops.frame_resize_supported(Hw, Ww, *self.resize):
            raise ValueError(f"resize: a {Hw} x {Ww} window to {self.resize[0]} x {self.resize[1]} shrinks by more than "
                             f"{hip_ops.FRAME_RESIZE_MAX_RATIO} along an axis (hip_ops.frame_resize_ingest)")
        return hip_ops.frame_resize_taps(frames[0].device, Hw, Ww, *self.resize)

    def frames_of(self, frames: Frames, what: str) -> list:
        return _frames_of(frames, what, self.fmt)

    def yuv_of(self, frames: list) -> Optional[torch.Tensor]:
        """With a 4:2:0 ``pixel_format``: the device tables of Statement P, uploaded on the current stream when first used on that
        device and kept (``hip_ops.frame_yuv_tables``); None otherwise."""
        if self.fmt is None or not self.fmt.planar:
            return None
        if frames[0].device.type != "cuda":
            raise HipLibraryError(f"frames are on {frames[0].device}: the predict path runs only on a ROCm GPU (there is no CPU fallback)")
        return hip_ops.frame_yuv_tables(frames[0].device, self.fmt)

    def lens_of(self, frames: list) -> Optional[torch.Tensor]:
        """With ``lens``: the map on the frames' device, uploaded on the current stream when first used there and kept for good."""
        if self.lens is None:
            return None
        if frames[0].device.type != "cuda":
            raise HipLibraryError(f"frames are on {frames[0].device}: the predict path runs only on a ROCm GPU (there is no CPU fallback)")
        return self.lens.on(frames[0].device)

    def rgb24_of(self, frames: list, n: int, top: int, left: int, size: Tuple[int, int]) -> torch.Tensor:
        """The window of entry ``n`` of a step's ``frames`` as packed RGB24 (the point cloud's colour): ``hip_ops.frames_to_rgb24``; under
        ``lens`` the rectified window -- the copy the ingest made when it went through ``resize``, else one ``frames_remap_rgb24`` launch."""
        if self.lens is None:
            return hip_ops.frames_to_rgb24(frames[n], self.fmt, top, left, size)
        if self._rect[0] is frames:
            return self._rect[1][n]
        return hip_ops.frames_remap_rgb24(frames[n], self.lens, self.fmt)

    def ingest(self, frames: list, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> [batch | mirrored batch] (or the batch alone without TTA) fp32 NCHW: one launch per entry of ``frames``
        (``hip_ops.frame_window_ingest``).  With ``resize`` every frame's window is resized to the model's size by that launch; with
        ``pixel_format`` the frames are read in that format by the same launch.  With ``lens`` the launch is
        ``hip_ops.frame_remap_ingest`` (the rectified window, any format); ``lens`` and ``resize`` together take TWO launches per entry:
        ``hip_ops.frames_remap_rgb24``, then ``frame_resize_ingest`` of its output -- that RGB24 copy is kept for the step's readouts."""
        if self.lens is not None:
            self.window_of(frames)                   # a frame of another size than the map's is refused before anything else
        for f in frames:
            if f.device.type != "cuda":
                raise HipLibraryError(f"frames are on {f.device}: the predict path runs only on a ROCm GPU (there is no CPU fallback)")
        window = self.window_of(frames)
        H, W = self.model_size(frames)
        taps = self.taps_of(frames)
        B = sum(int(f.shape[0]) for f in frames)
        table = self._on(frames[0].device, False)["table"]
        if out is None:
            out = torch.empty((2 * B if self.flip_tta else B, 3, H, W), dtype=torch.float32, device=frames[0].device)
        elif int(out.shape[0]) != (2 * B if self.flip_tta else B):
            raise ValueError(f"{B} frame(s) do not fill a batch of {tuple(out.shape)}")
        i = 0
        rect = []
        for f in frames:
            if self.lens is None:
                top, left, _, _ = _window(self.args, int(f.shape[1]), int(f.shape[2]), self.crop)
                hip_ops.frame_window_ingest(f, table, top, left, window, self.resize, self.fmt, mirror_too=self.flip_tta, out=out,
                                            out_index=i, taps=taps)
            elif self.resize is None:
                hip_ops.frame_remap_ingest(f, table, self.lens, self.fmt, mirror_too=self.flip_tta, out=out, out_index=i)
            else:
                rect.append(hip_ops.frames_remap_rgb24(f, self.lens, self.fmt))
                hip_ops.frame_window_ingest(rect[-1], table, 0, 0, window, self.resize, None, mirror_too=self.flip_tta, out=out,
                                            out_index=i, taps=taps)
            i += int(f.shape[0])
        self._rect = (frames, rect) if rect else (None, None)
        return out

    def ground_truth(self, depth_gt, B: int) -> Optional[torch.Tensor]:
        """fp32 [B, 1, H, W] as given, or uint16 frames (tensor or list) through ``depth_ingest`` with the frames' crop rule."""
        if depth_gt is None:
            return None
        if isinstance(depth_gt, torch.Tensor) and depth_gt.dtype == torch.float32:
            if depth_gt.dim() != 4 or depth_gt.shape[0] != B or depth_gt.shape[1] != 1:
                raise ValueError(f"depth_gt: expected fp32 [{B}, 1, H, W] or uint16 frames, got {tuple(depth_gt.shape)}")
            return depth_gt.contiguous()
        if self.lens is not None:
            raise ValueError("depth_gt: under lens= the ground truth is fp32 [B, 1, Hw, Ww] in the rectified window; uint16 frames are "
                             "refused because depth cannot be interpolated across the lens map (rectify the ground truth beforehand)")
        maps = _frame_list(depth_gt, "depth_gt", 3)
        H, W = self.window_of(maps)
        if sum(int(m.shape[0]) for m in maps) != B:
            raise ValueError("depth_gt: one ground-truth map per frame")
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=maps[0].device)
        i = 0
        for m in maps:
            top, left, _, _ = _window(self.args, int(m.shape[1]), int(m.shape[2]), self.crop)
            hip_ops.depth_ingest(m, depth_factor(self.args), top, left, (H, W), out=out, out_index=i)
            i += int(m.shape[0])
        return out

    def boxes_on(self, boxes, device, B: int):
        """The boxes of a step as (xywh, counts) on the device, or None without boxes / with neither the ``object_depth`` nor the
        ``object_metrics`` keyword."""
        if (self.readout is None and self.errors is None) or boxes is None:
            return None
        xywh, counts = pad_boxes(boxes, device)
        if xywh.dim() != 3 or int(xywh.shape[0]) != B or tuple(counts.shape) != (B,):
            raise ValueError(f"boxes: one entry per un-mirrored frame ({B}), got xywh {tuple(xywh.shape)} / counts {tuple(counts.shape)}")
        return xywh, counts

    def intrinsics_on(self, intrinsics, device, B: int) -> Optional[torch.Tensor]:
        """The intrinsics of a step -- a [B, 4] tensor or a list of per-frame 4-vectors, fx, fy, cx, cy in pixels of the SOURCE frames --
        as fp32 [B, 4] on the device, or None without intrinsics / with none of the ``point_cloud``, ``surface_normals``,
        ``ground_plane`` and ``ground_grid`` keywords."""
        if self.cloud is None and self.normals is None and self.plane is None and self.ground is None:
            return None
        if intrinsics is None:
            if not self.has_default_K:
                return None
            ent = self._on(device, False)                                          # the rectified window's own camera, for every frame
            key = ("lens_K", B)
            if key not in ent:
                ent[key] = torch.tensor(self.lens.new_K, dtype=torch.float32).expand(B, 4).contiguous().to(device)
            return ent[key]
        if not isinstance(intrinsics, torch.Tensor):
            intrinsics = torch.stack([torch.as_tensor(k, dtype=torch.float32).reshape(-1).cpu() for k in intrinsics], 0)
        if tuple(intrinsics.shape) != (B, 4):
            raise ValueError(f"intrinsics: one (fx, fy, cx, cy) per frame ([{B}, 4]), got {tuple(intrinsics.shape)}")
        return intrinsics.to(device=device, dtype=torch.float32).contiguous()

    @property
    def has_default_K(self) -> bool:
        """Whether a call without ``intrinsics=`` still has a camera: the ``lens`` map's ``new_K``."""
        return self.lens is not None and self.lens.new_K is not None

    def pose_on(self, camera_pose, device, B: int) -> Optional[torch.Tensor]:
        """The camera poses of a step -- a [B, 12] (or [B, 3, 4]) tensor or a list of per-frame 3 x 4 [R | t], camera frame to ground
        frame -- as fp32 [B, 12] on the device, or None without them / without the ``ground_grid`` keyword (whose own pose then holds)."""
        if self.ground is None or camera_pose is None:
            return None
        if not isinstance(camera_pose, torch.Tensor):
            camera_pose = torch.stack([torch.as_tensor(p, dtype=torch.float32).reshape(-1).cpu() for p in camera_pose], 0)
        if camera_pose.dim() == 3:
            camera_pose = camera_pose.reshape(camera_pose.shape[0], -1)
        if tuple(camera_pose.shape) != (B, 12):
            raise ValueError(f"camera_pose: one row-major 3 x 4 [R | t] per frame ([{B}, 12]), got {tuple(camera_pose.shape)}")
        return camera_pose.to(device=device, dtype=torch.float32).contiguous()

    def motion_on(self, ego_motion, reset: bool, device, B: int) -> Optional[dict]:
        """The ``memory`` entry of a step record: None without the ``ground_memory`` keyword, else {"motion", "reset"} with the step's
        ``ego_motion`` -- [B, 3] = (dx, dy, dyaw) per frame (``ground_memory.ego_motion`` makes (cos, sin, dx, dy) of it) or [B, 4]
        as that function returns it, a tensor or a list -- as fp32 [B, 4] on the device; None stays None: the identity, a standing
        camera."""
        if self.memory is None:
            return None
        if ego_motion is None:
            return {"motion": None, "reset": bool(reset)}
        m = ego_motion if isinstance(ego_motion, torch.Tensor) else torch.as_tensor(ego_motion, dtype=torch.float64)
        if m.dim() != 2 or int(m.shape[0]) != B or int(m.shape[1]) not in (3, 4):
            raise ValueError(f"ego_motion: one (dx, dy, dyaw) or (cos, sin, dx, dy) per frame ([{B}, 3] or [{B}, 4]), got {tuple(m.shape)}")
        if int(m.shape[1]) == 3:
            m = m.detach().to("cpu", torch.float64)
            m = _ego_motion(m[:, 0], m[:, 1], m[:, 2])
        return {"motion": m.to(device=device, dtype=torch.float32).contiguous(), "reset": bool(reset)}

    def _shift(self, device, top: int, left: int) -> torch.Tensor:
        ent = self._on(device, False)
        key = ("shift", top, left)
        if key not in ent:
            ent[key] = torch.tensor([0.0, 0.0, float(left), float(top)], dtype=torch.float32, device=device)
        return ent[key]

    def step(self, frames: list, size: Optional[Tuple[int, int]] = None, depth_gt=None, boxes=None, intrinsics=None, camera_pose=None,
             ego_motion=None, reset: bool = False) -> _Step:
        """The step record of a call's keywords: boxes padded, intrinsics, poses and motions uploaded, on the current stream.  ``size``:
        the frames' window size where the caller has it already."""
        B, dev = sum(int(f.shape[0]) for f in frames), frames[0].device
        return _Step(depth_gt, self.boxes_on(boxes, dev, B), self.intrinsics_on(intrinsics, dev, B), frames,
                     self.pose_on(camera_pose, dev, B), size or self.window_of(frames), self.motion_on(ego_motion, reset, dev, B))

    def finish(self, out, mirror, step: _Step, first_image_id: int, want: Tuple[str, ...]) -> PredictResult:
        """Final map + (with ground truth) the metric launch, on the current stream, from the outputs of the un-mirrored and (or None)
        the mirrored forward; their ``depth_var`` / ``confidence`` are read when ``want`` names "depth_std" / "confidence".  Behind them
        every readout of ``READOUTS`` whose keyword is set and whose ``needs`` the step has, in that order: the per-object error right
        behind the metric launch, the object readout, the point cloud, the normals, the ground plane, the occupancy grid, then ``TEMPORAL_READOUTS``: the ground memory, then ``DERIVED_READOUTS``: the obstacle list of that grid (or of the fused map).  The maps they
        read are made even when ``want`` leaves them out (and are then not handed out)."""
        asked = want
        live = [r for r, _ in self.readouts if None not in [getattr(step, n) for n in r.needs]]
        for r, reads in self.readouts:
            want = want + tuple(w for w in reads if r in live and w not in want)
        pred = out.depth_pred.contiguous()
        mirror_pred = None if mirror is None else mirror.depth_pred.contiguous()
        depth_gt = self.ground_truth(step.depth_gt, int(pred.shape[0]))
        edges = getattr(out, "bin_edges", None)
        maps = {}
        if want:
            cmap = self._on(pred.device, True)["cmap"] if "rgb8" in want else None
            stats = [getattr(o, k, None) if _need_stats(want) else None for o in (out, mirror) for k in ("depth_var", "confidence")]
            stats = [None if t is None else t.contiguous() for t in stats]
            maps = hip_ops.depth_finalize(pred, self.min_depth, self.max_depth, step.size, pred_mirror=mirror_pred, want=want,
                                          u16_scale=self.u16_scale, colormap=cmap, vmin=self.vmin, vmax=self.vmax,
                                          var=stats[0], pmax=stats[1], var_mirror=stats[2], pmax_mirror=stats[3])
        rec = None
        if depth_gt is not None:
            rec = _records(pred, mirror_pred, edges, depth_gt, self.args, self.min_depth, self.max_depth, first_image_id, self.loss)
        res = PredictResult(maps.get("depth") if "depth" in asked else None, maps.get("depth_u16"), maps.get("rgb8"), rec, edges,
                            maps.get("depth_std") if "depth_std" in asked else None,
                            maps.get("confidence") if "confidence" in asked else None)
        if not live:
            return res
        made = {"maps": maps, "asked": asked, "pred": pred, "mirror": mirror_pred, "depth_gt": depth_gt}
        for r in live:
            made[r.attr] = r.run(self, step, made)
        return _ObjectsResult(*res, **{r.attr: made[r.attr] for r in live})


def _need_stats(want) -> bool:
    return any(w in STATS_WANT for w in want)


def _turn_stats_on(model) -> None:
    """"depth_std" / "confidence" are wanted: the model must return ``depth_var`` / ``confidence``.  A module gets its ``bin_stats`` set;
    a captured graph read the flag when it was captured and cannot change."""
    from .graph import GraphedGraphBins
    if isinstance(model, GraphedGraphBins):
        if not model.bin_stats:
            raise ValueError("want names 'depth_std' / 'confidence', but this graph was captured without bin_stats: set "
                             "model.bin_stats = True before the capture (or pass GraphedGraphBins(..., bin_stats=True))")
    elif not getattr(model, "bin_stats", False):
        if not hasattr(type(model), "bin_stats"):
            raise ValueError(f"want names 'depth_std' / 'confidence', but {type(model).__name__} has no bin_stats")
        model.bin_stats = True


def _check_want(want) -> Tuple[str, ...]:
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = set(want) - set(WANT)
    if bad:
        raise ValueError(f"want: unknown output(s) {sorted(bad)}; expected some of {WANT}")
    return want


class Predictor:
    """``Predictor(model, args)(frames_u8, depth_gt=None, first_image_id=0, want=("depth",))`` -> ``PredictResult``.

    ``frames_u8``: a uint8 device tensor [B, Hs, Ws, 3] or a list of [Hs_i, Ws_i, 3] tensors (KITTI's frames vary in size; every
    frame is cropped to 352 x 1216 by its own origin, one ingest launch per frame into one batch tensor).  ``depth_gt``: fp32
    [B, 1, H, W] metres, or the uint16 maps of the 16-bit PNGs (tensor or list; same crop, / depth_norm_factor).  ``want``: any of
    "depth" (fp32 [B, 1, H, W] at the cropped input size), "depth_u16" ([B, H, W], x ``u16_scale``: the dataset's PNG convention),
    "rgb8" ([B, H, W, 3] through ``colormap`` -- a uint8 [256, 3] tensor or a matplotlib name, default "inferno_r" -- over
    [vmin, vmax], default the dataset's depth range), "depth_std" / "confidence" (fp32 [B, 1, H, W]: standard deviation in metres and
    largest bin probability of the predicted depth distribution -- the mixture of the source pixels' distributions under the same
    TTA and bilinear weights; wanting either sets ``model.bin_stats = True``, a captured graph must have been captured with it).
    ``records``: the [B, 10] / [B, 16] table of ``ValidationStep`` when ground
    truth is given; ``bin_edges``: those of the un-mirrored forward (a captured graph hands out its static tensor).
    ``model``: GraphBins / AdaBins, or a ``GraphedGraphBins`` captured for the [batch | mirrored batch] shape with
    ``object_group = B`` -- the frames are then ingested straight into its static input and it is called through ``checked``.
    ``resize``: None (the window must have the model's size, as above), or the model's (H, W): the window -- ``crop``, e.g.
    ``fit_window(Hs, Ws, H, W)``, else the dataset's rule -- may then have ANY size and is resized to (H, W) by the ingest launch
    (csrc/frame_resize.hip: antialiased, normalised, mirrored, straight into a captured graph's static input of that shape).  Every
    output is still written at the WINDOW's size -- the final map is resized to it like to any size -- so ground truth, ``boxes=``,
    ``intrinsics=`` and the cloud's colour stay in window / source-frame pixels exactly as described here; only boxes fed to the MODEL's
    object provider live in model-input pixels (``boxes_to_model``).  A window may shrink by at most
    ``hip_ops.FRAME_RESIZE_MAX_RATIO`` along an axis.
    ``pixel_format``: None (packed RGB, as above, through the same launches as ever), a ``PixelFormat`` or a name
    (objcavit_amd/pixel_formats.py): "bgr24" (OpenCV), "rgba32" / "bgra32" (tensors [B, Hs, Ws, 4], alpha ignored), "nv12" (hardware
    decoders) / "i420" (software decoders) -- the frames are then a ``PlanarFrames`` (or a list of them), and Y, Cb, Cr become R, G, B by
    Statement P (integer, tables by the host for the format's ``matrix`` and ``range``; chroma replicated) INSIDE the ingest launch, with
    or without ``resize``.  Everything behind the ingest is unchanged; the point cloud's colour is read from the window's RGB24 copy
    (``hip_ops.frames_to_rgb24``, one more launch).
    ``lens``: None, or a ``LensMap`` (objcavit_amd/lens.py: ``LensMap.brown`` / ``fisheye`` / ``from_coordinates``) -- the frames are
    DISTORTED frames of the map's source size (else ``ValueError``), in any ``pixel_format``, and the ingest launch gathers the map's
    rectified window out of them (Statement L, csrc/frame_remap.hip: bilinear, integer, black border) straight into the model's
    input.  The map's window is the window: ``crop=`` is refused, the window origin is (0, 0), every output has the window's size, and
    ``boxes=`` / fp32 ground truth ([B, 1, Hw, Ww]) are in pixels of the rectified window; uint16 ground-truth frames are refused
    (depth cannot be interpolated).  ``intrinsics=`` is in pixels of the rectified window and DEFAULTS to ``lens.new_K``: the readouts
    that need a camera then run without the keyword.  With ``resize`` the ingest takes two launches per frame batch
    (``hip_ops.frames_remap_rgb24``, then ``frame_resize_ingest`` of its output); the point cloud's colour reads the rectified RGB24
    copy -- that one, or without ``resize`` one more ``frames_remap_rgb24`` launch.  ``lens.valid`` tells which pixels have all four taps
    inside the frame; nothing masks by it.
    ``object_depth``: None, or a dict with some of ``quantiles`` / ``shrink`` -- the per-object readout (objcavit_amd/object_depth.py).
    With it, ``boxes=`` of a call -- the boxes a detector found in the B frames, in pixels of the cropped window: a list of [N_i, >= 4]
    tensors / None, an (xywh, counts) pair or a ``PaddedObjects``; independent of the objects the model's provider is fed -- is read out
    of the final map by one launch behind the finalize launch, and the result's ``objects`` ATTRIBUTE holds the ``ObjectDepths`` (None
    otherwise; ``PredictResult``'s fields are what they were).  The fp32 map is made for it even when ``want`` leaves "depth" out;
    ``std_mean`` is filled when ``want`` names "depth_std".
    ``point_cloud``: None, or a dict with some of ``stride`` ((sy, sx) or one int), ``near`` / ``far`` (default the dataset's depth range),
    ``min_confidence``, ``max_std``, ``capacity`` (rows per image, default the strided grid's size), ``colour`` (default True: the
    frame's R, G, B in every record), ``pixel`` (default False: the y * W + x index of every point) -- the final map as compacted 3-D
    points (objcavit_amd/point_cloud.py).  With it, ``intrinsics=`` of a call -- a [B, 4] tensor or a list of per-frame (fx, fy, cx, cy),
    in pixels of the SOURCE frame: the predictor shifts the principal point by each frame's window origin -- is read by two launches
    behind the finalize launch (and the object readout), and the result's ``points`` ATTRIBUTE holds the ``PointCloud`` (None
    otherwise).  ``min_confidence > 0`` / a finite ``max_std`` make the "confidence" / "depth_std" maps for the filter (``bin_stats`` is
    turned on) even when ``want`` leaves them out; byte 15 of a record is the confidence whenever that map is made, else 255.  Rows of
    ``points.points`` at or beyond ``points.counts[b]`` are not written.  ``boxes`` and ``intrinsics`` are keyword arguments.
    ``surface_normals``: None, or a dict with some of ``radius`` (1..4, default 2), ``edge_ratio`` (default 0.05), ``near`` / ``far``
    (default the dataset's depth range), ``picture`` (the rgb8 normal map), ``valid`` (the uint8 mask) -- the orientation of the surface
    at every pixel (objcavit_amd/surface_normals.py, Statement N).  With it, ``intrinsics=`` of a call is read by one more launch behind
    the finalize launch, beside the point cloud, and the result's ``normals`` ATTRIBUTE holds the ``SurfaceNormals`` (None otherwise);
    K is shifted by each frame's window origin as for the cloud; the fp32 map is made for it even when ``want`` leaves "depth" out.
    ``point_cloud=dict(..., normals=True)`` also gathers a normal per point into ``normals.points`` [B, capacity, 4], row for row with
    ``points.points`` (a kept point at a pixel without a normal carries zeros; the cloud itself is unchanged), and implies
    ``surface_normals={}`` when that keyword is absent.  Pass it by keyword.
    ``ground_grid``: None, or a dict with some of ``cell`` (0.1 m), ``x_range`` ((-10, 10)), ``y_range`` ((0, 40)), ``height`` (1.65),
    ``pitch`` / ``roll`` (0.0, radians: ``ground_grid.ground_pose``), ``band`` ((-0.5, 2.5)), ``obstacle_height`` (0.3), ``min_points``
    (1), ``min_obstacle_points`` (3), ``stride``, ``near`` / ``far`` (default the dataset's depth range), ``min_confidence`` /
    ``max_std`` (as the cloud's: the maps are made for the filter even when ``want`` leaves them out), ``want`` (a subset of the
    outputs), ``pose`` (None, or "plane": the ``ground_plane`` keyword's estimate of the same step, below) -- the bird's-eye occupancy
    grid of the final map (objcavit_amd/ground_grid.py, Statement G).  With it, ``intrinsics=`` of a call is read by three more launches behind the finalize launch, and the result's ``ground`` ATTRIBUTE holds the ``GroundGrid`` (None
    otherwise); K is shifted by each frame's window origin as for the cloud.  ``camera_pose=`` of a call -- fp32 [B, 12] (or [B, 3, 4],
    or a list of 3 x 4), camera frame to ground frame -- replaces the keyword's pose for that call (an IMU's pose per frame).  Pass both
    by keyword.
    ``ground_plane``: None, or a dict with some of ``hypotheses`` (256), ``rows`` ((first, end) of the map's rows the triples are drawn
    from, default its lower half), ``seed`` (0), ``tol`` (0.05 m), ``rel_tol`` (0.01), ``max_tilt`` (0.35 rad), ``height_range``
    ((0.5, 4.0)), ``min_cross`` (1e-3), ``min_inliers`` (64), ``height`` / ``pitch`` / ``roll`` of the prior (1.65, 0.0, 0.0),
    ``stride``, ``near`` / ``far``, ``min_confidence`` / ``max_std`` (as the grid's) -- the camera's pose over the ground, estimated from
    the final map (objcavit_amd/ground_plane.py, Statement E).  With it, ``intrinsics=`` of a call is read by four more launches behind
    the normals and in front of the grid, and the result's ``plane`` ATTRIBUTE holds the ``GroundPlane`` (pose [B, 12], stats [B, 4]; None
    otherwise); where no plane is found the pose is the prior's.  ``ground_grid=dict(pose="plane")`` makes the grid of the same step read
    that pose on the device (refused at construction without ``ground_plane=``); ``camera_pose=`` of a call still wins.  Pass it by keyword.
    ``obstacles``: None, or a dict with some of ``link`` (1: 8-connectivity; 2 or 3 bridge one- or two-cell holes), ``min_cells`` (2),
    ``min_obstacle_points`` (0), ``capacity`` (64 rows per image), ``labels`` (False: the per-cell label map) -- the occupied cells of the
    step's grid grouped into obstacles, nearest first (objcavit_amd/obstacles.py, Statement O).  Refused at construction without
    ``ground_grid=``.  With it, at most seven more launches behind the grid's read its buffers on the device, and the result's
    ``obstacles`` ATTRIBUTE holds the ``Obstacles`` (cells, metres [B, capacity, 8], counts, total [B], labels or None; None otherwise).
    The grid's ``state``, ``count``, ``obstacle`` and ``h_max`` are made for it even when the grid's ``want`` leaves them out;
    ``result.ground`` still hands out only what was asked for.  Pass it by keyword.
    ``ground_memory``: None, or a dict with some of ``free`` (2), ``occupied`` (4), ``decay`` (1), ``limit`` (32), ``free_at`` (4),
    ``occupied_at`` (6), ``want`` (a subset of "evidence", "state", "h_max", "first_occupied"), ``obstacles`` (False) -- the grid fused
    over the calls of THIS predictor, every image of the batch a camera stream of its own (objcavit_amd/ground_memory.py, Statement F).
    Refused at construction without ``ground_grid=``.  With it, one more launch behind the grid's (and in front of the obstacle list's)
    carries the previous call's evidence through ``ego_motion=`` of the call -- [B, 3] = (dx, dy, dyaw) since the previous call, or
    [B, 4] as ``ground_memory.ego_motion`` returns it, a tensor or a list, uploaded like ``camera_pose``; None: the camera stood --,
    adds this call's grid, and the result's ``ground_memory`` ATTRIBUTE holds the ``FusedGrid`` (None otherwise).  ``reset=True`` on a
    call forgets before that call.  The grid's ``state`` and ``h_max`` are made for it even when the grid's ``want`` leaves them out.
    ``obstacles=True`` makes the ``obstacles=`` keyword's list from the FUSED ``state`` and ``h_max`` (``points`` / ``obstacle_points`` of
    a row are then 0); otherwise the list reads the frame's grid as without the memory.  Every result's tensors are fresh: the memory
    keeps the newest by reference and overwrites nothing.  Pass them by keyword.
    ``object_metrics``: None, or a dict with some of ``shrink`` / ``regions`` -- the depth error per box and over objects against
    background (objcavit_amd/object_metrics.py).  With it, a call that has both ``depth_gt`` and ``boxes=`` (in pixels of the ground
    truth's grid) issues one more call right behind the metric launch, on the tensors that launch reads, and the result's
    ``object_metrics`` ATTRIBUTE holds the ``ObjectMetrics`` (None otherwise); ``records`` and every field are what they were.  Pass it
    by keyword."""

    def __init__(self, model, args, flip_tta: bool = True, loss: bool = False, colormap=None, vmin: Optional[float] = None,
                 vmax: Optional[float] = None, u16_scale: Optional[float] = None, surface_normals: Optional[dict] = None,
                 ground_grid: Optional[dict] = None, lens: Optional[LensMap] = None, ground_plane: Optional[dict] = None,
                 obstacles: Optional[dict] = None, ground_memory: Optional[dict] = None, pixel_format=None,
                 crop: Optional[Tuple[int, int, int, int]] = None, resize: Optional[Tuple[int, int]] = None,
                 object_metrics: Optional[dict] = None, point_cloud: Optional[dict] = None, object_depth: Optional[dict] = None):
        self.model = model
        self.ends = _Ends(args, flip_tta=flip_tta, loss=loss, colormap=colormap, vmin=vmin, vmax=vmax, u16_scale=u16_scale, crop=crop,
                          resize=resize, pixel_format=pixel_format, lens=lens, object_depth=object_depth, point_cloud=point_cloud,
                          object_metrics=object_metrics, surface_normals=surface_normals, ground_grid=ground_grid,
                          ground_plane=ground_plane, obstacles=obstacles, ground_memory=ground_memory)
        self.flip_tta = flip_tta

    def _forward(self, frames: List[torch.Tensor], B: int):
        """(output of the un-mirrored forward, the mirrored forward's output or None): ``validation._forward_pair`` fed by the ingest,
        which writes straight into a captured graph's static input when that has the step's shape."""
        static = getattr(self.model, "static_image", None)
        fits = static is not None and tuple(static.shape[2:]) == self.ends.model_size(frames)
        if not self.flip_tta:
            return _call(self.model, self.ends.ingest(frames, out=static if fits and int(static.shape[0]) == B else None)), None
        return _forward_pair(self.model, both=self.ends.ingest(frames, out=static if fits and _joint(self.model, B) else None))

    @torch.no_grad()
    def __call__(self, frames_u8: Frames, depth_gt=None, first_image_id: int = 0, want: Sequence[str] = ("depth",),
                 ego_motion=None, reset: bool = False, camera_pose=None, intrinsics=None, boxes=None) -> PredictResult:
        want = _check_want(want)
        if _need_stats(want) or ((intrinsics is not None or self.ends.has_default_K) and (_cloud_want(self.ends.cloud) or _cloud_want(self.ends.plane) or _cloud_want(self.ends.ground))):
            _turn_stats_on(self.model)
        frames = self.ends.frames_of(frames_u8, "frames_u8")
        out, mirror = self._forward(frames, sum(int(f.shape[0]) for f in frames))
        step = self.ends.step(frames, depth_gt=depth_gt, boxes=boxes, intrinsics=intrinsics, camera_pose=camera_pose,
                              ego_motion=ego_motion, reset=reset)
        return self.ends.finish(out, mirror, step, first_image_id, want)


class PipelinedPredictor(_SlotPipeline):
    """``slots`` predict steps IN FLIGHT, on ``PipelinedValidation``'s slot pipeline (``validation._SlotPipeline``): one captured graph of
    the joint [batch | mirrored batch] forward per slot, each on a stream with a hardware queue of its own.  ``submit`` ingests the
    frames DIRECTLY into the slot's static input -- no ``flip``, no ``cat``, no ``copy_`` of the image: the graph sees its own
    pointer and skips its copy --, replays, and writes the final map (and, with ground truth, the metric records) on the slot's
    stream; ``collect`` returns the ``PredictResult`` of every submitted step in submission order; a step whose fp16 range guard
    tripped is ingested again from its kept frames for the re-run.  ``bin_edges`` of a result is
    None unless ``want`` names "bin_edges" (the graph's static tensor is then copied per step).  Wants ``GPU_MAX_HW_QUEUES`` >= slots
    set before the HIP runtime starts, like ``PipelinedValidation``.  ``object_depth`` / ``submit(..., boxes=)``: as ``Predictor``'s; the
    readout runs on the slot's stream, a re-run step is read out from the re-run's map.  ``point_cloud`` / ``submit(..., intrinsics=)``:
    likewise; a list of differently sized frames gives one launch pair per frame.  ``surface_normals``: as ``Predictor``'s, on the slot's
    stream behind the cloud, no host read.  ``ground_grid`` / ``submit(..., camera_pose=)``: as ``Predictor``'s, on the slot's stream behind
    the normals; the pose is uploaded in ``submit`` and held like the frames.  ``ground_plane``: as ``Predictor``'s, on the slot's stream
    between the normals and the grid, no host read; with ``ground_grid=dict(pose="plane")`` the grid reads the step's own estimate.
    ``obstacles``: as ``Predictor``'s, on the slot's stream behind the grid, no host read; its tensors are recorded like the grid's.
    ``ground_memory`` / ``submit(..., ego_motion=, reset=)``: as ``Predictor``'s, fused in SUBMISSION order: the first state that crosses
    steps.  The slots run on streams of their own, so a step's fuse launch waits (on the device) for the event the previous step's
    recorded; only that launch is ordered, the forwards overlap as before.  A step that ``collect`` re-runs (fp16 range guard) is fused
    again from the previous evidence and the motion it had read, and the memory is not advanced a second time: the steps behind it have
    fused its FIRST map (``_run_memory``).
    ``object_metrics``: as ``Predictor``'s, on the slot's stream behind the step's metric launch; a re-run step gets its table from the re-run's forward.  ``resize``: as ``Predictor``'s; the
    graphs are captured for (H, W), a step's window may have another size than the example's (one size within a step) and its outputs
    have that size; a size's tap tables are uploaded when it is first submitted; a re-run step is resized again from its kept frames.
    ``pixel_format``: as ``Predictor``'s; every plane of a submitted ``PlanarFrames`` is held like the frames, the tables of Statement P
    are uploaded on the caller's stream when first used, a re-run step is ingested again from its kept planes.
    ``lens``: as ``Predictor``'s; the map's device copy is made once and outlives every step, the RGB24 copy of a ``resize`` step is
    made on the slot's stream and kept with the step.

        pp = PipelinedPredictor(model, args, example_frames, want=("depth_u16",))
        for i, frame in enumerate(frames):                    # uint8 [1, Hs, Ws, 3] on the device
            pp.submit(frame, first_image_id=i)
        results = pp.collect()
    """

    name = "PipelinedPredictor"

    def __init__(self, model, args, example_frames: Frames, slots: int = 4, object_capacity: Optional[int] = None,
                 flip_tta: bool = True, loss: bool = False, want: Sequence[str] = ("depth",), colormap=None,
                 vmin: Optional[float] = None, vmax: Optional[float] = None, u16_scale: Optional[float] = None, surface_normals: Optional[dict] = None,
                 ground_grid: Optional[dict] = None, lens: Optional[LensMap] = None, ground_plane: Optional[dict] = None,
                 obstacles: Optional[dict] = None, ground_memory: Optional[dict] = None, pixel_format=None,
                 crop: Optional[Tuple[int, int, int, int]] = None, resize: Optional[Tuple[int, int]] = None,
                 object_metrics: Optional[dict] = None, point_cloud: Optional[dict] = None, object_depth: Optional[dict] = None):
        super().__init__(slots)
        self.want_edges = "bin_edges" in tuple(want)
        self.want = _check_want(tuple(w for w in ((want,) if isinstance(want, str) else want) if w != "bin_edges"))
        self.ends = _Ends(args, flip_tta=flip_tta, loss=loss, colormap=colormap, vmin=vmin, vmax=vmax, u16_scale=u16_scale, crop=crop,
                          resize=resize, pixel_format=pixel_format, lens=lens, object_depth=object_depth, point_cloud=point_cloud,
                          object_metrics=object_metrics, surface_normals=surface_normals, ground_grid=ground_grid,
                          ground_plane=ground_plane, obstacles=obstacles, ground_memory=ground_memory)
        if _need_stats(self.want) or _cloud_want(self.ends.cloud) or _cloud_want(self.ends.plane) or _cloud_want(self.ends.ground):
            _turn_stats_on(model)                            # before the captures below: a graph reads the flag when it is captured
        self.flip_tta = flip_tta
        ex = self.ends.frames_of(example_frames, "example_frames")
        self.B = sum(int(f.shape[0]) for f in ex)
        self.size = self.ends.window_of(ex)
        both = self.ends.ingest(ex)
        if "rgb8" in self.want:
            self.ends._on(both.device, True)                 # the colour table is uploaded here, not inside a step
        self._capture(model, both, object_capacity, self.B if flip_tta else None)

    def _stage(self, frames: List[torch.Tensor], g):
        return self.ends.ingest(frames, out=g.static_image), frames

    def _restage(self, frames: List[torch.Tensor]) -> torch.Tensor:
        return self.ends.ingest(frames)                      # the slot's static input has long been overwritten: ingest again

    def _finish(self, out, step: _Step, first_image_id: int) -> PredictResult:
        out, mirror = _split(out, self.B) if self.flip_tta else (out, None)
        res = self.ends.finish(out, mirror, step, first_image_id, self.want)
        return res._replace(bin_edges=res.bin_edges.clone() if (self.want_edges and res.bin_edges is not None) else None)

    def collect(self) -> List[PredictResult]:
        """Wait for every submitted step; -> their results in submission order (and forget them)."""
        return self._collect()

    def submit(self, frames_u8: Frames, depth_gt=None, first_image_id: int = 0, object_features=None, object_xywh_list=None,
               ego_motion=None, reset: bool = False, camera_pose=None, intrinsics=None, boxes=None) -> None:
        """Enqueue one predict step on the next slot's stream; returns at once.  ``boxes``: the boxes of the step's frames
        (``object_depth`` / ``object_metrics`` keywords); lists are padded here, on the caller's stream, and the tensors are held like the frames.
        ``intrinsics``: the frames' (fx, fy, cx, cy) for the point cloud (``point_cloud`` keyword), uploaded here and held likewise;
        the cloud's buffers are made per step on the slot's stream, its workspace is the slot's.
        ``object_features``: as ``PipelinedValidation.submit``'s -- a ``Detections`` of the B frames (the model's provider a
        ``DeviceObjectProvider``, with ``mirror_width`` under flip-TTA) is written into the slot's static buffers by one launch."""
        frames = self.ends.frames_of(frames_u8, "frames_u8")
        size = self.ends.window_of(frames)
        if sum(int(f.shape[0]) for f in frames) != self.B or (size != self.size and self.ends.resize is None):
            raise ValueError(f"captured for {self.B} frame(s) cropped to {self.size}")
        # ``resize``: a window size seen for the first time has its tap tables uploaded HERE, on the caller's stream, which the slot's
        # stream waits for before its launch; the cache keeps them alive, and they are held like the frames
        # ``pixel_format``: likewise the tables of Statement P; every plane of a ``PlanarFrames`` is held like the frames
        taps = self.ends.taps_of(frames)
        yuv = self.ends.yuv_of(frames)
        self.ends.lens_of(frames)                    # ``lens``: the map's device copy is made HERE when the device is new; it is kept for good
        step = self.ends.step(frames, size, depth_gt=depth_gt, boxes=boxes, intrinsics=intrinsics, camera_pose=camera_pose,
                              ego_motion=ego_motion, reset=reset)
        held = list(taps or ()) + ([] if yuv is None else [yuv]) + _tensors_of(frames) + step.held()
        self._submit(frames, held, step, first_image_id, (object_features, object_xywh_list))
        made = self._pending[-1].result
        for r, _ in self.ends.readouts:                                    # ``READOUTS.streamed``: made on the slot's stream, read by
            for t in tuple(getattr(made, r.attr) or ())[r.streamed]:       # the caller on this one
                if isinstance(t, torch.Tensor):
                    t.record_stream(torch.cuda.current_stream(t.device))

    def records(self, results: Sequence[PredictResult]) -> torch.Tensor:
        """The record table [N * B, 10] ([N * B, 16] with ``loss``) of collected results that carried ground truth."""
        recs = [r.records for r in results if r.records is not None]
        return torch.cat(recs, 0) if recs else _empty_records(self.ends.loss)
