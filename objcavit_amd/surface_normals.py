"""How is the surface at every pixel oriented: unit normals of the predict path's final map, on the device.

``surface_normals(depth, K)`` takes the fp32 map [B, 1, H, W] of ``Predictor`` / ``hip_ops.depth_finalize`` and the cameras' intrinsics ``K``
[B, 4] = fx, fy, cx, cy in pixels of the map's own grid (``point_cloud.shift_intrinsics`` moves a source frame's K to a crop window), and
returns in ONE launch (csrc/surface_normals.hip), without a copy of the map to the host:

    normals  fp32 [B, 3, H, W]: the unit normal (nx, ny, nz) of the surface seen at every pixel, in the camera frame of the point cloud
             (x right, y down, z forward), pointing AT the camera (nz < 0 for a wall that faces it); (0, 0, 0) where there is none
    rgb8     uint8 [B, H, W, 3] (``picture``): rint(127.5 n + 127.5), the usual normal-map picture; (0, 0, 0) where there is none
    valid    uint8 [B, H, W] (``valid``): 1 where the pixel has a normal
    points   fp32 [B, capacity, 4] (with a ``PointCloud`` that carries ``pixel``): (nx, ny, nz, 0) of every point of the cloud, row for
             row with ``cloud.points``; rows at or beyond ``cloud.counts[b]`` are NOT written, like the cloud's

The final map is a 2x bilinear enlargement of the head's map, so it is piecewise bilinear and the cross product of one-pixel differences
gives faceted normals.  The slope here is the LEAST-SQUARES plane fitted to the (2 radius + 1)^2 depths around the pixel:

    zu = sum_j sum_i i (z(x + i, y + j) - z(x - i, y + j)) / D,    zv likewise along y,    D = (2r + 1) 2 (1 + 4 + ... + r^2)
    m  = (fx zu, fy zv, -(z + (x - cx) zu + (y - cy) zv)),          n = m / |m|

which is the normal of the surface ((x - cx) z / fx, (y - cy) z / fy, z) the point cloud is made of.  A pixel has a normal iff its window
lies inside the map (a border of ``radius`` pixels has none), every depth in the window is finite and within [near, far], and the
window's largest and smallest depth differ from the centre's by at most ``edge_ratio`` times the centre's depth -- a window that straddles
a depth discontinuity (an object's silhouette) has no plane to fit; and the image's fx, fy must be finite and positive.  The rule is
evaluated in fp32, every operation rounded on its own, so the mask is the same bits everywhere (tests/normals_ref.py is the statement the
kernel is compared with; include/objcavit_hip.h carries it as Statement N).
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

from . import hip_ops
from .point_cloud import PointCloud

SurfaceNormals = namedtuple("SurfaceNormals", ["normals", "rgb8", "valid", "points"], defaults=(None, None, None))
SurfaceNormals.__doc__ = """normals fp32 [B, 3, H, W]; rgb8 uint8 [B, H, W, 3] or None; valid uint8 [B, H, W] or None; points fp32
[B, capacity, 4] (a normal per point of a cloud) or None -- all on the device."""

DEFAULT_RADIUS = 2
DEFAULT_EDGE_RATIO = 0.05


def surface_normals(depth: torch.Tensor, K: torch.Tensor, radius: int = DEFAULT_RADIUS, edge_ratio: float = DEFAULT_EDGE_RATIO,
                    near: float = 0.0, far: float = float("inf"), picture: bool = False, valid: bool = False,
                    cloud: Optional[PointCloud] = None, out: Optional[dict] = None) -> SurfaceNormals:
    """-> ``SurfaceNormals`` (see the module's text).  ``cloud``: a ``PointCloud`` of the same map made with ``pixel=True``; its points
    get their normals by one more launch.  ``out``: {"normals" / "rgb8" / "valid": tensor} to write into."""
    want = ("normals",) + (("rgb8",) if picture else ()) + (("valid",) if valid else ())
    res = hip_ops.depth_normals(depth, K, radius=radius, near=near, far=far, edge_ratio=edge_ratio, want=want, out=out)
    points = None
    if cloud is not None:
        if cloud.pixel is None:
            raise ValueError("surface_normals: the cloud carries no pixel index (point_cloud(..., pixel=True))")
        points = hip_ops.normals_gather(res["normals"], cloud.pixel, cloud.counts)
    return SurfaceNormals(res["normals"], res.get("rgb8"), res.get("valid"), points)
