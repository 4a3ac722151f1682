"""Where is every pixel in space: the predict path's final map as 3-D points in the camera frame, compacted on the device.

``point_cloud(depth, K)`` takes the fp32 map [B, 1, H, W] of ``Predictor`` / ``hip_ops.depth_finalize`` and the cameras' intrinsics ``K``
[B, 4] = fx, fy, cx, cy in pixels of the map's own grid, and returns per image the kept pixels' points in row-major pixel order, in TWO
launches (csrc/point_cloud.hip) without a copy of the map to the host and without a count read on the host:

    points   fp32 [B, capacity, 4]: 16-byte records X, Y, Z (metres; x right, y down, z forward: the OpenCV camera frame) + 4 bytes
             R, G, B, A -- the colour of the frame's pixel (0 without frames) and 255 * confidence rounded (255 without a confidence map)
    counts   int32 [B]: valid rows per image = min(total, capacity)
    total    int32 [B]: kept pixels per image (total > counts: the cloud was cut at ``capacity``)
    pixel    int32 [B, capacity] = y * W + x of every point (``want_pixel``), to gather any other map with or to match points to boxes

ROWS AT OR BEYOND ``counts[b]`` ARE NOT WRITTEN -- they hold whatever the memory held; read ``points[b, :counts[b]]``.  A pixel is kept
iff it lies on the ``stride`` grid, its depth is finite and within [near, far], and (where the maps are given) its confidence is at least
``min_confidence`` and its ``depth_std`` at most ``max_std``; an image whose fx / fy are not finite and positive keeps nothing.

The reference carries the focal length only (third column of its split files): ``intrinsics_from_focal`` puts the principal point at the
frame's centre; a caller with a calibration passes its own K.  K refers to the grid of the MAP: ``shift_intrinsics`` moves the principal
point of a source frame's K by a crop window's origin.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Tuple

import torch

from . import hip_ops
from .object_depth import ObjectDepths


class PointCloud(namedtuple("PointCloud", ["points", "counts", "total", "pixel"])):
    """points fp32 [B, cap, 4], counts / total int32 [B], pixel int32 [B, cap] or None -- all on the device."""
    __slots__ = ()

    @property
    def xyz(self) -> torch.Tensor:
        """fp32 [B, cap, 3]: a strided VIEW of ``points`` (row stride 4)."""
        return self.points[..., :3]

    @property
    def rgba(self) -> torch.Tensor:
        """uint8 [B, cap, 4]: bytes 12-15 of every record, a strided VIEW of ``points`` (row stride 16)."""
        return self.points.view(torch.uint8)[..., 12:16]


def intrinsics_from_focal(focal, Hs: int, Ws: int) -> torch.Tensor:
    """fp32 [B, 4] = [f, f, (Ws - 1) / 2, (Hs - 1) / 2] per focal length (a number, a sequence or a tensor [B]): square pixels, the
    principal point at the centre of the Hs x Ws frame (pixel centres at integer coordinates)."""
    f = torch.as_tensor(focal, dtype=torch.float32).reshape(-1)
    c = torch.tensor([(int(Ws) - 1) / 2.0, (int(Hs) - 1) / 2.0], dtype=torch.float32, device=f.device)
    return torch.cat([f.view(-1, 1).expand(-1, 2), c.view(1, 2).expand(f.numel(), 2)], 1).contiguous()


def shift_intrinsics(K: torch.Tensor, top: int, left: int) -> torch.Tensor:
    """K [..., 4] of a frame -> K of its window at (top, left): fp32 cx - left, cy - top (one op on K's device)."""
    return K - K.new_tensor([0.0, 0.0, float(left), float(top)])


def point_cloud(depth: torch.Tensor, K: torch.Tensor, capacity: Optional[int] = None, stride: Tuple[int, int] = (1, 1),
                near: float = 0.0, far: float = float("inf"), confidence: Optional[torch.Tensor] = None, min_confidence: float = 0.0,
                depth_std: Optional[torch.Tensor] = None, max_std: float = float("inf"), frames: Optional[torch.Tensor] = None,
                top: int = 0, left: int = 0, pixel: bool = False, out: Optional[dict] = None) -> PointCloud:
    """-> ``PointCloud`` (see the module's text).  ``capacity``: rows per image, default the strided grid's size (every pixel fits)."""
    if capacity is None:
        gh, gw = hip_ops.unproject_grid(int(depth.shape[-2]), int(depth.shape[-1]), stride)
        capacity = gh * gw
    res = hip_ops.depth_unproject(depth, K, capacity, stride=stride, near=near, far=far, confidence=confidence,
                                  min_confidence=min_confidence, depth_std=depth_std, max_std=max_std, frames=frames, top=top, left=left,
                                  want_pixel=pixel, out=out)
    return PointCloud(res["points"], res["counts"], res["total"], res.get("pixel"))


def object_positions(objects: ObjectDepths, xywh: torch.Tensor, K: torch.Tensor, field: str = "q0.5") -> torch.Tensor:
    """fp32 [B, cap, 3]: the 3-D point at the centre of every box of an ``ObjectDepths`` table, at the depth column ``field`` (default the
    box's median).  ``xywh`` [B, cap, >= 4] are the boxes the table was read with -- pixel-EDGE coordinates (a pixel's centre is at
    x + 0.5), so the centre's pixel coordinate is u = cx_box - 0.5 --, ``K`` [B, 4] the intrinsics of the map's grid.
    ((u - cx) / fx * z, (v - cy) / fy * z, z); zero for a row without a valid pixel (n = 0).  A few torch ops, no kernel."""
    table = objects.table
    z = table[..., objects.fields.index(field)]
    k = K.to(table.dtype).unsqueeze(1)                                         # [B, 1, 4]
    u, v = xywh[..., 0] - 0.5, xywh[..., 1] - 0.5
    pos = torch.stack([(u - k[..., 2]) / k[..., 0] * z, (v - k[..., 3]) / k[..., 1] * z, z], -1)
    return torch.where((table[..., 0] > 0).unsqueeze(-1), pos, torch.zeros_like(pos))
