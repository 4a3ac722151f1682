"""Which ground in front of the camera is free, and how far is the first obstacle in each lane: a bird's-eye occupancy grid of the
predict path's final map, on the device.

``ground_grid(depth, K, pose)`` takes the fp32 map [B, 1, H, W] of ``Predictor`` / ``hip_ops.depth_finalize``, the cameras' intrinsics ``K``
[B, 4] = fx, fy, cx, cy in pixels of the map's own grid (``point_cloud.shift_intrinsics`` moves a source frame's K to a crop window) and the
cameras' poses [B, 12] (``ground_pose``), and returns in three launches (csrc/ground_grid.hip), without a copy of the map or of a cloud to
the host, a ``GroundGrid`` of GX x GY cells of ``cell`` metres, lateral x forward, from the corner (x0, y0) of the ground frame:

    count           int32 [B, GY, GX]  the points of the map that fall into the cell with a height inside ``band``
    obstacle        int32 [B, GY, GX]  those of them above ``obstacle_height``
    h_min, h_max    fp32  [B, GY, GX]  the lowest and the highest of them (0 in an empty cell: ``count`` = 0 is the flag)
    h_mean          fp32  [B, GY, GX]  their mean height, from a 64-bit integer sum in units of 1 / 1024 m
    state           uint8 [B, GY, GX]  0 = unknown (fewer than ``min_points``), 2 = occupied (at least ``min_obstacle_points`` obstacle
                                       points), 1 = free
    first_occupied  fp32  [B, GX]      per lateral column, the forward distance y0 + iy * cell of its nearest occupied cell; +inf without one

A pixel becomes a point iff the point cloud would keep it (``stride``, ``near`` / ``far``, ``confidence`` / ``depth_std`` thresholds, a
usable camera) and its image's pose is finite.  The point P = ((x - cx) z / fx, (y - cy) z / fy, z) of the camera frame (x right, y down,
z forward) goes to the GROUND frame g = R P + t: g_0 lateral (right), g_1 forward, g_2 height (up); ``pose`` is the row-major 3 x 4
[R | t].  Everything per point is fp32 with every operation rounded on its own, everything per cell integer arithmetic (integer atomics
on chip and in memory), so the grid is the same bits on every call and equal to the statement (Statement G of include/objcavit_hip.h,
tests/ground_grid_ref.py), not merely close to it.  Cells between the camera and the first hit stay "unknown" unless they are seen: there
is no ray casting, and the pose is the caller's (an IMU's, a calibration's), not estimated from the map -- unless the
predictors' ``ground_plane=`` keyword estimates it in the same step and ``ground_grid=dict(pose="plane")`` reads it
(objcavit_amd/ground_plane.py).  A grid is ONE frame's answer and flickers as the depth map does; fusing it over time -- per-cell
evidence carried from step to step through the vehicle's motion -- is ``objcavit_amd/ground_memory.py`` (the predictors'
``ground_memory=`` keyword), which reads this grid's ``state`` and ``h_max``.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Sequence, Tuple

import torch

from . import hip_ops

OUTPUTS = hip_ops.GROUND_GRID_WANT

GroundGrid = namedtuple("GroundGrid", OUTPUTS + ("x0", "y0", "cell"), defaults=(None,) * len(OUTPUTS) + (0.0, 0.0, 1.0))
GroundGrid.__doc__ = """count, obstacle int32 [B, GY, GX]; h_min, h_max, h_mean fp32 [B, GY, GX]; state uint8 [B, GY, GX]; first_occupied
fp32 [B, GX] -- on the device, None where not asked for -- and the grid's x0, y0, cell in metres."""


def _x_centres(self, GX: Optional[int] = None) -> torch.Tensor:
    """fp64 [GX] on the host: the lateral coordinate of every column's centre."""
    n = GX if GX is not None else next(int(t.shape[-1]) for t in self[:len(OUTPUTS)] if t is not None)
    return self.x0 + (torch.arange(n, dtype=torch.float64) + 0.5) * self.cell


def _y_centres(self, GY: Optional[int] = None) -> torch.Tensor:
    """fp64 [GY] on the host: the forward coordinate of every row's centre."""
    n = GY if GY is not None else next(int(t.shape[-2]) for t in self[:len(OUTPUTS) - 1] if t is not None)
    return self.y0 + (torch.arange(n, dtype=torch.float64) + 0.5) * self.cell


GroundGrid.x_centres = _x_centres
GroundGrid.y_centres = _y_centres

DEFAULTS = {"cell": 0.1, "x_range": (-10.0, 10.0), "y_range": (0.0, 40.0), "height": 1.65, "pitch": 0.0, "roll": 0.0, "band": (-0.5, 2.5),
            "obstacle_height": 0.3, "min_points": 1, "min_obstacle_points": 3}


def grid_of(cell: float = 0.1, x_range: Tuple[float, float] = (-10.0, 10.0), y_range: Tuple[float, float] = (0.0, 40.0)):
    """(x0, y0, cell, GX, GY): the cells of ``cell`` metres that cover [x_range) x [y_range) from their lower corner (the count rounded
    to the nearest whole number of cells, at least one)."""
    cell = float(cell)
    if not 0.0 < cell < float("inf"):
        raise ValueError(f"ground_grid: cell must be > 0 and finite, got {cell}")
    spans = []
    for name, r in (("x_range", x_range), ("y_range", y_range)):
        lo, hi = float(r[0]), float(r[1])
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise ValueError(f"ground_grid: {name} must be (lo, hi) with lo < hi, both finite, got {tuple(r)}")
        spans.append((lo, max(1, int(round((hi - lo) / cell)))))
    return spans[0][0], spans[1][0], cell, spans[0][1], spans[1][1]


def ground_pose(height, pitch=0.0, roll=0.0) -> torch.Tensor:
    """fp32 [B, 12] on the host: the row-major 3 x 4 [R | t] of a camera ``height`` metres above flat ground, per image (scalars or
    sequences of one length), made in float64 and rounded once:

        R = A . Rx(pitch) . Rz(roll),    t = (0, 0, height)

        A = [[1, 0, 0], [0, 0, 1], [0, -1, 0]]                       camera (x right, y down, z forward) -> ground (x right, y forward, z up)
        Rx(p) = [[1, 0, 0], [0, cos p, sin p], [0, -sin p, cos p]]   pitch > 0 tilts the optical axis DOWN
        Rz(r) = [[cos r, -sin r, 0], [sin r, cos r, 0], [0, 0, 1]]   roll about the optical axis

    (radians).  Row 0 of the result gives the lateral ground coordinate, row 1 the forward one, row 2 the height."""
    cols = [torch.as_tensor(v, dtype=torch.float64).reshape(-1) for v in (height, pitch, roll)]
    B = max(int(c.numel()) for c in cols)
    if any(int(c.numel()) not in (1, B) for c in cols):
        raise ValueError("ground_pose: height, pitch and roll must be scalars or sequences of one length")
    h, p, r = (c.expand(B) for c in cols)
    one, zero = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    A = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]], dtype=torch.float64)
    Rx = torch.stack([one, zero, zero, zero, p.cos(), p.sin(), zero, -p.sin(), p.cos()], 1).view(B, 3, 3)
    Rz = torch.stack([r.cos(), -r.sin(), zero, r.sin(), r.cos(), zero, zero, zero, one], 1).view(B, 3, 3)
    R = A.unsqueeze(0) @ Rx @ Rz
    t = torch.stack([zero, zero, h], 1).view(B, 3, 1)
    return torch.cat([R, t], 2).reshape(B, 12).to(torch.float32)


def ground_grid(depth: torch.Tensor, K: torch.Tensor, pose: torch.Tensor, cell: float = 0.1, x_range: Tuple[float, float] = (-10.0, 10.0),
                y_range: Tuple[float, float] = (0.0, 40.0), band: Tuple[float, float] = (-0.5, 2.5), obstacle_height: float = 0.3,
                min_points: int = 1, min_obstacle_points: int = 3, stride: Tuple[int, int] = (1, 1), near: float = 0.0,
                far: float = float("inf"), confidence: Optional[torch.Tensor] = None, min_confidence: float = 0.0,
                depth_std: Optional[torch.Tensor] = None, max_std: float = float("inf"), want: Sequence[str] = OUTPUTS,
                out: Optional[dict] = None) -> GroundGrid:
    """-> ``GroundGrid`` (see the module's text).  ``pose``: fp32 [B, 12] on the device (``ground_pose(...).to(device)``), or on the host
    (it is uploaded).  ``want``: the outputs to make; ``out``: {name: tensor} to write into."""
    spec = grid_of(cell, x_range, y_range)
    if isinstance(pose, torch.Tensor) and pose.device != depth.device:
        pose = pose.to(device=depth.device, dtype=torch.float32).contiguous()
    res = hip_ops.ground_grid(depth, K, pose, spec, band=band, obstacle_height=obstacle_height, min_points=min_points,
                              min_obstacle_points=min_obstacle_points, stride=stride, near=near, far=far, confidence=confidence,
                              min_confidence=min_confidence, depth_std=depth_std, max_std=max_std, want=want, out=out)
    return GroundGrid(*(res.get(n) for n in OUTPUTS), x0=spec[0], y0=spec[1], cell=spec[2])
