"""Where is the ground: the camera's pose over the ground plane, estimated from the predict path's final map, on the device -- the
pose ``ground_grid`` needs and a camera without an IMU cannot give.

``ground_plane(depth, K)`` takes the fp32 map [B, 1, H, W] of ``Predictor`` / ``hip_ops.depth_finalize`` and the cameras' intrinsics ``K``
[B, 4] and returns in four launches (csrc/ground_plane.hip), without a copy of the map or of a cloud to the host, a ``GroundPlane``:

    pose    fp32  [B, 12]  the row-major 3 x 4 [R | t] of ``ground_grid.ground_pose``: row 0 right, row 1 forward (the optical axis
                           projected onto the plane), row 2 the plane's unit normal (up) and the camera's height above it
    stats   int32 [B, 4]   the best hypothesis (-1: none), its inlier count, the points of the refit, ok (1: ``pose`` is the estimate;
                           0: ``pose`` is the PRIOR, bit for bit)

The estimate is a consensus over a FIXED table of hypotheses -- RANSAC whose random draws are made once, on the host, by
``plane_triples`` (a seed, pixel triples of the map's lower half), so that nothing is random at run time: every triple of kept pixels
spans a plane; planes tilted more than ``max_tilt`` from the prior's up, outside ``height_range`` or spanned by a degenerate triple are
dropped; each of the others is scored by the number of the map's points (the pixels ``ground_grid`` would turn into points: ``stride``,
``near`` / ``far``, ``confidence`` / ``depth_std`` thresholds, a usable camera) within ``tol`` + ``rel_tol`` * Z of it; the best one
(the first of equals) with at least ``min_inliers`` is refitted ONCE, by least squares over its inliers, from nine 64-bit integer sums.
Everything per point is fp32 with every operation rounded on its own, the sums are integers, the solve is float64: the result is the
same bits on every call and equal to the statement (Statement E of include/objcavit_hip.h, tests/ground_plane_ref.py).  ``pose_angles``
turns a pose back into height, pitch and roll.

What is NOT done: no filtering over time (every frame is estimated on its own: smooth ``pose_angles`` outside if the ride is bumpy), ONE
plane (a ramp, a kerb or a crowned road is fitted by the plane most points agree on), ONE refit (no iteratively re-weighted fit, no
second consensus around the refit)."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip_ops
from .ground_grid import ground_pose

GroundPlane = namedtuple("GroundPlane", ["pose", "stats"])
GroundPlane.__doc__ = """pose fp32 [B, 12] (``ground_pose``'s layout), stats int32 [B, 4] = best, count, N, ok -- on the device."""

DEFAULTS = {"hypotheses": 256, "rows": None, "seed": 0, "tol": 0.05, "rel_tol": 0.01, "max_tilt": 0.35, "height_range": (0.5, 4.0),
            "min_cross": 1e-3, "min_inliers": 64, "height": 1.65, "pitch": 0.0, "roll": 0.0}


def plane_triples(H: int, W: int, T: int = 256, rows: Optional[Tuple[int, int]] = None, seed: int = 0) -> torch.Tensor:
    """int32 [T, 3] on the host: the table of hypotheses, T pixel triples y * W + x whose pixels are drawn uniformly, by
    ``numpy.random.default_rng(seed)``, from the rows ``rows`` = (first, end) -- default the map's lower half, H // 2 .. H -- and all
    columns.  The same arguments give the same table."""
    H, W, T = int(H), int(W), int(T)
    if H < 1 or W < 1:
        raise ValueError(f"plane_triples: H, W must be >= 1, got {H}, {W}")
    if not 1 <= T <= hip_ops.GROUND_PLANE_MAX_HYPOTHESES:
        raise ValueError(f"plane_triples: T must be in 1..{hip_ops.GROUND_PLANE_MAX_HYPOTHESES}, got {T}")
    r0, r1 = (H // 2, H) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 < r1 <= H:
        raise ValueError(f"plane_triples: rows must be (first, end) with 0 <= first < end <= {H}, got {rows}")
    rng = np.random.default_rng(int(seed))
    y = rng.integers(r0, r1, size=(T, 3), dtype=np.int64)
    x = rng.integers(0, W, size=(T, 3), dtype=np.int64)
    return torch.from_numpy((y * W + x).astype(np.int32))


def cos_of_tilt(max_tilt: float) -> float:
    """cos(max_tilt) for a tilt in [0, pi / 2) radians: the ``cos_tilt`` of ``hip_ops.ground_plane``."""
    max_tilt = float(max_tilt)
    if not 0.0 <= max_tilt < math.pi / 2:
        raise ValueError(f"ground_plane: max_tilt must be in [0, pi / 2) radians, got {max_tilt}")
    return math.cos(max_tilt)


def pose_angles(pose) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(height, pitch, roll), float64 [B] each on the host: the inverse of ``ground_pose`` on a pose [B, 12] (or [12]) of its layout --
    up = row 2 = (-cos p sin r, -cos p cos r, -sin p), so pitch = asin(-up_2) and roll = atan2(-up_0, -up_1); height = pose[11]."""
    p = torch.as_tensor(pose).detach().to("cpu", torch.float64).reshape(-1, 12)
    return p[:, 11].clone(), torch.asin((-p[:, 10]).clamp(-1.0, 1.0)), torch.atan2(-p[:, 8], -p[:, 9])


def ground_plane(depth: torch.Tensor, K: torch.Tensor, triples: Optional[torch.Tensor] = None, prior: Optional[torch.Tensor] = None,
                 hypotheses: int = 256, rows: Optional[Tuple[int, int]] = None, seed: int = 0, tol: float = 0.05, rel_tol: float = 0.01,
                 max_tilt: float = 0.35, height_range: Tuple[float, float] = (0.5, 4.0), min_cross: float = 1e-3, min_inliers: int = 64,
                 height: float = 1.65, pitch: float = 0.0, roll: float = 0.0, stride: Tuple[int, int] = (1, 1), near: float = 0.0,
                 far: float = float("inf"), confidence: Optional[torch.Tensor] = None, min_confidence: float = 0.0,
                 depth_std: Optional[torch.Tensor] = None, max_std: float = float("inf"), out: Optional[dict] = None) -> GroundPlane:
    """-> ``GroundPlane`` (see the module's text).  ``triples``: int32 [T, 3] (default ``plane_triples(H, W, hypotheses, rows, seed)``);
    ``prior``: fp32 [B, 12] (default ``ground_pose(height, pitch, roll)`` for every image); either may be on the host (it is uploaded).
    ``out``: {"pose", "stats"} to write into."""
    B, _, H, W = (int(v) for v in depth.shape)
    if triples is None:
        triples = plane_triples(H, W, hypotheses, rows, seed)
    if prior is None:
        prior = ground_pose(height, pitch, roll).expand(B, 12)
    triples = triples.to(device=depth.device, dtype=torch.int32).contiguous()
    prior = prior.to(device=depth.device, dtype=torch.float32).contiguous()
    res = hip_ops.ground_plane(depth, K, triples, prior, tol=tol, rel_tol=rel_tol, height_range=height_range, cos_tilt=cos_of_tilt(max_tilt),
                               min_cross=min_cross, min_inliers=min_inliers, stride=stride, near=near, far=far, confidence=confidence,
                               min_confidence=min_confidence, depth_std=depth_std, max_std=max_std, out=out)
    return GroundPlane(res["pose"], res["stats"])
