"""What is in front of the camera: the occupied cells of the bird's-eye grid grouped into obstacles, on the device.

``obstacles(grid)`` takes a ``GroundGrid`` (objcavit_amd/ground_grid.py: its ``state`` and, where it has them, ``count``, ``obstacle`` and
``h_max``) and returns, in at most seven launches (csrc/obstacles.hip) and without a copy of the grid to the host, an ``Obstacles``:

    cells    int32 [B, capacity, 8]  ix_min, ix_max, iy_min, iy_max, n, points, obstacle_points, root      (``CELL_FIELDS``)
    metres   fp32  [B, capacity, 8]  x_min, x_max, y_min, y_max, x_mean, y_mean, h_max, fill               (``METRE_FIELDS``)
    counts   int32 [B]               rows written = min(total, capacity); rows at or beyond it are all zero
    total    int32 [B]               obstacles kept
    labels   int32 [B, GY, GX]       -1 = not occupied, k = the cell belongs to row k, -2 = its obstacle was dropped or did not fit

Occupied cells (state 2) at most ``link`` cells apart along both axes belong to one obstacle: ``link=1`` is 8-connectivity, 2 or 3 bridges
the one- or two-cell holes that a depth map's sparse far field leaves in a wall.  An obstacle of at least ``min_cells`` cells and
``min_obstacle_points`` obstacle points is kept; the kept ones are ranked by their smallest iy * GX + ix, so row 0 is the nearest in
forward distance, ties left to right.  ``n`` = its cells, ``points`` / ``obstacle_points`` = the grid's counts summed over them, the extent
in cells and (outer edges) in metres, the centroid of its cells' centres, the highest point, ``fill`` = n over the extent's area.
Connected components by union-find with union by smaller index, in LDS per tile of 32 x 32 cells and across tile edges in memory; the
statistics are integer atomics at the component's root, so the list is the same bits on every call and equal to the statement (Statement
O of include/objcavit_hip.h, tests/obstacles_ref.py), not merely close to it.  No tracking over time and no classification: a list of
extents per frame -- or, through ``FusedGrid.as_grid()`` / ``ground_memory=dict(obstacles=True)``, of the grid fused over time
(objcavit_amd/ground_memory.py), whose cells do not flicker with the depth map; the rows are still not associated from step to step."""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Sequence

import torch

from . import hip_ops
from .ground_grid import GroundGrid

OUTPUTS = hip_ops.OBSTACLES_WANT
CELL_FIELDS = ("ix_min", "ix_max", "iy_min", "iy_max", "n", "points", "obstacle_points", "root")
METRE_FIELDS = ("x_min", "x_max", "y_min", "y_max", "x_mean", "y_mean", "h_max", "fill")
DEFAULTS = {"link": 1, "min_cells": 2, "min_obstacle_points": 0, "capacity": 64, "labels": False}      # the predictors' keyword
GRID_INPUTS = ("state", "count", "obstacle", "h_max")       # the grid outputs Statement O reads

Obstacles = namedtuple("Obstacles", OUTPUTS + ("x0", "y0", "cell"), defaults=(None,) * len(OUTPUTS) + (0.0, 0.0, 1.0))
Obstacles.__doc__ = """cells int32 [B, capacity, 8]; metres fp32 [B, capacity, 8]; counts, total int32 [B]; labels int32 [B, GY, GX] -- on
the device, None where not asked for -- and the grid's x0, y0, cell in metres."""


def _rows(self, b: int) -> List[dict]:
    """The kept rows of image ``b`` as a list of dicts {``CELL_FIELDS`` and ``METRE_FIELDS``: value}, nearest first.  COPIES the
    image's count and its rows to the host (a synchronisation): for the caller that wants Python objects, not for a pipeline."""
    if self.counts is None or self.cells is None or self.metres is None:
        raise ValueError("Obstacles.rows needs 'cells', 'metres' and 'counts'")
    n = int(self.counts[b])
    cells, metres = self.cells[b, :n].cpu().tolist(), self.metres[b, :n].cpu().tolist()
    return [dict(zip(CELL_FIELDS + METRE_FIELDS, c + m)) for c, m in zip(cells, metres)]


Obstacles.rows = _rows


def obstacles(grid: GroundGrid, link: int = 1, min_cells: int = 1, min_obstacle_points: int = 0, capacity: int = 64,
              want: Sequence[str] = OUTPUTS, out: Optional[dict] = None) -> Obstacles:
    """-> ``Obstacles`` (see the module's text) of a ``GroundGrid`` that has its ``state``; ``count``, ``obstacle`` and ``h_max`` are read
    where the grid has them (``points``, ``obstacle_points`` and ``h_max`` of a row are 0 without).  ``want``: the outputs to make;
    ``out``: {name: tensor} to write into."""
    if not isinstance(grid, GroundGrid) or grid.state is None:
        raise ValueError("obstacles: expected a GroundGrid with its 'state' (ground_grid(..., want=(..., 'state')))")
    B, GY, GX = (int(v) for v in grid.state.shape)
    res = hip_ops.obstacles(grid.state, (grid.x0, grid.y0, grid.cell, GX, GY), count=grid.count, obstacle=grid.obstacle, h_max=grid.h_max,
                            link=link, min_cells=min_cells, min_obstacle_points=min_obstacle_points, capacity=capacity, want=want, out=out)
    return Obstacles(*(res.get(n) for n in OUTPUTS), x0=grid.x0, y0=grid.y0, cell=grid.cell)
