"""An occupancy grid with memory: the bird's-eye grid fused over time, on the device.

A monocular depth map flickers from frame to frame, and with it every cell of ``GroundGrid.state``.  ``GroundMemory`` keeps per-cell
EVIDENCE -- a small signed integer, positive for "occupied", negative for "free" -- and updates it once per step, in one launch
(csrc/ground_fuse.hip), without a copy of the grid to the host:

    1. carry    every cell takes the evidence of the cell of the PREVIOUS map that its centre was in, through the vehicle's motion
                since the previous step (``ego_motion``: a rotation about the vertical axis and a shift, nearest cell; nothing is carried
                from outside the grid)
    2. fade     the carried evidence moves ``decay`` towards 0
    3. observe  +``occupied`` where this step's grid says occupied, -``free`` where it says free, nothing where it does not know
    4. clamp    to +-``limit``: how long an obstacle is remembered once it is out of sight

and returns a ``FusedGrid``:

    evidence        int16 [B, GY, GX]  the evidence after this step (what the next step carries)
    state           uint8 [B, GY, GX]  2 = occupied (evidence >= ``occupied_at``), 1 = free (evidence <= -``free_at``), 0 = unknown
    h_max           fp32  [B, GY, GX]  the highest point seen of a cell with positive evidence (this step's or the carried one), else 0
    first_occupied  fp32  [B, GX]      per lateral column, the forward distance of its nearest cell whose FUSED state is occupied

With the defaults (free 2, occupied 4, decay 1, limit 32, free_at 4, occupied_at 6) a cell is occupied after two occupied frames in a
row, survives a frame in which it is unknown, and one that has reached the limit stays occupied for 26 frames out of sight.  ``FusedGrid.as_grid()``
is a ``GroundGrid`` of the fused outputs, so ``obstacles(fused.as_grid())`` lists the obstacles of the fused map.  Everything is integer
arithmetic per cell behind an fp32 warp whose every operation is rounded on its own: the map is the same bits on every call and equal
to the statement (Statement F of include/objcavit_hip.h, tests/ground_memory_ref.py), not merely close to it.  The images of a batch are
independent streams.  The motion is the caller's (odometry, an IMU): it is not estimated here; there is no ray casting of free space."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence

import torch

from . import hip_ops
from .ground_grid import GroundGrid

OUTPUTS = hip_ops.GROUND_FUSE_WANT
OPTIONS = ("free", "occupied", "decay", "limit", "free_at", "occupied_at")
DEFAULTS = {"free": 2, "occupied": 4, "decay": 1, "limit": 32, "free_at": 4, "occupied_at": 6}
_LOWEST = {"free": 0, "occupied": 0, "decay": 0, "limit": 1, "free_at": 1, "occupied_at": 1}

FusedGrid = namedtuple("FusedGrid", OUTPUTS + ("x0", "y0", "cell"), defaults=(None,) * len(OUTPUTS) + (0.0, 0.0, 1.0))
FusedGrid.__doc__ = """evidence int16 [B, GY, GX]; state uint8 [B, GY, GX]; h_max fp32 [B, GY, GX]; first_occupied fp32 [B, GX] -- on the
device, None where not asked for -- and the grid's x0, y0, cell in metres."""


def _as_grid(self) -> GroundGrid:
    """A ``GroundGrid`` that holds the fused ``state``, ``h_max`` and ``first_occupied`` (by reference; its other outputs are None)."""
    return GroundGrid(state=self.state, h_max=self.h_max, first_occupied=self.first_occupied, x0=self.x0, y0=self.y0, cell=self.cell)


FusedGrid.as_grid = _as_grid


def ego_motion(dx=0.0, dy=0.0, dyaw=0.0) -> torch.Tensor:
    """fp32 [B, 4] on the host = (cos dyaw, sin dyaw, dx, dy) per image (scalars or sequences of one length), made in float64 and rounded
    once: the motion ``GroundMemory.update`` takes.  ``dx``, ``dy``: the vehicle's displacement since the previous step, in metres in
    the PREVIOUS step's ground frame (x right, y forward); ``dyaw``: its turn in radians, counter-clockwise seen from above.  A point at
    p in the current ground frame was at R(dyaw) p + (dx, dy) in the previous one.  ``ego_motion()`` is the identity: a standing camera."""
    cols = [torch.as_tensor(v, dtype=torch.float64).reshape(-1) for v in (dx, dy, dyaw)]
    B = max(int(c.numel()) for c in cols)
    if any(int(c.numel()) not in (1, B) for c in cols):
        raise ValueError("ego_motion: dx, dy and dyaw must be scalars or sequences of one length")
    x, y, a = (c.expand(B) for c in cols)
    return torch.stack([a.cos(), a.sin(), x, y], 1).to(torch.float32)


def options_of(given: dict, who: str = "ground_memory") -> dict:
    """The six integers of Statement F from a dict that may hold some of them (default ``DEFAULTS``), each checked against its range."""
    out = {}
    for name in OPTIONS:
        v = given.get(name, DEFAULTS[name])
        if isinstance(v, bool) or int(v) != v or not _LOWEST[name] <= int(v) <= hip_ops.GROUND_FUSE_MAX:
            raise ValueError(f"{who}: {name} must be an integer in {_LOWEST[name]}..{hip_ops.GROUND_FUSE_MAX}, got {v}")
        out[name] = int(v)
    return out


def check_want(want, who: str = "ground_memory") -> tuple:
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or set(want) - set(OUTPUTS):
        raise ValueError(f"{who}: want must name some of {OUTPUTS} (got {want})")
    return tuple(n for n in OUTPUTS if n in want)


class GroundMemory:
    """``GroundMemory(spec, free=2, occupied=4, decay=1, limit=32, free_at=4, occupied_at=6, want=OUTPUTS)``: the memory of one batch of
    camera streams over the grid ``spec`` = (x0, y0, cell, GX, GY).  ``update(grid, motion=None, reset=False)`` fuses one step's
    ``GroundGrid`` (its ``state`` and, where it has it, ``h_max``) and returns the ``FusedGrid``; ``motion``: ``ego_motion(...)`` since the
    previous update, fp32 [B, 4] on the host or the device (None: the identity); ``reset=True`` forgets before this step, ``reset()``
    before the next one.  The memory keeps the last step's ``evidence`` and ``h_max`` BY REFERENCE and never writes into them: every step's
    outputs are fresh tensors, so a result handed out is never overwritten (and ``evidence`` and ``h_max`` are made even when ``want``
    leaves them out; they are then not handed out).  One launch per update on the current stream, nothing read on the host."""

    def __init__(self, spec: Sequence, want: Sequence[str] = OUTPUTS, **options):
        bad = set(options) - set(OPTIONS)
        if bad:
            raise ValueError(f"GroundMemory: unknown option(s) {sorted(bad)}; expected some of {OPTIONS}")
        if len(tuple(spec)) != 5:
            raise ValueError(f"GroundMemory: spec must be the grid's (x0, y0, cell, GX, GY), got {spec}")
        self.spec = (float(spec[0]), float(spec[1]), float(spec[2]), int(spec[3]), int(spec[4]))
        self.options = options_of(options, "GroundMemory")
        self.want = check_want(want, "GroundMemory")
        self.evidence: Optional[torch.Tensor] = None
        self.h_max: Optional[torch.Tensor] = None
        self._identity = {}

    def reset(self) -> None:
        """Forget: the next update starts from nothing."""
        self.evidence = self.h_max = None

    def _motion(self, motion, B: int, device) -> torch.Tensor:
        if motion is None:
            key = (device, B)
            if key not in self._identity:
                self._identity[key] = ego_motion().expand(B, 4).contiguous().to(device)
            return self._identity[key]
        motion = torch.as_tensor(motion, dtype=torch.float32)
        if tuple(motion.shape) != (B, 4):
            raise ValueError(f"GroundMemory: motion must be [{B}, 4] (ego_motion(dx, dy, dyaw)), got {tuple(motion.shape)}")
        return motion.to(device=device, dtype=torch.float32).contiguous()

    def update(self, grid: GroundGrid, motion=None, reset: bool = False) -> FusedGrid:
        if not isinstance(grid, GroundGrid) or grid.state is None:
            raise ValueError("GroundMemory: expected a GroundGrid with its 'state' (ground_grid(..., want=(..., 'state')))")
        if reset:
            self.reset()
        B = int(grid.state.shape[0])
        if self.evidence is not None and self.evidence.shape != grid.state.shape:
            raise ValueError(f"GroundMemory: the grid changed from {tuple(self.evidence.shape)} to {tuple(grid.state.shape)} (reset() first)")
        made = tuple(n for n in OUTPUTS if n in self.want or n in ("evidence", "h_max"))
        res = hip_ops.ground_fuse(grid.state, self.spec, self._motion(motion, B, grid.state.device), prev_evidence=self.evidence,
                                  h_max=grid.h_max, prev_h=self.h_max, want=made, **self.options)
        self.evidence, self.h_max = res["evidence"], res["h_max"]
        x0, y0, cell = self.spec[:3]
        return FusedGrid(*(res[n] if n in self.want else None for n in OUTPUTS), x0=x0, y0=y0, cell=cell)
