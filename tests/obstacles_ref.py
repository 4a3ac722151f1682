"""Statement O (include/objcavit_hip.h) in numpy on the CPU: the obstacle list csrc/obstacles.hip is compared with.

The components are found by a flood fill over the (2 link + 1)^2 window, started at every occupied cell not yet reached in row-major
order -- so the cell a fill starts from is its component's smallest iy * GX + ix, the root.  The statistics are Python / int64 integers;
the float formulas are the statement's, word for word: the four edges in fp32 with one numpy scalar operation per rounding, the two means
and the fill in float64 one operation at a time and rounded once to fp32, the height through the order-preserving integer key written out
on the bit patterns.  Nothing here has a tolerance: the tests ask for EQUALITY of every output.

``pattern`` makes the occupancy patterns the tests share; TILE is the kernel's tile (OCV_OBSTACLES_TILE: seams lie at its multiples) and
GRIDS the ground grid's own sizes plus the one of two tiles by two tiles and one cell more in each direction."""
from collections import namedtuple

import numpy as np
import torch

import ground_grid_ref

TILE = 32
LINKS = (1, 2, 3)
CELL_FIELDS = ("ix_min", "ix_max", "iy_min", "iy_max", "n", "points", "obstacle_points", "root")
METRE_FIELDS = ("x_min", "x_max", "y_min", "y_max", "x_mean", "y_mean", "h_max", "fill")
OUTPUTS = ("cells", "metres", "counts", "total", "labels")
CLAMP = 2 ** 31 - 1

Spec = ground_grid_ref.Spec
# 1 x 1, 7 x 5, 64 x 48, 33 x 129 (the grid's), and 2 x 2 tiles + 1
GRIDS = tuple(ground_grid_ref.GRIDS[:4]) + (Spec(-3.21, 0.37, 0.2, 2 * TILE + 1, 2 * TILE + 1),)
Result = namedtuple("Result", OUTPUTS + ("roots",))


def roots_of(occupied: np.ndarray, link: int) -> np.ndarray:
    """int64 [GY, GX]: the root (smallest iy * GX + ix of its component) of every occupied cell, -1 elsewhere.  Flood fill."""
    GY, GX = occupied.shape
    root = np.full((GY, GX), -1, dtype=np.int64)
    todo = occupied.copy()
    for start in np.flatnonzero(occupied):
        sy, sx = divmod(int(start), GX)
        if not todo[sy, sx]:
            continue
        todo[sy, sx] = False
        root[sy, sx] = start
        stack = [(sy, sx)]
        while stack:
            y, x = stack.pop()
            y0, x0 = max(0, y - link), max(0, x - link)
            win = todo[y0:y + link + 1, x0:x + link + 1]
            ys, xs = np.nonzero(win)
            if len(ys):
                win[ys, xs] = False
                root[y0 + ys, x0 + xs] = start
                stack.extend(zip((y0 + ys).tolist(), (x0 + xs).tolist()))
    return root


def key_of(h: np.ndarray) -> np.ndarray:
    """The order-preserving integer image of fp32 values (csrc/float_key.hpp), as uint32."""
    u = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k: int) -> np.float32:
    k = np.uint32(k)
    return (np.array([k & np.uint32(0x7fffffff) if k >> 31 else ~k], dtype=np.uint32)).view(np.float32)[0]


def obstacles(state, spec, count=None, obstacle=None, h_max=None, link=1, min_cells=1, min_obstacle_points=0, cap=64) -> Result:
    """Statement O.  state uint8 [B, GY, GX] (+ count, obstacle int32, h_max fp32 of that shape, or None) on the host, ``spec`` = (x0, y0,
    cell, GX, GY) -> ``Result`` of torch tensors: cells int32 [B, cap, 8], metres fp32 [B, cap, 8], counts / total int32 [B], labels int32
    [B, GY, GX], roots int64 [B, GY, GX] (the root of every occupied cell, -1 elsewhere: not an output of the kernel)."""
    state = np.asarray(state)
    B, GY, GX = state.shape
    assert (GX, GY) == (spec[3], spec[4]) and link in LINKS and min_cells >= 1 and min_obstacle_points >= 0 and cap >= 1
    x0, y0, cell = (np.float32(v) for v in spec[:3])
    cnt, obs, hmx = (None if t is None else np.asarray(t) for t in (count, obstacle, h_max))
    cells = np.zeros((B, cap, 8), dtype=np.int32)
    metres = np.zeros((B, cap, 8), dtype=np.float32)
    labels = np.full((B, GY, GX), -1, dtype=np.int32)
    counts, total = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    roots = np.stack([roots_of(state[b] == 2, link) for b in range(B)], 0)
    for b in range(B):
        flat = roots[b].reshape(-1)
        where = np.flatnonzero(flat >= 0)
        labels[b].reshape(-1)[where] = -2
        order = np.argsort(flat[where], kind="stable")
        members = np.split(where[order], np.flatnonzero(np.diff(flat[where][order])) + 1) if len(where) else []
        k = 0
        for m in members:                                                       # by root, ascending
            root = int(flat[m[0]])
            iy, ix = m // GX, m % GX
            n = int(len(m))
            points = 0 if cnt is None else int(cnt[b].reshape(-1)[m].astype(np.int64).sum())
            obstacle_points = 0 if obs is None else int(obs[b].reshape(-1)[m].astype(np.int64).sum())
            if n < min_cells or obstacle_points < min_obstacle_points:
                continue
            if k < cap:
                ix_min, ix_max, iy_min, iy_max = int(ix.min()), int(ix.max()), int(iy.min()), int(iy.max())
                sum_ix, sum_iy = int(ix.astype(np.int64).sum()), int(iy.astype(np.int64).sum())
                cells[b, k] = (ix_min, ix_max, iy_min, iy_max, n, min(points, CLAMP), min(obstacle_points, CLAMP), root)
                height = np.float32(0.0) if hmx is None else unkey(key_of(hmx[b].reshape(-1)[m]).max())
                x_mean = np.float32(np.float64(x0) + (np.float64(sum_ix) / np.float64(n) + np.float64(0.5)) * np.float64(cell))
                y_mean = np.float32(np.float64(y0) + (np.float64(sum_iy) / np.float64(n) + np.float64(0.5)) * np.float64(cell))
                fill = np.float32(np.float64(n) / (np.float64(ix_max - ix_min + 1) * np.float64(iy_max - iy_min + 1)))
                metres[b, k] = (x0 + np.float32(ix_min) * cell, x0 + np.float32(ix_max + 1) * cell, y0 + np.float32(iy_min) * cell,
                                y0 + np.float32(iy_max + 1) * cell, x_mean, y_mean, height, fill)
                labels[b].reshape(-1)[m] = k
            k += 1
        total[b], counts[b] = k, min(k, cap)
    return Result(*(torch.from_numpy(a) for a in (cells, metres, counts, total, labels, roots)))


# ---------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------
PATTERNS = ("empty", "full", "corners", "serpentine", "comb", "diagonal", "gaps", "isolated", "bernoulli30", "bernoulli41", "bernoulli60")


def _seam(n: int) -> int:
    """The first seam of a side of n cells, or its middle when the side has one tile."""
    return TILE if n > TILE else max(1, n // 2)


def pattern(name: str, GX: int, GY: int, link: int = 1, seed: int = 0) -> np.ndarray:
    """bool [GY, GX]: the occupied cells.  Cells a pattern would put outside a small grid are dropped."""
    occ = np.zeros((GY, GX), dtype=bool)

    def put(y, x):
        if 0 <= y < GY and 0 <= x < GX:
            occ[y, x] = True

    if name == "full":
        occ[:] = True
    elif name == "corners":
        occ[0, 0] = occ[0, -1] = occ[-1, 0] = occ[-1, -1] = True
    elif name == "serpentine":                              # one cell wide: full rows joined alternately at the right and the left end
        occ[0::2] = True
        occ[1::4, -1] = True
        occ[3::4, 0] = True
    elif name == "comb":                                    # teeth link + 1 apart (not adjacent) that join only in the last row
        occ[:, 0::link + 1] = True
        occ[-1] = True
    elif name == "diagonal":                                # two blobs that touch only across the corner (sy, sx)
        sy, sx = _seam(GY), _seam(GX)
        for d in range(1, 4):
            for e in range(1, 4):
                put(sy - d, sx - e)
                put(sy + d - 1, sx + e - 1)
    elif name == "gaps":                                    # pairs link, link + 1 and link + 2 cells apart: across a vertical seam, a
        sy, sx = _seam(GY), _seam(GX)                       # horizontal one and a tile corner
        for j, d in enumerate((link, link + 1, link + 2)):
            a = d // 2
            put(2 + 9 * j, sx - 1 - a), put(2 + 9 * j, sx - 1 - a + d)                  # along x, at rows far from each other
            put(sy - 1 - a, 2 + 9 * j), put(sy - 1 - a + d, 2 + 9 * j)                  # along y
            put(sy - 1 - a, sx + 6 + 9 * j - 1 - a), put(sy - 1 - a + d, sx + 6 + 9 * j - 1 - a + d)      # diagonal, across seam rows
        for j, d in enumerate((link, link + 1, link + 2)):                               # and straight across the corner itself
            if j == seed % 3:
                a = d // 2
                put(sy - 1 - a, sx - 1 - a), put(sy - 1 - a + d, sx - 1 - a + d)
    elif name == "isolated":
        occ[0::link + 1, 0::link + 1] = True
    elif name.startswith("bernoulli"):
        occ = np.random.default_rng(1000 * seed + int(name[9:])).random((GY, GX)) < int(name[9:]) / 100.0
    else:
        assert name == "empty", name
    return occ


def grid_inputs(occupied: np.ndarray, seed: int = 0, big: bool = False):
    """(state uint8, count int32, obstacle int32, h_max fp32) [B, GY, GX] around the occupancy ``occupied`` bool [B, GY, GX]: state 2
    where occupied and 0 / 1 elsewhere, obstacle <= count, heights of either sign.  ``big``: counts of 2^30, so that a component's sums
    pass 2^31 and are clamped."""
    rng = np.random.default_rng(77 + seed)
    shape = occupied.shape
    state = np.where(occupied, 2, rng.integers(0, 2, shape)).astype(np.uint8)
    count = rng.integers(1, 60, shape).astype(np.int32)
    if big:
        count[:] = 2 ** 30
    obstacle = np.minimum(count, rng.integers(0, 40, shape) + (2 ** 29 if big else 0)).astype(np.int32)
    h_max = (rng.random(shape) * 3.0 - 0.5).astype(np.float32)
    return state, count, obstacle, h_max
