"""Statement F of include/objcavit_hip.h (the ground memory: the occupancy grid fused over time) in numpy on the CPU: fp32 arrays, ONE
numpy operation per rounding of the statement, integers in int32 -- what csrc/ground_fuse.hip must equal bit for bit --, and the
generators of the cases the host and the GPU tests share."""
from collections import namedtuple

import numpy as np

from ground_grid_ref import Spec

OUTPUTS = ("evidence", "state", "h_max", "first_occupied")
DEFAULTS = dict(free=2, occupied=4, decay=1, limit=32, free_at=4, occupied_at=6)
MAX_INT = 16383
Result = namedtuple("Result", OUTPUTS + ("inside",))

# GX x GY: one cell; a handful; ragged in both axes against the 16 x 16 tile and the 8-column scan; whole tiles; the default grid
GRIDS = (Spec(-0.5, 0.0, 1.0, 1, 1), Spec(-3.5, 0.0, 1.0, 7, 5), Spec(-1.65, 0.3, 0.1, 33, 129), Spec(-8.0, 0.0, 0.25, 64, 64))
DEFAULT_GRID = Spec(-10.0, 0.0, 0.1, 200, 400)
EXTRA_GRIDS = (Spec(-10.0, 0.0, 0.05, 400, 800),)        # checked on the CPU only
F = np.float32


def motion_of(dx=0.0, dy=0.0, dyaw=0.0) -> np.ndarray:
    """fp32 [4] = (cos dyaw, sin dyaw, dx, dy), made in float64 and rounded once: ``objcavit_amd.ground_memory.ego_motion``'s statement."""
    return np.array([np.cos(np.float64(dyaw)), np.sin(np.float64(dyaw)), dx, dy], dtype=np.float64).astype(F)


def motions(spec) -> dict:
    """The motions of the issue by name, each fp32 [4], for a grid's cell size."""
    cell = float(F(spec.cell))
    return {"identity": motion_of(), "shift": motion_of(3 * cell, -2 * cell), "half": motion_of(0.5 * cell, 0.5 * cell),
            "yaw": motion_of(0.0, 6.0, np.pi / 2), "small": motion_of(0.12, 0.31, 0.03), "far": motion_of(0.0, 100.0),
            "nan": np.array([1.0, 0.0, np.nan, 0.0], dtype=F)}


TRIPLES = (("identity", "shift", "half"), ("yaw", "small", "far"), ("shift", "nan", "small"))     # B = 3: a motion per image


def source(spec, motion: np.ndarray):
    """(inside bool [B, GY, GX], iy', ix' int64 [B, GY, GX]) of every output cell: the statement's warp, one fp32 operation at a time."""
    x0, y0, cell, GX, GY = F(spec.x0), F(spec.y0), F(spec.cell), int(spec.GX), int(spec.GY)
    motion = np.asarray(motion, dtype=F).reshape(-1, 4)
    c, s, tx, ty = (motion[:, i].reshape(-1, 1, 1) for i in range(4))
    with np.errstate(all="ignore"):
        xc = (x0 + (np.arange(GX, dtype=F) + F(0.5)) * cell).reshape(1, 1, GX)
        yc = (y0 + (np.arange(GY, dtype=F) + F(0.5)) * cell).reshape(1, GY, 1)
        px = ((c * xc) - (s * yc)) + tx
        py = ((s * xc) + (c * yc)) + ty
        fxi = np.floor((px - x0) / cell)
        fyi = np.floor((py - y0) / cell)
        assert px.dtype == F and fxi.dtype == F and fyi.dtype == F
        forget = ~np.isfinite(motion).all(1).reshape(-1, 1, 1)
        inside = ~forget & (fxi >= 0) & (fxi < F(GX)) & (fyi >= 0) & (fyi < F(GY))
    sy = np.where(inside, fyi, 0).astype(np.int64)
    sx = np.where(inside, fxi, 0).astype(np.int64)
    return inside, sy, sx


def fuse(state, spec, motion, prev_evidence=None, h_max=None, prev_h=None, free=2, occupied=4, decay=1, limit=32, free_at=4,
         occupied_at=6) -> Result:
    """Statement F: numpy in, numpy out (evidence int16, state uint8, h_max fp32 [B, GY, GX]; first_occupied fp32 [B, GX])."""
    state = np.asarray(state, dtype=np.uint8)
    B, GY, GX = state.shape
    assert (GX, GY) == (int(spec.GX), int(spec.GY))
    inside, sy, sx = source(spec, motion)
    b = np.arange(B).reshape(B, 1, 1)
    carried = np.zeros((B, GY, GX), dtype=np.int32)
    if prev_evidence is not None:
        carried = np.where(inside, np.asarray(prev_evidence, dtype=np.int16)[b, sy, sx].astype(np.int32), 0).astype(np.int32)
    m = np.abs(carried) - np.int32(decay)
    faded = np.where(m > 0, np.sign(carried) * m, 0).astype(np.int32)
    hit = np.where(state == 2, np.int32(occupied), np.where(state == 1, -np.int32(free), 0)).astype(np.int32)
    evidence = np.clip(faded + hit, -int(limit), int(limit)).astype(np.int32)
    fused = np.where(evidence >= occupied_at, 2, np.where(evidence <= -free_at, 1, 0)).astype(np.uint8)
    h = np.full((B, GY, GX), -np.inf, dtype=F)
    with np.errstate(invalid="ignore"):
        if h_max is not None:
            h = np.where(state == 2, np.asarray(h_max, dtype=F), h)
        if prev_h is not None:
            q = np.asarray(prev_h, dtype=F)[b, sy, sx]
            h = np.where(inside & (carried > 0) & (q > h), q, h)
        fused_h = np.where((evidence > 0) & (h > -np.inf), h, F(0.0)).astype(F)
    occ = fused == 2
    first = np.where(occ.any(1), occ.argmax(1), -1)
    y = F(spec.y0) + first.astype(F) * F(spec.cell)
    first_occupied = np.where(first >= 0, y, F(np.inf)).astype(F)
    return Result(evidence.astype(np.int16), fused, fused_h, first_occupied, inside)


def same_bytes(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
Case = namedtuple("Case", ["state", "h_max", "prev_evidence", "prev_h"])


def field(rng, shape, occupied=0.35, free=0.35) -> np.ndarray:
    """uint8 states: ``occupied`` of the cells 2, ``free`` of them 1, the rest 0."""
    u = rng.random(shape)
    return np.where(u < occupied, 2, np.where(u < occupied + free, 1, 0)).astype(np.uint8)


def case(spec, B=3, seed=0, limit=32) -> Case:
    """One step's inputs as a previous step could have left them: evidence anywhere in +-limit (a quarter of the cells 0), a fused h_max
    that is 0 where the evidence is not positive, and this step's heights with both signs, both zeros and a few -inf / NaN."""
    rng = np.random.default_rng(1000 + 17 * seed + int(spec.GX) * 3 + int(spec.GY))
    shape = (B, int(spec.GY), int(spec.GX))
    state = field(rng, shape)
    h_max = (rng.random(shape) * 3.0 - 0.5).astype(F)
    special = rng.random(shape)
    h_max[special < 0.02] = -np.inf
    h_max[(special >= 0.02) & (special < 0.04)] = np.nan
    h_max[(special >= 0.04) & (special < 0.06)] = -0.0
    prev_evidence = rng.integers(-limit, limit + 1, shape).astype(np.int16)
    prev_evidence[rng.random(shape) < 0.25] = 0
    prev_h = np.where(prev_evidence > 0, (rng.random(shape) * 3.0 - 0.5).astype(F), F(0.0)).astype(F)
    return Case(state, h_max, prev_evidence, prev_h)


SEQ_STEPS, SEQ_FADE_FROM, SEQ_B = 12, 8, 4


def sequence(spec, seed=0):
    """12 steps of a batch of four streams -> [(state uint8 [4, GY, GX], h_max fp32, motion fp32 [4, 4])] per step.  Image 0 drives and
    turns a little every step, image 1 stands, image 2 sees free ground everywhere and image 3 an obstacle everywhere (a random field
    does not reach the lower clamp by itself); from step 9 on every state is unknown, so that the evidence fades."""
    rng = np.random.default_rng(77 + seed + int(spec.GX))
    shape = (SEQ_B, int(spec.GY), int(spec.GX))
    cell = float(F(spec.cell))
    steps = []
    for t in range(SEQ_STEPS):
        state = field(rng, shape)
        state[2] = 1
        state[3] = 2
        if t >= SEQ_FADE_FROM:
            state[:] = 0
        h_max = (rng.random(shape) * 2.5).astype(F)
        motion = np.stack([motion_of(0.3 * cell, 1.7 * cell, 0.01 * (t % 3 - 1)), motion_of(), motion_of(), motion_of()], 0)
        steps.append((state, h_max, motion))
    return steps


def run_sequence(spec, steps, **options):
    """The statement fed forward: -> [Result] per step."""
    out, prev_e, prev_h = [], None, None
    for state, h_max, motion in steps:
        r = fuse(state, spec, motion, prev_e, h_max, prev_h, **options)
        out.append(r)
        prev_e, prev_h = r.evidence, r.h_max
    return out
