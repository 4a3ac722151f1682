"""-m "not gpu": the ground memory's host side -- the properties of Statement F's reference (tests/ground_memory_ref.py) that the GPU
test relies on, ``ego_motion``, ``FusedGrid``, the library's symbol and argument checks (no launch happens), the wrappers' signatures,
the predictors' ``ground_memory`` keyword and, with stand-in wrappers, the order of a step's launches and what the keyword changes."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import ground_memory_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------
ALL_GRIDS = ref.GRIDS + (ref.DEFAULT_GRID,) + ref.EXTRA_GRIDS


@pytest.mark.parametrize("spec", ALL_GRIDS, ids=lambda s: f"{s.GX}x{s.GY}")
def test_identity_maps_every_cell_onto_itself_and_a_whole_cell_motion_is_an_exact_shift(spec):
    m = ref.motions(spec)
    inside, sy, sx = ref.source(spec, np.stack([m["identity"], m["shift"]]))
    iy, ix = np.mgrid[0:spec.GY, 0:spec.GX]
    assert inside[0].all() and (sy[0] == iy).all() and (sx[0] == ix).all()
    want = (ix + 3 < spec.GX) & (iy - 2 >= 0)
    assert (inside[1] == want).all() and (sx[1][want] == (ix + 3)[want]).all() and (sy[1][want] == (iy - 2)[want]).all()
    if spec.GX > 3 and spec.GY > 2:
        assert want.any() and not want.all()


@pytest.mark.parametrize("spec", ref.GRIDS[1:] + (ref.DEFAULT_GRID,), ids=lambda s: f"{s.GX}x{s.GY}")
def test_the_motions_do_what_their_names_say(spec):
    m = ref.motions(spec)
    for name in ("yaw", "small"):                                       # the rotated cases have cells both inside and outside
        inside = ref.source(spec, m[name])[0]                           # (cells of 1 m keep all of a 0.3 m step inside)
        assert inside.any() and (not inside.all() or (name == "small" and spec.cell >= 1.0)), name
    assert not ref.source(spec, m["far"])[0].any() and not ref.source(spec, m["nan"])[0].any()
    # the half-cell shift lands ON cell edges: (px - x0) / cell is a whole number there, and floor keeps it
    x0, cell = np.float32(spec.x0), np.float32(spec.cell)
    xc = x0 + (np.arange(spec.GX, dtype=np.float32) + np.float32(0.5)) * cell
    q = ((xc + m["half"][2]) - x0) / cell
    assert (q == np.floor(q)).any()
    # a NaN motion forgets: the result is that of no previous map at all
    c = ref.case(spec, B=1, seed=3)
    forgot = ref.fuse(c.state, spec, m["nan"], c.prev_evidence, c.h_max, c.prev_h)
    fresh = ref.fuse(c.state, spec, m["identity"], None, c.h_max, None)
    assert all(ref.same_bytes(getattr(forgot, n), getattr(fresh, n)) for n in ref.OUTPUTS)
    # a null previous map is a zero map
    zero = ref.fuse(c.state, spec, m["small"], np.zeros_like(c.prev_evidence), c.h_max, c.prev_h)
    assert all(ref.same_bytes(getattr(zero, n), getattr(fresh, n)) for n in ref.OUTPUTS)


def test_the_statement_on_a_hand_made_case():
    spec = ref.Spec(-1.0, 2.0, 0.5, 4, 3)
    state = np.array([[[2, 1, 0, 2], [0, 0, 1, 2], [2, 2, 0, 0]]], dtype=np.uint8)
    prev = np.array([[[5, -3, 1, -1], [0, 7, -8, 8], [-2, 2, 32, -32]]], dtype=np.int16)
    h = np.arange(12, dtype=np.float32).reshape(1, 3, 4) / 4 + 1
    ph = np.where(prev > 0, np.float32(2.0), np.float32(0.0)).astype(np.float32)
    r = ref.fuse(state, spec, ref.motion_of(), prev, h, ph, limit=8)
    #            4+4 clamp -2-2  0    0+4 |  0  6  -7-2 clamp  7+4 clamp |  -1+4  1+4  8 (31 clamp)  -8
    assert r.evidence.tolist() == [[[8, -4, 0, 4], [0, 6, -8, 8], [3, 5, 8, -8]]]
    assert r.state.tolist() == [[[2, 1, 0, 0], [0, 2, 1, 2], [0, 0, 2, 1]]]
    assert r.h_max.tolist() == [[[2.0, 0.0, 0.0, 1.75], [0.0, 2.0, 0.0, 2.75], [3.0, 3.25, 2.0, 0.0]]]
    assert r.first_occupied.tolist() == [[2.0, 2.5, 3.0, 2.5]]
    none = ref.fuse(np.zeros_like(state), spec, ref.motion_of(), None)
    assert not none.evidence.any() and not none.state.any() and np.isposinf(none.first_occupied).all()
    # without this step's heights the carried one is all there is; without the carried one, this step's where it is occupied
    assert ref.fuse(state, spec, ref.motion_of(), prev, None, ph, limit=8).h_max[0, 0].tolist() == [2.0, 0.0, 0.0, 0.0]
    assert ref.fuse(state, spec, ref.motion_of(), prev, h, None, limit=8).h_max[0, 2].tolist() == [3.0, 3.25, 0.0, 0.0]


@pytest.mark.parametrize("limit", (8, 32))
def test_the_sequences_reach_every_state_the_clamps_and_a_fade_to_zero(limit):
    """What the GPU test's sequences must exercise, asserted so that a vacuous case fails.  At the default limit of 32 eight observed
    steps cannot reach a clamp (4 + 7 * 3 = 25), so the clamps are asserted at limit 8."""
    spec = ref.GRIDS[2]
    steps = ref.sequence(spec)
    assert len(steps) == ref.SEQ_STEPS and all(not s[0].any() for s in steps[ref.SEQ_FADE_FROM:]) and steps[ref.SEQ_FADE_FROM - 1][0].any()
    out = ref.run_sequence(spec, steps, **dict(ref.DEFAULTS, limit=limit))
    states = set()
    for r in out:
        states.update(np.unique(r.state).tolist())
    assert states == {0, 1, 2}
    ev = np.stack([r.evidence for r in out]).astype(np.int32)
    if limit == 8:
        assert (ev == limit).any() and (ev == -limit).any()
        assert (ev[:, 0] == limit).any()                                       # (a random field need not reach the LOWER clamp by itself)
        assert (ev[:, 2] == -limit).all(axis=(1, 2)).any() and (ev[:, 3] == limit).all(axis=(1, 2)).any()
    assert np.abs(ev).max() <= limit
    fade = ev[ref.SEQ_FADE_FROM - 1:, 1]                                       # the standing stream: a cell is its own source
    assert ((fade[0] == 4) & (fade[-1] == 0)).any() and ((fade[-2] == 1) & (fade[-1] == 0)).any()
    assert (np.abs(fade[-1]) <= np.maximum(np.abs(fade[0]) - 4, 0)).all()
    moved = ref.source(spec, steps[0][2])[0]
    assert moved[0].any() and not moved[0].all() and moved[1:].all()           # the driving stream loses cells at the border


# ---------------------------------------------------------------------------
# ego_motion, FusedGrid, GroundMemory
# ---------------------------------------------------------------------------
def test_ego_motion_is_the_identity_by_default_and_composes_as_float64_says():
    from objcavit_amd.ground_memory import ego_motion
    assert ego_motion().dtype == torch.float32 and ego_motion().tolist() == [[1.0, 0.0, 0.0, 0.0]]
    m = ego_motion([0.12, -3.0, 0.0], [0.31, 0.5, 6.0], [0.03, -1.2, math.pi / 2])
    assert tuple(m.shape) == (3, 4)
    for row, (dx, dy, a) in zip(m.tolist(), ((0.12, 0.31, 0.03), (-3.0, 0.5, -1.2), (0.0, 6.0, math.pi / 2))):
        assert row == [float(np.float32(math.cos(a))), float(np.float32(math.sin(a))), float(np.float32(dx)), float(np.float32(dy))]
        assert np.array_equal(ref.motion_of(dx, dy, a), np.array(row, dtype=np.float32))
    # two steps composed: a point of the newest frame in the oldest frame, against float64
    (c1, s1, x1, y1), (c2, s2, x2, y2) = m[0].double().tolist(), m[1].double().tolist()
    p = np.array([1.5, 7.25])
    mid = np.array([c2 * p[0] - s2 * p[1] + x2, s2 * p[0] + c2 * p[1] + y2])
    old = np.array([c1 * mid[0] - s1 * mid[1] + x1, s1 * mid[0] + c1 * mid[1] + y1])
    a = 0.03 - 1.2
    R1 = np.array([[math.cos(0.03), -math.sin(0.03)], [math.sin(0.03), math.cos(0.03)]])
    want = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]) @ p + R1 @ np.array([-3.0, 0.5]) + np.array([0.12, 0.31])
    assert np.abs(old - want).max() < 1e-6
    # counter-clockwise seen from above: after a left turn of 90 degrees, what is ahead now was to the LEFT before
    q = ego_motion(0.0, 0.0, math.pi / 2)[0].double().tolist()
    ahead = (q[0] * 0.0 - q[1] * 1.0 + q[2], q[1] * 0.0 + q[0] * 1.0 + q[3])
    assert abs(ahead[0] + 1.0) < 1e-6 and abs(ahead[1]) < 1e-6
    with pytest.raises(ValueError):
        ego_motion([0.0, 1.0], [0.0, 1.0, 2.0])


def test_fused_grid_and_ground_memory_without_a_device():
    from objcavit_amd import ground_memory as gm, hip_ops
    from objcavit_amd._lib import HipLibraryError
    from objcavit_amd.ground_grid import GroundGrid
    from objcavit_amd.obstacles import obstacles
    assert gm.OUTPUTS == hip_ops.GROUND_FUSE_WANT == ref.OUTPUTS and gm.DEFAULTS == ref.DEFAULTS
    assert gm.FusedGrid._fields == ref.OUTPUTS + ("x0", "y0", "cell")
    state = torch.zeros(1, 4, 4, dtype=torch.uint8)
    f = gm.FusedGrid(evidence=state.short(), state=state, h_max=state.float(), first_occupied=torch.zeros(1, 4), x0=-1.0, y0=0.5, cell=0.5)
    g = f.as_grid()
    assert isinstance(g, GroundGrid) and g.state is f.state and g.h_max is f.h_max and g.first_occupied is f.first_occupied
    assert (g.x0, g.y0, g.cell) == (-1.0, 0.5, 0.5) and g.count is None and g.obstacle is None and g.h_min is None and g.h_mean is None
    with pytest.raises(HipLibraryError):
        obstacles(g)                                                            # it is a grid to the list: refused for the device only
    mem = gm.GroundMemory((-1.0, 0.5, 0.5, 4, 4), limit=8)
    assert mem.options == dict(ref.DEFAULTS, limit=8) and mem.want == ref.OUTPUTS and mem.evidence is None
    with pytest.raises(HipLibraryError):
        mem.update(GroundGrid(state=state, x0=-1.0, y0=0.5, cell=0.5))
    with pytest.raises(ValueError):
        mem.update(GroundGrid(count=state.int()))
    with pytest.raises(ValueError, match="limits"):
        gm.GroundMemory((-1.0, 0.5, 0.5, 4, 4), limits=8)
    for bad in (dict(limit=0), dict(free=-1), dict(decay=1.5), dict(occupied=True), dict(free_at=0), dict(occupied_at=16384)):
        with pytest.raises(ValueError):
            gm.GroundMemory((-1.0, 0.5, 0.5, 4, 4), **bad)
    with pytest.raises(ValueError):
        gm.GroundMemory((-1.0, 0.5, 0.5, 4, 4), want=("evidence", "count"))
    assert list(inspect.signature(mem.update).parameters) == ["grid", "motion", "reset"]


# ---------------------------------------------------------------------------
# the library and the wrapper
# ---------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported(lib):
    from objcavit_amd import _lib, build, hip_ops
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_ground_fuse_fwd\s*\(", header) and "STATEMENT F" in header
    assert re.search(r"#define\s+OCV_ABI_VERSION\s+5\b", header) and lib.ocv_abi_version() == 5
    assert "ocv_ground_fuse_fwd" in _lib.PROTOTYPES and hasattr(lib, "ocv_ground_fuse_fwd") and "ground_fuse.hip" in build.SOURCES
    assert re.search(r"#define\s+OCV_GROUND_FUSE_TILE\s+%d\b" % hip_ops.GROUND_FUSE_TILE, header)
    assert hip_ops.GROUND_FUSE_MAX == ref.MAX_INT
    text = open(os.path.join(ROOT, "objcavit_amd", "csrc", "ground_fuse.hip")).read()
    assert '#include "rounded_mul.hpp"' in text and "gg_mul(" in text
    assert not re.search(r"\batomic(Add|Max|Min|CAS|Exch)\b", text)               # no atomics at all: nothing is joined


def test_wrapper_has_the_documented_signature_and_refuses_host_tensors():
    from objcavit_amd import hip_ops
    from objcavit_amd._lib import HipLibraryError
    params = inspect.signature(hip_ops.ground_fuse).parameters
    assert list(params) == ["state", "spec", "motion", "prev_evidence", "h_max", "prev_h", "free", "occupied", "decay", "limit", "free_at",
                            "occupied_at", "want", "out", "image_index"]
    assert [params[n].default for n in ("free", "occupied", "decay", "limit", "free_at", "occupied_at")] == [2, 4, 1, 32, 4, 6]
    assert params["want"].default == ref.OUTPUTS and params["prev_evidence"].default is None and params["image_index"].default == 0
    with pytest.raises(HipLibraryError):
        hip_ops.ground_fuse(torch.zeros(1, 4, 4, dtype=torch.uint8), (-1.0, 0.0, 0.5, 4, 4), torch.zeros(1, 4))


# The entry point's refusals, ONE table for this file (made-up addresses, never dereferenced) and for tests/test_hip_ground_memory.py
# (real buffers).  A value ("name", k) stands for the address of operand ``name`` plus k bytes.
BASE = dict(B=1, GX=4, GY=4, x0=-1.0, y0=0.0, cell=0.5, free=2, occupied=4, decay=1, limit=32, free_at=4, occupied_at=6)
POINTERS = ("state", "h_max", "prev_e", "prev_h", "motion", "evidence", "fstate", "fh", "first")
N = 16                                                                          # cells of the base case
REFUSALS = [
    (dict(state=None), "null"), (dict(motion=None), "null"), (dict(evidence=None, fstate=None, fh=None, first=None), "no output"),
    (dict(B=0), "sizes"), (dict(GX=0), "sizes"), (dict(GY=-1), "sizes"),
    (dict(GX=1 << 16, GY=1 << 15), "2^31"), (dict(B=1 << 12, GX=1 << 10, GY=1 << 9), "2^31"), (dict(GX=(1 << 24) + 1, GY=1), "2^24"),
    (dict(cell=0.0), "cell"), (dict(cell=-0.1), "cell"), (dict(cell=NAN), "cell"), (dict(cell=INF), "cell"),
    (dict(x0=NAN), "origin"), (dict(y0=INF), "origin"), (dict(x0=-INF), "origin"),
    (dict(free=-1), "free ="), (dict(free=16384), "free ="), (dict(occupied=-1), "occupied ="), (dict(occupied=16384), "occupied ="),
    (dict(decay=-1), "decay ="), (dict(decay=16384), "decay ="), (dict(limit=0), "limit ="), (dict(limit=16384), "limit ="),
    (dict(free_at=0), "free_at ="), (dict(free_at=16384), "free_at ="), (dict(occupied_at=0), "occupied_at ="),
    (dict(occupied_at=16384), "occupied_at ="),
    (dict(motion=("motion", 4)), "misaligned"), (dict(motion=("motion", 8)), "misaligned"), (dict(h_max=("h_max", 2)), "misaligned"),
    (dict(prev_h=("prev_h", 1)), "misaligned"), (dict(fh=("fh", 2)), "misaligned"), (dict(first=("first", 3)), "misaligned"),
    (dict(prev_e=("prev_e", 1)), "misaligned"), (dict(evidence=("evidence", 1)), "misaligned"),
    (dict(evidence=("prev_e", 0)), "overlaps"), (dict(evidence=("prev_e", 2 * N - 2)), "overlaps"),
    (dict(evidence=("prev_e", -2 * N + 2)), "overlaps"), (dict(fh=("prev_h", 0)), "overlaps"), (dict(fh=("prev_h", 4 * N - 4)), "overlaps"),
    (dict(evidence=("prev_h", 0)), "overlaps"), (dict(fh=("prev_e", 0)), "overlaps"), (dict(fstate=("state", N - 1)), "overlaps"),
    (dict(fh=("h_max", 0)), "overlaps"), (dict(first=("prev_h", 4 * N - 4)), "overlaps"),
]


def call_entry(lib, addresses, kw, stream=None):
    """``ocv_ground_fuse_fwd`` on ``BASE`` and the operands' ``addresses`` with ``kw`` on top."""
    a = dict(BASE, **addresses)
    for k, v in kw.items():
        a[k] = addresses[v[0]] + v[1] if isinstance(v, tuple) else v
    return lib.ocv_ground_fuse_fwd(a["state"], a["h_max"], a["prev_e"], a["prev_h"], a["motion"], a["B"], a["GX"], a["GY"], a["x0"], a["y0"],
                                   a["cell"], a["free"], a["occupied"], a["decay"], a["limit"], a["free_at"], a["occupied_at"], a["evidence"],
                                   a["fstate"], a["fh"], a["first"], stream)


@pytest.mark.parametrize("kw,word", REFUSALS)
def test_bad_arguments_are_refused_before_any_launch(lib, kw, word):
    made_up = {n: (i + 1) << 20 for i, n in enumerate(POINTERS)}
    assert call_entry(lib, made_up, kw) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_ground_fuse_fwd:") and word in msg, msg


# ---------------------------------------------------------------------------
# the predictors' keyword
# ---------------------------------------------------------------------------
def _args():
    from objcavit_amd.config import make_args
    return make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip")


def test_predictors_validate_the_ground_memory_keyword():
    from objcavit_amd import predict
    from objcavit_amd.predict import PipelinedPredictor, Predictor, PredictResult, _ObjectsResult, _Step
    args = _args()
    pr = Predictor(None, args, ground_grid={}, ground_memory={})
    assert pr.ends.memory == dict(ref.DEFAULTS, obstacles=False, want=ref.OUTPUTS)
    assert Predictor(None, args, ground_grid={}).ends.memory is None and Predictor(None, args).ends.memory is None
    o = Predictor(None, args, ground_grid={}, obstacles={}, ground_memory=dict(free=1, occupied=3, decay=0, limit=9, free_at=2, occupied_at=5,
                                                                                 obstacles=True, want=("state", "evidence")))
    assert o.ends.memory == dict(free=1, occupied=3, decay=0, limit=9, free_at=2, occupied_at=5, obstacles=True, want=("evidence", "state"))
    assert o.ends.obstacles == dict(link=1, min_cells=2, min_obstacle_points=0, capacity=64, labels=False)     # the source is not its option
    example = torch.zeros(1, 8, 12, 3, dtype=torch.uint8)
    for make in (lambda **kw: Predictor(None, args, **kw), lambda **kw: PipelinedPredictor(None, args, example, **kw)):
        with pytest.raises(ValueError, match="ground_grid"):
            make(ground_memory={})                                              # refused without the grid
        for bad in (dict(limits=2), dict(limit=0), dict(limit=16384), dict(free=-1), dict(decay=0.5), dict(occupied=True), dict(free_at=0),
                    dict(occupied_at=0), dict(want=()), dict(want=("count",))):
            with pytest.raises(ValueError) as e:
                make(ground_grid={}, ground_memory=bad)
            if "limits" in bad:
                assert "limits" in str(e.value)                                 # an unknown key is named
    for fn in (Predictor.__init__, PipelinedPredictor.__init__):
        assert inspect.signature(fn).parameters["ground_memory"].default is None
    for fn in (Predictor.__call__, PipelinedPredictor.submit):
        params = inspect.signature(fn).parameters
        assert params["ego_motion"].default is None and params["reset"].default is False
    # it runs between the grid and its list, in a table of its own; an attribute and no field; its tensors are recorded for the caller
    assert [r.keyword for r in predict.TEMPORAL_READOUTS] == ["ground_memory"]
    assert [r.keyword for r in predict.RUN_ORDER][-3:] == ["ground_grid", "ground_memory", "obstacles"]
    assert predict.RUN_ORDER == predict.READOUTS + predict.TEMPORAL_READOUTS + predict.DERIVED_READOUTS
    assert "ground_memory" not in [r.keyword for r in predict.ALL_READOUTS]
    t = predict.TEMPORAL_READOUTS[0]
    assert t.attr == "ground_memory" and t.options == "memory" and t.streamed == slice(4) and t.needs == ("K",) and t.maps(o.ends.memory) == ()
    assert [r.keyword for r, _ in o.ends.readouts] == ["ground_grid", "ground_memory", "obstacles"]
    assert PredictResult.ground_memory is None and PredictResult._fields == ("depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence")
    res = _ObjectsResult(1, 2, 3, 4, 5, ground_memory="fused")
    assert res.ground_memory == "fused" and res.obstacles is None and tuple(res) == (1, 2, 3, 4, 5, None, None)
    assert res._replace(depth=0).ground_memory == "fused"
    assert _Step._fields[-1] == "memory" and _Step(1, 2, 3, 4, 5, 6).memory is None


def test_ego_motion_of_a_call_is_uploaded_as_the_four_vector():
    from objcavit_amd.ground_memory import ego_motion
    from objcavit_amd.predict import Predictor
    ends = Predictor(None, _args(), ground_grid={}, ground_memory={}).ends
    cpu = torch.device("cpu")
    assert ends.motion_on(None, False, cpu, 2) == {"motion": None, "reset": False}
    three = [[0.12, 0.31, 0.03], [0.0, 6.0, math.pi / 2]]
    got = ends.motion_on(three, True, cpu, 2)
    assert got["reset"] is True and got["motion"].dtype == torch.float32
    assert torch.equal(got["motion"], ego_motion([0.12, 0.0], [0.31, 6.0], [0.03, math.pi / 2]))
    four = ego_motion(1.0, 2.0, 0.5).expand(2, 4)
    assert torch.equal(ends.motion_on(four, False, cpu, 2)["motion"], four) and ends.motion_on(four, False, cpu, 2)["motion"].is_contiguous()
    t3 = torch.tensor(three)                                                    # an fp32 tensor: its values, as they are, in float64
    assert torch.equal(ends.motion_on(t3, False, cpu, 2)["motion"], ego_motion(t3[:, 0], t3[:, 1], t3[:, 2]))
    for bad in ([[0.0, 0.0]], torch.zeros(3, 4), torch.zeros(2, 5), torch.zeros(4)):
        with pytest.raises(ValueError):
            ends.motion_on(bad, False, cpu, 2)
    assert Predictor(None, _args(), ground_grid={}).ends.motion_on(three, False, cpu, 2) is None          # no keyword: nothing is held
    step = ends.step(ends.frames_of(torch.zeros(2, 8, 12, 3, dtype=torch.uint8), "frames_u8"), ego_motion=three)
    assert any(t is step.memory["motion"] for t in step.held())


class _Recorder:
    """Stand-ins for the wrappers of a step with the grid, the memory and the list: they log what they were asked for."""

    def __init__(self, monkeypatch):
        from objcavit_amd import hip_ops
        self.calls, self.fused = [], []
        monkeypatch.setattr(hip_ops, "depth_finalize", self.depth_finalize)
        monkeypatch.setattr(hip_ops, "ground_grid", self.ground_grid)
        monkeypatch.setattr(hip_ops, "ground_fuse", self.ground_fuse)
        monkeypatch.setattr(hip_ops, "obstacles", self.obstacles)

    def depth_finalize(self, pred, min_depth, max_depth, size, want=("depth",), **kw):
        return {n: torch.zeros((int(pred.shape[0]), 1) + tuple(size)) for n in want}

    def ground_grid(self, depth, K, pose, grid, want=(), out=None, image_index=0, **kw):
        self.calls.append(("ground_grid", tuple(want), tuple(sorted(out)), image_index))
        self.grid = out
        return out

    def ground_fuse(self, state, spec, motion, prev_evidence=None, h_max=None, prev_h=None, want=(), **kw):
        g = self.grid
        self.calls.append(("ground_fuse", tuple(want), spec, state is g["state"], h_max is g["h_max"], motion, prev_evidence, prev_h, kw))
        self.fused.append({n: torch.zeros(tuple(state.shape)) for n in want})
        return self.fused[-1]

    def obstacles(self, state, spec, count=None, obstacle=None, h_max=None, want=(), **kw):
        self.calls.append(("obstacles", state, count, obstacle, h_max))
        return {n: n for n in want}


def test_the_step_fuses_between_the_grid_and_the_list_and_a_rerun_does_not_advance_the_memory(monkeypatch):
    from types import SimpleNamespace
    from objcavit_amd import predict
    from objcavit_amd.ground_memory import FusedGrid
    args = _args()
    rec = _Recorder(monkeypatch)
    frames = torch.zeros(2, 8, 12, 3, dtype=torch.uint8)
    out = SimpleNamespace(depth_pred=torch.ones(2, 1, 4, 6), bin_edges=torch.zeros(2, 9))
    K = torch.tensor([[10.0, 10.0, 6.0, 4.0]] * 2)

    def run(ends, **kw):
        del rec.calls[:]
        step = ends.step(ends.frames_of(frames, "frames_u8"), intrinsics=K, **kw)
        return step, ends.finish(out, None, step, 0, ("depth",))

    # without the keyword a step calls exactly what it calls today: the grid asked for what it was asked for, then the list on the grid's own
    ends = predict._Ends(args, flip_tta=False, ground_grid={"want": ("first_occupied",)}, obstacles={})
    _, res = run(ends)
    assert [c[0] for c in rec.calls] == ["ground_grid", "obstacles"] and res.ground_memory is None
    assert rec.calls[0] == ("ground_grid", ("count", "obstacle", "h_max", "state", "first_occupied"), ("count", "first_occupied", "h_max", "obstacle", "state"), 0)
    g = rec.grid
    assert rec.calls[1][1] is g["state"] and rec.calls[1][2] is g["count"] and rec.calls[1][3] is g["obstacle"] and rec.calls[1][4] is g["h_max"]
    ends = predict._Ends(args, flip_tta=False, ground_grid={"want": ("first_occupied",)})
    _, res = run(ends)
    assert rec.calls == [("ground_grid", ("first_occupied",), ("first_occupied",), 0)] and type(res.ground_memory) is type(None)

    # with it: grid, then fuse, then list; the grid's state and h_max are made for the memory and not handed out
    ends = predict._Ends(args, flip_tta=False, ground_grid={"want": ("first_occupied",)}, obstacles={}, ground_memory={"limit": 9, "want": ("state", "first_occupied")})
    step1, res = run(ends, ego_motion=[[0.1, 0.2, 0.0]] * 2)
    assert [c[0] for c in rec.calls] == ["ground_grid", "ground_fuse", "obstacles"]
    assert {"state", "h_max"} <= set(rec.calls[0][1]) and res.ground.state is None and res.ground.h_max is None
    name, want, spec, same_state, same_h, motion, prev_e, prev_h, kw = rec.calls[1]
    assert want == ref.OUTPUTS and spec == (-10.0, 0.0, 0.1, 200, 400) and same_state and same_h and prev_e is None and prev_h is None
    assert kw == dict(ref.DEFAULTS, limit=9) and motion is step1.memory["motion"] and tuple(motion.shape) == (2, 4)
    f = res.ground_memory
    assert isinstance(f, FusedGrid) and f.state is rec.fused[0]["state"] and f.first_occupied is rec.fused[0]["first_occupied"]
    assert f.evidence is None and f.h_max is None and (f.x0, f.y0, f.cell) == (-10.0, 0.0, 0.1)
    assert rec.calls[2][1] is rec.grid["state"] and rec.calls[2][2] is rec.grid["count"]          # the list still reads the frame's grid
    # the second step reads what the first one wrote; the motion defaults to the identity
    step2, res2 = run(ends)
    name, want, spec, same_state, same_h, motion, prev_e, prev_h, kw = rec.calls[1]
    assert prev_e is rec.fused[0]["evidence"] and prev_h is rec.fused[0]["h_max"] and motion.tolist() == [[1.0, 0.0, 0.0, 0.0]] * 2
    assert ends._memory[0] is rec.fused[1]["evidence"] and ends._memory[1] is rec.fused[1]["h_max"]
    # a re-run of the FIRST step reads what it had read -- nothing -- and its own motion, and does not advance the memory
    del rec.calls[:]
    again = ends.finish(out, None, step1, 0, ("depth",))
    name, want, spec, same_state, same_h, motion, prev_e, prev_h, kw = rec.calls[1]
    assert prev_e is None and prev_h is None and motion is step1.memory["motion"]
    assert again.ground_memory.state is rec.fused[2]["state"] and ends._memory[0] is rec.fused[1]["evidence"]
    # ... and of the second step: the first step's outputs
    del rec.calls[:]
    ends.finish(out, None, step2, 0, ("depth",))
    assert rec.calls[1][6] is rec.fused[0]["evidence"] and ends._memory[0] is rec.fused[1]["evidence"]
    # reset=True forgets before that step
    _, res3 = run(ends, reset=True)
    assert rec.calls[1][6] is None and rec.calls[1][7] is None and ends._memory[0] is rec.fused[-1]["evidence"]
    # without intrinsics neither the grid nor the memory runs, and the memory is left alone
    kept = ends._memory
    del rec.calls[:]
    res = ends.finish(out, None, ends.step(ends.frames_of(frames, "frames_u8")), 0, ("depth",))
    assert not rec.calls and type(res) is predict.PredictResult and ends._memory is kept

    # obstacles=True hands the list the fused tensors, and no counts
    ends = predict._Ends(args, flip_tta=False, ground_grid={}, obstacles={}, ground_memory={"obstacles": True, "want": ("evidence",)})
    _, res = run(ends)
    assert [c[0] for c in rec.calls] == ["ground_grid", "ground_fuse", "obstacles"] and "state" in rec.calls[1][1]
    assert rec.calls[2][1] is rec.fused[-1]["state"] and rec.calls[2][4] is rec.fused[-1]["h_max"] and rec.calls[2][2] is None and rec.calls[2][3] is None
    assert res.ground_memory.state is None and res.ground_memory.evidence is rec.fused[-1]["evidence"] and res.obstacles is not None
