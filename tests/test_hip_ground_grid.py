"""-m gpu: csrc/ground_grid.hip against Statement G in fp32 torch (tests/ground_grid_ref.py) -- EQUAL, not close: counts, obstacle counts
and states element for element, the heights and the column scan by value -- with strides, filters and thresholds, at full size on the
contention case, between poisoned guards, inside a captured graph, and (in a child process) through the predict path that carries it."""
import os
import subprocess
import sys

import pytest
import torch

import ground_grid_ref as ref
import test_hip_memory_bounds as bounds

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
POISON = 0x7FC0DEAD                       # a NaN payload no computation produces
ALL = ref.OUTPUTS
INT = ("count", "obstacle", "state")


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def grid_of(spec):
    return (spec.x0, spec.y0, spec.cell, spec.GX, spec.GY)


_CASES = {}


def case(H, W, bad=None, kind="camera"):
    key = (H, W, bad, kind)
    if key not in _CASES:
        _CASES[key] = ref.case(H, W, bad=bad, kind=kind)
    return _CASES[key]


_WANT = {}


def reference(H, W, bad, kind, spec, **kw):
    """The statement on a case, made once per (case, grid, options) and left unchanged."""
    key = (H, W, bad, kind, spec, tuple(sorted((k, v) for k, v in kw.items() if not isinstance(v, torch.Tensor))))
    if key not in _WANT:
        c = case(H, W, bad, kind)
        _WANT[key] = ref.ground_grid(c.depth, c.K, c.pose, spec, **dict(c.options, **kw))
    return _WANT[key]


def poisoned(n, spec, names=ALL, byte=0xAB):
    out = {}
    for name in names:
        shape = (n, spec.GX) if name == "first_occupied" else (n, spec.GY, spec.GX)
        if name == "state":
            out[name] = torch.full(shape, byte, dtype=torch.uint8, device="cuda")
        elif name in INT:
            out[name] = torch.full(shape, POISON ^ byte, dtype=torch.int32, device="cuda")
        else:
            out[name] = torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    return out


def check(got, want, what=""):
    """``got``: the wrapper's dict (any subset of the outputs) against the reference's Grid: EQUAL."""
    for name, t in got.items():
        g, w = t.cpu(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, tuple(g.shape))
        if name in INT:
            assert torch.equal(g, w), (what, name, int((g != w).sum()), "elements differ")
        else:
            assert not bool((g.view(torch.int32) == POISON).any()), (what, name, "elements never written")
            assert bool((g == w).all()), (what, name, int((g != w).sum()), "elements differ")      # by value: -0 == +0, inf == inf, no NaN


def run(ops, c, spec, names=ALL, out=None, **kw):
    return ops.ground_grid(c.depth.cuda(), c.K.cuda(), c.pose.cuda(), grid_of(spec), want=names, out=out,
                           **dict(dict(c.options, near=ref.NEAR, far=ref.FAR, min_obstacle_points=1), **kw))


# ---------------------------------------------------------------------------
# equality with the statement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ref.GRIDS, ids=lambda s: f"{s.GX}x{s.GY}x{s.cell}")
@pytest.mark.parametrize("shape", ref.CASE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_outputs_equal_the_statement(ops, shape, spec):
    """B = 3: flat ground with a slab, a model-like map with NaN, +-inf and out-of-range cells, a wall (whole pixel columns in a handful
    of cells); one image with a bad camera or a non-finite pose, rotating with the case.  The one-cell grid puts every point into one
    record (the 64-bit sum, the worst contention); 400 x 400 has far more cells than the on-chip table, nearly all empty."""
    H, W = shape
    n = ref.CASE_SHAPES.index(shape) * len(ref.GRIDS) + ref.GRIDS.index(spec)
    bad, kind = n % 3, ("camera", "pose")[(n // 3) % 2]
    c = case(H, W, bad, kind)
    want = reference(H, W, bad, kind, spec)
    assert not want.count[bad].any() and not want.state[bad].any() and bool(torch.isinf(want.first_occupied[bad]).all())
    assert int(want.count.sum()) > 0
    out = poisoned(ref.CASE_B, spec)
    got = run(ops, c, spec, out=out)
    assert all(got[k] is out[k] for k in ALL)
    check(got, want, (shape, spec))
    # the bad image: all-zero, unknown, +inf
    for name in ALL[:-1]:
        assert not got[name][bad].any(), name
    assert bool(torch.isinf(got["first_occupied"][bad]).all()) and bool((got["first_occupied"][bad] > 0).all())
    # every element is written, in integers: a second call over another poison gives the same bytes
    again = run(ops, c, spec, out=poisoned(ref.CASE_B, spec, byte=0x54))
    for k in ALL:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), (shape, spec, k)


@pytest.mark.parametrize("names", [("count",), ("state",), ("first_occupied",), ("h_mean", "obstacle"), ("h_min", "h_max", "first_occupied"),
                                   ("state", "count", "h_mean")], ids=lambda v: "+".join(v))
def test_subsets_of_the_outputs(ops, names):
    H, W = 37, 131
    spec = ref.GRIDS[2]
    c = case(H, W)
    want = reference(H, W, None, "camera", spec)
    full = run(ops, c, spec, out=poisoned(ref.CASE_B, spec))
    got = run(ops, c, spec, names=names, out=poisoned(ref.CASE_B, spec, names))
    assert set(got) == set(names)
    check(got, want, names)
    for n in names:
        assert torch.equal(got[n].view(torch.uint8), full[n].view(torch.uint8)), n


def test_bad_options_are_refused(ops):
    c = case(8, 8)
    d, k, p = c.depth.cuda(), c.K.cuda(), c.pose.cuda()
    g = grid_of(ref.GRIDS[1])
    for kw in (dict(want=()), dict(want=("count", "depth")), dict(band=(1.0, 0.0)), dict(band=(0.0, 1e4)), dict(min_points=0),
               dict(min_obstacle_points=0), dict(stride=(0, 1)), dict(near=2.0, far=1.0), dict(obstacle_height=float("nan"))):
        with pytest.raises(ValueError):
            ops.ground_grid(d, k, p, g, **kw)
    for bad in ((0.0, 0.0, 0.0, 4, 4), (0.0, 0.0, 1.0, 0, 4), (0.0, 0.0, 1.0, 4), (float("nan"), 0.0, 1.0, 4, 4), (0.0, 0.0, 1.0, 1 << 16, 1 << 16)):
        with pytest.raises(ValueError):
            ops.ground_grid(d, k, p, bad)
    with pytest.raises(ValueError):
        ops.ground_grid(d, k, p[:, :9].contiguous(), g)
    with pytest.raises(ValueError):
        ops.ground_grid(d, k[:2], p, g)


# ---------------------------------------------------------------------------
# options
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(19, 70), (37, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stride_filters_and_thresholds(ops, shape):
    H, W = shape
    c = case(H, W)
    spec = ref.GRIDS[2]
    conf = ref.confidence_map(H, W)
    std = ref.confidence_map(H, W, seed=9)
    plain = reference(H, W, None, "camera", spec)
    for tag, kw in (("stride", dict(stride=(2, 3))), ("confidence", dict(confidence=conf, min_confidence=0.5)),
                    ("std", dict(depth_std=std, max_std=0.5)), ("both", dict(stride=(3, 2), confidence=conf, min_confidence=0.25, depth_std=std, max_std=0.75)),
                    ("thresholds", dict(min_points=3, min_obstacle_points=4)), ("coarse thresholds", dict(min_points=2, min_obstacle_points=2, stride=(1, 2)))):
        want = ref.ground_grid(c.depth, c.K, c.pose, spec, **dict(c.options, **kw))
        dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        got = run(ops, c, spec, out=poisoned(ref.CASE_B, spec), **dict(dict(min_obstacle_points=1), **dev))
        check(got, want, (shape, tag))
        assert not torch.equal(want.state, plain.state), tag                   # the option matters on this case


def test_wall_at_full_size_into_a_few_cells(ops):
    """B = 1, 480 x 640, the wall into the (7, 5, 1.0) grid with a band that takes every row: all of the 3 x 10^5 pixels are points and
    those within the grid's 7 m (2.7 x 10^5) land in seven cells."""
    H, W = 480, 640
    spec = ref.GRIDS[1]
    c = case(H, W)
    one = ref.Case(c.depth[2:3].contiguous(), c.K[2:3].contiguous(), c.pose[2:3].contiguous(), dict(c.options, band=(-10.0, 10.0)))
    want = ref.ground_grid(one.depth, one.K, one.pose, spec, **one.options)
    assert int(ref.keep(one.depth, one.K, one.pose).sum()) == H * W and int(want.count.sum()) > 200000 and int((want.count > 0).sum()) <= 7
    got = run(ops, one, spec, out=poisoned(1, spec))
    check(got, want, "full size")
    again = run(ops, one, spec, out=poisoned(1, spec, byte=0x11))
    for k in ALL:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), k


def test_image_index_fills_a_batch_and_the_workspace_may_be_the_callers(ops):
    from objcavit_amd import _lib
    H, W = 21, 132
    spec = ref.GRIDS[3]
    c = case(H, W)
    d, k, p = c.depth.cuda(), c.K.cuda(), c.pose.cuda()
    kw = dict(c.options, near=ref.NEAR, far=ref.FAR, min_obstacle_points=1)
    a = ops.ground_grid(d, k, p, grid_of(spec), out=poisoned(3, spec), **kw)
    check(a, reference(H, W, None, "camera", spec), "whole batch")
    pick = [2, 0, 1]
    out = poisoned(3, spec)
    need = int(_lib.load().ocv_ground_grid_workspace_bytes(1, spec.GX, spec.GY))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for slot, i in enumerate(pick):
        got = ops.ground_grid(d[i:i + 1], k[i:i + 1], p[i:i + 1], grid_of(spec), out=out, image_index=slot, workspace=ws, **kw)
        assert got["count"] is out["count"]
    for n in ALL:
        assert torch.equal(out[n].view(torch.uint8), a[n][pick].contiguous().view(torch.uint8)), n
    with pytest.raises(ValueError):
        ops.ground_grid(d[:1], k[:1], p[:1], grid_of(spec), out=out, image_index=3, **kw)
    with pytest.raises(ValueError):
        ops.ground_grid(d, k, p, grid_of(spec), out={"count": out["count"]}, **kw)
    with pytest.raises(_lib.HipLibraryError):
        ops.ground_grid(d, k, p, grid_of(spec), workspace=ws[:need - 8], **kw)       # too small for three images: refused, no launch
    fresh = ops.ground_grid(d, k, p, grid_of(spec), **kw)
    for n in ALL:
        assert torch.equal(fresh[n].view(torch.uint8), a[n].view(torch.uint8)), n


# ---------------------------------------------------------------------------
# guarded memory: a row of tests/test_hip_memory_bounds.py's table (its accounting test wants every *_fwd entry point in a row)
# ---------------------------------------------------------------------------
ROW = "ground_grid|19x70 33x129"


def _grid_row(c):
    """19 x 70 (two pixel tiles, the second ragged) into (33, 129, 0.1), B = 3; once with every output, once with one alone.  Every
    element of every output and of the workspace is written (``c.out``)."""
    H, W = 19, 70
    spec = ref.GRIDS[3]
    cs = case(H, W, 1, "pose")
    want = reference(H, W, 1, "pose", spec)
    d, k, p = c.put(cs.depth), c.put(cs.K), c.put(cs.pose)
    need = int(c.lib.ocv_ground_grid_workspace_bytes(ref.CASE_B, spec.GX, spec.GY))
    kw = dict(cs.options, near=ref.NEAR, far=ref.FAR, min_obstacle_points=1)
    for names in (ALL, ("first_occupied",)):
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        got = c.ops.ground_grid(d, k, p, grid_of(spec), want=names, workspace=ws, **kw)
        check(got, want, ("guarded", names))
        c.out(ws, *got.values())


if ROW not in bounds.ROWS:
    bounds.row(ROW)(_grid_row)


def test_launches_between_poisoned_guards():
    bounds.run_row(ROW)
    assert "ocv_ground_grid_fwd" in bounds.RAN[ROW]


def test_captured_graph_replays_with_a_new_map_camera_and_pose():
    """In a fresh child process (tests/ground_grid_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "ground_grid_graph_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


def test_predict_path_carries_the_grid():
    """``Predictor`` and ``PipelinedPredictor`` with the keyword, in a fresh child process (tests/ground_grid_predict_child.py, which says
    what it checks and why it is a process of its own) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "ground_grid_predict_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
