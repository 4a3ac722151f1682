"""-m "not gpu": the obstacle list's host side -- Statement O's reference (tests/obstacles_ref.py) against a brute-force transitive
closure and, where scipy imports, against ``scipy.ndimage.label`` / ``find_objects``; the union / find header of csrc/obstacles.hip as
plain host C++ in a stand-alone driver (tests/obstacles_uf_driver.cpp) built under the address and undefined-behaviour sanitizers and run
as a process of its own; the library's symbols, workspace size and argument checks (no launch happens), the wrappers and the predictors'
``obstacles`` keyword."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import obstacles_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


_ROOTS = {}


def roots(name, spec, link, seed=0):
    """The reference's roots of a pattern, made once."""
    key = (name, spec.GX, spec.GY, link, seed)
    if key not in _ROOTS:
        occ = ref.pattern(name, spec.GX, spec.GY, link, seed)
        _ROOTS[key] = (occ, ref.roots_of(occ, link))
    return _ROOTS[key]


# ---------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------
def _closure_roots(occ, link):
    """Brute force: the adjacency matrix of the occupied cells, closed under composition; the root of a cell is the smallest cell it reaches."""
    GY, GX = occ.shape
    cells = [(y, x) for y in range(GY) for x in range(GX) if occ[y, x]]
    out = np.full((GY, GX), -1, dtype=np.int64)
    if not cells:
        return out
    ys, xs = np.array([c[0] for c in cells]), np.array([c[1] for c in cells])
    reach = (np.abs(ys[:, None] - ys[None]) <= link) & (np.abs(xs[:, None] - xs[None]) <= link)
    for _ in range(len(cells)):
        wider = (reach.astype(np.int64) @ reach.astype(np.int64)) > 0
        if (wider == reach).all():
            break
        reach = wider
    index = ys * GX + xs
    for i, (y, x) in enumerate(cells):
        out[y, x] = index[reach[i]].min()
    return out


@pytest.mark.parametrize("link", ref.LINKS)
def test_components_equal_the_transitive_closure_on_small_grids(link):
    rng = np.random.default_rng(5 + link)
    grids = [rng.random((GY, GX)) < p for GY, GX in ((1, 1), (1, 6), (6, 1), (3, 5), (6, 6), (5, 6)) for p in (0.2, 0.4, 0.6)]
    grids += [ref.pattern(name, GX, GY, link) for name in ref.PATTERNS for GX, GY in ((6, 6), (5, 4))]
    seen = set()
    for occ in grids:
        got, want = ref.roots_of(occ, link), _closure_roots(occ, link)
        assert np.array_equal(got, want), (link, occ.astype(int))
        seen.add(len(np.unique(got[got >= 0])))
    assert len(seen) >= 4                                                       # empty, one, several components


@pytest.mark.parametrize("spec", ref.GRIDS, ids=lambda s: f"{s.GX}x{s.GY}")
def test_link_1_equals_scipy_label_and_find_objects(spec):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name in ref.PATTERNS:
        occ, root = roots(name, spec, 1)
        lab, n = ndimage.label(occ, structure=np.ones((3, 3), dtype=bool))
        assert ((lab > 0) == (root >= 0)).all(), name
        pairs = set(zip(lab[occ].tolist(), root[occ].tolist()))
        assert len(pairs) == n == len({p[1] for p in pairs}) == len({p[0] for p in pairs}), name      # a bijection of the labels
        state = np.where(occ, 2, 0).astype(np.uint8)[None]
        got = ref.obstacles(state, spec, link=1, cap=max(1, n))
        assert int(got.total[0]) == n == int(got.counts[0]) or n == 0, name
        boxes = {}
        for k, sl in enumerate(ndimage.find_objects(lab)):
            r = int(root[lab == k + 1].min())
            boxes[r] = (sl[1].start, sl[1].stop - 1, sl[0].start, sl[0].stop - 1, int((lab == k + 1).sum()))
        rows = got.cells[0, :int(got.counts[0])].tolist()
        assert [r[7] for r in rows] == sorted(boxes), name                      # ranked by root
        for r in rows:
            assert tuple(r[:5]) == boxes[r[7]], (name, r)
        if n:
            assert got.labels[0][torch.from_numpy(occ)].min() >= 0 and int(got.labels[0].max()) == n - 1


def test_statistics_filters_capacity_and_formulas():
    spec = ref.Spec(-1.5, 2.0, 0.25, 7, 5)
    occ = np.zeros((1, 5, 7), dtype=bool)
    occ[0, 0, 0:2] = True                   # root 0: two cells
    occ[0, 2, 4] = True                     # root 18: one cell
    occ[0, 3:5, 5:7] = True                 # root 26: joins 18 diagonally under link 1 -> one component of five with root 18
    occ[0, 4, 0] = True                     # root 28: one cell
    state, count, obstacle, h_max = ref.grid_inputs(occ, seed=3)
    got = ref.obstacles(state, spec, count, obstacle, h_max, link=1, cap=4)
    assert got.total.tolist() == [3] and got.counts.tolist() == [3] and got.cells[0, :, 7].tolist() == [0, 18, 28, 0]
    a = got.cells[0, 1].tolist()
    m = occ[0] & (got.roots[0].numpy() == 18)
    assert a[:5] == [4, 6, 2, 4, 5] and a[5] == int(count[0][m].sum()) and a[6] == int(obstacle[0][m].sum())
    x = got.metres[0, 1].tolist()
    assert x[0] == -1.5 + 4 * 0.25 and x[1] == -1.5 + 7 * 0.25 and x[2] == 2.0 + 2 * 0.25 and x[3] == 2.0 + 5 * 0.25
    assert x[4] == np.float32(-1.5 + ((4 + 5 + 6 + 5 + 6) / 5 + 0.5) * 0.25) and x[6] == float(h_max[0][m].max()) and x[7] == np.float32(5 / 9)
    assert not got.cells[0, 3].any() and not got.metres[0, 3].any()
    assert got.labels[0, 0, 0] == 0 and got.labels[0, 2, 4] == 1 and got.labels[0, 4, 6] == 1 and got.labels[0, 4, 0] == 2 and got.labels[0, 1, 1] == -1
    # filters: min_cells drops the single cell, and the ranks close up; the labels of a dropped component are -2
    f = ref.obstacles(state, spec, count, obstacle, h_max, link=1, min_cells=2, cap=4)
    assert f.total.tolist() == [2] and f.cells[0, :2, 7].tolist() == [0, 18] and f.labels[0, 4, 0] == -2
    big = int(obstacle[0][m].sum())
    f = ref.obstacles(state, spec, count, obstacle, h_max, link=1, min_obstacle_points=big, cap=4)
    assert 18 in f.cells[0, :int(f.counts[0]), 7].tolist() and all(r[6] >= big for r in f.cells[0, :int(f.counts[0])].tolist())
    # capacity below the number kept: total says so, the rest is labelled -2
    c = ref.obstacles(state, spec, count, obstacle, h_max, link=1, cap=2)
    assert c.total.tolist() == [3] and c.counts.tolist() == [2] and c.labels[0, 4, 0] == -2 and c.labels[0, 2, 4] == 1
    # null inputs: zeros in their columns
    z = ref.obstacles(state, spec, link=1, cap=4)
    assert not z.cells[0, :, 5:7].any() and not z.metres[0, :, 6].any() and torch.equal(z.cells[0, :, :5], got.cells[0, :, :5])
    # link 2 joins nothing new; link 3 reaches from (0, 1) to (2, 4): the first two components become one
    assert ref.obstacles(state, spec, link=2, cap=4).total.tolist() == [3]
    wide = ref.obstacles(state, spec, link=3, cap=4)
    assert wide.total.tolist() == [2] and wide.cells[0, :2, 7].tolist() == [0, 28] and wide.cells[0, 0, 4] == 7
    # sums beyond 2^31 are clamped
    s2, c2, o2, h2 = ref.grid_inputs(np.ones((1, 5, 7), dtype=bool), big=True)
    full = ref.obstacles(s2, spec, c2, o2, h2, cap=1)
    assert full.cells[0, 0].tolist()[:7] == [0, 6, 0, 4, 35, ref.CLAMP, ref.CLAMP] and full.metres[0, 0, 7] == 1.0
    # the key orders negative heights, zeros of either sign and positive ones
    h = np.array([-2.0, -0.0, 0.0, 1e-30, 3.5, -1e-30], dtype=np.float32)
    k = ref.key_of(h)
    assert list(np.argsort(k, kind="stable")) == [0, 5, 1, 2, 3, 4] and all(ref.unkey(v) == w for v, w in zip(k, h))


# ---------------------------------------------------------------------------
# the union / find header as plain host C++, under the sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("uf") / "obstacles_uf_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "objcavit_amd", "csrc"), os.path.join(HERE, "obstacles_uf_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def _drive(exe, occ, link, tile):
    GY, GX = occ.shape
    text = f"{GX} {GY} {link} {tile}\n" + "\n".join(" ".join(str(int(v)) for v in row) for row in occ) + "\n"
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    return np.array(r.stdout.split(), dtype=np.int64).reshape(GY, GX)


@pytest.mark.parametrize("link", ref.LINKS)
@pytest.mark.parametrize("spec", ref.GRIDS, ids=lambda s: f"{s.GX}x{s.GY}")
def test_host_driver_reproduces_the_roots(driver, spec, link):
    """Every pattern, on the kernel's tile; the small grids also on a tile of 3, which gives them seams."""
    for name in ref.PATTERNS:
        occ, want = roots(name, spec, link)
        for tile in (ref.TILE,) + ((3,) if spec.GX * spec.GY <= 64 * 48 and name != "full" else ()):
            assert np.array_equal(_drive(driver, occ, link, tile), want), (name, tile)


# ---------------------------------------------------------------------------
# the library and the wrappers
# ---------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported(lib):
    from objcavit_amd import _lib, build, hip_ops, obstacles as ob
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_obstacles_fwd\s*\(", header) and re.search(r"\bsize_t\s+ocv_obstacles_workspace_bytes\s*\(", header)
    assert re.search(r"#define\s+OCV_ABI_VERSION\s+5\b", header) and "STATEMENT O" in header
    for name in ("ocv_obstacles_fwd", "ocv_obstacles_workspace_bytes", "ocv_obstacles_set_dispatch"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "obstacles.hip" in build.SOURCES and lib.ocv_abi_version() == 5
    assert re.search(r"#define\s+OCV_OBSTACLES_TILE\s+%d\b" % hip_ops.OBSTACLES_TILE, header) and hip_ops.OBSTACLES_TILE == ref.TILE
    assert hip_ops.OBSTACLES_WANT == ref.OUTPUTS and ob.CELL_FIELDS == ref.CELL_FIELDS and ob.METRE_FIELDS == ref.METRE_FIELDS
    # the segmented reduction, the float key and the union / find are stated once, in headers the kernels include
    csrc = os.path.join(ROOT, "objcavit_amd", "csrc")
    for name in ("ground_grid.hip", "obstacles.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "seg_reduce.hpp"' in text and '#include "float_key.hpp"' in text and "seg_reduce(" in text, name
        assert "unsigned gg_key" not in text and "__shfl_up(" not in text.split("seg_runs(")[0], name
    assert '#include "union_find.hpp"' in open(os.path.join(csrc, "obstacles.hip")).read()
    assert lib.ocv_obstacles_set_dispatch(2) == -1 and lib.ocv_obstacles_set_dispatch(0) == 0 and lib.ocv_obstacles_set_dispatch(1) == 0


def test_workspace_bytes(lib):
    assert lib.ocv_obstacles_workspace_bytes(1, 1, 1) == 64 + 4
    assert lib.ocv_obstacles_workspace_bytes(3, 33, 129) == 3 * 33 * 129 * 64 + 3 * 5 * 4
    assert lib.ocv_obstacles_workspace_bytes(16, 200, 400) == 16 * 200 * 400 * 64 + 16 * 79 * 4
    for B, GX, GY in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 1 << 16, 1 << 15), (1, (1 << 24) + 1, 1)):
        assert lib.ocv_obstacles_workspace_bytes(B, GX, GY) == 0


def _call(lib, **kw):
    """The entry point with made-up (never dereferenced) device addresses: every call here must be refused before any launch."""
    a = dict(state=64, count=64, obstacle=64, h_max=64, B=1, GX=4, GY=4, x0=-1.0, y0=0.0, cell=0.5, link=1, min_cells=1, min_obstacle=0,
             cap=8, cells=64, metres=None, labels=None, counts=None, total=None, ws=64, ws_bytes=1 << 20)
    a.update(kw)
    return lib.ocv_obstacles_fwd(a["state"], a["count"], a["obstacle"], a["h_max"], a["B"], a["GX"], a["GY"], a["x0"], a["y0"], a["cell"],
                                 a["link"], a["min_cells"], a["min_obstacle"], a["cap"], a["cells"], a["metres"], a["labels"], a["counts"],
                                 a["total"], a["ws"], a["ws_bytes"], None)


REFUSALS = [
    (dict(state=None), "null"), (dict(ws=None), "null"), (dict(cells=None), "no output"),
    (dict(link=0), "link"), (dict(link=4), "link"), (dict(link=-1), "link"),
    (dict(min_cells=0), "min_cells"), (dict(min_obstacle=-1), "min_obstacle_points"), (dict(cap=0), "cap"),
    (dict(B=0), "sizes"), (dict(GX=0), "sizes"), (dict(GY=-1), "sizes"),
    (dict(GX=1 << 16, GY=1 << 15, ws_bytes=1 << 62), "2^31"), (dict(B=1 << 12, GX=1 << 10, GY=1 << 9, ws_bytes=1 << 62), "2^31"),
    (dict(B=2, cap=1 << 27), "2^31"), (dict(GX=(1 << 24) + 1, GY=1, ws_bytes=1 << 62), "2^24"),
    (dict(cell=0.0), "cell"), (dict(cell=-0.1), "cell"), (dict(cell=NAN), "cell"), (dict(cell=INF), "cell"),
    (dict(x0=NAN), "origin"), (dict(y0=INF), "origin"),
    (dict(ws=68), "misaligned"), (dict(count=65), "misaligned"), (dict(obstacle=66), "misaligned"), (dict(h_max=67), "misaligned"),
    (dict(cells=70), "misaligned"), (dict(metres=65), "misaligned"), (dict(labels=66), "misaligned"), (dict(counts=67), "misaligned"),
    (dict(total=69), "misaligned"),
    (dict(ws_bytes=4 * 4 * 64 + 4 - 1), "workspace too small"), (dict(B=2, ws_bytes=4 * 4 * 64 + 4), "workspace too small"),
]


@pytest.mark.parametrize("kw,word", REFUSALS)
def test_bad_arguments_are_refused_before_any_launch(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_obstacles_fwd:") and word in msg, msg


def test_wrapper_refuses_host_tensors_and_has_the_documented_signature():
    from objcavit_amd import hip_ops
    from objcavit_amd._lib import HipLibraryError
    from objcavit_amd.ground_grid import GroundGrid
    from objcavit_amd.obstacles import Obstacles, obstacles
    state = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(HipLibraryError):
        hip_ops.obstacles(state, (-1.0, 0.0, 0.5, 4, 4))
    with pytest.raises(HipLibraryError):
        obstacles(GroundGrid(state=state, x0=-1.0, y0=0.0, cell=0.5))
    with pytest.raises(ValueError):
        obstacles(GroundGrid(count=state.int()))
    params = inspect.signature(hip_ops.obstacles).parameters
    assert list(params) == ["state", "spec", "count", "obstacle", "h_max", "link", "min_cells", "min_obstacle_points", "capacity", "want", "out",
                            "workspace", "image_index"]
    assert [params[n].default for n in ("link", "min_cells", "min_obstacle_points", "capacity", "want")] == [1, 1, 0, 64, ref.OUTPUTS]
    assert Obstacles._fields == ref.OUTPUTS + ("x0", "y0", "cell")
    o = Obstacles(cells=torch.tensor([[[1, 2, 3, 4, 5, 6, 7, 8], [0] * 8]], dtype=torch.int32), metres=torch.arange(16.0).view(1, 2, 8),
                  counts=torch.tensor([1], dtype=torch.int32))
    assert o.rows(0) == [dict(zip(ref.CELL_FIELDS + ref.METRE_FIELDS, [1, 2, 3, 4, 5, 6, 7, 8] + [float(v) for v in range(8)]))]
    with pytest.raises(ValueError):
        Obstacles(cells=o.cells).rows(0)


def test_predictors_validate_the_obstacles_keyword():
    from objcavit_amd import predict
    from objcavit_amd.config import make_args
    from objcavit_amd.predict import PipelinedPredictor, Predictor, PredictResult, _ObjectsResult
    args = make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip")
    pr = Predictor(None, args, ground_grid={}, obstacles={})
    assert pr.ends.obstacles == dict(link=1, min_cells=2, min_obstacle_points=0, capacity=64, labels=False)
    assert Predictor(None, args, ground_grid={}).ends.obstacles is None and Predictor(None, args).ends.obstacles is None
    o = Predictor(None, args, ground_grid={}, obstacles=dict(link=3, min_cells=5, min_obstacle_points=7, capacity=9, labels=True)).ends.obstacles
    assert o == dict(link=3, min_cells=5, min_obstacle_points=7, capacity=9, labels=True)
    with pytest.raises(ValueError, match="ground_grid"):
        Predictor(None, args, obstacles={})                                     # refused without the grid
    for bad in (dict(links=2), dict(link=0), dict(link=4), dict(link=1.5), dict(link=True), dict(min_cells=0), dict(min_obstacle_points=-1),
                dict(capacity=0), dict(capacity=2.5)):
        with pytest.raises(ValueError) as e:
            Predictor(None, args, ground_grid={}, obstacles=bad)
        if "links" in bad:
            assert "links" in str(e.value)                                     # an unknown key is named
    for fn in (Predictor.__init__, PipelinedPredictor.__init__):
        assert inspect.signature(fn).parameters["obstacles"].default is None
    # it runs behind the grid, is an attribute and no field, and its tensors are recorded for the caller's stream
    assert [r.keyword for r in predict.ALL_READOUTS][-2:] == ["ground_grid", "obstacles"]
    last = predict.ALL_READOUTS[-1]
    assert last.attr == "obstacles" and last.streamed == slice(5) and last.needs == ("K",) and last.maps(o) == ()
    assert PredictResult.obstacles is None and PredictResult._fields == ("depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence")
    res = _ObjectsResult(1, 2, 3, 4, 5, obstacles="list")
    assert res.obstacles == "list" and res.ground is None and tuple(res) == (1, 2, 3, 4, 5, None, None) and res._replace(depth=0).obstacles == "list"


class _Recorder:
    """Stand-ins for the three wrappers of a step with the grid and the list: they log what they were asked for."""

    def __init__(self, monkeypatch):
        from objcavit_amd import hip_ops
        self.calls = []
        monkeypatch.setattr(hip_ops, "depth_finalize", self.depth_finalize)
        monkeypatch.setattr(hip_ops, "ground_grid", self.ground_grid)
        monkeypatch.setattr(hip_ops, "obstacles", self.obstacles)

    def depth_finalize(self, pred, min_depth, max_depth, size, want=("depth",), **kw):
        return {n: torch.zeros((int(pred.shape[0]), 1) + tuple(size)) for n in want}

    def ground_grid(self, depth, K, pose, grid, want=(), out=None, image_index=0, **kw):
        self.calls.append(("ground_grid", tuple(want), tuple(sorted(out)), image_index))
        self.grid = out
        return out

    def obstacles(self, state, spec, count=None, obstacle=None, h_max=None, want=(), **kw):
        g = self.grid
        self.calls.append(("obstacles", tuple(want), spec, state is g["state"], count is g["count"], obstacle is g["obstacle"],
                           h_max is g["h_max"], kw))
        return {n: n for n in want}


def test_the_step_makes_the_grids_buffers_for_the_list_and_hands_out_only_what_was_asked(monkeypatch):
    from types import SimpleNamespace
    from objcavit_amd import predict
    from objcavit_amd.config import make_args
    args = make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip")
    rec = _Recorder(monkeypatch)
    frames = torch.zeros(2, 8, 12, 3, dtype=torch.uint8)
    out = SimpleNamespace(depth_pred=torch.ones(2, 1, 4, 6), bin_edges=torch.zeros(2, 9))
    K = torch.tensor([[10.0, 10.0, 6.0, 4.0]] * 2)

    def drive(**kw):
        del rec.calls[:]
        ends = predict._Ends(args, flip_tta=False, **kw)
        step = ends.step(ends.frames_of(frames, "frames_u8"), intrinsics=K)
        return ends.finish(out, None, step, 0, ("depth",))

    res = drive(ground_grid={"want": ("first_occupied", "h_mean")}, obstacles={"labels": True, "capacity": 5, "link": 2})
    made = ("obstacle", "count", "h_max", "h_mean", "state", "first_occupied")
    assert rec.calls[0] == ("ground_grid", tuple(n for n in predict.hip_ops.GROUND_GRID_WANT if n in made), tuple(sorted(made)), 0)
    name, want, spec, *same, kw = rec.calls[1]
    assert name == "obstacles" and want == ref.OUTPUTS and all(same) and spec == (-10.0, 0.0, 0.1, 200, 400)
    assert kw == dict(link=2, min_cells=2, min_obstacle_points=0, capacity=5)
    g = res.ground
    assert g.first_occupied is not None and g.h_mean is not None and g.state is None and g.count is None and g.obstacle is None and g.h_max is None
    assert res.obstacles.cells == "cells" and res.obstacles.labels == "labels" and (res.obstacles.x0, res.obstacles.cell) == (-10.0, 0.1)
    # without ``labels`` the label map is not made; with the grid's default ``want`` nothing is added
    res = drive(ground_grid={}, obstacles={})
    assert rec.calls[0][1] == predict.hip_ops.GROUND_GRID_WANT and rec.calls[1][1] == ref.OUTPUTS[:4] and res.obstacles.labels is None
    assert res.ground.state is not None
    # without the keyword the grid is asked for what it was asked for before, and there is no list
    res = drive(ground_grid={"want": ("first_occupied",)})
    assert rec.calls == [("ground_grid", ("first_occupied",), ("first_occupied",), 0)] and res.obstacles is None
    # without intrinsics neither runs
    ends = predict._Ends(args, flip_tta=False, ground_grid={}, obstacles={})
    del rec.calls[:]
    res = ends.finish(out, None, ends.step(ends.frames_of(frames, "frames_u8")), 0, ("depth",))
    assert not rec.calls and type(res) is predict.PredictResult
