"""-m gpu: csrc/obstacles.hip against Statement O in numpy (tests/obstacles_ref.py) -- EQUAL, not close: every table bit for bit -- on
every pattern that can break a union-find across tiles, with the filters, capacities, output subsets and null inputs, between poisoned
guards, inside a captured graph, and (in a child process) through the predict path that carries it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import obstacles_ref as ref
import test_hip_memory_bounds as bounds
from test_obstacles_host import REFUSALS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
POISON = 0x7FC0DEAD                       # a NaN payload no computation produces
ALL = ref.OUTPUTS
B = 3
# B = 3 with a different pattern per image: every pattern is in one triple
TRIPLES = (("empty", "full", "corners"), ("serpentine", "comb", "diagonal"), ("gaps", "isolated", "bernoulli30"),
           ("bernoulli41", "bernoulli60", "gaps"))


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


_CASES = {}


def case(spec, link, triple, big=False):
    """(state, count, obstacle, h_max) numpy [3, GY, GX] of a triple of patterns, made once."""
    key = (spec, link, triple, big)
    if key not in _CASES:
        occ = np.stack([ref.pattern(name, spec.GX, spec.GY, link, seed=i) for i, name in enumerate(triple)], 0)
        _CASES[key] = ref.grid_inputs(occ, seed=10 * TRIPLES.index(triple) + link, big=big)
    return _CASES[key]


_WANT = {}


def reference(spec, link, triple, big=False, nulls=(), **kw):
    """The statement on a case, made once per (case, options) and left unchanged."""
    key = (spec, link, triple, big, tuple(nulls), tuple(sorted(kw.items())))
    if key not in _WANT:
        state, count, obstacle, h_max = case(spec, link, triple, big)
        given = {n: (None if n in nulls else v) for n, v in (("count", count), ("obstacle", obstacle), ("h_max", h_max))}
        _WANT[key] = ref.obstacles(state, spec, link=link, **given, **kw)
    return _WANT[key]


def poisoned(n, spec, cap, names=ALL, byte=0xAB):
    shapes = {"cells": (n, cap, 8), "metres": (n, cap, 8), "counts": (n,), "total": (n,), "labels": (n, spec.GY, spec.GX)}
    out = {name: torch.full(shapes[name], POISON ^ byte, dtype=torch.int32, device="cuda") for name in names}
    if "metres" in out:
        out["metres"] = out["metres"].view(torch.float32)
    return out


def check(got, want, what=""):
    """``got``: the wrapper's dict (any subset of the outputs) against the reference's Result: EQUAL, the floats by their bits."""
    for name, t in got.items():
        g, w = t.cpu(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, tuple(g.shape))
        bad = g.view(torch.int32) != w.view(torch.int32)
        assert not bool(bad.any()), (what, name, int(bad.sum()), "elements differ", bad.nonzero()[:4].tolist())


def run(ops, spec, arrays, link, names=ALL, out=None, nulls=(), **kw):
    state, count, obstacle, h_max = (torch.from_numpy(a).cuda() for a in arrays)
    given = {n: (None if n in nulls else v) for n, v in (("count", count), ("obstacle", obstacle), ("h_max", h_max))}
    return ops.obstacles(state, tuple(spec), link=link, want=names, out=out, **given, **kw)


# ---------------------------------------------------------------------------
# equality with the statement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("link", ref.LINKS)
@pytest.mark.parametrize("spec", ref.GRIDS, ids=lambda s: f"{s.GX}x{s.GY}")
def test_outputs_equal_the_statement(ops, spec, link):
    """Every pattern, three to a batch, into poisoned buffers of 64 rows: the isolated cells and the Bernoulli fields of the larger grids
    have more components than rows (total > counts, labels -2), the others fewer (zero tail).  A second call over another poison gives
    the same bytes: every element is written, and nothing depends on the order of arrival."""
    cap = 64
    seen = set()
    for triple in TRIPLES:
        arrays = case(spec, link, triple)
        want = reference(spec, link, triple, cap=cap)
        out = poisoned(B, spec, cap)
        got = run(ops, spec, arrays, link, out=out, capacity=cap)
        assert all(got[k] is out[k] for k in ALL)
        check(got, want, (spec, link, triple))
        again = run(ops, spec, arrays, link, out=poisoned(B, spec, cap, byte=0x54), capacity=cap)
        for k in ALL:
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (spec, link, triple, k)
        seen.update(int(v) for v in want.total)
    assert 0 in seen and (max(seen) > 1 or spec.GX * spec.GY < 4)
    if spec.GX * spec.GY > 64 * 4:
        assert max(seen) > cap


def test_serpentine_over_the_default_grid(ops):
    """B = 1, 200 x 400, one component that winds through all 91 tiles: the longest parent chains across every seam."""
    spec = ref.Spec(-10.0, 0.0, 0.1, 200, 400)
    occ = ref.pattern("serpentine", spec.GX, spec.GY)[None]
    arrays = ref.grid_inputs(occ, seed=1)
    want = ref.obstacles(arrays[0], spec, *arrays[1:], link=1, cap=4)
    assert want.total.tolist() == [1] and int(want.cells[0, 0, 4]) == int(occ.sum()) > 40000
    check(run(ops, spec, arrays, 1, out=poisoned(1, spec, 4), capacity=4), want, "serpentine")


def test_sums_beyond_int32_are_clamped(ops):
    spec = ref.GRIDS[4]
    want = reference(spec, 1, TRIPLES[0], big=True, cap=8)
    assert int(want.cells[1, 0, 5]) == ref.CLAMP and int(want.cells[1, 0, 6]) == ref.CLAMP and int(want.cells[2, 0, 5]) == 2 ** 30
    check(run(ops, spec, case(spec, 1, TRIPLES[0], big=True), 1, out=poisoned(B, spec, 8), capacity=8), want, "clamp")


# ---------------------------------------------------------------------------
# options
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("link", (1, 3))
def test_filters(ops, link):
    spec, triple = ref.GRIDS[2], TRIPLES[2]
    arrays = case(spec, link, triple)
    plain = reference(spec, link, triple, cap=64)
    for kw in (dict(min_cells=2), dict(min_cells=5), dict(min_obstacle_points=30), dict(min_cells=3, min_obstacle_points=60)):
        want = reference(spec, link, triple, cap=64, **kw)
        assert not torch.equal(want.total, plain.total), kw                     # the option matters on this case
        check(run(ops, spec, arrays, link, out=poisoned(B, spec, 64), capacity=64, **kw), want, (link, kw))


def test_capacity_below_equal_and_above_the_number_kept(ops):
    spec, link, triple = ref.GRIDS[3], 2, TRIPLES[0]
    arrays = case(spec, link, triple)
    kept = int(reference(spec, link, triple, cap=64).total.max())
    assert 2 <= kept < 64
    for cap in (1, kept - 1, kept, kept + 1, 3 * kept):
        want = reference(spec, link, triple, cap=cap)
        got = run(ops, spec, arrays, link, out=poisoned(B, spec, cap), capacity=cap)
        check(got, want, cap)
        t, c = got["total"].cpu(), got["counts"].cpu()
        assert int(t.max()) == kept and torch.equal(c, t.clamp(max=cap))
        for b in range(B):
            assert not got["cells"][b, int(c[b]):].any() and not got["metres"][b, int(c[b]):].any()
        if cap < kept:
            assert bool((got["labels"] == -2).any()) and int(got["labels"].max()) == cap - 1


@pytest.mark.parametrize("names", [("cells",), ("metres",), ("labels",), ("counts",), ("total", "metres"), ("labels", "cells", "counts")],
                         ids=lambda v: "+".join(v))
def test_subsets_of_the_outputs(ops, names):
    spec, link, triple = ref.GRIDS[4], 1, TRIPLES[2]
    arrays = case(spec, link, triple)
    want = reference(spec, link, triple, cap=32)
    got = run(ops, spec, arrays, link, names=names, out=poisoned(B, spec, 32, names), capacity=32)
    assert set(got) == set(names)
    check(got, want, names)


@pytest.mark.parametrize("nulls", [("count",), ("obstacle",), ("h_max",), ("count", "obstacle", "h_max")], ids=lambda v: "+".join(v))
def test_null_inputs_give_zero_columns(ops, nulls):
    spec, link, triple = ref.GRIDS[3], 1, TRIPLES[3]
    want = reference(spec, link, triple, nulls=nulls, cap=64)
    got = run(ops, spec, case(spec, link, triple), link, out=poisoned(B, spec, 64), nulls=nulls, capacity=64)
    check(got, want, nulls)
    for n, col, table in (("count", 5, "cells"), ("obstacle", 6, "cells"), ("h_max", 6, "metres")):
        assert bool(got[table][:, :, col].any()) == (n not in nulls), n


def test_without_the_on_chip_merge_the_bytes_are_the_same(ops):
    spec, link, triple = ref.GRIDS[4], 2, TRIPLES[0]
    arrays = case(spec, link, triple)
    want = reference(spec, link, triple, cap=16)
    ops.obstacles_set_dispatch(False)
    try:
        got = run(ops, spec, arrays, link, out=poisoned(B, spec, 16), capacity=16)
    finally:
        ops.obstacles_set_dispatch(True)
    check(got, want, "no merge")


def test_image_index_fills_a_batch_and_the_workspace_may_be_the_callers(ops):
    from objcavit_amd import _lib
    spec, link, triple = ref.GRIDS[3], 1, TRIPLES[1]
    arrays = case(spec, link, triple)
    state, count, obstacle, h_max = (torch.from_numpy(a).cuda() for a in arrays)
    kw = dict(link=link, capacity=16)
    a = ops.obstacles(state, tuple(spec), count=count, obstacle=obstacle, h_max=h_max, out=poisoned(B, spec, 16), **kw)
    check(a, reference(spec, link, triple, cap=16), "whole batch")
    pick = [2, 0, 1]
    out = poisoned(B, spec, 16)
    need = int(_lib.load().ocv_obstacles_workspace_bytes(1, spec.GX, spec.GY))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for slot, i in enumerate(pick):
        got = ops.obstacles(state[i:i + 1], tuple(spec), count=count[i:i + 1], obstacle=obstacle[i:i + 1], h_max=h_max[i:i + 1], out=out,
                            image_index=slot, workspace=ws, **kw)
        assert got["cells"] is out["cells"]
    for n in ALL:
        assert torch.equal(out[n].view(torch.int32), a[n][pick].contiguous().view(torch.int32)), n
    with pytest.raises(ValueError):
        ops.obstacles(state[:1], tuple(spec), out=out, image_index=3, **kw)
    with pytest.raises(ValueError):
        ops.obstacles(state, tuple(spec), out={"cells": out["cells"]}, **kw)
    with pytest.raises(_lib.HipLibraryError):
        ops.obstacles(state, tuple(spec), workspace=ws[:need - 8], **kw)             # too small for three images: refused, no launch
    fresh = ops.obstacles(state, tuple(spec), count=count, obstacle=obstacle, h_max=h_max, **kw)
    for n in ALL:
        assert torch.equal(fresh[n].view(torch.int32), a[n].view(torch.int32)), n


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_bad_options_are_refused(ops):
    spec = ref.GRIDS[1]
    state = torch.zeros(1, spec.GY, spec.GX, dtype=torch.uint8, device="cuda")
    for kw in (dict(want=()), dict(want=("cells", "state")), dict(link=0), dict(link=4), dict(link=1.5), dict(min_cells=0),
               dict(min_obstacle_points=-1), dict(capacity=0), dict(capacity=1 << 28), dict(count=state.int()[:, :2].contiguous()),
               dict(h_max=state.float()[:, :, :3].contiguous())):
        with pytest.raises(ValueError):
            ops.obstacles(state, tuple(spec), **kw)
    for bad in ((0.0, 0.0, 0.0, 7, 5), (0.0, 0.0, 1.0, 5, 7), (0.0, 0.0, 1.0, 7), (float("nan"), 0.0, 1.0, 7, 5), (0.0, float("inf"), 1.0, 7, 5)):
        with pytest.raises(ValueError):
            ops.obstacles(state, bad)
    with pytest.raises(TypeError):
        ops.obstacles(state.int(), tuple(spec))
    with pytest.raises(TypeError):
        ops.obstacles(state, tuple(spec), count=state.float())


@pytest.mark.parametrize("kw,word", REFUSALS)
def test_entry_point_refuses_before_any_launch(kw, word):
    """The entry point on real device buffers, every refusal of the list tests/test_obstacles_host.py runs without a GPU: -1, the
    message, and no byte of the outputs or of the workspace touched."""
    from objcavit_amd import _lib
    lib = _lib.load()
    GX = GY = 4
    state = torch.full((1, GY, GX), 2, dtype=torch.uint8, device="cuda")
    grid = [torch.ones((1, GY, GX), dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.ones((1, GY, GX), device="cuda")]
    cells = torch.full((1, 8, 8), POISON, dtype=torch.int32, device="cuda")
    ws = torch.full((1 << 18,), POISON, dtype=torch.int32, device="cuda")
    a = dict(state=state.data_ptr(), count=grid[0].data_ptr(), obstacle=grid[1].data_ptr(), h_max=grid[2].data_ptr(), B=1, GX=GX, GY=GY,
             x0=-1.0, y0=0.0, cell=0.5, link=1, min_cells=1, min_obstacle=0, cap=8, cells=cells.data_ptr(), metres=None, labels=None,
             counts=None, total=None, ws=ws.data_ptr(), ws_bytes=1 << 20)
    a.update(kw)
    rc = lib.ocv_obstacles_fwd(a["state"], a["count"], a["obstacle"], a["h_max"], a["B"], a["GX"], a["GY"], a["x0"], a["y0"], a["cell"],
                               a["link"], a["min_cells"], a["min_obstacle"], a["cap"], a["cells"], a["metres"], a["labels"], a["counts"],
                               a["total"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    msg = lib.ocv_last_error().decode()
    assert rc == -1 and msg.startswith("ocv_obstacles_fwd:") and word in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((cells == POISON).all()) and bool((ws == POISON).all())


# ---------------------------------------------------------------------------
# guarded memory: a row of tests/test_hip_memory_bounds.py's table (its accounting test wants every *_fwd entry point in a row)
# ---------------------------------------------------------------------------
ROW = "obstacles|33x129"


def _obstacles_row(c):
    """(33, 129) -- two tiles by five, both ragged; five chunks, the last ragged --, B = 3, link 3; once with every output, once with
    ``cells`` alone.  Every element of every output and of the workspace is written (``c.out``)."""
    spec, link, triple = ref.GRIDS[3], 3, TRIPLES[2]
    arrays = case(spec, link, triple)
    want = reference(spec, link, triple, cap=16)
    state, count, obstacle, h_max = (c.put(torch.from_numpy(a)) for a in arrays)
    need = int(c.lib.ocv_obstacles_workspace_bytes(B, spec.GX, spec.GY))
    for names in (ALL, ("cells",)):
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        got = c.ops.obstacles(state, tuple(spec), count=count, obstacle=obstacle, h_max=h_max, link=link, capacity=16, want=names, workspace=ws)
        check(got, want, ("guarded", names))
        c.out(ws, *got.values())


if ROW not in bounds.ROWS:
    bounds.row(ROW)(_obstacles_row)


def test_launches_between_poisoned_guards():
    bounds.run_row(ROW)
    assert "ocv_obstacles_fwd" in bounds.RAN[ROW]


def test_captured_graph_replays_with_a_new_map_and_pose():
    """In a fresh child process (tests/obstacles_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "obstacles_graph_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


def test_predict_path_carries_the_list():
    """``Predictor`` and ``PipelinedPredictor`` with the keyword, in a fresh child process (tests/obstacles_predict_child.py, which says
    what it checks) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "obstacles_predict_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
