"""-m "not gpu": the ground grid's host side -- Statement G's reference (tests/ground_grid_ref.py) on flat ground, its fp32 evaluation
against float64 (a condition on the test inputs), the planted errors the cases must tell apart, the new symbols and their argument
checks (no launch happens), the wrappers, ``ground_pose`` and the predictors' ``ground_grid`` keyword."""
import math
import os
import re

import pytest
import torch

import ground_grid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------
# the reference and its cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.CASE_SHAPES + ((60, 80),), ids=lambda s: f"{s[0]}x{s[1]}")
def test_flat_ground_is_recovered_at_height_zero(shape):
    """Flat ground made analytically in float64, rounded to an fp32 map: the fp32 statement puts every kept point within
    8 * 2^-23 * (|t_2| + sum_i |p[2][i] P_i|) of height 0 -- fp32's rounding of the four terms, evaluated per pixel in float64."""
    H, W = shape
    K = ref.intrinsics(H, W)
    P = ref.pose_matrix()
    pose = P.reshape(1, 12).float().expand(ref.CASE_B, 12).contiguous()
    depth = torch.stack([ref.flat_ground(H, W, K[b], P).float() for b in range(ref.CASE_B)], 0).unsqueeze(1)
    kept = ref.keep(depth, K, pose)
    assert int(kept.sum()) > H * W // 4                                        # (the sky is +inf: not kept)
    g2 = ref.ground_points(depth, K, pose)[2]
    p64 = pose.double().view(ref.CASE_B, 3, 4)
    for b in range(ref.CASE_B):
        r = ref.rays(H, W, K[b])
        pts = r * depth[b, 0].double()                                         # X, Y, Z of every pixel in float64
        bound = 8.0 * 2.0 ** -23 * (p64[b, 2, 3].abs() + (p64[b, 2, :3].view(3, 1, 1) * pts).abs().sum(0))
        m = kept[b]
        assert bool((g2[b][m].double().abs() <= bound[m]).all()), (shape, b, float((g2[b][m].double().abs() / bound[m]).max()))


@pytest.mark.parametrize("shape", ref.CASE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fp32_statement_against_float64(shape):
    """The share of kept points whose cell or band membership differs between the fp32 statement and float64 is at most 1e-3 on every
    case: a condition on the inputs, not on the kernel."""
    H, W = shape
    for bad in (None, 0):
        c = ref.case(H, W, bad=bad)
        for spec in ref.GRIDS:
            differ, kept = ref.membership_gap(c.depth, c.K, c.pose, spec, c.options["band"])
            print(shape, bad, spec, differ, kept)
            assert kept > 0 and differ <= 1e-3 * kept, (shape, spec, differ, kept)


def test_fp32_statement_against_float64_at_full_size():
    c = ref.case(480, 640)
    for spec in ref.GRIDS[1:4]:
        differ, kept = ref.membership_gap(c.depth, c.K, c.pose, spec, c.options["band"])
        print(spec, differ, kept)
        assert kept > 500000 and differ <= 1e-3 * kept, (spec, differ, kept)


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_each_planted_error_changes_the_cells_of_some_case(mutation):
    """Each deliberate error changes (count, obstacle or state of) at least 1 % of the non-empty cells of some case."""
    best = 0.0
    for H, W in ref.CASE_SHAPES:
        c = ref.case(H, W)
        for spec in ref.GRIDS:
            good = ref.ground_grid(c.depth, c.K, c.pose, spec, **c.options)
            wrong = ref.ground_grid(c.depth, c.K, c.pose, spec, mutation=mutation, **c.options)
            changed, filled = ref.changed_cells(good, wrong)
            if filled:
                best = max(best, changed / filled)
    print(mutation, best)
    assert best >= 0.01, (mutation, best)


def test_cases_have_what_the_gpu_test_needs():
    for H, W in ref.CASE_SHAPES:
        c = ref.case(H, W)
        assert c.depth.dtype == torch.float32 and tuple(c.depth.shape) == (3, 1, H, W) and tuple(c.pose.shape) == (3, 12)
        lo, hi = c.options["band"]
        assert lo < c.options["obstacle_height"] < hi
        g0, g1, g2 = ref.ground_points(c.depth, c.K, c.pose)
        # the planted thresholds: a wall point exactly on the band's upper edge and one exactly at the obstacle height
        assert bool((g2[2] == hi).any()) and bool((g2[2] == c.options["obstacle_height"]).any())
        for bad in range(3):
            for kind in ("camera", "pose"):
                cb = ref.case(H, W, bad=bad, kind=kind)
                kept = ref.keep(cb.depth, cb.K, cb.pose).flatten(1).sum(1)
                assert [int(v) > 0 for v in kept] == [i != bad for i in range(3)], (H, W, bad, kind)
    c = ref.case(37, 131)
    assert torch.isnan(c.depth[1]).any() and torch.isinf(c.depth[1]).any()
    kept = ref.keep(c.depth, c.K, c.pose)
    g0, g1, g2 = ref.ground_points(c.depth, c.K, c.pose)
    spec = ref.GRIDS[1]
    # points fall off every side of the (7, 5, 1.0) grid, and g_0 - x0 is negative for some of them
    assert bool((g0[kept] < spec.x0).any()) and bool((g0[kept] >= spec.x0 + spec.GX * spec.cell).any())
    assert bool((g1[kept] < spec.y0).any()) and bool((g1[kept] >= spec.y0 + spec.GY * spec.cell).any())
    grid = ref.ground_grid(c.depth, c.K, c.pose, ref.GRIDS[2], **c.options)
    assert bool((grid.state == 0).any()) and bool((grid.state == 1).any()) and bool((grid.state == 2).any())
    assert bool(torch.isinf(grid.first_occupied).any()) and bool(torch.isfinite(grid.first_occupied).any())
    # the one-cell grid takes every point of the band: the 64-bit sum's case
    one = ref.ground_grid(c.depth, c.K, c.pose, ref.GRIDS[0], **c.options)
    assert int(one.count[2, 0, 0]) > 4000 and float(one.h_min[2, 0, 0]) < float(one.h_mean[2, 0, 0]) < float(one.h_max[2, 0, 0])


def test_reference_counts_a_hand_made_scene():
    """Identity-like pose, four pixels: cells, band edges (inclusive), obstacle threshold (exclusive), floor of a negative coordinate."""
    K = torch.tensor([[1.0, 1.0, 0.0, 0.0]])
    pose = torch.tensor([[1.0, 0, 0, 0, 0, 0, 1.0, 0, 0, -1.0, 0, 1.0]])                 # g = (X, Z, 1 - Y)
    depth = torch.tensor([[2.0, 2.0], [0.5, 2.0]]).view(1, 1, 2, 2)                       # points (0, 0, 2) (2, 0, 2) (0, .5, .5) (2, 2, 2)
    spec = ref.Spec(-0.5, 0.0, 1.0, 3, 3)
    g = ref.ground_grid(depth, K, pose, spec, band=(-1.0, 1.0), obstacle_height=0.5, near=0.1, far=10.0)
    want = torch.zeros(3, 3, dtype=torch.int32)
    want[2, 0], want[2, 2], want[0, 0] = 1, 2, 1                                         # heights 1, (1, -1), 0.5
    assert torch.equal(g.count[0], want)
    assert int(g.obstacle[0, 2, 0]) == 1 and int(g.obstacle[0, 2, 2]) == 1 and int(g.obstacle[0, 0, 0]) == 0      # 0.5 > 0.5 is false
    assert float(g.h_min[0, 2, 2]) == -1.0 and float(g.h_max[0, 2, 2]) == 1.0 and float(g.h_mean[0, 2, 2]) == 0.0
    assert g.state[0].tolist() == [[1, 0, 0], [0, 0, 0], [2, 0, 2]]
    assert g.first_occupied[0].tolist() == [2.0, INF, 2.0]
    moved = ref.ground_grid(depth, K, pose, ref.Spec(0.5, 0.0, 1.0, 3, 3), band=(-1.0, 1.0), near=0.1, far=10.0)
    assert int(moved.count.sum()) == 2                                                   # x = 0 is left of the grid: floor(-0.5) = -1


# ---------------------------------------------------------------------------
# the library and the wrappers
# ---------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported(lib):
    from objcavit_amd import _lib, build, hip_ops
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_ground_grid_fwd\s*\(", header) and re.search(r"\bsize_t\s+ocv_ground_grid_workspace_bytes\s*\(", header)
    assert re.search(r"#define\s+OCV_ABI_VERSION\s+5\b", header) and "STATEMENT G" in header
    for name in ("ocv_ground_grid_fwd", "ocv_ground_grid_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "ground_grid.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "objcavit_amd", "csrc", "keep_pixel.hpp"))
    assert lib.ocv_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert callable(hip_ops.ground_grid) and hip_ops.GROUND_GRID_WANT == ref.OUTPUTS
    assert re.search(r"#define\s+OCV_GROUND_GRID_TILE\s+%d\b" % hip_ops.GROUND_GRID_TILE, header)
    # the keep rule is stated once, in the header both kernels include
    for name in ("point_cloud.hip", "ground_grid.hip"):
        text = open(os.path.join(ROOT, "objcavit_amd", "csrc", name)).read()
        assert '#include "keep_pixel.hpp"' in text and "up_keep(" in text and "up_camera_ok(" in text, name
        assert "bool up_finite" not in text, name


def test_workspace_bytes(lib):
    assert lib.ocv_ground_grid_workspace_bytes(1, 1, 1) == 24
    assert lib.ocv_ground_grid_workspace_bytes(16, 200, 400) == 16 * 200 * 400 * 24
    for B, GX, GY in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 1 << 16, 1 << 16), (1, (1 << 24) + 1, 1)):
        assert lib.ocv_ground_grid_workspace_bytes(B, GX, GY) == 0


def _call(lib, **kw):
    """The entry point with made-up (never dereferenced) device addresses: every call here must be refused before any launch."""
    a = dict(depth=64, K=64, pose=64, conf=None, std=None, B=1, H=8, W=8, sy=1, sx=1, near=0.0, far=10.0, min_conf=0.0, max_std=INF,
             x0=-1.0, y0=0.0, cell=0.5, GX=4, GY=4, lo=-0.5, hi=2.5, oh=0.3, min_points=1, min_obstacle=1, count=64, obstacle=None,
             h_min=None, h_max=None, h_mean=None, state=None, first=None, ws=64, ws_bytes=1 << 20)
    a.update(kw)
    return lib.ocv_ground_grid_fwd(a["depth"], a["K"], a["pose"], a["conf"], a["std"], a["B"], a["H"], a["W"], a["sy"], a["sx"], a["near"],
                                   a["far"], a["min_conf"], a["max_std"], a["x0"], a["y0"], a["cell"], a["GX"], a["GY"], a["lo"], a["hi"],
                                   a["oh"], a["min_points"], a["min_obstacle"], a["count"], a["obstacle"], a["h_min"], a["h_max"],
                                   a["h_mean"], a["state"], a["first"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("kw,word", [
    (dict(depth=None), "null"), (dict(K=None), "null"), (dict(pose=None), "null"), (dict(ws=None), "null"),
    (dict(count=None), "no output"),
    (dict(B=0), "sizes"), (dict(H=0), "sizes"), (dict(W=-3), "sizes"), (dict(GX=0), "sizes"), (dict(GY=-1), "sizes"),
    (dict(H=1 << 16, W=1 << 16), "2^31"), (dict(GX=1 << 16, GY=1 << 16, ws_bytes=1 << 62), "2^31"), (dict(B=1 << 12, GX=1 << 10, GY=1 << 10), "2^31"),
    (dict(B=1 << 22, H=1 << 10, W=1 << 11, GX=1, GY=1), "2^31"),                       # B * tiles = 2^22 * 2^11 / 2^10 ... = 2^33
    (dict(GX=(1 << 24) + 1, GY=1), "2^24"),
    (dict(sy=0), "stride"), (dict(sx=-2), "stride"),
    (dict(near=2.0, far=1.0), "near"), (dict(near=NAN), "near"), (dict(far=NAN), "near"),
    (dict(lo=1.0, hi=0.5), "band"), (dict(lo=NAN), "band"), (dict(hi=NAN), "band"), (dict(lo=-1000.5), "band"), (dict(hi=1001.0), "band"),
    (dict(hi=INF), "band"),
    (dict(cell=0.0), "cell"), (dict(cell=-0.1), "cell"), (dict(cell=NAN), "cell"), (dict(cell=INF), "cell"),
    (dict(x0=NAN), "origin"), (dict(y0=INF), "origin"), (dict(oh=NAN), "obstacle_height"),
    (dict(min_points=0), "min_points"), (dict(min_obstacle=0), "min_points"), (dict(min_obstacle=-4), "min_obstacle_points"),
    (dict(K=72), "16-byte"), (dict(pose=68), "16-byte"), (dict(depth=66), "misaligned"), (dict(count=65), "misaligned"),
    (dict(first=70), "misaligned"), (dict(ws=68), "misaligned"), (dict(conf=33), "misaligned"),
    (dict(ws_bytes=4 * 4 * 24 - 1), "workspace too small"), (dict(B=2, ws_bytes=4 * 4 * 24), "workspace too small"),
])
def test_bad_arguments_are_refused_before_any_launch(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_ground_grid_fwd:") and word in msg, msg


def test_wrapper_refuses_host_tensors_and_bad_options():
    import inspect
    from objcavit_amd import hip_ops
    from objcavit_amd._lib import HipLibraryError
    from objcavit_amd.ground_grid import ground_grid, ground_pose
    d, k, p = torch.ones(1, 1, 8, 8), torch.ones(1, 4), ground_pose(1.65)
    with pytest.raises(HipLibraryError):
        hip_ops.ground_grid(d, k, p, (-1.0, 0.0, 0.5, 4, 4))
    with pytest.raises(HipLibraryError):
        ground_grid(d, k, p)
    params = inspect.signature(hip_ops.ground_grid).parameters
    assert list(params) == ["depth", "K", "pose", "grid", "band", "obstacle_height", "min_points", "min_obstacle_points", "stride", "near", "far",
                            "confidence", "min_confidence", "depth_std", "max_std", "want", "out", "workspace", "image_index"]
    assert params["band"].default == (-0.5, 2.5) and params["obstacle_height"].default == 0.3
    assert params["min_points"].default == 1 and params["min_obstacle_points"].default == 3 and params["want"].default == ref.OUTPUTS


def test_ground_pose_equals_the_float64_matrices():
    from objcavit_amd.ground_grid import ground_pose
    for h, p, r in ((1.65, 0.0, 0.0), (ref.HEIGHT, ref.PITCH, ref.ROLL), (0.4, -0.3, 1.1), (2.0, math.pi / 2, 0.0)):
        got = ground_pose(h, p, r)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 12)
        assert torch.equal(got[0], ref.pose_matrix(h, p, r).reshape(12).float()), (h, p, r)
    level = ground_pose(1.65).view(3, 4)
    assert torch.equal(level, torch.tensor([[1.0, 0, 0, 0], [0, 0, 1.0, 0], [0, -1.0, 0, 1.65]]))
    # pitch > 0 tilts the optical axis down: a point straight ahead on the axis lies below the camera
    down = ground_pose(1.0, 0.2).view(3, 4)
    assert float(down[2, 2]) < 0 and abs(float(down[2, 2]) + math.sin(0.2)) < 1e-7 and abs(float(down[1, 2]) - math.cos(0.2)) < 1e-7
    many = ground_pose([1.0, 1.5, 2.0], 0.1, [0.0, 0.01, -0.02])
    assert tuple(many.shape) == (3, 12) and torch.equal(many[1], ground_pose(1.5, 0.1, 0.01)[0])
    with pytest.raises(ValueError):
        ground_pose([1.0, 2.0], [0.1, 0.2, 0.3])


def test_module_and_result_type():
    from objcavit_amd import ground_grid as gg
    from objcavit_amd.predict import PredictResult, _ObjectsResult
    assert gg.GroundGrid._fields == ref.OUTPUTS + ("x0", "y0", "cell")
    g = gg.GroundGrid(count=torch.zeros(2, 4, 3), x0=-1.0, y0=2.0, cell=0.5)
    assert g.x_centres().tolist() == [-0.75, -0.25, 0.25] and g.y_centres().tolist() == [2.25, 2.75, 3.25, 3.75]
    assert gg.grid_of() == (-10.0, 0.0, 0.1, 200, 400) and gg.grid_of(0.25, (-8, 8), (1, 13)) == (-8.0, 1.0, 0.25, 64, 48)
    for bad in (dict(cell=0.0), dict(cell=NAN), dict(x_range=(1, 1)), dict(y_range=(0, INF))):
        with pytest.raises(ValueError):
            gg.grid_of(**bad)
    assert PredictResult.ground is None
    res = _ObjectsResult(1, 2, 3, 4, 5, ground=g)
    assert res.ground is g and res.normals is None and tuple(res) == (1, 2, 3, 4, 5, None, None)
    assert res._replace(bin_edges=None).ground is g


def test_predictors_validate_the_ground_grid_keyword():
    import inspect
    from objcavit_amd.config import make_args
    from objcavit_amd.ground_grid import ground_pose
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    args = make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip")
    ds = args[args.basic.dataset]
    pr = Predictor(None, args, ground_grid={})
    o = pr.ends.ground
    assert o["grid"] == (-10.0, 0.0, 0.1, 200, 400) and o["band"] == (-0.5, 2.5) and o["obstacle_height"] == 0.3
    assert o["min_points"] == 1 and o["min_obstacle_points"] == 3 and o["stride"] == (1, 1) and o["want"] == ref.OUTPUTS
    assert o["near"] == float(ds.min_depth) and o["far"] == float(ds.max_depth) and o["min_confidence"] == 0.0 and o["max_std"] == INF
    assert torch.equal(o["pose"], ground_pose(1.65))
    assert Predictor(None, args).ends.ground is None and pr.ends.cloud is None and pr.ends.normals is None
    o = Predictor(None, args, ground_grid=dict(cell=0.25, x_range=(-8, 8), y_range=(1, 13), height=1.2, pitch=0.05, roll=-0.01, band=(-1, 3),
                                               obstacle_height=0.5, min_points=2, min_obstacle_points=4, stride=(2, 3), near=0.3, far=9.0,
                                               min_confidence=0.4, max_std=0.7, want=("state", "count"))).ends.ground
    assert o["grid"] == (-8.0, 1.0, 0.25, 64, 48) and o["band"] == (-1.0, 3.0) and o["stride"] == (2, 3) and o["want"] == ("count", "state")
    assert torch.equal(o["pose"], ground_pose(1.2, 0.05, -0.01)) and (o["min_points"], o["min_obstacle_points"]) == (2, 4)
    for bad in (dict(cells=3), dict(cell=0.0), dict(cell=-1.0), dict(x_range=(2, 1)), dict(band=(1.0, 0.0)), dict(band=(0.0, 2000.0)),
                dict(min_points=0), dict(min_obstacle_points=1.5), dict(stride=(0, 1)), dict(near=3.0, far=1.0), dict(want=()),
                dict(want=("depth",)), dict(height=NAN), dict(obstacle_height=NAN)):
        with pytest.raises(ValueError) as e:
            Predictor(None, args, ground_grid=bad)
        if "cells" in bad:
            assert "cells" in str(e.value)                                     # an unknown key is named
    # intrinsics and poses are taken with the keyword, and only with it
    K = torch.tensor([[500.0, 500.0, 10.0, 10.0]])
    cpu = torch.device("cpu")
    assert pr.ends.intrinsics_on(K, cpu, 1) is not None and Predictor(None, args).ends.intrinsics_on(K, cpu, 1) is None
    pose = ground_pose(1.5, 0.1)
    assert torch.equal(pr.ends.pose_on(pose, cpu, 1), pose) and torch.equal(pr.ends.pose_on([pose.view(3, 4)], cpu, 1), pose)
    assert torch.equal(pr.ends.pose_on(pose.view(1, 3, 4), cpu, 1), pose)
    assert Predictor(None, args).ends.pose_on(pose, cpu, 1) is None and pr.ends.pose_on(None, cpu, 1) is None
    with pytest.raises(ValueError):
        pr.ends.pose_on(pose, cpu, 2)
    for fn in (Predictor.__init__, PipelinedPredictor.__init__):
        assert inspect.signature(fn).parameters["ground_grid"].default is None
    for fn in (Predictor.__call__, PipelinedPredictor.submit):
        assert inspect.signature(fn).parameters["camera_pose"].default is None
