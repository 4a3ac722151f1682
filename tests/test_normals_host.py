"""-m "not gpu": the surface normals' host side -- Statement N's reference (tests/normals_ref.py) against analytic surfaces, the test
maps' distance from every threshold, the mutation condition that gives the GPU test's angle bar its meaning, the two new symbols and
their argument checks (no launch happens), and the predictors' ``surface_normals`` keyword."""
import math
import os
import re

import pytest
import torch

import normals_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
# z = 1 / (q + a x) has the odd differences z(i) - z(-i) = -2 a i z^2 / (1 - (a i z)^2): the least-squares slope over a window is the
# derivative times 1 + (a z)^2 S4 / S2 + ..., S4 / S2 = sum i^4 / sum i^2 <= 11.8 (r = 4).  The normal's tangent is fx a z, so the
# fitted normal is off by about 11.8 (a z)^3 fx radians: below 1e-9 only for a z <= 4e-5, a plane within 1.2 degrees of facing the
# camera at fx ~ 520.  GENTLE planes are held to the issue's 1e-9; a plane tilted by ~40 degrees to the formula's own figure.
GENTLE = [(1.0e-5, -0.8e-5, 0.4), (-0.5e-5, 1.0e-5, 0.25), (0.0, 0.0, 0.5)]
STEEP = (8.0e-4, -5.0e-4, 0.45)


@pytest.mark.parametrize("r", ref.RADII)
def test_reference_recovers_the_normal_of_a_plane(r):
    H, W = 23, 31
    K = ref.intrinsics(H, W)                                                   # fx != fy, cx and cy off the centre, per image
    for a, b, c in GENTLE:
        depth = ref.plane(H, W, a, b, c).view(1, 1, H, W).expand(ref.CASE_B, 1, H, W).contiguous()
        got = ref.normals(depth, K, r, near=0.1, far=100.0)
        assert int(got.valid.sum()) == ref.CASE_B * (H - 2 * r) * (W - 2 * r)
        for i in range(ref.CASE_B):
            want = ref.plane_normal(K[i], a, b, c).view(1, 3, 1, 1).expand(1, 3, H, W)
            # the map is the plane rounded to fp32: a slope over (2r + 1)^2 cells of relative noise 2^-24 moves the normal by
            # fx z 2^-24 / sqrt(D) < 1e-4 rad; the fp64 plane itself is recovered to 1e-9
            ang = ref.angle(got.normals[i:i + 1], want)[got.valid[i:i + 1]]
            assert float(ang.max()) < 1e-4
        exact = _normals_of_fp64_plane(H, W, K, a, b, c, r)
        for i in range(ref.CASE_B):
            want = ref.plane_normal(K[i], a, b, c).view(1, 3, 1, 1).expand(1, 3, H, W)
            ang = ref.angle(exact[i:i + 1], want)[0, r:H - r, r:W - r]
            assert float(ang.max()) < 1e-9, (r, a, b, c, float(ang.max()))
    a, b, c = STEEP
    exact = _normals_of_fp64_plane(H, W, K, a, b, c, r)
    z = 1.0 / c
    bound = 2.0 * 11.8 * ((abs(a) + abs(b)) * 1.3 * z) ** 3 * 530.0            # (z grows to ~1.3 / c over this map)
    for i in range(ref.CASE_B):
        want = ref.plane_normal(K[i], a, b, c).view(1, 3, 1, 1).expand(1, 3, H, W)
        ang = ref.angle(exact[i:i + 1], want)[0, r:H - r, r:W - r]
        assert float(ang.max()) < bound < 1e-3, (r, float(ang.max()), bound)
    assert abs(float(ref.plane_normal(K[0], a, b, c)[2])) < 0.8                # tilted by more than 36 degrees


def _normals_of_fp64_plane(H, W, K, a, b, c, r):
    """Statement N's slopes and normal on the plane in fp64 (the fp32 rounding of the map left out): ref.slopes takes an fp64 map too."""
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    z = (1.0 / (a * x + b * y + c)).view(1, 1, H, W).expand(ref.CASE_B, 1, H, W)
    zu, zv = ref.slopes(z, r)
    k = K.double()
    fx, fy, cx, cy = (k[:, i].view(-1, 1, 1) for i in range(4))
    m = torch.stack([fx * zu, fy * zv, -(z[:, 0] + (x - cx) * zu + (y - cy) * zv)], 1)
    return m / m.norm(dim=1, keepdim=True)


def test_validity_on_the_step_map_is_the_windows_that_do_not_straddle_the_step():
    H, W, col = 21, 70, 38
    depth = ref.step(H, W, col).view(1, 1, H, W)
    K = ref.intrinsics(H, W, 1)
    for r in ref.RADII:
        valid = ref.validity(depth, K, r, ref.NEAR, ref.FAR, ref.EDGE)[0]
        x = torch.arange(W).view(1, W).expand(H, W)
        y = torch.arange(H).view(H, 1).expand(H, W)
        inside = (x >= r) & (x < W - r) & (y >= r) & (y < H - r)
        straddles = (x + r >= col) & (x - r < col)
        assert torch.equal(valid, inside & ~straddles), r
        assert int(valid.sum()) == (H - 2 * r) * (W - 2 * r - 2 * r)
    # a camera that cannot be used has no valid pixel
    for i, v in ((0, 0.0), (0, float("nan")), (1, -3.0), (1, INF), (2, float("nan")), (3, -INF)):
        k = K.clone()
        k[0, i] = v
        assert not ref.validity(depth, k, 2, ref.NEAR, ref.FAR, ref.EDGE).any()


def test_special_cells_invalidate_exactly_their_windows():
    H, W, r = 17, 19, 2
    base = ref.plane(H, W, 2e-5, 1e-5, 0.4)
    K = ref.intrinsics(H, W, 1)
    for v in (float("nan"), INF, -INF, 0.2, 12.0):
        z = base.clone()
        z[8, 9] = v
        valid = ref.validity(z.view(1, 1, H, W), K, r, ref.NEAR, ref.FAR, ref.EDGE)[0]
        want = torch.zeros(H, W, dtype=torch.bool)
        want[r:H - r, r:W - r] = True
        want[8 - r:8 + r + 1, 9 - r:9 + r + 1] = False
        assert torch.equal(valid, want), v
    n = ref.normals(base.view(1, 1, H, W), K, r)
    assert not n.normals[0][:, ~n.valid[0]].any() and not n.rgb8[0][~n.valid[0]].any()
    assert bool(((n.normals[0].norm(dim=0) - 1).abs()[n.valid[0]] < 1e-12).all())
    assert bool((n.normals[0, 2][n.valid[0]] < 0).all())                       # pointing at the camera


def test_no_pixel_of_the_step_and_range_maps_is_near_a_threshold():
    """So a rounding on the reference's side cannot flip a pixel of these maps: everything tested is at least 1e-4 (relative) away from
    its threshold."""
    for H, W in ref.CASE_SHAPES:
        for r in ref.RADII:
            depth, _ = ref.case(H, W)
            assert ref.threshold_margin(depth[0:1], r) > 1e-4, (H, W, r, "step / plane")
            assert ref.threshold_margin(depth[2:3], r) > 1e-4, (H, W, r, "sphere")
    z = ref.sprinkle(ref.plane(24, 40, 2e-5, 1e-5, 0.4), 3).view(1, 1, 24, 40)
    assert torch.isnan(z).any() and torch.isinf(z).any() and bool((z == 0.2).any()) and bool((z == 12.0).any())
    for r in ref.RADII:
        assert ref.threshold_margin(z, r) > 1e-4


def test_each_planted_error_moves_the_normals_by_far_more_than_the_bar():
    """The mutation condition: each of the four deliberate errors moves at least 1 % of the valid pixels of the test maps by more than
    1e-2 rad -- ten times the highest bar the GPU test may use (1e-3 rad)."""
    for mutation in ref.MUTATIONS:
        moved = total = 0
        for H, W in ref.CASE_SHAPES[2:]:
            for r in ref.RADII:
                depth, K = ref.case(H, W)
                good = ref.normals(depth, K, r)
                bad = ref.normals(depth, K, r, mutation=mutation)
                assert torch.equal(good.valid, bad.valid)
                ang = ref.angle(good.normals, bad.normals)[good.valid]
                moved += int((ang > 1e-2).sum())
                total += ang.numel()
        assert total > 2000 and moved >= 0.01 * total, (mutation, moved, total)


def test_case_maps_have_what_the_gpu_test_needs():
    for H, W in ref.CASE_SHAPES:
        depth, K = ref.case(H, W, bad_camera=1)
        assert depth.dtype == torch.float32 and tuple(depth.shape) == (3, 1, H, W) and torch.isnan(K[1, 0])
        counts = [[int(v) for v in ref.validity(depth, K, r, ref.NEAR, ref.FAR, ref.EDGE).flatten(1).sum(1)] for r in ref.RADII]
        assert all(c[1] == 0 for c in counts)
        if (H, W) == (8, 8):
            assert counts[3] == [0, 0, 0]
        if (H, W) == (9, 9):
            assert counts[3][0] == 1
    depth, K = ref.case(37, 131)
    v = ref.validity(depth, K, 2, ref.NEAR, ref.FAR, ref.EDGE).flatten(1).float().mean(1)
    assert all(0.05 < float(f) < 0.97 for f in v), v                            # every image has valid and invalid pixels
    assert torch.isnan(depth[1]).any() and torch.isinf(depth[1]).any()


# ---------------------------------------------------------------------------
# the library and the wrappers
# ---------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported(lib):
    from objcavit_amd import _lib, build, hip_ops
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_depth_normals_fwd\s*\(", header) and re.search(r"\bint\s+ocv_normals_gather_fwd\s*\(", header)
    assert re.search(r"#define\s+OCV_ABI_VERSION\s+5\b", header) and "STATEMENT N" in header
    for name in ("ocv_depth_normals_fwd", "ocv_normals_gather_fwd"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "surface_normals.hip" in build.SOURCES
    assert lib.ocv_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert callable(hip_ops.depth_normals) and callable(hip_ops.normals_gather)
    assert hip_ops.NORMALS_MAX_RADIUS == max(ref.RADII)


def _dense(lib, depth=64, K=64, H=8, W=8, r=2, near=0.0, far=10.0, edge=0.05, normals=64, rgb8=None, valid=None, B=1):
    """The entry point with made-up (never dereferenced) device addresses: every call here must be refused before any launch."""
    return lib.ocv_depth_normals_fwd(depth, K, H, W, r, near, far, edge, normals, rgb8, valid, B, None)


@pytest.mark.parametrize("kw,word", [
    (dict(r=0), "radius"), (dict(r=5), "radius"), (dict(r=-1), "radius"),
    (dict(normals=None), "no output"),
    (dict(depth=None), "null"), (dict(K=None), "null"),
    (dict(B=0), "sizes"), (dict(H=0), "sizes"), (dict(W=-3), "sizes"), (dict(H=1 << 16, W=1 << 16), "2^31"),
    (dict(near=2.0, far=1.0), "near"), (dict(near=float("nan")), "near"),
    (dict(edge=0.0), "edge_ratio"), (dict(edge=-0.1), "edge_ratio"), (dict(edge=float("nan")), "edge_ratio"),
    (dict(K=72), "aligned"), (dict(normals=66), "misaligned"), (dict(depth=65), "misaligned"),
])
def test_bad_arguments_of_the_dense_launch_are_refused_before_any_launch(lib, kw, word):
    assert _dense(lib, **kw) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_depth_normals_fwd:") and word in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(normals=None), "null"), (dict(pixel=None), "null"), (dict(counts=None), "null"), (dict(out=None), "null"),
    (dict(cap=0), "sizes"), (dict(B=0), "sizes"), (dict(H=0), "sizes"), (dict(B=1 << 20, cap=1 << 20), "2^31"),
    (dict(out=72), "16-byte"), (dict(pixel=66), "misaligned"),
])
def test_bad_arguments_of_the_gather_are_refused_before_any_launch(lib, kw, word):
    a = dict(normals=64, pixel=64, counts=64, H=8, W=8, cap=16, out=64, B=1)
    a.update(kw)
    assert lib.ocv_normals_gather_fwd(a["normals"], a["pixel"], a["counts"], a["H"], a["W"], a["cap"], a["out"], a["B"], None) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_normals_gather_fwd:") and word in msg, msg


def test_wrappers_refuse_host_tensors_and_bad_options():
    import inspect
    from objcavit_amd import hip_ops
    from objcavit_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError):
        hip_ops.depth_normals(torch.ones(1, 1, 8, 8), torch.ones(1, 4))
    with pytest.raises(HipLibraryError):
        hip_ops.normals_gather(torch.ones(1, 3, 8, 8), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    params = inspect.signature(hip_ops.depth_normals).parameters
    assert list(params) == ["depth", "K", "radius", "near", "far", "edge_ratio", "want", "out", "image_index"]
    assert params["radius"].default == 2 and params["edge_ratio"].default == 0.05 and params["want"].default == ("normals",)
    assert params["near"].default == 0.0 and params["far"].default == INF


def test_module_and_result_type():
    from objcavit_amd import surface_normals as sn
    from objcavit_amd.predict import PredictResult, WANT, _ObjectsResult
    assert sn.SurfaceNormals._fields == ("normals", "rgb8", "valid", "points")
    assert "least-squares" in sn.__doc__.lower() and callable(sn.surface_normals)
    assert PredictResult._fields == ("depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence")
    assert WANT == ("depth", "depth_u16", "rgb8", "depth_std", "confidence") and PredictResult.normals is None
    res = _ObjectsResult(1, 2, 3, 4, 5, normals=sn.SurfaceNormals("n"))
    assert res.normals.normals == "n" and res.points is None and tuple(res) == (1, 2, 3, 4, 5, None, None)
    assert res._replace(bin_edges=None).normals is res.normals


def test_predictors_validate_the_surface_normals_keyword():
    from objcavit_amd.config import make_args
    from objcavit_amd.predict import Predictor, _Ends
    args = make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip")
    ds = args[args.basic.dataset]
    pr = Predictor(None, args, surface_normals={})
    assert pr.ends.normals == {"radius": 2, "edge_ratio": 0.05, "near": float(ds.min_depth), "far": float(ds.max_depth), "picture": False,
                               "valid": False}
    assert Predictor(None, args).ends.normals is None and pr.ends.cloud is None
    o = Predictor(None, args, surface_normals=dict(radius=4, edge_ratio=0.1, near=0.25, far=6.0, picture=True, valid=True)).ends.normals
    assert o == {"radius": 4, "edge_ratio": 0.1, "near": 0.25, "far": 6.0, "picture": True, "valid": True}
    for bad in (dict(radius=0), dict(radius=5), dict(radius=2.5), dict(edge_ratio=0.0), dict(edge_ratio=float("nan")),
                dict(near=3.0, far=1.0), dict(window=3)):
        with pytest.raises(ValueError):
            Predictor(None, args, surface_normals=bad)
    # the cloud's normals=True implies the keyword with its defaults, and the cloud's own options stay what they are
    both = Predictor(None, args, point_cloud=dict(normals=True, stride=(2, 3)))
    assert both.ends.normals == pr.ends.normals and both.ends.cloud_normals is True and both.ends.cloud["pixel"] is False and "normals" not in both.ends.cloud
    assert Predictor(None, args, point_cloud={}).ends.normals is None
    # intrinsics are taken with either keyword
    K = torch.tensor([[500.0, 500.0, 10.0, 10.0]])
    assert pr.ends.intrinsics_on(K, torch.device("cpu"), 1) is not None and Predictor(None, args).ends.intrinsics_on(K, torch.device("cpu"), 1) is None
    assert isinstance(pr.ends, _Ends)
