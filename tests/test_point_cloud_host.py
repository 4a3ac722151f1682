"""-m "not gpu": the point-cloud output's host side -- the two new symbols and their argument checks (no launch happens), the workspace
formula, the reference statement of tests/point_cloud_ref.py against float64, the intrinsics helpers, and the pinned predict interface."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import point_cloud_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from objcavit_amd import _lib, build, hip_ops
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_depth_unproject_fwd\s*\(", header)
    assert re.search(r"\bsize_t\s+ocv_depth_unproject_workspace_bytes\s*\(", header)
    assert re.search(r"#define\s+OCV_ABI_VERSION\s+5\b", header) and re.search(r"#define\s+OCV_UNPROJECT_TILE\s+2048\b", header)
    for name in ("ocv_depth_unproject_fwd", "ocv_depth_unproject_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "point_cloud.hip" in build.SOURCES
    assert lib.ocv_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert callable(hip_ops.depth_unproject) and hip_ops.UNPROJECT_TILE == ref.TILE == 2048


def _call(lib, depth=64, K=64, points=64, counts=64, total=64, ws=64, ws_bytes=1 << 20, frames=None, frame_stride=0, row_stride=0, Hs=0,
          Ws=0, top=0, left=0, B=1, H=8, W=8, sy=1, sx=1, near=0.0, far=10.0, cap=64, pixel=None):
    """The entry point with made-up (never dereferenced) device addresses: every call here must be refused before any launch."""
    return lib.ocv_depth_unproject_fwd(depth, K, None, None, frames, frame_stride, row_stride, Hs, Ws, top, left, B, H, W, sy, sx, near,
                                       far, 0.0, INF, cap, points, pixel, counts, total, ws, ws_bytes, None)


FRAME = dict(frames=64, Hs=10, Ws=12, row_stride=36, frame_stride=360)


@pytest.mark.parametrize("kw,word", [
    (dict(depth=None), "null pointer"), (dict(K=None), "null pointer"), (dict(points=None), "null pointer"),
    (dict(counts=None), "null pointer"), (dict(total=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(B=0), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"), (dict(H=1 << 16, W=1 << 16), "bad sizes"),
    (dict(sy=0), "stride"), (dict(sx=0), "stride"), (dict(sx=-2), "stride"),
    (dict(cap=0), "capacity"), (dict(cap=-5), "capacity"),
    (dict(near=2.0, far=1.0), "near"), (dict(near=float("nan")), "near"), (dict(far=float("nan")), "near"),
    (dict(FRAME, top=3), "outside"), (dict(FRAME, left=5), "outside"), (dict(FRAME, top=-1), "outside"), (dict(FRAME, Hs=7), "outside"),
    (dict(FRAME, row_stride=35), "strides"), (dict(FRAME, B=2, frame_stride=359), "strides"),
    (dict(ws_bytes=3), "workspace too small"), (dict(H=61, W=83, B=3, ws_bytes=35), "workspace too small"),
    (dict(points=72), "16-byte aligned"), (dict(K=68), "16-byte aligned"), (dict(depth=66), "misaligned"), (dict(pixel=65), "misaligned"),
])
def test_bad_arguments_are_refused_with_a_message_before_any_launch(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_depth_unproject_fwd:") and word in msg, msg


def test_workspace_bytes_is_one_int_per_tile(lib):
    """B * T * 4, T = ceil(ceil(H / sy) * ceil(W / sx) / 2048); 0 for sizes the entry point refuses."""
    for B, H, W, sy, sx in ((1, 1, 1, 1, 1), (3, 61, 83, 1, 1), (3, 61, 83, 2, 3), (16, 480, 640, 1, 1), (16, 480, 640, 2, 2),
                            (2, 352, 1216, 1, 1), (1, 32, 64, 1, 1), (1, 32, 64, 1, 64), (1, 32, 65, 1, 64), (5, 7, 9, 100, 100)):
        n = math.ceil(H / sy) * math.ceil(W / sx)
        assert lib.ocv_depth_unproject_workspace_bytes(B, H, W, sy, sx) == B * math.ceil(n / 2048) * 4, (B, H, W, sy, sx)
    assert lib.ocv_depth_unproject_workspace_bytes(16, 480, 640, 1, 1) == 16 * 150 * 4          # NYU: 150 tiles per image
    assert lib.ocv_depth_unproject_workspace_bytes(1, 352, 1216, 1, 1) == 209 * 4               # KITTI: 209
    for bad in ((0, 8, 8, 1, 1), (1, 0, 8, 1, 1), (1, 8, 8, 0, 1), (1, 8, 8, 1, -1), (1, 1 << 16, 1 << 16, 1, 1)):
        assert lib.ocv_depth_unproject_workspace_bytes(*bad) == 0, bad


def test_wrapper_refuses_host_tensors_and_has_the_documented_signature():
    import inspect
    from objcavit_amd import hip_ops
    from objcavit_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError):
        hip_ops.depth_unproject(torch.ones(1, 1, 4, 4), torch.ones(1, 4), 16)
    params = inspect.signature(hip_ops.depth_unproject).parameters
    assert list(params) == ["depth", "K", "capacity", "stride", "near", "far", "confidence", "min_confidence", "depth_std", "max_std",
                            "frames", "top", "left", "want_pixel", "out", "workspace", "image_index"]
    assert params["stride"].default == (1, 1) and params["max_std"].default == INF and params["image_index"].default == 0
    assert hip_ops.unproject_grid(61, 83, (2, 3)) == (31, 28) and hip_ops.unproject_grid(480, 640) == (480, 640)
    with pytest.raises(ValueError):
        hip_ops.unproject_grid(8, 8, (0, 1))


# ---------------------------------------------------------------------------
# the reference statement itself
# ---------------------------------------------------------------------------
def test_reference_agrees_with_a_float64_pinhole_computation():
    """X = fl(fl(fl(x - cx) / fx) * z): three roundings, each within u = 2^-24 relative (no subnormals here: |x - cx| >= 0.2, fx ~ 70,
    z >= 1), so |X - X64| <= ((1 + u)^3 - 1) |X64| < 3 u (1 + 2^-20) |X64| -- at most 3 fp32 ulps of |X| (one ulp is at least u |X|)."""
    u = 2.0 ** -24
    bound = 3.0 * u * (1.0 + 2.0 ** -20)
    assert (1.0 + u) ** 3 - 1.0 < bound
    K = ref.case_intrinsics()
    for mask, stride in (("all", (1, 1)), ("random_half", (2, 3))):
        depth = ref.case_depth(mask)
        clouds = ref.unproject(depth, K, stride, ref.NEAR, ref.FAR)
        assert sum(c.records.shape[0] for c in clouds) > 1000
        gap = ref.float64_gap(depth, K, clouds)
        assert 0.0 < gap <= bound, (gap, bound)
        for b, c in enumerate(clouds):
            assert torch.equal(c.records[:, 2], depth[b, 0].reshape(-1)[c.pixel.long()])          # Z is the map's element


def test_reference_masks_order_and_bytes():
    K = ref.case_intrinsics()
    H, W = ref.CASE_H, ref.CASE_W
    full = ref.unproject(ref.case_depth("all"), K, (1, 1), ref.NEAR, ref.FAR)
    assert [c.records.shape[0] for c in full] == [H * W] * 3 and torch.equal(full[0].pixel, torch.arange(H * W, dtype=torch.int32))
    assert all(c.records.shape[0] == 0 for c in ref.unproject(ref.case_depth("none"), K, (1, 1), ref.NEAR, ref.FAR))
    assert ref.unproject(ref.case_depth("first_pixel"), K, (2, 3), ref.NEAR, ref.FAR)[1].pixel.tolist() == [0]
    assert ref.unproject(ref.case_depth("last_tile"), K, (1, 1), ref.NEAR, ref.FAR)[2].pixel[0] == 2 * ref.TILE
    strided = ref.unproject(ref.case_depth("all"), K, (2, 3), ref.NEAR, ref.FAR)[0].pixel.long()
    assert strided.numel() == 31 * 28 and bool(((strided // W) % 2 == 0).all()) and bool(((strided % W) % 3 == 0).all())
    assert bool((strided[1:] > strided[:-1]).all())
    # the camera rule: fx = 0, fx = NaN, cx = inf, fy < 0 keep nothing
    for i, v in ((0, 0.0), (0, float("nan")), (2, INF), (1, -3.0), (3, -INF)):
        k = K.clone()
        k[1, i] = v
        got = ref.unproject(ref.case_depth("all"), k, (1, 1), ref.NEAR, ref.FAR)
        assert got[1].records.shape[0] == 0 and torch.equal(got[0].records, full[0].records) and torch.equal(got[2].pixel, full[2].pixel)
    # bytes 12-15: colour of the window's pixel, confidence rounded half to even, 255 / 0 without
    frames = ref.case_frames(0, 3, H + 5, W + 4)
    conf = ref.case_confidence()
    c = ref.unproject(ref.case_depth("all"), K, (1, 1), ref.NEAR, ref.FAR, confidence=conf, min_confidence=0.25, frames=frames, top=2, left=3)[0]
    by = c.records.view(torch.uint8)
    y, x = c.pixel.long() // W, c.pixel.long() % W
    assert torch.equal(by[:, 12:15], frames[0][2 + y, 3 + x])
    cv = conf[0, 0].reshape(-1)[c.pixel.long()]
    assert not torch.isnan(cv).any() and bool((cv >= 0.25).all()) and bool((cv == 0.25).any())        # NaN failed, the threshold passed
    assert bool((by[cv == 0.5, 15] == 128).all()) and bool((cv == 0.5).any())                       # 127.5 -> 128
    assert bool((by[cv >= 1.0, 15] == 255).all()) and bool((by[cv == 0.25, 15] == 64).all())        # 63.75 -> 64
    plain = ref.unproject(ref.case_depth("all"), K, (1, 1), ref.NEAR, ref.FAR)[0].records.view(torch.uint8)
    assert bool((plain[:, 15] == 255).all()) and not plain[:, 12:15].any()
    assert torch.round(torch.tensor([0.5, 1.5, 2.5, 126.5, 127.5])).tolist() == [0.0, 2.0, 2.0, 126.0, 128.0]


# ---------------------------------------------------------------------------
# objcavit_amd/point_cloud.py on CPU tensors
# ---------------------------------------------------------------------------
def test_intrinsics_helpers():
    from objcavit_amd.point_cloud import intrinsics_from_focal, shift_intrinsics
    K = intrinsics_from_focal([518.8579, 721.5377], 480, 640)
    assert K.dtype == torch.float32 and tuple(K.shape) == (2, 4) and K.is_contiguous()
    f = torch.tensor([518.8579, 721.5377], dtype=torch.float32)
    assert torch.equal(K[:, 0], f) and torch.equal(K[:, 1], f) and K[:, 2].tolist() == [319.5, 319.5] and K[:, 3].tolist() == [239.5, 239.5]
    assert intrinsics_from_focal(500.0, 375, 1242).tolist() == [[500.0, 500.0, 620.5, 187.0]]
    s = shift_intrinsics(K, 23, 13)
    assert torch.equal(s, ref.shift_intrinsics(K, 23, 13)) and s.dtype == torch.float32
    assert s.tolist() == [[float(f[0]), float(f[0]), 306.5, 216.5], [float(f[1]), float(f[1]), 306.5, 216.5]]
    assert torch.equal(shift_intrinsics(K, 0, 0), K)


def test_object_positions():
    from objcavit_amd.object_depth import ObjectDepths, object_fields
    from objcavit_amd.point_cloud import object_positions
    fields = object_fields((0.1, 0.5, 0.9))
    table = torch.zeros(2, 3, len(fields))
    table[0, 0] = torch.tensor([12.0, 1.0, 3.0, 2.0, 0.0, 1.5, 2.5, 2.9])
    table[0, 1] = torch.tensor([4.0, 4.0, 4.0, 4.0, 0.0, 4.0, 4.0, 4.0])
    table[1, 0] = torch.tensor([7.0, 5.0, 9.0, 6.0, 0.0, 5.5, 8.0, 8.5])          # rows [0, 2], [1, 1], [1, 2]: n = 0
    xywh = torch.tensor([[[100.5, 50.5, 20.0, 10.0, 9.0], [10.0, 20.0, 4.0, 4.0, 9.0], [30.0, 30.0, 5.0, 5.0, 9.0]],
                         [[64.0, 32.5, 8.0, 8.0, 9.0], [1.0, 1.0, 1.0, 1.0, 9.0], [2.0, 2.0, 2.0, 2.0, 9.0]]])
    K = torch.tensor([[50.0, 25.0, 60.0, 40.0], [100.0, 200.0, 13.5, 2.0]])
    pos = object_positions(ObjectDepths(table, torch.tensor([2, 1], dtype=torch.int32), fields), xywh, K)
    assert tuple(pos.shape) == (2, 3, 3) and pos.dtype == torch.float32
    # box centre 100.5 in pixel-edge coordinates = pixel coordinate 100.0: ((100 - 60) / 50) * 2.5 = 2.0, ((50 - 40) / 25) * 2.5 = 1.0
    assert pos[0, 0].tolist() == [2.0, 1.0, 2.5]
    assert pos[0, 1].tolist() == pytest.approx([(9.5 - 60.0) / 50.0 * 4.0, (19.5 - 40.0) / 25.0 * 4.0, 4.0], rel=1e-6)
    assert pos[1, 0].tolist() == pytest.approx([(63.5 - 13.5) / 100.0 * 8.0, (32.0 - 2.0) / 200.0 * 8.0, 8.0], rel=1e-6)
    assert not pos[0, 2].any() and not pos[1, 1:].any()
    assert object_positions(ObjectDepths(table, None, fields), xywh, K, field="min")[0, 0].tolist() == pytest.approx([0.8, 0.4, 1.0], rel=1e-6)


def test_point_cloud_views():
    from objcavit_amd.point_cloud import PointCloud
    pts = torch.zeros(2, 5, 4)
    pts.view(torch.uint8)[..., 12:16] = torch.tensor([1, 2, 3, 4], dtype=torch.uint8)
    pts[..., 0] = 7.0
    pc = PointCloud(pts, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), None)
    assert pc._fields == ("points", "counts", "total", "pixel") and pc.pixel is None and len(pc) == 4
    assert tuple(pc.xyz.shape) == (2, 5, 3) and pc.xyz.stride() == (20, 4, 1) and pc.xyz.dtype == torch.float32
    assert tuple(pc.rgba.shape) == (2, 5, 4) and pc.rgba.stride() == (80, 16, 1) and pc.rgba.dtype == torch.uint8
    assert pc.xyz.data_ptr() == pts.data_ptr() and pc.rgba.data_ptr() == pts.data_ptr() + 12          # views, not copies
    assert pc.rgba[1, 3].tolist() == [1, 2, 3, 4] and pc.xyz[1, 3].tolist() == [7.0, 0.0, 0.0]


# ---------------------------------------------------------------------------
# the predict interface
# ---------------------------------------------------------------------------
def test_predictors_reject_unknown_point_cloud_keys_and_fill_the_defaults():
    import inspect
    from objcavit_amd.config import make_args
    from objcavit_amd.predict import PipelinedPredictor, Predictor, _cloud_options, _cloud_want
    args = make_args()
    with pytest.raises(ValueError, match="unknown option"):
        Predictor(None, args, point_cloud={"strid": (2, 2)})
    with pytest.raises(ValueError, match="unknown option"):
        PipelinedPredictor(None, args, None, point_cloud={"color": True})          # refused before anything is captured
    for bad in ({"stride": (0, 1)}, {"capacity": 0}, {"near": 3.0, "far": 2.0}):
        with pytest.raises(ValueError):
            Predictor(None, args, point_cloud=bad)
    p = Predictor(None, args, point_cloud={})
    ds = args[args.basic.dataset]
    assert p.ends.cloud == {"stride": (1, 1), "near": float(ds.min_depth), "far": float(ds.max_depth), "min_confidence": 0.0,
                            "max_std": INF, "capacity": None, "colour": True, "pixel": False}
    assert Predictor(None, args).ends.cloud is None and Predictor(None, make_args(dataset="kitti"), point_cloud={}).ends.cloud["far"] == 80.0
    assert _cloud_options({"stride": 2, "colour": False}, 0.0, 1.0)["stride"] == (2, 2)
    assert _cloud_want(None) == () and _cloud_want(p.ends.cloud) == ()
    assert _cloud_want(_cloud_options({"min_confidence": 0.3, "max_std": 1.0}, 0.0, 1.0)) == ("confidence", "depth_std")
    for fn, name in ((Predictor.__init__, "point_cloud"), (PipelinedPredictor.__init__, "point_cloud"), (Predictor.__call__, "intrinsics"),
                     (PipelinedPredictor.submit, "intrinsics")):
        params = inspect.signature(fn).parameters
        assert name in params and params[name].default is None


def test_result_fields_are_unchanged_and_points_is_an_attribute():
    from objcavit_amd.predict import WANT, PredictResult, _ObjectsResult
    assert PredictResult._fields == ("depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence")
    assert WANT == ("depth", "depth_u16", "rgb8", "depth_std", "confidence")
    r = PredictResult(1, 2, 3, 4, 5)
    assert r.points is None and r.objects is None and len(r) == 7
    both = _ObjectsResult(*r, objects="table", points="cloud")
    assert isinstance(both, PredictResult) and both == r and tuple(both) == tuple(r) and both._fields == r._fields
    assert both.objects == "table" and both.points == "cloud"
    kept = both._replace(bin_edges=None)
    assert kept.objects == "table" and kept.points == "cloud" and kept.bin_edges is None and kept.depth == 1
    only = _ObjectsResult(*r, objects="table")                                     # the earlier keyword still stands alone
    assert only.points is None and only.objects == "table" and _ObjectsResult(*r, points="cloud").objects is None
