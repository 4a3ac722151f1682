"""-m "not gpu": host side of the lens on ingest -- the quantisation of Statement L, ``LensMap``'s builders against the models restated in
tests/lens_ref.py and against a Newton inversion written here, the two entry points' declarations and argument checks, the ``lens``
keyword's rules.  No kernel runs."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import lens_ref as ref
from objcavit_amd import _lib, hip_ops
from objcavit_amd.config import make_args
from objcavit_amd.lens import LensMap, quantise, taps_inside

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ocv_frame_remap_ingest_fwd", "ocv_frames_remap_rgb24_fwd")

# (name, builder, point of lens_ref, K, dist, source size, window size, new_K, R)
_c, _s = math.cos(0.03), math.sin(0.03)
CASES = [
    ("barrel", "brown", (41.3, 40.1, 18.2, 6.4), (-0.31, 0.09, 0.0012, -0.0007, -0.01), (13, 37), (11, 30), (38.0, 38.0, 14.6, 5.1), None),
    ("pincushion", "brown", (41.3, 40.1, 18.2, 6.4), (0.22, 0.05, -0.001, 0.0005), (13, 37), (13, 37), None, None),
    ("rational, rotated", "brown", (300.0, 301.5, 31.7, 23.2), (0.4, -0.2, 0.001, 0.002, 0.05, 0.38, -0.15, 0.03), (48, 64), (40, 56),
     (290.0, 290.0, 27.5, 19.5), [[_c, 0.0, _s], [0.0, 1.0, 0.0], [-_s, 0.0, _c]]),
    ("fisheye", "fisheye", (20.5, 20.1, 18.4, 6.2), (-0.02, 0.004, -0.0006, 0.00004), (13, 37), (12, 32), (9.0, 9.0, 15.5, 5.5), None),
]


def _build(case):
    name, kind, K, dist, src, win, new_K, R = case
    lm = getattr(LensMap, kind)(K, dist, src, window_size=win, new_K=new_K, R=R)
    point = ref.brown_point if kind == "brown" else ref.fisheye_point
    xs, ys = ref.model_coordinates(point, K, dist, win, new_K, R)
    return lm, xs, ys


def test_quantisation_rounds_half_up_clamps_and_marks_nan():
    Hs, Ws = 5, 9
    nan, inf = float("nan"), float("inf")
    #                half-way up     half-way (negative) up    below / above      the sentinels' edges              NaN, +-inf
    xs = torch.tensor([[127.5 / 256, -0.5 / 256, -1.5 / 256, 3.0, 2.25, -1.0, -1.0 - 1e-9, -7.0, float(Ws), Ws + 0.4, nan, inf, -inf]], dtype=torch.float64)
    want_x = [128, 0, -1, 768, 576, -256, -256, -256, Ws * 256, Ws * 256, -256, Ws * 256, -256]
    ys = torch.tensor([[0.0, 255.5 / 256, 4.0, float(Hs), 1e9, nan, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]], dtype=torch.float64)
    want_y = [0, 256, 1024, Hs * 256, Hs * 256, -256, 256, 256, 256, 256, 256, 256, 256]
    m = quantise(xs, ys, (Hs, Ws))
    assert m.dtype == torch.int32 and tuple(m.shape) == (1, 13, 2)
    assert m[0, :, 0].tolist() == want_x and m[0, :, 1].tolist() == want_y
    assert np.array_equal(m.numpy(), ref.quantise(xs.numpy(), ys.numpy(), Hs, Ws))
    lm = LensMap.from_coordinates(xs, ys, (Hs, Ws))
    assert lm.M == 1 and lm.window_size == (1, 13) and lm.source_size == (Hs, Ws) and lm.new_K is None and torch.equal(lm.map[0], m)
    # random coordinates around and beyond the frame, against the element-wise restatement
    g = torch.Generator().manual_seed(5)
    rx = (torch.rand(2, 7, 11, generator=g, dtype=torch.float64) * (Ws + 6) - 3)
    ry = (torch.rand(2, 7, 11, generator=g, dtype=torch.float64) * (Hs + 6) - 3)
    rx[0, 0, 0], ry[1, 2, 3] = nan, nan
    lm = LensMap.from_coordinates(rx, ry, (Hs, Ws), new_K=(1.0, 2.0, 3.0, 4.0))
    assert lm.M == 2 and lm.new_K == (1.0, 2.0, 3.0, 4.0)
    assert np.array_equal(lm.map.numpy(), ref.quantise(rx.numpy(), ry.numpy(), Hs, Ws))
    assert int(lm.map.min()) == -256 and int(lm.map[..., 0].max()) == Ws * 256 and int(lm.map[..., 1].max()) == Hs * 256


def test_valid_is_exactly_four_taps_inside():
    Hs, Ws = 5, 9
    X = torch.tensor([-256, -1, 0, 255, 256, (Ws - 2) * 256 + 255, (Ws - 1) * 256, (Ws - 1) * 256 + 1, Ws * 256], dtype=torch.int32)
    Y = torch.tensor([-256, -1, 0, (Hs - 2) * 256 + 255, (Hs - 1) * 256, Hs * 256], dtype=torch.int32)
    m = torch.stack([X.view(1, -1).expand(len(Y), len(X)), Y.view(-1, 1).expand(len(Y), len(X))], -1).contiguous()
    lm = LensMap(m, (Hs, Ws))
    count = ref.taps_inside(m.numpy(), Hs, Ws)
    assert set(count.ravel().tolist()) == {0, 1, 2, 4}
    assert np.array_equal(lm.valid[0].numpy(), (count == 4).astype(np.uint8)) and lm.valid.dtype == torch.uint8
    assert torch.equal(lm.valid[0], taps_inside(m, (Hs, Ws)))
    # x0 = Ws - 1 on the last column: the second tap is outside even at weight 0 -> not "valid"
    assert lm.valid[0, 2].tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 0]
    with pytest.raises(TypeError):
        LensMap(m.float(), (Hs, Ws))
    with pytest.raises(ValueError):
        LensMap(m[..., :1].contiguous(), (Hs, Ws))


def test_identity_and_brown_without_coefficients():
    src = (13, 37)
    ident = LensMap.identity(src, 2, 5, (9, 30))
    u, v = np.meshgrid(np.arange(30), np.arange(9))
    assert np.array_equal(ident.map[0, ..., 0].numpy(), 256 * (5 + u)) and np.array_equal(ident.map[0, ..., 1].numpy(), 256 * (2 + v))
    assert bool(ident.valid.all()) and ident.window_size == (9, 30)
    rest = LensMap.identity(src, 2, 5)
    assert rest.window_size == (11, 32) and not bool(rest.valid[0, -1].any()) and not bool(rest.valid[0, :, -1].any())
    K = (41.3, 40.1, 18.2, 6.4)
    for dist in ((0.0, 0.0, 0.0, 0.0), (0.0,) * 5, (0.0,) * 8):
        lm = LensMap.brown(K, dist, src)
        assert torch.equal(lm.map, LensMap.identity(src).map) and lm.new_K == K and lm.window_size == src
    # a window at an offset is the identity with the principal point moved
    shifted = LensMap.brown(K, (0.0,) * 4, src, window_size=(9, 30), new_K=(K[0], K[1], K[2] - 5, K[3] - 2))
    assert torch.equal(shifted.map, ident.map)
    mat = [[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]]
    assert torch.equal(LensMap.brown(mat, (0.1, 0.0, 0.0, 0.0), src).map, LensMap.brown(K, (0.1, 0.0, 0.0, 0.0), src).map)
    with pytest.raises(ValueError):
        LensMap.brown(K, (0.1, 0.2, 0.3), src)
    with pytest.raises(ValueError):
        LensMap.fisheye(K, (0.1,) * 5, src)
    with pytest.raises(ValueError):
        LensMap.brown((0.0, 1.0, 1.0, 1.0), (0.0,) * 4, src)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_builders_equal_the_restated_models(case):
    """Entries are equal; an entry may differ by 1 only where the float64 coordinate x 256 lies within 1e-6 of a half-integer -- the only
    place where two float64 evaluations that differ in their last bits may round apart."""
    lm, xs, ys = _build(case)
    Hs, Ws = case[4]
    want = ref.quantise(xs, ys, Hs, Ws).astype(np.int64)
    got = lm.map[0].numpy().astype(np.int64)
    assert got.shape == want.shape
    diff = np.abs(got - want)
    coord = np.stack([xs, ys], -1) * 256
    near_half = np.abs(coord - np.floor(coord) - 0.5) < 1e-6
    print(f"{case[0]}: {int((diff != 0).sum())} entries differ, {int(near_half.sum())} within 1e-6 of a half-integer")
    assert int(diff.max()) <= 1 and not bool(((diff != 0) & ~near_half).any())
    assert lm.new_K == tuple(float(v) for v in (case[6] or case[2]))
    u, _ = np.meshgrid(np.arange(got.shape[1]), np.arange(got.shape[0]))
    assert int(np.abs(got[..., 0] - 256 * u).max()) > 128                         # the case does bend: more than half a pixel off the identity


def _undistort(xs, ys, K, forward):
    """Newton iteration in float64 on the ray (x, y) with forward(x, y) = (xs, ys): numerical 2 x 2 Jacobian."""
    fx, fy, cx, cy = K
    x, y = (xs - cx) / fx, (ys - cy) / fy
    for _ in range(60):
        px, py = forward(x, y)
        ex, ey = px - xs, py - ys
        if abs(ex) < 1e-13 and abs(ey) < 1e-13:
            break
        h = 1e-7
        ax, ay = forward(x + h, y)
        bx, by = forward(x, y + h)
        j00, j10, j01, j11 = (ax - px) / h, (ay - py) / h, (bx - px) / h, (by - py) / h
        det = j00 * j11 - j01 * j10
        x, y = x - (j11 * ex - j01 * ey) / det, y - (-j10 * ex + j00 * ey) / det
    return x, y


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=lambda c: c[0])
def test_round_trip_through_a_newton_inversion(case):
    """Rectified pixel -> the model's source coordinate -> undistorted by Newton -> back at the pixel within 1e-9 px; and the map's entry
    is that source coordinate within half a map unit."""
    name, kind, K, dist, src, win, new_K, R = case
    nk = new_K or K
    lm = getattr(LensMap, kind)(K, dist, src, window_size=win, new_K=new_K)
    point = ref.brown_point if kind == "brown" else ref.fisheye_point
    worst = 0.0
    for v in range(0, win[0], 2):
        for u in range(0, win[1], 3):
            x, y = (u - nk[2]) / nk[0], (v - nk[3]) / nk[1]
            xs, ys = point(x, y, K, dist)
            bx, by = _undistort(xs, ys, K, lambda a, b: point(a, b, K, dist))
            worst = max(worst, abs(bx * nk[0] + nk[2] - u), abs(by * nk[1] + nk[3] - v))
            X, Y = (int(t) for t in lm.map[0, v, u])
            if -256 < X < src[1] * 256 and -256 < Y < src[0] * 256:
                assert abs(X - xs * 256) <= 0.5 + 1e-9 and abs(Y - ys * 256) <= 0.5 + 1e-9, (u, v)
    print(f"{name}: round trip off by at most {worst:.3e} px")
    assert worst < 1e-9


def test_fisheye_without_coefficients_is_f_atan_r():
    K, src = (20.5, 20.5, 18.0, 6.0), (13, 37)
    lm = LensMap.fisheye(K, (0.0, 0.0, 0.0, 0.0), src, new_K=(9.0, 9.0, 18.0, 6.0))
    for v in range(13):
        for u in range(37):
            x, y = (u - 18.0) / 9.0, (v - 6.0) / 9.0
            r = math.hypot(x, y)
            rd = K[0] * math.atan(r)                                             # the distance from the principal point, in source pixels
            X, Y = (int(t) for t in lm.map[0, v, u])
            xs, ys = (X / 256 - K[2], Y / 256 - K[3])
            if -256 < X < 37 * 256 and -256 < Y < 13 * 256:
                assert abs(math.hypot(xs, ys) - rd) <= math.sqrt(0.5) / 256 + 1e-9, (u, v)
                if r > 0:
                    assert abs(xs * y - ys * x) <= (abs(x) + abs(y)) / 256, (u, v)          # on the ray's own line through the centre
    assert (int(lm.map[0, 6, 18, 0]), int(lm.map[0, 6, 18, 1])) == (18 * 256, 6 * 256)


def test_entry_points_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    declared = set(re.findall(r"\b(ocv_[a-z0-9_]+)\s*\(", hdr))
    assert "STATEMENT L" in hdr
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES, name
    for name in ("frame_remap_ingest", "frames_remap_rgb24"):
        assert callable(getattr(hip_ops, name)) and name in hip_ops.frames.__all__
    assert list(inspect.signature(hip_ops.frame_remap_ingest).parameters) == ["frames", "table", "lens_map", "pixel_format", "mirror_too", "out",
                                                                             "out_index", "yuv_tables"]
    assert list(inspect.signature(hip_ops.frames_remap_rgb24).parameters) == ["frames", "lens_map", "pixel_format", "out", "yuv_tables"]
    from objcavit_amd import build
    assert "frame_remap.hip" in build.SOURCES
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.ocv_abi_version() == _lib.ABI_VERSION == 5                        # symbols are only added
    p = 4096                                                                     # any non-null, aligned address: it is never dereferenced
    Hs, Ws, B = 9, 13, 2
    dense = {0: [p, Hs * Ws * 3, Ws * 3, None, 0, 0, None, 0, 0], 1: [p, Hs * Ws * 3, Ws * 3, None, 0, 0, None, 0, 0],
             2: [p, Hs * Ws * 4, Ws * 4, None, 0, 0, None, 0, 0], 3: [p, Hs * Ws * 4, Ws * 4, None, 0, 0, None, 0, 0],
             4: [p, Hs * Ws, Ws, p, 5 * 14, 14, None, 0, 0], 5: [p, Hs * Ws, Ws, p, 35, 7, p, 35, 7]}

    def fused(fmt=4, yuv=p, Hs=Hs, Ws=Ws, map_=p, M=1, Hw=6, Ww=8, table=p, out=p, B=B, mirror=0, off=0, **edit):
        pl = list(dense.get(fmt, dense[5]))
        for i, v in edit.items():
            pl[int(i[1:])] = v
        return lib.ocv_frame_remap_ingest_fwd(fmt, *pl, yuv, Hs, Ws, map_, M, Hw, Ww, table, out, B, mirror, off, None)

    def to_rgb(fmt=4, yuv=p, Hs=Hs, Ws=Ws, map_=p, M=1, Hw=6, Ww=8, out=p, B=B, **edit):
        pl = list(dense.get(fmt, dense[5]))
        for i, v in edit.items():
            pl[int(i[1:])] = v
        return lib.ocv_frames_remap_rgb24_fwd(fmt, *pl, yuv, Hs, Ws, map_, M, Hw, Ww, out, B, None)

    for call, who in ((fused, b"ocv_frame_remap_ingest_fwd"), (to_rgb, b"ocv_frames_remap_rgb24_fwd")):
        def refused(what, **kw):
            assert call(**kw) == -1, (who, kw)
            msg = lib.ocv_last_error()
            assert msg.startswith(who + b":") and what in msg, (who, kw, msg)

        refused(b"null pointer", a0=None)
        refused(b"null pointer", fmt=4, a3=None)
        refused(b"null pointer", fmt=5, a6=None)
        refused(b"null pointer", out=None)
        refused(b"null pointer", map_=None)
        refused(b"16-byte aligned", map_=p + 4)                                  # 4-byte aligned is not enough: the map is read 16 bytes at a time
        refused(b"16-byte aligned", map_=p + 8)
        refused(b"M = 3", M=3)                                                   # neither 1 nor B
        refused(b"M = 0", M=0)
        refused(b"M = 2", M=2, B=3, a1=Hs * Ws, a4=5 * 14)
        assert call(M=2, Hw=0) == -1 and b"bad sizes" in lib.ocv_last_error()    # M = B passes the M check
        refused(b"unknown pixel format", fmt=6)
        refused(b"bad sizes", B=0)
        refused(b"bad sizes", Hs=0)
        refused(b"bad sizes", Hw=0)                                              # the window
        refused(b"bad sizes", Ww=-1)
        refused(b"strides", fmt=4, a2=Ws - 1)
        refused(b"strides", fmt=4, a1=Hs * Ws - 1)
        refused(b"strides", fmt=4, a5=13)
        refused(b"strides", fmt=5, a8=6)
        refused(b"strides", fmt=1, a2=Ws * 3 - 1)
        refused(b"strides", fmt=3, a2=Ws * 4 - 1)
        refused(b"yuv_table", fmt=4, yuv=None)
        refused(b"yuv_table", fmt=5, yuv=p + 2)
        for fmt in range(4):
            assert call(fmt=fmt, yuv=None, B=0) == -1 and b"bad sizes" in lib.ocv_last_error()      # packed: no tables asked for
    assert fused(table=None) == -1 and b"null pointer" in lib.ocv_last_error()
    assert fused(out=p + 2) == -1 and b"aligned" in lib.ocv_last_error()
    assert fused(table=p + 1) == -1 and b"aligned" in lib.ocv_last_error()
    assert fused(mirror=1, off=8) == -1 and b"mirror" in lib.ocv_last_error()
    assert fused(mirror=1, off=-(B * 3 * 6 * 8 - 1)) == -1 and b"mirror" in lib.ocv_last_error()


def test_wrappers_refuse_host_tensors_and_wrong_maps():
    table = torch.zeros(3, 256)
    frames = torch.zeros(2, 13, 37, 3, dtype=torch.uint8)
    lm = LensMap.identity((13, 37), 1, 2, (8, 12))
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.frame_remap_ingest(frames, table, lm)
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.frames_remap_rgb24(frames, lm, "rgb24")
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.frames_remap_rgb24(frames, lm.map)                               # a map tensor on the host
    with pytest.raises(_lib.HipLibraryError):
        lm.on("cpu")
    with pytest.raises(TypeError):
        hip_ops.frames_remap_rgb24(frames, lm, "nv12")                           # a tensor where planes are needed


def test_the_lens_keyword_of_both_predictors():
    from objcavit_amd import predict
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    for fn in (Predictor.__init__, PipelinedPredictor.__init__):
        params = inspect.signature(fn).parameters
        assert "lens" in params and params["lens"].default is None
        assert list(params)[-6:] == ["pixel_format", "crop", "resize", "object_metrics", "point_cloud", "object_depth"]      # pinned by earlier tests
    for fn in (Predictor.__call__, PipelinedPredictor.submit):
        assert "lens" not in inspect.signature(fn).parameters
    args = make_args()
    K = (41.3, 40.1, 18.2, 6.4)
    lm = LensMap.brown(K, (-0.2, 0.05, 0.0, 0.0), (13, 37), window_size=(8, 12), new_K=(30.0, 31.0, 5.5, 3.5))
    assert Predictor(None, args).ends.lens is None and Predictor(None, args, lens=lm).ends.lens is lm
    with pytest.raises(ValueError, match="crop"):
        Predictor(None, args, lens=lm, crop=(0, 0, 8, 12))
    with pytest.raises(TypeError):
        Predictor(None, args, lens=lm.map)
    # every frame has the map's source size
    pr = Predictor(None, args, lens=lm)
    with pytest.raises(ValueError, match="13 x 37"):
        pr(torch.zeros(1, 13, 36, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="13 x 37"):
        pr([torch.zeros(13, 37, 3, dtype=torch.uint8), torch.zeros(12, 37, 3, dtype=torch.uint8)])
    with pytest.raises(_lib.HipLibraryError):
        pr(torch.zeros(1, 13, 37, 3, dtype=torch.uint8))                         # the right size, on the host
    ends = pr.ends
    frames = [torch.zeros(2, 13, 37, 3, dtype=torch.uint8)]
    assert ends.window_of(frames) == (8, 12) and ends.model_size(frames) == (8, 12) and ends.origin_of(frames[0]) == (0, 0)
    assert predict._Ends(args, lens=lm, resize=(4, 6)).model_size(frames) == (4, 6)
    # ground truth: fp32 in the rectified window passes through; uint16 frames are refused, and the text says why
    gt = torch.ones(2, 1, 8, 12)
    assert ends.ground_truth(gt, 2) is not None
    with pytest.raises(ValueError, match="interpolated"):
        ends.ground_truth(torch.zeros(2, 13, 37, dtype=torch.uint16), 2)
    # intrinsics default to the map's new_K -- only for a keyword that reads them, and a call's own intrinsics win
    cpu = torch.device("cpu")
    assert ends.intrinsics_on(None, cpu, 2) is None and not Predictor(None, args).ends.has_default_K
    ends = predict._Ends(args, lens=lm, surface_normals={})
    k = ends.intrinsics_on(None, cpu, 2)
    assert ends.has_default_K and k.dtype == torch.float32 and torch.equal(k, torch.tensor([lm.new_K] * 2, dtype=torch.float32))
    own = torch.tensor([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]])
    assert torch.equal(ends.intrinsics_on(own, cpu, 2), own)
    assert predict._Ends(args, surface_normals={}).intrinsics_on(None, cpu, 2) is None
    bare = LensMap.identity((13, 37), 0, 0, (8, 12))                             # a map that was not told its camera
    assert predict._Ends(args, lens=bare, surface_normals={}).intrinsics_on(None, cpu, 2) is None
