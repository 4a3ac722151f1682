"""-m "not gpu": host side of the resize on ingest -- statement R (tests/resize_ref.py) against torch's CPU float64 antialiased
interpolation, ``hip_ops.resize_taps`` against R, the derived fp32 bar, the new entry points' declarations and argument checks, the
``resize`` keyword and the two helpers of objcavit_amd/predict.py.  No kernel runs."""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import resize_ref
from objcavit_amd import _lib, hip_ops
from objcavit_amd.config import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ocv_frame_resize_ingest", "ocv_frame_resize_supported")
PIN_SHAPES = [((375, 1242), (352, 1216)), ((481, 641), (480, 640)), ((37, 53), (16, 24)), ((9, 7), (16, 12)), ((100, 100), (7, 3))]
# window -> model size of every case tests/test_hip_resize_ingest.py runs on the GPU
GPU_SHAPES = [((31, 45), (16, 24)), ((31, 45), (15, 23)), ((9, 7), (16, 12)), ((40, 10), (16, 24)), ((33, 41), (32, 40)),
              ((128, 96), (16, 12)), ((96, 72), (16, 12)), ((61, 150), (20, 72)), ((61, 150), (21, 72))]


def _table():
    from objcavit_amd.predict import normalisation_table
    return normalisation_table(make_args())


@pytest.mark.parametrize("src,dst", PIN_SHAPES)
def test_statement_r_is_torchs_cpu_float64_antialiased_bilinear(src, dst):
    """The third-party pin: R's two matrices applied to random float64 input against ``F.interpolate(antialias=True)`` in float64."""
    x = torch.rand(2, 3, *src, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 5.0 - 2.5
    want = F.interpolate(x, size=dst, mode="bilinear", antialias=True, align_corners=False)
    got = resize_ref.matrix(src[0], dst[0]) @ x @ resize_ref.matrix(src[1], dst[1]).t()
    diff = float((got - want).abs().max())
    print(f"{src} -> {dst}: R against torch CPU float64 {diff:.3g}")
    assert diff < 1e-13


@pytest.mark.parametrize("n_in,n_out", [(375, 352), (481, 480), (1242, 1216), (641, 640), (53, 24), (37, 16), (7, 12), (9, 16), (100, 7),
                                        (100, 3), (96, 16), (128, 16), (150, 72), (1080, 480), (1920, 640), (5, 5), (1, 4), (4, 1)])
def test_resize_taps_are_statement_r_rounded_once(n_in, n_out):
    start, weight = hip_ops.resize_taps(n_in, n_out)
    rows = resize_ref.taps(n_in, n_out)
    K = max(len(w) for _, w in rows)
    assert start.dtype == torch.int32 and weight.dtype == torch.float32 and start.device.type == "cpu"
    assert tuple(start.shape) == (n_out,) and tuple(weight.shape) == (n_out, K)
    for i, (lo, w) in enumerate(rows):
        assert int(start[i]) == lo, i
        assert int((weight[i] != 0).nonzero().max()) < len(w)                    # no weight beyond the row's own taps
        assert torch.equal(weight[i, :len(w)], torch.tensor(w, dtype=torch.float64).to(torch.float32)), i
        assert not bool(weight[i, len(w):].any())
        assert lo >= 0 and lo + len(w) <= n_in                                   # the row's real taps lie inside the axis
    assert bool((start[1:] >= start[:-1]).all())                                # what the kernel's staging relies on


def test_identity_taps_are_exactly_one_and_zero():
    for n in (1, 5, 480):
        start, weight = hip_ops.resize_taps(n, n)
        assert start.tolist() == list(range(n))
        assert tuple(weight.shape) == (n, 2 if n > 1 else 1)
        assert bool((weight[:, 0] == 1.0).all()) and not bool(weight[:, 1:].any())
    with pytest.raises(ValueError):
        hip_ops.resize_taps(0, 4)


def _two_pass_fp32(vals, taps_y, taps_x):
    """fp32 values, fp32 weights rounded from float64, fp32 accumulation with one rounding per tap (fma), x pass then y pass, taps
    in ascending source index -- the kernel's arithmetic, restated with torch CPU ops."""
    (ys, yw), (xs, xw) = taps_y, taps_x
    B, C, Hw, Ww = vals.shape

    def apply(v, start, weight, n_in):                                           # along the last axis
        acc = torch.zeros(v.shape[:-1] + (start.numel(),), dtype=torch.float32)
        for k in range(weight.shape[1]):
            idx = (start.long() + k).clamp_(max=n_in - 1)
            acc = torch.addcmul(acc.double(), v[..., idx].double(), weight[:, k].double()).to(torch.float32)   # one rounding: an fma
        return acc

    mid = apply(vals, xs, xw, Ww)
    return apply(mid.transpose(2, 3), ys, yw, Hw).transpose(2, 3)


@pytest.mark.parametrize("src,dst", GPU_SHAPES)
def test_fp32_two_pass_emulation_stays_under_the_derived_bar(src, dst):
    table = _table()
    g = torch.Generator().manual_seed(17)
    frames = torch.randint(0, 256, (2, src[0], src[1], 3), dtype=torch.uint8, generator=g)
    ref = resize_ref.resized_input(frames, table, 0, 0, src[0], src[1], dst[0], dst[1])
    vals = torch.stack([table[c][frames[..., c].long()] for c in range(3)], 1)
    got = _two_pass_fp32(vals, hip_ops.resize_taps(src[0], dst[0]), hip_ops.resize_taps(src[1], dst[1]))
    bar = resize_ref.bar(src[0], src[1], dst[0], dst[1], table)
    diff = float((got.double() - ref).abs().max())
    print(f"{src} -> {dst}: fp32 two-pass against R {diff:.3g}, bar {bar:.3g} ({diff / bar:.2f} of it)")
    assert diff <= bar
    assert bar < 3e-5                                                            # a misplaced tap is worth 1e-4 or more


def test_supported_ratios():
    assert hip_ops.frame_resize_supported(96, 72, 16, 12)                        # ratio 6
    assert hip_ops.frame_resize_supported(2160, 3840, 480, 640)                  # 4.5 and 6
    assert hip_ops.frame_resize_supported(1080, 1920, 480, 640) and hip_ops.frame_resize_supported(375, 1242, 352, 1216)
    for Hw, Ww, H, W in [(9, 7, 16, 12), (1, 1, 480, 640), (3, 1000, 999, 1000), (480, 640, 480, 640)]:
        assert hip_ops.frame_resize_supported(Hw, Ww, H, W)                      # any enlargement, identity
    R = hip_ops.FRAME_RESIZE_MAX_RATIO
    assert R >= 6
    assert hip_ops.frame_resize_supported(R * 16, R * 12, 16, 12)
    assert not hip_ops.frame_resize_supported(R * 16 + 1, 12, 16, 12) and not hip_ops.frame_resize_supported(16, R * 12 + 1, 16, 12)


def test_wrapper_refuses_host_tensors_and_unsupported_ratios():
    frames = torch.zeros(1, 48, 64, 3, dtype=torch.uint8)
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.frame_resize_ingest(frames, torch.zeros(3, 256), (24, 32))
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.frame_resize_taps("cpu", 48, 64, 24, 32)
    R = hip_ops.FRAME_RESIZE_MAX_RATIO
    with pytest.raises(ValueError, match=str(R)):
        hip_ops.frame_resize_ingest(torch.zeros(1, R * 4 + 1, 64, 3, dtype=torch.uint8), torch.zeros(3, 256), (4, 32))
    with pytest.raises(ValueError):
        hip_ops.frame_resize_ingest(frames, torch.zeros(3, 256), (24, 32), top=40, window=(16, 16))      # window outside the frame
    params = inspect.signature(hip_ops.frame_resize_ingest).parameters
    assert list(params) == ["frames_u8", "table", "size", "top", "left", "window", "mirror_too", "out", "out_index", "taps"]
    assert hip_ops.frame_resize_ingest.__defaults__ == (0, 0, None, False, None, 0, None)
    from objcavit_amd.predict import Predictor
    with pytest.raises(_lib.HipLibraryError):
        Predictor(None, make_args(), resize=(24, 32))(frames)


def test_new_entry_points_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    declared = set(re.findall(r"\b(ocv_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and not name.endswith("_fwd"), name
    assert "OCV_FRAME_RESIZE_MAX_RATIO" in hdr and f"#define OCV_FRAME_RESIZE_MAX_RATIO {hip_ops.FRAME_RESIZE_MAX_RATIO}" in hdr
    from objcavit_amd import build
    assert "frame_resize.hip" in build.SOURCES
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.ocv_abi_version() == _lib.ABI_VERSION == 5                        # symbols are only added
    p = 4096                                                                     # any non-null, aligned address: it is never dereferenced

    def call(frames=p, fs=24 * 8, rs=24, Hs=8, Ws=8, top=0, left=0, Hw=8, Ww=8, table=p, ys=p, yw=p, Ky=3, xs=p, xw=p, Kx=3, out=p, B=1, H=4,
             W=4, mirror=0, off=0):
        return lib.ocv_frame_resize_ingest(frames, fs, rs, Hs, Ws, top, left, Hw, Ww, table, ys, yw, Ky, xs, xw, Kx, out, B, H, W, mirror,
                                           off, None)

    assert call(frames=None) == -1 and b"ocv_frame_resize_ingest: null pointer" in lib.ocv_last_error()
    assert call(xw=None) == -1 and b"null pointer" in lib.ocv_last_error()
    assert call(H=0) == -1 and b"bad sizes" in lib.ocv_last_error()
    assert call(top=1) == -1 and b"window outside the frame" in lib.ocv_last_error()
    assert call(left=2, Ww=7) == -1 and b"window outside the frame" in lib.ocv_last_error()
    assert call(rs=23) == -1 and b"strides" in lib.ocv_last_error()
    assert call(out=p + 2) == -1 and b"aligned" in lib.ocv_last_error()
    assert call(B=2, mirror=1, off=8) == -1 and b"mirror" in lib.ocv_last_error()
    assert call(Hs=64, fs=24 * 64, Hw=33) == -1                                  # 33 rows to 4: above the ratio
    assert b"OCV_FRAME_RESIZE_MAX_RATIO = 8" in lib.ocv_last_error()
    assert call(Ky=19) == -1 and b"OCV_FRAME_RESIZE_MAX_TAPS = 18" in lib.ocv_last_error()
    assert call(Kx=0) == -1


def test_constructors_take_resize_in_front_of_the_pinned_parameters():
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    for fn in (Predictor.__init__, PipelinedPredictor.__init__):
        params = inspect.signature(fn).parameters
        names = list(params)
        assert names[-3:] == ["object_metrics", "point_cloud", "object_depth"]
        assert names[-5:-3] == ["crop", "resize"] and params["resize"].default is None
    for fn in (Predictor.__call__, PipelinedPredictor.submit):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["intrinsics", "boxes"] and "resize" not in params
    with pytest.raises(ValueError):
        Predictor(None, make_args(), resize=(0, 32))


def test_fit_window():
    from objcavit_amd.predict import fit_window
    assert fit_window(1080, 1920, 480, 640) == (0, 240, 1080, 1440)              # 16:9 to 4:3: full height, 1080 * 640 / 480 columns
    assert fit_window(720, 1280, 480, 640) == (0, 160, 720, 960)
    assert fit_window(480, 640, 480, 640) == (0, 0, 480, 640)
    assert fit_window(250, 300, 192, 208) == (0, 15, 250, 270)                   # 250 * 208 / 192 = 270.83 -> 270, margin 30
    assert fit_window(375, 1242, 480, 640) == (0, 371, 375, 500)
    assert fit_window(640, 480, 480, 640) == (140, 0, 360, 480)                  # a portrait frame: full width, 480 * 480 / 640 rows
    assert fit_window(101, 50, 10, 10) == (25, 0, 50, 50)                        # margin 51: the odd pixel stays at the bottom
    assert fit_window(1, 1000, 480, 640) == (0, 499, 1, 1)                       # never below one pixel
    with pytest.raises(ValueError):
        fit_window(0, 10, 4, 4)


def test_boxes_to_model():
    from objcavit_amd.predict import boxes_to_model
    b = torch.tensor([[135.0, 125.0, 27.0, 50.0, 0.9], [-1.0, -1.0, -1.0, -1.0, 0.0], [-1.0, 5.0, -1.0, -1.0, 1.0]])
    got = boxes_to_model(b, (250, 270), (125, 540))                              # x doubles, y halves
    assert torch.equal(got, torch.tensor([[270.0, 62.5, 54.0, 25.0, 0.9], [-1.0, -1.0, -1.0, -1.0, 0.0], [-2.0, 2.5, -2.0, -0.5, 1.0]]))
    assert got is not b and float(b[0, 0]) == 135.0
    batch = boxes_to_model(b.view(1, 3, 5).expand(2, 3, 5), (250, 270), (125, 540))
    assert tuple(batch.shape) == (2, 3, 5) and torch.equal(batch[1], got)
    lst = boxes_to_model([b[:1, :4], None, b[1:2]], (250, 270), (125, 540))
    assert lst[1] is None and torch.equal(lst[0], got[:1, :4]) and torch.equal(lst[2], b[1:2])
    assert boxes_to_model(None, (1, 1), (2, 2)) is None
    with pytest.raises(ValueError):
        boxes_to_model(torch.zeros(2, 3), (1, 1), (2, 2))
