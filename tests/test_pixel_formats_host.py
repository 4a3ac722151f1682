"""-m "not gpu": host side of the pixel formats on ingest -- ``pixel_formats.yuv_tables`` against Statement P (tests/pixel_format_ref.py),
Statement P against the float64 real-coefficient formula over all 2^24 (Y, Cb, Cr) triples and against PIL, ``PlanarFrames``, the new
entry points' declarations and argument checks, the ``pixel_format`` keyword.  No kernel runs."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pixel_format_ref as ref
from objcavit_amd import _lib, hip_ops
from objcavit_amd.config import make_args
from objcavit_amd.pixel_formats import FORMAT_IDS, PixelFormat, PlanarFrames, yuv_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ocv_frame_ingest_format", "ocv_frame_resize_ingest_format", "ocv_frames_to_rgb24")
VARIANTS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]


@pytest.mark.parametrize("matrix,range_", VARIANTS)
def test_yuv_tables_are_statement_p(matrix, range_):
    t = yuv_tables(matrix, range_)
    assert t.dtype == torch.int32 and tuple(t.shape) == (5, 256) and t.device.type == "cpu"
    want = ref.tables(matrix, range_)
    assert np.array_equal(t.numpy().astype(np.int64), want)
    # every sum of the statement fits int32 sixty times over (the largest, 3.51e7, is T0[255] + T4[255] of bt601 limited)
    big = max(abs(int(want[0].max()) + int(want[i].max())) for i in (1, 4))
    big = max(big, abs(int(want[0].min()) + int(want[1].min())), abs(int(want[0].min()) + int(want[4].min())),
              abs(int(want[0].max()) + int(want[2].max()) + int(want[3].max())), abs(int(want[0].min()) + int(want[2].min()) + int(want[3].min())))
    print(f"{matrix} {range_}: largest |sum| {big}")
    assert big < 2 ** 31 // 32
    with pytest.raises(ValueError):
        yuv_tables("bt2020", range_)
    with pytest.raises(ValueError):
        yuv_tables(matrix, "tv")


@pytest.mark.parametrize("matrix,range_", VARIANTS)
def test_statement_p_against_the_float64_formula_on_all_triples(matrix, range_):
    """R and B identical to clamp(floor(x + 0.5)) of the real-coefficient formula everywhere; G within 1 LSB, different on fewer than
    256 of the 2^24 triples."""
    v = np.arange(256)
    y2, c2 = np.meshgrid(v, v, indexing="ij")
    # R depends on (Y, Cr) alone, B on (Y, Cb) alone: 2^16 pairs each cover all triples
    p = ref.ycbcr_to_rgb(y2, c2, c2, matrix, range_)
    q = ref.real_rgb(y2, c2, c2, matrix, range_)
    assert np.array_equal(p[..., 0], q[..., 0]) and np.array_equal(p[..., 2], q[..., 2])
    cb, cr = np.meshgrid(v, v, indexing="ij")
    differ, worst = 0, 0
    for y in range(256):
        yy = np.full_like(cb, y)
        d = np.abs(ref.ycbcr_to_rgb(yy, cb, cr, matrix, range_)[..., 1].astype(np.int64) - ref.real_rgb(yy, cb, cr, matrix, range_)[..., 1])
        differ += int((d != 0).sum())
        worst = max(worst, int(d.max()))
    print(f"{matrix} {range_}: G differs on {differ} of 2^24 triples, by at most {worst}")
    assert worst <= 1 and differ < 256


def test_bt601_full_range_is_within_one_lsb_of_pil():
    Image = pytest.importorskip("PIL.Image", reason="PIL is not installed: no third-party YCbCr -> RGB to compare with")
    v = np.arange(256, dtype=np.uint8)
    cb, cr = np.meshgrid(v, v, indexing="ij")
    worst = 0
    for y0 in range(0, 256, 16):                                       # 16 Y values per image: 16 x 65536 triples, all 2^24 in 16 images
        y = np.repeat(np.arange(y0, y0 + 16, dtype=np.uint8), 65536).reshape(16 * 256, 256)
        ycc = np.stack([y, np.tile(cb, (16, 1)), np.tile(cr, (16, 1))], -1)
        pil = np.asarray(Image.frombytes("YCbCr", (256, 16 * 256), np.ascontiguousarray(ycc).tobytes()).convert("RGB")).astype(np.int64)
        ours = ref.ycbcr_to_rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2], "bt601", "full").astype(np.int64)
        worst = max(worst, int(np.abs(pil - ours).max()))
    print(f"bt601 full against PIL: at most {worst} LSB")
    assert worst <= 1


def test_pixel_format():
    f = PixelFormat("nv12", "bt709", "full")
    assert (f.name, f.matrix, f.range, f.id, f.planar, f.channels) == ("nv12", "bt709", "full", 4, True, 0)
    assert PixelFormat("i420") == PixelFormat("i420", "bt601", "limited") and PixelFormat("i420") != f
    assert PixelFormat("bgr24", "bt709") == PixelFormat("bgr24") and hash(PixelFormat("bgr24", "bt709")) == hash(PixelFormat("bgr24"))
    assert PixelFormat.of(None) == PixelFormat("rgb24") and PixelFormat.of("bgra32").channels == 4 and PixelFormat.of(f) is f
    assert torch.equal(f.tables(), yuv_tables("bt709", "full"))
    assert FORMAT_IDS == {"rgb24": 0, "bgr24": 1, "rgba32": 2, "bgra32": 3, "nv12": 4, "i420": 5}
    hdr = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    for name, i in FORMAT_IDS.items():
        assert f"#define OCV_PIXFMT_{name.upper()} {i}" in hdr
    for bad in (("yuyv",), ("nv12", "bt2020"), ("nv12", "bt601", "pc")):
        with pytest.raises(ValueError):
            PixelFormat(*bad)


def test_planar_frames_from_buffer_views_and_strides():
    B, Hs, Ws = 2, 6, 8
    buf = torch.arange(B * Hs * 3 // 2 * Ws, dtype=torch.int64).remainder(251).to(torch.uint8).view(B, Hs * 3 // 2, Ws)
    flat = buf.view(B, -1)
    nv = PlanarFrames.from_buffer(buf, "nv12", Hs, Ws)
    assert nv.shape == (B, Hs, Ws) and nv.device == buf.device and len(nv) == B and len(nv.planes) == 2
    y, c = nv.planes
    assert tuple(y.shape) == (B, Hs, Ws) and tuple(c.shape) == (B, 3, 4, 2)
    assert y.data_ptr() == buf.data_ptr() and c.data_ptr() == buf.data_ptr() + Hs * Ws                   # views, nothing copied
    assert y.stride() == (Hs * 3 // 2 * Ws, Ws, 1) and c.stride() == (Hs * 3 // 2 * Ws, Ws, 2, 1)
    assert torch.equal(y.reshape(B, -1), flat[:, :Hs * Ws]) and torch.equal(c.reshape(B, -1), flat[:, Hs * Ws:])
    i4 = PlanarFrames.from_buffer(buf, "i420", Hs, Ws)
    _, cb, cr = i4.planes
    assert tuple(cb.shape) == tuple(cr.shape) == (B, 3, 4) and cb.stride() == (Hs * 3 // 2 * Ws, 4, 1)
    assert torch.equal(cb.reshape(B, -1), flat[:, Hs * Ws:Hs * Ws + 12]) and torch.equal(cr.reshape(B, -1), flat[:, Hs * Ws + 12:])
    one = PlanarFrames.from_buffer(buf[1], "nv12", Hs, Ws)                                                # a single frame
    assert one.shape == (1, Hs, Ws) and torch.equal(one.planes[1], c[1:2])
    assert nv[1].shape == (1, Hs, Ws) and torch.equal(nv[1].planes[0], y[1:2]) and nv[0:2].shape == (B, Hs, Ws)
    with pytest.raises(ValueError):
        PlanarFrames.from_buffer(buf, "nv12", 5, 8)                                                       # odd: explicit planes
    with pytest.raises(ValueError):
        PlanarFrames.from_buffer(buf[:, :8], "nv12", Hs, Ws)
    with pytest.raises(ValueError):
        PlanarFrames.from_buffer(buf, "rgb24", Hs, Ws)


def test_planar_frames_odd_sizes_and_refusals():
    B, Hs, Ws = 2, 9, 13                                                                                  # 5 x 7 chroma samples
    y = torch.zeros(B, Hs, Ws, dtype=torch.uint8)
    nv = PlanarFrames("nv12", (y, torch.zeros(B, 5, 7, 2, dtype=torch.uint8)), Hs, Ws)
    assert nv.shape == (B, Hs, Ws)
    big = torch.zeros(B, 40, 64, dtype=torch.uint8)                                                       # strided views into one allocation
    i4 = PlanarFrames("i420", (big[:, :9, 3:16], big[:, 10:15, 1:8], big[:, 20:25, 9:16]), Hs, Ws)
    assert i4.planes[1].stride() == (40 * 64, 64, 1) and not i4.planes[0].is_contiguous()
    assert PlanarFrames("i420", (y[0], torch.zeros(5, 7, dtype=torch.uint8), torch.zeros(5, 7, dtype=torch.uint8)), Hs, Ws).shape == (1, Hs, Ws)
    with pytest.raises(ValueError, match="planes"):
        PlanarFrames("nv12", (y,), Hs, Ws)                                                                # wrong plane count
    with pytest.raises(ValueError, match="planes"):
        PlanarFrames("i420", (y, torch.zeros(B, 5, 7, 2, dtype=torch.uint8)), Hs, Ws)
    with pytest.raises(ValueError, match="at least"):
        PlanarFrames("nv12", (y, torch.zeros(B, 4, 7, 2, dtype=torch.uint8)), Hs, Ws)                     # chroma plane too small: floor, not ceil
    with pytest.raises(ValueError, match="at least"):
        PlanarFrames("i420", (y, torch.zeros(B, 5, 7, dtype=torch.uint8), torch.zeros(B, 5, 6, dtype=torch.uint8)), Hs, Ws)
    with pytest.raises(ValueError, match="is on"):
        PlanarFrames("nv12", (y, torch.zeros(B, 5, 7, 2, dtype=torch.uint8, device="meta")), Hs, Ws)      # mixed devices
    with pytest.raises(ValueError):
        PlanarFrames("nv12", (y, torch.zeros(B, 5, 14, 2, dtype=torch.uint8)[:, :, ::2]), Hs, Ws)         # samples of a row not dense
    with pytest.raises(TypeError):
        PlanarFrames("nv12", (y.float(), torch.zeros(B, 5, 7, 2, dtype=torch.uint8)), Hs, Ws)
    with pytest.raises(ValueError):
        PlanarFrames("rgb24", (y,), Hs, Ws)


def test_new_entry_points_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    declared = set(re.findall(r"\b(ocv_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and not name.endswith("_fwd"), name
    for name in ("frame_ingest_format", "frame_resize_ingest_format", "frames_to_rgb24"):
        assert callable(getattr(hip_ops, name))
    from objcavit_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.ocv_abi_version() == _lib.ABI_VERSION == 5                        # symbols are only added
    p = 4096                                                                     # any non-null, aligned address: it is never dereferenced
    Hs, Ws, B = 9, 13, 2                                                         # 5 x 7 chroma samples
    # the planes of each format at their smallest strides: (pointer, frame stride, row stride) x 3
    dense = {0: [p, Hs * Ws * 3, Ws * 3, None, 0, 0, None, 0, 0], 1: [p, Hs * Ws * 3, Ws * 3, None, 0, 0, None, 0, 0],
             2: [p, Hs * Ws * 4, Ws * 4, None, 0, 0, None, 0, 0], 3: [p, Hs * Ws * 4, Ws * 4, None, 0, 0, None, 0, 0],
             4: [p, Hs * Ws, Ws, p, 5 * 14, 14, None, 0, 0], 5: [p, Hs * Ws, Ws, p, 35, 7, p, 35, 7]}

    def ingest(fmt=4, planes=None, yuv=p, Hs=Hs, Ws=Ws, top=1, left=1, table=p, out=p, B=B, H=6, W=8, mirror=0, off=0, **edit):
        pl = list(dense.get(fmt, dense[5]) if planes is None else planes)
        for i, v in edit.items():
            pl[int(i[1:])] = v
        return lib.ocv_frame_ingest_format(fmt, *pl, yuv, Hs, Ws, top, left, table, out, B, H, W, mirror, off, None)

    def resize(fmt=4, yuv=p, Hs=Hs, Ws=Ws, top=1, left=1, Hw=6, Ww=8, table=p, ys=p, yw=p, Ky=3, xs=p, xw=p, Kx=3, out=p, B=B, H=4, W=4,
               mirror=0, off=0, **edit):
        pl = list(dense.get(fmt, dense[5]))
        for i, v in edit.items():
            pl[int(i[1:])] = v
        return lib.ocv_frame_resize_ingest_format(fmt, *pl, yuv, Hs, Ws, top, left, Hw, Ww, table, ys, yw, Ky, xs, xw, Kx, out, B, H, W,
                                                  mirror, off, None)

    def to_rgb(fmt=4, yuv=p, Hs=Hs, Ws=Ws, top=1, left=1, out=p, B=B, Hw=6, Ww=8, **edit):
        pl = list(dense.get(fmt, dense[5]))
        for i, v in edit.items():
            pl[int(i[1:])] = v
        return lib.ocv_frames_to_rgb24(fmt, *pl, yuv, Hs, Ws, top, left, out, B, Hw, Ww, None)

    for call, who in ((ingest, b"ocv_frame_ingest_format"), (resize, b"ocv_frame_resize_ingest_format"), (to_rgb, b"ocv_frames_to_rgb24")):
        def refused(what, **kw):
            assert call(**kw) == -1, (who, kw)
            msg = lib.ocv_last_error()
            assert msg.startswith(who + b":") and what in msg, (who, kw, msg)

        refused(b"null pointer", a0=None)                                        # the plane every format has
        refused(b"null pointer", fmt=4, a3=None)                                 # nv12's CbCr plane
        refused(b"null pointer", fmt=5, a6=None)                                 # i420's Cr plane
        refused(b"null pointer", out=None)
        refused(b"unknown pixel format", fmt=6)
        refused(b"unknown pixel format", fmt=-1)
        refused(b"bad sizes", B=0)
        refused(b"bad sizes", Hs=0)
        refused(b"outside the frame", top=4)                                     # 4 + 6 > 9 rows
        refused(b"outside the frame", left=6)
        refused(b"outside the frame", top=-1)
        refused(b"strides", fmt=4, a2=Ws - 1)                                    # Y row
        refused(b"strides", fmt=4, a1=Hs * Ws - 1)                               # Y frame
        refused(b"strides", fmt=4, a5=13)                                        # nv12 chroma rows: 2 * ceil(13 / 2) = 14 bytes
        refused(b"strides", fmt=4, a4=4 * 14 + 13)
        refused(b"strides", fmt=5, a5=6)                                         # i420 chroma rows: 7 bytes
        refused(b"strides", fmt=5, a8=6)
        refused(b"strides", fmt=5, a7=4 * 7 + 6)
        refused(b"strides", fmt=1, a2=Ws * 3 - 1)
        refused(b"strides", fmt=3, a2=Ws * 4 - 1)                                # 4 * Ws for the 32-bit formats
        refused(b"strides", fmt=2, a1=Hs * Ws * 4 - 1)
        refused(b"yuv_table", fmt=4, yuv=None)
        refused(b"yuv_table", fmt=5, yuv=p + 2)
        for fmt in range(4):
            assert call(fmt=fmt, yuv=None, B=0) == -1 and b"bad sizes" in lib.ocv_last_error()      # packed: no tables asked for
    # the rgb24 entry points' own checks
    assert ingest(H=0) == -1 and b"bad sizes" in lib.ocv_last_error()
    assert ingest(table=None) == -1 and b"null pointer" in lib.ocv_last_error()
    assert ingest(out=p + 2) == -1 and b"aligned" in lib.ocv_last_error()
    assert ingest(mirror=1, off=8) == -1 and b"mirror" in lib.ocv_last_error()
    assert resize(xw=None) == -1 and b"null pointer" in lib.ocv_last_error()
    assert resize(out=p + 2) == -1 and b"aligned" in lib.ocv_last_error()
    assert resize(mirror=1, off=8) == -1 and b"mirror" in lib.ocv_last_error()
    assert resize(Hs=64, a1=64 * Ws, a4=32 * 14, Hw=33) == -1 and b"OCV_FRAME_RESIZE_MAX_RATIO = 8" in lib.ocv_last_error()
    assert resize(Ky=19) == -1 and b"OCV_FRAME_RESIZE_MAX_TAPS = 18" in lib.ocv_last_error()
    assert resize(Kx=0) == -1
    assert to_rgb(Hw=0) == -1 and b"bad sizes" in lib.ocv_last_error()


def test_constructors_take_pixel_format_in_front_of_crop():
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    for fn in (Predictor.__init__, PipelinedPredictor.__init__):
        params = inspect.signature(fn).parameters
        names = list(params)
        assert names[-5:] == ["crop", "resize", "object_metrics", "point_cloud", "object_depth"]        # pinned by earlier tests
        assert names[-6] == "pixel_format" and params["pixel_format"].default is None
    for fn in (Predictor.__call__, PipelinedPredictor.submit):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["intrinsics", "boxes"] and "pixel_format" not in params
    import objcavit_amd.predict as predict
    assert predict.PixelFormat is PixelFormat and predict.PlanarFrames is PlanarFrames                   # exported beside fit_window
    assert Predictor(None, make_args(), pixel_format="nv12").ends.fmt == PixelFormat("nv12")
    assert Predictor(None, make_args()).ends.fmt is None
    with pytest.raises(ValueError):
        Predictor(None, make_args(), pixel_format="yuyv")
    # the signatures the earlier tests pin are what they were
    assert list(inspect.signature(hip_ops.frame_ingest).parameters) == ["frames_u8", "table", "top", "left", "size", "mirror_too", "out", "out_index"]
    assert "pixel_format" in inspect.signature(hip_ops.frame_ingest_format).parameters
    assert "pixel_format" in inspect.signature(hip_ops.frame_resize_ingest_format).parameters


def test_wrappers_and_predictors_refuse_host_tensors():
    table = torch.zeros(3, 256)
    nv = PlanarFrames.from_buffer(torch.zeros(1, 12, 8, dtype=torch.uint8), "nv12", 8, 8)
    bgra = torch.zeros(1, 8, 8, 4, dtype=torch.uint8)
    for frames, fmt in ((nv, "nv12"), (bgra, "bgra32"), (bgra[..., :3], "bgr24")):
        with pytest.raises(_lib.HipLibraryError):
            hip_ops.frame_ingest_format(frames, table, fmt)
        with pytest.raises(_lib.HipLibraryError):
            hip_ops.frame_resize_ingest_format(frames, table, (4, 4), fmt)
        with pytest.raises(_lib.HipLibraryError):
            hip_ops.frames_to_rgb24(frames, fmt)
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.frame_yuv_tables("cpu", "nv12")
    with pytest.raises(TypeError):
        hip_ops.frames_to_rgb24(bgra, "nv12")                                    # a tensor where planes are needed
    from objcavit_amd.predict import Predictor
    with pytest.raises(_lib.HipLibraryError):
        Predictor(None, make_args(), pixel_format=PixelFormat("nv12", "bt709"))(nv)
    with pytest.raises(_lib.HipLibraryError):
        Predictor(None, make_args(), pixel_format="bgra32", resize=(4, 4))(bgra)
    with pytest.raises(ValueError):
        Predictor(None, make_args(), pixel_format="bgra32")(bgra[..., :3])       # 3 bytes per pixel for a 32-bit format
    with pytest.raises(ValueError):
        Predictor(None, make_args(), pixel_format="nv12")(bgra)
