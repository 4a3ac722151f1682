"""-m gpu: the lens on ingest -- csrc/frame_remap.hip through its two entry points against Statement L (tests/lens_ref.py, numpy
integers) BYTE FOR BYTE with the same map tensor as input, in all six pixel formats, its guarded runs (a row of
tests/test_hip_memory_bounds.py's table), inside a captured graph and through both predictors (child processes).  Source frames are
13 x 37 (odd: the 4:2:0 chroma planes are 7 x 19) and every plane is a strided view -- padded rows, padded frames, a base pointer at
an odd byte -- as in tests/test_hip_pixel_formats.py; the windows are 11 x 30 (the scalar form) and 12 x 32 (the VEC form)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lens_ref as ref
import pixel_format_ref
import test_hip_memory_bounds as bounds
from objcavit_amd.config import make_args
from objcavit_amd.lens import LensMap
from objcavit_amd.pixel_formats import PixelFormat, PlanarFrames, chroma_size
from test_hip_pixel_formats import _strided

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
B, HS, WS = 3, 13, 37
SCALAR, VEC = (11, 30), (12, 32)
FORMATS = [PixelFormat("rgb24"), PixelFormat("bgr24"), PixelFormat("rgba32"), PixelFormat("bgra32"), PixelFormat("nv12"),
           PixelFormat("i420", "bt709", "full")]
POISON = 0x7FC0DEAD
_MADE = {}


def _id(fmt):
    return fmt.name


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def _table():
    if "table" not in _MADE:
        from objcavit_amd.predict import normalisation_table
        _MADE["table"] = normalisation_table(make_args())
    return _MADE["table"]


def host_planes(name, n, Hs, Ws, seed):
    """The planes of ``n`` random frames on the host, every byte value present in every plane that is large enough."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        k = int(np.prod(shape))
        return (torch.arange(k) % 256)[torch.randperm(k, generator=g)].to(torch.uint8).view(*shape)

    Hc, Wc = chroma_size(Hs, Ws)
    if name == "nv12":
        return [rnd(n, Hs, Ws), rnd(n, Hc, Wc, 2)]
    if name == "i420":
        return [rnd(n, Hs, Ws), rnd(n, Hc, Wc), rnd(n, Hc, Wc)]
    return [rnd(n, Hs, Ws, 4 if name.endswith("32") else 3)]


def on_device(fmt, planes, Hs, Ws, strided=True):
    dev = [_strided(p, k) if strided else p.cuda() for k, p in enumerate(planes)]
    return PlanarFrames(fmt.name, dev, Hs, Ws) if fmt.planar else dev[0]


def source(fmt):
    """(host planes, strided device frames, the format's own R, G, B of the whole frames uint8 [B, HS, WS, 3]): made once per format."""
    if fmt.name not in _MADE:
        planes = host_planes(fmt.name, B, HS, WS, 500 + len(fmt.name) + fmt.id)
        rgb = pixel_format_ref.rgb_of(planes if fmt.planar else planes[0], fmt, 0, 0, HS, WS)
        _MADE[fmt.name] = (planes, on_device(fmt, planes, HS, WS), rgb)
    return _MADE[fmt.name]


# --------------------------------------------------------------------------- the maps
def barrel(window):
    """A strong barrel seen through a short focal length: the window looks past the frame on every side."""
    Hw, Ww = window
    return LensMap.brown((30.0, 29.0, 18.3, 6.1), (-0.38, 0.11, 0.002, -0.001, -0.012), (HS, WS), window_size=window,
                         new_K=(11.0, 10.5, (Ww - 1) / 2 + 0.3, (Hw - 1) / 2 - 0.2))


def _axis(n_out, n_src):
    """n_out source coordinates that walk from outside the frame to outside the frame, in exact multiples of 1/256: both sentinels, the
    last sub-pixel before the frame, weights 0 and 255, odd and even x0, the last pixel exactly and one step beyond."""
    u = 1.0 / 256
    head = [-3.0, -1.0, -1.0 + u, -u, 0.0, 255 * u, 1.0, 1.5, 2.0 + 77 * u, 3.0, 4.0 + 255 * u]
    tail = [n_src - 2.0, n_src - 2 + 255 * u, n_src - 1.0, n_src - 1 + u, n_src - 1 + 128 * u, float(n_src), n_src + 2.0]
    k = n_out - len(head) - len(tail)
    assert k >= 2
    mid = [round((5.0 + (n_src - 7.5) * i / (k - 1)) * 256) / 256 for i in range(k)]
    return torch.tensor(head + mid + tail, dtype=torch.float64)


def _axis_short(n_out, n_src):
    """The same walk for the 11 or 12 rows of the windows: the special values alone."""
    u = 1.0 / 256
    vals = [-3.0, -u, 0.0, 255 * u, 3.0 + 99 * u, 6.5, n_src - 2 + 255 * u, n_src - 1.0, n_src - 1 + u, float(n_src), n_src + 2.0]
    assert n_out >= len(vals)
    vals = vals[:6] + [7.0 + 30 * u] * (n_out - len(vals)) + vals[6:]
    return torch.tensor(vals, dtype=torch.float64)


def shifted(window):
    """A map shifted off the frame: the window's columns and rows walk across the whole frame and out on both sides."""
    Hw, Ww = window
    xs, ys = _axis(Ww, WS), _axis_short(Hw, HS)
    return LensMap.from_coordinates(xs.view(1, Ww).expand(Hw, Ww), ys.view(Hw, 1).expand(Hw, Ww), (HS, WS), new_K=(20.0, 20.0, 15.0, 6.0))


def fisheye(window):
    Hw, Ww = window
    return LensMap.fisheye((14.0, 14.0, 18.0, 6.0), (-0.03, 0.005, -0.0008, 0.00005), (HS, WS), window_size=window,
                           new_K=(7.0, 7.0, (Ww - 1) / 2, (Hw - 1) / 2))


def maps(window):
    """name -> LensMap: the two single maps and the three-map batch (M = B = 3: barrel, shifted, fisheye)."""
    key = ("maps", window)
    if key not in _MADE:
        a, b, c = barrel(window), shifted(window), fisheye(window)
        _MADE[key] = {"barrel": a, "shifted": b, "three": LensMap(torch.cat([a.map, b.map, c.map], 0), (HS, WS))}
    return _MADE[key]


def want_rgb(fmt, window, name):
    """The statement's rectified bytes uint8 [B, Hw, Ww, 3] (numpy) of a format's frames through a map: computed once, shared."""
    key = ("rgb", fmt.name, window, name)
    if key not in _MADE:
        _MADE[key] = ref.remap_rgb(source(fmt)[2], maps(window)[name].map.numpy())
    return _MADE[key]


@pytest.mark.parametrize("window", [SCALAR, VEC], ids=["11x30", "12x32"])
def test_the_maps_hold_every_case_the_kernel_can_meet(window):
    """Asserted on the maps themselves: together the barrel and the shifted map contain taps outside on each side and at a corner,
    pixels with one, two, four and no taps inside (THREE cannot occur: the taps form an axis-aligned 2 x 2 square, the frame is a
    rectangle, so the count is a product of two numbers out of 0, 1, 2), weights 0 and 255 along both axes, coordinates exactly on the
    last row / column (x0 = Ws - 1: the second tap is outside), both sentinels, and for 4:2:0 odd and even x0 with both taps inside."""
    m = torch.cat([maps(window)["barrel"].map, maps(window)["shifted"].map], 0).numpy().astype(np.int64)
    X, Y = m[..., 0], m[..., 1]
    x0, wx, y0, wy = X >> 8, X & 255, Y >> 8, Y & 255
    x_in, y_in = (x0 >= 0) & (x0 + 1 < WS), (y0 >= 0) & (y0 + 1 < HS)
    assert bool(((x0 < 0) & (x0 + 1 >= 0) & y_in).any()) and bool(((x0 + 1 >= WS) & (x0 < WS) & y_in).any())      # left, right
    assert bool(((y0 < 0) & (y0 + 1 >= 0) & x_in).any()) and bool(((y0 + 1 >= HS) & (y0 < HS) & x_in).any())      # top, bottom
    assert bool(((x0 == -1) & (y0 == -1)).any()) and bool(((x0 == WS - 1) & (y0 == HS - 1)).any())               # corners: one tap inside
    count = ref.taps_inside(m, HS, WS)
    assert set(count.ravel().tolist()) == {0, 1, 2, 4}
    for w in (wx, wy):
        assert bool((w == 0).any()) and bool((w == 255).any())
    assert bool(((X == (WS - 1) * 256) & y_in).any()) and bool(((Y == (HS - 1) * 256) & x_in).any())
    assert bool((X == -256).any()) and bool((X == WS * 256).any()) and bool((Y == -256).any()) and bool((Y == HS * 256).any())
    assert bool((x_in & y_in & (x0 % 2 == 1)).any()) and bool((x_in & y_in & (x0 % 2 == 0)).any())
    # the barrel alone looks past every side of the frame, and is valid in its middle
    bar = maps(window)["barrel"]
    v = bar.valid[0]
    assert bool(v.any()) and not bool(v[0].any()) and not bool(v[-1].any()) and not bool(v[:, 0].any()) and not bool(v[:, -1].any())
    # the shifted map touches the first and the last byte of every plane (the guarded row relies on it)
    sh = maps(window)["shifted"].map[0].numpy().astype(np.int64)
    assert bool(((sh[..., 0] >> 8 == 0) & (sh[..., 1] >> 8 == 0)).any()) and bool(((sh[..., 0] >> 8 == WS - 2) & (sh[..., 1] >> 8 == HS - 2)).any())


# --------------------------------------------------------------------------- the two launches against the statement
@pytest.mark.parametrize("fmt", FORMATS, ids=_id)
def test_rgb24_launch_is_statement_l_byte_for_byte(ops, fmt):
    _, frames, _ = source(fmt)
    for window in (SCALAR, VEC):
        for name, lm in maps(window).items():
            want = torch.from_numpy(want_rgb(fmt, window, name))
            got = ops.frames_remap_rgb24(frames, lm, fmt)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (B,) + window + (3,) and got.is_contiguous()
            assert torch.equal(got.cpu(), want), (fmt.name, window, name, int((got.cpu() != want).sum()))
            # the same map as a device tensor, into out= over another fill: every byte is written
            out = torch.full_like(got, 0x5A)
            assert ops.frames_remap_rgb24(frames, lm.on("cuda"), fmt, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError):
        ops.frames_remap_rgb24(frames[0] if fmt.planar else frames[:1], maps(VEC)["three"], fmt)      # three maps, one frame
    with pytest.raises(ValueError):
        ops.frames_remap_rgb24(frames, LensMap.identity((HS, WS + 1)), fmt)                          # a map made for another size


@pytest.mark.parametrize("fmt", FORMATS, ids=_id)
def test_fused_launch_is_statement_l_byte_for_byte(ops, fmt):
    """With and without the mirror, scalar and VEC form, M = 1 and M = 3; equal to ``frame_ingest`` of the rgb24 launch's bytes; two
    calls give equal bytes."""
    _, frames, _ = source(fmt)
    table = _table().cuda()
    for window in (SCALAR, VEC):
        Hw, Ww = window
        for name, lm in maps(window).items():
            rect = want_rgb(fmt, window, name)
            for mirror in (False, True):
                want = torch.from_numpy(ref.ingest(rect, _table().numpy(), mirror))
                out = torch.full((2 * B if mirror else B, 3, Hw, Ww), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
                got = ops.frame_remap_ingest(frames, table, lm, fmt, mirror_too=mirror, out=out)
                assert got is out and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (fmt.name, window, name, mirror)
                again = ops.frame_remap_ingest(frames, table, lm, fmt, mirror_too=mirror)
                assert torch.equal(again.view(torch.int32), got.view(torch.int32))
                two = ops.frame_ingest(ops.frames_remap_rgb24(frames, lm, fmt), table, mirror_too=mirror)
                assert torch.equal(two.view(torch.int32), got.view(torch.int32)), (fmt.name, window, name, mirror)


@pytest.mark.parametrize("fmt", [FORMATS[0], FORMATS[4]], ids=_id)
def test_out_index_fills_a_larger_batch(ops, fmt):
    """``out=`` a batch of four (eight with the mirrors) at ``out_index = 1``: the three images land behind image 0, their mirrors behind
    image 4; the rest stays what it was.  The VEC window keeps its 16-byte stores (an image is a multiple of 16 bytes)."""
    _, frames, _ = source(fmt)
    table = _table().cuda()
    for window in (SCALAR, VEC):
        Hw, Ww = window
        lm = maps(window)["three"]
        want = torch.from_numpy(ref.ingest(want_rgb(fmt, window, "three"), _table().numpy(), True))
        out = torch.full((8, 3, Hw, Ww), float("nan"), device="cuda")
        assert ops.frame_remap_ingest(frames, table, lm, fmt, mirror_too=True, out=out, out_index=1) is out
        assert torch.equal(out[1:4].cpu(), want[:B]) and torch.equal(out[5:8].cpu(), want[B:]) and bool(torch.isnan(out[[0, 4]]).all())
        one = torch.full((4, 3, Hw, Ww), float("nan"), device="cuda")
        ops.frame_remap_ingest(frames, table, lm, fmt, out=one, out_index=1)
        assert torch.equal(one[1:].cpu(), want[:B]) and bool(torch.isnan(one[0]).all())
        with pytest.raises(ValueError):
            ops.frame_remap_ingest(frames, table, lm, fmt, mirror_too=True, out=out, out_index=2)
        with pytest.raises(ValueError):
            ops.frame_remap_ingest(frames, table, lm, fmt, out=torch.empty(4, 3, Hw + 1, Ww, device="cuda"))


@pytest.mark.parametrize("fmt", FORMATS, ids=_id)
def test_identity_map_equals_the_plain_ingest(ops, fmt):
    """X = 256 (left + u), Y = 256 (top + v): bit-equal to ``frame_ingest`` / ``frame_ingest_format`` at (top, left)."""
    _, frames, rgb = source(fmt)
    table = _table().cuda()
    for (top, left), window in (((1, 3), SCALAR), ((0, 4), VEC), ((1, 5), VEC)):       # (1, 5) + (12, 32) ends on the last row and column
        lm = LensMap.identity((HS, WS), top, left, window)
        for mirror in (False, True):
            got = ops.frame_remap_ingest(frames, table, lm, fmt, mirror_too=mirror)
            plain = ops.frame_ingest_format(frames, table, fmt, top, left, window, mirror_too=mirror)
            assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), (fmt.name, top, left, window, mirror)
            if fmt.name == "rgb24":
                assert torch.equal(got.view(torch.int32), ops.frame_ingest(frames, table, top, left, window, mirror_too=mirror).view(torch.int32))
        crop = torch.from_numpy(np.ascontiguousarray(rgb[:, top:top + window[0], left:left + window[1]]))
        assert torch.equal(ops.frames_remap_rgb24(frames, lm, fmt).cpu(), crop)


@pytest.mark.parametrize("fmt", [FORMATS[1], FORMATS[5]], ids=_id)
def test_rgb24_launch_then_resize_equals_the_resize_of_the_statements_bytes(ops, fmt):
    """The two launches ``lens`` + ``resize`` takes: ``frame_resize_ingest`` of the rgb24 launch's output is ``frame_resize_ingest`` of the
    reference's rectified bytes."""
    _, frames, _ = source(fmt)
    table = _table().cuda()
    for window, size in ((SCALAR, (7, 17)), (VEC, (8, 20))):
        lm = maps(window)["three"]
        rect = torch.from_numpy(want_rgb(fmt, window, "three")).cuda()
        for mirror in (False, True):
            got = ops.frame_resize_ingest(ops.frames_remap_rgb24(frames, lm, fmt), table, size, mirror_too=mirror)
            want = ops.frame_resize_ingest(rect, table, size, mirror_too=mirror)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (fmt.name, window, mirror)


# --------------------------------------------------------------------------- guarded memory: a row of tests/test_hip_memory_bounds.py's table
ROW = "frame_remap|13x37 -> 12x32, 11x30, six formats"


def _remap_row(c):
    """Both entry points, every plane at its exact size between poisoned guards (a chroma plane of 7 x 19 samples, not one more), through
    the shifted map -- its taps touch the first and the last byte of every plane and walk off the frame on all four sides -- and the
    three-map batch; VEC and scalar form, with the mirror.  Every byte of every output is written."""
    table = c.put(_table())
    for fmt in FORMATS:
        planes, _, _ = source(fmt)
        dev = [c.put(p) for p in planes]
        frames = PlanarFrames(fmt.name, dev, HS, WS) if fmt.planar else dev[0]
        yuv = c.put(fmt.tables()) if fmt.planar else None
        for window in (VEC, SCALAR):
            for name in ("shifted", "three"):
                m = c.put(maps(window)[name].map)
                rgb = c.ops.frames_remap_rgb24(frames, m, fmt, yuv_tables=yuv)
                got = c.ops.frame_remap_ingest(frames, table, m, fmt, mirror_too=True, yuv_tables=yuv)
                rect = want_rgb(fmt, window, name)
                assert torch.equal(rgb.cpu(), torch.from_numpy(rect)), (fmt.name, window, name)
                want = torch.from_numpy(ref.ingest(rect, _table().numpy(), True))
                assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (fmt.name, window, name)
                c.out(got)
                if rgb.numel() % 4 == 0:                                         # (the harness counts unwritten 32-bit words)
                    c.out(rgb)


if ROW not in bounds.ROWS:
    bounds.row(ROW)(_remap_row)


def test_both_launches_between_poisoned_guards():
    bounds.run_row(ROW)
    assert "ocv_frame_remap_ingest_fwd" in bounds.RAN[ROW] and "ocv_frames_remap_rgb24_fwd" in bounds.RAN[ROW]


# --------------------------------------------------------------------------- child processes: a captured graph, the predict path
def _child(script, seconds):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=seconds)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


def test_captured_graph_replays_with_new_frames_and_a_new_map():
    """In a fresh child process (tests/lens_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    _child("lens_graph_child.py", 300)


def test_predictors_with_lens_equal_the_predictors_on_rectified_frames():
    """In a fresh child process (tests/lens_predict_child.py), for the reason tests/ground_grid_predict_child.py gives."""
    _child("lens_predict_child.py", 600)
