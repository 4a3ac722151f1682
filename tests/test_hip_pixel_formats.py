"""-m gpu: the pixel formats on ingest -- csrc/pixel_fetch.hpp through its three entry points against Statement P
(tests/pixel_format_ref.py, numpy integers) BIT FOR BIT, their guarded runs (tests/mem_guard.py), and ``Predictor`` /
``PipelinedPredictor`` with ``pixel_format`` against the same predictors on the statement's RGB frames.  Every source plane is a strided
view -- padded rows, padded frames, a base pointer at an odd byte -- unless a test says otherwise."""
import numpy as np
import pytest
import torch

import gen
import mem_guard
import pixel_format_ref as ref
from objcavit_amd.config import make_args
from objcavit_amd.pixel_formats import PixelFormat, PlanarFrames, chroma_size

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
B = 2
PACKED = ("rgb24", "bgr24", "rgba32", "bgra32")
VARIANTS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
FORMATS = [PixelFormat(n) for n in PACKED] + [PixelFormat(n, m, r) for n in ("nv12", "i420") for m, r in VARIANTS]
# (Hs, Ws, top, left, Hw, Ww): 10 x 14 at four origin parities and two window sizes; 9 x 13 (odd: the last chroma row and column) with
# the window touching the bottom-right corner
WINDOWS = [(10, 14, t, l, h, w) for (t, l) in ((1, 1), (0, 3), (1, 0), (2, 2)) for (h, w) in ((6, 8), (5, 7))] + [(9, 13, 3, 5, 6, 8)]
ODD_ORIGIN, ODD_SCALAR, CORNER = (10, 14, 1, 1, 6, 8), (10, 14, 1, 1, 5, 7), (9, 13, 3, 5, 6, 8)
_MADE = {}


def _id(fmt):
    return f"{fmt.name}-{fmt.matrix}-{fmt.range}" if fmt.planar else fmt.name


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def _table():
    if "table" not in _MADE:
        from objcavit_amd.predict import normalisation_table
        _MADE["table"] = normalisation_table(make_args())
    return _MADE["table"]


def _host_planes(name, Hs, Ws, seed):
    """The planes of B random frames on the host, every byte value present in every plane that is large enough."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        n = int(np.prod(shape))
        return (torch.arange(n) % 256)[torch.randperm(n, generator=g)].to(torch.uint8).view(*shape)

    Hc, Wc = chroma_size(Hs, Ws)
    if name == "nv12":
        return [rnd(B, Hs, Ws), rnd(B, Hc, Wc, 2)]
    if name == "i420":
        return [rnd(B, Hs, Ws), rnd(B, Hc, Wc), rnd(B, Hc, Wc)]
    return [rnd(B, Hs, Ws, 4 if name.endswith("32") else 3)]


def _strided(p, k):
    """A device copy of a host plane as a view into a larger buffer of other bytes: rows padded by 5 bytes, frames by 7 more, the base
    pointer 1 (3, 5 for the next planes) bytes off the allocation's alignment."""
    n, rows = int(p.shape[0]), int(p.shape[1])
    row_bytes = int(np.prod(p.shape[2:]))
    rs, off = row_bytes + 5, 2 * k + 1
    fs = rows * rs + 7
    buf = torch.full((off + n * fs + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    inner = tuple(int(np.prod(p.shape[i + 1:])) for i in range(2, p.dim()))
    view = torch.as_strided(buf, tuple(p.shape), (fs, rs) + inner, off)
    view.copy_(p.cuda())
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    return view


def _device(name, planes, Hs, Ws, strided=True):
    dev = [_strided(p, k) if strided else p.cuda() for k, p in enumerate(planes)]
    return PlanarFrames(name, dev, Hs, Ws) if name in ("nv12", "i420") else dev[0]


def _case(fmt, Hs, Ws):
    """(host planes, device frames, the statement's RGB of the whole frame uint8 [B, Hs, Ws, 3] on the host): made once, shared."""
    key = (_id(fmt), Hs, Ws)
    if key not in _MADE:
        planes = _host_planes(fmt.name, Hs, Ws, 300 + 17 * Hs + Ws)
        src = planes if fmt.planar else planes[0]
        _MADE[key] = (planes, _device(fmt.name, planes, Hs, Ws), torch.from_numpy(ref.rgb_of(src, fmt, 0, 0, Hs, Ws)))
    return _MADE[key]


# ---------------------------------------------------------------------------
# frames_to_rgb24: the device-side witness of Statement P
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=_id)
def test_frames_to_rgb24_is_statement_p_bit_for_bit(ops, fmt):
    for Hs, Ws, top, left, Hw, Ww in WINDOWS:
        planes, frames, _ = _case(fmt, Hs, Ws)
        want = torch.from_numpy(ref.rgb_of(planes if fmt.planar else planes[0], fmt, top, left, Hw, Ww))
        got = ops.frames_to_rgb24(frames, fmt, top, left, (Hw, Ww))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (B, Hw, Ww, 3) and got.is_contiguous()
        assert torch.equal(got.cpu(), want), (Hs, Ws, top, left, Hw, Ww)
    Hs, Ws = 10, 14                                                              # the whole frame by default; out=
    planes, frames, rgb = _case(fmt, Hs, Ws)
    out = torch.zeros(B, Hs, Ws, 3, dtype=torch.uint8, device="cuda")
    assert ops.frames_to_rgb24(frames, fmt, out=out) is out and torch.equal(out.cpu(), rgb)
    with pytest.raises(ValueError):
        ops.frames_to_rgb24(frames, fmt, 5, 0, (6, 8))                           # 5 + 6 > 10 rows


def _every_value_frames(name):
    """208 x 208 luma: every Y value against every (Cb, Cr) of 13 x 13 values around the ends, the clamps and the centre -- 169 pairs x 64
    chroma samples, whose 2 x 2 blocks hold the 256 Y values; the second frame holds 255 - Y."""
    vals = np.array([0, 1, 15, 16, 17, 127, 128, 129, 239, 240, 241, 254, 255], dtype=np.uint8)
    s = np.arange(104 * 104)
    pair, block = s // 64, s % 64
    cb = vals[pair // 13].reshape(104, 104)
    cr = vals[pair % 13].reshape(104, 104)
    y = np.zeros((208, 208), dtype=np.uint8)
    blk = block.reshape(104, 104)
    for dy in range(2):
        for dx in range(2):
            y[dy::2, dx::2] = blk * 4 + dy * 2 + dx
    Y = np.stack([y, 255 - y])
    Cb, Cr = np.stack([cb, cb]), np.stack([cr, cr])
    for b in range(2):                                                           # every (Y, Cb, Cr) of the 256 x 169 is there
        seen = set(zip(Y[b].ravel().tolist(), np.repeat(np.repeat(cb, 2, 0), 2, 1).ravel().tolist(),
                       np.repeat(np.repeat(cr, 2, 0), 2, 1).ravel().tolist()))
        assert len(seen) == 256 * 169
    if name == "nv12":
        return [torch.from_numpy(Y), torch.from_numpy(np.ascontiguousarray(np.stack([Cb, Cr], -1)))]
    return [torch.from_numpy(Y), torch.from_numpy(np.ascontiguousarray(Cb)), torch.from_numpy(np.ascontiguousarray(Cr))]


@pytest.mark.parametrize("fmt", [f for f in FORMATS if f.planar], ids=_id)
def test_every_luma_value_against_every_chroma_end_and_clamp(ops, fmt):
    if ("every", fmt.name) not in _MADE:
        planes = _every_value_frames(fmt.name)
        _MADE[("every", fmt.name)] = (planes, _device(fmt.name, planes, 208, 208))
    planes, frames = _MADE[("every", fmt.name)]
    want = ref.rgb_of(planes, fmt, 0, 0, 208, 208)
    assert want.min() == 0 and want.max() == 255                                 # both clamps are hit
    got = ops.frames_to_rgb24(frames, fmt)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ---------------------------------------------------------------------------
# frame_ingest_format = frame_ingest on the statement's RGB frames
# ---------------------------------------------------------------------------
INGEST_FORMATS = [PixelFormat("nv12", "bt709", "limited"), PixelFormat("nv12", "bt601", "full"), PixelFormat("i420", "bt601", "limited"),
                  PixelFormat("i420", "bt709", "full"), PixelFormat("bgr24"), PixelFormat("rgba32"), PixelFormat("bgra32"), PixelFormat("rgb24")]


@pytest.mark.parametrize("fmt", INGEST_FORMATS, ids=_id)
def test_frame_ingest_format_equals_frame_ingest_on_the_statements_rgb(ops, fmt):
    table = _table().cuda()
    for Hs, Ws, top, left, H, W in WINDOWS:                                      # W = 8: 16-byte stores; W = 7: scalar stores
        _, frames, rgb = _case(fmt, Hs, Ws)
        rgb = rgb.cuda()
        for mirror in (False, True):
            want = ops.frame_ingest(rgb, table, top, left, (H, W), mirror_too=mirror)
            got = ops.frame_ingest_format(frames, table, fmt, top, left, (H, W), mirror_too=mirror)
            assert tuple(got.shape) == ((2 * B if mirror else B), 3, H, W) and got.dtype == torch.float32
            assert torch.equal(got, want), (Hs, Ws, top, left, H, W, mirror)
    # out= / out_index: one batch filled by one launch per frame; the other images stay what they were
    Hs, Ws, top, left, H, W = ODD_ORIGIN
    _, frames, rgb = _case(fmt, Hs, Ws)
    want = ops.frame_ingest(rgb.cuda(), table, top, left, (H, W), mirror_too=True)
    out = torch.full((6, 3, H, W), float("nan"), device="cuda")
    for i in range(B):
        one = frames[i] if fmt.planar else frames[i:i + 1]
        assert ops.frame_ingest_format(one, table, fmt, top, left, (H, W), mirror_too=True, out=out, out_index=i + 1) is out
    assert torch.equal(out[1:3], want[:B]) and torch.equal(out[4:6], want[B:]) and bool(torch.isnan(out[[0, 3]]).all())
    with pytest.raises(ValueError):
        ops.frame_ingest_format(frames, table, fmt, top, left, (H, W), mirror_too=True, out=out, out_index=2)


def test_rgb24_through_the_new_entry_point_equals_the_old_one(ops):
    table = _table().cuda()
    fmt = PixelFormat("rgb24")
    for Hs, Ws, top, left, H, W in WINDOWS:
        _, frames, _ = _case(fmt, Hs, Ws)
        for mirror in (False, True):
            assert torch.equal(ops.frame_ingest_format(frames, table, "rgb24", top, left, (H, W), mirror_too=mirror),
                               ops.frame_ingest(frames, table, top, left, (H, W), mirror_too=mirror))
    _, frames, _ = _case(fmt, 10, 14)
    assert torch.equal(ops.frame_resize_ingest_format(frames, table, (5, 8), "rgb24", 1, 1, (8, 12), mirror_too=True),
                       ops.frame_resize_ingest(frames, table, (5, 8), 1, 1, (8, 12), mirror_too=True))


# ---------------------------------------------------------------------------
# frame_resize_ingest_format = frame_resize_ingest on the statement's RGB frames (same tap tables, hence the same arithmetic)
# ---------------------------------------------------------------------------
# name -> (Hs, Ws, top, left, Hw, Ww, H, W)
RESIZE_CASES = {
    "offset window, 16-byte stores": (37, 53, 3, 5, 31, 45, 16, 24),
    "odd W, scalar stores": (31, 45, 0, 0, 31, 45, 15, 23),
    "enlarge": (9, 7, 0, 0, 9, 7, 16, 12),
    "ratio 8, the smallest tile with the tables in LDS": (128, 96, 0, 0, 128, 96, 16, 12),
    "every tile edge": (61, 150, 0, 0, 61, 150, 21, 72),
}
RESIZE_FORMATS = [PixelFormat("nv12", "bt709", "limited"), PixelFormat("i420", "bt601", "full"), PixelFormat("bgra32")]


@pytest.mark.parametrize("fmt", RESIZE_FORMATS, ids=_id)
@pytest.mark.parametrize("name", list(RESIZE_CASES))
def test_frame_resize_ingest_format_equals_frame_resize_ingest_on_the_statements_rgb(ops, name, fmt):
    Hs, Ws, top, left, Hw, Ww, H, W = RESIZE_CASES[name]
    _, frames, rgb = _case(fmt, Hs, Ws)
    table = _table().cuda()
    want = ops.frame_resize_ingest(rgb.cuda(), table, (H, W), top, left, (Hw, Ww), mirror_too=True)
    got = ops.frame_resize_ingest_format(frames, table, (H, W), fmt, top, left, (Hw, Ww), mirror_too=True)
    assert tuple(got.shape) == (2 * B, 3, H, W)
    assert torch.equal(got, want)
    assert torch.equal(got[B:], got[:B].flip(3))
    assert torch.equal(ops.frame_resize_ingest_format(frames, table, (H, W), fmt, top, left, (Hw, Ww)), want[:B])      # without the mirror


def test_resize_refusals(ops):
    table = _table().cuda()
    fmt = PixelFormat("nv12")
    _, frames, _ = _case(fmt, 128, 96)
    R = ops.FRAME_RESIZE_MAX_RATIO
    with pytest.raises(ValueError, match=str(R)):
        ops.frame_resize_ingest_format(frames, table, (15, 12), fmt)              # 128 rows to 15: above the ratio
    with pytest.raises(ValueError):
        ops.frame_resize_ingest_format(frames, table, (16, 12), fmt, 1, 0, (128, 96))
    with pytest.raises(TypeError):
        ops.frame_resize_ingest_format(frames, table, (16, 12), "i420")          # nv12 planes for an i420 call


# ---------------------------------------------------------------------------
# guarded runs: the three entry points have no row in tests/test_hip_memory_bounds.py (their names do not end in _fwd)
# ---------------------------------------------------------------------------
GUARD_FORMATS = [PixelFormat("nv12", "bt601", "limited"), PixelFormat("i420", "bt709", "full"), PixelFormat("bgra32"), PixelFormat("bgr24")]


@pytest.mark.parametrize("case", [ODD_ORIGIN, ODD_SCALAR, CORNER], ids=["odd origin", "odd origin, scalar stores", "bottom-right corner"])
@pytest.mark.parametrize("fmt", GUARD_FORMATS, ids=_id)
def test_guarded_runs_write_every_output_and_nothing_else(fmt, case):
    """Every plane at its exact size between poisoned guards (a chroma plane of ceil(Hs / 2) x ceil(Ws / 2) samples, not one more)."""
    from objcavit_amd import hip_ops
    Hs, Ws, top, left, Hw, Ww = case
    planes, _, rgb = _case(fmt, Hs, Ws)
    H, W = (3, 4) if case is ODD_ORIGIN else (4, 5)                              # the resize's output: 16-byte stores / scalar stores
    host_taps = hip_ops.resize_taps(Hw, H) + hip_ops.resize_taps(Ww, W)
    want_rgb = rgb[:, top:top + Hw, left:left + Ww]
    try:
        with mem_guard.guarded("cuda") as g:
            g.record_calls()
            dev = [g.copy(p) for p in planes]
            frames = PlanarFrames(fmt.name, dev, Hs, Ws) if fmt.planar else dev[0]
            table = g.copy(_table())
            yuv = g.copy(fmt.tables()) if fmt.planar else None
            taps = tuple(g.copy(t) for t in host_taps)
            runs = []
            for _ in range(2):
                a = hip_ops.frames_to_rgb24(frames, fmt, top, left, (Hw, Ww), yuv_tables=yuv)
                b = hip_ops.frame_ingest_format(frames, table, fmt, top, left, (Hw, Ww), mirror_too=True, yuv_tables=yuv)
                c = hip_ops.frame_resize_ingest_format(frames, table, (H, W), fmt, top, left, (Hw, Ww), mirror_too=True, taps=taps,
                                                       yuv_tables=yuv)
                runs.append((a, b, c))
            torch.cuda.synchronize()
            g.check()
            for name in ("ocv_frames_to_rgb24", "ocv_frame_ingest_format", "ocv_frame_resize_ingest_format"):
                assert g.calls.count(name) == 2, g.calls
            assert not g.stray, g.stray
            for a, b, c in runs:
                assert g.never_written(b) == 0 and g.never_written(c) == 0
                assert torch.equal(a.cpu(), want_rgb)                            # every byte of the RGB copy is the statement's: all written
            for x, y in zip(*runs):
                assert torch.equal(x, y)                                         # two calls give identical bytes
            want = hip_ops.frame_ingest(g.copy(rgb), table, top, left, (Hw, Ww), mirror_too=True)
            assert torch.equal(runs[0][1], want)
            want = hip_ops.frame_resize_ingest(g.copy(rgb), table, (H, W), top, left, (Hw, Ww), mirror_too=True, taps=taps)
            assert torch.equal(runs[0][2], want)
    except RuntimeError as e:                      # a device fault ends the session: nothing more is launched on a faulted GPU
        if "HIP error" in str(e) or "illegal memory" in str(e) or "hipError" in str(e):
            pytest.exit(f"GPU fault in the guarded run of {_id(fmt)}: {e}", returncode=3)
        raise


# ---------------------------------------------------------------------------
# predict path: a 192 x 208 model (the smallest end-to-end size the suite runs)
# ---------------------------------------------------------------------------
MH, MW = 192, 208
NV12_709 = PixelFormat("nv12", "bt709")


def _model():
    if "model" not in _MADE:
        from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
        args = make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip", do_final_upscale=True,
                         dimensions_train=[MH, MW], dimensions_test=[MH, MW])
        m = GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5)).eval()
        gen.load_into(m, 23, gen.PEAKY)
        _MADE["model"] = (m.cuda(), args)
    return _MADE["model"]


def _nv12(seed, n, Hs, Ws):
    """(PlanarFrames over ONE contiguous buffer [n, Hs * 3 / 2, Ws] on the device, the statement's RGB frames on the device)."""
    buf = torch.randint(0, 256, (n, Hs * 3 // 2, Ws), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    host = PlanarFrames.from_buffer(buf, "nv12", Hs, Ws)
    rgb = torch.from_numpy(ref.rgb_of(host.planes, NV12_709, 0, 0, Hs, Ws))
    return PlanarFrames.from_buffer(buf.cuda(), "nv12", Hs, Ws), rgb.cuda()


def _gt(n, H, W, seed, dmax=10.0):
    return torch.rand(n, 1, H, W, generator=torch.Generator().manual_seed(seed)) * 0.9 * dmax + 0.05 * dmax


def _same(a, b):
    assert torch.equal(a.depth, b.depth) and torch.equal(a.records, b.records) and torch.equal(a.bin_edges, b.bin_edges)


def test_predictor_on_nv12_frames_equals_the_predictor_on_the_statements_rgb(ops):
    from objcavit_amd.predict import Predictor
    m, args = _model()
    nv, rgb = _nv12(71, 2, MH, MW)
    gt = _gt(2, MH, MW, 72).cuda()
    ops.enable_timing(True)
    res = Predictor(m, args, pixel_format=NV12_709)(nv, gt, first_image_id=4)
    counts = {k: v[0] for k, v in ops.timing_results().items()}
    ops.enable_timing(False)
    assert counts.get("frame_ingest_format") == 1 and "frame_ingest" not in counts, counts
    want = Predictor(m, args)(rgb, gt, first_image_id=4)
    _same(res, want)
    assert tuple(res.depth.shape) == (2, 1, MH, MW) and bool(torch.isfinite(res.depth).all())
    # a list of single frames, as today
    lst = Predictor(m, args, pixel_format=NV12_709)([nv[0], nv[1]], gt, first_image_id=4)
    _same(lst, want)


def test_predictor_on_nv12_frames_with_crop_and_resize_and_the_clouds_colour(ops):
    from objcavit_amd.predict import Predictor, fit_window
    m, args = _model()
    nv, rgb = _nv12(73, 2, 250, 300)
    top, left, Hw, Ww = fit_window(250, 300, MH, MW)
    assert (top, left, Hw, Ww) == (0, 15, 250, 270)                              # an odd left edge: the window starts inside a chroma sample
    gt = _gt(2, Hw, Ww, 74).cuda()
    K = torch.tensor([[280.0, 285.0, 149.5, 124.5], [300.0, 300.0, 140.0, 130.0]])
    kw = dict(crop=(top, left, Hw, Ww), resize=(MH, MW), point_cloud=dict(stride=(2, 3), colour=True))
    res = Predictor(m, args, pixel_format=NV12_709, **kw)(nv, gt, first_image_id=2, intrinsics=K)
    want = Predictor(m, args, **kw)(rgb, gt, first_image_id=2, intrinsics=K)
    _same(res, want)
    assert tuple(res.depth.shape) == (2, 1, Hw, Ww)
    assert torch.equal(res.points.counts, want.points.counts) and int(want.points.counts.min()) > 0
    for b in range(2):
        k = int(want.points.counts[b])
        assert torch.equal(res.points.rgba[b, :k], want.points.rgba[b, :k])      # bytes 12 - 14: Statement P's R, G, B
        assert torch.equal(res.points.points[b, :k].view(torch.int32), want.points.points[b, :k].view(torch.int32))
    assert int(res.points.rgba[0, :int(want.points.counts[0]), :3].max()) > 0
    # without resize: the cropped window at the model's size
    kw = dict(crop=(29, 45, MH, MW), point_cloud=dict(colour=True))
    res = Predictor(m, args, pixel_format=NV12_709, **kw)(nv, intrinsics=K)
    want = Predictor(m, args, **kw)(rgb, intrinsics=K)
    assert torch.equal(res.depth, want.depth)
    k = int(want.points.counts[0])
    assert k > 0 and torch.equal(res.points.rgba[0, :k], want.points.rgba[0, :k])


def test_bgr_and_bgra_frames_give_the_rgb_runs_result(ops):
    from objcavit_amd.predict import Predictor
    m, args = _model()
    rgb = torch.randint(0, 256, (2, MH, MW, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(75)).cuda()
    gt = _gt(2, MH, MW, 76).cuda()
    want = Predictor(m, args)(rgb, gt)
    _same(Predictor(m, args, pixel_format="bgr24")(rgb.flip(3).contiguous(), gt), want)
    bgra = torch.cat([rgb.flip(3), torch.full((2, MH, MW, 1), 77, dtype=torch.uint8, device="cuda")], 3)
    _same(Predictor(m, args, pixel_format="bgra32")(bgra, gt), want)
    _same(Predictor(m, args, pixel_format="rgb24")(rgb, gt), want)


def test_pipelined_predictor_on_nv12_frames_equals_the_sequential_predictor(ops):
    """Four bs-1 steps over two slots: bit for bit the sequential ``Predictor`` on a captured graph of the same shape (both sides replay a
    GraphedGraphBins, so the dispatch is identical)."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor, normalisation_table
    m, args = _model()
    steps = [_nv12(80 + i, 1, MH, MW) for i in range(4)]
    gts = [_gt(1, MH, MW, 90 + i).cuda() for i in range(4)]
    pp = PipelinedPredictor(m, args, steps[0][0], slots=2, pixel_format="nv12")
    assert len(pp.graphs) == 2 and tuple(pp.graphs[0].static_image.shape) == (2, 3, MH, MW)
    example = ops.frame_ingest_format(steps[0][0], normalisation_table(args).cuda(), "nv12", mirror_too=True)
    seq = Predictor(GraphedGraphBins(m, example, object_group=1, in_flight=2), args, pixel_format="nv12")
    want = []
    for i in range(4):
        r = seq(steps[i][0], gts[i], first_image_id=i)
        want.append((r.depth.clone(), r.records.clone()))
    for i in range(4):
        pp.submit(steps[i][0], gts[i], first_image_id=i)
    got = pp.collect()
    assert len(got) == 4 and pp.rerun_steps == 0
    for i in range(4):
        assert torch.equal(got[i].depth, want[i][0]) and torch.equal(got[i].records, want[i][1]), i
    with pytest.raises(ValueError):
        pp.submit(steps[0][1])                                                   # an RGB tensor for an nv12 pipeline
