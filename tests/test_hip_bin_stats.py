"""-m gpu: the bin head's per-pixel statistics -- the STATS instantiations of csrc/bin_head.hip on every route,
ocv_depth_finalize_stats_fwd, and the two new ``want`` outputs of the predict path -- against the float64 helpers of
tests/bin_stats_ref.py.

Bars.  Head: per case the plain fp32 formulation a user of the reference would write (``bin_stats_ref.head_stats_fp32``, on the CPU) is
measured against float64 as well: with e32 its largest error and eHIP the kernel's, eHIP <= 2 e32 + 8.5e-9 (max_depth - min_depth)^2
for var and eHIP <= 2 e32 + 8.5e-9 + 2^-23 for pmax.  The factor 2 is what test_pixel_dot_and_bin_head_channels_last allows a different
summation order; 8.5e-9 = 224 e^-24 is the weight of the bins the two-level kernel may leave out.  Finalize: the same rule against the
same mixture formula evaluated in fp32 torch, plus 2 ulp of the result."""
import math
import os

import pytest
import torch

import bin_stats_ref
import gen
import predict_ref
from objcavit_amd.config import make_args

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DMIN, DMAX = 0.001, 10.0
SPAN2 = (DMAX - DMIN) ** 2
SKIP = 8.5e-9                    # 224 e^-24
ULP1 = 2.0 ** -23


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def rnd(key, shape, seed=0, scale=1.0):
    return gen.randn(key, shape, seed, scale)


# ---------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------
SHAPES = [(1, 8, 16), (3, 37, 53)]            # less than one workgroup tile; ragged 32-pixel tiles, several images with own centres
GAINS = ["stress", "flat", "bimodal"]
ROUTES = ["nchw", "nhwc_exact", "h2", "h2dense", "split3", "bf16_pairs"]
_CASES = {}


def _case(shape, gain):
    """Inputs as test_bin_head builds them + the float64 and the plain-fp32 references, computed once per (shape, gain)."""
    key = (shape, gain)
    if key not in _CASES:
        from objcavit_amd.modules.AdaBins import bin_edges_and_centers
        B, h, w = shape
        feat, q = rnd("f", (B, 128, h, w), 1), rnd("q", (B, 300, 128), 2, 0.5)
        wout, bout = rnd("wo", (256, 128, 1, 1), 3, 6 / math.sqrt(128)), rnd("bo", (256,), 4, 0.5)
        if gain != "stress":                   # flat: every tile is kept under TWO_LEVEL, var near range^2 / 12
            wout = wout * 0.02
        if gain == "bimodal":                  # the mass in the first and the last bin tile: the skipped tiles lie between kept ones
            bout = bout.clone()
            bout[10] += 12.0
            bout[200] += 12.0
        widths = torch.rand(B, 256, generator=torch.Generator().manual_seed(5)) + 0.1
        widths = widths / widths.sum(1, keepdim=True)
        _, centers = bin_edges_and_centers(widths.cuda(), DMIN, DMAX)
        queries = q[:, 1:129, :]
        ref64 = bin_stats_ref.head_stats(feat, queries, wout, bout, centers)
        ref32 = bin_stats_ref.head_stats_fp32(feat, queries, wout, bout, centers, DMIN, DMAX)
        _CASES[key] = dict(feat=feat.cuda(), q=q.cuda(), wout=wout.cuda(), bout=bout.cuda(), centers=centers, ref64=ref64,
                           e32_var=float((ref32[1].double() - ref64[1]).abs().max()),
                           e32_pmax=float((ref32[2].double() - ref64[2]).abs().max()))
    return _CASES[key]


def _run(ops, monkeypatch, c, route, stats, feat=None):
    fg = c["feat"] if feat is None else feat
    if route != "nchw" and feat is None:
        fg = fg.contiguous(memory_format=torch.channels_last)
    args = (fg, c["q"][:, 1:129, :], c["wout"], c["bout"], c["centers"])
    monkeypatch.delenv("OCV_BINHEAD", raising=False)
    if route in ("h2", "h2dense", "split3"):
        monkeypatch.setenv("OCV_BINHEAD", route)
    if route == "bf16_pairs":
        with ops.bf16_pairs():
            return ops.bin_head(*args, stats=stats)
    return ops.bin_head(*args, exact=route == "nhwc_exact", stats=stats)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bin_head_stats(ops, monkeypatch, shape, gain, route):
    c = _case(shape, gain)
    plain = _run(ops, monkeypatch, c, route, False)
    depth, var, pmax = _run(ops, monkeypatch, c, route, True)
    again = _run(ops, monkeypatch, c, route, True)
    assert tuple(var.shape) == tuple(pmax.shape) == tuple(plain.shape)
    assert torch.equal(depth, plain)                                        # depth keeps its bits
    assert all(torch.equal(a, b) for a, b in zip((depth, var, pmax), again))
    d64, var64, pmax64 = c["ref64"]
    e_var = float((var.cpu().double() - var64).abs().max())
    e_pmax = float((pmax.cpu().double() - pmax64).abs().max())
    print(f"bin_stats {'x'.join(map(str, shape))} {gain} {route}: var e32 {c['e32_var']:.3e} eHIP {e_var:.3e}   "
          f"pmax e32 {c['e32_pmax']:.3e} eHIP {e_pmax:.3e}   (var64 max {float(var64.max()):.4g}, pmax64 min {float(pmax64.min()):.4g})")
    assert float(var.min()) >= 0.0 and float(pmax.min()) > 0.0 and float(pmax.max()) <= 1.0
    assert e_var <= 2.0 * c["e32_var"] + SKIP * SPAN2, (e_var, c["e32_var"])
    assert e_pmax <= 2.0 * c["e32_pmax"] + SKIP + ULP1, (e_pmax, c["e32_pmax"])
    if gain == "flat":
        assert abs(float(var64.mean()) - SPAN2 / 12) < 0.2 * SPAN2 / 12     # the case is what it says
    if gain == "stress":
        assert float(var64.median()) < 0.05


def test_bin_head_stats_one_nan_pixel(ops, monkeypatch):
    c = _case((3, 37, 53), "stress")
    bad = c["feat"].contiguous(memory_format=torch.channels_last).clone(memory_format=torch.preserve_format)
    bad[1, 77, 20, 41] = float("nan")
    good = _run(ops, monkeypatch, c, "h2", True)
    got = _run(ops, monkeypatch, c, "h2", True, feat=bad)
    for g, t in zip(good, got):
        nan = torch.isnan(t)
        assert int(nan.sum()) == 1 and bool(nan[1, 0, 20, 41])
        assert torch.equal(t[~nan], g[~nan])


def test_bin_head_stats_only_one_of_the_two(ops):
    """The C entry point with var or pmax left out: the other one keeps its bits."""
    from objcavit_amd import _lib
    lib = _lib.load()
    c = _case((1, 8, 16), "stress")
    fg = c["feat"].contiguous(memory_format=torch.channels_last)
    depth, var, pmax = ops.bin_head(fg, c["q"][:, 1:129, :], c["wout"], c["bout"], c["centers"], stats=True)
    q = c["q"][:, 1:129, :]
    wf = torch.empty(1, 256, 128, device="cuda")
    _lib.check(lib.ocv_bin_head_fold_fwd(q.data_ptr(), q.stride(0), q.stride(1), c["wout"].data_ptr(), wf.data_ptr(), 1, 128, 128, 256, None), "fold")
    for keep in ("var", "pmax"):
        d2, o = torch.empty_like(depth), torch.empty_like(depth)
        _lib.check(lib.ocv_bin_head_folded_stats_fwd(fg.data_ptr(), 4, wf.data_ptr(), c["bout"].data_ptr(), c["centers"].data_ptr(), d2.data_ptr(),
                                                     1, 128, 256, 128, None, 0, o.data_ptr() if keep == "var" else None,
                                                     o.data_ptr() if keep == "pmax" else None, None), "stats")
        torch.cuda.synchronize()
        assert torch.equal(d2, depth) and torch.equal(o, var if keep == "var" else pmax)


# ---------------------------------------------------------------------------
# finalize
# ---------------------------------------------------------------------------
def _maps(seed, B, h, w):
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(B, 1, h, w, generator=g) * 11.0 - 0.5                  # some beyond [min_depth, max_depth]: the mixture takes them unclamped
    var = torch.rand(B, 1, h, w, generator=g) * 2.0
    pmax = torch.rand(B, 1, h, w, generator=g) * 0.99 + 0.01
    return d, var, pmax


# the issue's two sizes (P = 140 and 143: scalar stores) + every other path of the launch: the staged tile (W % 8 == 0), eight pixels a
# thread without a tile (P % 8 == 0, W % 8 != 0), the equal-size short-cut, and a tile whose source window does not fit the LDS stage
FIN_SIZES = [(5, 7, 10, 14), (5, 7, 11, 13), (5, 7, 12, 16), (5, 7, 8, 12), (4, 8, 4, 8), (70, 130, 16, 128)]


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("h,w,H,W", FIN_SIZES)
def test_depth_finalize_stats(ops, h, w, H, W, mirror):
    B = 2
    d, var, pmax = _maps(7, B, h, w)
    dm, varm, pmaxm = _maps(8, B, h, w) if mirror else (None, None, None)
    std64, conf64, _, _ = bin_stats_ref.full_stats(d, var, pmax, dm, varm, pmaxm, (H, W))
    std32, conf32, _, _ = bin_stats_ref.full_stats(d, var, pmax, dm, varm, pmaxm, (H, W), dtype=torch.float32)
    cu = lambda t: None if t is None else t.cuda()   # noqa: E731
    kw = dict(pred_mirror=cu(dm), var=cu(var), pmax=cu(pmax), var_mirror=cu(varm), pmax_mirror=cu(pmaxm))
    got = ops.depth_finalize(cu(d), DMIN, DMAX, (H, W), want=("depth", "depth_u16", "depth_std", "confidence"), **kw)
    assert tuple(got["depth_std"].shape) == tuple(got["confidence"].shape) == (B, 1, H, W)
    for name, r64, r32 in (("depth_std", std64, std32), ("confidence", conf64, conf32)):
        e32 = float((r32.double() - r64).abs().max())
        err = (got[name].cpu().double() - r64).abs()
        print(f"finalize_stats {h}x{w}->{H}x{W} mirror={mirror} {name}: e32 {e32:.3e} eHIP {float(err.max()):.3e}")
        assert bool((err <= 2.0 * e32 + 2.0 * ULP1 * r64.abs()).all()), (name, float(err.max()), e32)
    # the first three outputs are what they are without the new ones; the new ones alone, or one of them, keep their bits
    base = ops.depth_finalize(cu(d), DMIN, DMAX, (H, W), pred_mirror=cu(dm), want=("depth", "depth_u16"))
    assert torch.equal(got["depth"], base["depth"]) and torch.equal(got["depth_u16"].view(torch.uint8), base["depth_u16"].view(torch.uint8))
    only = ops.depth_finalize(cu(d), DMIN, DMAX, (H, W), want=("depth_std", "confidence"), **kw)
    assert set(only) == {"depth_std", "confidence"} and all(torch.equal(only[k], got[k]) for k in only)
    one = ops.depth_finalize(cu(d), DMIN, DMAX, (H, W), pred_mirror=cu(dm), want=("confidence",), pmax=cu(pmax), pmax_mirror=cu(pmaxm))
    assert torch.equal(one["confidence"], got["confidence"])
    with pytest.raises(ValueError):
        ops.depth_finalize(cu(d), DMIN, DMAX, (H, W), pred_mirror=cu(dm), want=("depth_std",))
    # a NaN source pixel: the substitutes at exactly the output pixels that have it as a tap
    d2, p2 = d.clone(), pmax.clone()
    d2[0, 0, 0, 3] = float("nan")                                           # (row 0 is a tap at every size here, the strong down-scale included)
    p2[1, 0, h - 1, 0] = float("nan")
    if mirror:
        varm = varm.clone()
        varm[1, 0, 1, 1] = float("nan")
        kw["var_mirror"] = cu(varm)
    kw["pmax"] = cu(p2)
    sref, cref, _, _ = bin_stats_ref.full_stats(d2, var, p2, dm, varm, pmaxm, (H, W))
    bad = ops.depth_finalize(cu(d2), DMIN, DMAX, (H, W), want=("depth_std", "confidence"), **kw)
    span = float(torch.tensor(DMAX, dtype=torch.float32) - torch.tensor(DMIN, dtype=torch.float32))
    for name, ref in (("depth_std", sref), ("confidence", cref)):
        hit = torch.isnan(ref)
        out = bad[name].cpu()
        assert int(hit.sum()) >= 1 and not bool(torch.isnan(out).any())
        assert bool((out[hit] == (span if name == "depth_std" else 0.0)).all())
        assert torch.equal(out[~hit], got[name].cpu()[~hit])


# ---------------------------------------------------------------------------
# through the interface
# ---------------------------------------------------------------------------
# 352 x 384: the size tests/test_hip_predict.py builds its small GraphBins at for the captured-graph / pipelined case (its eager case runs
# at 480 x 640); one size here, the smaller, so that the float64 reference over all 256 bins of every head pixel stays a few seconds
H_, W_, B_ = 352, 384, 2
WANT3 = ("depth", "depth_std", "confidence")


def _frames(seed, B, Hs, Ws):
    return torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _model(model, seed):
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    args = make_args(model=model, dataset="nyu", strategy="learned", language="clip", dimensions_train=[H_, W_], dimensions_test=[H_, W_])
    m = (AdaBins(args) if model == "adabins" else GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5))).eval()
    gen.load_into(m, seed, gen.PEAKY)
    return m.cuda(), args


def _interface_refs(m, args, frames):
    """float64 helpers (and the fp32 formulation through the fp32 mixture: the bar's e32) fed with the model's own head inputs."""
    ds = args[args.basic.dataset]
    img = predict_ref.frames_to_input(frames, args, 0, 0, H_, W_).cuda()
    both = torch.cat([img, img.flip(3)], 0)
    B = img.shape[0]
    parts = m.forward_until_head(both, None, None, None, B) if hasattr(m, "objcavit") else m.forward_until_head(both)
    feat, queries, centers = parts[:3]
    conv = m.conv_out[0]
    d, v, p = bin_stats_ref.head_stats(feat, queries, conv.weight, conv.bias, centers)
    std64, conf64, var64, _ = bin_stats_ref.full_stats(d[:B], v[:B], p[:B], d[B:], v[B:], p[B:], (H_, W_))
    d, v, p = bin_stats_ref.head_stats_fp32(feat, queries, conv.weight, conv.bias, centers, float(ds.min_depth), float(ds.max_depth))
    _, conf32, var32, _ = bin_stats_ref.full_stats(d[:B], v[:B], p[:B], d[B:], v[B:], p[B:], (H_, W_), dtype=torch.float32)
    return dict(var64=var64, conf64=conf64, e32_var=float((var32.double() - var64).abs().max()),
                e32_conf=float((conf32.double() - conf64).abs().max()), span2=(float(ds.max_depth) - float(ds.min_depth)) ** 2)


def _within_bars(res, ref, what):
    """Head bar + finalize bar, in the variance domain (depth_std squared: the square costs 2 more ulp of the result)."""
    var = res.depth_std.cpu().double() ** 2
    e_var = (var - ref["var64"]).abs()
    e_conf = (res.confidence.cpu().double() - ref["conf64"]).abs()
    print(f"{what}: var e32 {ref['e32_var']:.3e} eHIP {float(e_var.max()):.3e}   confidence e32 {ref['e32_conf']:.3e} eHIP {float(e_conf.max()):.3e}")
    assert float(res.depth_std.min()) >= 0.0 and float(res.confidence.min()) > 0.0 and float(res.confidence.max()) <= 1.0
    assert bool((e_var <= 2.0 * ref["e32_var"] + SKIP * ref["span2"] + 4.0 * ULP1 * ref["var64"]).all()), what
    assert bool((e_conf <= 2.0 * ref["e32_conf"] + SKIP + ULP1 + 2.0 * ULP1 * ref["conf64"]).all()), what


_SHARED = {}


def _graphbins():
    if "m" not in _SHARED:
        m, args = _model("graphbins", 23)
        frames = _frames(21, B_, H_, W_)
        _SHARED.update(m=m, args=args, frames=frames, ref=_interface_refs(m, args, frames))
    return _SHARED["m"], _SHARED["args"], _SHARED["frames"], _SHARED["ref"]


@pytest.mark.parametrize("model", ["graphbins", "adabins"])
def test_predictor_hands_out_depth_std_and_confidence(model):
    from objcavit_amd.predict import Predictor
    if model == "graphbins":
        m, args, frames, ref = _graphbins()
        m.bin_stats = False
    else:
        m, args = _model(model, 23)
        frames = _frames(21, B_, H_, W_)
        ref = _interface_refs(m, args, frames)
    pr = Predictor(m, args)
    plain = pr(frames.cuda(), want=("depth",))
    assert plain.depth_std is None and plain.confidence is None and m.bin_stats is False
    res = pr(frames.cuda(), want=WANT3)
    assert m.bin_stats is True                                              # the predictor turned it on for the model it was given
    assert torch.equal(res.depth, plain.depth)
    assert tuple(res.depth_std.shape) == tuple(res.confidence.shape) == (B_, 1, H_, W_)
    _within_bars(res, ref, f"Predictor({model})")
    out = m(predict_ref.frames_to_input(frames, args, 0, 0, H_, W_).cuda())
    assert out._fields[-2:] == ("depth_var", "confidence") and out[1] is out.bin_edges and tuple(out.depth_var.shape) == tuple(out.depth_pred.shape)


def test_captured_graph_and_pipelined_predictor_hand_them_out():
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args, frames, ref = _graphbins()
    img = predict_ref.frames_to_input(frames, args, 0, 0, H_, W_).cuda()
    both = torch.cat([img, img.flip(3)], 0)
    m.bin_stats = False
    without = GraphedGraphBins(m, both, object_group=B_)
    assert without.bin_stats is False and without.ReturnType._fields == ("depth_pred", "bin_edges", "detections")
    plain = Predictor(without, args)(frames.cuda(), want=("depth",))
    with pytest.raises(ValueError, match="captured without bin_stats"):
        Predictor(without, args)(frames.cuda(), want=WANT3)
    m.bin_stats = True
    g = GraphedGraphBins(m, both, object_group=B_)
    m.bin_stats = False                                                     # read at capture: the graph keeps what it was captured with
    assert g.bin_stats is True and g.ReturnType._fields[-2:] == ("depth_var", "confidence")
    res = Predictor(g, args)(frames.cuda(), want=WANT3)
    assert g.trips == 0 and torch.equal(res.depth, plain.depth)
    _within_bars(res, ref, "Predictor(GraphedGraphBins)")
    back = g.rerun_on_bf16(both)                                            # the bf16-pair re-capture carries the flag (split-3 head)
    assert g._fallback.bin_stats is True and back._fields[-2:] == ("depth_var", "confidence")
    assert tuple(back.depth_var.shape) == tuple(back.depth_pred.shape) and float(back.depth_var.min()) >= 0.0
    pp = PipelinedPredictor(m, args, frames.cuda(), slots=2, want=WANT3)
    assert m.bin_stats is True and all(gr.bin_stats for gr in pp.graphs)
    for i in range(3):
        pp.submit(frames.cuda(), first_image_id=i)
    got = pp.collect()
    assert len(got) == 3 and pp.rerun_steps == 0
    for r in got:
        assert torch.equal(r.depth, got[0].depth) and torch.equal(r.depth_std, got[0].depth_std) and torch.equal(r.confidence, got[0].confidence)
    _within_bars(got[0], ref, "PipelinedPredictor(2 slots)")
