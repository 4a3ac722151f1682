"""-m gpu: the predict path -- csrc/frame_ingest.hip and csrc/depth_finalize.hip against the reference statements of
tests/predict_ref.py, and ``Predictor`` / ``PipelinedPredictor`` (objcavit_amd/predict.py) against the validation step fed by hand."""
import numpy as np
import pytest
import torch

import gen
import predict_ref
from oracle import restate, validation_ref
from objcavit_amd.config import make_args
from util import max_rel, rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TOL = 2e-5              # the project's kernel tolerance


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def _frames(seed, B, Hs, Ws):
    return torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _table(args):
    from objcavit_amd.predict import normalisation_table
    return normalisation_table(args).cuda()


# ---------------------------------------------------------------------------
# frame ingest
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hs,Ws,window", [(1, 480, 640, None), (3, 375, 1242, "kb"), (2, 37, 53, (4, 5, 31, 45))])
@pytest.mark.parametrize("mirror", [False, True])
def test_frame_ingest_is_the_reference_statement_bit_for_bit(ops, B, Hs, Ws, window, mirror):
    from objcavit_amd.predict import kb_crop_origin
    args = make_args(dataset="kitti" if window == "kb" else "nyu")
    top, left, H, W = (0, 0, Hs, Ws) if window is None else (kb_crop_origin(Hs, Ws) + (352, 1216)) if window == "kb" else window
    f = _frames(11, B, Hs, Ws)
    ref = predict_ref.frames_to_input(f, args, top, left, H, W)
    got = ops.frame_ingest(f.cuda(), _table(args), top, left, (H, W), mirror_too=mirror)
    assert tuple(got.shape) == ((2 * B if mirror else B), 3, H, W) and got.dtype == torch.float32
    assert torch.equal(got[:B].cpu(), ref)
    if mirror:
        assert torch.equal(got[B:], got[:B].flip(3)) and torch.equal(got[B:].cpu(), ref.flip(3))
    assert torch.equal(ops.frame_ingest(f.cuda(), _table(args), top, left, (H, W), mirror_too=mirror), got)


def test_frame_ingest_every_value_strided_input_and_out_argument(ops):
    args = make_args()
    # every one of the 256 values in each channel (channel c holds the values rotated by 85 c: no two channels alike at a pixel)
    v = torch.arange(256, dtype=torch.int64)
    ex = torch.stack([(v + 85 * c) % 256 for c in range(3)], 1).to(torch.uint8).view(1, 8, 32, 3)
    got = ops.frame_ingest(ex.cuda(), _table(args), mirror_too=True)
    assert torch.equal(got[:1].cpu(), predict_ref.frames_to_input(ex, args, 0, 0, 8, 32))
    for c in range(3):
        assert torch.equal(got[0, c].flatten().cpu().sort().values, _table(args)[c].cpu().sort().values)
    # strided input: a window view into a larger buffer (rows and frames strided, origin at an odd byte), cropped again by the kernel
    big = _frames(12, 2, 50, 70)
    view = big.cuda()[:, 3:43, 5:61]                      # [2, 40, 56, 3], not contiguous
    assert not view.is_contiguous()
    ref = predict_ref.frames_to_input(big[:, 3:43, 5:61], args, 2, 3, 36, 48)
    got = ops.frame_ingest(view, _table(args), 2, 3, (36, 48), mirror_too=True)
    assert torch.equal(got[:2].cpu(), ref) and torch.equal(got[2:].cpu(), ref.flip(3))
    # out=: one batch tensor filled by one launch per frame, the mirrors in its second half
    out = torch.full((4, 3, 36, 48), float("nan"), device="cuda")
    for i in range(2):
        assert ops.frame_ingest(view[i:i + 1], _table(args), 2, 3, (36, 48), mirror_too=True, out=out, out_index=i) is out
    assert torch.equal(out, got)
    with pytest.raises(ValueError):
        ops.frame_ingest(view, _table(args), 2, 3, (36, 48), mirror_too=True, out=out, out_index=1)
    with pytest.raises(ValueError):
        ops.frame_ingest(view, _table(args), 10, 3, (36, 48))


# ---------------------------------------------------------------------------
# depth ingest
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1000.0, 256.0])
def test_depth_ingest_all_65536_values_equal_torch_fp32_division(ops, factor):
    """Settles whether the device's fp32 `/` (the library is built without fast-math flags) is torch's correctly rounded division."""
    v = torch.from_numpy(np.arange(65536, dtype=np.uint16)).view(1, 256, 256)
    ref = v.to(torch.int32).float() / factor
    got = ops.depth_ingest(v.cuda(), factor)
    assert tuple(got.shape) == (1, 1, 256, 256)
    diff = int((got.cpu().view(-1).view(torch.int32) != ref.view(-1).view(torch.int32)).sum())
    print(f"depth_ingest / {factor}: {diff} of 65536 values differ from torch CPU fp32 division")
    assert diff == 0
    # the scalar path (a width that is no multiple of 4) gives the same quotients
    got_s = ops.depth_ingest(v.cuda(), factor, 0, 0, (256, 255))
    assert torch.equal(got_s.cpu(), ref.view(1, 1, 256, 256)[..., :255])


def test_depth_ingest_crop_matches_the_frame_crop(ops):
    from objcavit_amd.predict import kb_crop_origin
    args = make_args(dataset="kitti")
    Hs, Ws = 375, 1242
    top, left = kb_crop_origin(Hs, Ws)
    g = torch.Generator().manual_seed(3)
    d = torch.from_numpy(torch.randint(0, 65536, (2, Hs, Ws), generator=g).numpy().astype(np.uint16))
    f = torch.zeros(2, Hs, Ws, 3, dtype=torch.uint8)
    f[..., 0] = (d.to(torch.int32) % 256).to(torch.uint8)      # the frame's red channel = the depth's low byte: same pixels, same window
    got = ops.depth_ingest(d.cuda(), 256.0, top, left, (352, 1216))
    assert torch.equal(got.cpu(), predict_ref.depth_to_metres(d, 256.0, top, left, 352, 1216))
    img = ops.frame_ingest(f.cuda(), _table(args), top, left, (352, 1216))
    low = (torch.round(got * 256.0).to(torch.int64) % 256)
    assert torch.equal(img[:, 0], _table(args)[0][low[:, 0]])
    out = torch.empty(3, 1, 37, 50, device="cuda")             # odd window, strided view, out=
    view = d.cuda()[:, 100:140, 200:260]
    ops.depth_ingest(view[1:], 1000.0, 1, 2, (37, 50), out=out, out_index=2)
    assert torch.equal(out[2:].cpu(), predict_ref.depth_to_metres(d[1:, 100:140, 200:260], 1000.0, 1, 2, 37, 50))


# ---------------------------------------------------------------------------
# depth finalize
# ---------------------------------------------------------------------------
def _pred(key, B, h, w, lo, hi, seed):
    """A smooth depth map that straddles both clamp bounds: a 5 x 7 grid of uniform control points over [lo - 0.1 (hi - lo),
    hi + 0.15 (hi - lo)] (its two ends included), interpolated to h x w in float64.  Smooth, as a depth map is, because of what the
    comparison with float64 can show: ATen's fp32 source coordinate fp32(scale) * X is off by up to 3e-5 of a pixel at the far end of a
    1216-wide row (6e-8 relative on the scale, half an ulp of 607 on the product), an error the fp32 torch statement shares and which
    is multiplied by the DIFFERENCE between neighbouring source pixels -- for white noise that alone exceeds the 2e-5 bar."""
    c = torch.rand(B, 1, 5, 7, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    c[:, :, 0, 0], c[:, :, -1, -1] = 0.0, 1.0
    u = torch.nn.functional.interpolate(c, (h, w), mode="bilinear", align_corners=True)
    return (lo - 0.1 * (hi - lo) + u * 1.25 * (hi - lo)).float()


@pytest.mark.parametrize("h,w,H,W,dmax", [(240, 320, 480, 640, 10.0), (176, 608, 352, 1216, 80.0), (17, 23, 45, 61, 10.0),
                                          # beyond the three sizes a model produces, the kernel's other routes: a down-scale whose source
                                          # window does not fit a tile's LDS, equal sizes (ATen's identity), rows of 20 pixels in groups of 8
                                          (200, 520, 16, 64, 10.0), (24, 32, 24, 32, 10.0), (6, 10, 12, 20, 10.0)])
@pytest.mark.parametrize("with_mirror", [False, True])
def test_depth_finalize_vs_float64_and_its_integer_forms(ops, h, w, H, W, dmax, with_mirror):
    B, dmin = 2, 0.001
    pred = _pred("p", B, h, w, dmin, dmax, 1)
    mirror = _pred("m", B, h, w, dmin, dmax, 2) if with_mirror else None
    table = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    scale = 256.0 if dmax > 10 else 1000.0
    res = ops.depth_finalize(pred.cuda(), dmin, dmax, (H, W), pred_mirror=None if mirror is None else mirror.cuda(),
                             want=("depth", "depth_u16", "rgb8"), u16_scale=scale, colormap=table.cuda(), vmin=dmin, vmax=dmax)
    d = res["depth"]
    assert tuple(d.shape) == (B, 1, H, W) and tuple(res["depth_u16"].shape) == (B, H, W) and tuple(res["rgb8"].shape) == (B, H, W, 3)
    ref = predict_ref.final_depth(pred, mirror, dmin, dmax, H, W, torch.float64)
    err = rel_dev(d, ref)                                              # max |difference| / max |reference|: the measure of every 2e-5 bar here
    print(f"depth_finalize {h}x{w} -> {H}x{W} mirror={with_mirror}: deviation from float64 {err:.3e}")
    assert err < TOL
    assert bool((pred < dmin).any()) and bool((pred > dmax).any())           # the predictions straddle both clamp bounds
    assert float(d.min()) >= dmin * (1 - 1e-6) and float(d.max()) <= dmax * (1 + 1e-6)
    # the integer forms are functions of the kernel's own fp32 map, bit for bit
    assert torch.equal(res["depth_u16"].cpu().to(torch.int32), predict_ref.to_u16(d[:, 0], scale))
    assert torch.equal(res["rgb8"].cpu(), predict_ref.to_rgb8(d[:, 0], table, dmin, dmax))
    # each output alone is the same launch's output; two calls are bit-equal
    again = ops.depth_finalize(pred.cuda(), dmin, dmax, (H, W), pred_mirror=None if mirror is None else mirror.cuda(),
                               want=("depth", "depth_u16", "rgb8"), u16_scale=scale, colormap=table.cuda(), vmin=dmin, vmax=dmax)
    for k in res:
        assert torch.equal(again[k].view(torch.uint8), res[k].view(torch.uint8)), k
    only = ops.depth_finalize(pred.cuda(), dmin, dmax, (H, W), pred_mirror=None if mirror is None else mirror.cuda(), want=("depth_u16",),
                              u16_scale=scale)
    assert set(only) == {"depth_u16"} and torch.equal(only["depth_u16"].view(torch.uint8), res["depth_u16"].view(torch.uint8))


@pytest.mark.parametrize("h,w,H,W", [(17, 23, 33, 45), (17, 23, 45, 61), (24, 32, 48, 64)])
def test_depth_finalize_non_finite_values_follow_the_fp32_torch_statement(ops, h, w, H, W):
    """Values only: NaN / +-inf planted in the predictions (interior, a corner, a pixel that output pixels sit on exactly).  A NaN
    source pixel turns every output pixel that has it as a tap -- zero-weight taps included, ATen computes 0 * NaN -- into
    min_depth; +-inf are clamped to the bounds before the resize.  (17 x 23 -> 33 x 45 has the exact scale 1 / 2: the output pixels
    (14 .. 17, 20 .. 23) have source pixel (8, 11) as a tap, (14, 20) through two zero weights.)"""
    dmin, dmax = 0.001, 10.0
    g = torch.Generator().manual_seed(9)
    pred = torch.rand(2, 1, h, w, generator=g) * 8.0 + 1.0            # strictly inside the bounds: min_depth can only come from a NaN or -inf
    mirror = torch.rand(2, 1, h, w, generator=g) * 8.0 + 1.0
    nan, inf = float("nan"), float("inf")
    pred[0, 0, 8, 11] = nan
    pred[0, 0, 0, 0] = nan
    pred[1, 0, h - 1, w - 1] = nan
    pred[1, 0, 3, 15] = inf
    pred[1, 0, 10, 4] = -inf
    pred[0, 0, h - 1, 0] = inf
    mirror[0, 0, 5, 2] = nan                                           # lands on column w - 3 of the averaged map
    mirror[1, 0, 12, 20] = -inf
    for mir in (None, mirror):
        ref = predict_ref.final_depth(pred, mir, dmin, dmax, H, W, torch.float32)
        got = ops.depth_finalize(pred.cuda(), dmin, dmax, (H, W), pred_mirror=None if mir is None else mir.cuda())["depth"].cpu()
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())
        lo = torch.tensor(dmin, dtype=torch.float32)
        assert torch.equal(got == lo, ref == lo)                       # the same set of pixels equals min_depth
        assert int((ref == lo).sum()) >= 16 + 1 + 1
        assert max_rel(got, ref.double()) < TOL
        if (H, W) == (33, 45):
            assert bool((got[0, 0, 14:18, 20:24] == lo).all()) and float(got[0, 0, 13, 20]) != dmin and float(got[0, 0, 14, 19]) != dmin


@pytest.mark.parametrize("dataset,h,w,H,W", [("nyu", 240, 320, 480, 640), ("kitti", 176, 608, 352, 1216)])
def test_materialised_map_gives_the_metric_kernels_numbers(ops, dataset, h, w, H, W):
    """The eight metrics in float64 on the host from the map ``depth_finalize`` wrote (ground-truth mask and the crop box of
    validation.crop_box: NYU Eigen, KITTI Garg) against ``depth_metrics`` on the same inputs, which forms that map per pixel."""
    from objcavit_amd.validation import crop_box
    args = make_args(dataset=dataset)
    ds = args[dataset]
    dmin, dmax, B = float(ds.min_depth), float(ds.max_depth), 2
    pred, mirror = _pred("p", B, h, w, dmin, dmax, 5), _pred("m", B, h, w, dmin, dmax, 6)
    gt = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(7)) * 1.2 * dmax - 0.1 * dmax      # invalid pixels at both ends
    box = crop_box(args, H, W)
    assert box is not None
    d = ops.depth_finalize(pred.cuda(), dmin, dmax, (H, W), pred_mirror=mirror.cuda())["depth"].cpu()
    rec = ops.depth_metrics(pred.cuda(), gt.cuda(), dmin, dmax, crop=box, pred_mirror=mirror.cuda()).cpu().double()
    mask = (gt > dmin) & (gt <= dmax)
    ev = torch.zeros(H, W, dtype=torch.bool)
    ev[box[0]:box[1], box[2]:box[3]] = True
    mask = mask & ev
    for b in range(B):
        m = mask[b]
        n = int(m.sum())
        f = validation_ref.finish(validation_ref.pixel_sums(d[b][m], gt[b][m]))
        assert n > 1000 and float(rec[b, 8]) == n
        for i, k in enumerate(validation_ref.METRICS):
            dev = abs(float(rec[b, i]) - f[k])
            bar = TOL * abs(f[k]) if i < 5 else TOL + 2.0 / n           # delta metrics: a pixel on a threshold may fall either way
            print(f"{dataset} image {b} {k}: host {f[k]:.8g} kernel {float(rec[b, i]):.8g}")
            assert dev <= bar, (k, dev, bar)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _model(model, dataset, H, W, seed):
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    args = make_args(model=model, dataset=dataset, strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    m = (AdaBins(args) if model == "adabins" else GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5))).eval()
    sd = gen.load_into(m, seed, gen.PEAKY)
    return m.cuda(), sd, args


def _gt(B, H, W, seed, dmax=10.0):
    return torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(seed)) * 0.9 * dmax + 0.05 * dmax


def _by_hand(ops, m, args, img, gt, flip_tta=True, first_image_id=0):
    """Route 2: the validation step run on the reference-statement input ``img`` (fp32, host), then the final map from the same
    forward's outputs (issued a second time: the forward is deterministic)."""
    from objcavit_amd.validation import ValidationStep
    img = img.cuda()
    step = ValidationStep(m, args, flip_tta=flip_tta)
    ds = args[args.basic.dataset]
    rec, _ = step(img, gt.cuda(), first_image_id=first_image_id)
    rec = rec.clone()
    if flip_tta:
        out, mirror = step._forward_pair(img)
    else:
        out, mirror = step._call(img), None
    depth = ops.depth_finalize(out.depth_pred.contiguous(), float(ds.min_depth), float(ds.max_depth), tuple(img.shape[2:]),
                               pred_mirror=None if mirror is None else mirror.contiguous())["depth"]
    return rec, depth


@pytest.mark.parametrize("model", ["graphbins", "adabins"])
def test_predictor_equals_the_validation_step_fed_by_hand(ops, model):
    from objcavit_amd.predict import Predictor
    H, W, B = 480, 640, 2
    m, _, args = _model(model, "nyu", H, W, 23)
    frames, gt = _frames(21, B, H, W), _gt(B, H, W, 22)
    res = Predictor(m, args)(frames.cuda(), gt.cuda(), first_image_id=5, want=("depth", "depth_u16"))
    rec, depth = _by_hand(ops, m, args, predict_ref.frames_to_input(frames, args, 0, 0, H, W), gt, first_image_id=5)
    assert tuple(res.records.shape) == (B, 10) and torch.equal(res.records, rec)
    assert tuple(res.depth.shape) == (B, 1, H, W) and torch.equal(res.depth, depth)
    assert torch.equal(res.depth_u16.cpu().to(torch.int32), predict_ref.to_u16(res.depth[:, 0], 1000.0)) and res.rgb8 is None
    assert res.bin_edges is not None and res.bin_edges.shape[0] == B
    # without TTA: the reference's own predict step (GraphBinsLM.py:295-301) = the single forward
    res1 = Predictor(m, args, flip_tta=False)(frames.cuda(), gt.cuda(), first_image_id=5)
    rec1, depth1 = _by_hand(ops, m, args, predict_ref.frames_to_input(frames, args, 0, 0, H, W), gt, flip_tta=False, first_image_id=5)
    assert torch.equal(res1.records, rec1) and torch.equal(res1.depth, depth1) and not torch.equal(res1.depth, res.depth)
    # uint16 ground truth goes through depth_ingest: the records of the fp32 map it stands for
    gt16 = torch.from_numpy(torch.round(gt[:, 0] * 1000.0).numpy().astype(np.uint16))
    res16 = Predictor(m, args)(frames.cuda(), gt16.cuda(), first_image_id=5, want=())
    rec16, _ = _by_hand(ops, m, args, predict_ref.frames_to_input(frames, args, 0, 0, H, W), predict_ref.depth_to_metres(gt16, 1000.0, 0, 0, H, W),
                         first_image_id=5)
    assert res16.depth is None and torch.equal(res16.records, rec16)


def test_predictor_takes_kitti_frames_of_different_sizes(ops):
    """A list of differently sized frames, each cropped to 352 x 1216 by its own origin: bit for bit the batch the reference
    statement builds frame by frame, and the per-frame calls' result up to batch-size-dependent kernel dispatch (split-K, tile shapes:
    1e-4, the bar tests/test_hip_objects.py holds the joint forward against two calls to)."""
    from objcavit_amd.predict import Predictor, kb_crop_origin
    H, W = 352, 1216
    m, _, args = _model("graphbins", "kitti", H, W, 27)
    frames = [_frames(31, 1, 375, 1242)[0], _frames(32, 1, 370, 1224)[0]]
    gt = _gt(2, H, W, 33, 80.0)
    pr = Predictor(m, args)
    res = pr([f.cuda() for f in frames], gt.cuda())
    windows = [kb_crop_origin(*f.shape[:2]) + (H, W) for f in frames]
    assert windows == [(23, 13, H, W), (18, 4, H, W)]
    img = torch.cat([predict_ref.frames_to_input(f.unsqueeze(0), args, *w) for f, w in zip(frames, windows)], 0)
    rec, depth = _by_hand(ops, m, args, img, gt)
    assert torch.equal(res.records, rec) and torch.equal(res.depth, depth)
    for i, f in enumerate(frames):
        one = pr(f.cuda().unsqueeze(0), gt[i:i + 1].cuda(), first_image_id=i)
        assert max_rel(res.depth[i:i + 1], one.depth) < 1e-4
        assert torch.equal(res.records[i, 8:], one.records[0, 8:]) and rel_dev(res.records[i, :8], one.records[0, :8]) < 1e-4


def test_pipelined_predictor_equals_sequential_predictor_on_a_captured_graph(ops, monkeypatch):
    """Six bs-1 steps over four slots == six sequential ``Predictor`` calls on a captured graph of the same shape, bit for bit
    (replay == eager bit for bit; both sides replay a GraphedGraphBins, so the dispatch is identical).  And the
    point of the ingest: a submit hands the graph its OWN static input -- no flip, no cat, no copy_ of the image."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    H, W, N = 352, 384, 6
    m, _, args = _model("graphbins", "nyu", H, W, 29)
    frames = [_frames(40 + i, 1, H, W).cuda() for i in range(N)]
    gts = [_gt(1, H, W, 50 + i).cuda() for i in range(N)]
    table = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    want = ("depth", "depth_u16", "rgb8")
    pp = PipelinedPredictor(m, args, frames[0], want=want, colormap=table)
    assert len(pp.graphs) == 4 and tuple(pp.graphs[0].static_image.shape) == (2, 3, H, W)
    example = predict_ref.frames_to_input(frames[0], args, 0, 0, H, W)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_group=1, in_flight=4)
    seq = Predictor(g, args, colormap=table)
    ref = []
    for i in range(N):
        r = seq(frames[i], gts[i], first_image_id=i, want=want)
        ref.append(type(r)(*[None if v is None else v.clone() for v in r]))
    assert g.trips == 0
    for i in range(N):
        pp.submit(frames[i], gts[i], first_image_id=i)
    got = pp.collect()
    assert len(got) == N and pp.rerun_steps == 0 and pp.collect() == []
    for i in range(N):
        for k in ("depth", "depth_u16", "rgb8", "records"):
            assert torch.equal(getattr(got[i], k).view(torch.uint8), getattr(ref[i], k).view(torch.uint8)), (i, k)
    assert tuple(pp.records(got).shape) == (N, 10)
    # launches of one submit: the image reaches the graph through its own static tensor
    statics = {gr.static_image.data_ptr() for gr in pp.graphs}
    seen = []
    real_call, real_copy = GraphedGraphBins.__call__, torch.Tensor.copy_

    def call(self, image, *a, **kw):
        seen.append(image.data_ptr() == self.static_image.data_ptr())
        return real_call(self, image, *a, **kw)

    def copy_(self, *a, **kw):
        if self.data_ptr() in statics:
            raise AssertionError("copy_ into a slot's static image during submit")
        return real_copy(self, *a, **kw)

    def forbidden(*a, **kw):
        raise AssertionError("flip / cat during submit")

    monkeypatch.setattr(GraphedGraphBins, "__call__", call)
    monkeypatch.setattr(torch.Tensor, "copy_", copy_)
    monkeypatch.setattr(torch.Tensor, "flip", forbidden)
    monkeypatch.setattr(torch, "cat", forbidden)
    ops.enable_timing(True)
    pp.submit(frames[1], gts[1], first_image_id=1)
    monkeypatch.undo()
    counts = {k: v[0] for k, v in ops.timing_results().items()}
    ops.enable_timing(False)
    assert seen == [True]
    assert counts.get("frame_ingest") == 1 and counts.get("depth_finalize") == 1 and counts.get("depth_metrics") == 1, counts
    again = pp.collect()
    assert len(again) == 1 and torch.equal(again[0].depth, ref[1].depth) and torch.equal(again[0].records, ref[1].records)


def test_pipelined_predictor_reruns_a_tripped_step_at_collect(ops):
    """The pattern of tests/test_hip_fp16_route.py: a network whose decoder carries a large intermediate, calibrated on a tame batch;
    the same batch x 8 takes that intermediate beyond the fp16 pairs' guarded range, the step's guard word trips, and collect() re-runs
    it from the kept frames on the bf16-pair capture: finite, within 1e-3 of the CPU oracle's final map; its neighbours untouched.
    The x 8 is meant for the NORMALISED batch (every layer up to the bin softmax is positively homogeneous: the oracle bar is a
    statement about that scale, see the route test).  With uint8 frames and x = (v / f - mean) / std that takes frame values
    v_big = 8 v - 7 mean f: under image_norm_factor f = 64 the offsets 7 mean f = 217.3, 204.3, 181.9 round to integers (what the
    rounding leaves, < 0.03 after normalisation, is the only departure from an exact x 8), and v in [c / 8, (255 + c) / 8] keeps
    v_big a uint8."""
    from test_hip_fp16_route import GUARD_SCALE, _guard_alpha, _guard_model
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    H, W, F = 352, 384, 64.0
    assert GUARD_SCALE == 8.0
    off = [round(7 * mean * F) for mean in predict_ref.MEAN]
    assert off == [217, 204, 182]

    def tame_frame(seed):
        g = torch.Generator().manual_seed(seed)
        return torch.stack([torch.randint(-(-c // 8), (255 + c) // 8 + 1, (1, H, W), generator=g) for c in off], 3).to(torch.uint8)

    tame = [tame_frame(60 + i) for i in range(4)]
    frames = [f.clone() for f in tame]
    big16 = frames[2].to(torch.int32) * 8 - torch.tensor(off, dtype=torch.int32)
    assert int(big16.min()) >= 0 and int(big16.max()) <= 255
    frames[2] = big16.to(torch.uint8)
    args0 = make_args(strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W], image_norm_factor=F)
    alpha = _guard_alpha(ops, predict_ref.frames_to_input(tame[0], args0, 0, 0, H, W), H, W)
    m, sd, args = _guard_model(H, W, alpha=alpha)
    args["nyu"]["image_norm_factor"] = F
    m(predict_ref.frames_to_input(tame[0], args, 0, 0, H, W).cuda())         # the model's first batch: calibrates the fp16 pairs
    ops.ROUTE_REPORT.clear()
    pp = PipelinedPredictor(m, args, tame[0].cuda(), slots=2, flip_tta=False)
    for i in range(4):
        pp.submit(frames[i].cuda(), first_image_id=i)
    got = pp.collect()
    assert pp.rerun_steps == 1 and "bf16" in ops.ROUTE_REPORT.get("range_guard", ""), (pp.rerun_steps, ops.ROUTE_REPORT)
    assert all(bool(torch.isfinite(r.depth).all()) for r in got)
    big = predict_ref.frames_to_input(frames[2], args, 0, 0, H, W)
    assert float((big - 8.0 * predict_ref.frames_to_input(tame[2], args, 0, 0, H, W)).abs().max()) < 0.03
    feats, boxes, _ = m.object_provider(big.cuda())
    ref_d, _ = restate.graphbins_forward(big, [f.cpu() for f in feats], [b.cpu() for b in boxes], sd, 0.001, 10.0, strategy="learned")
    ref = predict_ref.final_depth(ref_d, None, 0.001, 10.0, H, W, torch.float64)
    err = max_rel(got[2].depth, ref)
    print(f"tripped step vs CPU oracle: {err:.3e}")
    assert err < 1e-3
    seq = Predictor(m, args, flip_tta=False)                                  # eager: the model guards itself
    for i in (0, 1, 3):
        assert max_rel(got[i].depth, seq(frames[i].cuda()).depth) < 1e-5


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_pipelined_predictor_takes_the_callers_objects(ops):
    """Live objects through the predictor: a graph per slot captured with ``object_capacity``, the objects of [frame | mirrored frame]
    handed to ``submit`` -- the model's provider is then not asked.  Three steps on two slots (one slot is used twice before
    ``collect``) == the sequential ``Predictor`` on a graph of the same capacity, whose provider returns the same objects, bit for bit."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    from test_hip_objects import _objects
    H, W, N, CAP = 352, 384, 3, 24

    class Scripted:                                         # a "detector" that returns what the test wrote into ``now``
        now, calls = None, 0

        def __call__(self, image):
            self.calls += 1
            return [f.to(image.device) for f in self.now[0]], [b.to(image.device) for b in self.now[1]], None

    m, _, args = _model("graphbins", "nyu", H, W, 29)
    prov = m.object_provider = Scripted()
    objs = [_objects([3 + 5 * i, 1 + 7 * i], 70 + i, H, W) for i in range(N)]            # ragged, different for frame and mirror
    frames = [_frames(80 + i, 1, H, W).cuda() for i in range(N)]
    gts = [_gt(1, H, W, 90 + i).cuda() for i in range(N)]
    prov.now = objs[0]
    example = predict_ref.frames_to_input(frames[0], args, 0, 0, H, W)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_capacity=CAP, object_group=1, in_flight=2)
    seq = Predictor(g, args)
    ref = []
    for i in range(N):
        prov.now = objs[i]
        r = seq(frames[i], gts[i], first_image_id=i)
        ref.append((r.depth.clone(), r.records.clone()))
    assert g.trips == 0
    pp = PipelinedPredictor(m, args, frames[0], slots=2, object_capacity=CAP)
    assert len(pp.graphs) == 2 and all(gr.objects is not None for gr in pp.graphs)
    prov.now, asked = None, prov.calls
    for i in range(N):
        pp.submit(frames[i], gts[i], first_image_id=i, object_features=[f.cuda() for f in objs[i][0]],
                  object_xywh_list=[b.cuda() for b in objs[i][1]])
    got = pp.collect()
    assert len(got) == N and pp.rerun_steps == 0 and prov.calls == asked
    for i in range(N):
        assert torch.equal(got[i].depth, ref[i][0]) and torch.equal(got[i].records, ref[i][1]), i
    assert torch.equal(pp.records(got), torch.cat([r[1] for r in ref], 0))
    assert not torch.equal(ref[0][0], ref[1][0])


class _Fp16Only:
    """A captured graph without its fallback: what the fp16 pairs alone make of a step (no ``checked``, so a sequential step replays it
    and reads no guard word)."""
    images_are_independent = True

    def __init__(self, g):
        self.g, self.static_image, self.object_group = g, g.static_image, g.object_group

    def __call__(self, image):
        return self.g(image)


@pytest.fixture(scope="module")
def guard_steps(ops):
    """Five bs-1 steps for a network whose decoder carries a large intermediate (tests/test_hip_fp16_route.py), step 2 the tame frame
    x 8 after normalisation (see ``test_pipelined_predictor_reruns_a_tripped_step_at_collect`` for the uint8 arithmetic)."""
    from test_hip_fp16_route import GUARD_SCALE, _guard_alpha, _guard_model
    H, W, F = 352, 384, 64.0
    assert GUARD_SCALE == 8.0
    off = [round(7 * mean * F) for mean in predict_ref.MEAN]
    frames = []
    for i in range(5):
        g = torch.Generator().manual_seed(60 + i)
        frames.append(torch.stack([torch.randint(-(-c // 8), (255 + c) // 8 + 1, (1, H, W), generator=g) for c in off], 3).to(torch.uint8))
    args0 = make_args(strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W], image_norm_factor=F)
    alpha = _guard_alpha(ops, predict_ref.frames_to_input(frames[0], args0, 0, 0, H, W), H, W)
    m, _, args = _guard_model(H, W, alpha=alpha)
    args["nyu"]["image_norm_factor"] = F
    m(predict_ref.frames_to_input(frames[0], args, 0, 0, H, W).cuda())       # the model's first batch: calibrates the fp16 pairs
    big = frames[2].to(torch.int32) * 8 - torch.tensor(off, dtype=torch.int32)
    assert int(big.min()) >= 0 and int(big.max()) <= 255
    frames[2] = big.to(torch.uint8)
    gts = [_gt(1, H, W, 170 + i).cuda() for i in range(5)]
    return m, args, [f.cuda() for f in frames], [predict_ref.frames_to_input(f, args, 0, 0, H, W).cuda() for f in frames], gts


@pytest.mark.parametrize("which", ["PipelinedValidation", "PipelinedPredictor"])
def test_slot_pipeline_reruns_one_tripped_step_and_forgets_collected_steps(ops, guard_steps, which):
    """The same scenario through both pipelines: five steps on two slots, step 2 beyond the fp16 pairs' guarded range.  The results
    come back in submission order; one step is re-run at ``collect()`` and only its result differs from what the fp16-pair graph alone
    gives (a sequential step on ``_Fp16Only``: same graph shape, same slots in flight, hence the same kernels -- bit for bit); a
    second ``collect()`` returns the class's empty form; a further submit + collect round returns that one step."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    from objcavit_amd.validation import PipelinedValidation, ValidationStep
    m, args, frames, imgs, gts = guard_steps
    g = _Fp16Only(GraphedGraphBins(m, torch.cat([imgs[0], imgs[0].flip(3)], 0), object_group=1, in_flight=2))
    if which == "PipelinedValidation":
        seq, pipe, inputs = ValidationStep(g, args), PipelinedValidation(m, args, imgs[0], slots=2), imgs
        fp16 = [seq(imgs[i], gts[i], first_image_id=i)[0].clone() for i in range(5)]

        def steps(collected):                               # -> per step, the tensors to compare
            assert isinstance(collected, torch.Tensor) and collected.device.type == "cuda"
            return [(r,) for r in collected.split(1)]
        empty = lambda c: isinstance(c, torch.Tensor) and tuple(c.shape) == (0, 10) and c.device.type == "cpu"
        fp16 = [(r,) for r in fp16]
    else:
        seq, pipe, inputs = Predictor(g, args), PipelinedPredictor(m, args, frames[0], slots=2), frames
        fp16 = []
        for i in range(5):
            r = seq(frames[i], gts[i], first_image_id=i)
            fp16.append((r.records.clone(), r.depth.clone()))

        def steps(collected):
            assert isinstance(collected, list)
            return [(r.records, r.depth) for r in collected]
        empty = lambda c: c == []
    assert len(pipe.graphs) == 2 and empty(pipe.collect())
    for i in range(5):
        pipe.submit(inputs[i], gts[i], first_image_id=i)
    got = steps(pipe.collect())
    assert len(got) == 5 and pipe.rerun_steps == 1
    assert [int(s[0][0, 9]) for s in got] == list(range(5))                 # image ids: submission order
    for i in range(5):
        same = all(_same(a, b) for a, b in zip(got[i], fp16[i]))
        assert same == (i != 2), i
        assert all(bool(torch.isfinite(t).all()) for t in got[i]), i
    assert empty(pipe.collect()) and pipe.rerun_steps == 1
    pipe.submit(inputs[1], gts[1], first_image_id=1)
    again = steps(pipe.collect())
    assert len(again) == 1 and all(_same(a, b) for a, b in zip(again[0], fp16[1])) and pipe.rerun_steps == 1
    assert empty(pipe.collect())
