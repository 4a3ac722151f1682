"""-m gpu: csrc/point_cloud.hip against the torch statement of tests/point_cloud_ref.py -- EQUALITY of the int32 views of every output
(the definition fixes every rounding), rows at or beyond counts[b] still holding the poison they were given -- and the predict path
that carries it."""
import os
import subprocess
import sys

import pytest
import torch

import gen
import point_cloud_ref as ref
from objcavit_amd.config import make_args

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
POISON, POISON_I = 0x7FC0DEAD, -7          # a NaN payload no computation produces; a pixel index / count no call produces
B, H, W = ref.CASE_B, ref.CASE_H, ref.CASE_W


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def poisoned(n, cap, pixel=True):
    out = {"points": torch.full((n, cap, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32),
           "counts": torch.full((n,), POISON_I, dtype=torch.int32, device="cuda"),
           "total": torch.full((n,), POISON_I, dtype=torch.int32, device="cuda")}
    if pixel:
        out["pixel"] = torch.full((n, cap), POISON_I, dtype=torch.int32, device="cuda")
    return out


def check(got, want, cap, what=""):
    """``got``: the wrapper's dict (or a PointCloud's _asdict), ``want``: the reference's per-image full clouds.  counts / total, the
    first min(total, cap) records and pixel indices EQUAL as int32; the tail untouched poison (where the buffers were poisoned)."""
    points, counts, total = got["points"].cpu(), got["counts"].cpu(), got["total"].cpu()
    pixel = None if got.get("pixel") is None else got["pixel"].cpu()
    assert points.dtype == torch.float32 and tuple(points.shape) == (len(want), cap, 4) and counts.dtype == total.dtype == torch.int32
    for b, c in enumerate(want):
        n = c.records.shape[0]
        assert int(total[b]) == n and int(counts[b]) == min(n, cap), (what, b, int(total[b]), int(counts[b]), n, cap)
        k = min(n, cap)
        assert torch.equal(points[b, :k].view(torch.int32), c.records[:k].view(torch.int32)), (what, b)
        assert bool((points[b, k:].view(torch.int32) == POISON).all()), (what, b, "tail written")
        if pixel is not None:
            assert torch.equal(pixel[b, :k], c.pixel[:k]) and bool((pixel[b, k:] == POISON_I).all()), (what, b)


# ---------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps():
    """Shared inputs, made once: per mask the depth on the host and the device; confidence, std, frames."""
    d = {m: ref.case_depth(m) for m in ref.MASKS}
    frames = ref.case_frames(1, B, H, W)
    return {"depth": d, "depth_dev": {m: v.cuda() for m, v in d.items()}, "K": ref.case_intrinsics(), "conf": ref.case_confidence(),
            "std": ref.case_std(), "frames": frames}


@pytest.mark.parametrize("stride", [(1, 1), (2, 3)])
@pytest.mark.parametrize("mask", ref.MASKS)
def test_points_equal_the_reference(ops, maps, mask, stride):
    """B = 3, 61 x 83 (three tiles at stride 1; odd, W % 4 != 0), a camera per image.  Capacity above, below and far below the total."""
    depth, K = maps["depth"][mask], maps["K"]
    want = ref.unproject(depth, K, stride, ref.NEAR, ref.FAR)
    totals = [c.records.shape[0] for c in want]
    if mask == "all":
        gh, gw = ops.unproject_grid(H, W, stride)
        assert totals == [gh * gw] * B
    if mask == "none":
        assert totals == [0] * B
    d_dev, k_dev = maps["depth_dev"][mask], K.cuda()
    caps = {max(totals) + 5, max(1, max(totals) // 2), max(1, max(totals) - 1), 1}
    for cap in sorted(caps):
        out = poisoned(B, cap)
        got = ops.depth_unproject(d_dev, k_dev, cap, stride=stride, near=ref.NEAR, far=ref.FAR, want_pixel=True, out=out)
        assert got["points"] is out["points"] and got["pixel"] is out["pixel"]
        check(got, want, cap, (mask, stride, cap))


@pytest.mark.parametrize("use_conf,use_std,use_frames", [(c, s, f) for c in (False, True) for s in (False, True) for f in (False, True)])
def test_every_combination_of_confidence_std_and_frames(ops, maps, use_conf, use_std, use_frames):
    """NaN confidence / std fail, values exactly at the thresholds and z exactly at near / far pass; byte 15 rounds half to even."""
    depth = maps["depth"]["random_half"].clone()
    depth[:, :, 5::11, 1::9] = ref.NEAR
    depth[:, :, 2::13, 4::8] = ref.FAR
    depth[:, :, 7::12, 3::10] = ref.FAR + 1e-6 * ref.FAR          # the next fp32 above far or so: out
    conf, std, frames = maps["conf"], maps["std"], maps["frames"]
    kw = dict(confidence=conf if use_conf else None, min_confidence=0.25, depth_std=std if use_std else None, max_std=0.75)
    want = ref.unproject(depth, maps["K"], (1, 1), ref.NEAR, ref.FAR, frames=frames if use_frames else None, **kw)
    z0 = want[0].records[:, 2]
    assert bool((z0 == ref.NEAR).any()) and bool((z0 == ref.FAR).any()) and bool((z0 <= ref.FAR).all())
    if use_conf:
        cv = conf[0, 0].reshape(-1)[want[0].pixel.long()]
        a = want[0].records.view(torch.uint8)[:, 15]
        assert bool((cv == 0.25).any()) and bool((cv == 0.5).any()) and bool((a[cv == 0.5] == 128).all()) and not torch.isnan(cv).any()
    if use_std:
        sv = std[0, 0].reshape(-1)[want[0].pixel.long()]
        assert bool((sv == 0.75).any()) and bool((sv <= 0.75).all())
    cap = H * W
    out = poisoned(B, cap)
    dev = {k: (None if v is None else v.cuda()) for k, v in kw.items() if isinstance(v, torch.Tensor) or v is None}
    got = ops.depth_unproject(depth.cuda(), maps["K"].cuda(), cap, near=ref.NEAR, far=ref.FAR, min_confidence=0.25, max_std=0.75,
                              frames=frames.cuda() if use_frames else None, want_pixel=True, out=out, **dev)
    check(got, want, cap, (use_conf, use_std, use_frames))
    if not use_frames:
        assert not got["points"].view(torch.uint8)[0, :got["counts"][0], 12:15].any()
    if not use_conf:
        assert bool((got["points"].view(torch.uint8)[0, :got["counts"][0], 15] == 255).all())


def test_special_values(ops, maps):
    """NaN, +-inf are never kept; -0.0 and negative depths are values like any other once near allows them (near = -inf)."""
    depth = maps["depth"]["all"].clone()
    depth[:, :, 0::5, 0::7] = float("nan")
    depth[:, :, 1::5, 1::7] = float("inf")
    depth[:, :, 2::5, 2::7] = float("-inf")
    depth[:, :, 3::5, 3::7] = -0.0
    depth[:, :, 4::5, 4::7] = -3.25
    depth[:, :, 0, 1] = 0.0
    for near, far in ((float("-inf"), float("inf")), (float("-inf"), 5.0), (0.0, float("inf")), (-3.25, -3.25)):
        want = ref.unproject(depth, maps["K"], (1, 1), near, far)
        z = torch.cat([c.records[:, 2] for c in want])
        assert torch.isfinite(z).all() and z.numel() > 0
        if near == float("-inf"):
            assert bool((z == -3.25).any()) and bool((z.view(torch.int32) == -2 ** 31).any())          # the bits of -0.0
        if near == 0.0:
            assert bool((z.view(torch.int32) == -2 ** 31).any()) and not bool((z < 0).any())          # 0.0 <= -0.0 holds
        cap = H * W
        out = poisoned(B, cap)
        check(ops.depth_unproject(depth.cuda(), maps["K"].cuda(), cap, near=near, far=far, want_pixel=True, out=out), want, cap, (near, far))


def test_images_without_a_usable_camera_keep_nothing(ops, maps):
    depth = torch.cat([maps["depth"]["checkerboard"], maps["depth"]["all"][:2]], 0)                     # B = 5
    K = torch.cat([maps["K"], maps["K"][:2]], 0)
    K[1, 0], K[2, 0], K[3, 2] = 0.0, float("nan"), float("inf")
    want = ref.unproject(depth, K, (1, 1), ref.NEAR, ref.FAR)
    assert [c.records.shape[0] > 0 for c in want] == [True, False, False, False, True]
    cap = H * W
    out = poisoned(5, cap)
    got = ops.depth_unproject(depth.cuda(), K.cuda(), cap, near=ref.NEAR, far=ref.FAR, want_pixel=True, out=out)
    check(got, want, cap)
    assert got["counts"].tolist()[1:4] == [0, 0, 0] and got["total"].tolist()[1:4] == [0, 0, 0]
    for i, v in ((1, -2.0), (1, float("inf")), (3, float("nan"))):                                     # fy < 0, fy = inf, cy = NaN
        k = maps["K"].clone()
        k[0, i] = v
        got = ops.depth_unproject(depth[:3].cuda(), k.cuda(), cap, near=ref.NEAR, far=ref.FAR, out=poisoned(3, cap, False))
        check(got, ref.unproject(depth[:3], k, (1, 1), ref.NEAR, ref.FAR), cap, (i, v))
        assert got["total"].tolist()[0] == 0


def test_frames_as_a_strided_view_with_a_window_origin(ops, maps):
    big = ref.case_frames(2, B, H + 9, W + 13)
    view_h, view_d = big[:, 3:H + 8, 5:W + 11], big.cuda()[:, 3:H + 8, 5:W + 11]                          # frames of (H + 5) x (W + 6)
    assert not view_d.is_contiguous()
    depth = maps["depth"]["checkerboard"]
    cap = 1500
    for stride, top, left in (((1, 1), 2, 3), ((2, 3), 5, 6), ((1, 1), 0, 0)):
        want = ref.unproject(depth, maps["K"], stride, ref.NEAR, ref.FAR, frames=view_h, top=top, left=left)
        out = poisoned(B, cap)
        got = ops.depth_unproject(maps["depth_dev"]["checkerboard"], maps["K"].cuda(), cap, stride=stride, near=ref.NEAR, far=ref.FAR,
                                  frames=view_d, top=top, left=left, want_pixel=True, out=out)
        check(got, want, cap, (stride, top, left))
    with pytest.raises(ValueError):
        ops.depth_unproject(maps["depth_dev"]["all"], maps["K"].cuda(), cap, frames=view_d, top=6, left=0)      # 6 + 61 > 66


def test_two_calls_are_bit_equal_and_image_index_fills_a_batch(ops, maps):
    depth, K = maps["depth_dev"]["random_half"], maps["K"].cuda()
    conf, frames = maps["conf"].cuda(), maps["frames"].cuda()
    cap = 3000
    kw = dict(near=ref.NEAR, far=ref.FAR, confidence=conf, min_confidence=0.25, frames=frames, want_pixel=True)
    a = ops.depth_unproject(depth, K, cap, out=poisoned(B, cap), **kw)
    b = ops.depth_unproject(depth, K, cap, out=poisoned(B, cap), **kw)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    # a batch of two filled by two calls (images 2 and 0 of the case, in that order) == one call on the two images
    pick = [2, 0]
    one = ops.depth_unproject(depth[pick].contiguous(), K[pick].contiguous(), cap, out=poisoned(2, cap), near=ref.NEAR, far=ref.FAR,
                              confidence=conf[pick].contiguous(), min_confidence=0.25, frames=frames[pick].contiguous(), want_pixel=True)
    out = poisoned(2, cap)
    for slot, i in enumerate(pick):
        got = ops.depth_unproject(depth[i:i + 1], K[i:i + 1], cap, out=out, image_index=slot, near=ref.NEAR, far=ref.FAR,
                                  confidence=conf[i:i + 1], min_confidence=0.25, frames=frames[i:i + 1], want_pixel=True)
        assert got["points"] is out["points"]
    for k in one:
        assert torch.equal(one[k].view(torch.int32), out[k].view(torch.int32)), k
    assert out["counts"].tolist() == [a["counts"][2].item(), a["counts"][0].item()]
    with pytest.raises(ValueError):
        ops.depth_unproject(depth[:1], K[:1], cap, out=out, image_index=2)
    # without ``out`` the buffers are new and the workspace is the stream's own
    fresh = ops.depth_unproject(depth, K, cap, **kw)
    n = fresh["counts"].tolist()
    for i in range(B):
        assert torch.equal(fresh["points"][i, :n[i]].view(torch.int32), a["points"][i, :n[i]].view(torch.int32))


def test_captured_graph_replays_with_a_new_map():
    """In a fresh child process (tests/point_cloud_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "point_cloud_graph_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


# ---------------------------------------------------------------------------
# the predict path
# ---------------------------------------------------------------------------
PH, PW = 352, 384          # the smallest shape tests/test_hip_predict.py runs a model on


def _frames(seed, n, h=PH, w=PW):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _model_of(dataset, h, w, seed):
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    args = make_args(model="graphbins", dataset=dataset, strategy="learned", language="clip", dimensions_train=[h, w], dimensions_test=[h, w])
    m = GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5)).eval()
    gen.load_into(m, seed, gen.PEAKY)
    return m.cuda(), args


@pytest.fixture(scope="module")
def model():
    return _model_of("nyu", PH, PW, 29)


def _equal_clouds(a, b, what=""):
    """Two PointClouds on the device: counts, total and the valid rows equal as int32."""
    assert torch.equal(a.counts, b.counts) and torch.equal(a.total, b.total), what
    assert a.points.shape == b.points.shape and (a.pixel is None) == (b.pixel is None)
    for i, n in enumerate(a.counts.tolist()):
        assert torch.equal(a.points[i, :n].view(torch.int32), b.points[i, :n].view(torch.int32)), (what, i)
        if a.pixel is not None:
            assert torch.equal(a.pixel[i, :n], b.pixel[i, :n]), (what, i)


def _against_reference(cloud, want, cap):
    counts = cloud.counts.tolist()
    for b, c in enumerate(want):
        n = c.records.shape[0]
        assert int(cloud.total[b]) == n and counts[b] == min(n, cap)
        assert torch.equal(cloud.points[b, :counts[b]].cpu().view(torch.int32), c.records[:counts[b]].view(torch.int32)), b
        if cloud.pixel is not None:
            assert torch.equal(cloud.pixel[b, :counts[b]].cpu(), c.pixel[:counts[b]]), b


def test_predictor_unprojects_its_own_map(ops, model):
    from objcavit_amd.point_cloud import PointCloud, intrinsics_from_focal
    from objcavit_amd.predict import Predictor, PredictResult
    m, args = model
    n = 2
    frames_h = _frames(61, n)
    frames = frames_h.cuda()
    K = intrinsics_from_focal([518.8579, 300.25], PH, PW)
    K[1, 2] += 3.25
    stride = (2, 3)
    plain = Predictor(m, args)(frames).depth.flatten()[::7].float()
    near, far = float(plain.quantile(0.2)), float(plain.quantile(0.8))          # a window that cuts some of this model's map and keeps some
    pr = Predictor(m, args, point_cloud=dict(stride=stride, near=near, far=far, pixel=True))
    res = pr(frames, intrinsics=K.cuda())
    assert isinstance(res, PredictResult) and isinstance(res.points, PointCloud) and res.objects is None and res.confidence is None
    gh, gw = ops.unproject_grid(PH, PW, stride)
    cap = gh * gw
    assert tuple(res.points.points.shape) == (n, cap, 4) and tuple(res.points.pixel.shape) == (n, cap)
    direct = ops.depth_unproject(res.depth, K.cuda(), cap, stride=stride, near=near, far=far, frames=frames, want_pixel=True)
    _equal_clouds(res.points, PointCloud(direct["points"], direct["counts"], direct["total"], direct["pixel"]))
    want = ref.unproject(res.depth.cpu(), K, stride, near, far, frames=frames_h)
    _against_reference(res.points, want, cap)
    assert 0 < int(res.points.total.sum()) < n * cap                               # the depth window cuts some and keeps some
    # a list of per-frame 4-vectors is the same K; the map is made for the cloud even when it is not wanted -- and then not handed out
    u16 = pr(frames, want=("depth_u16",), intrinsics=[K[0].tolist(), K[1]])
    assert u16.depth is None and u16.depth_u16 is not None
    _equal_clouds(u16.points, res.points)
    # without intrinsics, or without the keyword, there is no cloud and the result is the plain tuple
    assert type(pr(frames)) is PredictResult and Predictor(m, args)(frames, intrinsics=K.cuda()).points is None
    with pytest.raises(ValueError):
        pr(frames, intrinsics=K[:1].cuda())


def test_predictor_filters_by_confidence_and_std_and_runs_beside_the_object_readout(ops, model):
    import object_depth_ref
    from objcavit_amd.point_cloud import intrinsics_from_focal, object_positions
    from objcavit_amd.predict import Predictor
    m, args = model
    n = 2
    frames_h = _frames(63, n)
    frames = frames_h.cuda()
    K = intrinsics_from_focal([400.0, 450.5], PH, PW)
    everything = Predictor(m, args)(frames, want=("depth", "depth_std", "confidence"))
    minc = float(everything.confidence.median())
    maxs = float(everything.depth_std.float().quantile(0.7))
    cap = 40000                                                                    # below the grid's 135168: cut or not, as it falls
    pr = Predictor(m, args, point_cloud=dict(min_confidence=minc, max_std=maxs, capacity=cap, colour=False), object_depth={})
    boxes = [torch.tensor([[100.5, 80.0, 60.0, 40.0], [300.0, 200.0, 90.0, 120.0]]).cuda(), None]
    res = pr(frames, intrinsics=K.cuda(), boxes=boxes)
    assert res.confidence is None and res.depth_std is None                       # made for the filter, not asked for
    assert torch.equal(res.depth.view(torch.int32), everything.depth.view(torch.int32))
    ds = args[args.basic.dataset]
    want = ref.unproject(res.depth.cpu(), K, (1, 1), float(ds.min_depth), float(ds.max_depth), confidence=everything.confidence.cpu(),
                         min_confidence=minc, depth_std=everything.depth_std.cpu(), max_std=maxs)
    _against_reference(res.points, want, cap)
    total = res.points.total.tolist()
    assert all(0 < t < PH * PW for t in total) and res.points.pixel is None
    assert not res.points.points.view(torch.uint8)[0, :res.points.counts[0], 12:15].any()               # colour=False
    assert res.points.points.view(torch.uint8)[0, :res.points.counts[0], 15].min() >= round(255 * minc) - 1
    # the readout is what it is without the cloud, and its boxes get a position
    alone = Predictor(m, args, object_depth={})(frames, boxes=boxes)
    assert torch.equal(res.objects.table.view(torch.int32), alone.objects.table.view(torch.int32)) and alone.points is None
    xywh = torch.full((n, 2, 4), -1.0)
    xywh[0] = boxes[0].cpu()
    pos = object_positions(res.objects, xywh.cuda(), K.cuda())
    z = res.objects.table[0, :, res.objects.fields.index("q0.5")].cpu()
    assert tuple(pos.shape) == (n, 2, 3) and torch.equal(pos[0, :, 2].cpu(), z) and not pos[1].any()
    assert torch.allclose(pos[0, :, 0].cpu(), (xywh[0, :, 0] - 0.5 - K[0, 2]) / K[0, 0] * z, rtol=1e-6, atol=0)
    # with the maps wanted as well they are handed out, and the cloud is the same
    full = pr(frames, want=("depth", "confidence", "depth_std"), intrinsics=K.cuda())
    assert torch.equal(full.confidence, everything.confidence) and torch.equal(full.depth_std, everything.depth_std)
    _equal_clouds(full.points, res.points)


def test_predictor_takes_kitti_frames_of_different_sizes(ops):
    """Two frames of different sizes, each cropped to 352 x 1216 by its own origin: one launch pair per frame, the principal point of
    each shifted by ITS origin, the colour read from ITS window."""
    from objcavit_amd.predict import Predictor, kb_crop_origin
    KH, KW = 352, 1216
    m, args = _model_of("kitti", KH, KW, 27)
    frames_h = [_frames(31, 1, 375, 1242)[0], _frames(32, 1, 370, 1224)[0]]
    K = torch.tensor([[721.5377, 721.5377, 609.5593, 172.854], [718.856, 718.856, 607.1928, 185.2157]])
    stride = (4, 4)
    pr = Predictor(m, args, point_cloud=dict(stride=stride, pixel=True))
    ops.enable_timing(True)
    res = pr([f.cuda() for f in frames_h], intrinsics=K.cuda())
    timings = ops.timing_results()
    ops.enable_timing(False)
    assert timings["depth_unproject"][0] == 2                                      # one call (= one launch pair) per frame
    cap = (KH // 4) * (KW // 4)
    ds = args[args.basic.dataset]
    assert tuple(res.points.points.shape) == (2, cap, 4)
    for i, f in enumerate(frames_h):
        top, left = kb_crop_origin(*f.shape[:2])
        want = ref.unproject(res.depth[i:i + 1].cpu(), ref.shift_intrinsics(K[i:i + 1], top, left), stride, float(ds.min_depth), float(ds.max_depth),
                             frames=f.unsqueeze(0), top=top, left=left)
        one = type(res.points)(*(None if t is None else t[i:i + 1] for t in res.points))
        _against_reference(one, want, cap)
        assert int(res.points.total[i]) > 0
    assert [kb_crop_origin(*f.shape[:2]) for f in frames_h] == [(23, 13), (18, 4)]


def test_pipelined_predictor_clouds_equal_the_sequential_predictors(ops, model):
    """Four bs-1 steps over TWO slots (every slot is used twice before the collect): every step's cloud is bit-equal to the sequential
    ``Predictor``'s on a captured graph of the same shape, in submission order; a step without intrinsics has no cloud."""
    import predict_ref
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args = model
    N = 4
    frames = [_frames(70 + i, 1).cuda() for i in range(N)]
    Ks = [intrinsics_from_focal(400.0 + 25.0 * i, PH, PW).cuda() for i in range(N)]
    opts = dict(stride=(1, 2), near=0.5, far=7.0, min_confidence=0.05, pixel=True)
    boxes = [torch.tensor([[150.0, 100.0, 80.0, 60.0]]).cuda()]
    pp = PipelinedPredictor(m, args, frames[0], slots=2, want=("depth",), point_cloud=opts, object_depth={})
    assert len(pp.graphs) == 2
    example = predict_ref.frames_to_input(frames[0].cpu(), args, 0, 0, PH, PW)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_group=1, in_flight=2)
    seq = Predictor(g, args, point_cloud=opts, object_depth={})
    refs = []
    for i in range(N):
        r = seq(frames[i], intrinsics=Ks[i], boxes=boxes)
        refs.append((r.depth.clone(), type(r.points)(*(t.clone() for t in r.points)), r.objects.table.clone()))
    for i in range(N):
        pp.submit(frames[i], intrinsics=Ks[i] if i % 2 else [Ks[i][0].cpu()], boxes=boxes)
    pp.submit(frames[0])
    got = pp.collect()
    assert len(got) == N + 1 and pp.rerun_steps == 0 and got[N].points is None and got[N].objects is None
    for i in range(N):
        assert torch.equal(got[i].depth.view(torch.int32), refs[i][0].view(torch.int32)), i
        _equal_clouds(got[i].points, refs[i][1], i)
        assert torch.equal(got[i].objects.table.view(torch.int32), refs[i][2].view(torch.int32)), i
        assert got[i].confidence is None and got[i].bin_edges is None
        assert 0 < int(got[i].points.total[0]) <= PH * (PW // 2)
