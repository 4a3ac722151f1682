"""-m gpu: csrc/object_metrics.hip against the CPU statement of tests/object_metrics_ref.py -- n_valid and delta_k * n_valid EXACT (the
inputs keep clear of the delta thresholds: object_metrics_ref.guard), rows that must be zero exactly zero, every column within the
project's TOL of the float64 reference -- its invariants against ``depth_metrics`` on the same inputs, and the predict path that
carries it."""
import os
import subprocess
import sys

import pytest
import torch

import gen
import object_depth_ref as odr
import object_metrics_ref as ref
import predict_ref
from objcavit_amd.config import make_args
from util import rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2e-5          # the project's tolerance for fp32 per-pixel arithmetic against float64 (tests/test_hip_validation.py)
DMIN, DMAX = ref.MIN_DEPTH, ref.MAX_DEPTH


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def dev(t):
    return None if t is None else t.cuda()


def _check(got, want, what):
    """A device table [..., 10] against the float64 reference: counts and delta counts equal, zero rows zero, columns within TOL; no
    element left unwritten."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.float32 and not torch.isnan(got).any(), what
    assert torch.equal(got[..., 8].double(), want[..., 8]), (what, got[..., 8], want[..., 8])
    assert torch.equal(ref.delta_counts(got), ref.delta_counts(want)), what
    empty = want[..., 8] == 0
    assert not got[empty].any(), (what, got[empty])
    for c in range(ref.FIELDS):
        d = rel_dev(got[..., c], want[..., c])
        print(f"{what} column {c}: rel_dev {d:.3g}")
        assert d < TOL, (what, c, d)


def _run(ops, pred, mirror, gt, xywh, counts, shrink=1.0, crop=None, what=""):
    """One call held to the reference and to the invariants that tie it to ``depth_metrics``; -> (boxes, regions) on the device."""
    assert ref.band_size(pred, gt, pred_mirror=mirror) == 0
    want_b, want_r = ref.object_metrics(pred, gt, xywh[..., :4], counts, crop=crop, pred_mirror=mirror, shrink=shrink)
    p, m, g, x, c = dev(pred), dev(mirror), dev(gt), dev(xywh), dev(counts)
    out = torch.full(tuple(xywh.shape[:2]) + (10,), float("nan"), device="cuda")
    boxes, regions = ops.object_metrics(p, g, x, c, DMIN, DMAX, crop=crop, pred_mirror=m, shrink=shrink, out=out)
    assert boxes is out and tuple(regions.shape) == (gt.shape[0], 2, 10)
    _check(boxes, want_b, (what, "boxes"))
    _check(regions, want_r, (what, "regions"))
    # the two regions partition what depth_metrics counts, and recombine to its record
    image = ops.depth_metrics(p, g, DMIN, DMAX, crop=crop, pred_mirror=m).cpu()
    assert torch.equal(regions[:, 0, 8].cpu() + regions[:, 1, 8].cpu(), image[:, 8]), (what, regions[:, :, 8], image[:, 8])
    whole = ref.recombine(regions.cpu())
    for col in range(8):
        assert rel_dev(whole[:, col], image[:, col]) < TOL, (what, col)
    # bit-equal on repeat; the region pass does not touch the boxes
    again_b, again_r = ops.object_metrics(p, g, x, c, DMIN, DMAX, crop=crop, pred_mirror=m, shrink=shrink)
    assert torch.equal(again_b.view(torch.int32), boxes.view(torch.int32)) and torch.equal(again_r.view(torch.int32), regions.view(torch.int32))
    alone, none = ops.object_metrics(p, g, x, c, DMIN, DMAX, crop=crop, pred_mirror=m, shrink=shrink, regions=False)
    assert none is None and torch.equal(alone.view(torch.int32), boxes.view(torch.int32))
    return boxes, regions


def _view6(name):
    """The box set in rows of six floats, as the strided [3, 6, 4] view the kernel must read with the row stride."""
    xywh6, counts = odr.case_boxes(name, 6)
    return xywh6, counts


@pytest.fixture(scope="module")
def maps():
    """{form: (pred, pred_mirror, gt)}: made (and guarded) once, read by every test."""
    return {"resize": ref.case_maps(seed=1), "identity": ref.case_maps(h=odr.CASE_H, w=odr.CASE_W, mirror=False, seed=2),
            "special": ref.case_maps(seed=3, special=True, dead_image=1)}


# ---------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("boxes", sorted(odr.BOX_SETS))
@pytest.mark.parametrize("form", ["resize", "identity"])
def test_records_equal_the_reference(ops, maps, form, boxes):
    """B = 3, gt 37 x 53 (odd, W % 4 != 0, one tile); pred 19 x 27 with mirror, and 37 x 53 without (the identity short-cut); shrink 0.3
    (half = 0.15: no power of two) catches a contracted half * w; rows of six floats read through a strided view; rows at or beyond
    counts[b] hold a valid box and must be zero; ``out`` is NaN before the call."""
    pred, mirror, gt = maps[form]
    xywh6, counts = _view6(boxes)
    for shrink in (1.0, 0.3):
        got, _ = _run(ops, pred, mirror, gt, xywh6, counts, shrink, what=(form, boxes, shrink))
        for b, c in enumerate(counts.tolist()):
            assert not got[b, c:].any()
        view = xywh6.cuda()[:, :, :4]
        assert not view.is_contiguous()
        strided, _ = ops.object_metrics(dev(pred), dev(gt), view, dev(counts), DMIN, DMAX, pred_mirror=dev(mirror), shrink=shrink, regions=False)
        assert torch.equal(strided.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("boxes", sorted(odr.BOX_SETS))
@pytest.mark.parametrize("crop", [None, "garg"])
def test_special_taps_an_image_without_valid_pixels_and_a_crop_through_the_boxes(ops, maps, boxes, crop):
    """A NaN and a +inf tap in pred, a NaN in the mirror; image 1 has no valid ground truth (all its rows zero, both regions zero); a
    Garg-style crop (rows 15 .. 35, columns 1 .. 50 of 37 x 53) cuts through the boxes of every set."""
    pred, mirror, gt = maps["special"]
    xywh6, counts = _view6(boxes)
    box = ref.GARG_STYLE(odr.CASE_H, odr.CASE_W) if crop else None
    assert box is None or box == (15, 36, 1, 51)
    for shrink in (1.0, 0.3):
        got, regions = _run(ops, pred, mirror, gt, xywh6, counts, shrink, crop=box, what=("special", boxes, crop, shrink))
        assert not got[1].any() and not regions[1].any()


def test_nyu_eigen_crop_cuts_through_boxes(ops):
    """B = 1, gt 480 x 640 (the size the NYU Eigen crop 45 .. 471 x 41 .. 601 is stated for; 75 tiles), pred 240 x 320 with mirror: boxes
    across each edge of the crop, one inside, one outside it (zero), the whole frame."""
    pred, mirror, gt = ref.case_maps(B=1, H=480, W=640, h=240, w=320, seed=4)
    rows = [(320.0, 240.0, 640.0, 480.0), (41.0, 200.0, 60.0, 80.0), (601.0, 100.0, 50.0, 120.0), (300.0, 45.0, 200.0, 40.0),
            (300.0, 471.0, 280.0, 30.0), (300.0, 250.0, 33.0, 21.0), (20.0, 20.0, 30.0, 30.0)]
    xywh, counts = torch.tensor(rows).view(1, len(rows), 4), torch.tensor([len(rows)], dtype=torch.int32)
    got, regions = _run(ops, pred, mirror, gt, xywh, counts, crop=ref.NYU_EIGEN, what="eigen")
    assert not got[0, 6].any() and got[0, 5, 8] > 0 and not regions[0, 1].any()             # the whole frame leaves no background
    assert torch.equal(got[0, 0].view(torch.int32), regions[0, 0].view(torch.int32)) or rel_dev(got[0, 0], regions[0, 0]) < 1e-6


def test_more_boxes_than_a_wave_over_several_tiles_and_an_image_without_boxes(ops):
    """B = 2, gt 96 x 131 (four tiles per image, their seams inside rows), pred 48 x 66 with mirror, cap = 70 seeded boxes over and
    beyond the map (more than one wave of the list build, boxes across tile seams); counts (70, 0): image 1 is all background."""
    pred, mirror, gt = ref.case_maps(B=2, H=96, W=131, h=48, w=66, seed=5)
    xywh, counts = ref.random_boxes(2, 70, (70, 0), 96, 131)
    got, regions = _run(ops, pred, mirror, gt, xywh, counts, what="tiles")
    assert not got[1].any() and not regions[1, 0].any() and regions[1, 1, 8] > 0 and (got[0, :, 8] > 0).sum() > 40
    got, regions = _run(ops, pred, mirror, gt, xywh, counts, shrink=0.6, what="tiles, shrink 0.6")


def test_boxes_wider_than_the_workgroup(ops):
    """B = 2, gt 31 x 300, pred 30 x 40 without mirror: the whole map (300 wide) and a 280-wide box take the column loop beyond 256
    threads; a 256- and a 257-wide box sit on and above its first step."""
    pred, mirror, gt = ref.case_maps(B=2, H=31, W=300, h=30, w=40, mirror=False, seed=6)
    rows = [(150.0, 15.5, 300.0, 31.0), (150.0, 15.0, 280.0, 9.0), (150.0, 10.0, 256.0, 5.0), (150.5, 20.0, 257.0, 3.0)]
    xywh = torch.tensor([rows, rows[::-1]])
    counts = torch.tensor([4, 2], dtype=torch.int32)
    got, regions = _run(ops, pred, mirror, gt, xywh, counts, what="wide")
    assert torch.equal(got[0, 0].view(torch.int32), regions[0, 0].view(torch.int32)) or rel_dev(got[0, 0], regions[0, 0]) < 1e-6
    assert not regions[0, 1].any() and regions[1, 1, 8] > 0 and not got[1, 2:].any()


def test_one_pixel_maps(ops):
    pred, gt = torch.tensor([[[[2.0]]]]), torch.tensor([[[[3.0]]]])                  # ratio 1.5: above 1.25, below 1.25^2
    xywh, counts = torch.tensor([[[0.5, 0.5, 1.0, 1.0]]]), torch.tensor([1], dtype=torch.int32)
    got, regions = _run(ops, pred, None, gt, xywh, counts, what="1 x 1")
    assert got[0, 0, 8] == 1 and got[0, 0, 9] == 3.0 and got[0, 0, 5] == 0 and got[0, 0, 6] == 1 and not regions[0, 1].any()
    got, regions = _run(ops, pred, None, gt, torch.tensor([[[5.0, 5.0, 1.0, 1.0]]]), counts, what="1 x 1, box outside")
    assert not got.any() and not regions[0, 0].any() and regions[0, 1, 8] == 1


def test_wrapper_refuses_what_the_region_pass_cannot_take(ops):
    pred, mirror, gt = ref.case_maps(B=1, seed=7)
    xywh = torch.zeros(1, ops.OBJECT_METRICS_MAX_BOXES + 1, 4).cuda()
    one = torch.tensor([1], dtype=torch.int32).cuda()
    with pytest.raises(ValueError):
        ops.object_metrics(dev(pred), dev(gt), xywh, one, DMIN, DMAX)
    boxes, none = ops.object_metrics(dev(pred), dev(gt), xywh, one, DMIN, DMAX, regions=False)       # the box pass has no such bound
    assert none is None and not boxes.any()
    with pytest.raises(ValueError):
        ops.object_metrics(dev(pred), dev(gt), xywh[:, :4], one, DMIN, DMAX, shrink=0.0)
    with pytest.raises(ValueError):
        ops.object_metrics(dev(pred), dev(gt), xywh[:, :4, :3], one, DMIN, DMAX)


def test_captured_graph_replays_with_new_boxes_counts_and_maps():
    """In a fresh child process (tests/object_metrics_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "object_metrics_graph_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


# ---------------------------------------------------------------------------
# the predict path (model, frames and boxes of tests/test_hip_object_depth.py)
# ---------------------------------------------------------------------------
H, W = 352, 384


def _frames(seed, B):
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _boxes(seed, B, cap):
    """Per image 1 .. cap boxes over (and a little beyond) the window, as the reference's list of [N_i, 4] tensors."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        n = int(torch.randint(1, cap + 1, (1,), generator=g))
        c = torch.rand(n, 2, generator=g) * torch.tensor([W + 20.0, H + 20.0]) - 10.0
        s = torch.rand(n, 2, generator=g) * torch.tensor([W / 2.0, H / 2.0]) + 1.0
        out.append(torch.cat([c, s], 1))
    return out


def _gt(seed, B):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, 1, H, W, generator=g) * 10.5 + 0.5
    gt[torch.rand(B, 1, H, W, generator=g) < 0.05] = 0.0
    return gt


@pytest.fixture(scope="module")
def model():
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    args = make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    m = GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5)).eval()
    gen.load_into(m, 29, gen.PEAKY)
    return m.cuda(), args


def test_predictor_tables_equal_the_reference_on_the_steps_own_prediction(ops, model):
    from objcavit_amd.object_metrics import OBJECT_METRIC_FIELDS, ObjectMetrics
    from objcavit_amd.predict import Predictor, PredictResult
    from objcavit_amd.validation import _depth_range, crop_box
    m, args = model
    B = 2
    dmin, dmax = _depth_range(args)
    crop = crop_box(args, H, W)
    frames = _frames(161, B).cuda()
    boxes = _boxes(162, B, 5)
    boxes[1] = None                                                             # an image without detections: the <UNK> row, all zero
    on = Predictor(m, args, object_metrics=dict(shrink=0.8))
    out, mirror = on._forward([frames], B)                                      # the forward the step below repeats
    pred, pmirror = out.depth_pred.cpu(), mirror.depth_pred.cpu()
    gt = ref.guard(pred, _gt(163, B), dmin, dmax, pmirror)
    res = on(frames, gt.cuda(), boxes=[None if b is None else b.cuda() for b in boxes])
    assert isinstance(res, PredictResult) and isinstance(res.object_metrics, ObjectMetrics) and res.objects is None and res.points is None
    om = res.object_metrics
    assert om.fields == OBJECT_METRIC_FIELDS and om.counts.tolist() == [boxes[0].shape[0], 1]
    cap = boxes[0].shape[0]
    xywh = torch.zeros(B, cap, 4)
    xywh[0], xywh[1, 0] = boxes[0], -1.0
    assert ref.band_size(pred, gt, dmin, dmax, pmirror) == 0
    want_b, want_r = ref.object_metrics(pred, gt, xywh, om.counts.cpu(), dmin, dmax, crop=crop, pred_mirror=pmirror, shrink=0.8)
    _check(om.table, want_b, "predict boxes")
    _check(om.regions, want_r, "predict regions")
    assert om.table[0, :, 8].sum() > 0 and not om.table[1].any() and not om.regions[1, 0].any()
    assert torch.equal(om.regions[:, 0, 8] + om.regions[:, 1, 8], res.records[:, 8])
    # records and every field are what they are without the keyword; without ground truth or without boxes there is no table
    base = Predictor(m, args)(frames, gt.cuda(), boxes=[None if b is None else b.cuda() for b in boxes])
    assert type(base) is PredictResult and base.object_metrics is None
    for k in PredictResult._fields:
        a, b = getattr(res, k), getattr(base, k)
        assert (a is None and b is None) or torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
    assert on(frames, boxes=(xywh.cuda(), om.counts)).object_metrics is None
    assert on(frames, gt.cuda()).object_metrics is None
    # regions=False; both keywords together give both attributes, each what it is alone
    both = Predictor(m, args, object_metrics=dict(shrink=0.8, regions=False), object_depth={})(frames, gt.cuda(), boxes=(xywh.cuda(), om.counts))
    assert both.object_metrics.regions is None and torch.equal(both.object_metrics.table.view(torch.int32), om.table.view(torch.int32))
    alone = Predictor(m, args, object_depth={})(frames, gt.cuda(), boxes=(xywh.cuda(), om.counts))
    assert alone.object_metrics is None and torch.equal(both.objects.table.view(torch.int32), alone.objects.table.view(torch.int32))
    assert torch.equal(both.records.view(torch.int32), res.records.view(torch.int32))


def test_pipelined_predictor_tables_equal_the_sequential_predictors(ops, model):
    """Six bs-1 steps with different boxes and ground truth over four slots: every step's tables are bit-equal to the sequential
    ``Predictor``'s (both sides replay a captured graph of the same shape), in submission order."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args = model
    N = 6
    frames = [_frames(170 + i, 1).cuda() for i in range(N)]
    gts = [_gt(190 + i, 1).cuda() for i in range(N)]
    boxes = [[b.cuda() for b in _boxes(180 + i, 1, 7)] for i in range(N)]
    boxes[2] = [None]
    opts = dict(shrink=0.9)
    pp = PipelinedPredictor(m, args, frames[0], want=("depth",), object_metrics=opts)
    example = predict_ref.frames_to_input(frames[0].cpu(), args, 0, 0, H, W)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_group=1, in_flight=4)
    seq = Predictor(g, args, object_metrics=opts)
    refs = []
    for i in range(N):
        r = seq(frames[i], gts[i], first_image_id=i, boxes=boxes[i])
        refs.append((r.records.clone(), r.object_metrics.table.clone(), r.object_metrics.regions.clone(), r.object_metrics.counts.clone()))
    for i in range(N):
        pp.submit(frames[i], gts[i], first_image_id=i, boxes=boxes[i])
    pp.submit(frames[0], gts[0])                                                # steps without boxes / without ground truth
    pp.submit(frames[0], boxes=boxes[0])
    got = pp.collect()
    assert len(got) == N + 2 and pp.rerun_steps == 0 and got[N].object_metrics is None and got[N + 1].object_metrics is None
    for i in range(N):
        om = got[i].object_metrics
        assert torch.equal(got[i].records.view(torch.int32), refs[i][0].view(torch.int32)), i
        assert om.table.shape == refs[i][1].shape and torch.equal(om.counts, refs[i][3])
        assert torch.equal(om.table.view(torch.int32), refs[i][1].view(torch.int32)), i
        assert torch.equal(om.regions.view(torch.int32), refs[i][2].view(torch.int32)), i
        assert got[i].bin_edges is None and got[i].objects is None              # _finish's _replace kept the table
    assert not got[2].object_metrics.table.any() and got[0].object_metrics.table[0, :, 8].sum() > 0
