"""-m "not gpu": the per-object / per-region depth error's host side -- the CPU statement of tests/object_metrics_ref.py against a
brute-force pixel loop and against its own invariants, the new symbols and every argument refusal of the entry point (no launch
happens), the wrapper, the predict interface's pins and ``totals`` on a hand-made table."""
import inspect
import math
import os
import re

import pytest
import torch

import object_depth_ref as odr
import object_metrics_ref as ref
from oracle import validation_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = odr.CASE_H, odr.CASE_W


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def maps():
    """pred 19 x 27 with mirror, a NaN and a +inf tap; gt 37 x 53 -- made once, read by every test."""
    return ref.case_maps(special=True)


# ---------------------------------------------------------------------------
# the CPU statement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(odr.BOX_SETS))
@pytest.mark.parametrize("shrink,crop", [(1.0, None), (0.3, None), (1.0, ref.GARG_STYLE(H, W))])
def test_reference_agrees_with_a_brute_force_pixel_loop(maps, name, shrink, crop):
    pred, mirror, gt = maps
    xywh, counts = odr.case_boxes(name)
    boxes, regions = ref.object_metrics(pred, gt, xywh, counts, crop=crop, pred_mirror=mirror, shrink=shrink)
    assert tuple(boxes.shape) == (3, 6, 10) and tuple(regions.shape) == (3, 2, 10)
    p, valid = ref.pixel_value(pred, gt, ref.MIN_DEPTH, ref.MAX_DEPTH, mirror, crop)
    close = lambda a, e: a == e or abs(a - e) <= 1e-12 * abs(e)             # noqa: E731  (float64 sums in another order)
    for b in range(3):
        union = torch.zeros(H, W, dtype=torch.bool)
        for r in range(6):
            want, inside = ref.brute_force(p[b, 0], gt[b, 0], valid[b, 0], xywh[b, r].tolist() if r < int(counts[b]) else None, shrink)
            union |= inside
            assert all(close(a, e) for a, e in zip(boxes[b, r].tolist(), want)), (name, b, r, boxes[b, r].tolist(), want)
            assert boxes[b, r, 8] == want[8]
        for row, m in ((0, union), (1, ~union)):
            want = ref.brute_record(p[b, 0], gt[b, 0], valid[b, 0] & m)
            assert all(close(a, e) for a, e in zip(regions[b, row].tolist(), want)), (name, b, row)
            assert regions[b, row, 8] == want[8]


@pytest.mark.parametrize("name", sorted(odr.BOX_SETS))
@pytest.mark.parametrize("shrink", [1.0, 0.3])
def test_regions_partition_the_image_record(maps, name, shrink):
    pred, mirror, gt = maps
    xywh, counts = odr.case_boxes(name)
    assert ref.band_size(pred, gt, pred_mirror=mirror) == 0
    _, regions = ref.object_metrics(pred, gt, xywh, counts, pred_mirror=mirror, shrink=shrink)
    image = vr.per_image_records(pred, gt, ref.MIN_DEPTH, ref.MAX_DEPTH, depth_pred_mirror=mirror).double()
    assert torch.equal(regions[:, 0, 8] + regions[:, 1, 8], image[:, 8])
    whole = ref.recombine(regions)
    assert ((whole[:, :8] - image[:, :8]).abs() <= 2e-7 * image[:, :8].abs()).all(), (whole, image)      # image is rounded to fp32


def test_whole_map_box_is_the_objects_region_and_duplicates_count_once(maps):
    pred, mirror, gt = maps
    big, spare = (26.5, 18.5, 53.0, 37.0), (10.3, 7.7, 4.6, 3.2)
    xywh = torch.tensor([[big, spare], [spare, spare], [big, big]])
    counts = torch.tensor([1, 2, 2], dtype=torch.int32)
    boxes, regions = ref.object_metrics(pred, gt, xywh, counts, pred_mirror=mirror)
    image = vr.per_image_records(pred, gt, ref.MIN_DEPTH, ref.MAX_DEPTH, depth_pred_mirror=mirror).double()
    # one whole-map box: its row is the objects row, the background is empty, and both are the image's record
    assert torch.equal(boxes[0, 0], regions[0, 0]) and not regions[0, 1].any() and not boxes[0, 1].any()
    assert regions[0, 0, 8] == image[0, 8] and ((regions[0, 0, :8] - image[0, :8]).abs() <= 2e-7 * image[0, :8].abs()).all()
    # a duplicated box: identical rows, counted once in the union
    assert torch.equal(boxes[1, 0], boxes[1, 1]) and boxes[1, 0, 8] > 0 and torch.equal(regions[1, 0], boxes[1, 0])
    assert torch.equal(boxes[2, 0], boxes[2, 1]) and torch.equal(regions[2, 0], boxes[2, 0]) and regions[2, 0, 8] == image[2, 8]


def test_input_generator_guards_the_delta_thresholds():
    """Without the guard the band is not empty on maps of this size (so the guard is doing something); with it, it is."""
    pred, mirror, gt = ref.case_maps(B=2, H=96, W=131, h=48, w=66, seed=3)
    assert ref.band_size(pred, gt, pred_mirror=mirror) == 0
    p, mask = ref.pixel_value(pred, gt, ref.MIN_DEPTH, ref.MAX_DEPTH, mirror)
    moved = gt.clone()
    y, x = (int(v) for v in (mask[0, 0] & (p[0, 0] < 7.0)).nonzero()[0])          # (1.25 p stays inside the depth range)
    moved[0, 0, y, x] = p[0, 0, y, x] * 1.25
    assert ref.band_size(pred, moved, pred_mirror=mirror) == 1
    assert ref.band_size(pred, ref.guard(pred, moved, pred_mirror=mirror), pred_mirror=mirror) == 0


# ---------------------------------------------------------------------------
# header, bindings, argument checks
# ---------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported(lib):
    from objcavit_amd import _lib, build, hip_ops
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_object_metrics_fwd\s*\(", header) and re.search(r"\bsize_t\s+ocv_object_metrics_workspace_bytes\s*\(", header)
    assert re.search(r"#define\s+OCV_ABI_VERSION\s+5\b", header)
    m = re.search(r"#define\s+OCV_OBJECT_METRICS_MAX_BOXES\s+(\d+)\b", header)
    assert m and int(m.group(1)) >= 1024 and hip_ops.OBJECT_METRICS_MAX_BOXES == int(m.group(1))
    for name in ("ocv_object_metrics_fwd", "ocv_object_metrics_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "object_metrics.hip" in build.SOURCES
    for shared in ("metric_pixel.hpp", "box_edges.hpp"):
        assert os.path.exists(os.path.join(ROOT, "objcavit_amd", "csrc", shared))
    assert lib.ocv_abi_version() == 5 and _lib.ABI_VERSION == 5
    # two sets of ten float64 sums per workgroup, the image record's tiling
    assert lib.ocv_object_metrics_workspace_bytes(16, 480, 640) == lib.ocv_depth_metrics_workspace_bytes(16, 480, 640) // 9 * 20
    assert lib.ocv_object_metrics_workspace_bytes(1, 1, 1) == 160 and lib.ocv_object_metrics_workspace_bytes(0, 4, 4) == 0


def _call(lib, pred=64, mirror=None, gt=64, xywh=64, counts=64, boxes=64, regions=64, ws=64, ws_bytes=1 << 20, B=1, cap=1, h=4, w=4, Hh=8,
          Ww=8, dmin=0.1, dmax=10.0, crop=(0, 8, 0, 8), stride=4, half=0.5):
    """The entry point with made-up (never dereferenced) device addresses: every call here must be refused before any launch."""
    return lib.ocv_object_metrics_fwd(pred, mirror, h, w, gt, Hh, Ww, dmin, dmax, crop[0], crop[1], crop[2], crop[3], xywh, stride, counts,
                                      B, cap, half, boxes, regions, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(pred=None), "null pointer"), (dict(gt=None), "null pointer"), (dict(xywh=None), "null pointer"),
    (dict(counts=None), "null pointer"), (dict(boxes=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(B=0), "bad sizes"), (dict(B=65536), "bad sizes"), (dict(cap=0), "bad sizes"), (dict(h=0), "bad sizes"), (dict(w=0), "bad sizes"),
    (dict(Hh=0, crop=(0, 0, 0, 8)), "bad sizes"), (dict(Ww=0, crop=(0, 8, 0, 0)), "bad sizes"),
    (dict(Hh=1 << 25, Ww=1, crop=(0, 1, 0, 1)), "bad sizes"), (dict(Hh=1 << 16, Ww=1 << 16, crop=(0, 1, 0, 1)), "bad sizes"),
    (dict(dmin=10.0), "min_depth"), (dict(dmin=11.0), "min_depth"), (dict(dmax=float("nan")), "min_depth"),
    (dict(crop=(0, 9, 0, 8)), "crop box"), (dict(crop=(5, 4, 0, 8)), "crop box"), (dict(crop=(0, 8, -1, 8)), "crop box"),
    (dict(crop=(0, 8, 0, 9)), "crop box"),
    (dict(half=0.0), "half"), (dict(half=0.6), "half"), (dict(half=float("nan")), "half"),
    (dict(stride=3), "xywh_row_stride"),
    (dict(cap=1025), "at most 1024"),
    (dict(pred=66), "misaligned"), (dict(mirror=65), "misaligned"), (dict(gt=62), "misaligned"), (dict(xywh=67), "misaligned"),
    (dict(counts=66), "misaligned"), (dict(boxes=65), "misaligned"), (dict(regions=66), "misaligned"),
    (dict(ws_bytes=159), "workspace too small"), (dict(ws=68), "workspace too small or misaligned"),
])
def test_bad_arguments_are_refused_with_a_message_before_any_launch(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_object_metrics_fwd:") and word in msg, msg


def test_wrapper_refuses_host_tensors_and_has_the_documented_signature():
    from objcavit_amd import hip_ops
    from objcavit_amd._lib import HipLibraryError
    p, g, x, c = torch.ones(1, 1, 4, 4), torch.ones(1, 1, 8, 8), torch.zeros(1, 2, 4), torch.ones(1, dtype=torch.int32)
    with pytest.raises(HipLibraryError):
        hip_ops.object_metrics(p, g, x, c, 0.1, 10.0)
    params = inspect.signature(hip_ops.object_metrics).parameters
    assert list(params) == ["pred", "gt", "xywh", "counts", "min_depth", "max_depth", "crop", "pred_mirror", "shrink", "regions", "out"]
    assert hip_ops.object_metrics.__defaults__ == (None, None, 1.0, True, None)
    assert hip_ops.OBJECT_METRICS_COLUMNS == 10
    from objcavit_amd.object_metrics import object_metrics
    with pytest.raises(HipLibraryError):
        object_metrics(p, g, (x, c), __import__("objcavit_amd.config", fromlist=["make_args"]).make_args())


# ---------------------------------------------------------------------------
# the predict interface and the summariser
# ---------------------------------------------------------------------------
def test_predict_keyword_is_parsed_and_the_pins_hold():
    from objcavit_amd.config import make_args
    from objcavit_amd.predict import WANT, PipelinedPredictor, Predictor, PredictResult, _Ends, _metric_options, _ObjectsResult
    assert _metric_options(None) is None and _metric_options({}) == {"shrink": 1.0, "regions": True}
    assert _metric_options({"shrink": 0.5, "regions": 0}) == {"shrink": 0.5, "regions": False}
    with pytest.raises(ValueError, match="object_metrics: unknown option"):
        _metric_options({"shrinks": 0.5})
    args = make_args()
    with pytest.raises(ValueError):
        Predictor(None, args, object_metrics={"quantiles": (0.5,)})
    with pytest.raises(ValueError):
        PipelinedPredictor(None, args, None, object_metrics={"region": True})                # refused before anything is captured
    # the fields, WANT and the older keywords are where they were; the new keyword sits in front of them and defaults to None
    assert PredictResult._fields == ("depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence")
    assert WANT == ("depth", "depth_u16", "rgb8", "depth_std", "confidence")
    for fn in (Predictor.__init__, PipelinedPredictor.__init__):
        names = list(inspect.signature(fn).parameters)
        assert names[-3:] == ["object_metrics", "point_cloud", "object_depth"]
        assert all(inspect.signature(fn).parameters[k].default is None for k in names[-3:])
    for fn in (Predictor.__call__, PipelinedPredictor.submit):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["intrinsics", "boxes"] and "object_metrics" not in params
    # the attribute rides beside objects / points and survives _replace
    r = PredictResult(1, 2, 3, 4, 5)
    assert r.object_metrics is None and len(r) == 7
    o = _ObjectsResult(*r, objects="o", points="p", object_metrics="m")
    assert o == r and (o.objects, o.points, o.object_metrics) == ("o", "p", "m")
    k = o._replace(bin_edges=None)
    assert (k.objects, k.points, k.object_metrics, k.bin_edges) == ("o", "p", "m", None)
    # the boxes are handed through with either keyword, and with neither they are not
    dev = torch.device("cpu")
    boxes = [torch.tensor([[5.0, 5.0, 2.0, 2.0]])]
    ends = lambda **kw: _Ends(args, flip_tta=True, loss=False, **kw)      # noqa: E731
    assert ends().boxes_on(boxes, dev, 1) is None and ends(object_metrics={}).boxes_on(None, dev, 1) is None
    for kw in (dict(object_metrics={}), dict(object_depth={}), dict(object_metrics={}, object_depth={})):
        xywh, counts = ends(**kw).boxes_on(boxes, dev, 1)
        assert tuple(xywh.shape) == (1, 1, 4) and counts.tolist() == [1]
    assert ends(object_metrics={}).readout is None and ends(object_depth={}).errors is None


def test_totals_on_a_hand_made_table():
    from objcavit_amd.object_metrics import OBJECT_METRIC_FIELDS, ObjectMetrics, totals
    from objcavit_amd.dp import RECORD_FIELDS
    assert OBJECT_METRIC_FIELDS == RECORD_FIELDS[:8] + ("n_valid", "gt_mean") and len(OBJECT_METRIC_FIELDS) == 10
    row = lambda v, rm, n, gm: [v, v, rm, rm, v, v, v, v, n, gm]           # noqa: E731
    zero = [0.0] * 10
    table = torch.tensor([[row(0.1, 3.0, 10.0, 2.0), row(0.3, 4.0, 30.0, 6.0), zero], [row(0.5, 1.0, 60.0, 1.0), zero, zero]])
    regions = torch.tensor([[row(0.2, 2.0, 35.0, 4.0), row(0.4, 1.0, 65.0, 8.0)], [row(0.5, 1.0, 60.0, 1.0), zero]])
    res = ObjectMetrics(table, regions, torch.tensor([2, 1], dtype=torch.int32), OBJECT_METRIC_FIELDS)
    t = totals(res)
    obj, bg = t["objects"]["pixels"], t["background"]["pixels"]
    assert obj["n_valid"] == 95 and bg["n_valid"] == 65 and "groups" not in t
    assert math.isclose(obj["abs_rel"], (0.2 * 35 + 0.5 * 60) / 95, rel_tol=1e-6) and math.isclose(bg["delta1"], 0.4, rel_tol=1e-6)
    assert math.isclose(obj["rmse"], math.sqrt((4.0 * 35 + 1.0 * 60) / 95), rel_tol=1e-6)
    assert math.isclose(obj["gt_mean"], (4.0 * 35 + 1.0 * 60) / 95, rel_tol=1e-6)
    per = t["objects"]["boxes"]
    assert per["boxes"] == 3 and math.isclose(per["abs_rel"], (0.1 + 0.3 + 0.5) / 3, rel_tol=1e-6)
    assert math.isclose(per["rmse"], (3.0 + 4.0 + 1.0) / 3, rel_tol=1e-6) and math.isclose(per["gt_mean"], 3.0, rel_tol=1e-6)
    # groups: a label per box row; rows without a valid pixel never vote; two results concatenate
    labels = torch.tensor([[7, 9, 9], [7, 7, 9]])
    g = totals([res, res], groups=[labels, labels])["groups"]
    assert sorted(g) == [7, 9] and g[7]["boxes"]["boxes"] == 4 and g[9]["boxes"]["boxes"] == 2
    assert g[7]["pixels"]["n_valid"] == 140 and math.isclose(g[7]["pixels"]["abs_rel"], (0.1 * 10 + 0.5 * 60) / 70, rel_tol=1e-6)
    assert math.isclose(g[7]["pixels"]["rmse"], math.sqrt((9.0 * 10 + 1.0 * 60) / 70), rel_tol=1e-6)
    assert math.isclose(g[9]["boxes"]["abs_rel"], 0.3, rel_tol=1e-6) and totals(res, groups=labels)["groups"][9]["pixels"]["n_valid"] == 30
    assert totals(res._replace(regions=None))["objects"]["pixels"] is None
    with pytest.raises(ValueError):
        totals(res, groups=torch.zeros(2, 2))
