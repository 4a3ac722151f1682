"""-m "not gpu": what the finishing half of a predict step ASKS of ``hip_ops`` -- which wrappers, in which order, with which slice of
the batch, which intrinsics and which of the uncertainty maps -- pinned with recorders in the wrappers' place, on CPU tensors; and the
argument rules the four ingest wrappers share, on CPU tensors as well.  The first test was written against the predict path before its
readouts became a table and passes unchanged on both; only ``_drive`` below, the one place that constructs ``_Ends`` and calls
``finish``, follows the call form.

The frames are a list of two single KITTI-sized frames under the dataset's benchmark crop: that rule (not ``crop=``, which fixes one
origin for every frame) gives one window size with an origin per frame, so every per-frame call must shift K by its own frame's."""
from types import SimpleNamespace

import pytest
import torch

from objcavit_amd import hip_ops, predict
from objcavit_amd.config import make_args
from objcavit_amd.predict import KB_CROP, PredictResult, kb_crop_origin

H, W = KB_CROP
SIZES = ((370, 1224), (376, 1242))                       # two frames, two origins: (18, 4) and (24, 13)
ORIGINS = tuple(kb_crop_origin(*s) for s in SIZES)
K_SRC = torch.tensor([[700.0, 710.0, 600.0, 180.0], [720.0, 730.0, 610.0, 170.0]])
INF = float("inf")


def _drive(args, keywords: dict, out, mirror, frames, want, depth_gt=None, boxes=None, intrinsics=None, camera_pose=None):
    """The adapter: (``_Ends`` of the predictors' keywords, the result of the finishing half of one step on the step's inputs)."""
    ends = predict._Ends(args, flip_tta=mirror is not None, **keywords)
    step = ends.step(ends.frames_of(frames, "frames_u8"), depth_gt=depth_gt, boxes=boxes, intrinsics=intrinsics, camera_pose=camera_pose)
    return ends, ends.finish(out, mirror, step, 0, want)


class _Recorder:
    """Stand-ins for the wrappers behind the final map: each logs (name, the arguments that matter) and returns CPU tensors of the
    documented shapes."""

    def __init__(self, monkeypatch):
        self.calls = []
        self.maps = {}
        for name in ("depth_finalize", "object_depth", "object_metrics", "depth_unproject", "frames_to_rgb24", "depth_normals",
                     "normals_gather", "ground_grid"):
            monkeypatch.setattr(hip_ops, name, getattr(self, name))
        monkeypatch.setattr(predict, "_records", self.records)            # the metric launch of a step with ground truth

    def names(self):
        return [c[0] for c in self.calls]

    def of(self, name):
        return [c[1] for c in self.calls if c[0] == name]

    def _slice(self, t, of):
        """None, or (first image, images) of a batch slice of the map ``of`` -- by its storage, not by its values."""
        if t is None:
            return None
        whole = self.maps[of]
        assert t.untyped_storage().data_ptr() == whole.untyped_storage().data_ptr(), f"not a slice of the '{of}' map"
        per = whole[0].numel()
        assert t.storage_offset() % per == 0 and tuple(t.shape[1:]) == tuple(whole.shape[1:])
        return t.storage_offset() // per, int(t.shape[0])

    def depth_finalize(self, pred, min_depth, max_depth, size, pred_mirror=None, want=("depth",), var=None, pmax=None, var_mirror=None,
                       pmax_mirror=None, **kw):
        self.calls.append(("depth_finalize", dict(want=tuple(want), size=tuple(size), mirror=pred_mirror is not None,
                                                  stats=tuple(t is not None for t in (var, pmax, var_mirror, pmax_mirror)))))
        B = int(pred.shape[0])
        shapes = {"depth": ((B, 1) + tuple(size), torch.float32), "depth_u16": ((B,) + tuple(size), torch.uint16),
                  "depth_std": ((B, 1) + tuple(size), torch.float32), "confidence": ((B, 1) + tuple(size), torch.float32)}
        self.maps = {n: torch.zeros(shapes[n][0], dtype=shapes[n][1]) for n in want}
        return dict(self.maps)

    def records(self, pred, mirror, edges, depth_gt, *rest):
        self.calls.append(("records", dict(gt=tuple(depth_gt.shape))))
        return torch.zeros(int(pred.shape[0]), 10)

    def object_metrics(self, pred, gt, xywh, counts, min_depth, max_depth, crop=None, pred_mirror=None, shrink=1.0, regions=True, out=None):
        self.calls.append(("object_metrics", dict(shrink=shrink, regions=regions, mirror=pred_mirror is not None)))
        B, cap = int(xywh.shape[0]), int(xywh.shape[1])
        return torch.zeros(B, cap, 10), (torch.zeros(B, 2, 10) if regions else None)

    def object_depth(self, depth, xywh, counts, depth_std=None, quantiles=(0.1, 0.5, 0.9), shrink=1.0, out=None):
        self.calls.append(("object_depth", dict(depth=self._slice(depth, "depth"), std=self._slice(depth_std, "depth_std"),
                                                quantiles=tuple(quantiles), shrink=shrink)))
        return torch.zeros(int(xywh.shape[0]), int(xywh.shape[1]), 5 + len(quantiles))

    def frames_to_rgb24(self, frames, pixel_format, top=0, left=0, size=None, **kw):
        self.calls.append(("frames_to_rgb24", dict(frame=tuple(frames.shape[1:3]), origin=(top, left), size=tuple(size))))
        self.rgb = torch.zeros((int(frames.shape[0]),) + tuple(size) + (3,), dtype=torch.uint8)
        return self.rgb

    def _per_frame(self, depth, K, confidence, depth_std, image_index):
        return dict(image_index=image_index, depth=self._slice(depth, "depth"), K=K.tolist(),
                    confidence=self._slice(confidence, "confidence"), depth_std=self._slice(depth_std, "depth_std"))

    def depth_unproject(self, depth, K, capacity, stride=(1, 1), near=0.0, far=INF, confidence=None, min_confidence=0.0,
                        depth_std=None, max_std=INF, frames=None, top=0, left=0, want_pixel=False, out=None, image_index=0, **kw):
        self.calls.append(("depth_unproject", dict(self._per_frame(depth, K, confidence, depth_std, image_index), capacity=capacity,
                                                   want_pixel=want_pixel, names=tuple(sorted(out)), origin=(top, left),
                                                   colour=None if frames is None else "copy" if frames is getattr(self, "rgb", None)
                                                   else tuple(frames.shape[1:3]))))
        self.cloud = out
        return out

    def depth_normals(self, depth, K, radius=2, near=0.0, far=INF, edge_ratio=0.05, want=("normals",), out=None, image_index=0):
        self.calls.append(("depth_normals", dict(self._per_frame(depth, K, None, None, image_index), want=tuple(want),
                                                 names=tuple(sorted(out)), radius=radius)))
        self.normal_bufs = out
        return out

    def normals_gather(self, normals, pixel, counts, out=None):
        self.calls.append(("normals_gather", dict(normals=normals is self.normal_bufs["normals"], pixel=pixel is self.cloud["pixel"],
                                                  counts=counts is self.cloud["counts"])))
        self.gathered = torch.zeros(tuple(pixel.shape) + (4,))
        return self.gathered

    def ground_grid(self, depth, K, pose, grid, confidence=None, depth_std=None, want=(), out=None, image_index=0, **kw):
        self.calls.append(("ground_grid", dict(self._per_frame(depth, K, confidence, depth_std, image_index), pose=pose.tolist(),
                                               want=tuple(want), names=tuple(sorted(out)), min_confidence=kw["min_confidence"],
                                               max_std=kw["max_std"])))
        return out


def _step_inputs(stats: bool):
    frames = [torch.zeros(Hs, Ws, 3, dtype=torch.uint8) for Hs, Ws in SIZES]
    half = lambda: SimpleNamespace(depth_pred=torch.ones(2, 1, 4, 6), bin_edges=torch.zeros(2, 9),             # noqa: E731
                                   **(dict(depth_var=torch.ones(2, 1, 4, 6), confidence=torch.ones(2, 1, 4, 6)) if stats else {}))
    return frames, half(), half()


def _shifted(i):
    top, left = ORIGINS[i]
    return [(K_SRC[i] - torch.tensor([0.0, 0.0, float(left), float(top)])).tolist()]


@pytest.fixture(scope="module")
def args():
    return make_args(dataset="kitti")


def test_every_keyword_on_asks_for_the_launches_in_order_with_each_frames_own_slice_and_origin(args, monkeypatch):
    rec = _Recorder(monkeypatch)
    frames, out, mirror = _step_inputs(stats=True)
    boxes = [torch.tensor([[50.0, 60.0, 20.0, 10.0], [300.0, 100.0, 40.0, 40.0]]), None]
    pose = torch.arange(24, dtype=torch.float32).reshape(2, 12)
    kw = dict(object_depth={"shrink": 0.5}, object_metrics={"regions": False}, surface_normals={"picture": True},
              point_cloud={"min_confidence": 0.5, "max_std": 2.0, "normals": True, "stride": 2},
              ground_grid={"min_confidence": 0.25, "want": ("state", "count")}, pixel_format="bgr24")
    ends, res = _drive(args, kw, out, mirror, frames, ("depth_u16",), depth_gt=torch.ones(2, 1, H, W), boxes=boxes,
                       intrinsics=K_SRC, camera_pose=pose)
    # the order: finalize, metric records, per-object error, object readout, the cloud frame by frame behind its RGB24 copy, the dense
    # normals frame by frame, the gather, the grid frame by frame
    assert rec.names() == ["depth_finalize", "records", "object_metrics", "object_depth", "frames_to_rgb24", "depth_unproject",
                           "frames_to_rgb24", "depth_unproject", "depth_normals", "depth_normals", "normals_gather", "ground_grid",
                           "ground_grid"]
    # want: "depth" forced by the readouts, "confidence" / "depth_std" by the cloud's thresholds (the grid's min_confidence adds nothing new)
    fin, = rec.of("depth_finalize")
    assert fin == dict(want=("depth_u16", "depth", "confidence", "depth_std"), size=(H, W), mirror=True, stats=(True,) * 4)
    assert rec.of("object_metrics") == [dict(shrink=1.0, regions=False, mirror=True)]
    # the object readout gets the whole map, and depth_std only when the CALLER's want names it
    assert rec.of("object_depth") == [dict(depth=(0, 2), std=None, quantiles=(0.1, 0.5, 0.9), shrink=0.5)]
    gh, gw = -(-H // 2), -(-W // 2)
    for i in range(2):
        assert rec.of("frames_to_rgb24")[i] == dict(frame=SIZES[i], origin=ORIGINS[i], size=(H, W))
        assert rec.of("depth_unproject")[i] == dict(image_index=i, depth=(i, 1), K=_shifted(i), confidence=(i, 1), depth_std=(i, 1),
                                                    capacity=gh * gw, want_pixel=True, names=("counts", "pixel", "points", "total"),
                                                    origin=(0, 0), colour="copy")
        assert rec.of("depth_normals")[i] == dict(image_index=i, depth=(i, 1), K=_shifted(i), confidence=None, depth_std=None,
                                                  want=("normals", "rgb8"), names=("normals", "rgb8"), radius=2)
        assert rec.of("ground_grid")[i] == dict(image_index=i, depth=(i, 1), K=_shifted(i), confidence=(i, 1), depth_std=None,
                                                pose=pose[i:i + 1].tolist(), want=("count", "state"), names=("count", "state"),
                                                min_confidence=0.25, max_std=INF)
    assert rec.of("normals_gather") == [dict(normals=True, pixel=True, counts=True)]
    # the result: the maps made for the readouts alone are not handed out; the pixel index made for the gather alone is not either
    assert isinstance(res, PredictResult) and res.depth is None and res.depth_std is None and res.confidence is None
    assert res.depth_u16 is rec.maps["depth_u16"] and tuple(res.records.shape) == (2, 10) and res.bin_edges is out.bin_edges
    assert tuple(res.objects.table.shape) == (2, 2, 8) and res.objects.counts.tolist() == [2, 1]
    assert tuple(res.object_metrics.table.shape) == (2, 2, 10) and res.object_metrics.regions is None
    assert res.points.points is rec.cloud["points"] and tuple(res.points.points.shape) == (2, gh * gw, 4)
    assert res.points.counts is rec.cloud["counts"] and res.points.total is rec.cloud["total"] and res.points.pixel is None
    assert res.normals.normals is rec.normal_bufs["normals"] and tuple(res.normals.normals.shape) == (2, 3, H, W)
    assert tuple(res.normals.rgb8.shape) == (2, H, W, 3) and res.normals.valid is None and res.normals.points is rec.gathered
    GX, GY = ends.ground["grid"][3:]
    assert tuple(res.ground.count.shape) == (2, GY, GX) and res.ground.state.dtype == torch.uint8 and res.ground.h_min is None
    assert res.ground.first_occupied is None and res.ground.cell == ends.ground["grid"][2]
    assert res._replace(bin_edges=None).ground is res.ground and res._replace(bin_edges=None).bin_edges is None


def test_each_readout_gets_the_maps_its_own_thresholds_ask_for(args, monkeypatch):
    rec = _Recorder(monkeypatch)
    frames, out, mirror = _step_inputs(stats=True)
    kw = dict(point_cloud={"pixel": True, "colour": False, "capacity": 100}, ground_grid={"max_std": 3.0}, object_depth={})
    boxes = [torch.tensor([[50.0, 60.0, 20.0, 10.0]])] * 2
    ends, res = _drive(args, kw, out, None, frames, ("depth", "confidence"), boxes=boxes, intrinsics=[k for k in K_SRC])
    assert rec.names() == ["depth_finalize", "object_depth", "depth_unproject", "depth_unproject", "ground_grid", "ground_grid"]
    # "depth_std" is forced by the grid's finite max_std alone; without TTA the mirrored statistics are not read
    assert rec.of("depth_finalize") == [dict(want=("depth", "confidence", "depth_std"), size=(H, W), mirror=False,
                                             stats=(True, True, False, False))]
    assert rec.of("object_depth")[0]["std"] is None                       # made, but not asked for by the caller
    keyword_pose = ends.ground["pose"].reshape(1, 12).tolist()
    for i in range(2):
        # the cloud carries the confidence whenever that map is made (byte 15 of a record) and depth_std only under a finite max_std;
        # the grid reads each only under its own threshold
        assert rec.of("depth_unproject")[i] == dict(image_index=i, depth=(i, 1), K=_shifted(i), confidence=(i, 1), depth_std=None,
                                                    capacity=100, want_pixel=True, names=("counts", "pixel", "points", "total"),
                                                    origin=ORIGINS[i], colour=None)
        g = rec.of("ground_grid")[i]
        assert (g["image_index"], g["K"], g["confidence"], g["depth_std"]) == (i, _shifted(i), None, (i, 1))
        assert g["pose"] == keyword_pose and g["want"] == hip_ops.GROUND_GRID_WANT and g["max_std"] == 3.0
    assert res.depth is rec.maps["depth"] and res.confidence is rec.maps["confidence"] and res.depth_std is None
    assert res.points.pixel is rec.cloud["pixel"] and res.normals is None and res.object_metrics is None and res.records is None
    assert tuple(res.points.points.shape) == (2, 100, 4) and tuple(res.ground.first_occupied.shape) == (2, ends.ground["grid"][3])
    # the cloud's frame colour: the frame itself, at its own origin, when the format is the packed RGB of old
    rec.calls.clear()
    _drive(args, dict(point_cloud={}), out, None, frames, (), intrinsics=K_SRC)
    assert rec.of("depth_finalize")[0]["want"] == ("depth",) and rec.names()[1:] == ["depth_unproject"] * 2
    assert [(c["colour"], c["origin"], c["confidence"], c["want_pixel"]) for c in rec.of("depth_unproject")] == \
        [(SIZES[i], ORIGINS[i], None, False) for i in range(2)]


def test_without_intrinsics_or_boxes_nothing_runs_behind_the_final_map(args, monkeypatch):
    rec = _Recorder(monkeypatch)
    frames, out, mirror = _step_inputs(stats=False)
    kw = dict(object_depth={}, object_metrics={}, point_cloud={"min_confidence": 0.5, "normals": True}, surface_normals={},
              ground_grid={"max_std": 1.0})
    boxes = [torch.tensor([[50.0, 60.0, 20.0, 10.0]])] * 2
    ends, res = _drive(args, kw, out, mirror, frames, ("depth_u16",))
    assert rec.names() == ["depth_finalize"] and rec.of("depth_finalize")[0]["want"] == ("depth_u16",)
    assert (res.objects, res.points, res.object_metrics, res.normals, res.ground, res.records, res.depth) == (None,) * 7
    rec.calls.clear()
    ends, res = _drive(args, kw, out, mirror, frames, ("depth_u16",), boxes=boxes)             # boxes alone: the readout alone
    assert rec.names() == ["depth_finalize", "object_depth"] and rec.of("depth_finalize")[0]["want"] == ("depth_u16", "depth")
    assert res.objects is not None and (res.points, res.object_metrics, res.normals, res.ground, res.depth) == (None,) * 5
    rec.calls.clear()
    ends, res = _drive(args, kw, out, mirror, frames, (), boxes=boxes, depth_gt=torch.ones(2, 1, H, W))
    assert rec.names() == ["depth_finalize", "records", "object_metrics", "object_depth"]
    rec.calls.clear()
    ends, res = _drive(args, dict(kw, object_depth=None), out, mirror, frames, (), depth_gt=torch.ones(2, 1, H, W))
    assert rec.names() == ["records"] and res.records is not None and res.object_metrics is None       # nothing wanted, nothing made


# ---------------------------------------------------------------------------
# the ingest fronts: one set of argument rules, each wrapper's own name in the text
# ---------------------------------------------------------------------------
def _ingest_fronts():
    """name -> call(frames, table, **kw): the four public ingest wrappers over packed frames, H x W = 8 x 12 out of a 16 x 24 window."""
    return {"frame_ingest": lambda f, t, **kw: hip_ops.frame_ingest(f, t, 0, 0, (8, 12), **kw),
            "frame_ingest_format": lambda f, t, **kw: hip_ops.frame_ingest_format(f, t, "rgb24", 0, 0, (8, 12), **kw),
            "frame_resize_ingest": lambda f, t, **kw: hip_ops.frame_resize_ingest(f, t, (8, 12), **kw),
            "frame_resize_ingest_format": lambda f, t, **kw: hip_ops.frame_resize_ingest_format(f, t, (8, 12), "rgb24", **kw)}


@pytest.mark.parametrize("name", sorted(_ingest_fronts()))
def test_ingest_fronts_refuse_the_same_arguments_with_the_same_words(name, monkeypatch):
    """The rules are host arithmetic on shapes; the device check in front of them is taken out so that CPU tensors reach them, and every
    case raises before a launch."""
    import re
    from objcavit_amd.hip_ops import frames as frames_mod
    monkeypatch.setattr(frames_mod, "_req", lambda t, *a, **kw: t)
    call = _ingest_fronts()[name]
    resize = "resize" in name
    frames, table = torch.zeros(2, 16 if resize else 8, 24 if resize else 12, 3, dtype=torch.uint8), torch.zeros(3, 256)
    taps = (torch.zeros(8, dtype=torch.int32), torch.zeros(8, 3), torch.zeros(12, dtype=torch.int32), torch.zeros(12, 3))
    kw = dict(taps=taps) if resize else {}
    odd = torch.zeros(5, 3, 8, 12)
    with pytest.raises(ValueError, match=re.escape(f"{name}: 2 image(s) at index 0 do not fit out (5, 3, 8, 12) (first half: the second "
                                                   "takes the mirrors)")):
        call(frames, table, mirror_too=True, out=odd, **kw)
    with pytest.raises(ValueError, match=re.escape(f"{name}: 2 image(s) at index 2 do not fit out (6, 3, 8, 12) (first half: the second "
                                                   "takes the mirrors)")):
        call(frames, table, mirror_too=True, out=torch.zeros(6, 3, 8, 12), out_index=2, **kw)
    with pytest.raises(ValueError, match=re.escape(f"{name}: 2 image(s) at index 3 do not fit out (4, 3, 8, 12)") + "$"):
        call(frames, table, out=torch.zeros(4, 3, 8, 12), out_index=3, **kw)
    with pytest.raises(ValueError, match=re.escape(f"{name}: table must be [3, 256], got (3, 255)")):
        call(frames, torch.zeros(3, 255), **kw)
    if resize:
        with pytest.raises(ValueError, match=re.escape(f"{name}: taps = (ystart, yweight, xstart, xweight)")):
            call(frames, table, taps=taps + taps[:1])
        big = torch.zeros(1, 8 * hip_ops.FRAME_RESIZE_MAX_RATIO + 1, 24, 3, dtype=torch.uint8)
        with pytest.raises(ValueError, match=re.escape(f"{name}: a {big.shape[1]} x 24 window to 8 x 12 shrinks by more than "
                                                       f"{hip_ops.FRAME_RESIZE_MAX_RATIO} along an axis, the most one launch takes")):
            call(big, table, taps=taps)
