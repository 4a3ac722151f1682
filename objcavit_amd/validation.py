"""The reference's validation step around the model (row N2 of SURVEY.md section 8f), on the device.

``ValidationStep(model, args)(image, depth_gt)`` does what ``GraphBinsLM.validation_step`` does between the batch and
its logged numbers (modules/GraphBinsLM.py:154-212): forward on the image and on its mirror -- here as ONE forward over the
2B images [batch | mirrored batch] (the reference forces bs 1, main.py:58, and calls the model twice, :159,173: at that size
every launch is latency, so two calls cost twice one; images are independent and the one coupling between them, the Nmax the
object rows are padded to with ``use_2_saca``, is formed per GROUP of B images on the device) --, clamp, un-flip, average,
then metrics/MetricsPreprocess.py (resize to the ground truth, nan/inf fix, validity mask, Garg / Eigen crop) and the
eight metrics -- the last three steps in ONE kernel (csrc/metrics.hip) that returns one record per image.  A
data-parallel job all-gathers the records once (objcavit_amd/dp.py); ``dp.summarise`` gives the reference's
running-average numbers, ``totals`` below its pixel-total numbers.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional, Tuple

import torch

from . import hip_ops
from .dp import LOSS_FIELDS, RECORD_FIELDS


def crop_box(args, H: int, W: int) -> Optional[Tuple[int, int, int, int]]:
    """(y0, y1, x0, x1) evaluation box of metrics/MetricsPreprocess.py:28-43 for ``args.basic.dataset``, or None."""
    ds = args[args.basic.dataset]
    if ds.get("garg_crop", False):
        return int(0.40810811 * H), int(0.99189189 * H), int(0.03594771 * W), int(0.96405229 * W)
    if ds.get("eigen_crop", False):
        if args.basic.dataset == "kitti":
            return int(0.3324324 * H), int(0.91351351 * H), int(0.0359477 * W), int(0.96405229 * W)
        return 45, min(471, H), 41, min(601, W)
    return None


def _depth_range(args) -> Tuple[float, float]:
    """(min_depth, max_depth) of ``args.basic.dataset``."""
    ds = args[args.basic.dataset]
    return float(ds.min_depth), float(ds.max_depth)


def _empty_records(loss: bool) -> torch.Tensor:
    """The record table of no step at all: [0, 10], or [0, 16] with the loss pieces, on the host."""
    return torch.empty(0, len(RECORD_FIELDS) + (len(LOSS_FIELDS) if loss else 0))


def _call(model, *a):
    """One forward.  A captured graph is called through ``checked``: its fp16 range guard is read here (a sequential step
    reads its result next anyway) and a tripped batch re-run on the bf16-pair capture; an eager model guards itself."""
    fn = getattr(model, "checked", None)
    return fn(*a) if fn is not None else model(*a)


def _joint(model, B: int, allowed: bool = True) -> bool:
    """Whether image and mirror go through ``model`` as ONE forward over the 2B images [batch | mirrored batch]."""
    return bool(allowed and getattr(model, "images_are_independent", False) and _joint_fits(model, B))


def _split(out, B: int):
    """(un-mirrored half, mirrored half) of the output of a joint forward over [batch | mirrored batch]: views, no launch."""
    return tuple(type(out)(**{k: (None if v is None else v[s]) for k, v in out._asdict().items()}) for s in (slice(0, B), slice(B, None)))


def _forward_pair(model, halves=None, both=None, joint: bool = True):
    """(output of the un-mirrored forward, output of the mirrored forward -- still mirrored) of ``halves`` = (batch, mirrored batch)
    or of ``both`` = the 2B tensor [batch | mirrored batch], whichever the caller has: the other form is made here only on the route
    that needs it (``cat`` for the joint forward, two slices for two calls)."""
    assert (halves is None) != (both is None), "_forward_pair takes the two halves or the 2B tensor, not both and not neither"
    B = int(halves[0].shape[0]) if both is None else int(both.shape[0]) // 2
    if not _joint(model, B, joint):
        image, mirrored = (both[:B], both[B:]) if halves is None else halves
        first = _call(model, image)
        if getattr(model, "static_image", None) is not None:
            # a captured graph hands out its STATIC result tensors (bin_edges): the mirror's replay would overwrite them
            first = type(first)(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in first._asdict().items()})
        return first, _call(model, mirrored)
    if both is None:
        both = torch.cat(halves, dim=0)
    # the provider sees the mirrored images as images of their own, exactly as the reference's detector does (:173); the two
    # halves keep their own Nmax (object_group = B): bit for bit what two calls compute, up to batch-size-dependent kernel
    # dispatch (split-K, tile shapes)
    return _split(model(both, None, None, None, B) if _takes_group(model) else _call(model, both), B)


class ValidationStep:
    """``joint`` (default): image and mirror as one 2B-image forward when the model declares ``images_are_independent`` (GraphBins,
    AdaBins, a GraphedGraphBins captured for 2B images with ``object_group = B``); False: two forwards, as the reference issues
    them (A/B)."""

    def __init__(self, model, args, flip_tta: bool = True, joint: bool = True, loss: bool = False):
        self.model, self.args, self.flip_tta, self.joint, self.loss = model, args, flip_tta, joint, loss
        self.min_depth, self.max_depth = _depth_range(args)

    def _call(self, *a):
        return _call(self.model, *a)

    def _forward_pair(self, image: torch.Tensor):
        """(output of the un-mirrored forward, depth of the mirrored forward -- still mirrored, as the metric kernel wants it)."""
        out, mirror = _forward_pair(self.model, halves=(image, image.flip(dims=[3])), joint=self.joint)
        return out, mirror.depth_pred

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, depth_gt: torch.Tensor, first_image_id: int = 0):
        """-> (records [B, 10] fp32 on the device, model output namedtuple of the un-mirrored forward).  With ``loss`` the
        records are [B, 16]: RECORD_FIELDS + LOSS_FIELDS, the pieces of the reference's val/loss (``val_loss``), from the same
        pass over the ground truth; the Chamfer term reads the bin edges of the un-mirrored forward, as the reference does."""
        if self.flip_tta:
            out, mirror = self._forward_pair(image)
        else:
            out, mirror = self._call(image), None
        return _records(out.depth_pred, mirror, getattr(out, "bin_edges", None), depth_gt, self.args, self.min_depth, self.max_depth,
                        first_image_id, self.loss), out


def _records(pred, mirror, bin_edges, depth_gt, args, min_depth, max_depth, first_image_id, loss) -> torch.Tensor:
    """The metric launch of a validation step: [B, 10], or [B, 16] with the loss pieces."""
    mirror = None if mirror is None else mirror.contiguous()
    box = crop_box(args, *depth_gt.shape[2:])
    if not loss:
        return hip_ops.depth_metrics(pred.contiguous(), depth_gt.contiguous(), min_depth, max_depth, crop=box, pred_mirror=mirror,
                                     first_image_id=first_image_id)
    if bin_edges is None:
        raise ValueError("a validation step with loss=True needs the model's bin_edges (the Chamfer term), and this output has none")
    rec, lrec = hip_ops.depth_metrics_loss(pred.contiguous(), depth_gt.contiguous(), bin_edges.contiguous(), min_depth, max_depth,
                                           crop=box, pred_mirror=mirror, first_image_id=first_image_id)
    return torch.cat([rec, lrec], 1)


def _takes_group(model) -> bool:
    """Whether ``model.forward`` has the ``object_group`` argument.  A captured graph (``GraphedGraphBins``: ``__call__`` only,
    no ``forward``) does not -- its group was fixed when it was captured."""
    import inspect
    fwd = getattr(model, "forward", None)
    if fwd is None:
        return False
    try:
        return "object_group" in inspect.signature(fwd).parameters
    except (TypeError, ValueError):
        return False


def _joint_fits(model, B: int) -> bool:
    """A model of free shape takes any 2B-image batch.  A captured graph takes the joint [batch | mirrored batch] forward only
    if it was captured for exactly that: 2B images with ``object_group = B`` (each half keeps its own Nmax);
    a graph captured for B images serves the pair as two replays instead."""
    static = getattr(model, "static_image", None)
    if static is None:
        return True
    return int(static.shape[0]) == 2 * B and getattr(model, "object_group", None) == B


def hw_queue_note(slots: int) -> Optional[str]:
    """None when the environment gives ``slots`` concurrent streams hardware queues of their own, else what is wrong."""
    import os
    if slots <= 1:
        return None
    raw = os.environ.get("GPU_MAX_HW_QUEUES")
    try:
        have = int(raw) if raw is not None else None
    except ValueError:
        have = None
    if have is not None and have >= slots:
        return None
    return (f"{slots} steps in flight want GPU_MAX_HW_QUEUES >= {slots} set before the HIP runtime starts (found "
            f"{'unset: the runtime default of 4 shares queues between later streams' if raw is None else repr(raw)}); slots that "
            "share a hardware queue serialise (measured 781 vs 840 img/s)")


_Pending = namedtuple("_Pending", ["result", "graph", "flag", "kept", "depth_gt", "first_image_id", "objects"])


class _SlotPipeline:
    """``slots`` steps IN FLIGHT -- what ``PipelinedValidation`` and ``PipelinedPredictor`` share: one captured graph per slot, each on
    a stream with a hardware queue of its own, the steps dealt to the slots round-robin, and at ``collect()`` the fp16 range guard:
    every step's guard word (``g.last_flag``) read in ONE host copy, a tripped step re-run on its slot's bf16-pair capture (captured
    once, on the first trip) from the inputs kept since ``submit()``.  A subclass supplies ``_stage`` (inputs -> the graph's input and
    what a re-run is made from, on the slot's stream), ``_finish`` (graph output -> the step's result) and, where a re-run's input has
    to be made again, ``_restage``."""

    name = None                                              # the subclass's public name: in its messages and its ROUTE_REPORT key

    def __init__(self, slots: int):
        name = self.name
        if slots < 1:
            raise ValueError(f"{name}: slots must be >= 1")
        note = hw_queue_note(slots)
        if note:
            import warnings
            warnings.warn(f"{name}: {note}", RuntimeWarning, stacklevel=3)
            hip_ops.ROUTE_REPORT[name] = note
        self._slots = slots
        self._next = 0
        self._pending: List[_Pending] = []
        self.rerun_steps = 0                                 # steps re-run on bf16 pairs by collect() (fp16 range guard)

    def _capture(self, model, example: torch.Tensor, object_capacity: Optional[int], object_group: Optional[int]) -> None:
        """One graph of ``example`` ([batch | mirrored batch] with ``object_group`` = the batch, or the batch alone) per slot."""
        from .graph import GraphedGraphBins
        # slot streams that do NOT share a hardware queue (checked: hip_ops.independent_streams; the runtime's own dealing put two of
        # four consecutive streams on one queue -- 349 instead of 441 validated img/s at bs 1, profiles/r06_stream_queues.txt)
        streams = hip_ops.independent_streams(self._slots, example.device) if self._slots > 1 else [None]
        self.graphs = [GraphedGraphBins(model, example, object_capacity=object_capacity, object_group=object_group,
                                        in_flight=self._slots, stream=s) for s in streams]

    @staticmethod
    def _replay(g, staged: torch.Tensor, objects, rerun: bool = False):
        """A graph with live objects takes the caller's (None: it asks the model's provider); one with baked-in objects takes none."""
        fn = g.rerun_on_bf16 if rerun else g
        return fn(staged, *objects) if g.objects is not None else fn(staged)

    def _restage(self, kept):
        return kept

    @torch.no_grad()
    def _submit(self, inputs, held, depth_gt, first_image_id: int, objects) -> None:
        """``held``: the caller's tensors that the step reads."""
        g = self.graphs[self._next]
        self._next = (self._next + 1) % len(self.graphs)
        g.stream.wait_stream(torch.cuda.current_stream(held[0].device))     # the inputs were produced on the caller's stream
        with torch.cuda.stream(g.stream):
            staged, kept = self._stage(inputs, g)
            result = self._finish(self._replay(g, staged, objects), depth_gt, first_image_id)
        for t in held:
            t.record_stream(g.stream)                        # the caching allocator must not recycle them under the slot's launches
        # the step's inputs stay referenced until collect(): a tripped step is re-run from them
        self._pending.append(_Pending(result, g, g.last_flag, kept, depth_gt, first_image_id, objects))

    @torch.no_grad()
    def _collect(self) -> list:
        pending = self._pending
        for p in pending:
            p.graph.stream.synchronize()
        results = [p.result for p in pending]
        flags = [p.flag for p in pending if p.flag is not None]
        if flags:
            dev = flags[0].device
            hit = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev) if p.flag is None else p.flag for p in pending]).cpu()
            for i in hit.nonzero().flatten().tolist():
                p = pending[i]
                out = self._replay(p.graph, self._restage(p.kept), p.objects, rerun=True)
                results[i] = self._finish(out, p.depth_gt, p.first_image_id)
                self.rerun_steps += 1
            torch.cuda.current_stream(dev).synchronize()
        self._pending = []
        return results


class PipelinedValidation(_SlotPipeline):
    """The reference's validation loop -- one image at a time (main.py:58), model(image) and model(mirror) per image
    (modules/GraphBinsLM.py:159,173) -- with ``slots`` validation steps IN FLIGHT: each slot is a hipGraph of the joint
    [batch | mirrored batch] forward captured on a stream of its own (objcavit_amd/graph.py; live objects with
    ``object_capacity``), the steps go to the slots round-robin, the per-image records are collected at the end (or whenever the
    caller asks).  At bs 1 every launch is latency, so consecutive images overlap almost freely: measured on MI355X
    (bench.py --batch 1: the same slot mechanism) 288 img/s one after the other, 609 with three in flight, **685 - 692 with
    four** (the default; five and more collapse to 420 - 530 whatever GPU_MAX_HW_QUEUES says: the slots then share hardware queues);
    bs 2 (= image + mirror) 461 -> 817 -> 872.  Results are those of ``ValidationStep(joint=True)``: same kernels, same order per step.
    WANTS ``GPU_MAX_HW_QUEUES=4`` (= the default ``slots``) in the environment BEFORE the HIP runtime initialises: set explicitly the
    runtime deals every slot stream a hardware queue of its own (unset, its default of 4 gives only the first streams one: slots
    that share a queue run one after the other, measured 781 instead of 840 img/s); ``OCV_SET_HW_QUEUES=4`` before ``import
    objcavit_amd`` sets it, bench.py and tests/conftest.py do the same.  NOT more than 4: on 6+ queues a captured forward that forks
    side streams replays 3x slower (hip_ops.hw_queues_allow_forks), so the package then captures lone batches without forks,
    process-wide.  A smaller or unset value is accepted but WARNED about and recorded in ``hip_ops.ROUTE_REPORT["PipelinedValidation"]``.

        pv = PipelinedValidation(model, args, example_image)
        for i, (image, depth_gt) in enumerate(loader):      # bs 1, as the reference
            pv.submit(image.cuda(non_blocking=True), depth_gt.cuda(non_blocking=True), first_image_id=i)
        records = pv.collect()                                # [N, 10] per-image records, submission order
    """

    name = "PipelinedValidation"

    def __init__(self, model, args, example_image: torch.Tensor, slots: int = 4, object_capacity: Optional[int] = None,
                 flip_tta: bool = True, loss: bool = False):
        super().__init__(slots)
        self.args, self.flip_tta, self.loss = args, flip_tta, loss
        self.min_depth, self.max_depth = _depth_range(args)
        self.B = int(example_image.shape[0])
        self._capture(model, self._stage(example_image)[0], object_capacity, self.B if flip_tta else None)

    def submit(self, image: torch.Tensor, depth_gt: torch.Tensor, first_image_id: int = 0, object_features=None, object_xywh_list=None) -> None:
        """Enqueue one validation step (image [B, 3, H, W] as captured, ground truth [B, 1, H', W']) on the next slot's stream;
        returns at once.  ``object_features`` / ``object_xywh_list``: the objects of the 2B images [batch | mirrored batch] for a
        graph with ``object_capacity`` (default: the model's provider is asked, on the slot's stream).  ``object_features`` may be an
        ``objects.Detections`` when the model's provider is a ``DeviceObjectProvider``: its one launch writes the slot's static
        buffers on the slot's stream (of the batch alone with the provider's ``mirror_width`` set, else of all 2B images)."""
        if tuple(image.shape[1:]) != tuple(self.graphs[0].static_image.shape[1:]) or image.shape[0] != self.B:
            raise ValueError(f"captured for images {(self.B,) + tuple(self.graphs[0].static_image.shape[1:])}, got {tuple(image.shape)}")
        self._submit(image, [image, depth_gt], depth_gt, first_image_id, (object_features, object_xywh_list))

    def _stage(self, image: torch.Tensor, g=None):
        both = torch.cat([image, image.flip(dims=[3])], 0) if self.flip_tta else image
        return both, both

    def _finish(self, out, depth_gt: torch.Tensor, first_image_id: int) -> torch.Tensor:
        # (with ``loss``: the graph's STATIC bin_edges, un-mirrored half, read by this launch on the slot's stream before the slot's
        # next replay can overwrite them)
        B, edges = self.B, getattr(out, "bin_edges", None)
        return _records(out.depth_pred[:B], out.depth_pred[B:] if self.flip_tta else None, None if edges is None else edges[:B],
                        depth_gt, self.args, self.min_depth, self.max_depth, first_image_id, self.loss)

    def collect(self) -> torch.Tensor:
        """Wait for every submitted step; -> records [N * B, 10] ([N * B, 16] with ``loss``) in submission order (and forget them).  The steps' inputs are held
        until here (fp16 range guard: a tripped step is re-run on bf16 pairs): call it every few hundred steps on a long run."""
        recs = self._collect()
        return torch.cat(recs, 0) if recs else _empty_records(self.loss)


def totals(records: torch.Tensor) -> Dict[str, float]:
    """Pixel-total metrics over all images of a record table (the reference's non-running metric classes after an
    epoch): weights n_valid, the two RMSEs recombined through their squares."""
    r = records.double().cpu()
    n = r[:, 8]
    tot = float(n.sum()) if float(n.sum()) > 0 else 1.0
    out = {}
    for i, k in enumerate(RECORD_FIELDS[:8]):
        if k in ("rmse", "rmse_log"):
            out[k] = float(((r[:, i] ** 2) * n).sum() / tot) ** 0.5
        else:
            out[k] = float((r[:, i] * n).sum() / tot)
    out["n_valid"] = int(n.sum())
    return out


def val_loss(records: torch.Tensor, args, group: int = 1) -> Dict[str, float]:
    """The reference's ``val/loss`` from a wide record table [N, 16] (``ValidationStep(loss=True)``), in float64 on the host.
    Consecutive groups of ``group`` images are recombined as ONE reference call each -- SILog (losses/SILogLoss.py:50-56) from the
    group's sum n mean_g, sum n mean_g2, sum n (NaN for a group without a masked pixel, as there); Chamfer (pytorch3d defaults:
    point reduction mean, batch reduction mean) sum (cham_x + cham_y) / group size -- and the groups averaged weighted by their
    size.  ``group = 1`` is the reference's bs-1 epoch value (Lightning's mean of the per-step losses).
    -> {"val/loss", "silog", "bins_chamfer"}: the total weighted by ``args.loss.coeffs`` and the two unweighted components."""
    from .config import checked_loss
    if records.dim() != 2 or records.shape[1] != len(RECORD_FIELDS) + len(LOSS_FIELDS):
        raise ValueError(f"val_loss: expected the [N, 16] table of a loss=True validation step, got {tuple(records.shape)}")
    if group < 1:
        raise ValueError("val_loss: group must be >= 1")
    if args.get("loss") is None:
        raise ValueError("val_loss: args has no loss section (losses/LossWrapper.py:29)")
    cfg = checked_loss(args["loss"])
    r = records[records[:, RECORD_FIELDS.index("image_id")] >= 0].double().cpu()[:, len(RECORD_FIELDS):]
    mg, mg2, n, cx, cy = (r[:, LOSS_FIELDS.index(k)] for k in ("mean_g", "mean_g2", "n_mask", "cham_x", "cham_y"))
    comp = {"silog": 0.0, "bins_chamfer": 0.0}
    N = int(r.shape[0])
    for lo in range(0, N, group):
        s = slice(lo, min(N, lo + group))
        size = s.stop - s.start
        nt = n[s].sum()
        dg = (n[s] * mg2[s]).sum() / nt - (0.85 / nt ** 2) * (n[s] * mg[s]).sum() ** 2
        comp["silog"] += size * float(10.0 * torch.sqrt(dg))
        comp["bins_chamfer"] += size * float((cx[s] + cy[s]).sum() / size)
    out = {k: (v / N if N else float("nan")) for k, v in comp.items()}
    out["val/loss"] = sum(float(c) * out[k] for k, c in zip(cfg["names"], cfg["coeffs"]))
    return out
