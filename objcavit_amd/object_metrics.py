"""How wrong is the depth ON the objects: the validation metrics per detection box, and over objects against background, on the device.

``object_metrics(pred, depth_gt, boxes, args)`` takes what a validation step's metric launch takes -- the model's ``depth_pred``
[B, 1, h, w] (and the mirrored forward's, still mirrored), the ground truth [B, 1, H, W], the dataset's depth range and evaluation crop
from ``args`` -- plus the boxes a detector found, centre x, centre y, width, height in pixels of the ground truth's grid, and returns in
three launches (csrc/object_metrics.hip), without a copy of a map to the host:

    table    fp32 [B, cap, 10]: per box the eight metrics of the image record (``dp.RECORD_FIELDS[:8]``) over the box's VALID pixels
             (min_depth < gt <= max_depth inside the crop), then ``n_valid`` and ``gt_mean`` (the mean ground truth there: bin the
             error by distance with it).  Overlapping boxes each count their own pixels.
    regions  fp32 [B, 2, 10]: the same record over the valid pixels under ANY box of the image (row 0, a pixel counts once) and under
             none (row 1).  The two ``n_valid`` add up to the image record's; their n-weighted recombination is the image record.

The per-pixel value is the metric launch's own (clamp, TTA average, bilinear resize, nan / inf fix), the box-to-pixels rule is
``object_depth``'s (``shrink`` included).  A row beyond an image's count, an empty box, the ``<UNK>`` box and a box without a valid pixel
give an all-zero record: ``n_valid = 0`` is the flag.  ``totals`` summarises collected tables on the host.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, Optional

import torch

from . import hip_ops
from .dp import RECORD_FIELDS
from .object_depth import pad_boxes
from .validation import _depth_range, crop_box

OBJECT_METRIC_FIELDS = RECORD_FIELDS[:8] + ("n_valid", "gt_mean")

# table fp32 [B, cap, 10], regions fp32 [B, 2, 10] or None, counts int32 [B] on the device; fields: the column names
ObjectMetrics = namedtuple("ObjectMetrics", ["table", "regions", "counts", "fields"])


def object_metrics(pred: torch.Tensor, depth_gt: torch.Tensor, boxes, args, pred_mirror: Optional[torch.Tensor] = None,
                   shrink: float = 1.0, regions: bool = True) -> ObjectMetrics:
    """-> ``ObjectMetrics(table, regions, counts, fields)`` (see the module's text).  ``boxes``: a ``PaddedObjects``, an (xywh, counts)
    pair or a list of [N_i, >= 4] tensors / None, as ``object_depth.pad_boxes`` takes them; depth range and crop: those of
    ``args.basic.dataset``, as a validation step applies them; ``regions=False`` leaves the region pass out (``regions`` is None)."""
    xywh, counts = pad_boxes(boxes, pred.device)
    min_depth, max_depth = _depth_range(args)
    table, reg = hip_ops.object_metrics(pred.contiguous(), depth_gt.contiguous(), xywh, counts, min_depth, max_depth,
                                        crop=crop_box(args, *depth_gt.shape[2:]),
                                        pred_mirror=None if pred_mirror is None else pred_mirror.contiguous(), shrink=shrink,
                                        regions=regions)
    return ObjectMetrics(table, reg, counts, OBJECT_METRIC_FIELDS)


def _pixel_totals(rows: torch.Tensor) -> Dict[str, float]:
    """Pixel-total record of [N, 10] rows (float64): weights n_valid, the RMSEs through their squares -- ``validation.totals``' rule."""
    n = rows[:, 8]
    tot = float(n.sum())
    div = tot if tot > 0 else 1.0
    out = {}
    for i, k in enumerate(OBJECT_METRIC_FIELDS[:8]):
        out[k] = float(((rows[:, i] ** 2) * n).sum() / div) ** 0.5 if k in ("rmse", "rmse_log") else float((rows[:, i] * n).sum() / div)
    out["n_valid"] = int(tot)
    out["gt_mean"] = float((rows[:, 9] * n).sum() / div)
    return out


def _box_means(rows: torch.Tensor) -> Dict[str, float]:
    """Every box one vote: the plain mean of each column over the rows with a valid pixel, and how many those are."""
    rows = rows[rows[:, 8] > 0]
    out = {k: (float(rows[:, i].mean()) if len(rows) else 0.0) for i, k in enumerate(OBJECT_METRIC_FIELDS) if k != "n_valid"}
    out["boxes"] = int(len(rows))
    return out


def totals(results, groups=None) -> Dict[str, dict]:
    """Summary of one ``ObjectMetrics`` or a sequence of them (the collected steps of a run), on the host in float64:

        "objects"     {"pixels": pixel totals over the regions' row 0 (None without regions), "boxes": per-box means}
        "background"  {"pixels": pixel totals over the regions' row 1 (None without regions)}
        "groups"      with ``groups`` -- an integer label per box row ([B, cap] like ``table[..., 0]``; a sequence of them for a sequence
                      of results), a class id for instance --: {label: {"pixels": pixel totals over the label's boxes (a pixel under
                      two of them counts twice), "boxes": per-box means}}

    Pixel totals are n-weighted, the two RMSEs recombined through their squares (``validation.totals``), ``gt_mean`` n-weighted too;
    per-box means run over the boxes with ``n_valid > 0`` ("boxes": their number)."""
    if isinstance(results, ObjectMetrics):
        results, groups = [results], (None if groups is None else [groups])
    results = list(results)
    rows = torch.cat([r.table.detach().double().cpu().reshape(-1, len(OBJECT_METRIC_FIELDS)) for r in results], 0) if results \
        else torch.zeros(0, len(OBJECT_METRIC_FIELDS), dtype=torch.float64)
    regs = [r.regions.detach().double().cpu() for r in results if r.regions is not None]
    reg = torch.cat(regs, 0) if regs else None
    out = {"objects": {"pixels": None if reg is None else _pixel_totals(reg[:, 0]), "boxes": _box_means(rows)},
           "background": {"pixels": None if reg is None else _pixel_totals(reg[:, 1])}}
    if groups is not None:
        groups = list(groups)
        if len(groups) != len(results):
            raise ValueError(f"totals: {len(groups)} group tensor(s) for {len(results)} result(s)")
        for g, r in zip(groups, results):
            if tuple(torch.as_tensor(g).shape) != tuple(r.table.shape[:2]):
                raise ValueError(f"totals: groups must label every box row {tuple(r.table.shape[:2])}, got {tuple(torch.as_tensor(g).shape)}")
        labels = torch.cat([torch.as_tensor(g).detach().cpu().reshape(-1).to(torch.int64) for g in groups], 0) if groups \
            else torch.zeros(0, dtype=torch.int64)
        live = rows[:, 8] > 0
        out["groups"] = {int(v): {"pixels": _pixel_totals(rows[live & (labels == v)]), "boxes": _box_means(rows[live & (labels == v)])}
                         for v in sorted(set(labels[live].tolist()))}
    return out
