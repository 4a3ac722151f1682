"""How far away is each detected object: depth statistics per detection box, read out of the predict path's final map on the device.

``object_depths(depth, boxes)`` takes the fp32 map [B, 1, H, W] of ``Predictor`` / ``hip_ops.depth_finalize`` and the boxes a detector
found in those frames -- centre x, centre y, width, height in pixels of the map's own grid (the cropped model input) -- and returns one
record per box in ONE launch (csrc/object_depth.hip), without a copy of the map to the host:

    n          number of non-NaN pixels whose centre (x + 0.5, y + 0.5) lies inside the box; 0 flags a row without a valid pixel
    min, max   smallest / largest of those pixels
    mean       their mean (float64 sum, rounded once)
    std_mean   mean of ``depth_std`` over the same pixels (0 when no ``depth_std`` is given)
    q<q>       per quantile q: v[floor(q * (n - 1))] of the sorted pixels v -- an element of the map, not an interpolation; q0.5 is the
               lower median (``torch.median``'s)

``shrink`` in (0, 1] reads the central part of every box (width and height scaled about the centre): the usual guard against
background inside a detection box.  A row beyond an image's count, a box outside the map, of no size or with NaN / inf coordinates,
the ``<UNK>`` box (-1, -1, -1, -1) of an image without detections and a box whose pixels are all NaN give an all-zero record.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence, Tuple

import torch

from . import hip_ops

OBJECT_FIELDS = ("n", "min", "max", "mean", "std_mean")
DEFAULT_QUANTILES = (0.1, 0.5, 0.9)

# table fp32 [B, cap, len(fields)] and counts int32 [B] on the device; fields: the column names
ObjectDepths = namedtuple("ObjectDepths", ["table", "counts", "fields"])


def object_fields(quantiles: Sequence[float] = DEFAULT_QUANTILES) -> Tuple[str, ...]:
    """Column names of a table: ``OBJECT_FIELDS`` + one "q<q>" per quantile ("q0.1", "q0.5", "q0.9")."""
    return OBJECT_FIELDS + tuple(f"q{float(q):g}" for q in quantiles)


def pad_boxes(boxes, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """``boxes`` in one of its three forms -> (xywh [B, cap, k >= 4], counts int32 [B] on the device): a ``PaddedObjects``, an
    ``(xywh, counts)`` pair, or the reference's list of [N_i, >= 4] tensors / None -- padded exactly as ``PaddedObjects.from_lists``
    pads (None: the one <UNK> row (-1, -1, -1, -1); the counts tensor from the same small cache)."""
    from .modules.ObjCAViT import PaddedObjects
    if isinstance(boxes, PaddedObjects):
        return boxes.xywh, boxes.counts
    if isinstance(boxes, tuple) and len(boxes) == 2 and isinstance(boxes[0], torch.Tensor) and boxes[0].dim() == 3:
        return boxes
    if isinstance(boxes, torch.Tensor) or not isinstance(boxes, (list, tuple)):
        raise TypeError("boxes: expected a PaddedObjects, an (xywh [B, cap, k], counts [B]) pair or a list of [N_i, >= 4] tensors / None")
    sizes = [1 if b is None else int(b.shape[0]) for b in boxes]
    stand_in = [torch.empty((n, 0), dtype=torch.float32, device=device) for n in sizes]        # from_lists pads features alongside
    padded = PaddedObjects.from_lists(stand_in, list(boxes), device)
    return padded.xywh, padded.counts


def object_depths(depth: torch.Tensor, boxes, depth_std: Optional[torch.Tensor] = None, quantiles: Sequence[float] = DEFAULT_QUANTILES,
                  shrink: float = 1.0, out: Optional[torch.Tensor] = None) -> ObjectDepths:
    """-> ``ObjectDepths(table, counts, fields)``: ``table`` fp32 [B, cap, 5 + Q] with the columns ``fields`` (see the module's text),
    ``counts`` the int32 [B] device tensor of valid rows per image.  ``out``: a table to write into (a pipeline slot's)."""
    xywh, counts = pad_boxes(boxes, depth.device)
    table = hip_ops.object_depth(depth, xywh, counts, depth_std=depth_std, quantiles=quantiles, shrink=shrink, out=out)
    return ObjectDepths(table, counts, object_fields(quantiles))
