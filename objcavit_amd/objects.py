"""Object front-end formats (row N4 of SURVEY.md section 8f): what the frozen detector + phrase builder + CLIP hand to
the hot path, and a table-driven provider that replaces the last two with one gather.

Formats (modules/Yolov7Wrapper.py:45-150, modules/GraphBins.py:90-107), per image of a batch, all optional (None = no
detection in that image):
  xywh  [N, 4] fp32   bounding boxes, centre x, centre y, width, height in full-resolution pixels
  cls   [N]    int    class index of the detector (LVIS: 0..1203)
  names N strings     class labels (LVIS: WordNet synsets "chair.n.01")
The reference turns (names, boxes) into a phrase per object (modules/ObjectLanguageStrategy.py:128-179) and the phrase
into a 512-d CLIP text feature (modules/CLIPWrapper.py:21-24, un-normalised, cast .float() at GraphBins.py:106).  For
the strategies whose phrase depends on the class only ("none", "synset_def_wn") that is a fixed [n_classes, 512] table;
for "name_synset_def_wn_rel_sz" the phrase also names the next object and one of 7 size relations, so the table key is
(class, next class, relation) -- a phrase cache filled by whoever owns CLIP.  ``TableObjectProvider`` is the device
side of both: detections in, ``(features_list, xywh_list, None)`` out -- the ``object_provider`` of ``GraphBins`` --
with no CLIP in the loop.  ``DeviceObjectProvider`` is the same front end for detections that stay on the device
(``Detections``): one launch of csrc/object_frontend.hip, the phrase cache as a hash table (``PhraseTable``), no host read.

Parity: the relation index below restates ObjectLanguageStrategy.py:69-81 and is PINNED: tests/golden/make_golden.py g7
runs the reference's own get_single_relative_size_clause (nltk, imported at the module top but unused by that method,
replaced by an empty stand-in module) on boxes that include equal areas, both ends of the scale and the half-way points
of the rounding; tests/golden/g7_relsize.npz holds its clauses and relation indices.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .modules.ObjCAViT import PaddedObjects

REL_SIZE_SCALE = ("much smaller than", "smaller than", "a bit smaller than", "about the same size as",
                  "a bit bigger than", "bigger than", "much bigger than")          # ObjectLanguageStrategy.py:23-31


def relative_size_index(xywh: torch.Tensor) -> List[int]:
    """Index into REL_SIZE_SCALE for every object of one image against the NEXT object of the list (cyclic),
    ObjectLanguageStrategy.py:69-81: ratio of box areas -> log -> [1/e, e] mapped onto the 5 middle entries, rounded
    (numpy's round-half-to-even), clipped to the 7-entry scale.  Empty for fewer than 2 objects (no clause is made)."""
    n = 0 if xywh is None else int(xywh.shape[0])
    if n <= 1:
        return []
    # the reference multiplies and divides 0-d fp32 TENSORS (obj_xywh[2] * obj_xywh[3], area / next_area) and only then
    # leaves torch (math.log of the fp32 quotient): areas and the ratio are rounded to fp32, the rest is double
    b = xywh.detach().to("cpu", torch.float32)
    area = b[:, 2] * b[:, 3]
    ratio = (area / torch.roll(area, -1)).tolist()
    out = []
    L = len(REL_SIZE_SCALE)
    for j in range(n):
        f = (math.log(ratio[j]) + 1.0) / 2.0 * (L - 3)
        r = round(f) + 1                      # Python's round == numpy's: half to even
        out.append(int(min(max(r, 0), L - 1)))
    return out


class TableObjectProvider:
    """``object_provider`` for ``GraphBins`` backed by precomputed text features.

    ``detector(image) -> (xywh_list, cls_list)`` supplies the detections in the formats above (lists of length B,
    entries None where nothing was found).  ``class_table`` is [n_classes, 512] (phrase depends on the class only);
    alternatively ``phrase_features(cls_i, cls_next, relation) -> 512-d tensor`` serves the relative-size strategy
    from its cache.  An image without detections gets ONE zero feature and no box, as the reference does
    (LanguageEmbeddingWrapper.py:56-61 with cls = [0]; ObjCAViT.py handles xywh None)."""

    def __init__(self, detector: Callable, class_table: Optional[torch.Tensor] = None,
                 phrase_features: Optional[Callable[[int, int, int], torch.Tensor]] = None, dim: int = 512):
        if (class_table is None) == (phrase_features is None):
            raise ValueError("TableObjectProvider: give exactly one of class_table / phrase_features")
        if class_table is not None and (class_table.dim() != 2 or class_table.shape[1] != dim):
            raise ValueError(f"TableObjectProvider: class_table must be [n_classes, {dim}]")
        self.detector, self.table, self.phrase_features, self.dim = detector, class_table, phrase_features, dim

    def __call__(self, image: torch.Tensor):
        xywh_list, cls_list = self.detector(image)
        if len(xywh_list) != image.shape[0] or len(cls_list) != image.shape[0]:
            raise ValueError("TableObjectProvider: the detector must return one entry per image")
        dev = image.device
        feats: List[torch.Tensor] = []
        boxes: List[Optional[torch.Tensor]] = []
        for xywh, cls in zip(xywh_list, cls_list):
            if cls is None or len(cls) == 0:
                feats.append(torch.zeros(1, self.dim, dtype=torch.float32, device=dev))
                boxes.append(None)
                continue
            cls = torch.as_tensor(cls, device=dev).long()
            if xywh is None or xywh.shape != (cls.shape[0], 4):
                raise ValueError("TableObjectProvider: xywh must be [N, 4] for N classes")
            if self.table is not None:
                if int(cls.min()) < 0 or int(cls.max()) >= self.table.shape[0]:
                    raise ValueError("TableObjectProvider: class index outside the table")
                f = self.table.to(dev).index_select(0, cls).float()
            else:
                rel = relative_size_index(xywh)
                c = cls.tolist()
                n = len(c)
                f = torch.stack([self.phrase_features(c[j], c[(j + 1) % n], rel[j] if rel else -1).to(dev).float()
                                 for j in range(n)], 0)
            feats.append(f)
            boxes.append(xywh.to(dev).float())
        return feats, boxes, None


# ---------------------------------------------------------------------------
# the same front end on the device (csrc/object_frontend.hip): detections in shape-static form, the phrase cache as a hash table
# ---------------------------------------------------------------------------
FLAG_MISS, FLAG_BAD_CLASS, FLAG_BAD_RATIO, FLAG_COUNT_CLAMPED = 1, 2, 4, 8        # include/objcavit_hip.h: OCV_OBJFE_*
MAX_CLASSES = 1 << 20
EMPTY_KEY = (1 << 64) - 1


def _relation_of_ratio(ratio: float) -> int:
    """``relative_size_index``'s arithmetic on ONE fp32 ratio (given as a Python float): the reference's formula in double."""
    L = len(REL_SIZE_SCALE)
    f = (math.log(ratio) + 1.0) / 2.0 * (L - 3)
    return int(min(max(round(f) + 1, 0), L - 1))


def _f32_of_bits(bits: int) -> float:
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def relative_size_thresholds() -> Tuple[float, ...]:
    """The six fp32 values t_1 < ... < t_6 with  relation(ratio) == #{k: t_k <= ratio}  for every finite positive fp32 ratio.  The
    relation is a non-decreasing step function of the ratio, and positive fp32 values order as their bit patterns do, so step k is
    found by bisection over bit patterns, the reference's own formula evaluated at every probe (the device of
    ``predict.normalisation_table``: equal to the reference by construction, nothing re-derived in another precision)."""
    out = []
    for k in range(1, len(REL_SIZE_SCALE)):
        lo, hi = 1, 0x7f7fffff                       # smallest subnormal (relation 0) .. largest finite (relation 6)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _relation_of_ratio(_f32_of_bits(mid)) >= k:
                hi = mid
            else:
                lo = mid
        out.append(_f32_of_bits(hi))
    return tuple(out)


REL_SIZE_THRESHOLDS = relative_size_thresholds()      # derived at import; tests/test_object_frontend_host.py pins the bit patterns


class Detections:
    """A detector's SELECTED detections of a batch in shape-static form, all on the device: ``xywh`` fp32 [B, cap, >= 4] (centre x,
    centre y, width, height; rows may be wider than 4 and strided, as ``PaddedObjects.xywh``), ``cls`` int32 [B, cap], ``counts``
    int32 [B].  ``counts[b] == 0`` = nothing found in image b; rows at or beyond the count are never read."""
    __slots__ = ("xywh", "cls", "counts")

    def __init__(self, xywh: torch.Tensor, cls: torch.Tensor, counts: torch.Tensor):
        if xywh.dim() != 3 or xywh.shape[2] < 4 or cls.shape != xywh.shape[:2] or counts.shape != xywh.shape[:1]:
            raise ValueError("Detections: expected xywh [B, cap, >= 4], cls [B, cap], counts [B]")
        if xywh.dtype != torch.float32 or cls.dtype != torch.int32 or counts.dtype != torch.int32:
            raise TypeError("Detections: xywh must be float32, cls and counts int32")
        if xywh.shape[0] < 1 or xywh.shape[1] < 1:
            raise ValueError("Detections: B and cap must be >= 1")
        self.xywh, self.cls, self.counts = xywh, cls, counts

    @property
    def capacity(self) -> int:
        return int(self.xywh.shape[1])

    @staticmethod
    def from_lists(xywh_list, cls_list, device, capacity: Optional[int] = None) -> "Detections":
        """The reference's per-image lists ([N_i, 4] boxes, N_i classes; None or empty = nothing found) -> padded tensors.  Built on the
        host and uploaded: for tests and for detectors that live on the host."""
        if len(xywh_list) != len(cls_list) or len(cls_list) < 1:
            raise ValueError("Detections.from_lists: one entry per image in both lists")
        cls_np = [np.zeros(0, np.int32) if c is None else np.asarray(torch.as_tensor(c).cpu(), dtype=np.int32).reshape(-1) for c in cls_list]
        counts = [int(c.shape[0]) for c in cls_np]
        cap = max(max(counts), int(capacity or 0), 1)
        if capacity is not None and max(counts) > capacity:
            raise ValueError(f"Detections.from_lists: an image has {max(counts)} detections, capacity is {capacity}")
        B = len(counts)
        xywh, cls = np.zeros((B, cap, 4), np.float32), np.zeros((B, cap), np.int32)
        for b, (box, c) in enumerate(zip(xywh_list, cls_np)):
            if counts[b] == 0:
                continue
            box = np.asarray(torch.as_tensor(box).detach().cpu(), dtype=np.float32)
            if box.shape != (counts[b], 4):
                raise ValueError("Detections.from_lists: xywh must be [N, 4] for N classes")
            xywh[b, :counts[b]], cls[b, :counts[b]] = box, c
        return Detections(torch.from_numpy(xywh).to(device), torch.from_numpy(cls).to(device),
                          torch.tensor(counts, dtype=torch.int32).to(device))


class PhraseTable:
    """The phrase cache of the relative-size strategy as a device lookup: (class, next class, relation) -> a row of text features.

    A dense table would be n_classes^2 x 8 rows; this is an open-addressing hash table BUILT ON THE HOST (numpy) and READ ON THE
    DEVICE.  ``key = cls << 24 | next << 3 | (rel + 1)`` (uint64; classes below 2^20; rel in -1 .. 6, -1 = the phrase of a lone object,
    whose ``next`` is the object itself); ``keys`` uint64 [slots], slots a power of two >= 2 x entries, the empty slot all ones;
    ``rows`` int32 [slots]; ``features`` [M, dim] fp32 or fp16 (CLIP's text features are fp16 widened by ``.float()``, reference
    GraphBins.py:106 -- the widening is exact, so fp16 storage halves the table at no change in value).  Linear probing from
    ``splitmix64_finaliser(key) & (slots - 1)``.  ``lookup_host`` is the host model of the device's probe."""

    def __init__(self, n_classes: int, dim: int = 512, dtype: torch.dtype = torch.float32, device=None,
                 mapping: Optional[Dict[Tuple[int, int, int], torch.Tensor]] = None, min_slots: int = 8):
        if not 1 <= int(n_classes) <= MAX_CLASSES:
            raise ValueError(f"PhraseTable: n_classes must be in [1, 2^20], got {n_classes}")
        if dtype not in (torch.float32, torch.float16):
            raise TypeError("PhraseTable: features are stored as float32 or float16")
        if dim < 4 or dim % 4:
            raise ValueError("PhraseTable: dim must be a positive multiple of 4")
        if min_slots < 2 or min_slots & (min_slots - 1):
            raise ValueError("PhraseTable: min_slots must be a power of two >= 2")
        self.n_classes, self.dim, self.dtype, self.device, self.min_slots = int(n_classes), int(dim), dtype, device, int(min_slots)
        self._index: Dict[int, int] = {}                              # key -> feature row
        self._host = torch.zeros(0, dim, dtype=dtype)                 # the rows, on the host, in insertion order
        self.keys_host = self.rows_host = None                        # numpy: the table as uploaded
        self.keys = self.rows = self.features = None                  # device tensors (keys as int64 bit patterns)
        self.add(mapping or {})

    def __len__(self) -> int:
        return len(self._index)

    @property
    def slots(self) -> int:
        return int(self.keys_host.shape[0])

    def key(self, cls: int, nxt: int, rel: int) -> int:
        if not (0 <= cls < self.n_classes and 0 <= nxt < self.n_classes and -1 <= rel <= 6):
            raise ValueError(f"PhraseTable: ({cls}, {nxt}, {rel}) outside classes [0, {self.n_classes}) / relations [-1, 6]")
        return (int(cls) << 24) | (int(nxt) << 3) | (int(rel) + 1)

    @staticmethod
    def unpack(key: int) -> Tuple[int, int, int]:
        return int(key) >> 24, (int(key) >> 3) & (MAX_CLASSES * 2 - 1), (int(key) & 7) - 1

    @staticmethod
    def home(keys, slots: int) -> np.ndarray:
        """The slot probing starts from: the splitmix64 finaliser of the key, masked."""
        z = np.atleast_1d(np.asarray(keys, dtype=np.uint64)).copy()
        with np.errstate(over="ignore"):
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
            z = z ^ (z >> np.uint64(31))
        return (z & np.uint64(slots - 1)).astype(np.int64)

    @staticmethod
    def build(keys: Sequence[int], rows: Sequence[int], min_slots: int = 8) -> Tuple[np.ndarray, np.ndarray]:
        """(keys uint64 [slots], rows int32 [slots]): the smallest power of two >= max(2 x entries, min_slots), keys inserted in
        ascending order (the layout is a function of the key set alone)."""
        slots = min_slots
        while slots < 2 * len(keys):
            slots *= 2
        tk, tr = np.full(slots, EMPTY_KEY, dtype=np.uint64), np.full(slots, -1, dtype=np.int32)
        order = np.argsort(np.asarray(keys, dtype=np.uint64), kind="stable") if len(keys) else []
        homes = PhraseTable.home(np.asarray(keys, dtype=np.uint64), slots) if len(keys) else []
        for i in order:
            h = int(homes[i])
            while tk[h] != np.uint64(EMPTY_KEY):
                if tk[h] == np.uint64(keys[i]):
                    raise ValueError(f"PhraseTable.build: key {keys[i]} given twice")
                h = (h + 1) & (slots - 1)
            tk[h], tr[h] = np.uint64(keys[i]), rows[i]
        return tk, tr

    def lookup_host(self, keys) -> np.ndarray:
        """rows int32 of ``keys`` (-1 = absent): the probe sequence the kernel walks, on the host copy of the table."""
        keys = np.atleast_1d(np.asarray(keys, dtype=np.uint64))
        out = np.full(keys.shape[0], -1, dtype=np.int32)
        slots = self.slots
        for i, (k, h) in enumerate(zip(keys, self.home(keys, slots))):
            h = int(h)
            for _ in range(slots):
                if self.keys_host[h] == k:
                    out[i] = self.rows_host[h]
                    break
                if self.keys_host[h] == np.uint64(EMPTY_KEY):
                    break
                h = (h + 1) & (slots - 1)
        return out

    def add(self, mapping: Dict[Tuple[int, int, int], torch.Tensor]) -> None:
        """Insert (or replace) the features of ``(cls, next, rel)`` triples, rebuild the table and upload it: NEW device tensors
        replace the old ones.  A call for a moment when no step is in flight (after ``collect()``): launches already enqueued keep
        reading the tensors they were given, later ones see the new table."""
        new = []
        for (c, n, r), f in mapping.items():
            f = torch.as_tensor(f).detach().to("cpu").reshape(-1)
            if f.numel() != self.dim:
                raise ValueError(f"PhraseTable.add: features must have {self.dim} elements")
            k, f = self.key(c, n, r), f.to(self.dtype)
            if k in self._index:
                self._host[self._index[k]] = f
            else:
                self._index[k] = self._host.shape[0] + len(new)
                new.append(f)
        if new:
            self._host = torch.cat([self._host, torch.stack(new, 0)], 0)
        ks = list(self._index)
        self.keys_host, self.rows_host = self.build(ks, [self._index[k] for k in ks], self.min_slots)
        if self.device is not None:
            dev = self.device
            self.keys = torch.from_numpy(self.keys_host.view(np.int64).copy()).to(dev)
            self.rows = torch.from_numpy(self.rows_host.copy()).to(dev)
            # (a table without entries still hands the kernel one addressable row: every lookup misses)
            self.features = (self._host if len(ks) else torch.zeros(1, self.dim, dtype=self.dtype)).to(dev).contiguous()


class DeviceObjectProvider:
    """``object_provider`` for ``GraphBins`` / ``GraphedGraphBins`` that does ``TableObjectProvider``'s work in ONE launch and
    without a host read (``hip_ops.object_frontend``).  ``detector(image) -> Detections``.  Exactly one of ``class_table``
    ([n_classes, F] fp32 / fp16 on the device: the phrase depends on the class only) and ``phrases`` (a ``PhraseTable``: the
    relative-size strategy); with ``phrases``, ``fallback`` ([n_classes, F], the table's element type) supplies the feature of a
    (class, next, relation) the table does not hold yet -- without it such an object gets a zero feature.

    The device cannot raise where ``TableObjectProvider`` does: a class outside the table, an area ratio that is not a finite
    positive number and a count beyond the capacity are FLAGGED per row (``last`` holds the most recent ``rows`` / ``keys`` /
    ``flags``; FLAG_* above) and served as the header of ``ocv_object_frontend_fwd`` states.

    ``mirror_width = W``: the output describes the joint [batch | mirrored batch] forward -- image b + B carries image b's rows
    with ``cx -> W - cx``, same order, same features; the detector is handed the un-mirrored half.  The reference runs its detector
    again on the mirrored frame (GraphBinsLM.py:173); mirrored boxes are what a flip-EQUIVARIANT detector would return there and
    nothing more, so this is opt-in."""

    def __init__(self, detector: Optional[Callable], class_table: Optional[torch.Tensor] = None, phrases: Optional[PhraseTable] = None,
                 fallback: Optional[torch.Tensor] = None, mirror_width: Optional[float] = None):
        if (class_table is None) == (phrases is None):
            raise ValueError("DeviceObjectProvider: give exactly one of class_table / phrases")
        if fallback is not None and phrases is None:
            raise ValueError("DeviceObjectProvider: fallback goes with phrases (a dense class_table has no misses to fall back from)")
        if mirror_width is not None and not (0.0 < float(mirror_width) < float("inf")):
            raise ValueError("DeviceObjectProvider: mirror_width must be a positive width in pixels")
        self.detector, self.class_table, self.phrases, self.fallback = detector, class_table, phrases, fallback
        self.mirror_width = None if mirror_width is None else float(mirror_width)
        self.last: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None

    @property
    def dim(self) -> int:
        return int(self.class_table.shape[1]) if self.phrases is None else self.phrases.dim

    def images_out(self, dets: Detections) -> int:
        return int(dets.xywh.shape[0]) * (2 if self.mirror_width else 1)

    def write(self, dets: Detections, static: Optional[PaddedObjects] = None) -> PaddedObjects:
        """One launch on the current stream: ``dets`` -> ``static``'s ``features`` / ``xywh`` / ``counts`` (e.g. the static buffers of
        a captured graph, of at least the detections' capacity: rows beyond that capacity are not touched), or new tensors."""
        if not isinstance(dets, Detections):
            raise TypeError("DeviceObjectProvider: expected a Detections")
        from . import hip_ops
        out = None if static is None else (static.features, static.xywh, static.counts)
        f, x, c, rows, keys, flags = hip_ops.object_frontend(dets.xywh, dets.cls, dets.counts, class_table=self.class_table,
                                                            phrases=self.phrases, fallback=self.fallback,
                                                            mirror_width=self.mirror_width, out=out)
        self.last = (rows, keys, flags)
        return static if static is not None else PaddedObjects(f, x, c)

    def _detect(self, image: torch.Tensor) -> Detections:
        if self.mirror_width:
            if image.shape[0] % 2:
                raise ValueError("DeviceObjectProvider: with mirror_width the batch is [batch | mirrored batch]")
            image = image[: image.shape[0] // 2]
        dets = self.detector(image)
        if not isinstance(dets, Detections) or dets.xywh.shape[0] != image.shape[0]:
            raise ValueError("DeviceObjectProvider: the detector must return a Detections with one entry per image")
        return dets

    def padded(self, image: torch.Tensor) -> PaddedObjects:
        """The entry point ``GraphBins`` and ``GraphedGraphBins.load_objects`` prefer: outputs allocated, one launch."""
        return self.write(self._detect(image))

    def __call__(self, image: torch.Tensor):
        """The list protocol, for completeness: ``padded`` sliced by the counts -- which READS THE COUNTS ON THE HOST."""
        po = self.padded(image)
        n = po.counts.tolist()
        return [po.features[b, :k] for b, k in enumerate(n)], [po.xywh[b, :k, :4] for b, k in enumerate(n)], None

    def misses(self, rows: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None) -> List[Tuple[int, int, int]]:
        """The one deliberate host read: the unique ``(cls, next, rel)`` triples that were looked up and not found (default: in the
        most recent launch), sorted.  The owner of CLIP computes their features and hands them to ``PhraseTable.add``."""
        if rows is None or keys is None:
            if self.last is None:
                return []
            rows, keys = self.last[0], self.last[1]
        r = rows.detach().cpu().numpy().reshape(-1)
        k = keys.detach().cpu().view(torch.int64).numpy().reshape(-1).view(np.uint64)
        missed = np.unique(k[(r < 0) & (k != np.uint64(EMPTY_KEY))])
        return [PhraseTable.unpack(int(v)) for v in missed]
