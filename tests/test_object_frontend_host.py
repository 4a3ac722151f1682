"""-m "not gpu": the object front end's host side -- the relation thresholds against ``relative_size_index`` (and through it the
reference's golden), the ``PhraseTable`` builder and its host lookup, ``Detections.from_lists``, the new symbol and every refusal of
its entry point (no launch happens)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from util import load_golden
from objcavit_amd import objects
from objcavit_amd.objects import Detections, PhraseTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = (0x3e92b0c2, 0x3ef1da08, 0x3f475f7d, 0x3fa45af2, 0x40077cee, 0x405f61c8)      # ~ e^-1.25, e^-0.75, ..., e^1.25


def _bits(x: float) -> int:
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def _f32(bits: int) -> float:
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def _by_thresholds(ratio: float) -> int:
    return sum(1 for t in objects.REL_SIZE_THRESHOLDS if t <= ratio)


def test_thresholds_are_derived_pinned_and_strictly_increasing():
    t = objects.REL_SIZE_THRESHOLDS
    assert t == objects.relative_size_thresholds() and len(t) == 6
    assert tuple(_bits(x) for x in t) == PINNED
    assert all(_f32(_bits(x)) == x for x in t)                                # fp32 values, exactly
    assert all(a < b for a, b in zip(t, t[1:])) and t[0] > 0.0


def test_thresholds_reproduce_relative_size_index_on_the_golden_and_around_every_step():
    meta, z = load_golden("g7_relsize")
    seen = set()
    for i in range(meta["n_images"]):
        xywh = torch.from_numpy(z[f"xywh{i}"])
        want = objects.relative_size_index(xywh)
        assert want == z[f"idx{i}"].tolist()
        if len(want) < 2:
            continue
        area = xywh[:, 2] * xywh[:, 3]
        ratio = (area / torch.roll(area, -1)).tolist()
        assert [_by_thresholds(r) for r in ratio] == want, i
        seen.update(want)
    assert seen == set(range(7))
    # +- 50 ulp around every step, through relative_size_index itself: two boxes of areas (ratio, 1), row 0 against row 1
    for k, t in enumerate(objects.REL_SIZE_THRESHOLDS):
        for d in range(-50, 51):
            r = _f32(_bits(t) + d)
            got = objects.relative_size_index(torch.tensor([[0.0, 0.0, r, 1.0], [0.0, 0.0, 1.0, 1.0]]))[0]
            assert got == _by_thresholds(r) == (k + 1 if d >= 0 else k), (k, d)
    for r in (_f32(1), 1e-30, 1.0, 1e30, _f32(0x7f7fffff)):                    # both ends of fp32's positive range
        assert _by_thresholds(r) == objects._relation_of_ratio(r)


def _features(n, dim=8, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((n, dim)).astype(np.float32))


def test_phrase_table_finds_every_key_and_no_other():
    rs = np.random.RandomState(3)
    triples = sorted({(int(c), int(n), int(r)) for c, n, r in zip(rs.randint(0, 1204, 300), rs.randint(0, 1204, 300), rs.randint(-1, 7, 300))})
    f = _features(len(triples))
    t = PhraseTable(1204, dim=8, mapping={k: f[i] for i, k in enumerate(triples)})
    assert len(t) == len(triples) and t.slots >= 2 * len(t) and t.slots & (t.slots - 1) == 0 and t.slots < 4 * len(t)
    assert t.keys_host.dtype == np.uint64 and t.rows_host.dtype == np.int32
    assert int((t.keys_host != np.uint64(objects.EMPTY_KEY)).sum()) == len(triples)
    keys = [t.key(*k) for k in triples]
    rows = t.lookup_host(keys)
    assert sorted(rows.tolist()) == list(range(len(triples)))
    assert torch.equal(t._host[torch.from_numpy(rows).long()], f)
    assert [PhraseTable.unpack(k) for k in keys] == triples
    absent = [t.key(c, n, r) for c, n, r in ((1203, 1203, 6), (0, 0, -1), (5, 6, 2)) if (c, n, r) not in set(triples)]
    assert absent and (t.lookup_host(absent) == -1).all()
    assert t.key(1, 2, -1) == (1 << 24) | (2 << 3) and t.key(3, 1203, 6) == (3 << 24) | (1203 << 3) | 7
    for bad in ((-1, 0, 0), (1204, 0, 0), (0, 1204, 0), (0, 0, 7), (0, 0, -2)):
        with pytest.raises(ValueError):
            t.key(*bad)


def test_phrase_table_probe_chain_wraps_around_at_load_one_half():
    """Eight keys that share the LAST slot of a 16-slot table as their home: load factor exactly 0.5, a chain of eight that starts in
    slot 15 and continues in slots 0 .. 6."""
    slots, want = 16, 8
    cand = [(c, n, r) for c in range(40) for n in range(40) for r in range(-1, 7)]
    keys = np.array([(c << 24) | (n << 3) | (r + 1) for c, n, r in cand], dtype=np.uint64)
    share = [cand[i] for i in np.nonzero(PhraseTable.home(keys, slots) == slots - 1)[0][:want]]
    assert len(share) == want
    f = _features(want, seed=1)
    t = PhraseTable(40, dim=8, mapping={k: f[i] for i, k in enumerate(share)}, min_slots=2)
    assert t.slots == slots and len(t) * 2 == t.slots
    used = np.nonzero(t.keys_host != np.uint64(objects.EMPTY_KEY))[0].tolist()
    assert used == list(range(7)) + [15]                                       # wrapped around the end of the table
    rows = t.lookup_host([t.key(*k) for k in share])
    assert torch.equal(t._host[torch.from_numpy(rows).long()], f)
    others = [k for k in cand if k not in set(share)]
    same_home = [k for k in others if int(PhraseTable.home([t.key(*k)], slots)[0]) == slots - 1][:4]
    assert same_home and (t.lookup_host([t.key(*k) for k in same_home]) == -1).all()      # walks the whole chain, then an empty slot
    assert (t.lookup_host([t.key(*k) for k in others[:50]]) == -1).all()


def test_phrase_table_add_grows_replaces_and_keeps_rows():
    f = _features(40, seed=2)
    t = PhraseTable(50, dim=8, mapping={(i, i, -1): f[i] for i in range(4)})
    assert t.slots == 8 and len(t) == 4
    t.add({(i, i, -1): f[i] for i in range(4, 20)})
    assert t.slots == 64 and len(t) == 20
    rows = t.lookup_host([t.key(i, i, -1) for i in range(20)])
    assert rows.tolist() == list(range(20))                                   # earlier rows keep their place
    t.add({(2, 2, -1): f[30]})                                                # a key it holds: replaced in place
    assert len(t) == 20 and torch.equal(t._host[2], f[30]) and t.lookup_host([t.key(2, 2, -1)]).tolist() == [2]
    h = PhraseTable(50, dim=8, dtype=torch.float16, mapping={(1, 2, 3): f[0]})
    assert h._host.dtype == torch.float16 and torch.equal(h._host[0], f[0].half())
    empty = PhraseTable(50, dim=8)
    assert len(empty) == 0 and (empty.lookup_host([empty.key(1, 1, -1)]) == -1).all()
    with pytest.raises(ValueError):
        t.add({(1, 1, 0): torch.zeros(7)})
    with pytest.raises(ValueError):
        PhraseTable(1 << 21)
    with pytest.raises(TypeError):
        PhraseTable(10, dtype=torch.bfloat16)


def test_detections_from_lists_none_entries_and_capacity():
    boxes = [torch.arange(8.0).view(2, 4), None, torch.ones(1, 4), torch.zeros(0, 4)]
    cls = [torch.tensor([3, 9]), None, [7], torch.zeros(0, dtype=torch.long)]
    d = Detections.from_lists(boxes, cls, "cpu")
    assert tuple(d.xywh.shape) == (4, 2, 4) and d.capacity == 2
    assert d.counts.tolist() == [2, 0, 1, 0] and d.counts.dtype == torch.int32 and d.cls.dtype == torch.int32 and d.xywh.dtype == torch.float32
    assert torch.equal(d.xywh[0], boxes[0]) and d.cls[0].tolist() == [3, 9] and d.cls[2, 0].item() == 7 and torch.equal(d.xywh[2, 0], torch.ones(4))
    d5 = Detections.from_lists(boxes, cls, "cpu", capacity=5)
    assert tuple(d5.xywh.shape) == (4, 5, 4) and torch.equal(d5.xywh[:, :2], d.xywh) and d5.counts.tolist() == d.counts.tolist()
    assert tuple(Detections.from_lists([None], [None], "cpu").xywh.shape) == (1, 1, 4)
    with pytest.raises(ValueError):
        Detections.from_lists(boxes, cls, "cpu", capacity=1)
    with pytest.raises(ValueError):
        Detections.from_lists([torch.zeros(3, 4)], [[1, 2]], "cpu")
    with pytest.raises(TypeError):
        Detections(torch.zeros(1, 2, 4), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        Detections(torch.zeros(1, 2, 3), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


def test_provider_argument_checks():
    from objcavit_amd.objects import DeviceObjectProvider
    table, phrases = torch.zeros(4, 8), PhraseTable(4, dim=8)
    for kw in (dict(), dict(class_table=table, phrases=phrases), dict(class_table=table, fallback=table),
               dict(class_table=table, mirror_width=0.0), dict(class_table=table, mirror_width=float("inf"))):
        with pytest.raises(ValueError):
            DeviceObjectProvider(None, **kw)
    p = DeviceObjectProvider(None, phrases=phrases, fallback=table, mirror_width=640)
    assert p.dim == 8 and p.misses() == [] and p.images_out(Detections.from_lists([None], [None], "cpu")) == 2
    with pytest.raises(TypeError):
        p.write((None, None, None))


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


def test_symbol_is_declared_bound_and_exported(lib):
    from objcavit_amd import _lib, build, hip_ops
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_object_frontend_fwd\s*\(", header)
    assert re.search(r"#define\s+OCV_ABI_VERSION\s+5\b", header)
    for name, value in (("MISS", objects.FLAG_MISS), ("BAD_CLASS", objects.FLAG_BAD_CLASS), ("BAD_RATIO", objects.FLAG_BAD_RATIO),
                        ("COUNT_CLAMPED", objects.FLAG_COUNT_CLAMPED)):
        assert re.search(rf"#define\s+OCV_OBJFE_{name}\s+{value}\b", header)
    assert "ocv_object_frontend_fwd" in _lib.PROTOTYPES and "object_frontend.hip" in build.SOURCES
    assert hasattr(lib, "ocv_object_frontend_fwd") and callable(hip_ops.object_frontend)
    assert lib.ocv_abi_version() == 5 and _lib.ABI_VERSION == 5


def _call(lib, **kw):
    """The entry point with made-up (never dereferenced) device addresses: every call here must be refused before any launch."""
    a = dict(xywh=256, xywh_row_stride=4, cls=256, counts=256, B=2, cap=3, class_table=256, n_classes=10, hash_keys=256, hash_rows=256,
             slots=16, hash_features=256, n_rows=5, thresholds=(C.c_float * 6)(*objects.REL_SIZE_THRESHOLDS), f16=0, F=8, mirror_width=0.0,
             features=256, feat_image_stride=32, feat_row_stride=8, xywh_out=256, xywh_out_image_stride=16, xywh_out_row_stride=4,
             counts_out=256, cap_out=4, rows=256, keys=256, flags=256)
    a.update(kw)
    if isinstance(a["thresholds"], (tuple, list)):
        a["thresholds"] = (C.c_float * 6)(*a["thresholds"])
    return lib.ocv_object_frontend_fwd(*a.values(), None)


T = objects.REL_SIZE_THRESHOLDS


@pytest.mark.parametrize("kw,word", [
    (dict(xywh=None), "null pointer"), (dict(cls=None), "null pointer"), (dict(counts=None), "null pointer"),
    (dict(features=None), "null pointer"), (dict(xywh_out=None), "null pointer"), (dict(counts_out=None), "null pointer"),
    (dict(rows=None), "null pointer"), (dict(keys=None), "null pointer"), (dict(flags=None), "null pointer"),
    (dict(class_table=None, hash_keys=None, hash_rows=None, hash_features=None), "no table"),
    (dict(hash_keys=None), "null pointer"), (dict(hash_rows=None), "null pointer"), (dict(hash_features=None), "null pointer"),
    (dict(thresholds=None), "null pointer"),
    (dict(B=0), "bad sizes"), (dict(cap=0), "bad sizes"), (dict(B=1 << 30, cap=2), "bad sizes"),
    (dict(F=0), "multiple of 4"), (dict(F=6), "multiple of 4"), (dict(F=-4), "multiple of 4"),
    (dict(n_classes=0), "n_classes"), (dict(n_classes=(1 << 20) + 1), "n_classes"),
    (dict(cap_out=2), "cap_out"),
    (dict(xywh_row_stride=3), "box strides"), (dict(xywh_out_row_stride=3), "box strides"), (dict(xywh_out_image_stride=15), "box strides"),
    (dict(feat_row_stride=4), "feature strides"), (dict(feat_row_stride=10, feat_image_stride=40), "feature strides"),
    (dict(feat_image_stride=31), "feature strides"), (dict(feat_image_stride=34), "feature strides"),
    (dict(mirror_width=-1.0), "mirror_width"), (dict(mirror_width=float("nan")), "mirror_width"), (dict(mirror_width=float("inf")), "mirror_width"),
    (dict(slots=0), "power of two"), (dict(slots=12), "power of two"), (dict(slots=1), "power of two"),
    (dict(n_rows=0), "n_rows"),
    (dict(thresholds=(T[0], T[1], T[1], T[3], T[4], T[5])), "thresholds"), (dict(thresholds=(0.0,) + T[1:]), "thresholds"),
    (dict(thresholds=T[:5] + (float("nan"),)), "thresholds"), (dict(thresholds=T[:5] + (float("inf"),)), "thresholds"),
    (dict(features=264), "16-byte aligned"), (dict(class_table=264), "16-byte aligned"), (dict(hash_features=264), "16-byte aligned"),
    (dict(hash_keys=260), "misaligned"), (dict(hash_rows=258), "misaligned"), (dict(keys=260), "misaligned"), (dict(cls=258), "misaligned"),
    (dict(xywh=258), "misaligned"), (dict(rows=258), "misaligned"),
])
def test_bad_arguments_are_refused_with_a_message_before_any_launch(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_object_frontend_fwd:") and word in msg, msg


def test_wrapper_refuses_host_tensors_and_bad_operands():
    from objcavit_amd import hip_ops
    from objcavit_amd._lib import HipLibraryError
    d = Detections.from_lists([torch.zeros(2, 4)], [[1, 2]], "cpu")
    with pytest.raises(HipLibraryError):
        hip_ops.object_frontend(d.xywh, d.cls, d.counts, class_table=torch.zeros(4, 8))
    assert hip_ops.object_frontend.__defaults__ == (None,) * 5
