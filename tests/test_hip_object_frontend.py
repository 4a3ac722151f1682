"""-m gpu: the object front end on the device (csrc/object_frontend.hip) -- pinned to the reference's relation indices
(tests/golden/g7_relsize.npz) and to what ``TableObjectProvider`` + ``PaddedObjects.from_lists`` produce on the host, bit for bit; the
relation's steps to the ulp; degenerate rows, misses, the dense mode, the mirrored half; and under a captured graph, where a
``Detections`` replaces the provider's lists."""
import math

import numpy as np
import pytest
import torch

import gen
from objcavit_amd import objects
from objcavit_amd.objects import (FLAG_BAD_CLASS, FLAG_BAD_RATIO, FLAG_COUNT_CLAMPED, FLAG_MISS, Detections, DeviceObjectProvider,
                                  PhraseTable, TableObjectProvider)
from util import load_golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
NCLS = 12
EMPTY = np.uint64(objects.EMPTY_KEY)


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


class _Golden:
    """The seven images of g7_relsize.npz with classes drawn from 12, and per feature width F what the HOST path makes of them --
    computed once, shared, never modified."""

    def __init__(self):
        meta, z = load_golden("g7_relsize")
        self.n = meta["n_images"]
        self.xywh = [torch.from_numpy(z[f"xywh{i}"]) for i in range(self.n)]
        self.idx = [z[f"idx{i}"].tolist() for i in range(self.n)]
        rs = np.random.RandomState(7)
        self.cls = [torch.from_numpy(rs.randint(0, NCLS, b.shape[0]).astype(np.int64)) for b in self.xywh]
        assert [int(b.shape[0]) for b in self.xywh] == [12, 3, 13, 2, 1, 2, 0]
        self._host = {}

    def dets(self, capacity=None):
        return Detections.from_lists(self.xywh, self.cls, "cuda", capacity=capacity)

    def cube(self, F, half):
        """Phrase features of every (class, next, relation): [12, 12, 8, F]; ``half``: values an fp16 table holds exactly."""
        c = gen.randn(f"cube{F}", (NCLS, NCLS, 8, F), 5, 10.0 / np.sqrt(512))
        return c.half().float() if half else c

    def host(self, F, half):
        """(PaddedObjects at capacity 16 from the host path, the (cls, next, rel) triples it asked for)."""
        key = (F, half)
        if key not in self._host:
            cube, asked = self.cube(F, half), []

            def phrase(c, n, r):
                asked.append((c, n, r))
                return cube[c, n, r + 1]

            from objcavit_amd.modules.ObjCAViT import PaddedObjects
            prov = TableObjectProvider(lambda img: (self.xywh, self.cls), phrase_features=phrase, dim=F)
            feats, boxes, _ = prov(torch.zeros(self.n, 1, 1, 1, device="cuda"))
            self._host[key] = (PaddedObjects.from_lists(feats, boxes, torch.device("cuda"), capacity=16), sorted(set(asked)))
        return self._host[key]

    def table(self, F, half, drop=()):
        cube, (_, asked) = self.cube(F, half), self.host(F, half)
        return PhraseTable(NCLS, dim=F, dtype=torch.float16 if half else torch.float32, device="cuda",
                           mapping={k: cube[k[0], k[1], k[2] + 1] for k in asked if k not in set(drop)})


@pytest.fixture(scope="module")
def golden():
    return _Golden()


def _poisoned_out(Bo, cap_out, F):
    nan = float("nan")
    return (torch.full((Bo, cap_out, F), nan, device="cuda"), torch.full((Bo, cap_out, 6), nan, device="cuda")[:, :, :4],
            torch.full((Bo,), -7, dtype=torch.int32, device="cuda"))


def _keys(keys: torch.Tensor) -> np.ndarray:
    return keys.cpu().view(torch.int64).numpy().view(np.uint64)


@pytest.mark.parametrize("F", [512, 12])
@pytest.mark.parametrize("half", [False, True])
def test_pinned_to_the_reference_and_to_the_host_path(ops, golden, F, half):
    """B = 7, cap = 13 written into buffers of capacity 16 (strided boxes, rows 13 .. 15 untouched): relations = the reference's golden,
    features / boxes / counts = TableObjectProvider -> PaddedObjects.from_lists, bit for bit, the padding rows included."""
    want, asked = golden.host(F, half)
    dets, table = golden.dets(), golden.table(F, half)
    assert dets.capacity == 13 and dets.counts.tolist() == [12, 3, 13, 2, 1, 2, 0] and len(table) == len(asked)
    out = _poisoned_out(7, 16, F)
    f, x, c, rows, keys, flags = ops.object_frontend(dets.xywh, dets.cls, dets.counts, phrases=table, out=out)
    assert f is out[0] and x is out[1] and c is out[2]
    k = _keys(keys)
    for b in range(7):
        n = len(golden.xywh[b])
        if n >= 2:
            assert ((k[b, :n] & np.uint64(7)).astype(np.int64) - 1).tolist() == golden.idx[b], b
        elif n == 1:
            assert int(k[b, 0]) == table.key(int(golden.cls[b][0]), int(golden.cls[b][0]), -1)
        assert (k[b, n:] == EMPTY).all() and (rows[b, n:] == -1).all() and (rows[b, :n] >= 0).all()
        live = max(n, 1)
        assert torch.equal(f[b, :live], want.features[b, :live]) and torch.equal(x[b, :live], want.xywh[b, :live]), b
    assert int(flags.max()) == 0
    assert torch.equal(c, want.counts) and c.tolist() == [12, 3, 13, 2, 1, 2, 1]
    assert torch.equal(f[:, :13], want.features[:, :13]) and torch.equal(x[:, :13], want.xywh[:, :13])
    assert float(f[6, 0].abs().max()) == 0.0 and x[6, 0].tolist() == [-1.0] * 4                 # no detections: the <UNK> row
    assert bool(torch.isnan(f[:, 13:]).all()) and bool(torch.isnan(x[:, 13:]).all())              # rows it does not own
    assert bool(torch.isnan(out[1]._base[:, :, 4:]).all())                                       # nor columns beyond the fourth
    assert torch.equal(torch.from_numpy(table.lookup_host(k.reshape(-1)).reshape(7, 13)).cuda(), rows)      # device probe == host model


def test_relation_steps_to_the_ulp_and_ieee_rounding_on_the_device(ops):
    """Two-object images with areas (t_k +- d ulp, 1), d = 0, 1, 2, and 64 pairs of random boxes: row 0's (and 1's) relation equals
    ``relative_size_index`` -- product and quotient are IEEE-rounded on the device."""
    bits = lambda v: int(np.array([v], np.float32).view(np.uint32)[0])                           # noqa: E731
    f32 = lambda b: float(np.array([b], np.uint32).view(np.float32)[0])                          # noqa: E731
    boxes = [torch.tensor([[1.0, 2.0, f32(bits(t) + d), 1.0], [3.0, 4.0, 1.0, 1.0]]) for t in objects.REL_SIZE_THRESHOLDS for d in (-2, -1, 0, 1, 2)]
    rs = np.random.RandomState(11)
    for _ in range(64):
        wh = np.exp(rs.uniform(-0.9, 0.9, (2, 2))) * rs.uniform(1.0, 300.0)
        boxes.append(torch.from_numpy(np.concatenate([rs.uniform(0, 100, (2, 2)), wh], 1).astype(np.float32)))
    dets = Detections.from_lists(boxes, [[1, 2]] * len(boxes), "cuda")
    empty = PhraseTable(NCLS, dim=4, device="cuda")
    _, _, _, rows, keys, flags = ops.object_frontend(dets.xywh, dets.cls, dets.counts, phrases=empty)
    got = ((_keys(keys) & np.uint64(7)).astype(np.int64) - 1).tolist()
    want = [objects.relative_size_index(b) for b in boxes]
    assert got == want
    assert [g[0] for g in got[:30]] == [k + (d >= 0) for k in range(6) for d in (-2, -1, 0, 1, 2)]
    assert len({g[0] for g in got[30:]}) >= 4                                                   # the random pairs spread over the scale
    assert bool((rows == -1).all()) and bool((flags == FLAG_MISS).all())


def _model_of_the_rules(xywh, cls, counts, cap, n_classes, table, fallback, F):
    """The header's rules restated on the host for ONE batch given as padded numpy arrays: (features, xywh, counts, rows, keys, flags)."""
    B = len(counts)
    f, x = np.zeros((B, cap, F), np.float32), np.zeros((B, cap, 4), np.float32)
    rows, keys, flags = np.full((B, cap), -1, np.int32), np.full((B, cap), EMPTY, np.uint64), np.zeros((B, cap), np.uint8)
    cnt = np.zeros(B, np.int32)
    for b in range(B):
        n = min(max(int(counts[b]), 0), cap)
        cnt[b] = max(n, 1)
        if counts[b] > cap:
            flags[b, 0] |= FLAG_COUNT_CLAMPED
        if n == 0:
            x[b, 0] = -1.0
        with np.errstate(all="ignore"):
            area = (xywh[b, :, 2] * xywh[b, :, 3]).astype(np.float32)
        for j in range(n):
            c, rel, nxt = int(cls[b, j]), -1, int(cls[b, j])
            x[b, j] = xywh[b, j, :4]
            if n >= 2:
                with np.errstate(all="ignore"):
                    ratio = float(np.float32(area[j]) / np.float32(area[(j + 1) % n]))
                if ratio > 0.0 and math.isfinite(ratio):
                    rel, nxt = objects._relation_of_ratio(ratio), int(cls[b, (j + 1) % n])
                else:
                    flags[b, j] |= FLAG_BAD_RATIO
            ok = 0 <= c < n_classes
            if ok and 0 <= nxt < n_classes:
                keys[b, j] = np.uint64(table.key(c, nxt, rel))
                rows[b, j] = table.lookup_host([keys[b, j]])[0]
            else:
                flags[b, j] |= FLAG_BAD_CLASS
            if rows[b, j] >= 0:
                f[b, j] = table._host[rows[b, j]].float().numpy()
            else:
                flags[b, j] |= FLAG_MISS
                if ok and fallback is not None:
                    f[b, j] = fallback[c].float().cpu().numpy()
    return f, x, cnt, rows, keys, flags


@pytest.mark.parametrize("with_fallback", [False, True])
def test_degenerate_rows_are_flagged_and_served_as_specified(ops, with_fallback):
    nan, inf, cap, F = float("nan"), float("inf"), 4, 8
    box = lambda w, h=2.0: [5.0, 6.0, w, h]                                                      # noqa: E731
    images = [([box(0.0), box(3.0)], [1, 2], 2),                       # zero area: ratios 0 and inf
              ([box(-2.0), box(3.0)], [1, 2], 2),                      # negative width: both ratios negative
              ([box(nan), box(3.0), box(5.0)], [1, 2, 3], 3),          # NaN: rows 0 and 2 bad, row 1 fine
              ([box(inf), box(3.0)], [1, 2], 2),                       # inf: ratios inf and 0
              ([box(1.0), box(3.0)], [-1, 2], 2),                      # class -1: its row, and the row whose NEXT it is
              ([box(1.0), box(3.0), box(2.0)], [4, NCLS, 5], 3),       # class = n_classes
              ([], [], 0),                                             # nothing found
              ([box(1.0), box(2.0), box(4.0), box(30.0)], [1, 2, 3, 4], 9),      # a count beyond the capacity
              ([], [], -3),                                            # a stray negative count
              ([box(2.0)], [7], 1), ([box(1e-30, 1e-30), box(1e30, 1e30)], [1, 2], 2)]      # a lone object; a ratio that underflows to 0
    B = len(images)
    xywh, cls = np.full((B, cap, 4), nan, np.float32), np.full((B, cap), 1 << 30, np.int32)      # rows beyond the count are poison
    for b, (bx, cl, _) in enumerate(images):
        xywh[b, :len(bx)], cls[b, :len(cl)] = np.asarray(bx, np.float32).reshape(-1, 4), cl
    counts = np.asarray([im[2] for im in images], np.int32)
    cube = gen.randn("deg", (NCLS, NCLS, 8, F), 3)
    table = PhraseTable(NCLS, dim=F, device="cuda", mapping={(c, n, r): cube[c, n, r + 1] for c in (1, 2, 3, 4, 5, 7) for n in (1, 2, 3, 4, 5, 7)
                                                             for r in range(-1, 7) if (c + n + r) % 4})
    fallback = gen.randn("fb", (NCLS, F), 4).cuda() if with_fallback else None
    want = _model_of_the_rules(xywh, cls, counts, cap, NCLS, table, fallback, F)
    got = ops.object_frontend(torch.from_numpy(xywh).cuda(), torch.from_numpy(cls).cuda(), torch.from_numpy(counts).cuda(),
                              phrases=table, fallback=fallback)
    f, x, c, rows, keys, flags = (t.cpu() for t in got)
    assert c.tolist() == want[2].tolist() == [2, 2, 3, 2, 2, 3, 1, 4, 1, 1, 2]
    assert np.array_equal(rows.numpy(), want[3]) and np.array_equal(_keys(keys), want[4]) and np.array_equal(flags.numpy(), want[5])
    assert np.array_equal(f.numpy(), want[0]) and np.array_equal(x.numpy(), want[1], equal_nan=True)
    fl = flags.numpy()
    assert fl[0, :2].tolist() == [FLAG_BAD_RATIO | (fl[0, 0] & FLAG_MISS), FLAG_BAD_RATIO | (fl[0, 1] & FLAG_MISS)]
    assert all(fl[b, j] & FLAG_BAD_RATIO for b, j in ((1, 0), (1, 1), (2, 0), (2, 2), (3, 0), (3, 1), (10, 0), (10, 1))) and not fl[2, 1] & FLAG_BAD_RATIO
    k = _keys(keys)
    for b, j in ((0, 0), (1, 1), (2, 2), (3, 0)):                                               # the rel = -1 rule: the lone-object key
        assert int(k[b, j]) == table.key(int(cls[b, j]), int(cls[b, j]), -1)
    assert fl[4, 0] == fl[4, 1] == FLAG_BAD_CLASS | FLAG_MISS and fl[5, 0] == fl[5, 1] == FLAG_BAD_CLASS | FLAG_MISS and not fl[5, 2] & FLAG_BAD_CLASS
    assert float(f[4, 0].abs().max()) == 0.0 and float(f[5, 1].abs().max()) == 0.0             # an invalid class never reaches a table
    if with_fallback:
        assert torch.equal(f[4, 1], fallback[2].cpu()) and torch.equal(f[5, 0], fallback[4].cpu())
    assert fl[7, 0] & FLAG_COUNT_CLAMPED and not (fl[:, 1:] & FLAG_COUNT_CLAMPED).any() and not (fl[:7, 0] & FLAG_COUNT_CLAMPED).any()
    for b in (6, 8):
        assert x[b, 0].tolist() == [-1.0] * 4 and float(f[b].abs().max()) == 0.0 and fl[b].tolist() == [0] * cap
    assert not torch.isnan(f).any() and torch.isnan(x).nonzero().tolist() == [[2, 0, 2]]        # the poison beyond the counts was never read


@pytest.mark.parametrize("with_fallback", [False, True])
def test_misses_are_reported_filled_and_then_hit(ops, golden, with_fallback):
    F = 12
    want, asked = golden.host(F, False)
    removed = asked[::3]
    table = golden.table(F, False, drop=removed)
    fallback = gen.randn("fb12", (NCLS, F), 6).cuda() if with_fallback else None
    prov = DeviceObjectProvider(lambda img: golden.dets(), phrases=table, fallback=fallback)
    po = prov.padded(torch.zeros(7, 1, 1, 1, device="cuda"))
    rows, keys, flags = prov.last
    k = _keys(keys)
    gone = np.isin(k, np.asarray([table.key(*t) for t in removed], np.uint64))
    assert gone.any() and np.array_equal(rows.cpu().numpy() == -1, gone | (k == EMPTY))
    assert np.array_equal((flags.cpu().numpy() & FLAG_MISS) != 0, gone)
    cls = golden.dets().cls.long()
    fill = fallback[cls] if with_fallback else torch.zeros(7, 13, F, device="cuda")
    gone_t = torch.from_numpy(gone).cuda()
    assert torch.equal(po.features[gone_t], fill[gone_t]) and torch.equal(po.features[~gone_t], want.features[:, :13][~gone_t])
    assert prov.misses() == sorted(removed) == prov.misses(rows, keys)
    cube = golden.cube(F, False)
    table.add({t: cube[t[0], t[1], t[2] + 1] for t in prov.misses()})
    po = prov.padded(torch.zeros(7, 1, 1, 1, device="cuda"))
    assert prov.misses() == [] and int(prov.last[2].max()) == 0
    assert torch.equal(po.features, want.features[:, :13]) and torch.equal(po.xywh, want.xywh[:, :13]) and torch.equal(po.counts, want.counts)


@pytest.mark.parametrize("half", [False, True])
def test_dense_class_table_equals_index_select(ops, golden, half):
    F = 512
    table = gen.randn("dense", (NCLS, F), 8).cuda()
    table = table.half() if half else table
    dets = golden.dets(capacity=16)
    f, x, c, rows, keys, flags = ops.object_frontend(dets.xywh, dets.cls, dets.counts, class_table=table)
    live = torch.arange(16, device="cuda")[None, :] < dets.counts[:, None]
    want = table.float().index_select(0, dets.cls.long().flatten()).view(7, 16, F) * live[:, :, None]
    want_x = dets.xywh * live[:, :, None]
    want_x[6, 0] = -1.0
    assert torch.equal(f, want) and torch.equal(x, want_x)
    assert torch.equal(rows, torch.where(live, dets.cls, torch.full_like(dets.cls, -1))) and int(flags.max()) == 0
    assert c.tolist() == [12, 3, 13, 2, 1, 2, 1]
    k = _keys(keys)
    assert (((k & np.uint64(7)) == 0) | (k == EMPTY)).all()                                      # no relation in this mode
    bad = dets.cls.clone()
    bad[0, 0], bad[1, 2] = NCLS, -1
    f2, _, _, rows2, _, flags2 = ops.object_frontend(dets.xywh, bad, dets.counts, class_table=table)
    assert flags2[0, 0].item() == flags2[1, 2].item() == FLAG_BAD_CLASS | FLAG_MISS and int(flags2.sum()) == 2 * (FLAG_BAD_CLASS | FLAG_MISS)
    assert rows2[0, 0].item() == rows2[1, 2].item() == -1 and float(f2[0, 0].abs().max()) == float(f2[1, 2].abs().max()) == 0.0
    assert torch.equal(f2[2:], want[2:])


def test_mirror_width_appends_the_mirrored_half(ops, golden):
    F, W = 12, 640.0
    table, dets = golden.table(F, False), golden.dets()
    one = ops.object_frontend(dets.xywh, dets.cls, dets.counts, phrases=table)
    a = ops.object_frontend(dets.xywh, dets.cls, dets.counts, phrases=table, mirror_width=W)
    b = ops.object_frontend(dets.xywh, dets.cls, dets.counts, phrases=table, mirror_width=W)
    assert all(torch.equal(p.view(torch.int64) if p.dtype == torch.uint64 else p, q.view(torch.int64) if q.dtype == torch.uint64 else q)
               for p, q in zip(a, b))                                                           # two calls are bit-equal
    f, x, c, rows, keys, flags = a
    assert tuple(f.shape) == (14, 13, F) and tuple(x.shape) == (14, 13, 4) and tuple(rows.shape) == (14, 13)
    for t, t1 in zip((f, x, c, rows, flags), (one[0], one[1], one[2], one[3], one[5])):
        assert torch.equal(t[:7], t1)
    assert torch.equal(f[7:], f[:7]) and torch.equal(c[7:], c[:7]) and torch.equal(rows[7:], rows[:7])
    assert np.array_equal(_keys(keys)[7:], _keys(keys)[:7])
    live = (torch.arange(13, device="cuda")[None, :] < dets.counts[:, None])
    want = x[:7].clone()
    want[:, :, 0] = torch.where(live, W - x[:7, :, 0], x[:7, :, 0])                              # <UNK> and padding rows are not boxes
    assert torch.equal(x[7:], want) and x[13, 0].tolist() == [-1.0] * 4


# ---------------------------------------------------------------------------
# under a captured graph
# ---------------------------------------------------------------------------
GH, GW, SEED = 352, 384, 91


def _sync_debug_mode(mode: str) -> None:
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # "a prototype feature": torch says so on every call
        torch.cuda.set_sync_debug_mode(mode)


def _sync_error_mode_works() -> bool:
    """Whether torch's sync debug mode raises on a host read on this build."""
    t = torch.ones(1, device="cuda")
    _sync_debug_mode("error")
    try:
        t.item()
        return False
    except RuntimeError:
        return True
    finally:
        _sync_debug_mode("default")


class _no_host_wait:
    """``with`` block in which a host read of the device raises (where this build of torch can tell; ``on`` says whether)."""

    def __enter__(self):
        self.on = _sync_error_mode_works()
        if self.on:
            _sync_debug_mode("error")
        return self

    def __exit__(self, *exc):
        _sync_debug_mode("default")


@pytest.fixture(scope="module")
def graph_model():
    from test_hip_objects import _model
    table = gen.randn("table", (40, 512), SEED, 10.0 / np.sqrt(512)).cuda()
    m, sd, args = _model(dict(strategy="learned"), GH, GW, SEED)
    return m, args, table


def test_detections_under_a_captured_graph_equal_the_table_provider(graph_model):
    """The model and shapes of test_table_object_provider_under_a_captured_graph: a replay fed a ``Detections`` (one launch into the
    static buffers) equals the replay fed by ``TableObjectProvider`` through lists, pad and copy -- the live rows are the same, the
    stale ones (left by the replay before) are ignored."""
    from objcavit_amd.graph import GraphedGraphBins
    m, _, table = graph_model
    H, W, seed = GH, GW, SEED
    state = {"k": 0}
    sets = [([gen.boxes("b0", 5, seed, H, W), None, gen.boxes("b2", 1, seed, H, W)], [torch.tensor([3, 17, 17, 39, 0]), None, torch.tensor([8])]),
            ([None, gen.boxes("c1", 12, seed, H, W), gen.boxes("c2", 2, seed, H, W)], [None, torch.arange(12), torch.tensor([1, 2])])]

    def detector(image):
        xy, cl = sets[state["k"]]
        return [None if b is None else b.to(image.device) for b in xy], cl

    host = TableObjectProvider(detector, class_table=table)
    dev = DeviceObjectProvider(None, class_table=table)
    original, m.object_provider = m.object_provider, host
    img = gen.randn("img", (3, 3, H, W), seed).cuda()
    g = GraphedGraphBins(m, img, object_capacity=16)
    try:
        for k, other in ((0, 1), (1, 0)):
            dets = Detections.from_lists(*sets[k], "cuda", capacity=12 + k)
            state["k"] = other
            g(img)                                                # the OTHER set first: its rows are what is stale afterwards
            m.object_provider = dev
            with _no_host_wait():
                r = g(img, dets)
            d_dev, e_dev = r.depth_pred.clone(), r.bin_edges.clone()
            counts_dev = g.objects.counts.clone()
            m.object_provider = host
            state["k"] = k
            r = g(img)
            assert torch.equal(counts_dev, g.objects.counts) and torch.equal(d_dev, r.depth_pred) and torch.equal(e_dev, r.bin_edges), k
        with pytest.raises(TypeError, match="DeviceObjectProvider"):
            g(img, dets)                                          # a Detections with any other provider
        m.object_provider = dev
        with pytest.raises(ValueError):
            g(img, Detections.from_lists(*sets[0], "cuda", capacity=17))
        with pytest.raises(ValueError):
            g(img, Detections.from_lists(sets[0][0][:2], sets[0][1][:2], "cuda"))
    finally:
        m.object_provider = original


def test_pipelined_predictor_takes_detections_without_a_host_wait(graph_model):
    """One bs-1 step of a two-slot ``PipelinedPredictor`` with flip-TTA whose ``submit`` is given a ``Detections`` (mirrored half by
    ``mirror_width``) equals a ``Predictor`` on a captured graph of the same shape that asks the provider for the same objects."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args, table = graph_model
    frame = torch.randint(0, 256, (1, GH, GW, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    dets = Detections.from_lists([gen.boxes("p0", 9, SEED, GH, GW)], [torch.arange(9) * 4], "cuda", capacity=16)
    original, m.object_provider = m.object_provider, DeviceObjectProvider(lambda image: dets, class_table=table, mirror_width=GW)
    try:
        pp = PipelinedPredictor(m, args, frame, slots=2, object_capacity=16, want=("depth",))
        both = pp.graphs[0].static_image.clone()
        with _no_host_wait() as guard:
            pp.submit(frame, object_features=dets)
        got = pp.collect()[0].depth.clone()
        assert pp.rerun_steps == 0
        st = pp.graphs[0].objects
        assert st.counts.tolist() == [9, 9] and torch.equal(st.features[1, :9], st.features[0, :9])
        assert torch.equal(st.xywh[1, :9, 0], GW - st.xywh[0, :9, 0]) and torch.equal(st.xywh[1, :9, 1:], st.xywh[0, :9, 1:])
        g = GraphedGraphBins(m, both, object_group=1, object_capacity=16, in_flight=2)
        ref = Predictor(g, args)(frame, want=("depth",))
        assert torch.equal(got, ref.depth)
        print("sync debug mode was active around submit:", guard.on)
    finally:
        m.object_provider = original
