"""-m gpu: csrc/object_depth.hip against the torch statement of tests/object_depth_ref.py -- n, min, max and the quantiles EQUAL (they
are elements of the map), mean and std_mean within one fp32 ulp of the float64 reference (the kernel's float64 sum differs from the
reference's at the 1e-16 level only: the rounding to fp32 can flip at a tie, nowhere else) -- and the predict path that carries it."""
import os
import subprocess
import sys

import pytest
import torch

import gen
import object_depth_ref as ref
import predict_ref
from objcavit_amd.config import make_args

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def _check(got, want, Q, what=""):
    """got (device) against the reference table: columns 0-2 and the quantiles equal, 3-4 within one ulp; no element left unwritten."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    exact = [0, 1, 2] + list(range(5, 5 + Q))
    bad = (got[..., exact] != want[..., exact]) & ~(torch.isnan(got[..., exact]) & torch.isnan(want[..., exact]))
    assert not bad.any(), (what, bad.nonzero()[:5].tolist(), got[bad.any(-1)][:3], want[bad.any(-1)][:3])
    assert ref.within_one_ulp(got[..., 3:5], want[..., 3:5]), (what, got[..., 3:5], want[..., 3:5])


def _nan_out(B, cap, Q):
    return torch.full((B, cap, 5 + Q), float("nan"), device="cuda")


# ---------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("boxes", sorted(ref.BOX_SETS))
@pytest.mark.parametrize("kind", ref.VALUE_KINDS)
def test_records_equal_the_reference(ops, kind, boxes):
    """37 x 53 (odd, W % 4 != 0), B = 3, cap = 6, counts [6, 1, 3]; shrink 0.3 (half = 0.15: no power of two) catches a contracted
    half * w; xywh of width 4 and of width 6 as a strided view; rows at or beyond counts[b] hold a valid box and must be zero; ``out``
    is NaN before the call, so every element is shown to be written."""
    q = (0.1, 0.5, 0.9)
    depth, std = ref.case_map(kind), ref.case_map("uniform", seed=2)
    xywh4, counts = ref.case_boxes(boxes, 4)
    xywh6, _ = ref.case_boxes(boxes, 6)
    view6 = xywh6.cuda()[:, :, :4]
    assert not view6.is_contiguous()
    d_dev, s_dev, c_dev = depth.cuda(), std.cuda(), counts.cuda()
    for shrink in (1.0, 0.5, 0.3):
        want = ref.object_depth(depth, xywh4, counts, std, q, shrink)
        out = _nan_out(3, 6, 3)
        assert ops.object_depth(d_dev, xywh4.cuda(), c_dev, depth_std=s_dev, quantiles=q, shrink=shrink, out=out) is out
        assert not torch.isnan(out[..., 0]).any()
        _check(out, want, 3, (kind, boxes, shrink))
        for b, c in enumerate(counts.tolist()):
            assert not out[b, c:].any()
        wide = ops.object_depth(d_dev, xywh6.cuda(), c_dev, depth_std=s_dev, quantiles=q, shrink=shrink)
        strided = ops.object_depth(d_dev, view6, c_dev, depth_std=s_dev, quantiles=q, shrink=shrink)
        assert torch.equal(wide.view(torch.int32), out.view(torch.int32)) and torch.equal(strided.view(torch.int32), out.view(torch.int32))
    # without depth_std the column is 0 and the rest is what it was
    plain = ops.object_depth(d_dev, xywh4.cuda(), c_dev, quantiles=q, shrink=0.3)
    assert not plain[..., 4].any()
    keep = [0, 1, 2, 3, 5, 6, 7]
    assert torch.equal(plain[..., keep].view(torch.int32), out[..., keep].view(torch.int32))


def test_special_values_and_all_nan_boxes(ops):
    """The map with negative values, +-0, +-inf and NaN: a box whose pixels are all NaN is all zero, NaN pixels are not counted, the
    infinities are values (min / max of the whole map are -inf / +inf and its mean is NaN = inf - inf in both statements)."""
    depth = ref.case_map("special")
    q = (0.0, 0.5, 1.0)
    for boxes in ("inside", "small"):
        xywh, counts = ref.case_boxes(boxes)
        got = ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), quantiles=q).cpu()
        _check(got, ref.object_depth(depth, xywh, counts, None, q), 3, boxes)
        if boxes == "inside":
            assert not got[0, 1].any()                                          # the one-pixel box on a NaN pixel
            whole = got[0, 0]
            assert whole[0] == 37 * 53 - int(torch.isnan(depth[0]).sum()) and whole[1] == float("-inf") and whole[2] == float("inf")
            assert torch.isnan(whole[3])
        else:
            assert not got[0, :3].any() and got[0, 3, 0] == 4                   # n = 1, 2, 3 all NaN; the 2 x 2 box beside them


def test_lower_median_of_one_to_four_pixels(ops):
    depth = ref.case_map("uniform")
    xywh, counts = ref.case_boxes("small")
    got = ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), quantiles=(0.5,)).cpu()
    rows = {1: depth[0, 0, 11, 20:21], 2: depth[0, 0, 11, 20:22], 3: depth[0, 0, 11, 20:23], 4: depth[0, 0, 20:22, 30:32]}
    for r, (n, px) in enumerate(rows.items()):
        assert got[0, r, 0] == n and got[0, r, 5] == torch.median(px.reshape(-1)), (n, got[0, r])
        assert got[0, r, 5] == px.reshape(-1).sort().values[(n - 1) // 2]


@pytest.mark.parametrize("q", [(0.0, 1.0), (0.37,), (0.0, 0.05, 0.25, 0.5, 0.5, 0.75, 0.95, 1.0)])
def test_quantile_counts_and_the_ends_of_the_range(ops, q):
    depth, std = ref.case_map("uniform", seed=5), ref.case_map("uniform", seed=6)
    for boxes in ("inside", "borders"):
        xywh, counts = ref.case_boxes(boxes)
        out = _nan_out(3, 6, len(q))
        ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), depth_std=std.cuda(), quantiles=q, shrink=0.7, out=out)
        _check(out, ref.object_depth(depth, xywh, counts, std, q, 0.7), len(q), (q, boxes))
        if q == (0.0, 1.0):
            assert torch.equal(out[..., 5], out[..., 1]) and torch.equal(out[..., 6], out[..., 2])
    with pytest.raises(ValueError):
        ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), quantiles=(0.5,) * 9)
    with pytest.raises(ValueError):
        ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), quantiles=(1.5,))
    with pytest.raises(ValueError):
        ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), shrink=0.0)
    with pytest.raises(ValueError):
        ops.object_depth(depth.cuda(), xywh.cuda()[:, :, :3], counts.cuda())


@pytest.mark.parametrize("H,W", [(480, 640), (352, 1216)])
def test_whole_frame_and_the_widths_where_the_thread_layout_changes(ops, H, W):
    """B = 1.  The workgroup lays its 256 threads over a box as TW columns x 256 / TW rows, TW the power of two covering the width up
    to 256, eight rows per thread and step: widths 255 / 256 / 257 sit below, on and above the width from which a row takes more than
    one step; 128 / 129 change TW; at TW = 64 (four thread rows) heights 32 / 33 are one and two row steps, 4 / 5 one and two thread
    rows of a step's first; a 1-wide column and a 1-high row are the two extremes; and the whole frame (307 200 / 428 032 pixels in
    one workgroup)."""
    g = torch.Generator().manual_seed(H)
    depth = (torch.rand(1, 1, H, W, generator=g) * 9.9 + 0.1)
    depth[0, 0, 100:110, 300:320] = float("nan")
    std = torch.rand(1, 1, H, W, generator=g)
    cx, cy = W / 2.0, H / 2.0
    rows = [(cx, cy, float(W), float(H)), (cx, cy, 255.0, 9.0), (cx, cy, 256.0, 9.0), (cx, cy, 257.0, 9.0), (cx, cy, 128.0, 7.0),
            (cx, cy, 129.0, 7.0), (cx, cy, 64.0, 4.0), (cx, cy, 64.0, 5.0), (cx + 0.5, cy, 1.0, float(H)), (cx, cy + 0.5, float(W), 1.0),
            (cx, cy, 1e30, 1e30), (310.0, 105.0, 40.0, 30.0), (cx, cy, 64.0, 32.0), (cx, cy, 64.0, 33.0), (cx, cy, 256.0, 8.0), (cx, cy, 300.0, 17.0)]
    xywh = torch.tensor(rows).view(1, len(rows), 4)
    counts = torch.tensor([len(rows)], dtype=torch.int32)
    q = (0.1, 0.5, 0.9)
    got = ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), depth_std=std.cuda(), quantiles=q)
    want = ref.object_depth(depth, xywh, counts, std, q)
    assert want[0, 0, 0] == H * W - 200 and want[0, 9, 0] == W and want[0, 8, 0] == H and want[0, 6, 0] == 256 and want[0, 7, 0] == 320
    assert want[0, 12, 0] == 64 * 32 and want[0, 13, 0] == 64 * 33
    _check(got, want, 3, (H, W))
    assert torch.equal(got[0, 0].view(torch.int32), got[0, 10].view(torch.int32))              # the 1e30 box IS the whole frame


def test_two_calls_are_bit_equal(ops):
    depth, std = ref.case_map("special", seed=7), ref.case_map("uniform", seed=8)
    xywh, counts = ref.case_boxes("inside")
    a = ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), depth_std=std.cuda())
    b = ops.object_depth(depth.cuda(), xywh.cuda(), counts.cuda(), depth_std=std.cuda())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    big = torch.rand(1, 1, 480, 640, generator=torch.Generator().manual_seed(9)) * 10.0
    box = torch.tensor([[[320.0, 240.0, 640.0, 480.0], [300.0, 200.0, 333.0, 211.0]]]).cuda()
    two = torch.tensor([2], dtype=torch.int32).cuda()
    a, b = ops.object_depth(big.cuda(), box, two, depth_std=big.cuda()), ops.object_depth(big.cuda(), box, two, depth_std=big.cuda())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_captured_graph_replays_with_new_counts_boxes_and_map():
    """In a fresh child process (tests/object_depth_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "object_depth_graph_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


# ---------------------------------------------------------------------------
# the predict path
# ---------------------------------------------------------------------------
H, W = 352, 384          # the smallest shape tests/test_hip_predict.py runs a model on


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


@pytest.fixture(scope="module")
def model():
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    args = make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    m = GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5)).eval()
    gen.load_into(m, 29, gen.PEAKY)
    return m.cuda(), args


def test_predictor_reads_out_the_boxes_from_its_own_map(ops, model):
    from objcavit_amd.object_depth import OBJECT_FIELDS, ObjectDepths
    from objcavit_amd.predict import Predictor, PredictResult
    m, args = model
    B = 2
    frames = _frames(61, B).cuda()
    boxes = _boxes(62, B, 5)
    boxes[1] = None                                                             # an image without detections: the <UNK> row, n = 0
    q = (0.25, 0.5)
    on = Predictor(m, args, object_depth=dict(quantiles=q, shrink=0.8))
    res = on(frames, boxes=[None if b is None else b.cuda() for b in boxes])
    assert isinstance(res, PredictResult) and isinstance(res.objects, ObjectDepths) and res.depth_std is None
    assert res.objects.fields == OBJECT_FIELDS + ("q0.25", "q0.5") and res.objects.counts.tolist() == [boxes[0].shape[0], 1]
    cap = boxes[0].shape[0]
    xywh = torch.zeros(B, cap, 4)
    xywh[0], xywh[1, 0] = boxes[0], -1.0
    want = ref.object_depth(res.depth.cpu(), xywh, res.objects.counts.cpu(), None, q, 0.8)
    _check(res.objects.table, want, 2)
    assert res.objects.table[0, :, 0].sum() > 0 and not res.objects.table[1].any() and not res.objects.table[..., 4].any()
    # with the uncertainty: std_mean from the same call's depth_std; default options
    both = Predictor(m, args, object_depth={})(frames, want=("depth", "depth_std"), boxes=(xywh.cuda(), res.objects.counts))
    want = ref.object_depth(both.depth.cpu(), xywh, res.objects.counts.cpu(), both.depth_std.cpu(), (0.1, 0.5, 0.9), 1.0)
    _check(both.objects.table, want, 3)
    assert both.objects.table[0, :, 4].sum() > 0 and both.objects.fields[5:] == ("q0.1", "q0.5", "q0.9")
    # the map is made for the readout even when it is not wanted -- and then not handed out
    u16 = on(frames, want=("depth_u16",), boxes=(xywh.cuda(), res.objects.counts))
    assert u16.depth is None and torch.equal(u16.objects.table.view(torch.int32), res.objects.table.view(torch.int32))
    assert torch.equal(u16.depth_u16.cpu().to(torch.int32), predict_ref.to_u16(res.depth[:, 0], 1000.0))


def test_without_the_keyword_or_without_boxes_the_result_is_what_it_was(ops, model):
    from objcavit_amd.predict import Predictor, PredictResult
    m, args = model
    frames = _frames(63, 2).cuda()
    boxes = [b.cuda() for b in _boxes(64, 2, 4)]
    want = ("depth", "depth_u16", "depth_std", "confidence")
    base = Predictor(m, args)(frames, want=want)
    assert type(base) is PredictResult and base.objects is None
    for res in (Predictor(m, args, object_depth={})(frames, want=want), Predictor(m, args)(frames, want=want, boxes=boxes),
                Predictor(m, args, object_depth={})(frames, want=want, boxes=boxes)):
        for k in PredictResult._fields:
            a, b = getattr(res, k), getattr(base, k)
            assert (a is None and b is None) or torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
    assert res.objects is not None


def test_pipelined_predictor_tables_equal_the_sequential_predictors(ops, model):
    """Six bs-1 steps with different boxes over four slots: every step's table is bit-equal to the sequential ``Predictor``'s (both
    sides replay a captured graph of the same shape, as in tests/test_hip_predict.py), in submission order."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args = model
    N = 6
    frames = [_frames(70 + i, 1).cuda() for i in range(N)]
    boxes = [[b.cuda() for b in _boxes(80 + i, 1, 7)] for i in range(N)]
    boxes[2] = [None]
    opts = dict(quantiles=(0.1, 0.5, 0.9), shrink=0.9)
    want = ("depth", "depth_std")
    pp = PipelinedPredictor(m, args, frames[0], want=want, object_depth=opts)
    example = predict_ref.frames_to_input(frames[0].cpu(), args, 0, 0, H, W)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_group=1, in_flight=4)
    seq = Predictor(g, args, object_depth=opts)
    refs = []
    for i in range(N):
        r = seq(frames[i], want=want, boxes=boxes[i])
        refs.append((r.depth.clone(), r.objects.table.clone(), r.objects.counts.clone()))
    for i in range(N):
        pp.submit(frames[i], boxes=boxes[i] if i % 2 else list(boxes[i]))
    pp.submit(frames[0])                                                        # a step without boxes in the same pipeline
    got = pp.collect()
    assert len(got) == N + 1 and pp.rerun_steps == 0 and got[N].objects is None
    for i in range(N):
        assert torch.equal(got[i].depth.view(torch.int32), refs[i][0].view(torch.int32)), i
        assert got[i].objects.table.shape == refs[i][1].shape and torch.equal(got[i].objects.counts, refs[i][2])
        assert torch.equal(got[i].objects.table.view(torch.int32), refs[i][1].view(torch.int32)), i
        assert got[i].bin_edges is None                                         # _finish's _replace kept the readout
    assert not got[2].objects.table.any() and got[0].objects.table[0, :, 0].sum() > 0
