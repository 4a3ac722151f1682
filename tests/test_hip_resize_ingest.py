"""-m gpu: the resize on ingest -- csrc/frame_resize.hip against statement R (tests/resize_ref.py, float64) at the derived bar
(k_h + k_w + 4) 2^-24 max|table|, its guarded run (tests/mem_guard.py), and ``Predictor`` / ``PipelinedPredictor`` with ``resize``
against the same steps issued by hand."""
import pytest
import torch

import gen
import mem_guard
import resize_ref
from objcavit_amd.config import make_args

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
B = 2

# name -> (Hs, Ws, top, left, Hw, Ww, H, W)
CASES = {
    "offset window, 16-byte stores": (37, 53, 3, 5, 31, 45, 16, 24),
    "odd W, scalar stores": (31, 45, 0, 0, 31, 45, 15, 23),
    "enlarge": (9, 7, 0, 0, 9, 7, 16, 12),
    "down in y, up in x": (40, 10, 0, 0, 40, 10, 16, 24),
    "ratio just above 1": (33, 41, 0, 0, 33, 41, 32, 40),
    "ratio 8": (128, 96, 0, 0, 128, 96, 16, 12),
    "ratio 6": (96, 72, 0, 0, 96, 72, 16, 12),
    "tile edges 8 x 64": (63, 154, 1, 3, 61, 150, 20, 72),
    "tile edges, every tile shape": (61, 150, 0, 0, 61, 150, 21, 72),        # 21 rows: no multiple of 8 or 4; 72 columns: none of 64, 32, 16
}
_MADE = {}


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def _table():
    if "table" not in _MADE:
        from objcavit_amd.predict import normalisation_table
        _MADE["table"] = normalisation_table(make_args())
    return _MADE["table"]


def _frames(seed, Hs, Ws, top, left, Hw, Ww):
    """uint8 [B, Hs, Ws, 3] holding every byte value, with 0 and 255 at the window's four corners and at the middle of its four edges."""
    n = B * Hs * Ws * 3
    g = torch.Generator().manual_seed(seed)
    f = (torch.arange(n) % 256)[torch.randperm(n, generator=g)].to(torch.uint8).view(B, Hs, Ws, 3)
    y0, y1, x0, x1, ym, xm = top, top + Hw - 1, left, left + Ww - 1, top + Hw // 2, left + Ww // 2
    special = {(y0, x0): 0, (y0, x1): 255, (y1, x0): 255, (y1, x1): 0, (y0, xm): 255, (y1, xm): 0, (ym, x0): 0, (ym, x1): 255}
    keep = torch.ones(B, Hs, Ws, 3, dtype=torch.bool)
    for (y, x) in special:
        keep[:, y, x] = False
    free = int(keep.sum())
    assert free >= 256
    f[keep] = (torch.arange(free) % 256)[torch.randperm(free, generator=g)].to(torch.uint8)
    for (y, x), v in special.items():
        f[:, y, x] = v
    assert torch.unique(f).numel() == 256
    return f


def _case(name):
    """(frames, reference [2 B, 3, H, W] float64 with the mirrored half, bar): made once, shared, never changed."""
    if name not in _MADE:
        Hs, Ws, top, left, Hw, Ww, H, W = CASES[name]
        f = _frames(100 + list(CASES).index(name), Hs, Ws, top, left, Hw, Ww)
        _MADE[name] = (f, resize_ref.resized_input(f, _table(), top, left, Hw, Ww, H, W, mirror=True),
                       resize_ref.bar(Hw, Ww, H, W, _table()))
    return _MADE[name]


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_is_statement_r_at_the_derived_bar(ops, name, mirror):
    Hs, Ws, top, left, Hw, Ww, H, W = CASES[name]
    f, ref, bar = _case(name)
    table = _table().cuda()
    if not ops.frame_resize_supported(Hw, Ww, H, W):
        assert name == "ratio 8"                                                 # beyond the kernel's limit: refused, the limit named
        with pytest.raises(ValueError, match=str(ops.FRAME_RESIZE_MAX_RATIO)):
            ops.frame_resize_ingest(f.cuda(), table, (H, W), top, left, (Hw, Ww), mirror_too=mirror)
        return
    got = ops.frame_resize_ingest(f.cuda(), table, (H, W), top, left, (Hw, Ww), mirror_too=mirror)
    assert tuple(got.shape) == ((2 * B if mirror else B), 3, H, W) and got.dtype == torch.float32
    diff = float((got.cpu().double() - ref[:got.shape[0]]).abs().max())
    print(f"{name}, mirror {mirror}: {Hw} x {Ww} -> {H} x {W}: {diff:.3g} against R, bar {bar:.3g} ({diff / bar:.2f} of it)")
    assert diff <= bar
    if mirror:
        assert torch.equal(got[B:], got[:B].flip(3))                             # the same values, stored twice
    assert torch.equal(ops.frame_resize_ingest(f.cuda(), table, (H, W), top, left, (Hw, Ww), mirror_too=mirror), got)


@pytest.mark.parametrize("H,W", [(36, 48), (35, 47)])
def test_identity_window_is_frame_ingest_bit_for_bit(ops, H, W):
    f = _frames(7, 40, 56, 2, 3, H, W).cuda()
    table = _table().cuda()
    want = ops.frame_ingest(f, table, 2, 3, (H, W), mirror_too=True)
    got = ops.frame_resize_ingest(f, table, (H, W), 2, 3, (H, W), mirror_too=True)
    assert torch.equal(got, want)
    assert torch.equal(ops.frame_resize_ingest(f, table, (40, 56)), ops.frame_ingest(f, table))          # window = the rest of the frame


def test_strided_input_out_argument_and_refusals(ops):
    table = _table().cuda()
    big = _frames(12, 50, 70, 5, 8, 31, 45)
    view = big.cuda()[:, 3:43, 5:61]                                             # [2, 40, 56, 3]: rows and frames strided, origin at an odd byte
    assert not view.is_contiguous() and view.data_ptr() % 2 == 1
    dense = big[:, 3:43, 5:61].contiguous().cuda()
    got = ops.frame_resize_ingest(view, table, (16, 24), 2, 3, (31, 45), mirror_too=True)
    assert torch.equal(got, ops.frame_resize_ingest(dense, table, (16, 24), 2, 3, (31, 45), mirror_too=True))
    ref = resize_ref.resized_input(big[:, 3:43, 5:61], _table(), 2, 3, 31, 45, 16, 24, mirror=True)
    assert float((got.cpu().double() - ref).abs().max()) <= resize_ref.bar(31, 45, 16, 24, _table())
    # out= / out_index: one batch filled by one launch per frame; the other images' bytes stay what they were
    out = torch.full((6, 3, 16, 24), float("nan"), device="cuda")
    for i in range(2):
        assert ops.frame_resize_ingest(view[i:i + 1], table, (16, 24), 2, 3, (31, 45), mirror_too=True, out=out, out_index=i + 1) is out
        if i == 0:
            assert torch.equal(out[1], got[0]) and torch.equal(out[4], got[2])
            assert bool(torch.isnan(out[[0, 2, 3, 5]]).all())
    assert torch.equal(out[1:3], got[:2]) and torch.equal(out[4:6], got[2:]) and bool(torch.isnan(out[[0, 3]]).all())
    with pytest.raises(ValueError):
        ops.frame_resize_ingest(view, table, (16, 24), 2, 3, (31, 45), mirror_too=True, out=out, out_index=2)       # 2 images at 2 of 3
    with pytest.raises(ValueError):
        ops.frame_resize_ingest(view, table, (16, 24), 2, 3, (31, 45), out=torch.empty(2, 3, 16, 25, device="cuda"))
    with pytest.raises(ValueError):
        ops.frame_resize_ingest(view, table, (16, 24), 10, 3, (31, 45))                                            # 10 + 31 > 40 rows
    with pytest.raises(ValueError):
        ops.frame_resize_ingest(view, table, (16, 24), 2, 3, (31, 45), taps=ops.frame_resize_taps("cuda", 31, 45, 16, 20))
    R = ops.FRAME_RESIZE_MAX_RATIO
    with pytest.raises(ValueError, match=str(R)):
        ops.frame_resize_ingest(torch.zeros(1, 4 * R + 1, 8, 3, dtype=torch.uint8, device="cuda"), table, (4, 8))


@pytest.mark.parametrize("name", ["odd W, scalar stores", "ratio 6"])
def test_guarded_run_writes_every_output_word_and_nothing_else(name):
    """The new entry point between poisoned guards (it has no row in tests/test_hip_memory_bounds.py: its name does not end in _fwd)."""
    Hs, Ws, top, left, Hw, Ww, H, W = CASES[name]
    f, ref, bar = _case(name)
    from objcavit_amd import hip_ops
    host_taps = hip_ops.resize_taps(Hw, H) + hip_ops.resize_taps(Ww, W)
    try:
        with mem_guard.guarded("cuda") as g:
            g.record_calls()
            taps = tuple(g.copy(t) for t in host_taps)
            got = hip_ops.frame_resize_ingest(g.copy(f), g.copy(_table()), (H, W), top, left, (Hw, Ww), mirror_too=True, taps=taps)
            torch.cuda.synchronize()
            g.check()
            assert "ocv_frame_resize_ingest" in g.calls
            assert g.never_written(got) == 0
            assert not g.stray, g.stray
            assert float((got.cpu().double() - ref).abs().max()) <= bar
    except RuntimeError as e:                      # a device fault ends the session: nothing more is launched on a faulted GPU
        if "HIP error" in str(e) or "illegal memory" in str(e) or "hipError" in str(e):
            pytest.exit(f"GPU fault in the guarded run of {name}: {e}", returncode=3)
        raise


# ---------------------------------------------------------------------------
# predict path: a 192 x 208 model (the smallest end-to-end size the suite runs), frames of 250 x 300
# ---------------------------------------------------------------------------
MH, MW = 192, 208


def _model():
    if "model" not in _MADE:
        from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
        args = make_args(model="graphbins", dataset="nyu", strategy="learned", language="clip", do_final_upscale=True,
                         dimensions_train=[MH, MW], dimensions_test=[MH, MW])
        m = GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5)).eval()
        gen.load_into(m, 23, gen.PEAKY)
        _MADE["model"] = (m.cuda(), args)
    return _MADE["model"]


def _rand_frames(seed, n, Hs, Ws):
    return torch.randint(0, 256, (n, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _gt(n, H, W, seed, dmax=10.0):
    return torch.rand(n, 1, H, W, generator=torch.Generator().manual_seed(seed)) * 0.9 * dmax + 0.05 * dmax


def _by_hand(ops, m, args, both, size, gt, first_image_id):
    """The steps of a predict call, issued by hand on the ingested [batch | mirrored batch]."""
    from objcavit_amd.validation import _depth_range, _forward_pair, _records
    dmin, dmax = _depth_range(args)
    out, mirror = _forward_pair(m, both=both)
    pred, mpred = out.depth_pred.contiguous(), mirror.depth_pred.contiguous()
    depth = ops.depth_finalize(pred, dmin, dmax, size, pred_mirror=mpred)["depth"]
    rec = None if gt is None else _records(pred, mpred, None, gt, args, dmin, dmax, first_image_id, False)
    return depth, rec


def test_predictor_with_resize_equals_the_steps_issued_by_hand(ops):
    from objcavit_amd.predict import Predictor, fit_window, normalisation_table
    m, args = _model()
    frames = _rand_frames(21, 2, 250, 300).cuda()
    top, left, Hw, Ww = fit_window(250, 300, MH, MW)
    assert (top, left, Hw, Ww) == (0, 15, 250, 270)
    gt = _gt(2, Hw, Ww, 22).cuda()
    res = Predictor(m, args, crop=(top, left, Hw, Ww), resize=(MH, MW))(frames, gt, first_image_id=5)
    assert tuple(res.depth.shape) == (2, 1, Hw, Ww) and tuple(res.records.shape) == (2, 10)
    table = normalisation_table(args).cuda()
    both = ops.frame_resize_ingest(frames, table, (MH, MW), top, left, (Hw, Ww), mirror_too=True)
    assert tuple(both.shape) == (4, 3, MH, MW)
    depth, rec = _by_hand(ops, m, args, both, (Hw, Ww), gt, 5)
    assert torch.equal(res.depth, depth) and torch.equal(res.records, rec)
    assert bool(torch.isfinite(res.depth).all())


def test_predictor_without_resize_is_the_frame_ingest_path(ops):
    from objcavit_amd.predict import Predictor, normalisation_table
    m, args = _model()
    frames = _rand_frames(24, 2, MH, MW).cuda()
    gt = _gt(2, MH, MW, 25).cuda()
    ops.enable_timing(True)
    res = Predictor(m, args, resize=None)(frames, gt, first_image_id=3)
    counts = {k: v[0] for k, v in ops.timing_results().items()}
    ops.enable_timing(False)
    assert counts.get("frame_ingest") == 1 and "frame_resize_ingest" not in counts, counts
    both = ops.frame_ingest(frames, normalisation_table(args).cuda(), mirror_too=True)
    depth, rec = _by_hand(ops, m, args, both, (MH, MW), gt, 3)
    assert torch.equal(res.depth, depth) and torch.equal(res.records, rec)
    again = Predictor(m, args)(frames, gt, first_image_id=3)
    assert torch.equal(again.depth, res.depth) and torch.equal(again.records, res.records)


def test_pipelined_predictor_with_resize_takes_windows_of_two_sizes(ops):
    """Three bs-1 steps over two slots, the second frame of another size than the example: bit for bit the sequential ``Predictor`` on a
    captured graph of the same shape (both sides replay a GraphedGraphBins, so the dispatch is identical)."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.predict import PipelinedPredictor, Predictor, normalisation_table
    m, args = _model()
    sizes = [(250, 300), (230, 282), (250, 300)]
    frames = [_rand_frames(40 + i, 1, *s).cuda() for i, s in enumerate(sizes)]
    gts = [_gt(1, *s, 50 + i).cuda() for i, s in enumerate(sizes)]
    pp = PipelinedPredictor(m, args, frames[0], slots=2, resize=(MH, MW))
    assert len(pp.graphs) == 2 and tuple(pp.graphs[0].static_image.shape) == (2, 3, MH, MW)
    example = ops.frame_resize_ingest(frames[0], normalisation_table(args).cuda(), (MH, MW), mirror_too=True)
    seq = Predictor(GraphedGraphBins(m, example, object_group=1, in_flight=2), args, resize=(MH, MW))
    ref = []
    for i in range(3):
        r = seq(frames[i], gts[i], first_image_id=i)
        ref.append((r.depth.clone(), r.records.clone()))
    for i in range(3):
        pp.submit(frames[i], gts[i], first_image_id=i)
    got = pp.collect()
    assert len(got) == 3 and pp.rerun_steps == 0
    for i in range(3):
        assert tuple(got[i].depth.shape) == (1, 1) + sizes[i]
        assert torch.equal(got[i].depth, ref[i][0]) and torch.equal(got[i].records, ref[i][1]), i
    with pytest.raises(ValueError):
        pp.submit([frames[0][0], frames[1][0]])                                  # two frames for a one-frame capture


def test_readout_and_point_cloud_read_the_final_map_at_the_windows_size(ops):
    from objcavit_amd.object_depth import object_depths
    from objcavit_amd.point_cloud import point_cloud, shift_intrinsics
    from objcavit_amd.predict import Predictor, fit_window
    m, args = _model()
    frames = _rand_frames(61, 2, 250, 300).cuda()
    top, left, Hw, Ww = fit_window(250, 300, MH, MW)
    boxes = [torch.tensor([[135.0, 125.0, 60.0, 80.0], [260.0, 240.0, 30.0, 30.0]]).cuda(), None]          # pixels of the 250 x 270 window
    K = torch.tensor([[280.0, 285.0, 149.5, 124.5], [300.0, 300.0, 140.0, 130.0]])                         # of the 250 x 300 frames
    pr = Predictor(m, args, crop=(top, left, Hw, Ww), resize=(MH, MW), object_depth={}, point_cloud=dict(stride=(2, 3), pixel=True))
    res = pr(frames, intrinsics=K, boxes=boxes)
    assert tuple(res.depth.shape) == (2, 1, Hw, Ww)
    od = object_depths(res.depth, boxes)
    assert torch.equal(res.objects.table, od.table) and torch.equal(res.objects.counts, od.counts)
    assert float(res.objects.table[0, 0, 0]) == 60 * 80 and float(res.objects.table[0, 1, 0]) > 0          # boxes inside the window's map
    dmin, dmax = float(args.nyu.min_depth), float(args.nyu.max_depth)
    pc = point_cloud(res.depth, shift_intrinsics(K.cuda(), top, left), stride=(2, 3), near=dmin, far=dmax, frames=frames, top=top,
                     left=left, pixel=True)
    assert torch.equal(res.points.counts, pc.counts) and torch.equal(res.points.total, pc.total)
    n = int(pc.counts.min())
    assert n > 0
    for b in range(2):
        k = int(pc.counts[b])
        assert torch.equal(res.points.points[b, :k].view(torch.int32), pc.points[b, :k].view(torch.int32))
        assert torch.equal(res.points.pixel[b, :k], pc.pixel[b, :k])
