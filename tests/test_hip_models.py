"""-m gpu: the drop-in modules (HIP path, through the C ABI) against
(1) the committed golden vectors produced by the reference's own modules and
(2) the CPU oracle on the same seeded weights/inputs, plus size-independent
properties at the BASELINE.json sizes.  Depth tolerance: the north-star bar is
1e-3 relative on the depth map; the fp32 path is held to 1e-4 here."""
import numpy as np
import pytest
import torch

import gen
from oracle import restate
from objcavit_amd.config import make_args
from util import gains_of, golden_sample_dev, load_golden, max_rel, rel_dev, state_dict_from

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOK_TOL = 1e-4       # token-level intermediates after 8+ transformer layers
DEPTH_TOL = 1e-4


def _load(module, meta, key="shapes"):
    module.load_state_dict(state_dict_from(meta[key], meta["seed"], gains_of(meta)), strict=True)
    return module.eval().cuda()


@pytest.mark.parametrize("tag", ["mini", "nyu"])
def test_g1_mvit_vs_reference_golden(tag):
    from objcavit_amd.modules.miniViT import mViT
    meta, z = load_golden(f"g1_mvit_{tag}")
    m = _load(mViT(128, n_query_channels=128, patch_size=16, dim_out=256, embedding_dim=128, norm="linear", max_seq_len=500), meta)
    x = gen.randn("x", (meta["B"], 128, meta["fh"], meta["fw"]), meta["seed"]).cuda()
    y, ram = m(x)
    tgt = m.patch_transformer(x)
    assert tuple(tgt.shape) == z["tgt"].shape                       # S x B x E like the reference
    assert rel_dev(tgt, z["tgt"]) < TOK_TOL
    assert rel_dev(y, z["y"]) < TOK_TOL
    assert rel_dev(ram.flatten(2)[:, :, torch.from_numpy(z["pix"]).cuda()], z["ram_px"]) < TOK_TOL


@pytest.mark.parametrize("tag", ["16_5", "1_1", "100_3", "16_5_nosa", "8_8_8"])
def test_g2_saca_vs_reference_golden(tag):
    from objcavit_amd.modules.ObjCAViT import SelfAttnCrossAttn
    meta, z = load_golden(f"g2_saca_{tag}")
    m = _load(SelfAttnCrossAttn(make_args(no_obj_sa=meta["no_obj_sa"]), 128, 4, dim_feedforward=1024), meta)
    S, E = meta["S"], 128
    tok = gen.randn("tok", (len(meta["counts"]), S, E), meta["seed"]).cuda()
    objs = [gen.randn(f"obj{i}", (n, E), meta["seed"]).cuda() for i, n in enumerate(meta["counts"])]
    fi, fo = m(tok, objs)
    assert rel_dev(fi, z["final_img"]) < TOK_TOL
    assert rel_dev(fo, z["final_obj"]) < TOK_TOL


def _objcavit_inputs(meta):
    fh, fw, seed = meta["fh"], meta["fw"], meta["seed"]
    x = gen.randn("x", (len(meta["counts"]), 128, fh, fw), seed)
    feats, xywh = [], []
    for i, n in enumerate(meta["counts"]):
        k = 1 if n is None else n
        feats.append(gen.randn(f"f{i}", (k, 512), seed, 10.0 / np.sqrt(512)))
        xywh.append(None if n is None else gen.boxes(f"b{i}", n, seed, 2 * fh, 2 * fw))
    return x, feats, xywh


@pytest.mark.parametrize("tag", ["learned", "learned_nosa", "bbox_wh_2saca", "learned_2saca_eq", "grid_random",
                                 "learned_many", "bbox_wh_2saca_many"])
def test_g3_objcavit_vs_reference_golden(tag):
    from objcavit_amd.modules.ObjCAViT import ObjCAViT
    meta, z = load_golden(f"g3_objcavit_{tag}")
    H, W = 2 * meta["fh"], 2 * meta["fw"]
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], **meta["kw"])
    m = _load(ObjCAViT(args, n_query_channels=128, patch_size=16, im_feature_dim=128, obj_feature_dim=512,
                       embedding_dim=128, dim_out=256, norm="linear", max_seq_len=500), meta)
    x, feats, xywh = _objcavit_inputs(meta)
    cap = {}
    h = m.saca_1.register_forward_hook(lambda mod, inp, out: cap.__setitem__("img", out[0]))
    y, ram = m(x.cuda(), [f.cuda() for f in feats], [None if b is None else b.cuda() for b in xywh])
    h.remove()
    assert rel_dev(cap["img"], z["saca1_img"]) < TOK_TOL
    assert rel_dev(y, z["y"]) < TOK_TOL
    assert rel_dev(ram.flatten(2)[:, :, torch.from_numpy(z["pix"]).cuda()], z["ram_px"]) < TOK_TOL


@pytest.mark.parametrize("tag", ["mini", "nyu"])
def test_g5_adabins_depth_vs_reference_golden(tag):
    """BASELINE configs[0] on the GPU path vs the reference's CPU forward."""
    from objcavit_amd.modules.AdaBins import AdaBins
    meta, z = load_golden(f"g5_adabins_{tag}")
    m = _load(AdaBins(make_args(model="adabins")), meta)
    img = gen.randn("img", (1, 3, meta["H"], meta["W"]), meta["seed"]).cuda()
    out = m(img)
    assert out._fields == ("depth_pred", "bin_edges")
    assert tuple(out.depth_pred.shape) == (1, 1, meta["H"] // 2, meta["W"] // 2)
    got = out.depth_pred.flatten()[torch.from_numpy(z["pix"]).cuda()]
    # fp32 MIOpen convolutions (encoder + decoder, ~340 GFLOP) vs CPU oneDNN: 1e-3 is the north-star bar
    assert max_rel(got, z["depth_px"]) < 1e-3
    assert rel_dev(out.bin_edges, z["bin_edges"]) < 1e-4


def test_g5_adabins_final_upscale_vs_reference_golden():
    """do_final_upscale end to end on the GPU path vs the reference's own AdaBins(do_final_upscale=True) CPU forward:
    fifth decoder stage against the image, feature map / patch embedding / bin head at full resolution, 1200-row table."""
    from objcavit_amd.modules.AdaBins import AdaBins
    meta, z = load_golden("g5_adabins_mini_upscale")
    H, W = meta["H"], meta["W"]
    m = _load(AdaBins(make_args(model="adabins", do_final_upscale=True, dimensions_train=[H, W], dimensions_test=[H, W])), meta)
    out = m(gen.randn("img", (1, 3, H, W), meta["seed"]).cuda())
    assert tuple(out.depth_pred.shape) == (1, 1, H, W)
    got = out.depth_pred.flatten()[torch.from_numpy(z["pix"]).cuda()]
    assert max_rel(got, z["depth_px"]) < 1e-3
    assert rel_dev(out.bin_edges, z["bin_edges"]) < 1e-4


@pytest.mark.parametrize("model,H,W,B", [("adabins", 480, 640, 1), ("graphbins", 192, 208, 2), ("graphbins", 480, 640, 1)])
def test_final_upscale_models_end_to_end_vs_oracle(model, H, W, B):
    """GraphBins / AdaBins with do_final_upscale=True against the oracle (restate.*_forward(do_final_upscale=True), pinned
    by g5_adabins_mini_upscale).  480 x 640: S = 1200 tokens -- the longest sequence the reference allows
    (modules/AdaBins.py:43, GraphBins.py:45) -- through the patch embedding, both attention kernels and the bin head on a
    307 200-pixel map."""
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.GraphBins import GraphBins
    seed = 64
    args = make_args(model=model, do_final_upscale=True, language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    m = (AdaBins(args) if model == "adabins" else GraphBins(args)).eval()
    sd = gen.load_into(m, seed, gen.PEAKY)
    m = m.cuda()
    img = gen.randn("img", (B, 3, H, W), seed)
    if model == "adabins":
        out = m(img.cuda())
        ref_depth, ref_edges = restate.adabins_forward(img, sd, 0.001, 10, do_final_upscale=True)
    else:
        feats = [gen.randn(f"f{i}", (9 + i, 512), seed, 10.0 / np.sqrt(512)) for i in range(B)]
        xywh = [gen.boxes(f"b{i}", 9 + i, seed, H, W) for i in range(B)]
        out = m(img.cuda(), [f.cuda() for f in feats], [b.cuda() for b in xywh])
        ref_depth, ref_edges = restate.graphbins_forward(img, feats, xywh, sd, 0.001, 10, do_final_upscale=True, strategy="learned")
    assert tuple(out.depth_pred.shape) == tuple(ref_depth.shape) == (B, 1, H, W)
    assert rel_dev(out.bin_edges, ref_edges) < 1e-4
    assert max_rel(out.depth_pred, ref_depth) < 1e-3
    assert float(ref_depth.max() - ref_depth.min()) > 0.1


def _graphbins_pair(args_kw, B, H, W, n_obj, seed, lang="clip"):
    from objcavit_amd.modules.GraphBins import GraphBins
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language=lang, **args_kw)
    m = GraphBins(args).eval()
    sd = gen.load_into(m, seed, gen.PEAKY)
    img = gen.randn("img", (B, 3, H, W), seed)
    feats = [gen.randn(f"f{i}", (n_obj, 512), seed, 10.0 / np.sqrt(512)) for i in range(B)]
    xywh = [gen.boxes(f"b{i}", n_obj, seed, H, W) for i in range(B)]
    return m.cuda(), sd, img, feats, xywh, args


@pytest.mark.parametrize("kw,n_obj", [(dict(strategy="learned"), 16), (dict(strategy="learned_bbox_wh", use_2_saca=True), 90),
                                      (dict(strategy="grid_random"), 8), (dict(strategy="grid_random_roi_align"), 5)])
def test_graphbins_end_to_end_vs_oracle(kw, n_obj):
    """Boundary A: GraphBins.forward (HIP) vs oracle graphbins_forward (CPU) on a mini image, identical weights."""
    H, W = 352, 384
    m, sd, img, feats, xywh, args = _graphbins_pair(kw, 2, H, W, n_obj, 77)
    out = m(img.cuda(), [f.cuda() for f in feats], [b.cuda() for b in xywh])
    ref_depth, ref_edges = restate.graphbins_forward(img, feats, xywh, sd, 0.001, 10, **kw)
    assert out._fields == ("depth_pred", "bin_edges", "detections")
    assert rel_dev(out.bin_edges, ref_edges) < 1e-4
    assert max_rel(out.depth_pred, ref_depth) < 1e-3          # north-star tolerance
    assert float(ref_depth.max() - ref_depth.min()) > 0.1


def test_graphbins_with_table_object_provider():
    """Row N4: ragged detections (incl. an image without any) served from a class table, end to end vs the oracle."""
    from objcavit_amd.modules.GraphBins import GraphBins
    from objcavit_amd.objects import TableObjectProvider
    H, W, seed = 352, 384, 91
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language="clip")
    table = gen.randn("table", (40, 512), seed, 10.0 / np.sqrt(512))
    cls = [torch.tensor([3, 17, 17, 39, 0]), None, torch.tensor([8])]
    xywh = [gen.boxes("b0", 5, seed, H, W), None, gen.boxes("b2", 1, seed, H, W)]
    prov = TableObjectProvider(lambda image: ([None if b is None else b.to(image.device) for b in xywh], cls), class_table=table.cuda())
    m = GraphBins(args, object_provider=prov).eval()
    sd = gen.load_into(m, seed, gen.PEAKY)
    img = gen.randn("img", (3, 3, H, W), seed)
    out = m.cuda()(img.cuda())
    feats = [table[c] if c is not None else torch.zeros(1, 512) for c in cls]
    ref_depth, ref_edges = restate.graphbins_forward(img, feats, xywh, sd, 0.001, 10, strategy="learned")
    assert rel_dev(out.bin_edges, ref_edges) < 1e-4 and max_rel(out.depth_pred, ref_depth) < 1e-3


def test_side_streams_equal_the_single_stream(monkeypatch):
    """The forward's four forks (hip_ops.forks) -- obj (object branch beside the encoder), token (object branch beside the
    image tokens), head (token chain beside the heads' 3x3 convolution), skip (the decoder's skip-part
    convolutions beside the encoder) -- in every combination, eager and captured: the same kernels on the same operands, so the same
    bits as the single-stream forward, ragged object counts included.  The skip-part convolutions really are issued on the side
    stream (counted), and an AdaBins forward (no object branch) takes the same route."""
    import itertools
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    H, W = 352, 384
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language="clip")
    m = GraphBins(args, object_provider=SyntheticObjectProvider(8, "clip", seed=3)).eval()
    gen.load_into(m, 57, gen.PEAKY)
    m = m.cuda()
    img = gen.randn("img", (2, 3, H, W), 57).cuda()
    feats = [gen.randn("f0", (5, 512), 1).cuda(), gen.randn("f1", (2, 512), 2).cuda()]
    boxes = [torch.rand(5, 4, device="cuda") * 100 + 10, torch.rand(2, 4, device="cuda") * 100 + 10]

    from objcavit_amd import hip_ops as _ops

    def switches(obj, tok, head, skip):
        monkeypatch.setattr(_ops._TLS, "fork_override", {"obj": obj == "1", "token": tok == "1", "head": head == "1", "skip": skip == "1"})

    from objcavit_amd.modules import DenseFeatureExtractor as dfe
    issued = []
    real_on_feature = dfe.SkipPrepass.on_feature

    def counting(self, idx, t):
        real_on_feature(self, idx, t)
        issued.append(len(self.ready))
    monkeypatch.setattr(dfe.SkipPrepass, "on_feature", counting)

    switches("0", "0", "0", "0")
    ref = m(img).depth_pred.clone()
    ref_r = m(img, [f.clone() for f in feats], [b.clone() for b in boxes]).depth_pred.clone()
    assert not issued
    for obj, tok, head, skip in itertools.product("01", "01", "01", "01"):
        switches(obj, tok, head, skip)
        del issued[:]
        for _ in range(2):
            assert torch.equal(m(img).depth_pred, ref), (obj, tok, head, skip)
            assert torch.equal(m(img, [f.clone() for f in feats], [b.clone() for b in boxes]).depth_pred, ref_r), (obj, tok, head, skip)
        assert (max(issued) == 3) if skip == "1" else not issued, (skip, issued)      # three stages' skip parts rode the side stream
        g = GraphedGraphBins(m, img)
        assert torch.equal(g(img).depth_pred, ref) and torch.equal(g(img).depth_pred, ref), (obj, tok, head, skip)
    # a forward without an object branch (AdaBins) on the same route
    from objcavit_amd.modules.AdaBins import AdaBins
    a = AdaBins(make_args(model="adabins", dimensions_train=[H, W], dimensions_test=[H, W])).eval()
    gen.load_into(a, 58, gen.PEAKY)
    a = a.cuda()
    switches("0", "0", "0", "0")
    ref_a = a(img).depth_pred.clone()
    ref_a = a(img).depth_pred.clone()
    switches("1", "1", "1", "1")
    del issued[:]
    assert torch.equal(a(img).depth_pred, ref_a) and max(issued) == 3


def test_decoder_output_in_split_form_only(monkeypatch):
    """GraphBins / AdaBins ask the decoder for its output in split form only (hip_ops.map_placeholder: the last convolution writes 4
    bytes per value instead of 8): same kernels on the same split copy as with the fp32 map written too (OCV_DECODER_FP32=1), so the
    same bits; the placeholder has no storage (NaN, stride 0), ``fp32_map`` rebuilds the map to the pairs' 22 bits, and a patch-embedding
    weight that does NOT fit fp16 pairs takes the rebuilt map through the exact kernel -- reported, finite, at the oracle's bar."""
    from objcavit_amd import hip_ops
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    H, W = 352, 384
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language="clip")
    m = GraphBins(args, object_provider=SyntheticObjectProvider(8, "clip", seed=3)).eval()
    gen.load_into(m, 61, gen.PEAKY)
    m = m.cuda()
    img = gen.randn("img", (2, 3, H, W), 61).cuda()
    monkeypatch.setenv("OCV_DECODER_FP32", "1")
    ref = m(img)
    full = m.dense_feature_extractor(img, _split_only=True)                  # (switch off: the fp32 map is written)
    assert not getattr(full, "_ocv_fp32_missing", False) and bool(torch.isfinite(full).all())
    monkeypatch.delenv("OCV_DECODER_FP32")
    out = m(img)
    assert torch.equal(out.depth_pred, ref.depth_pred) and torch.equal(out.bin_edges, ref.bin_edges)
    ph = m.dense_feature_extractor(img, _split_only=True)
    assert ph._ocv_fp32_missing and ph.stride() == (0, 0, 0, 0) and tuple(ph.shape) == tuple(full.shape) and bool(torch.isnan(ph).all())
    rebuilt = hip_ops.fp32_map(ph)
    assert rebuilt.is_contiguous(memory_format=torch.channels_last) and rel_dev(rebuilt, full) < 2.0 ** -21
    assert m.dense_feature_extractor(img) is not None and not getattr(m.dense_feature_extractor(img), "_ocv_fp32_missing", False)   # the public call
    # the reported fallback: one input column of the patch embedding 2^-30 below the rest in every row -> no fp16 pairs for that weight
    hip_ops.ROUTE_REPORT.clear()
    m.objcavit.image_embedding_convPxP.weight[:, 0, 0, 0] *= 2.0 ** -30      # (in place on the parameter: its version moves)
    out2 = m(img)
    assert "patch_embed" in hip_ops.ROUTE_REPORT, hip_ops.ROUTE_REPORT
    assert bool(torch.isfinite(out2.depth_pred).all())
    hip_ops.ROUTE_REPORT.clear()


@pytest.mark.parametrize("head_overlap", ["1", "0"])
def test_graph_replay_with_eager_island_equals_eager_dispatch(monkeypatch, head_overlap):
    """GraphedGraphBins: graph segments + an eager island + the eager head give bit-identical depth to plain dispatch,
    for the captured image and for new contents of the static input.  With the token chain on a side stream beside the heads'
    3x3 convolution (the default) that launch stays inside the capture -- a capture cannot be cut while a fork is open."""
    n_isl = 2 if head_overlap == "1" else 3
    from objcavit_amd import hip_ops
    monkeypatch.setattr(hip_ops._TLS, "fork_override", {"head": head_overlap == "1"})
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    H, W = 352, 384
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language="clip")
    m = GraphBins(args, object_provider=SyntheticObjectProvider(8, "clip", seed=3)).eval()
    gen.load_into(m, 55, gen.PEAKY)
    m = m.cuda()
    img = gen.randn("img", (2, 3, H, W), 55).cuda()
    ref = m(img).depth_pred.clone()
    island = f"conv3x3|2,{H // 2},{W // 2},128,128"          # three launches per forward: decoder up4 / conv3, head conv3x3
    g = GraphedGraphBins(m, img, eager_ops=(island,))
    # the EMPTY segment between up4's second convolution and conv3 (two adjacent islands) is dropped at capture instead of being
    # replayed on every step; so is the one behind the heads' convolution when that is an island (nothing is launched behind it)
    n_graphs, n_empty = (2, 1) if head_overlap == "1" else (2, 2)
    assert g.islands == [island] * n_isl and len(g.segments) == n_isl + n_graphs and g.empty_segments_dropped == n_empty
    assert torch.equal(g(img).depth_pred, ref)
    img2 = gen.randn("img2", (2, 3, H, W), 56).cuda()
    ref2 = m(img2).depth_pred.clone()
    hip_ops.enable_timing(True)
    out2 = g(img2)
    t = hip_ops.timing_results()
    hip_ops.enable_timing(False)
    assert torch.equal(out2.depth_pred, ref2) and not torch.equal(ref2, ref)
    assert island in t and "bin_head" in t and t[island][0] == n_isl      # the islands are event-timed on every replay
    assert torch.equal(g(img).depth_pred, ref)


def test_shard_padded_to_the_global_nmax_reproduces_the_full_batch():
    """SURVEY.md Q3 under data-parallel sharding: with use_2_saca an image's result depends on the batch's longest object
    list.  A shard that passes the global Nmax (dp.sharded_forward / pad_objects_to) gives the full batch's result; padded to
    its own maximum it computes something else; and the padded shard equals the oracle's statement of the same thing."""
    from objcavit_amd import dp
    kw = dict(strategy="learned_bbox_wh", use_2_saca=True)
    H, W, counts = 352, 384, [70, 12, 5, 9]
    m, sd, img, _, _, _ = _graphbins_pair(kw, 4, H, W, 1, 91)
    feats = [gen.randn(f"f{i}", (n, 512), 91, 10.0 / np.sqrt(512)) for i, n in enumerate(counts)]
    xywh = [gen.boxes(f"b{i}", n, 91, H, W) for i, n in enumerate(counts)]
    cu = lambda ts: [t.cuda() for t in ts]          # noqa: E731
    full = m(img.cuda(), cu(feats), cu(xywh))
    naive = m(img[2:].cuda(), cu(feats[2:]), cu(xywh[2:]))
    shard = dp.sharded_forward(m, img[2:].cuda(), cu(feats[2:]), cu(xywh[2:]), world=2, global_counts=counts)
    # (kernel dispatch depends on the batch size -- split-K, FFN sharing -- so batches of 4 and 2 agree to rounding, not bits)
    assert rel_dev(shard.bin_edges, full.bin_edges[2:]) < 1e-5 and max_rel(shard.depth_pred, full.depth_pred[2:]) < 1e-3
    assert not torch.equal(naive.bin_edges, shard.bin_edges)      # same batch size, same kernels: only the padding rows differ
    ref_depth, ref_edges = restate.graphbins_forward(img[2:], feats[2:], xywh[2:], sd, 0.001, 10, batch_nmax=70, **kw)
    assert rel_dev(shard.bin_edges, ref_edges) < 1e-4 and max_rel(shard.depth_pred, ref_depth) < 1e-3
    with pytest.raises(ValueError):
        m(img[:2].cuda(), cu(feats[:2]), cu(xywh[:2]), pad_objects_to=12)      # smaller than the shard's own longest list


def test_config2_full_size_properties():
    """BASELINE configs[1] shape (NYU 480x640, 16 zero-feature objects, bs=8): runs, is finite, bin edges are
    monotone from min_depth to max_depth, depth lies inside the bin range, and an image's result does not depend
    on its batch mates (data-parallel sharding is safe)."""
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    args = make_args(strategy="learned", language="control_obj_zeros_512")
    m = GraphBins(args, object_provider=SyntheticObjectProvider(16, "control_obj_zeros_512")).eval()
    gen.load_into(m, 5, gen.PEAKY)
    m = m.cuda()
    img = gen.randn("img", (8, 3, 480, 640), 5).cuda()
    out = m(img)
    d, e = out.depth_pred, out.bin_edges
    assert tuple(d.shape) == (8, 1, 240, 320) and tuple(e.shape) == (8, 257)
    assert bool(torch.isfinite(d).all())
    assert bool((e[:, 1:] > e[:, :-1]).all())
    assert abs(float(e[0, 0]) - 0.001) < 1e-6 and abs(float(e[0, -1]) - 10.0) < 1e-3
    assert float(d.min()) >= 0.001 and float(d.max()) <= 10.0
    feats, boxes, _ = m.object_provider(img)
    solo = m(img[3:4], [feats[3]], [boxes[3]]).depth_pred
    # This configuration is a deliberate stress case (N(0,1) "images", 6x logit gain): it amplifies fp32 rounding
    # ~2000x (MIOpen-fp32 convolutions: 1.1e-4 vs CPU; split-bf16 convolutions: 4.7e-4).  Bar = north-star 1e-3.
    assert max_rel(solo, d[3:4]) < 1e-3
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref, _ = restate.graphbins_forward(img[3:4].cpu(), [feats[3].cpu()], [boxes[3].cpu()], sd, 0.001, 10, strategy="learned")
    assert max_rel(d[3:4], ref) < 1e-3 and max_rel(solo, ref) < 1e-3
    # MARGIN PIN (tightened in round 4): rounds 1 - 3 ran the decoder's / heads' convolutions on bf16 pairs
    # (2^-17 products) and measured 4.1e-4 .. 4.7e-4 on this stress case, all of it those products' (exact-fp32 convolutions:
    # 1.06e-4; profiles/r03_stress_margin.txt).  On fp16 pairs (2^-22, round 4) the case sits at ~1.2e-4: four fifths of the 1e-3
    # bar must stay free -- a new re-association or a wider Winograd dispatch that eats it fails HERE, not silently.
    assert max_rel(d[3:4], ref) <= 2e-4, max_rel(d[3:4], ref)


def test_encoder_fast_path_vs_oracle(monkeypatch):
    """EfficientNet-B5 encoder inference plan (folded BN, HIP depthwise kernel) vs the oracle's functional
    restatement on identical weights: every one of the five skip activations; the decoder on them (conv2 composed into
    the first stage's GEMM), the whole extractor (conv_head composed as well) and the un-composed route
    (OCV_UPCONV_FOLD=0), all against the oracle's decoder."""
    from oracle import effnet_ref
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    m = DenseFeatureExtractor(make_args()).eval()
    sd = gen.load_into(m, 9)
    img = gen.randn("img", (2, 3, 224, 288), 9)
    ref = effnet_ref.encoder_features(img, sd, "encoder.original_model.")
    feats = m.cuda().encoder(img.cuda())
    for i in (4, 5, 6, 8, 11):
        assert rel_dev(feats[i], ref[i]) < 1e-4, i
    out = m.decoder(feats)
    ref_out = restate.decoder_forward(ref, sd, "decoder.")
    assert rel_dev(out, ref_out) < 1e-4
    assert out.is_contiguous(memory_format=torch.channels_last)       # decoder runs NHWC on the GPU
    from objcavit_amd.modules.DenseFeatureExtractor import DeferredConv1x1
    deferred = m.encoder(img.cuda(), _defer_head=True)
    assert isinstance(deferred[11], DeferredConv1x1) and rel_dev(deferred[11].materialize(), ref[11]) < 1e-4
    whole = m(img.cuda())
    assert rel_dev(whole, ref_out) < 1e-4
    monkeypatch.setenv("OCV_UPCONV_FOLD", "0")
    separate = m(img.cuda())
    assert rel_dev(separate, ref_out) < 1e-4 and not torch.equal(separate, whole)


@pytest.mark.parametrize("every_project", [False, True])
def test_encoder_pre_split_pointwise_routes_vs_oracle(monkeypatch, every_project):
    """The late MBConv stages on their 1x1 routes: the fp32-row kernels and, where hip_ops.pointwise_hl_project_pays says so (or,
    with the policy patched, on EVERY late project layer), the depthwise output written pre-split with the gate folded into
    per-image weights -- the five skip activations and the extractor's output against the oracle, at a batch whose late stages
    have ragged row counts (7 x 9 and 4 x 5 pixels per image)."""
    from oracle import effnet_ref
    from objcavit_amd import hip_ops
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    if every_project:
        monkeypatch.setattr(hip_ops, "pointwise_hl_project_pays", lambda B, rows, cin, cout: cin % 32 == 0 and cout % 4 == 0 and cin >= 256)
    m = DenseFeatureExtractor(make_args()).eval()
    sd = gen.load_into(m, 9)
    img = gen.randn("img", (3, 3, 224, 288), 9)
    ref = effnet_ref.encoder_features(img, sd, "encoder.original_model.")
    feats = m.cuda().encoder(img.cuda())
    for i in (4, 5, 6, 8, 11):
        assert rel_dev(feats[i], ref[i]) < 1e-4, i
    assert rel_dev(m(img.cuda()), restate.decoder_forward(ref, sd, "decoder.")) < 1e-4


def test_final_upscale_variant_vs_oracle():
    """do_final_upscale=True (reference DenseFeatureExtractor.py:60,116-117): a fifth UpSampleWithSkip stage against the
    IMAGE (3 skip channels: the exact-fp32 convolution kernel takes what the split kernels do not), output at full
    resolution; the all-split pipeline and the composed conv_head / conv2 weight do not apply, so conv_head is applied
    where the encoder deferred it.  Encoder + decoder against the oracle."""
    from oracle import effnet_ref
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    args = make_args()
    args[args.model.name]["do_final_upscale"] = True
    m = DenseFeatureExtractor(args).eval()
    sd = gen.load_into(m, 21)
    img = gen.randn("img", (1, 3, 160, 192), 21)
    ref = restate.decoder_forward(effnet_ref.encoder_features(img, sd, "encoder.original_model."), sd, "decoder.",
                                  do_final_upscale=True)
    out = m.cuda()(img.cuda())
    assert out.shape == ref.shape == (1, 128, 160, 192)
    assert rel_dev(out, ref) < 1e-4


def test_graph_owns_its_scratch_and_survives_larger_eager_calls():
    """A captured graph bakes workspace addresses into its nodes: it keeps its own WorkspaceStore, so an eager forward
    at a LARGER batch afterwards (which re-allocates the module-level buffers) cannot free memory the graph still
    writes; growth inside the graph's frozen store raises instead of re-allocating silently."""
    from objcavit_amd import hip_ops
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    H, W = 352, 384
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language="clip")
    m = GraphBins(args, object_provider=SyntheticObjectProvider(8, "clip", seed=3)).eval()
    gen.load_into(m, 58, gen.PEAKY)
    m = m.cuda()
    img = gen.randn("img", (1, 3, H, W), 58).cuda()
    ref = m(img).depth_pred.clone()
    g = GraphedGraphBins(m, img)
    assert g.scratch.frozen and len(g.scratch) > 0
    own = {k: v.data_ptr() for k, v in g.scratch.items()}
    big = gen.randn("big", (4, 3, H, W), 59).cuda()
    m(big)                                                   # grows the module-level store, never the graph's
    junk = [torch.full((1 << 22,), float("nan"), device="cuda") for _ in range(16)]     # recycle whatever was freed
    assert all(g.scratch[k].data_ptr() == p for k, p in own.items())
    assert not (set(v.data_ptr() for v in g.scratch.values()) & set(v.data_ptr() for v in hip_ops._WS.values()))
    assert torch.equal(g(img).depth_pred, ref)
    del junk
    with hip_ops.workspace_scope(g.scratch), torch.cuda.stream(g.stream):
        k = next(k for k in g.scratch if k[1] == g.stream.cuda_stream)
        with pytest.raises(RuntimeError, match="captured graph"):
            hip_ops.workspace(g.scratch[k].numel() + 1, img.device, k[2])


def test_folded_encoder_weights_follow_in_place_updates():
    """The BN-folded / split-packed encoder weights are keyed on (data_ptr, version) of every parameter and buffer of
    the block: an in-place edit in eval mode must change the fast path's output exactly as it changes the oracle's."""
    from oracle import effnet_ref
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    m = DenseFeatureExtractor(make_args()).eval()
    gen.load_into(m, 9)
    m = m.cuda()
    img = gen.randn("img", (1, 3, 96, 128), 9)
    before = m.encoder(img.cuda())[11].clone()
    blk = m.encoder.original_model.blocks[6][2]              # last block in front of conv_head (activation 11)
    blk.bn2.running_var.mul_(4.0)                            # in place, eval mode, no load_state_dict / train()
    blk.conv_pwl.weight.data.mul_(-3.0)
    blk.se.conv_expand.bias.data.add_(1.0)
    after = m.encoder(img.cuda())[11]
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = effnet_ref.encoder_features(img, sd, "encoder.original_model.")[11]
    assert rel_dev(after, ref) < 1e-4 and rel_dev(before, ref) > 1e-3


def test_lightning_checkpoint_to_gpu_forward_equals_oracle(tmp_path):
    """Row N3 end to end: a checkpoint laid out like the reference's Lightning .ckpt of a full GraphBins run -- every
    model key under ``model.`` (the Q5 prototype-layer keys included), next to metric / loss states, hyper-parameters
    and optimizer state -- is loaded through checkpoint.load_reference_checkpoint into a FRESH drop-in model, and the
    HIP forward of that model equals the oracle's forward on the checkpoint's own tensors."""
    from objcavit_amd.checkpoint import load_reference_checkpoint
    from objcavit_amd.modules.GraphBins import GraphBins
    H, W, seed = 352, 384, 83
    kw = dict(strategy="learned_bbox_wh", use_2_saca=True)
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language="clip", **kw)
    src = GraphBins(args).eval()
    sd = gen.load_into(src, seed, gen.PEAKY)
    assert any(k.startswith("objcavit.saca_1.image_encoder_layers.") for k in sd)            # Q5 prototype keys
    lightning = {"model." + k: v.clone() for k, v in sd.items()}
    lightning.update({"abs_rel.normed_abs_diff_total": torch.tensor(3.0), "abs_rel.total_pixels": torch.tensor(7.0),
                      "loss_fn.silog_loss.dummy": torch.zeros(1)})
    path = tmp_path / "epoch=24-step=37875-last.ckpt"
    torch.save({"epoch": 24, "global_step": 37875, "pytorch-lightning_version": "1.7.7", "state_dict": lightning,
                "optimizer_states": [{"state": {}, "param_groups": []}], "lr_schedulers": [{}],
                "hyper_parameters": {"args": {"model": {"name": "graphbins"}}}}, str(path))
    dst = GraphBins(args).eval()
    gen.load_into(dst, seed + 1)                                                              # different weights first
    missing, unexpected = load_reference_checkpoint(dst, str(path), strict=True)
    assert missing == [] and unexpected == []                  # metric / loss states never reach the model
    dst = dst.cuda()
    img = gen.randn("img", (2, 3, H, W), seed)
    feats = [gen.randn(f"f{i}", (12, 512), seed, 10.0 / np.sqrt(512)) for i in range(2)]
    xywh = [gen.boxes(f"b{i}", 12, seed, H, W) for i in range(2)]
    out = dst(img.cuda(), [f.cuda() for f in feats], [b.cuda() for b in xywh])
    ref_depth, ref_edges = restate.graphbins_forward(img, feats, xywh, sd, 0.001, 10, **kw)
    assert rel_dev(out.bin_edges, ref_edges) < 1e-4
    assert max_rel(out.depth_pred, ref_depth) < 1e-3


def test_ocv_conv_exact_routes_every_dense_convolution_through_the_exact_kernel(monkeypatch):
    """OCV_CONV=exact (+ OCV_PW=fp32 for the 1x1 layers): the hand-written exact-fp32 route for A/B numerics -- round 1
    needed MIOpen for it.  Same model, same inputs: both routes meet the north-star bar against the oracle, and the
    exact one is closer."""
    from objcavit_amd.modules.GraphBins import GraphBins
    H, W, seed = 352, 384, 41
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language="clip")
    img = gen.randn("img", (1, 3, H, W), seed)
    feats = [gen.randn("f0", (7, 512), seed, 10.0 / np.sqrt(512))]
    xywh = [gen.boxes("b0", 7, seed, H, W)]
    errs = {}
    for mode in ("split_bf16", "exact"):
        monkeypatch.setenv("OCV_CONV", mode)
        monkeypatch.setenv("OCV_PW", "split" if mode == "split_bf16" else "fp32")
        m = GraphBins(args).eval()
        sd = gen.load_into(m, seed, gen.PEAKY)
        out = m.cuda()(img.cuda(), [f.cuda() for f in feats], [b.cuda() for b in xywh])
        ref_depth, _ = restate.graphbins_forward(img, feats, xywh, sd, 0.001, 10)
        errs[mode] = max_rel(out.depth_pred, ref_depth)
    assert errs["split_bf16"] < 1e-3 and errs["exact"] < 1e-3
    assert errs["exact"] <= errs["split_bf16"] * 1.5 + 1e-6, errs
    monkeypatch.setenv("OCV_CONV", "miopen")
    with pytest.raises(ValueError):
        GraphBins(args).eval().cuda()(img.cuda(), [f.cuda() for f in feats], [b.cuda() for b in xywh])


def test_two_batches_in_flight_give_the_same_bits():
    """bench.py's default keeps two batches in flight: one GraphedGraphBins per slot (own static input, own scratch
    store), each replayed on its own stream.  Interleaved replays of two slots on two streams must give, for every
    step, exactly the depth of a lone replay -- nothing is shared between slots but read-only weights."""
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    H, W = 352, 384
    args = make_args(dimensions_train=[H, W], dimensions_test=[H, W], language="clip")
    m = GraphBins(args, object_provider=SyntheticObjectProvider(8, "clip", seed=3)).eval()
    gen.load_into(m, 61, gen.PEAKY)
    m = m.cuda()
    imgs = [gen.randn(f"img{i}", (2, 3, H, W), 61 + i).cuda() for i in range(4)]
    refs = [m(im).depth_pred.clone() for im in imgs]
    slots = [GraphedGraphBins(m, imgs[0]) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    assert not (set(v.data_ptr() for v in slots[0].scratch.values()) & set(v.data_ptr() for v in slots[1].scratch.values()))
    torch.cuda.synchronize()
    outs = []
    for rep in range(3):
        for i, im in enumerate(imgs):
            k = i % 2
            with torch.cuda.stream(streams[k]):
                outs.append((i, slots[k](im).depth_pred.clone()))
    torch.cuda.synchronize()
    for i, d in outs:
        assert torch.equal(d, refs[i]), i


# ------------------------------------------------------------------ G8: the HIP encoder against an independent fp64 EfficientNet-B5
G8_CASES = ["nyu_b1", "kitti_b4", "nyu_b16"]
G8_FULL = ("nyu_b1", "kitti_b4")        # the five skips also compared with the oracle at EVERY element
_G8_ORACLE = {}


def _g8_setup(case):
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    meta, z = load_golden(f"g8_effnet_b5_{case}")
    m = DenseFeatureExtractor(make_args()).eval()
    sd = gen.load_into(m, meta["seed"])
    return meta, z, m.cuda(), sd, gen.randn("img", meta["input_shape"], meta["seed"])


def _g8_oracle_skips(case, img, sd):
    """effnet_ref (CPU fp32, pinned by test_g8_effnet_b5_oracle) at the five skips, once per case."""
    from oracle import effnet_ref
    if case not in _G8_ORACLE:
        f = effnet_ref.encoder_features(img, sd, "encoder.original_model.")
        _G8_ORACLE[case] = {i: f[i] for i in (4, 5, 6, 8, 11)}
    return _G8_ORACLE[case]


@pytest.mark.parametrize("route", ["default", "pw_fp32"])
@pytest.mark.parametrize("case", G8_CASES)
def test_g8_hip_encoder_vs_independent_b5(monkeypatch, case, route):
    """The HIP encoder (every stage end, the fused stem, conv_head) against G8 -- transformers' EfficientNetModel in float64 on
    the same seeded weights -- at the shipped sizes and batches, on samples and per-(image, channel) mean / rms relative to max
    |x| (tests/util.golden_sample_dev).  Default route (split-bf16 1x1 GEMMs): <= 1e-4, the bar of
    test_encoder_fast_path_vs_oracle.  OCV_PW=fp32 (exact 1x1 GEMMs): <= 1e-5.

    keep = 3 .. 11 rather than None: with None the Encoder keeps conv_stem / bn1 (1, 2) as well and so does not fuse the stem
    (csrc/stem.hip), which would move the stem to PyTorch ops; 3 .. 11 materialises stages 1, 3 and 4 (7, 9, 10) too and leaves
    every kernel route as in the product.

    Route guards: hip_ops.pointwise_hl_project_pays(B, rows, 1056, 176) is True at kitti_b4 and nyu_b16 and False at nyu_b1;
    expand_depthwise_fusable holds for blocks 1.* and 3.0 (Cin 24 .. 64, 3 x 3) on the split route and nowhere on the fp32 one;
    both routes are counted as they run.

    Measured (MI355X; worst of samples / moments over tensors 3 .. 11, then the five whole skips vs effnet_ref):
      nyu_b1    default 4.8e-6 / 2.3e-6, whole 8.6e-6     pw_fp32 8.2e-7 / 9.1e-8, whole 1.0e-6
      kitti_b4  default 7.1e-6 / 3.6e-6, whole 8.3e-6     pw_fp32 8.5e-7 / 1.0e-7, whole 1.4e-6
      nyu_b16   default 6.9e-6 / 2.6e-6                   pw_fp32 7.8e-7 / 1.1e-7
    The fp32 route sits at the CPU fp32 oracle's own distance from fp64 (<= 1.4e-6), 12x inside its bound; the default route's
    split-bf16 1x1 products (~2^-17 relative each) leave it 14x inside its own."""
    from objcavit_amd import hip_ops
    meta, z, m, sd, img = _g8_setup(case)
    if route == "pw_fp32":
        monkeypatch.setenv("OCV_PW", "fp32")
    B, _, H, W = meta["input_shape"]
    assert hip_ops.pointwise_hl_project_pays(B, (H // 16) * (W // 16), 1056, 176) == (case != "nyu_b1")
    blocks = m.encoder.original_model.blocks
    fusable = {f"{s}.{r}" for s, stage in enumerate(blocks) for r, blk in enumerate(stage) if hasattr(blk, "conv_pwl")
               and hip_ops.expand_depthwise_fusable(blk.conv_pw.in_channels, hip_ops.pointwise_weight(blk.conv_pw.weight),
                                                    blk.conv_dw.kernel_size[0])}
    want_fused = {f"1.{r}" for r in range(5)} | {"3.0"} if route == "default" else set()
    assert fusable == want_fused
    calls = {"pointwise_hl": 0, "expand_depthwise_se_gate": 0}
    for name in calls:
        def counted(*a, _f=getattr(hip_ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(hip_ops, name, counted)
    m.encoder.keep = tuple(range(3, 12))
    feats = m.encoder(img.cuda())
    assert calls["expand_depthwise_se_gate"] == len(want_fused)
    assert calls["pointwise_hl"] == (6 if route == "default" and case != "nyu_b1" else 0)   # stage 4's 1056 -> 176 projects
    bound = 1e-4 if route == "default" else 1e-5
    devs = {}
    for j in range(3, 12):
        assert feats[j] is not None and feats[j].is_cuda
        devs[j] = golden_sample_dev(feats[j], z, f"f{j}")
    print(f"\nG8 encoder [{case}][{route}] sampled / moments: " + " ".join(f"{j}:{s:.2e}/{mo:.2e}" for j, (s, mo) in devs.items()))
    for j, (s, mo) in devs.items():
        assert s <= bound and mo <= bound, (j, s, mo)
    if case in G8_FULL:
        ref = _g8_oracle_skips(case, img, sd)
        full = {i: rel_dev(feats[i], ref[i]) for i in ref}
        print(f"G8 encoder [{case}][{route}] whole skips vs effnet_ref: " + " ".join(f"{i}:{d:.2e}" for i, d in full.items()))
        for i, d in full.items():
            assert d <= 1e-4, (i, d)


@pytest.mark.parametrize("case", G8_CASES)
def test_g8_hip_extractor_vs_independent_b5(monkeypatch, case):
    """The whole extractor on the GPU -- fused stem, composed conv_head, skip prepass, split decoder -- against G8's ``out``: the
    reference's own Decoder in float64 on the independent encoder's activations.  <= 1e-4 composed and with OCV_UPCONV_FOLD=0.
    Measured (MI355X, samples / moments, composed then OCV_UPCONV_FOLD=0): nyu_b1 1.4e-6 / 3.1e-7, 1.4e-6 / 3.6e-7;
    kitti_b4 1.3e-6 / 2.7e-7, 1.3e-6 / 4.8e-7; nyu_b16 9.6e-7 / 2.2e-7, 1.0e-6 / 2.6e-7."""
    meta, z, m, sd, img = _g8_setup(case)
    x = img.cuda()
    devs = {"fold": golden_sample_dev(m(x), z, "out")}
    monkeypatch.setenv("OCV_UPCONV_FOLD", "0")
    devs["nofold"] = golden_sample_dev(m(x), z, "out")
    print(f"\nG8 extractor [{case}] sampled / moments: " + " ".join(f"{k}:{s:.2e}/{mo:.2e}" for k, (s, mo) in devs.items()))
    for k, (s, mo) in devs.items():
        assert s <= 1e-4 and mo <= 1e-4, (k, s, mo)
