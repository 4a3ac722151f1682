"""-m gpu: the EfficientNet-B1 / V2-S / V2-M encoders on the HIP path (reference modules/DenseFeatureExtractor.py:141-166).

* the strided 3x3 implicit GEMM (ocv_conv3x3_nhwc_strided_fwd) against a float64 F.conv2d, and at stride 1 bit for bit
  against ocv_conv_nhwc_fwd;
* each encoder's five skips and the whole extractor against the same module's float64 CPU forward on identical weights;
* AdaBins / GraphBins end to end against the same module's CPU forward (depth: the project's 1e-3 max-rel bar);
* graph replay of V2-M GraphBins bit for bit against eager dispatch;
* no PyTorch convolution anywhere in a GPU forward of the new encoders."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen
from objcavit_amd import hip_ops
from objcavit_amd.config import make_args
from util import max_rel, rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ENCODERS = ["efficientnet-b1", "efficientnet-v2-s", "efficientnet-v2-m"]
KERNEL_TOL = 5e-5
ENC_TOL = 1e-4


def _sweep():
    cases = []
    for i, (cin, cout) in enumerate([(24, 96), (48, 192), (64, 320), (80, 24), (24, 24), (48, 96), (80, 320), (64, 192)]):
        for stride in (1, 2):
            H, W = [(30, 40), (31, 41), (17, 26), (29, 18)][(i + stride) % 4]
            B = 3 if i % 3 == 0 else 1
            for pad in ("sym", "same"):
                act = hip_ops.ACT_SILU if (i + (pad == "same")) % 2 == 0 else hip_ops.ACT_NONE
                res = (i + stride) % 2 == 0
                cases.append((B, cin, cout, H, W, stride, pad, act, res))
    return cases


@pytest.mark.parametrize("B,cin,cout,H,W,stride,pad,act,res", _sweep())
def test_strided_conv3x3_vs_fp64(B, cin, cout, H, W, stride, pad, act, res):
    """act(conv3x3(x) + b) (+ r) with stride 1 / 2 and torchvision's symmetric padding (1, 1) or TF "SAME" offsets (pad_t =
    pad_l = 0, one zero row / column at the bottom / right, output ceil(H / 2) on an even size at stride 2), even and odd H / W, B 1 / 3, with and without SiLU and residual, against float64.
    Bar 5e-5 of max |y| (split-bf16: three bf16 products per term, fp32 accumulation).  Measured: <= 2.9e-6 over the sweep."""
    g = torch.Generator().manual_seed(B * 1000 + cin * 7 + cout + H + W + stride)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    b = torch.randn(cout, generator=g) * 0.1
    if pad == "sym":
        pt, pl = 1, 1
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    else:                                   # TF "SAME": output ceil(H / stride), the extra pad row / column at the bottom / right
        Ho, Wo = -(-H // stride), -(-W // stride)
        pt = max((Ho - 1) * stride + 3 - H, 0) // 2
        pl = max((Wo - 1) * stride + 3 - W, 0) // 2
    pb, pr = (Ho - 1) * stride + 3 - H - pt, (Wo - 1) * stride + 3 - W - pl
    assert pb >= 0 and pr >= 0
    ref = F.conv2d(F.pad(x.double(), (pl, pr, pt, pb)), w.double(), b.double(), stride=stride)
    if act == hip_ops.ACT_SILU:
        ref = F.silu(ref)
    r = torch.randn(B, cout, Ho, Wo, generator=g) if res else None
    if res:
        ref = ref + r.double()
    hi, lo = hip_ops.prep_conv_weight(w.cuda())
    cl = torch.channels_last
    y = hip_ops.conv3x3_strided(x.cuda().contiguous(memory_format=cl), hi, lo, b.cuda(), stride, (pt, pl), act,
                                residual=None if r is None else r.cuda().contiguous(memory_format=cl), out_hw=(Ho, Wo))
    assert tuple(y.shape) == tuple(ref.shape)
    assert rel_dev(y, ref) < KERNEL_TOL


@pytest.mark.parametrize("B,cin,cout,H,W", [(2, 24, 96, 32, 32), (1, 48, 40, 17, 23), (3, 80, 320, 31, 9)])
def test_strided_conv3x3_at_stride1_equals_conv_nhwc(B, cin, cout, H, W):
    """ocv_conv3x3_nhwc_strided_fwd at stride 1 with padding (1, 1) and ocv_conv_nhwc_fwd (k 3, one source) run the same
    kernel: bias, SiLU and residual included, the outputs are equal bit for bit.  M = 2048 fills its pixel tiles exactly;
    391 and 837 leave the last one ragged."""
    g = torch.Generator().manual_seed(B * 100 + cin + cout + H + W)
    cl = torch.channels_last
    x = torch.randn(B, cin, H, W, generator=g).cuda().contiguous(memory_format=cl)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).cuda()
    b = (torch.randn(cout, generator=g) * 0.1).cuda()
    r = torch.randn(B, cout, H, W, generator=g).cuda().contiguous(memory_format=cl)
    hi, lo = hip_ops.prep_conv_weight(w)
    for res in (None, r):
        y1 = hip_ops.conv_nhwc(x, None, hi, lo, b, 3, hip_ops.ACT_SILU, residual=res)
        y2 = hip_ops.conv3x3_strided(x, hi, lo, b, 1, (1, 1), hip_ops.ACT_SILU, residual=res)
        assert torch.equal(y1, y2)


def _extractor(enc, seed):
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    m = DenseFeatureExtractor(make_args(model="adabins", encoder_name=enc)).eval()
    sd = gen.load_into(m, seed)
    return m, sd


@pytest.mark.parametrize("enc", ENCODERS)
def test_hip_encoder_and_extractor_vs_fp64_cpu(enc):
    """Every one of the five skips and the extractor's output (decoder at 1280 features) of the HIP path against the same
    module's CPU forward in float64, identical weights, 480 x 640, B 1 and B 2 at 352 x 1216.  Bar 1e-4 of max |x| (the bar of
    test_encoder_fast_path_vs_oracle)."""
    m, _ = _extractor(enc, 21)
    ref_m = copy.deepcopy(m).double()
    g = m.cuda()
    for B, H, W in ((1, 480, 640), (2, 352, 1216)):
        img = gen.randn("img", (B, 3, H, W), 21 + B)
        ref = ref_m.encoder(img.double())
        feats = g.encoder(img.cuda())
        for i in g.decoder.feature_select:
            assert rel_dev(feats[i], ref[i]) < ENC_TOL, (enc, B, i)
        out = g(img.cuda())
        ref_out = ref_m.decoder(ref)
        assert rel_dev(out, ref_out) < ENC_TOL, (enc, B)


def _model(kind, enc, seed):
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    H, W = 480, 640
    if kind == "adabins":
        m = AdaBins(make_args(model="adabins", encoder_name=enc, dimensions_train=[H, W], dimensions_test=[H, W])).eval()
    else:
        args = make_args(strategy="learned", language="clip", encoder_name=enc, dimensions_train=[H, W], dimensions_test=[H, W])
        m = GraphBins(args, object_provider=SyntheticObjectProvider(8, "clip", seed=3)).eval()
    sd = gen.load_into(m, seed, gen.PEAKY)
    return m, sd


@pytest.mark.parametrize("kind,enc", [("graphbins", "efficientnet-v2-m"), ("adabins", "efficientnet-v2-s"),
                                      ("adabins", "efficientnet-b1")])
@pytest.mark.parametrize("B", [1, 16])
def test_models_end_to_end_vs_cpu(kind, enc, B):
    """V2-M GraphBins (learned positional embedding, the ObjCAViT config), V2-S AdaBins and B1 AdaBins at 480 x 640: depth of the
    HIP path within 1e-3 max-rel (the project's bar; at bs 16 on the first image, AbsRel < 1e-5 over the batch), bin edges within
    1e-4, and the dense features within 1e-4 of max |x|, of the CPU forward on identical weights: the same
    module's DenseFeatureExtractor on the CPU (plain PyTorch, float64), then the oracle's mViT / ObjCAViT and bin head."""
    from oracle import restate
    m, sd = _model(kind, enc, 31)
    img = gen.randn("img", (B, 3, 480, 640), 31 + B)
    dense = copy.deepcopy(m.dense_feature_extractor).double()(img.double()).float()     # the extractor's CPU forward, float64
    if kind == "adabins":
        out = m.cuda()(img.cuda())
        y, ram = restate.mvit_forward(dense, sd, "adaptive_bins_layer.")
    else:
        feats = [gen.randn(f"f{i}", (12, 512), 31, 10.0 / np.sqrt(512)) for i in range(B)]
        xywh = [gen.boxes(f"b{i}", 12, 31, 480, 640) for i in range(B)]
        out = m.cuda()(img.cuda(), [f.cuda() for f in feats], [b.cuda() for b in xywh])
        y, ram = restate.objcavit_forward(dense, feats, xywh, sd, "objcavit.", strategy="learned")
    ref_depth, ref_edges = restate.bin_head(y, ram, sd["conv_out.0.weight"], sd["conv_out.0.bias"], 0.001, 10)
    assert rel_dev(m.dense_feature_extractor(img.cuda()), dense) < ENC_TOL
    # bs 16: the max-rel bar on one image of the batch, as test_config2_full_size_properties does; AbsRel over all 16.  The
    # gen.PEAKY heads amplify the features' rounding ~100x at the worst pixel: V2-M GraphBins measured features 1.1e-5 of max |x|
    # from float64 and, over all 16 x 240 x 320 pixels, one pixel at 1.02e-3 max-rel
    assert max_rel(out.depth_pred[:1], ref_depth[:1]) < 1e-3
    assert restate.abs_rel(out.depth_pred.cpu(), ref_depth) < 1e-5
    assert rel_dev(out.bin_edges, ref_edges) < 1e-4
    assert float(ref_depth.max() - ref_depth.min()) > 0.01


def test_graph_replay_of_v2m_graphbins_equals_eager():
    from objcavit_amd.graph import GraphedGraphBins
    m = _model("graphbins", "efficientnet-v2-m", 41)[0].cuda()
    img = gen.randn("img", (2, 3, 480, 640), 41).cuda()
    ref = m(img).depth_pred.clone()
    g = GraphedGraphBins(m, img)
    assert torch.equal(g(img).depth_pred, ref)
    img2 = gen.randn("img2", (2, 3, 480, 640), 42).cuda()
    ref2 = m(img2).depth_pred.clone()
    out2 = g(img2).depth_pred
    assert torch.equal(out2, ref2) and not torch.equal(ref2, ref)


@pytest.mark.parametrize("enc", ENCODERS)
def test_no_pytorch_convolution_on_the_gpu_path(monkeypatch, enc):
    """F.conv2d and nn.Conv2d._conv_forward raise during a GPU forward of the extractor: every convolution of the new encoders
    (and of the decoder at 1280 features) is a hand-written kernel."""
    m, _ = _extractor(enc, 5)
    m = m.cuda()
    img = gen.randn("img", (1, 3, 480, 640), 5).cuda()

    def boom(*a, **k):
        raise AssertionError("PyTorch convolution on the GPU inference path")

    monkeypatch.setattr(F, "conv2d", boom)
    monkeypatch.setattr(torch.nn.Conv2d, "_conv_forward", boom)
    out = m(img)
    assert out.shape == (1, 128, 240, 320) and bool(torch.isfinite(out).all())


def test_no_pytorch_convolution_with_final_upscale_at_1280_features(monkeypatch):
    """V2-S with do_final_upscale: 80 up-sampled channels are no whole 32-blocks, so the fifth stage cannot take the all-split
    pipeline and the decoder runs stage by stage on conv2's materialised output (it once handed up1 the shape-only stand-in of
    the composed route).  Still no PyTorch convolution: the 83-channel convolution runs on the exact-fp32 kernel; the output is
    at full resolution and agrees with the module's float64 CPU forward."""
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    m = DenseFeatureExtractor(make_args(model="adabins", encoder_name="efficientnet-v2-s", do_final_upscale=True)).eval()
    gen.load_into(m, 5)
    img = gen.randn("img", (1, 3, 192, 208), 5)
    ref = copy.deepcopy(m).double()(img.double())
    m = m.cuda()

    def boom(*a, **k):
        raise AssertionError("PyTorch convolution on the GPU inference path")

    monkeypatch.setattr(F, "conv2d", boom)
    monkeypatch.setattr(torch.nn.Conv2d, "_conv_forward", boom)
    out = m(img.cuda())
    assert out.shape == ref.shape == (1, 128, 192, 208)
    assert rel_dev(out, ref) < ENC_TOL


G_FIXTURES = [("g9_effnet_b1_nyu_b1", "efficientnet-b1"), ("g9_effnet_b1_kitti_b2", "efficientnet-b1"),
              ("g10_effnet_v2s_nyu_b1", "efficientnet-v2-s"), ("g10_effnet_v2m_nyu_b1", "efficientnet-v2-m")]


@pytest.mark.parametrize("name,enc", G_FIXTURES)
def test_hip_encoder_vs_g9_g10(name, enc):
    """The HIP encoder's five skips and the whole extractor against the float64 fixtures (G9: transformers' B1 + the reference
    Decoder; G10: the reference's DenseFeatureExtractor class around the V2 backbone), samples and moments within 1e-4 of max |x|."""
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    from util import golden_sample_dev, load_golden
    meta, z = load_golden(name)
    m = DenseFeatureExtractor(make_args(model="adabins", encoder_name=enc)).eval()
    gen.load_into(m, meta["seed"])
    m = m.cuda()
    img = gen.randn("img", tuple(meta["input_shape"]), meta["seed"]).cuda()
    feats = m.encoder(img)
    for k, j in enumerate(m.decoder.feature_select):
        d = golden_sample_dev(feats[j], z, f"s{k}")
        assert max(d) < ENC_TOL, (k, d)
    d = golden_sample_dev(m(img), z, "out")
    assert max(d) < ENC_TOL, d


def test_pipelined_validation_with_v2m_graphbins():
    """PipelinedValidation (the reference's bs-1 validation loop, four steps in flight, captured image + mirror graphs) with the
    V2-M GraphBins model gives the records of ValidationStep(joint=True) issued one after the other."""
    from objcavit_amd.validation import PipelinedValidation, ValidationStep
    m = _model("graphbins", "efficientnet-v2-m", 51)[0].cuda()
    args = m.args
    N = 6
    imgs = [gen.randn(f"im{i}", (1, 3, 480, 640), 500 + i).cuda() for i in range(N)]
    gts = [(torch.rand(1, 1, 480, 640, generator=torch.Generator().manual_seed(i)) * 9.0 + 0.5).cuda() for i in range(N)]
    seq = ValidationStep(m, args, joint=True)
    ref = torch.cat([seq(imgs[i], gts[i], first_image_id=i)[0] for i in range(N)], 0)
    pv = PipelinedValidation(m, args, imgs[0])
    for i in range(N):
        pv.submit(imgs[i], gts[i], first_image_id=i)
    rec = pv.collect()
    assert rec.shape == (N, 10) and torch.equal(rec[:, 8:], ref[:, 8:])
    assert rel_dev(rec[:, :8], ref[:, :8]) < 1e-5
