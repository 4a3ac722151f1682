"""-m "not gpu": the EfficientNet-B1 / V2-S / V2-M encoders on the host (reference modules/DenseFeatureExtractor.py:141-166):
construction from the reference's six params/*.yaml files that name them (copies under tests/golden/params/), torchvision /
gen-efficientnet key forms and the published parameter counts, strict checkpoint loading, the CPU forward against the G9 / G10
fixtures, and the host-side contract of the strided convolution's entry point (no launch)."""
import ctypes
import glob
import os
import re

import pytest
import torch

import gen
from objcavit_amd import _lib
from objcavit_amd.config import load_reference_config, make_args
from util import golden_sample_dev, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "params", "*.yaml")))
torch.set_grad_enabled(False)


def test_six_reference_configs_are_present():
    names = [os.path.basename(p) for p in PARAMS]
    assert names == sorted(["nyu_efficientnet-v2-m_clip_0.1.yaml", "nyu_efficientnet-v2-m_clip_0.1_lossfixed.yaml",
                            "nyu_efficientnet-v2-m_swa.yaml", "nyu_graphbins_enet-v2-m_ocv_pos_learned_emb_128_1.yaml",
                            "nyu_efficientnet-v2-s_clip_0.1_lossfixed.yaml", "nyu_efficientnet-b1_clip_0.1.yaml"])


@pytest.mark.parametrize("path", PARAMS, ids=os.path.basename)
def test_reference_config_builds_its_model(path):
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    from objcavit_amd.modules.GraphBins import GraphBins
    args = load_reference_config(path)
    name = args.model.name
    enc = args[name].encoder_name
    dfe = DenseFeatureExtractor(args)
    m = (GraphBins if name == "graphbins" else AdaBins)(args)
    feats = 2048 if "b5" in enc else 1280
    assert dfe.decoder.conv2.in_channels == feats and dfe.decoder.conv3.in_channels == feats // 16
    expect = {"efficientnet-b1": [4, 5, 6, 8, 11], "efficientnet-v2-s": [2, 3, 4, 6, 9], "efficientnet-v2-m": [2, 3, 4, 6, 9]}
    assert m.dense_feature_extractor.decoder.feature_select == expect[enc]


PARAM_COUNTS = {"efficientnet_v2_s": 21458488, "efficientnet_v2_m": 54139356, "tf_efficientnet_b1_ap": 7794184}


@pytest.mark.parametrize("name", sorted(PARAM_COUNTS))
def test_backbone_parameter_counts_equal_the_published_ones(name):
    from objcavit_amd.modules import efficientnet, efficientnet_v2
    ctor = getattr(efficientnet_v2, name, None) or getattr(efficientnet, name)
    assert sum(p.numel() for p in ctor().parameters()) == PARAM_COUNTS[name]


def test_v2_key_forms_follow_torchvision():
    from objcavit_amd.modules.efficientnet_v2 import efficientnet_v2_m, efficientnet_v2_s
    for ctor, n_feat, head_in in ((efficientnet_v2_s, 8, 256), (efficientnet_v2_m, 9, 512)):
        m = ctor()
        assert list(m._modules) == ["features", "avgpool", "classifier"] and len(m.features) == n_feat
        sd = m.state_dict()
        assert tuple(sd["features.0.0.weight"].shape) == (24, 3, 3, 3)
        assert all(f"features.0.1.{p}" in sd for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"))
        assert tuple(sd["features.1.0.block.0.0.weight"].shape) == (24, 24, 3, 3) and "features.1.0.block.1.0.weight" not in sd
        assert tuple(sd["features.2.0.block.0.0.weight"].shape) == (96, 24, 3, 3)
        assert tuple(sd["features.2.0.block.1.0.weight"].shape) == (48, 96, 1, 1)
        assert tuple(sd["features.4.0.block.1.0.weight"].shape[1:]) == (1, 3, 3)
        mid = sd["features.4.0.block.0.0.weight"].shape[0]
        cin = sd["features.4.0.block.0.0.weight"].shape[1]
        assert tuple(sd["features.4.0.block.2.fc1.weight"].shape) == (cin // 4, mid, 1, 1)
        assert tuple(sd["features.4.0.block.2.fc2.bias"].shape) == (mid,)
        assert tuple(sd[f"features.{n_feat - 1}.0.weight"].shape) == (1280, head_in, 1, 1)
        assert tuple(sd["classifier.1.weight"].shape) == (1000, 1280)
        assert all(b.eps == 1e-3 for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
        assert all(c.padding == ((c.kernel_size[0] - 1) // 2,) * 2 for c in m.modules() if isinstance(c, torch.nn.Conv2d))


def test_b1_key_forms_follow_gen_efficientnet():
    from objcavit_amd.modules.efficientnet import tf_efficientnet_b1_ap, tf_efficientnet_b5_ap
    m = tf_efficientnet_b1_ap()
    sd = m.state_dict()
    assert [len(s) for s in m.blocks] == [2, 3, 3, 4, 4, 5, 2]
    assert tuple(sd["conv_stem.weight"].shape) == (32, 3, 3, 3) and tuple(sd["conv_head.weight"].shape) == (1280, 320, 1, 1)
    assert tuple(sd["blocks.0.0.se.conv_reduce.weight"].shape) == (8, 32, 1, 1)
    assert tuple(sd["blocks.1.0.conv_pw.weight"].shape) == (96, 16, 1, 1)
    b5 = tf_efficientnet_b5_ap()                      # default unchanged
    assert [len(s) for s in b5.blocks] == [3, 5, 5, 7, 7, 9, 3] and b5.conv_head.out_channels == 2048


@pytest.mark.parametrize("enc,model", [("efficientnet-b1", "adabins"), ("efficientnet-v2-s", "adabins"),
                                       ("efficientnet-v2-m", "graphbins")])
def test_lightning_shaped_checkpoint_loads_strictly(enc, model):
    from objcavit_amd.checkpoint import load_reference_checkpoint
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.GraphBins import GraphBins
    args = make_args(model=model, encoder_name=enc)
    ctor = GraphBins if model == "graphbins" else AdaBins
    src = ctor(args)
    sd = gen.load_into(src, 7)
    ckpt = {"state_dict": {"model." + k: v for k, v in sd.items()}, "epoch": 3}
    ckpt["state_dict"]["abs_rel.total_pixels"] = torch.tensor(1.0)
    dst = ctor(args)
    missing, unexpected = load_reference_checkpoint(dst, ckpt, strict=True)
    assert missing == [] and unexpected == []
    probe = [k for k in sd if ".encoder.original_model." in k][-3]
    assert torch.equal(dst.state_dict()[probe], sd[probe])


FIXTURES = [("g9_effnet_b1_nyu_b1", "efficientnet-b1"), ("g9_effnet_b1_kitti_b2", "efficientnet-b1"),
            ("g10_effnet_v2s_nyu_b1", "efficientnet-v2-s"), ("g10_effnet_v2m_nyu_b1", "efficientnet-v2-m")]


def fixture_extractor(name, enc):
    """(extractor with the fixture's seeded weights, input image, fixture meta, arrays)."""
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    meta, z = load_golden(name)
    m = DenseFeatureExtractor(make_args(model="adabins", encoder_name=enc)).eval()
    gen.load_into(m, meta["seed"])
    return m, gen.randn("img", tuple(meta["input_shape"]), meta["seed"]), meta, z


@pytest.mark.parametrize("name,enc", FIXTURES)
def test_cpu_forward_vs_g9_g10(name, enc):
    """The module's float32 CPU forward against the float64 fixtures (G9: transformers' B1 + the reference Decoder; G10: the
    reference's own DenseFeatureExtractor class around the local V2 backbone): the five skips and the output within 1e-5."""
    m, img, meta, z = fixture_extractor(name, enc)
    feats = m.encoder(img)
    sel = m.decoder.feature_select
    for k, j in enumerate(sel):
        d = golden_sample_dev(feats[j], z, f"s{k}")
        assert max(d) < 1e-5, (k, d)
    d = golden_sample_dev(m.decoder(feats), z, "out")
    assert max(d) < 1e-5, d


def test_strided_conv_symbol_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bocv_conv3x3_nhwc_strided_fwd\s*\(", hdr)
    assert "ocv_conv3x3_nhwc_strided_fwd" in _lib.PROTOTYPES and _lib.ABI_VERSION == 5


def test_strided_conv_argument_validation_on_the_host():
    if not os.path.exists(_lib.LIB_PATH):
        from objcavit_amd.build import build
        build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16          # a 16-byte aligned host address: never dereferenced

    def call(x=p, w=p, y=p, B=1, H=8, W=8, Cin=24, Cout=96, stride=2, pt=1, pl=1, Ho=4, Wo=4, act=3):
        return lib.ocv_conv3x3_nhwc_strided_fwd(x, Cin, w, w, None, None, y, B, H, W, Cout, stride, pt, pl, Ho, Wo, act, None)

    assert call(x=None) == -1 and b"null pointer" in lib.ocv_last_error()
    assert call(y=None) == -1 and b"null pointer" in lib.ocv_last_error()
    assert call(stride=3) == -1 and b"stride must be 1 or 2" in lib.ocv_last_error()
    assert call(stride=0) == -1 and b"stride" in lib.ocv_last_error()
    assert call(pt=3) == -1 and b"bad padding" in lib.ocv_last_error()
    assert call(pl=-1) == -1 and b"bad padding" in lib.ocv_last_error()
    assert call(Ho=6) == -1 and b"output larger" in lib.ocv_last_error()
    assert call(Cin=22) == -1 and b"multiple of 4" in lib.ocv_last_error()
    assert call(act=7) == -1 and b"activation" in lib.ocv_last_error()


def test_depthwise_argument_validation_on_the_host():
    """The three depthwise entry points share one geometry check; each keeps its own prefix, and a channel count of 0 (or any
    that is no multiple of 4) is an argument error of the two that walk channels in quads, never a launch."""
    if not os.path.exists(_lib.LIB_PATH):
        from objcavit_amd.build import build
        build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16          # a 16-byte aligned host address: never dereferenced

    def plain(B=1, C=8, H=8, W=8, k=3, s=1, pt=1, pl=1, Ho=8, Wo=8, act=0, x=p):
        return lib.ocv_depthwise_conv_nhwc_fwd(x, p, None, p, B, C, H, W, k, s, pt, pl, Ho, Wo, act, None)

    def summed(B=1, C=8, H=8, W=8, k=3, s=1, pt=1, pl=1, Ho=8, Wo=8, x=p):
        return lib.ocv_depthwise_conv_nhwc_sum_fwd(x, p, None, p, p, B, C, H, W, k, s, pt, pl, Ho, Wo, None)

    def summed_hl(B=1, C=32, H=8, W=8, k=3, s=1, pt=1, pl=1, Ho=8, Wo=8, x=p):
        return lib.ocv_depthwise_conv_nhwc_sum_hl_fwd(x, p, None, None, p, p, B, C, H, W, k, s, pt, pl, Ho, Wo, None)

    def fused(B=1, H=8, W=8, Cin=24, mid=144, k=3, s=1, pt=1, pl=1, Ho=8, Wo=8, x=p):
        return lib.ocv_mbconv_expand_dw_fwd(x, p, None, p, None, p, p, B, H, W, Cin, mid, k, s, pt, pl, Ho, Wo, None)

    for call, prefix in ((plain, b"ocv_depthwise_conv_nhwc_fwd: "), (summed, b"ocv_depthwise_conv_nhwc_sum_fwd: "),
                         (summed_hl, b"ocv_depthwise_conv_nhwc_sum_fwd: ")):
        for kw in (dict(C=0), dict(C=-4), dict(C=3), dict(C=6), dict(B=0), dict(H=0), dict(Wo=0)):
            if call is summed_hl and kw.get("C", 0) % 32 != 0:          # the split output's own check (C % 32) comes first
                continue
            assert call(**kw) == -1 and lib.ocv_last_error() == prefix + b"bad sizes (C must be a multiple of 4)", kw
    for call, prefix in ((plain, b"ocv_depthwise_conv_nhwc_fwd: "), (summed, b"ocv_depthwise_conv_nhwc_sum_fwd: "),
                         (fused, b"ocv_mbconv_expand_dw_fwd: ")):
        assert call(x=None) == -1 and lib.ocv_last_error() == prefix + b"null pointer"
        assert call(k=4) == -1 and lib.ocv_last_error().startswith(prefix + b"k must be 3 or 5 and stride 1 or 2")
        assert call(s=3) == -1 and lib.ocv_last_error().startswith(prefix + b"k must be 3 or 5 and stride 1 or 2")
        assert call(pt=3) == -1 and lib.ocv_last_error() == prefix + b"bad padding"
        assert call(pl=-1) == -1 and lib.ocv_last_error() == prefix + b"bad padding"
        assert call(Ho=10) == -1 and lib.ocv_last_error() == prefix + b"output larger than the padded input allows"
        assert call(x=p + 4) == -1 and lib.ocv_last_error() == prefix + b"operands must be 16-byte aligned"
    assert plain(act=2) == -1 and b"activation must be none or SiLU" in lib.ocv_last_error()
    assert summed_hl(C=8) == -1 and b"multiple of 32" in lib.ocv_last_error()
    assert fused(B=0) == -1 and lib.ocv_last_error() == b"ocv_mbconv_expand_dw_fwd: bad sizes"
    assert fused(Cin=20) == -1 and b"Cin must be a multiple of 8 in [24, 64] (got 20)" in lib.ocv_last_error()
    assert fused(mid=0) == -1 and b"expanded channels must be a multiple of 4 (got 0)" in lib.ocv_last_error()
