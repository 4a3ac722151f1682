"""Fixtures of the EfficientNet-B1 / V2-S / V2-M encoders (build machine only; reuses make_golden's helpers).

G9  B1: transformers' EfficientNetModel built from the B1 config (width 1.0, depth 1.1, hidden_dim 1280) -- an independent
    implementation, as G8 is for B5 -- loaded with the product's seeded weights paired in order, float64; its activations feed
    the reference's own Decoder (efficientnet-b1 branch).  480 x 640 B 1, 352 x 1216 B 2.
G10 V2-S / V2-M: the reference's own DenseFeatureExtractor class (oracle.ref_import) with torchvision.models.efficientnet_v2_{s,m}
    stubbed to return the local backbone: this pins the reference's Encoder order, its Identity replacements, feature_select,
    num_features and Decoder.  float64, 480 x 640 B 1.  At generation time the stubbed run is checked against the functional
    restatement tests/effnet_v2_ref.py (F.conv2d, explicit padding, weights by torchvision key) within 1e-6 of max |x|.
    There is no third-party EfficientNetV2 on the build machine: for V2 the arithmetic pin is that restatement plus the
    published parameter counts (tests/test_encoders_host.py).
Each fixture stores, per tensor (the five skips and the decoder output), G8's sampled values, per-(image, channel) mean / rms and
max |x|.   python tests/golden/make_golden_encoders.py [g9] [g10]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen                      # noqa: E402
import make_golden as mg        # noqa: E402
from objcavit_amd.config import make_args  # noqa: E402
from oracle import ref_import   # noqa: E402

torch.set_grad_enabled(False)

G9_CASES = {"nyu_b1": ((1, 3, 480, 640), 91), "kitti_b2": ((2, 3, 352, 1216), 92)}
G9_HF_STAGE_ENDS = (2, 5, 8, 12, 16, 21, 23)          # hidden_states index of the end of stages 0 .. 6 (23 blocks)
G10_CASES = {"v2s_nyu_b1": ("efficientnet-v2-s", (1, 3, 480, 640), 101), "v2m_nyu_b1": ("efficientnet-v2-m", (1, 3, 480, 640), 102)}
TENSORS = ("s0", "s1", "s2", "s3", "s4", "out")        # the decoder's five skips (feature_select order) and its output


def _stats(arrays, absmax, t, i, v, idx):
    sel = idx[:, 0] == i
    ii = torch.from_numpy(idx[sel].astype(np.int64))
    arrays[t + "_val"][sel] = mg._np(v[ii[:, 1], ii[:, 2], ii[:, 3]])
    arrays[t + "_mean"][i] = mg._np(v.mean((1, 2)))
    arrays[t + "_rms"][i] = mg._np(v.pow(2).mean((1, 2)).sqrt())
    absmax[t] = max(absmax[t], float(v.abs().max()))


def _write(name, meta, per_image, shape, seed):
    """per_image(i) -> {tensor: [C, H, W] float64} for image i of the seeded input."""
    B = shape[0]
    idx = shapes = None
    arrays, absmax = {}, {t: 0.0 for t in TENSORS}
    for i in range(B):
        f = per_image(i)
        if idx is None:
            shapes = {t: [B] + list(f[t].shape) for t in TENSORS}
            idx = {t: mg._g8_sample_index(shapes[t], seed, t) for t in TENSORS}
            for t in TENSORS:
                arrays[t + "_val"] = np.zeros(len(idx[t]), np.float64)
                arrays[t + "_mean"] = np.zeros(shapes[t][:2], np.float64)
                arrays[t + "_rms"] = np.zeros(shapes[t][:2], np.float64)
        for t in TENSORS:
            _stats(arrays, absmax, t, i, f[t], idx[t])
    out = {}
    for t in TENSORS:
        out[t + "_idx"] = idx[t]
        for s in ("val", "mean", "rms"):
            out[f"{t}_{s}"] = arrays[f"{t}_{s}"].astype(np.float32)
        out[t + "_absmax"] = np.array(absmax[t], np.float64)
    mg._save(name, dict(meta, seed=seed, input_shape=list(shape), shapes=shapes, tensors=list(TENSORS)), **out)


def _hf_b1():
    os.environ["HF_HUB_OFFLINE"] = "1"
    os.environ["TRANSFORMERS_OFFLINE"] = "1"
    stubs = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] == "torchvision"}
    try:
        import transformers
        from transformers import EfficientNetConfig, EfficientNetModel
    finally:
        sys.modules.update(stubs)
    cfg = EfficientNetConfig(width_coefficient=1.0, depth_coefficient=1.1, hidden_dim=1280)
    hf = EfficientNetModel(cfg).eval()
    assert sum(p.numel() for p in hf.parameters()) == 6513184
    return hf, cfg, transformers.__version__


def _load_hf(hf, product):
    enc = {k: v for k, v in product.state_dict().items() if k.startswith("encoder.original_model.")
           and not k.endswith("num_batches_tracked")}
    own = hf.state_dict()
    hf_keys = [k for k in own if not k.endswith("num_batches_tracked") and not k.startswith("encoder.top_bn.")]
    assert len(enc) == len(hf_keys), (len(enc), len(hf_keys))
    pairs = list(zip(enc, hf_keys))
    for pk, hk in pairs:
        assert tuple(enc[pk].shape) == tuple(own[hk].shape), (pk, hk)
    pd = dict(pairs)
    assert pd["encoder.original_model.conv_stem.weight"] == "embeddings.convolution.weight"
    assert pd["encoder.original_model.conv_head.weight"] == "encoder.top_conv.weight"
    sd = {hk: enc[pk] for pk, hk in pairs}
    sd.update({k: v for k, v in own.items() if k.endswith("num_batches_tracked") and not k.startswith("encoder.top_bn.")})
    res = hf.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and len(res.missing_keys) == 4, res
    return hf.double(), len(pairs)


def g9_effnet_b1():
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    dfe = ref_import.load("DenseFeatureExtractor")
    for tag, (shape, seed) in G9_CASES.items():
        m = DenseFeatureExtractor(make_args(model="adabins", encoder_name="efficientnet-b1")).eval()
        sd = gen.load_into(m, seed)
        hf, cfg, ver = _hf_b1()
        hf, n_keys = _load_hf(hf, m)
        dec = dfe.Decoder(num_classes=128, num_features=1280, bottleneck_features=1280, mode=None,
                          encoder_name="efficientnet-b1", do_final_upscale=None).eval()
        dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
        dec.double()
        img = gen.randn("img", shape, seed)
        m64 = m.double()
        dev = [0.0]

        def per_image(i):
            hs = hf(pixel_values=img[i:i + 1].double(), output_hidden_states=True).hidden_states
            assert len(hs) == 24
            feats = [None] * 16
            for j, e in zip((4, 5, 6, 8), (G9_HF_STAGE_ENDS[0], G9_HF_STAGE_ENDS[1], G9_HF_STAGE_ENDS[2], G9_HF_STAGE_ENDS[4])):
                feats[j] = hs[e]
            feats[11] = hf.encoder.top_conv(hs[23])
            f = {f"s{k}": feats[j][0] for k, j in enumerate((4, 5, 6, 8, 11))}
            f["out"] = dec(feats)[0]
            mine = m64(img[i:i + 1].double())[0]                 # the product's own module (CPU, float64)
            dev[0] = max(dev[0], float((mine - f["out"]).abs().max() / f["out"].abs().max()))
            return f

        _write(f"g9_effnet_b1_{tag}", dict(hf_version=ver, hf_config=cfg.to_diff_dict(), hf_stage_ends=list(G9_HF_STAGE_ENDS),
                                           n_keys=n_keys), per_image, shape, seed)
        print(f"G9 B1[{tag}] product module (fp64) vs HF + reference Decoder (fp64): {dev[0]:.2e}")
        assert dev[0] <= 1e-10


def g10_effnet_v2():
    import effnet_v2_ref
    from objcavit_amd.config import AttrDict
    from objcavit_amd.modules import efficientnet_v2
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    dfe = ref_import.load("DenseFeatureExtractor")
    tvm = sys.modules["torchvision.models"]
    for tag, (enc, shape, seed) in G10_CASES.items():
        variant = enc[-1]
        prod = DenseFeatureExtractor(make_args(model="adabins", encoder_name=enc)).eval()
        sd = gen.load_into(prod, seed)
        tvm.efficientnet_v2_s = lambda weights=None: efficientnet_v2.efficientnet_v2_s()
        tvm.efficientnet_v2_m = lambda weights=None: efficientnet_v2.efficientnet_v2_m()
        args = AttrDict(dict(model=dict(name="adabins"), adabins=dict(n_bins=256, encoder_name=enc)))
        ref = dfe.DenseFeatureExtractor(args).eval()
        ref.load_state_dict(sd, strict=True)
        ref.double()
        assert ref.decoder.feature_select == [2, 3, 4, 6, 9]
        img = gen.randn("img", shape, seed)
        dev = [0.0, 0.0]

        def per_image(i):
            x = img[i:i + 1].double()
            feats = ref.encoder(x)
            assert len(feats) == (11 if variant == "s" else 12)
            restated = effnet_v2_ref.features(x, sd, variant, "encoder.original_model.")
            for j, t in enumerate(feats[:len(restated)]):
                dev[0] = max(dev[0], float((t - restated[j]).abs().max() / restated[j].abs().max()))
            f = {f"s{k}": feats[j][0] for k, j in enumerate(ref.decoder.feature_select)}
            f["out"] = ref.decoder(feats)[0]
            mine = prod.double()(x)[0]
            dev[1] = max(dev[1], float((mine - f["out"]).abs().max() / f["out"].abs().max()))
            return f

        _write(f"g10_effnet_{tag}", dict(encoder=enc), per_image, shape, seed)
        print(f"G10 {enc}[{tag}] reference class (stubbed backbone) vs effnet_v2_ref restatement: {dev[0]:.2e}; "
              f"product module vs reference: {dev[1]:.2e}")
        assert dev[0] <= 1e-6 and dev[1] <= 1e-10


if __name__ == "__main__":
    for w in sys.argv[1:] or ["g9", "g10"]:
        {"g9": g9_effnet_b1, "g10": g10_effnet_v2}[w]()
