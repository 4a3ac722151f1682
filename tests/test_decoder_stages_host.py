"""The decoder shadow of tests/test_hip_decoder_stages.py on the CPU: the float32 module's plain PyTorch path stands in for the
device path and is checked against its float64 copy, unit by unit, each on its own input.  This pins the harness itself: every
unit is visited exactly once per forward (on the CPU a stage is ONE unit: ``forward`` computes its first convolution inline),
float32 rounding sits inside the tightest GPU bar, and a defect of five times that bar at one element of the LAST image of one
stage's output fails that (unit, image) and nothing else -- the stages behind it read the defective tensor as their own input."""
import pytest
import torch

import gen
from decoder_shadow import DecoderShadow, F16_TOL
from objcavit_amd.config import make_args

torch.set_grad_enabled(False)

# (encoder, do_final_upscale, the stage whose output is perturbed)
CASES = [("efficientnet-b5", False, "up3"), ("efficientnet-b1", False, "up4"), ("efficientnet-v2-s", False, "up1"),
         ("efficientnet-v2-m", False, "up2"), ("efficientnet-b5", True, "final_upscale")]
B, H, W = 3, 64, 96


def _run(m, sh, img, defect=None):
    sh.records.clear()
    sh.defect = defect
    try:
        with sh:
            m(img)
    finally:
        sh.defect = None
    return sh


@pytest.mark.parametrize("enc,final,target", CASES)
def test_decoder_shadow_harness_on_cpu(enc, final, target):
    """Measured (float32 CPU against float64, 3 x 64 x 96): worst unit deviation 5.8e-7 (B5), 4.7e-7 (B1), 4.9e-7 (V2-S),
    4.9e-7 (V2-M), 5.8e-7 (B5 + final_upscale), against an assert of 4e-6 (F16_TOL, the tightest GPU bar of a whole stage); the
    perturbed run fails (target, image 2) at 2e-5 and nothing else."""
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    m = DenseFeatureExtractor(make_args(model="adabins", encoder_name=enc, do_final_upscale=final)).eval()
    gen.load_into(m, 61)
    img = gen.randn("img", (B, 3, H, W), 61)
    sh = DecoderShadow(m.decoder, head=getattr(m.encoder.original_model, "conv_head", None))

    _run(m, sh, img)
    units = ["conv2", "up1", "up2", "up3", "up4"] + (["final_upscale"] if final else []) + ["conv3"]
    assert [r["name"] for r in sh.records] == units
    assert all(r["images"] == [0, 1, 2] and r["pad_ok"] for r in sh.records)
    h, w = (H, W) if final else (H // 2, W // 2)
    assert sh.records[-1]["out_shape"] == (128, h, w)
    worst = {r["name"]: max(r["devs"]) for r in sh.records}
    print(f"\n{enc}{' final_upscale' if final else ''}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) < F16_TOL, sh.failures(lambda n: F16_TOL)[:5]

    def bump(y):
        # +5 x the bar of image B-1's own largest value at one element: the stage's real output, read by the stages behind it
        y = y.clone()
        y[B - 1, 1, 2, 3] += 5 * F16_TOL * float(y[B - 1].abs().max())
        return y

    bad = _run(m, sh, img, defect=(target, bump)).failures(lambda n: F16_TOL)
    assert [(n, i) for _, n, i, _ in bad] == [(target, B - 1)], bad
    assert 0.9 * 5 * F16_TOL < bad[0][0] < 1.1 * 5 * F16_TOL, bad
    assert not _run(m, sh, img).failures(lambda n: F16_TOL)         # (and the defect is what made it fail)
