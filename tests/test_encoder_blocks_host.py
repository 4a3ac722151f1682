"""The block shadow of tests/test_hip_encoder_blocks.py on the CPU: the float32 module's plain PyTorch path stands in for the
device path and is checked against its float64 copy, block by block.  This pins the harness itself: every block is visited
exactly once per forward, float32 rounding sits far inside the GPU test's bar, and a defect of 1e-4 of one block's residual
branch, in the LAST image of the batch only, fails that block and no other."""
import pytest
import torch

import gen
from block_shadow import Shadow, is_residual
from objcavit_amd.config import make_args

torch.set_grad_enabled(False)

KERNEL_TOL = 5e-5
# (encoder, blocks, the block whose output is perturbed): B5 3 DS + 36 IR, B1 2 + 21, V2-S 10 Fused + 30 MBConv, V2-M 13 + 44
CASES = [("efficientnet-b5", 39, "blocks.4.3"), ("efficientnet-b1", 23, "blocks.3.2"),
         ("efficientnet-v2-s", 40, "features.2.2"), ("efficientnet-v2-m", 57, "features.5.6")]
B, H, W = 3, 64, 96


def _run(m, img, perturb=None):
    backbone = m.encoder.original_model
    sh = Shadow(backbone)
    with sh:
        handle = None
        if perturb is not None:
            blk = dict(backbone.named_modules())[perturb]
            assert is_residual(blk)

            def bump(mod, args, y):
                # +1e-4 of image B-1's own branch at one element, ahead of the shadow's hook (prepend)
                x = args[0]
                y = y.clone()
                y[B - 1, 1, 2, 3] += 1e-4 * float((y[B - 1] - x[B - 1]).abs().max())
                return y

            handle = blk.register_forward_hook(bump, prepend=True)
        try:
            feats = m.encoder(img)
        finally:
            if handle is not None:
                handle.remove()
        if feats[3] is not None and not hasattr(backbone, "features"):
            sh.check_stem(img, feats[3])
    return sh


@pytest.mark.parametrize("enc,n_blocks,target", CASES)
def test_block_shadow_harness_on_cpu(enc, n_blocks, target):
    """Measured (float32 CPU against float64, 3 x 64 x 96): worst block deviation 5.5e-7 (B5), 6.4e-7 (B1), 7.5e-7 (V2-S),
    8.4e-7 (V2-M), against an assert of 5e-6; the perturbed run fails (target, image 2) at 1e-4 and nothing else."""
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    m = DenseFeatureExtractor(make_args(model="adabins", encoder_name=enc)).eval()
    gen.load_into(m, 61)
    m.encoder.keep = tuple(range(3, 12))
    img = gen.randn("img", (B, 3, H, W), 61)

    sh = _run(m, img)
    blocks = [r for r in sh.records if r["kind"] in ("DepthwiseSeparableConv", "InvertedResidual", "FusedMBConv", "MBConv")]
    assert len(blocks) == n_blocks
    visits = sh.visits()
    assert set(visits.values()) == {1}, [n for n, c in visits.items() if c != 1]
    assert set(visits) == {n for n, _, _ in sh.targets} | ({"stem"} if "-v2-" not in enc else set())
    assert all(r["images"] == [0, 1, 2] for r in sh.records)
    worst = max(d for r in sh.records for d in r["devs"])
    print(f"\n{enc}: {len(sh.records)} checks, worst {worst:.1e}")
    assert worst < KERNEL_TOL / 10, sh.failures(KERNEL_TOL / 10)[:5]
    assert sum(r["residual"] for r in sh.records) > 0

    bad = _run(m, img, perturb=target).failures(KERNEL_TOL)
    assert [(n, i) for _, n, _, i in bad] == [(target, B - 1)], bad
    assert 0.9e-4 < bad[0][0] < 1.1e-4, bad
