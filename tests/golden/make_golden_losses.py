"""Fixtures of the validation loss (build machine only; reuses make_golden's helpers).

G11  The reference's OWN SILogLoss, BinsChamferLoss and LossWrapper (losses/*.py, imported from the reference tree), run in float64
     on the scenes of tests/loss_ref.py (LOSS_CASES), once on the B-image batch and once per single image -- the reference validates
     at bs 1 -- and once in fp32 (the classes' own rounding: the margin the device is judged against).
     pytorch3d is not on the build machine: ``pytorch3d.loss.chamfer_distance`` is a stand-in placed in sys.modules, a brute-force
     statement of the 0.7.0 defaults (squared distance; per cloud, mean over its valid points of the distance to the nearest valid
     point of the other cloud; point reduction mean, batch reduction mean) in the inputs' dtype, cross-checked here against
     scipy.spatial.cKDTree.  Masking, pad_sequence, the lengths and the weighted sum are the reference's code.
     NOT the reference's code: the prediction handed to the classes.  modules/GraphBinsLM.py:159-181 (clamp, un-flip the mirrored
     forward's map, average) sits inside a LightningModule step and is restated by loss_ref.final_prediction, as make_golden.py's
     G6 restates it for the metrics: pinned by reading only, so a mistake there (a wrong flip dimension, say) would enter fixture
     and loss_ref alike.  The device forms the value in csrc/metrics.hip's tap(), shared with the metric path.
     Each case asserts its preconditions: at least half of the centres have their nearest target beyond the adjacent intervals
     (an "adjacent interval only" Chamfer is wrong on them), and 0.85 mean(g)^2 <= 0.5 mean(g^2) (SILog's subtraction amplifies
     rounding by <= ~5x).  The fixtures hold seeds, shapes and results; inputs are regenerated from the seeds.
     python tests/golden/make_golden_losses.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden as mg        # noqa: E402
import loss_ref as lr           # noqa: E402
from objcavit_amd.config import make_args  # noqa: E402
from oracle import ref_import   # noqa: E402

torch.set_grad_enabled(False)
_LAST = {}                       # per-image (cham_x, cham_y) of the stand-in's last call


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, **kw):
    """pytorch3d 0.7.0 defaults for x [N, P, 1] (all P valid) and padded y [N, T, 1] with y_lengths."""
    assert not kw and x_lengths is None and x.shape[2] == 1 and y.shape[2] == 1
    N = x.shape[0]
    cx, cy = [], []
    for b in range(N):
        T = int(y_lengths[b])
        c, t = x[b, :, 0], y[b, :T, 0]
        if T == 0:
            cx.append(x.new_zeros(())); cy.append(x.new_zeros(()))
            continue
        mx = torch.full_like(c, float("inf"))
        sy = x.new_zeros(())
        for lo in range(0, T, 16384):
            d = (c[:, None] - t[None, lo:lo + 16384]) ** 2
            mx = torch.minimum(mx, d.min(1).values)
            sy = sy + d.min(0).values.sum()
        cx.append(mx.sum() / c.numel()); cy.append(sy / max(T, 1))
    _LAST["x"], _LAST["y"] = torch.stack(cx), torch.stack(cy)
    return (torch.stack(cx).sum() + torch.stack(cy).sum()) / N, None


def _reference_classes():
    if "pytorch3d" not in sys.modules:
        p3, p3l = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.loss")
        p3l.chamfer_distance = chamfer_distance
        p3.loss = p3l
        sys.modules["pytorch3d"], sys.modules["pytorch3d.loss"] = p3, p3l
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from losses.BinsChamferLoss import BinsChamferLoss
    from losses.LossWrapper import LossWrapper
    from losses.SILogLoss import SILogLoss
    return SILogLoss, BinsChamferLoss, LossWrapper


def _kdtree_witness(edges, gt, mask, b):
    from scipy.spatial import cKDTree
    c = (0.5 * (edges[b, 1:].double() + edges[b, :-1].double())).numpy()[:, None]
    t = gt[b].double()[mask[b]].numpy()[:, None]
    return float((cKDTree(t).query(c)[0] ** 2).mean()), float((cKDTree(c).query(t)[0] ** 2).sum() / len(t))


def _run(classes, args, final, gt, mask, edges):
    """(total, silog, bins_chamfer, per-image cham_x, cham_y) of one call of the reference's classes in final's dtype."""
    SILogLoss, BinsChamferLoss, LossWrapper = classes
    tup = (final, edges.to(final.dtype))
    g = gt.to(final.dtype)
    total = float(LossWrapper(args)(final, g, mask, tup))
    s = float(SILogLoss(args)(final, g, mask, tup))
    c = float(BinsChamferLoss(args)(final, g, mask, tup))
    assert abs(total - (args.loss.coeffs[0] * s + args.loss.coeffs[1] * c)) <= 1e-6 * abs(total)
    return total, s, c, _LAST["x"].double().numpy().copy(), _LAST["y"].double().numpy().copy()


def g11():
    classes = _reference_classes()
    args = make_args()
    assert list(args.loss.names) == ["silog", "bins_chamfer"] and tuple(args.loss.coeffs) == lr.COEFFS
    for tag, (B, (h, w), (H, W), dmin, dmax, sparse, seed) in lr.LOSS_CASES.items():
        gt, pa, pb, edges, _, _ = lr.case_inputs(tag)
        mask = (gt > dmin) & (gt <= dmax)
        final64 = lr.final_prediction(pa.double(), pb.double(), dmin, dmax)
        final32 = lr.final_prediction(pa, pb, dmin, dmax)
        tot, s, c, cx, cy = _run(classes, args, final64, gt, mask, edges)
        tot32, s32, c32, _, _ = _run(classes, args, final32, gt, mask, edges)
        single = np.array([_run(classes, args, final64[b:b + 1], gt[b:b + 1], mask[b:b + 1], edges[b:b + 1])[:3] for b in range(B)])
        # per-image SILog sums with the reference's own resize (F.interpolate, float64) and mask
        p = torch.nn.functional.interpolate(final64, (H, W), mode="bilinear", align_corners=True)
        pieces = np.zeros((B, 5))
        for b in range(B):
            g = torch.log(p[b][mask[b]]) - torch.log(gt[b].double()[mask[b]])
            pieces[b] = [float(g.sum()), float((g ** 2).sum()), g.numel(), cx[b], cy[b]]
            kx, ky = _kdtree_witness(edges, gt, mask, b)
            assert abs(kx - cx[b]) <= 1e-12 * kx and abs(ky - cy[b]) <= 1e-12 * ky, (tag, b, kx, cx[b], ky, cy[b])
        n = pieces[:, 2].sum()
        assert abs(10 * np.sqrt(pieces[:, 1].sum() / n - 0.85 / n ** 2 * pieces[:, 0].sum() ** 2) - s) <= 1e-12 * s
        # preconditions
        cen = lr.centres_of(edges).numpy()
        far = [lr.far_centres(cen[b], gt[b].double()[mask[b]].numpy()) for b in range(B)]
        assert min(far) >= cen.shape[1] // 2, (tag, far)
        lhs, rhs = lr.silog_conditioning(pieces)
        assert lhs <= rhs, (tag, lhs, rhs)
        for b in range(B):
            lhs, rhs = lr.silog_conditioning(pieces[b:b + 1])
            assert lhs <= rhs, (tag, b, lhs, rhs)
        print(f"  {tag}: total {tot:.9f} silog {s:.9f} chamfer {c:.9f}; fp32 classes rel dev silog {abs(s32 - s) / s:.1e} "
              f"chamfer {abs(c32 - c) / c:.1e}; far centres {far}; n {pieces[:, 2].astype(int).tolist()}")
        meta = dict(tag=tag, B=B, h=h, w=w, H=H, W=W, min_depth=dmin, max_depth=dmax, sparse=sparse, seed=seed, n_bins=256,
                    coeffs=list(lr.COEFFS), far_centres=far)
        mg._save(f"g11_val_loss_{tag}", meta, batch=np.array([tot, s, c]), single=single, pieces=pieces,
                 batch_fp32=np.array([tot32, s32, c32]))


if __name__ == "__main__":
    g11()
