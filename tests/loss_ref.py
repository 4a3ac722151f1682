"""Float64 restatement of the reference's validation loss (losses/LossWrapper.py:51-67, losses/SILogLoss.py:28-56,
losses/BinsChamferLoss.py:21-37 with pytorch3d 0.7.0 ``chamfer_distance`` defaults: squared distance, point reduction mean, batch
reduction mean), of the per-image pieces the device kernel writes (dp.LOSS_FIELDS), and the scenes of the G11 fixtures
(tests/golden/make_golden_losses.py pins this file to the reference's own classes).  numpy / torch on the CPU only.

The Chamfer terms are found by sorted search in both directions (centres among the sorted targets, targets among the sorted centres),
not by the 256 x T distance matrix the fixture generator's stand-in for pytorch3d forms: two statements of one number.
"""
import numpy as np
import torch

COEFFS = (1.0, 0.1)                       # loss.coeffs of 55 of the 57 reference configs, for names ['silog', 'bins_chamfer']

# tag: (B, (h, w), (H, W), min_depth, max_depth, share of pixels with ground truth, seed)
LOSS_CASES = {
    "nyu": (3, (240, 320), (480, 640), 0.001, 10.0, 1.0, 5),
    "kitti": (2, (176, 608), (352, 1216), 0.001, 80.0, 0.05, 6),
    "odd": (2, (11, 13), (37, 29), 0.001, 10.0, 0.9, 7),
    "equal": (2, (60, 80), (60, 80), 0.001, 10.0, 1.0, 8),          # do_final_upscale: prediction at the ground truth's size
}


def scene(B, H, W, dmax, sparse, seed):
    """Ground truth [B, 1, H, W] fp32: a smooth surface over a fifth of the depth range, roughly 37 - 57 % of it (most intervals
    between bin centres stay empty), a share ``sparse`` of the pixels measured (the others 0 = no ground truth), a block above the
    range.  (A band at 15 - 45 % under predictions uniform in [0.2, 1.2 max] has 0.85 mean(g)^2 = 0.70 .. 0.84 against 0.5 mean(g^2)
    = 0.49 .. 0.57: SILog's subtraction would amplify rounding by more than the tolerances below allow for.  The band sits where
    the fixtures' conditioning assertion holds for every image, with and without the mirror.)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for b in range(B):
        base = 0.42 * dmax + 0.10 * dmax * (yy / H) * rs.uniform(.5, 1) + 0.05 * dmax * np.sin(xx / W * 6 + b)
        base = base + rs.uniform(0, 0.002 * dmax, (H, W))
        m = rs.uniform(size=(H, W)) < sparse
        g = np.where(m, base, 0.0).astype(np.float32)
        g[:min(4, H), :min(4, W)] = 1.5 * dmax
        out.append(g)
    return torch.from_numpy(np.stack(out)[:, None])


def clustered_edges(B, n_bins, dmin, dmax, seed):
    """Bin edges [B, n_bins + 1] fp32 with widths u^8 + 0.1, normalised: a few wide bins, the centres in clusters."""
    rs = np.random.RandomState(seed)
    wdt = rs.uniform(0, 1, (B, n_bins)) ** 8 + 0.1
    wdt /= wdt.sum(1, keepdims=True)
    e = np.concatenate([np.full((B, 1), dmin), dmin + np.cumsum((dmax - dmin) * wdt, 1)], 1)
    return torch.from_numpy(e.astype(np.float32))


def case_inputs(tag, n_bins=256):
    """(gt, pred, pred_mirror, bin_edges, min_depth, max_depth) of a G11 case, regenerated from its seed."""
    B, (h, w), (H, W), dmin, dmax, sparse, seed = LOSS_CASES[tag]
    gt = scene(B, H, W, dmax, sparse, seed)
    rs = np.random.RandomState(seed + 100)
    pa = torch.from_numpy(rs.uniform(0.2, 1.2 * dmax, (B, 1, h, w)).astype(np.float32))
    pb = torch.from_numpy(rs.uniform(0.2, 1.2 * dmax, (B, 1, h, w)).astype(np.float32))
    return gt, pa, pb, clustered_edges(B, n_bins, dmin, dmax, seed + 200), dmin, dmax


# ---------------------------------------------------------------------------------------------------------------------------------
def final_prediction(pred, pred_mirror, dmin, dmax):
    """modules/GraphBinsLM.py:159-181: clamp, un-flip the mirrored forward's map, average.  The input's dtype is kept."""
    a = torch.clamp(pred, min=dmin, max=dmax)
    if pred_mirror is None:
        return a
    return 0.5 * (a + torch.clamp(pred_mirror.flip(dims=[3]), min=dmin, max=dmax))


def resize_bilinear_ac(x, H, W):
    """F.interpolate(x, (H, W), mode='bilinear', align_corners=True) written out (float64): four taps, all four terms always."""
    x = x.double()
    h, w = x.shape[2:]
    if (h, w) == (H, W):
        return x
    sy = torch.arange(H, dtype=torch.float64) * ((h - 1) / (H - 1) if H > 1 else 0.0)
    sx = torch.arange(W, dtype=torch.float64) * ((w - 1) / (W - 1) if W > 1 else 0.0)
    ya, xa = sy.floor().long().clamp(max=h - 1), sx.floor().long().clamp(max=w - 1)
    yb, xb = (ya + 1).clamp(max=h - 1), (xa + 1).clamp(max=w - 1)
    h1, w1 = (sy - ya)[:, None], (sx - xa)[None, :]
    h0, w0 = 1.0 - h1, 1.0 - w1
    t = lambda yi, xi: x[:, :, yi][:, :, :, xi]                                   # noqa: E731
    return h0 * (w0 * t(ya, xa) + w1 * t(ya, xb)) + h1 * (w0 * t(yb, xa) + w1 * t(yb, xb))


def depth_mask(gt, dmin, dmax):
    return (gt > dmin) & (gt <= dmax)


def silog(pred, gt, mask):
    """losses/SILogLoss.py:43-56 on any number of images at once (float64)."""
    p = resize_bilinear_ac(pred, *gt.shape[2:])[mask]
    g = torch.log(p) - torch.log(gt.double()[mask])
    n = g.numel()
    if n == 0:
        return float("nan")
    return float(10.0 * torch.sqrt((g ** 2).sum() / n - (0.85 / n ** 2) * g.sum() ** 2))


def chamfer_1d(centres, targets):
    """(cham_x, cham_y) of one image: mean over the centres of the squared distance to the nearest target, and the same over the
    targets to the nearest centre (float64 numpy arrays); (0, 0) without targets."""
    c, t = np.sort(np.asarray(centres, np.float64)), np.sort(np.asarray(targets, np.float64))
    if t.size == 0:
        return 0.0, 0.0

    def nearest_sq(a, s):                   # for every a: squared distance to the nearest element of the sorted s
        j = np.searchsorted(s, a)
        left, right = s[np.clip(j - 1, 0, s.size - 1)], s[np.clip(j, 0, s.size - 1)]
        return np.minimum((a - left) ** 2, (a - right) ** 2)
    return float(nearest_sq(c, t).mean()), float(nearest_sq(t, c).sum() / t.size)


def centres_of(bin_edges):
    e = bin_edges.double()
    return 0.5 * (e[:, 1:] + e[:, :-1])


def bins_chamfer(bin_edges, gt, mask):
    """losses/BinsChamferLoss.py:24-37: (sum_b cham_x_b + sum_b cham_y_b) / B."""
    c = centres_of(bin_edges).numpy()
    B = gt.shape[0]
    tot = 0.0
    for b in range(B):
        cx, cy = chamfer_1d(c[b], gt[b].double()[mask[b]].numpy())
        tot += cx + cy
    return tot / B


def loss_call(pred, pred_mirror, gt, bin_edges, dmin, dmax, coeffs=COEFFS):
    """One reference call on B images -> (total, silog, bins_chamfer)."""
    final, mask = final_prediction(pred.double(), None if pred_mirror is None else pred_mirror.double(), dmin, dmax), depth_mask(gt, dmin, dmax)
    s, c = silog(final, gt, mask), bins_chamfer(bin_edges, gt, mask)
    return coeffs[0] * s + coeffs[1] * c, s, c


def per_image_pieces(pred, pred_mirror, gt, bin_edges, dmin, dmax):
    """[B, 5] float64: sum g, sum g^2, n (masked pixels), cham_x, cham_y of every image."""
    final, mask = final_prediction(pred.double(), None if pred_mirror is None else pred_mirror.double(), dmin, dmax), depth_mask(gt, dmin, dmax)
    p = resize_bilinear_ac(final, *gt.shape[2:])
    c = centres_of(bin_edges).numpy()
    rows = []
    for b in range(gt.shape[0]):
        g = torch.log(p[b][mask[b]]) - torch.log(gt[b].double()[mask[b]])
        cx, cy = chamfer_1d(c[b], gt[b].double()[mask[b]].numpy())
        rows.append([float(g.sum()), float((g ** 2).sum()), float(g.numel()), cx, cy])
    return torch.tensor(rows, dtype=torch.float64)


def loss_records(pred, pred_mirror, gt, bin_edges, dmin, dmax, first_image_id=0):
    """[B, 6] float64, the device's loss record (dp.LOSS_FIELDS): mean_g, mean_g2, n_mask, cham_x, cham_y, image_id."""
    pc = per_image_pieces(pred, pred_mirror, gt, bin_edges, dmin, dmax)
    n = pc[:, 2].clamp(min=1.0)
    ids = torch.arange(first_image_id, first_image_id + pc.shape[0], dtype=torch.float64)
    return torch.stack([pc[:, 0] / n, pc[:, 1] / n, pc[:, 2], pc[:, 3], pc[:, 4], ids], 1)


def records_from_pieces(pieces, first_image_id=0):
    """The wide [B, 16] fp32 table a ``loss=True`` step returns, from per-image pieces [B, 5]: metric columns zero except n_valid
    (= n_mask here) and image_id."""
    pc = torch.as_tensor(pieces, dtype=torch.float64)
    B = pc.shape[0]
    n = pc[:, 2].clamp(min=1.0)
    ids = torch.arange(first_image_id, first_image_id + B, dtype=torch.float64)
    rec = torch.zeros(B, 16, dtype=torch.float64)
    rec[:, 8], rec[:, 9] = pc[:, 2], ids
    rec[:, 10], rec[:, 11], rec[:, 12], rec[:, 13], rec[:, 14], rec[:, 15] = pc[:, 0] / n, pc[:, 1] / n, pc[:, 2], pc[:, 3], pc[:, 4], ids
    return rec.float()


def far_centres(centres, targets):
    """How many centres have their nearest target beyond the two intervals (between sorted centres) adjacent to them."""
    c, t = np.sort(np.asarray(centres, np.float64)), np.sort(np.asarray(targets, np.float64))
    if t.size == 0:
        return 0
    j = np.searchsorted(t, c)
    left, right = t[np.clip(j - 1, 0, t.size - 1)], t[np.clip(j, 0, t.size - 1)]
    near = np.where((c - left) ** 2 <= (c - right) ** 2, left, right)
    interval = np.searchsorted(c, near, side="right")            # number of centres <= the target
    k = np.arange(c.size)
    return int(((interval != k) & (interval != k + 1)).sum())


def silog_conditioning(pieces):
    """(0.85 mean(g)^2, 0.5 mean(g^2)) of a batch from its per-image pieces: the first must not exceed the second."""
    pc = torch.as_tensor(pieces, dtype=torch.float64)
    n = pc[:, 2].sum()
    return float(0.85 * (pc[:, 0].sum() / n) ** 2), float(0.5 * pc[:, 1].sum() / n)
