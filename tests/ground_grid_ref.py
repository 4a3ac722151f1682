"""Statement G (include/objcavit_hip.h) in torch on the CPU: the bird's-eye occupancy grid csrc/ground_grid.hip is compared with.

Everything per point is evaluated in fp32 with ONE eager torch op per rounding (a subtraction, a division, a product, a sum: each rounded
on its own, as the kernel's ``__fmul_rn`` & co.), so cell and band membership are the kernel's bit for bit; what is accumulated per cell is
integers (counts, the 64-bit sum of rint(1024 h)) and extremes, which do not depend on an order.  The tests therefore ask for EQUALITY.
``dtype=torch.float64`` evaluates the same statement in float64 from the same fp32 inputs (``membership_gap``: how many points change
their cell or band membership -- a condition on the inputs, not on the kernel).  ``mutation`` plants one deliberate error
(tests/test_ground_grid_host.py shows that the cases tell each of them apart).  The keep rule is the point cloud's own statement
(tests/point_cloud_ref.py: ``keep_mask``), plus: all twelve pose values of the image finite.

The kernel's tile is 1024 consecutive candidates of the strided pixel grid in row-major order, not a 2-D tile, so the shapes are chosen by
the rule "one tile; a few ragged tiles; more ragged tiles; a W % 4 == 0 shape" in candidates: 8 x 8 = 64 (one ragged tile), 19 x 70 = 1330
(2 tiles), 37 x 131 = 4847 (5 tiles, the last ragged, rows straddling tile edges), 21 x 132 = 2772 (3 tiles) -- the normals' shapes."""
import math
from collections import namedtuple

import torch

import normals_ref
import point_cloud_ref

F32, F64 = torch.float32, torch.float64
INF = float("inf")
NEAR, FAR = 0.5, 25.0
CASE_B = 3
CASE_SHAPES = ((8, 8), (19, 70), (37, 131), (21, 132))
PITCH, ROLL, HEIGHT = 0.07, -0.03, 1.65
BAND_LO = -0.5
MUTATIONS = ("swap_xy", "trunc", "band_exclusive", "pose_rows", "obstacle_ge")
OUTPUTS = ("count", "obstacle", "h_min", "h_max", "h_mean", "state", "first_occupied")

Spec = namedtuple("Spec", ["x0", "y0", "cell", "GX", "GY"])
# (GX, GY, cell) are the issue's; the origins let points fall off every side and make g_0 - x0 negative for many of them (a truncation
# in place of floorf then fills column 0 / row 0), except the one-cell grid, which takes everything
GRIDS = (Spec(-50.0, -50.0, 100.0, 1, 1), Spec(-3.4, 3.3, 1.0, 7, 5), Spec(-7.9, 1.1, 0.25, 64, 48), Spec(-1.63, 2.05, 0.1, 33, 129),
         Spec(-10.02, 0.51, 0.05, 400, 400))
Grid = namedtuple("Grid", OUTPUTS)
Case = namedtuple("Case", ["depth", "K", "pose", "options"])      # options: band, obstacle_height (keywords of ``ground_grid``)


def _s(v, dtype) -> torch.Tensor:
    """A scalar argument as the C ABI receives it (a float: fp32), in the dtype of the evaluation."""
    return torch.tensor(float(v), dtype=F32).to(dtype)


def pose_matrix(height: float = HEIGHT, pitch: float = PITCH, roll: float = ROLL) -> torch.Tensor:
    """fp64 [3, 4] = [A Rx(pitch) Rz(roll) | (0, 0, height)] (objcavit_amd/ground_grid.py: ``ground_pose``'s matrices, written out)."""
    cp, sp, cr, sr = math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    A = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]], dtype=F64)
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, cp, sp], [0.0, -sp, cp]], dtype=F64)
    Rz = torch.tensor([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]], dtype=F64)
    return torch.cat([A @ Rx @ Rz, torch.tensor([[0.0], [0.0], [height]], dtype=F64)], 1)


def keep(depth, K, pose, stride=(1, 1), near=NEAR, far=FAR, confidence=None, min_confidence=0.0, depth_std=None, max_std=INF):
    """bool [B, H, W]: the cloud's predicate per image, and every pose value of the image finite."""
    B = depth.shape[0]
    rows = []
    for b in range(B):
        m = point_cloud_ref.keep_mask(depth[b, 0], K[b], stride, near, far, None if confidence is None else confidence[b, 0], min_confidence,
                                      None if depth_std is None else depth_std[b, 0], max_std)
        rows.append(m if bool(torch.isfinite(pose[b]).all()) else torch.zeros_like(m))
    return torch.stack(rows, 0)


def ground_points(depth, K, pose, dtype=F32, mutation=None):
    """(g_0, g_1, g_2) [B, H, W] of EVERY pixel (NaN where the inputs are), one op per rounding, the sums left to right."""
    B, _, H, W = depth.shape
    z = depth[:, 0].to(dtype)
    k, p = K.to(dtype), pose.to(dtype).view(B, 3, 4)
    if mutation == "pose_rows":
        p = p[:, [1, 2, 0]]
    fx, fy, cx, cy = (k[:, i].view(B, 1, 1) for i in range(4))
    x = torch.arange(W).to(dtype).view(1, 1, W)
    y = torch.arange(H).to(dtype).view(1, H, 1)
    rx = (x - cx) / fx
    ry = (y - cy) / fy
    X = rx * z
    Y = ry * z
    return tuple(((p[:, i, 0].view(B, 1, 1) * X + p[:, i, 1].view(B, 1, 1) * Y) + p[:, i, 2].view(B, 1, 1) * z) + p[:, i, 3].view(B, 1, 1)
                 for i in range(3))


def membership(depth, K, pose, spec: Spec, band, dtype=F32, mutation=None):
    """(member bool [B, H, W], cell int64 [B, H, W] = iy * GX + ix (0 where not a member), g_2) of every pixel, the keep rule aside."""
    g0, g1, g2 = ground_points(depth, K, pose, dtype, mutation)
    if mutation == "swap_xy":
        g0, g1 = g1, g0
    whole = torch.trunc if mutation == "trunc" else torch.floor
    fxi = whole((g0 - _s(spec.x0, dtype)) / _s(spec.cell, dtype))
    fyi = whole((g1 - _s(spec.y0, dtype)) / _s(spec.cell, dtype))
    inside = (fxi >= 0) & (fxi < _s(spec.GX, dtype)) & (fyi >= 0) & (fyi < _s(spec.GY, dtype))          # NaN fails
    lo, hi = _s(band[0], dtype), _s(band[1], dtype)
    in_band = ((lo < g2) & (g2 < hi)) if mutation == "band_exclusive" else ((lo <= g2) & (g2 <= hi))
    member = inside & in_band
    cell = torch.where(member, fyi * spec.GX + fxi, torch.zeros_like(fxi)).to(torch.int64)
    return member, cell, g2


def ground_grid(depth, K, pose, spec: Spec, band=(BAND_LO, 2.5), obstacle_height=0.3, min_points=1, min_obstacle_points=1, stride=(1, 1),
                near=NEAR, far=FAR, confidence=None, min_confidence=0.0, depth_std=None, max_std=INF, mutation=None) -> Grid:
    """Statement G.  depth fp32 [B, 1, H, W], K fp32 [B, 4], pose fp32 [B, 12] on the host -> ``Grid`` of [B, GY, GX] / [B, GX]."""
    assert depth.dtype == F32 and K.dtype == F32 and pose.dtype == F32 and mutation in (None,) + MUTATIONS
    B = depth.shape[0]
    GX, GY = spec.GX, spec.GY
    n = GX * GY
    kept = keep(depth, K, pose, stride, near, far, confidence, min_confidence, depth_std, max_std)
    member, cell, g2 = membership(depth, K, pose, spec, band, F32, mutation)
    member = member & kept
    oh = _s(obstacle_height, F32)
    out = {name: [] for name in OUTPUTS}
    for b in range(B):
        idx = cell[b][member[b]]
        h = g2[b][member[b]]
        count = torch.bincount(idx, minlength=n)
        tall = (h >= oh) if mutation == "obstacle_ge" else (h > oh)
        obstacle = torch.bincount(idx[tall], minlength=n)
        q = torch.round(h * _s(1024.0, F32)).to(torch.int64)                  # round: half to even = rintf; exact for |h| <= 1000
        total = torch.zeros(n, dtype=torch.int64).index_add_(0, idx, q)
        h_min = torch.zeros(n, dtype=F32).scatter_reduce_(0, idx, h, "amin", include_self=False)
        h_max = torch.zeros(n, dtype=F32).scatter_reduce_(0, idx, h, "amax", include_self=False)
        filled = count > 0
        h_mean = torch.where(filled, total.double() / (1024.0 * count.clamp_min(1).double()), torch.zeros(n, dtype=F64)).to(F32)
        state = torch.where(count < min_points, 0, torch.where(obstacle >= min_obstacle_points, 2, 1)).to(torch.uint8)
        occupied = (state == 2).view(GY, GX)
        iy = torch.where(occupied, torch.arange(GY).view(GY, 1).expand(GY, GX), torch.full((GY, GX), GY)).amin(0)
        first = _s(spec.y0, F32) + iy.to(F32) * _s(spec.cell, F32)           # two roundings
        first = torch.where(iy < GY, first, torch.full_like(first, INF))
        for name, v in (("count", count.to(torch.int32).view(GY, GX)), ("obstacle", obstacle.to(torch.int32).view(GY, GX)),
                        ("h_min", h_min.view(GY, GX)), ("h_max", h_max.view(GY, GX)), ("h_mean", h_mean.view(GY, GX)),
                        ("state", state.view(GY, GX)), ("first_occupied", first)):
            out[name].append(v)
    return Grid(*(torch.stack(out[name], 0) for name in OUTPUTS))


def membership_gap(depth, K, pose, spec: Spec, band, **keep_options):
    """(kept points whose cell or band membership differs between the fp32 statement and float64, kept points)."""
    kept = keep(depth, K, pose, **keep_options)
    m32, c32, _ = membership(depth, K, pose, spec, band, F32)
    m64, c64, _ = membership(depth, K, pose, spec, band, F64)
    differ = ((m32 != m64) | (m32 & m64 & (c32 != c64))) & kept
    return int(differ.sum()), int(kept.sum())


def changed_cells(a: Grid, b: Grid):
    """(cells that are non-empty in ``a`` or ``b`` and differ in count, obstacle or state, cells non-empty in ``a``)."""
    filled = (a.count > 0) | (b.count > 0)
    differ = (a.count != b.count) | (a.obstacle != b.obstacle) | (a.state != b.state)
    return int((differ & filled).sum()), int((a.count > 0).sum())


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def intrinsics(H: int, W: int, B: int = CASE_B) -> torch.Tensor:
    """fp32 [B, 4]: a wide lens whatever the map's size (fx = W / 2: the small maps still see ground, wall and sky), fx != fy, the
    principal point off the centre and different per image."""
    rows = [[0.5 * W + 0.37 * b, 0.45 * W - 0.21 * b, (W - 1) / 2.0 + 1.25 - 0.75 * b, (H - 1) / 2.0 - 0.75 + 0.5 * b] for b in range(B)]
    return torch.tensor(rows, dtype=F32)


def rays(H: int, W: int, k: torch.Tensor) -> torch.Tensor:
    """fp64 [3, H, W]: (rx, ry, 1) of camera k [4]."""
    fx, fy, cx, cy = (float(v) for v in k.double())
    x = torch.arange(W, dtype=F64).view(1, W).expand(H, W)
    y = torch.arange(H, dtype=F64).view(H, 1).expand(H, W)
    return torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones(H, W, dtype=F64)], 0)


def flat_ground(H: int, W: int, k: torch.Tensor, P: torch.Tensor, sky: float = INF) -> torch.Tensor:
    """fp64 [H, W]: the depth of the plane height = 0 seen by camera k through pose P [3, 4]: z = -t_2 / (R_row2 . (rx, ry, 1)) where that
    is positive, ``sky`` elsewhere."""
    d = (P[2, :3].view(3, 1, 1) * rays(H, W, k)).sum(0)
    z = -P[2, 3] / d
    return torch.where((d < 0) & (z > 0), z, torch.full_like(z, sky))


def ground_with_slab(H: int, W: int, k: torch.Tensor, P: torch.Tensor, forward: float, top: float) -> torch.Tensor:
    """fp32 [H, W]: flat ground, and across the columns [W / 3, W / 2) a slab facing the camera: the plane ground-y = ``forward`` from
    the ground up to ``top`` metres, where a ray meets it in front of the ground."""
    r = rays(H, W, k)
    z = flat_ground(H, W, k, P)
    d1 = (P[1, :3].view(3, 1, 1) * r).sum(0)
    zs = forward / d1
    hs = (P[2, :3].view(3, 1, 1) * r).sum(0) * zs + P[2, 3]
    cols = torch.zeros(H, W, dtype=torch.bool)
    cols[:, W // 3:max(W // 2, W // 3 + 1)] = True
    hit = cols & (d1 > 0) & (hs >= 0) & (hs <= top) & (zs < z)
    return torch.where(hit, zs, z).float()


def sprinkle(z: torch.Tensor, seed: int) -> torch.Tensor:
    """A copy of z [H, W] with a few cells NaN, +inf, -inf, below NEAR (0.2) and above FAR (40.0)."""
    g = torch.Generator().manual_seed(seed)
    out = z.clone()
    H, W = z.shape
    n = max(1, H * W // 300)
    for v in (float("nan"), INF, -INF, 0.2, 40.0):
        out.view(-1)[torch.randint(0, H * W, (n,), generator=g)] = v
    return out


def wall(H: int, W: int, distance: float = 4.0) -> torch.Tensor:
    """fp32 [H, W]: a fronto-parallel wall: every pixel at the same depth, whole pixel columns and long runs of a row in one cell."""
    return torch.full((H, W), distance, dtype=F32)


def case(H: int, W: int, bad: int = None, kind: str = "camera", seed: int = 0, B: int = CASE_B) -> Case:
    """depth fp32 [3, 1, H, W], K fp32 [3, 4], pose fp32 [3, 12] and the options the case is evaluated with.  Image 0: flat ground seen
    from the posed camera with a slab obstacle 6 m ahead; image 1: a model-like map (around 2.5 m) sprinkled with NaN, +-inf and
    out-of-range cells; image 2: a wall at 4 m.  ``bad``: the image whose fx is NaN (kind "camera") or whose pose holds an inf (kind
    "pose").  The band's upper edge and the obstacle height are PLANTED on the wall: they are the fp32 heights (this statement's g_2) of
    two of its pixels, so one point lies exactly on either threshold -- inclusive and exclusive comparisons differ on these cases."""
    K = intrinsics(H, W, B)
    P = pose_matrix()
    pose = P.reshape(1, 12).float().expand(B, 12).contiguous()
    z2 = wall(H, W)
    g2 = ground_points(z2.view(1, 1, H, W), K[2:3], pose[2:3])[2][0]
    hi = float(g2[(g2[:, W // 2] - 2.5).abs().argmin(), W // 2])               # the pixels of two columns nearest to the defaults 2.5 / 0.3
    oh = float(g2[(g2[:, W // 3] - 0.3).abs().argmin(), W // 3])
    assert BAND_LO < oh < hi <= 1000.0
    z0 = ground_with_slab(H, W, K[0], P, forward=6.0, top=oh + 0.6)
    z1 = sprinkle(normals_ref.model_like(H, W, 11 + seed), 5 + seed)
    if bad is not None:
        if kind == "camera":
            K[bad, 0] = float("nan")
        else:
            pose[bad, 7] = INF
    return Case(torch.stack([z0, z1, z2], 0).unsqueeze(1).contiguous(), K, pose, {"band": (BAND_LO, hi), "obstacle_height": oh})


def confidence_map(H: int, W: int, seed: int = 3, B: int = CASE_B) -> torch.Tensor:
    """fp32 [B, 1, H, W] in [0, 1) with a few NaN: about half of the pixels pass a threshold of 0.5."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand((B, 1, H, W), generator=g, dtype=F32)
    c.view(-1)[torch.randint(0, c.numel(), (max(1, c.numel() // 200),), generator=g)] = float("nan")
    return c
