"""Statement N (include/objcavit_hip.h) in torch on the CPU: the surface normals csrc/surface_normals.hip is compared with.

VALIDITY is evaluated in fp32, one torch op per statement (a comparison, a subtraction, a product: each rounded on its own, as the
kernel's), so it is the kernel's bit for bit.  SLOPES and the NORMAL are evaluated in fp64 from the fp32 map, differences first.
``mutation`` plants one deliberate error (tests/test_normals_host.py shows each of them moves the normals by far more than the bar the
kernel is held to).  The generators make the maps the tests run on; everything is seeded and made on the host."""
from collections import namedtuple

import torch
import torch.nn.functional as F

NEAR, FAR, EDGE = 0.5, 10.0, 0.05
RADII = (1, 2, 3, 4)
MUTATIONS = ("radius", "weights", "offset", "swap_f")
CASE_B = 3
CASE_SHAPES = ((8, 8), (9, 9), (19, 70), (37, 131))          # no pixel at r = 4; exactly one; 2 x 2 tiles; 3 x 3 tiles, the last three columns wide
VECTOR_SHAPES = ((21, 132),)                                 # W % 4 == 0 over 2 x 3 tiles: the kernel's wide stores (8 x 8 takes them too)

Normals = namedtuple("Normals", ["normals", "valid", "rgb8"])      # fp64 [B, 3, H, W], bool [B, H, W], uint8 [B, H, W, 3]


def camera_ok(K: torch.Tensor) -> torch.Tensor:
    """bool [B]: fx, fy finite and > 0, cx, cy finite."""
    K = K.float()
    return torch.isfinite(K).all(1) & (K[:, 0] > 0) & (K[:, 1] > 0)


def window_extremes(depth: torch.Tensor, r: int):
    """fp32 maps of the INTERIOR [B, H - 2r, W - 2r] (or None when the map has none): (all finite in the window, the window's min, max
    over its finite cells, the centre)."""
    z = depth[:, 0].float()
    B, H, W = z.shape
    if H <= 2 * r or W <= 2 * r:
        return None
    k = 2 * r + 1
    fin = torch.isfinite(z)
    bad = F.max_pool2d((~fin).float().unsqueeze(1), k, stride=1)[:, 0] > 0
    lo = -F.max_pool2d(torch.where(fin, -z, torch.full_like(z, float("-inf"))).unsqueeze(1), k, stride=1)[:, 0]
    hi = F.max_pool2d(torch.where(fin, z, torch.full_like(z, float("-inf"))).unsqueeze(1), k, stride=1)[:, 0]
    return ~bad, lo, hi, z[:, r:H - r, r:W - r]


def validity(depth: torch.Tensor, K: torch.Tensor, r: int, near: float, far: float, edge_ratio: float) -> torch.Tensor:
    """bool [B, H, W], every operation in fp32."""
    B, _, H, W = depth.shape
    valid = torch.zeros((B, H, W), dtype=torch.bool)
    w = window_extremes(depth, r)
    if w is None:
        return valid
    fin, lo, hi, zc = w
    near32, far32, edge32 = (torch.tensor(v, dtype=torch.float32) for v in (near, far, edge_ratio))
    t = edge32 * zc
    ok = fin & (near32 <= lo) & (hi <= far32) & ((hi - zc) <= t) & ((zc - lo) <= t)
    valid[:, r:H - r, r:W - r] = ok & camera_ok(K).view(B, 1, 1)
    return valid


def slopes(depth: torch.Tensor, r: int, unit_weights: bool = False):
    """fp64 (zu, zv) [B, H, W] of the interior (0 on the border and wherever a window holds a non-finite cell: masked by validity)."""
    z = torch.nan_to_num(depth[:, 0].double(), nan=0.0, posinf=0.0, neginf=0.0)
    B, H, W = z.shape
    zu, zv = torch.zeros_like(z), torch.zeros_like(z)
    if H <= 2 * r or W <= 2 * r:
        return zu, zv
    D = (2 * r + 1) * 2 * sum(i * i for i in range(1, r + 1))
    h, w = H - 2 * r, W - 2 * r
    su, sv = torch.zeros((B, h, w), dtype=torch.float64), torch.zeros((B, h, w), dtype=torch.float64)
    for j in range(-r, r + 1):
        for i in range(1, r + 1):
            wt = 1.0 if unit_weights else float(i)
            su += wt * (z[:, r + j:r + j + h, r + i:r + i + w] - z[:, r + j:r + j + h, r - i:r - i + w])
            sv += wt * (z[:, r + i:r + i + h, r + j:r + j + w] - z[:, r - i:r - i + h, r + j:r + j + w])
    zu[:, r:H - r, r:W - r] = su / D
    zv[:, r:H - r, r:W - r] = sv / D
    return zu, zv


def normals(depth: torch.Tensor, K: torch.Tensor, r: int, near: float = NEAR, far: float = FAR, edge_ratio: float = EDGE,
            mutation: str = None) -> Normals:
    """Statement N.  ``depth`` fp32 [B, 1, H, W], ``K`` fp32 [B, 4] on the host."""
    assert depth.dtype == torch.float32 and K.dtype == torch.float32 and mutation in (None,) + MUTATIONS
    B, _, H, W = depth.shape
    valid = validity(depth, K, r, near, far, edge_ratio)
    zu, zv = slopes(depth, r + 1 if mutation == "radius" else r, unit_weights=mutation == "weights")
    k = torch.nan_to_num(K.double(), nan=1.0, posinf=1.0, neginf=1.0)
    fx, fy, cx, cy = (k[:, i].view(B, 1, 1) for i in range(4))
    if mutation == "swap_f":
        fx, fy = fy, fx
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    zc = torch.nan_to_num(depth[:, 0].double(), nan=0.0, posinf=0.0, neginf=0.0)
    off = 0.0 if mutation == "offset" else (x - cx) * zu + (y - cy) * zv
    m = torch.stack([fx * zu, fy * zv, -(zc + off)], 1)
    length = m.norm(dim=1, keepdim=True)
    n = torch.where(length > 0, m / length.clamp_min(1e-300), torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).view(1, 3, 1, 1))
    n = n * valid.unsqueeze(1)
    rgb = torch.clamp(torch.round(127.5 * n + 127.5), 0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()      # round: ties to even = rint
    rgb = rgb * valid.unsqueeze(-1).to(torch.uint8)
    return Normals(n, valid, rgb)


def angle(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp64 [B, H, W]: the angle in radians between the vectors a, b [B, 3, H, W] (atan2 of |a x b| and a . b: exact for small angles)."""
    a, b = a.double(), b.double()
    return torch.atan2(torch.linalg.cross(a, b, dim=1).norm(dim=1), (a * b).sum(1))


def threshold_margin(depth: torch.Tensor, r: int, near: float = NEAR, far: float = FAR, edge_ratio: float = EDGE) -> float:
    """The smallest relative distance of any tested quantity of the map from its threshold (fp64): z from near and far, and, over the
    windows that are finite and in range, wmax - zc and zc - wmin from edge_ratio * zc."""
    z = depth[:, 0].double()
    zf = z[torch.isfinite(z)]
    out = min(float(((zf - near).abs() / abs(near)).min()), float(((zf - far).abs() / abs(far)).min()))
    w = window_extremes(depth, r)
    if w is not None:
        fin, lo, hi, zc = w
        ok = fin & (lo >= near) & (hi <= far)
        if bool(ok.any()):
            lo, hi, zc = lo.double()[ok], hi.double()[ok], zc.double()[ok]
            t = edge_ratio * zc
            out = min(out, float((((hi - zc) - t).abs() / t).min()), float((((zc - lo) - t).abs() / t).min()))
    return out


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def intrinsics(H: int, W: int, B: int = CASE_B) -> torch.Tensor:
    """fp32 [B, 4]: fx != fy, the principal point off the centre and different per image."""
    rows = [[518.8579 + 7.0 * b, 431.25 - 5.0 * b, (W - 1) / 2.0 + 3.25 - 2.0 * b, (H - 1) / 2.0 - 1.75 + 1.5 * b] for b in range(B)]
    return torch.tensor(rows, dtype=torch.float32)


def plane(H: int, W: int, a: float, b: float, c: float) -> torch.Tensor:
    """fp32 [H, W]: z = 1 / (a x + b y + c) in pixel coordinates -- an exact plane in space for every pinhole camera."""
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    return (1.0 / (a * x + b * y + c)).float()


def plane_normal(K: torch.Tensor, a: float, b: float, c: float) -> torch.Tensor:
    """fp64 [3]: the unit normal, pointing at the camera, of the plane ``plane(.., a, b, c)`` is seen as by camera K [4]: with
    x = fx X / Z + cx, y = fy Y / Z + cy the plane is  a fx X + b fy Y + (a cx + b cy + c) Z = 1."""
    fx, fy, cx, cy = (float(v) for v in K.double())
    n = torch.tensor([a * fx, b * fy, a * cx + b * cy + c], dtype=torch.float64)
    return -n / n.norm()


def sphere(H: int, W: int, K: torch.Tensor, centre=(0.05, -0.02, 2.5), radius: float = 0.4, background: float = 4.0) -> torch.Tensor:
    """fp32 [H, W]: the depth of a sphere in front of a wall at ``background`` metres, seen by camera K [4]."""
    fx, fy, cx, cy = (float(v) for v in K.double())
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    d = torch.stack([((x - cx) / fx).expand(H, W), ((y - cy) / fy).expand(H, W), torch.ones(H, W, dtype=torch.float64)], 0)      # z = 1 rays
    c = torch.tensor(centre, dtype=torch.float64).view(3, 1, 1)
    dd, dc = (d * d).sum(0), (d * c).sum(0)
    disc = dc * dc - dd * ((c * c).sum() - radius * radius)
    z = (dc - disc.clamp_min(0).sqrt()) / dd
    return torch.where(disc > 0, z, torch.full_like(z, background)).float()


def step(H: int, W: int, column: int, left: float = 2.0, right: float = 3.0) -> torch.Tensor:
    """fp32 [H, W]: two gently tilted planes, ``left`` metres up to ``column`` - 1 and ``right`` metres from ``column`` on: a depth
    discontinuity of (right - left) / left, within either side a range far below EDGE."""
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    tilt = 1.0 + 2e-4 * (x - W / 2) - 1.5e-4 * (y - H / 2)
    return (torch.where(x < column, torch.tensor(left, dtype=torch.float64), torch.tensor(right, dtype=torch.float64)) * tilt).float()


def model_like(H: int, W: int, seed: int, base: float = 2.5, amplitude: float = 0.025) -> torch.Tensor:
    """fp32 [H, W]: a bilinear align_corners enlargement (2x, cut to H x W) of random noise around ``base`` -- piecewise bilinear, the
    model's own kind of map; with EDGE = 0.05 some windows pass the discontinuity test and some do not."""
    g = torch.Generator().manual_seed(seed)
    h, w = (H + 1) // 2 + 1, (W + 1) // 2 + 1
    small = base * (1.0 + amplitude * torch.randn((1, 1, h, w), generator=g, dtype=torch.float32))
    return F.interpolate(small, size=(2 * h, 2 * w), mode="bilinear", align_corners=True)[0, 0, :H, :W].contiguous()


def sprinkle(z: torch.Tensor, seed: int) -> torch.Tensor:
    """A copy of z [H, W] with a few cells NaN, +inf, -inf, below NEAR (0.2) and above FAR (12.0): far from either threshold."""
    g = torch.Generator().manual_seed(seed)
    out = z.clone()
    H, W = z.shape
    n = max(1, H * W // 600)
    for v in (float("nan"), float("inf"), float("-inf"), 0.2, 12.0):
        idx = torch.randint(0, H * W, (n,), generator=g)
        out.view(-1)[idx] = v
    return out


def case(H: int, W: int, bad_camera: int = None, seed: int = 0):
    """(depth fp32 [3, 1, H, W], K fp32 [3, 4]): image 0 a tilted plane (from 32 columns on: with a step at column W // 2 + 3), image 1 a
    model-like map with sprinkled NaN / inf / out-of-range cells (none below 16 x 16: the map stays whole), image 2 a sphere in front of
    a wall.  ``bad_camera``: the image whose fx is NaN."""
    K = intrinsics(H, W)
    z0 = step(H, W, W // 2 + 3) if W >= 32 else plane(H, W, 3e-4, -2e-4, 0.4)
    z1 = model_like(H, W, 11 + seed)
    if H >= 16 and W >= 16:
        z1 = sprinkle(z1, 5 + seed)
    z2 = sphere(H, W, K[2], radius=0.4 if W >= 32 else 0.004)
    if bad_camera is not None:
        K[bad_camera, 0] = float("nan")
    return torch.stack([z0, z1, z2], 0).unsqueeze(1).contiguous(), K
