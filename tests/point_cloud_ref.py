"""The torch-CPU statement of the point-cloud output (include/objcavit_hip.h, ocv_depth_unproject_fwd): a boolean mask, ``nonzero``
order, and the fp32 statements in the order the definition gives them.  The tests compare the int32 views of the kernel's outputs with
this, bit for bit; ``float64_gap`` is the self-check of THIS file against a float64 pinhole computation."""
from collections import namedtuple
from typing import List, Optional, Tuple

import torch

F32 = torch.float32
Cloud = namedtuple("Cloud", ["records", "pixel"])          # per image: fp32 [n, 4] (16-byte records), int32 [n] = y * W + x; n = total


def _f32(v) -> torch.Tensor:
    return torch.tensor(float(v), dtype=F32)


def shift_intrinsics(K: torch.Tensor, top: int, left: int) -> torch.Tensor:
    """fp32 cx - left, cy - top: the statement ``objcavit_amd.point_cloud.shift_intrinsics`` makes on the device."""
    return K.to(F32) - torch.tensor([0.0, 0.0, float(left), float(top)], dtype=F32)


def keep_mask(depth: torch.Tensor, k: torch.Tensor, stride=(1, 1), near=0.0, far=float("inf"), confidence=None, min_confidence=0.0,
              depth_std=None, max_std=float("inf")) -> torch.Tensor:
    """bool [H, W] of one image: ``depth`` / ``confidence`` / ``depth_std`` [H, W] fp32, ``k`` [4]."""
    H, W = depth.shape
    sy, sx = stride
    m = ((torch.arange(H) % sy) == 0).view(H, 1) & ((torch.arange(W) % sx) == 0).view(1, W)
    m = m & torch.isfinite(depth) & (depth >= _f32(near)) & (depth <= _f32(far))
    if confidence is not None:
        m = m & (confidence >= _f32(min_confidence))          # NaN compares false
    if depth_std is not None:
        m = m & (depth_std <= _f32(max_std))
    fx, fy, cx, cy = (k[i] for i in range(4))
    camera = bool(torch.isfinite(k).all()) and bool(fx > 0) and bool(fy > 0)
    return m if camera else torch.zeros_like(m)


def unproject(depth: torch.Tensor, K: torch.Tensor, stride=(1, 1), near=0.0, far=float("inf"), confidence=None, min_confidence=0.0,
              depth_std=None, max_std=float("inf"), frames=None, top: int = 0, left: int = 0) -> List[Cloud]:
    """Per image the FULL cloud (every kept pixel, in row-major order): depth / confidence / depth_std fp32 [B, 1, H, W], K fp32 [B, 4],
    frames uint8 [B, Hs, Ws, 3] (any strides).  A caller with a capacity compares the first ``cap`` rows."""
    depth, K = depth.to(F32), K.to(F32)
    B, _, H, W = depth.shape
    out = []
    for b in range(B):
        z_map = depth[b, 0]
        conf = None if confidence is None else confidence[b, 0]
        m = keep_mask(z_map, K[b], stride, near, far, conf, min_confidence, None if depth_std is None else depth_std[b, 0], max_std)
        idx = m.reshape(-1).nonzero().flatten()               # ascending = row-major (y, x)
        y, x = idx // W, idx % W
        z = z_map.reshape(-1)[idx]
        fx, fy, cx, cy = (K[b, i] for i in range(4))
        rx = (x.to(F32) - cx) / fx                            # every statement an fp32 op of its own
        ry = (y.to(F32) - cy) / fy
        rec = torch.zeros(idx.numel(), 4, dtype=F32)
        rec[:, 0], rec[:, 1], rec[:, 2] = rx * z, ry * z, z
        by = rec.view(torch.uint8)                            # [n, 16]
        if frames is not None:
            by[:, 12:15] = frames[b][top + y, left + x]
        if conf is None:
            by[:, 15] = 255
        else:
            by[:, 15] = torch.round(_f32(255.0) * conf.reshape(-1)[idx].clamp(0.0, 1.0)).to(torch.uint8)      # round: half to even
        out.append(Cloud(rec, idx.to(torch.int32)))
    return out


def float64_gap(depth: torch.Tensor, K: torch.Tensor, clouds: List[Cloud]) -> float:
    """max over every point and X, Y of |fp32 - float64| / |float64| (0 where the float64 value is 0), the float64 value being
    (x - cx) / fx * z with the fp32 INPUTS taken exactly."""
    W = depth.shape[-1]
    worst = 0.0
    for b, c in enumerate(clouds):
        idx = c.pixel.long()
        y, x = (idx // W).double(), (idx % W).double()
        z = depth[b, 0].reshape(-1)[idx].double()
        k = K[b].double()
        want = torch.stack([(x - k[2]) / k[0] * z, (y - k[3]) / k[1] * z], 1)
        got = c.records[:, :2].double()
        rel = torch.where(want != 0, (got - want).abs() / want.abs(), (got != 0).double())
        worst = max(worst, float(rel.max()) if rel.numel() else 0.0)
    return worst


# ---------------------------------------------------------------------------
# the cases of tests/test_hip_point_cloud.py (made once, never changed)
# ---------------------------------------------------------------------------
CASE_B, CASE_H, CASE_W = 3, 61, 83          # odd, W % 4 != 0; 5063 candidates = 2 full tiles of 2048 + 967
TILE = 2048
NEAR, FAR, OUTSIDE = 0.5, 10.0, 20.0        # masks are made by setting depth OUTSIDE [NEAR, FAR]
MASKS = ("all", "none", "checkerboard", "random_half", "first_pixel", "last_tile", "tile_boundaries")


def case_intrinsics(B: int = CASE_B) -> torch.Tensor:
    """A different camera per image, none symmetric (fx != fy, the principal point off the centre and not on a pixel)."""
    return torch.tensor([[70.3 + 11.0 * b, 64.9 - 3.0 * b, 40.7 + b, 29.2 - 2.0 * b] for b in range(B)], dtype=F32)


def case_depth(mask: str, seed: int = 0, B: int = CASE_B, H: int = CASE_H, W: int = CASE_W) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 + seed)
    z = torch.rand(B, 1, H, W, generator=g) * 8.0 + 1.0
    flat = torch.arange(H * W).view(H, W)
    yy, xx = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    if mask == "all":
        keep = torch.ones(H, W, dtype=torch.bool)
    elif mask == "none":
        keep = torch.zeros(H, W, dtype=torch.bool)
    elif mask == "checkerboard":
        keep = ((yy + xx) % 2) == 0
    elif mask == "random_half":
        keep = torch.rand(H, W, generator=g) < 0.5
    elif mask == "first_pixel":
        keep = flat == 0
    elif mask == "last_tile":
        keep = flat >= 2 * TILE
    elif mask == "tile_boundaries":          # runs over the ends of tiles 0 and 1, of a wave (64) and of a round (256) inside a tile
        keep = ((flat >= TILE - 9) & (flat < TILE + 7)) | ((flat >= 2 * TILE - 3) & (flat < 2 * TILE + 70)) | ((flat >= 250) & (flat < 262))
    else:
        raise KeyError(mask)
    z[:, 0][:, ~keep] = OUTSIDE
    return z


def case_frames(seed: int, B: int, Hs: int, Ws: int) -> torch.Tensor:
    return torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(200 + seed))


def case_confidence(seed: int = 0, B: int = CASE_B, H: int = CASE_H, W: int = CASE_W, threshold: float = 0.25) -> torch.Tensor:
    """In [-0.1, 1.1] (the clamp has work to do), with NaNs, values exactly AT the threshold, and exact 0.5 (255 * 0.5 = 127.5 -> 128)."""
    g = torch.Generator().manual_seed(300 + seed)
    c = torch.rand(B, 1, H, W, generator=g) * 1.2 - 0.1
    c[:, :, 3::7, 2::5] = float("nan")
    c[:, :, 1::6, 1::4] = threshold
    c[:, :, 2::9, 0::3] = 0.5
    return c


def case_std(seed: int = 0, B: int = CASE_B, H: int = CASE_H, W: int = CASE_W, threshold: float = 0.75) -> torch.Tensor:
    g = torch.Generator().manual_seed(400 + seed)
    s = torch.rand(B, 1, H, W, generator=g) * 1.5
    s[:, :, 4::8, 3::6] = float("nan")
    s[:, :, 0::5, 2::7] = threshold
    return s
