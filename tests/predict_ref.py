"""Reference statements of the predict path's two ends, in torch on the CPU.  The reference's own ``Preprocess`` / ``Normalize``
classes cannot be imported here (kornia and torchvision are absent), so this end is restated by formula with the lines cited."""
from __future__ import annotations

from typing import Optional

import torch

from oracle import validation_ref

MEAN = [0.485, 0.456, 0.406]          # modules/GraphBinsLM.py:45 (ImageNet statistics)
STD = [0.229, 0.224, 0.225]


def image_norm_factor(args) -> float:
    """params/basicParams.yaml:117,144: 255 in both dataset blocks (a config made by config.make_args carries no such key)."""
    return float(args[args.basic.dataset].get("image_norm_factor", 255.0))


def frames_to_input(frames_u8: torch.Tensor, args, top: int, left: int, H: int, W: int) -> torch.Tensor:
    """uint8 [B, Hs, Ws, 3] -> fp32 [B, 3, H, W], in the reference's operation order:
    modules/Preprocess.py:85-87   np.asarray(image, float32) -> CHW tensor -> image /= factor
    modules/Preprocess.py:104-107 image[:, top:top + H, left:left + W]           (the KITTI benchmark crop; any window here)
    modules/GraphBinsLM.py:45,443 torchvision Normalize: tensor.sub_(mean[:, None, None]).div_(std[:, None, None]), fp32"""
    x = frames_u8.cpu().to(torch.float32).permute(0, 3, 1, 2).contiguous()
    x = x / image_norm_factor(args)
    x = x[:, :, top:top + H, left:left + W]
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
    return ((x - mean) / std).contiguous()


def depth_to_metres(depth_u16: torch.Tensor, factor: float, top: int, left: int, H: int, W: int) -> torch.Tensor:
    """modules/Preprocess.py:61-64 (float32 array, /= factor) and the crop of :109: uint16 [B, Hs, Ws] -> fp32 [B, 1, H, W]."""
    d = depth_u16.cpu().to(torch.int32).to(torch.float32) / factor
    return d[:, top:top + H, left:left + W].unsqueeze(1).contiguous()


def final_depth(pred: torch.Tensor, mirror: Optional[torch.Tensor], min_depth: float, max_depth: float, H: int, W: int,
                dtype=torch.float32) -> torch.Tensor:
    """modules/GraphBinsLM.py:159-183 (flip-TTA average of the clamped maps; :295-301 without a mirror: the clamp alone) followed by
    metrics/MetricsPreprocess.py:17-24 (bilinear align_corners resize, nan -> min_depth, +-inf -> max_depth), in ``dtype``."""
    p = pred.cpu().to(dtype)
    if mirror is not None:
        p = validation_ref.tta_average(p, mirror.cpu().to(dtype), min_depth, max_depth)
    else:
        p = torch.clamp(p, min=min_depth, max=max_depth)
    out, _ = validation_ref.metrics_preprocess(p, torch.ones(p.shape[0], 1, H, W, dtype=dtype), min_depth, max_depth)
    return out


def to_u16(depth: torch.Tensor, scale: float) -> torch.Tensor:
    """The datasets' 16-bit PNG convention (x 1000 NYU, x 256 KITTI): min(65535, rint(depth * scale)) in fp32, ties to even
    (torch.round); -> int32 values in 0 .. 65535."""
    v = torch.round(depth.cpu().to(torch.float32) * torch.tensor(scale, dtype=torch.float32))
    return v.clamp(min=0.0, max=65535.0).to(torch.int32)


def to_rgb8(depth: torch.Tensor, table: torch.Tensor, vmin: float, vmax: float) -> torch.Tensor:
    """matplotlib's Normalize(vmin, vmax) + colormap call as modules/GraphBinsLM.py:367 uses it, in fp32: the colormap turns a
    normalised x into row int(x * 256), 256 -> 255, below 0 -> the first colour, above -> the last (no set_under / set_over on the
    prediction's map).  Here: row clamp(floor((depth - vmin) * s), 0, 255) with s = 256 / (vmax - vmin) in fp32.
    depth [..., H, W] -> uint8 [..., H, W, 3]."""
    lo, hi = torch.tensor(vmin, dtype=torch.float32), torch.tensor(vmax, dtype=torch.float32)
    s = torch.tensor(256.0, dtype=torch.float32) / (hi - lo)
    idx = torch.floor((depth.cpu().to(torch.float32) - lo) * s).clamp(min=0.0, max=255.0).to(torch.int64)
    return table.cpu()[idx]
