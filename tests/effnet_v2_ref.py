"""Functional float64 restatement of torchvision's EfficientNetV2-S / -M ``features`` (test infrastructure).

Written from the architecture table alone (objcavit_amd/modules/efficientnet_v2.py header; torchvision 0.13.1): F.conv2d with
explicit symmetric padding (k - 1) // 2, BatchNorm in eval form (eps 1e-3), SiLU, squeeze-excite (mean, fc1, SiLU, fc2,
sigmoid), residual where stride 1 and widths equal.  Weights are read by torchvision key from a state dict; no module's
``forward`` is called.  ``features`` returns [x, features.0 output, ..., features.-1 output] -- what the reference's Encoder
collects before its two Identity children."""
import torch
import torch.nn.functional as F

EPS = 1e-3
STAGES = {
    "s": (("fused", 1, 3, 1, 24, 24, 2), ("fused", 4, 3, 2, 24, 48, 4), ("fused", 4, 3, 2, 48, 64, 4),
          ("mb", 4, 3, 2, 64, 128, 6), ("mb", 6, 3, 1, 128, 160, 9), ("mb", 6, 3, 2, 160, 256, 15)),
    "m": (("fused", 1, 3, 1, 24, 24, 3), ("fused", 4, 3, 2, 24, 48, 5), ("fused", 4, 3, 2, 48, 80, 5),
          ("mb", 4, 3, 2, 80, 160, 7), ("mb", 6, 3, 1, 160, 176, 14), ("mb", 6, 3, 2, 176, 304, 18),
          ("mb", 6, 3, 1, 304, 512, 5)),
}


def _cna(x, sd, p, stride=1, groups=1, act=True):
    """Conv2dNormActivation at key prefix p: p.0 conv (no bias), p.1 BatchNorm2d, SiLU."""
    w = sd[p + "0.weight"].double()
    k = w.shape[-1]
    y = F.conv2d(x, w, None, stride, (k - 1) // 2, 1, groups)
    g, b, m, v = (sd[p + "1." + n].double() for n in ("weight", "bias", "running_mean", "running_var"))
    y = (y - m.view(1, -1, 1, 1)) / torch.sqrt(v.view(1, -1, 1, 1) + EPS) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    return F.silu(y) if act else y


def _se(x, sd, p):
    s = x.mean((2, 3), keepdim=True)
    s = F.silu(F.conv2d(s, sd[p + "fc1.weight"].double(), sd[p + "fc1.bias"].double()))
    s = F.conv2d(s, sd[p + "fc2.weight"].double(), sd[p + "fc2.bias"].double())
    return x * torch.sigmoid(s)


def features(img, sd, variant, prefix=""):
    x = img.double()
    out = [x]
    x = _cna(x, sd, prefix + "features.0.", stride=2)
    out.append(x)
    for si, (kind, e, k, s, cin, cout, reps) in enumerate(STAGES[variant]):
        for r in range(reps):
            p = f"{prefix}features.{si + 1}.{r}.block."
            stride, ci = (s, cin) if r == 0 else (1, cout)
            if kind == "fused":
                if e == 1:
                    y = _cna(x, sd, p + "0.", stride)
                else:
                    y = _cna(_cna(x, sd, p + "0.", stride), sd, p + "1.", act=False)
            else:
                mid = ci * e
                y = _cna(x, sd, p + "0.")
                y = _cna(y, sd, p + "1.", stride, groups=mid)
                y = _se(y, sd, p + "2.")
                y = _cna(y, sd, p + "3.", act=False)
            x = y + x if stride == 1 and ci == cout else y
        out.append(x)
    x = _cna(x, sd, f"{prefix}features.{len(STAGES[variant]) + 1}.")
    out.append(x)
    return out
