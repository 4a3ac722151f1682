"""Block-local float64 shadow of an EfficientNet encoder (tests/test_hip_encoder_blocks.py, tests/test_encoder_blocks_host.py).

``Shadow(backbone)`` keeps a float64 CPU copy of the backbone.  Inside ``with shadow:`` a forward hook on every block -- the B
family's DepthwiseSeparableConv / InvertedResidual and conv_head, V2's FusedMBConv / MBConv and its stem and head
Conv2dNormActivation -- takes images {0, B // 2, B - 1} of the block's own input, runs the float64 copy of that block on them
(its plain PyTorch path: unfolded BatchNorm, no HIP kernel) and records util.branch_dev of the block's output against it, per
image.  Each block is checked on its own input, so the deviation is that block's alone: nothing accumulates from the blocks in
front of it.  ``check_stem`` does the same for the B family's stem (conv_stem + bn1 + act1), which the GPU path runs as one
fused launch with no module call to hook."""
import copy
from collections import Counter

import torch

from objcavit_amd.modules.efficientnet import DepthwiseSeparableConv, InvertedResidual
from objcavit_amd.modules.efficientnet_v2 import EfficientNetV2, FusedMBConv, MBConv
from util import branch_dev

BLOCKS = (DepthwiseSeparableConv, InvertedResidual, FusedMBConv, MBConv)


def sample_images(B):
    return sorted({0, B // 2, B - 1})


def is_residual(mod):
    return bool(getattr(mod, "has_residual", False) or getattr(mod, "use_res_connect", False))


def shadowed(backbone):
    """[(name, module)] in forward order: V2's stem, every block, then V2's head or the B family's conv_head.  Names are the
    state_dict paths inside the backbone (``blocks.<stage>.<index>``, ``features.<stage>.<index>``)."""
    v2 = isinstance(backbone, EfficientNetV2)
    out = [("features.0", backbone.features[0])] if v2 else []
    out += [(n, m) for n, m in backbone.named_modules() if isinstance(m, BLOCKS)]
    out.append((f"features.{len(backbone.features) - 1}", backbone.features[-1]) if v2 else ("conv_head", backbone.conv_head))
    return out


class Shadow:
    """Hooks and records; ``records``: one dict per block call (name, kind, residual, images, devs, in / out shape);
    ``current``: the name of the block whose forward is running (None between blocks)."""

    def __init__(self, backbone):
        self.ref = copy.deepcopy(backbone).to("cpu", torch.float64)
        refs = dict(self.ref.named_modules())
        self.targets = [(n, m, refs[n]) for n, m in shadowed(backbone)]
        self.records = []
        self.current = None
        self._handles = []

    def __enter__(self):
        for name, mod, ref in self.targets:
            self._handles.append(mod.register_forward_pre_hook(lambda m, a, _n=name: self._enter(_n)))
            self._handles.append(mod.register_forward_hook(lambda m, a, y, _n=name, _r=ref: self._check(_n, _r, m, a[0], y)))
        return self

    def __exit__(self, *exc):
        for h in self._handles:
            h.remove()
        self._handles = []
        self.current = None

    def _enter(self, name):
        self.current = name

    def _record(self, name, kind, res, idx, x_shape, y, ref, xi):
        self.records.append(dict(name=name, kind=kind, residual=res, images=idx, in_shape=tuple(x_shape),
                                 out_shape=tuple(y.shape), devs=branch_dev(y[idx], ref, xi if res else None)))

    def _check(self, name, ref, mod, x, y):
        idx = sample_images(x.shape[0])
        xi = x[idx].detach().to("cpu", torch.float64).contiguous()
        with torch.no_grad():
            r = ref(xi)
        self._record(name, type(mod).__name__, is_residual(mod), idx, x.shape, y, r, xi)
        self.current = None

    def check_stem(self, img, y):
        """The B family's stem output ``y`` (the Encoder's pushed activation 3) against conv_stem + bn1 + act1 in float64."""
        idx = sample_images(img.shape[0])
        xi = img[idx].detach().to("cpu", torch.float64).contiguous()
        with torch.no_grad():
            r = self.ref.act1(self.ref.bn1(self.ref.conv_stem(xi)))
        self._record("stem", "stem", False, idx, img.shape, y, r, xi)

    def visits(self):
        return Counter(r["name"] for r in self.records)

    def failures(self, bar, route_of=None):
        """[(dev, name, route, image)] of every (block, image) above ``bar``, worst first."""
        bad = [(d, r["name"], route_of(r["name"]) if route_of else r["kind"], i)
               for r in self.records for i, d in zip(r["images"], r["devs"]) if not d <= bar]
        return sorted(bad, reverse=True)
