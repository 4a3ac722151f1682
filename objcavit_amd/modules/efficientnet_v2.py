"""EfficientNetV2-S / -M backbones in torchvision's layout (torchvision 0.13.1 ``models.efficientnet_v2_{s,m}``).

The reference builds these with ``torchvision.models.efficientnet_v2_{s,m}(weights="IMAGENET1K_V1")``
(modules/DenseFeatureExtractor.py:159-166) and replaces ``avgpool`` / ``classifier`` by Identity.  Here the
architecture is local: children (features, avgpool, classifier), child order and state_dict keys equal torchvision's,
so a reference checkpoint (``...encoder.original_model.features.3.1.block.0.0.weight`` ...) loads with strict=True.

Layout (block type, expand, kernel, stride, in -> out, repeats):

    stage   V2-S                        V2-M
    1       Fused 1, 3, 1, 24->24,  x2  Fused 1, 3, 1, 24->24,  x3
    2       Fused 4, 3, 2, 24->48,  x4  Fused 4, 3, 2, 24->48,  x5
    3       Fused 4, 3, 2, 48->64,  x4  Fused 4, 3, 2, 48->80,  x5
    4       MBConv 4, 3, 2, 64->128, x6  MBConv 4, 3, 2, 80->160, x7
    5       MBConv 6, 3, 1, 128->160, x9 MBConv 6, 3, 1, 160->176, x14
    6       MBConv 6, 3, 2, 160->256, x15 MBConv 6, 3, 2, 176->304, x18
    7       --                          MBConv 6, 3, 1, 304->512, x5

features[0] is the stem (3x3 stride 2, 3 -> 24, BN, SiLU), features[-1] the head (1x1 -> 1280, BN, SiLU).  Every BN has
eps 1e-3; every convolution pads symmetrically by (k - 1) // 2 -- NOT TF "SAME" as the B family does (on an even input a
stride-2 3x3 layer pads 1 on both sides here, 0 on top / 1 at the bottom there).  StochasticDepth and Dropout are
identities in eval.

Inference plan on the GPU (eval + no_grad): BN folded once per parameter version (_FoldedMixin); stem on csrc/stem.hip
with padding (1, 1); a Fused-MBConv's 3x3 on the implicit GEMM at stride 1 or 2 (csrc/conv_igemm.hip,
ocv_conv3x3_nhwc_strided_fwd; SiLU and, for expand 1, the residual in its epilogue) and its 1x1 project on the pointwise
kernel (residual in its epilogue); MBConv blocks on the B family's plan (efficientnet.mbconv_plan: mbconv_fused /
depthwise_se / pointwise_split) with explicit padding; the head on the pointwise kernel with SiLU.  Nothing of the
encoder reaches MIOpen / hipBLASLt / ATen convolution; a shape no kernel takes raises HipLibraryError.  On the CPU or in
training the plain module graph runs.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import hip_ops
from .efficientnet import _FoldedMixin, _dw_tap_major, fold_bn, mbconv_plan

BN_EPS = 1e-3

# (block, expand, kernel, stride, cin, cout, repeats)
V2_S_STAGES = (("fused", 1, 3, 1, 24, 24, 2), ("fused", 4, 3, 2, 24, 48, 4), ("fused", 4, 3, 2, 48, 64, 4),
               ("mb", 4, 3, 2, 64, 128, 6), ("mb", 6, 3, 1, 128, 160, 9), ("mb", 6, 3, 2, 160, 256, 15))
V2_M_STAGES = (("fused", 1, 3, 1, 24, 24, 3), ("fused", 4, 3, 2, 24, 48, 5), ("fused", 4, 3, 2, 48, 80, 5),
               ("mb", 4, 3, 2, 80, 160, 7), ("mb", 6, 3, 1, 160, 176, 14), ("mb", 6, 3, 2, 176, 304, 18),
               ("mb", 6, 3, 1, 304, 512, 5))
V2_HEAD = 1280


def _no_kernel(what: str):
    from .._lib import HipLibraryError
    raise HipLibraryError(f"EfficientNetV2: no hand-written kernel for {what}")


class Conv2dNormActivation(_FoldedMixin, nn.Sequential):
    """conv (no bias) + BatchNorm2d(eps 1e-3) [+ activation], symmetric padding (k - 1) // 2 (torchvision.ops.misc).
    Its own GPU fast path covers the two places the Encoder calls it directly: the stem (dense 3x3, few input channels,
    csrc/stem.hip) and the head (1x1, pointwise kernel).  Inside blocks the block's fast path reads its parameters."""

    def __init__(self, cin, cout, k=3, stride=1, groups=1, act=True):
        layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout, eps=BN_EPS)]
        if act:
            layers.append(nn.SiLU(inplace=True))
        super().__init__(*layers)

    @property
    def has_act(self) -> bool:
        return len(self) == 3

    def _fold(self):
        w, b = fold_bn(self[0], self[1])
        if self[0].kernel_size == (1, 1):
            return hip_ops.pointwise_weight(w), b
        return w.float().contiguous(), b.float().contiguous()

    def forward(self, x):
        if not self._fast(x):
            return super().forward(x)
        c = self[0]
        act = hip_ops.ACT_SILU if self.has_act else hip_ops.ACT_NONE
        if c.kernel_size == (1, 1) and c.stride == (1, 1) and c.groups == 1 and c.in_channels % 8 == 0:
            w, b = self._folded(x)
            return hip_ops.pointwise_nhwc(x, w, b, act)
        if (c.kernel_size == (3, 3) and c.groups == 1 and c.in_channels * 9 <= 32 and c.out_channels <= 64
                and c.stride[0] == c.stride[1]):
            w, b = self._folded(x)
            return hip_ops.stem_conv_same(x.contiguous(), w, b, c.stride[0], act, padding=c.padding)
        _no_kernel(f"{c} on {tuple(x.shape)}")


class SqueezeExcitation(nn.Module):
    """torchvision.ops.SqueezeExcitation: avgpool, fc1 (1x1, bias), SiLU, fc2 (1x1, bias), sigmoid scale."""

    def __init__(self, chs, squeeze):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(chs, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, chs, 1)
        self.activation = nn.SiLU()
        self.scale_activation = nn.Sigmoid()

    def forward(self, x):
        s = self.fc2(self.activation(self.fc1(self.avgpool(x))))
        return x * self.scale_activation(s)

    def params(self):
        """(w1 [R, C], b1, w2t [R, C], b2): what hip_ops' squeeze-excite gate kernels read."""
        return (self.fc1.weight.detach().flatten(1).contiguous(), self.fc1.bias.detach().contiguous(),
                self.fc2.weight.detach().flatten(1).t().contiguous(), self.fc2.bias.detach().contiguous())


class StochasticDepth(nn.Module):
    """torchvision.ops.StochasticDepth("row"): identity in eval (and here in training too -- training is out of scope)."""

    def __init__(self, p: float):
        super().__init__()
        self.p = p

    def forward(self, x):
        return x


class FusedMBConv(_FoldedMixin, nn.Module):
    def __init__(self, cin, cout, expand, k, stride, sd_prob=0.0):
        super().__init__()
        self.use_res_connect = stride == 1 and cin == cout
        mid = cin * expand
        if mid != cin:
            self.block = nn.Sequential(Conv2dNormActivation(cin, mid, k, stride), Conv2dNormActivation(mid, cout, 1, act=False))
        else:
            self.block = nn.Sequential(Conv2dNormActivation(cin, cout, k, stride))
        self.stochastic_depth = StochasticDepth(sd_prob)
        self.out_channels = cout

    def _fold(self):
        w, b = fold_bn(self.block[0][0], self.block[0][1])
        hi, lo = hip_ops.prep_conv_weight(w)
        out = (hi, lo, b.float().contiguous())
        if len(self.block) == 2:
            wp, bp = fold_bn(self.block[1][0], self.block[1][1])
            out += (hip_ops.pointwise_weight(wp), bp)
        return out

    def forward(self, x):
        if self._fast(x):
            # expand 1: ONE launch (3x3 + BN + SiLU + residual); expand 4: 3x3 (+ BN + SiLU), then the 1x1 project (+ BN, + residual)
            f = self._folded(x)
            c = self.block[0][0]
            res = x if self.use_res_connect else None
            if len(self.block) == 1:
                return hip_ops.conv3x3_strided(x, f[0], f[1], f[2], c.stride[0], c.padding, hip_ops.ACT_SILU, residual=res)
            y = hip_ops.conv3x3_strided(x, f[0], f[1], f[2], c.stride[0], c.padding, hip_ops.ACT_SILU)
            return hip_ops.pointwise_nhwc(y, f[3], f[4], hip_ops.ACT_NONE, residual=res)
        result = self.block(x)
        if self.use_res_connect:
            result = self.stochastic_depth(result)
            result = result + x
        return result


class MBConv(_FoldedMixin, nn.Module):
    def __init__(self, cin, cout, expand, k, stride, sd_prob=0.0):
        super().__init__()
        self.use_res_connect = stride == 1 and cin == cout
        mid = cin * expand
        layers = []
        if mid != cin:
            layers.append(Conv2dNormActivation(cin, mid, 1))
        layers.append(Conv2dNormActivation(mid, mid, k, stride, groups=mid))
        layers.append(SqueezeExcitation(mid, max(1, cin // 4)))
        layers.append(Conv2dNormActivation(mid, cout, 1, act=False))
        self.block = nn.Sequential(*layers)
        self.stochastic_depth = StochasticDepth(sd_prob)
        self.out_channels = cout

    def _fold(self):
        if len(self.block) != 4:
            _no_kernel("an MBConv block without expansion")
        we, be = fold_bn(self.block[0][0], self.block[0][1])
        wd, bd = fold_bn(self.block[1][0], self.block[1][1])
        wl, bl = fold_bn(self.block[3][0], self.block[3][1])
        return (hip_ops.pointwise_weight(we), be, _dw_tap_major(wd), bd, hip_ops.pointwise_weight(wl), bl) + self.block[2].params() + \
            (wl.flatten(1).contiguous(),)

    def forward(self, x):
        if self._fast(x):
            # the B family's plan with torchvision's symmetric padding
            dw = self.block[1][0]
            return mbconv_plan(x, self._folded(x), dw.kernel_size[0], dw.stride[0], dw.padding, x if self.use_res_connect else None)
        result = self.block(x)
        if self.use_res_connect:
            result = self.stochastic_depth(result)
            result = result + x
        return result


class EfficientNetV2(nn.Module):
    def __init__(self, stages, head=V2_HEAD, num_classes=1000, dropout=0.2, stochastic_depth_prob=0.2):
        super().__init__()
        layers = [Conv2dNormActivation(3, stages[0][4], 3, 2)]
        total, bid = sum(s[6] for s in stages), 0
        for kind, e, k, s, cin, cout, reps in stages:
            stage = []
            for r in range(reps):
                blk = FusedMBConv if kind == "fused" else MBConv
                stage.append(blk(cin if r == 0 else cout, cout, e, k, s if r == 0 else 1, stochastic_depth_prob * bid / total))
                bid += 1
            layers.append(nn.Sequential(*stage))
        layers.append(Conv2dNormActivation(stages[-1][5], head, 1))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Dropout(p=dropout, inplace=True), nn.Linear(head, num_classes))

    def forward(self, x):
        x = self.avgpool(self.features(x))
        return self.classifier(torch.flatten(x, 1))


def efficientnet_v2_s(**kw) -> EfficientNetV2:
    """torchvision's efficientnet_v2_s architecture (21,458,488 parameters with the classifier); no weights -- load them."""
    return EfficientNetV2(V2_S_STAGES, dropout=0.2, **kw)


def efficientnet_v2_m(**kw) -> EfficientNetV2:
    """torchvision's efficientnet_v2_m architecture (54,139,356 parameters with the classifier); no weights -- load them."""
    return EfficientNetV2(V2_M_STAGES, dropout=0.3, **kw)
