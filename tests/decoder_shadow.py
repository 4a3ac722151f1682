"""Stage-local float64 shadow of the UNet decoder and of the two head consumers of its output (tests/test_hip_decoder_stages.py,
tests/test_decoder_stages_host.py): the decoder's counterpart of tests/block_shadow.py.

``DecoderShadow(decoder, head=, mvit=)`` keeps a float64 CPU copy of the decoder (plain PyTorch path, BatchNorm unfolded), of the
backbone's bias-free ``conv_head`` (which the GPU path may hand over un-applied) and of the heads' 3x3 convolution.  The GPU
pipeline calls ``forward_split`` / ``SplitConv3x3.run_split`` directly, so forward hooks do not fire: ``with shadow:`` wraps the
methods instead and records every unit on the input that unit actually read, images {0, B // 2, B - 1}, per image, as
max |y - ref| / max |ref| (util.branch_dev).  Units, in forward order:

    conv2                 Decoder._conv2_padded_1x1, where it runs at all (CPU; OCV_UPCONV_FOLD=0 / =direct, OCV_CONV=exact)
    upK.conv1             the stage input (for up1 the tensor the composed GEMM read: b4, or conv_head's input) and the skip ->
                          [conv_head ->] [conv2 ->] bilinear(align_corners) -> cat -> conv3x3 -> BN -> LeakyReLU, compared with
                          what the stage handed its second convolution
    upK.conv2             that tensor -> conv3x3 -> BN -> LeakyReLU
    upK                   a stage that never called its second convolution's plan (the CPU path computes it inline): one unit
    conv3                 its own input -> conv3x3 + bias
    heads.conv3x3         the map the head read -> mViT.conv3x3
    heads.patch_embed     the map the head read -> 16x16 / 16 convolution + bias + positional rows

(K = 1..4 and ``final_upscale``.)  A split tensor (hip_ops.SplitAct, or the split copy behind a ``map_placeholder``) is read as
hi.double() + lo.double(): exactly what the next kernel consumes; its pad channels must be zero (``pad_ok``).  A stage is
recorded at its outermost call only: ``forward`` entering ``forward_split`` is one visit."""
import copy
from collections import Counter

import torch
import torch.nn.functional as F

from block_shadow import sample_images
from objcavit_amd import hip_ops
from objcavit_amd.modules import DenseFeatureExtractor as dfe
from util import branch_dev

STAGES = ("up1", "up2", "up3", "up4", "final_upscale")
# Bars, as a share of max |ref| per image, by the kernel route a unit took -- the project's own, per kernel:
F16_TOL = 4e-6        # fp16 pairs: direct / low-resolution / packed-tap convolutions, conv3, both head consumers (test_hip_fp16_route.py)
WINO_TOL = 1e-5       # Winograd F(4x4, 3x3) (test_winograd43_reads_and_writes_fp16_pairs)
BF16_TOL = 2e-5       # bf16 pairs: OCV_CONV_SPLIT=bf16, and conv_nhwc on fp32 inputs (the per-stage fall-back route)
EXACT_TOL = 2e-6      # the exact-fp32 implicit GEMM (test_conv_nhwc_exact)
PW_TOL = 5e-5         # conv2 as a launch of its own: the encoder's 1x1 kernel, pointwise_nhwc (KERNEL_TOL, test_hip_encoder_blocks.py)


def bar_of(calls, f16):
    """The bar of a unit from the hip_ops entry points it called and the element type of the split pipeline."""
    if calls.get("conv3x3_winograd43_split"):
        return WINO_TOL           # (fp16 pairs inside whatever the input holds)
    if calls.get("conv_nhwc_exact"):
        return EXACT_TOL
    if calls.get("pointwise_nhwc"):
        return PW_TOL
    if calls.get("conv_nhwc") or (not f16 and not calls.get("patch_embed")):
        return BF16_TOL
    return F16_TOL


def read(t, idx):
    """(images ``idx`` of ``t`` as a float64 CPU tensor [n, C, H, W], whether the pad channels of a split tensor are zero)."""
    sp = t if isinstance(t, hip_ops.SplitAct) else getattr(t, "_ocv_split", None) if getattr(t, "_ocv_fp32_missing", False) else None
    if sp is None:
        return t[idx].detach().to("cpu", torch.float64).contiguous(), True
    hl = sp.hl[idx].cpu()
    n, H, W, c2 = hl.shape
    v = hl.view(n, H, W, c2 // 64, 2, 32).double()
    full = (v[..., 0, :] + v[..., 1, :]).reshape(n, H, W, c2 // 2)
    pad_ok = sp.C % 32 == 0 or bool((v[:, :, :, -1, :, sp.C % 32:] == 0).all())
    return full[..., :sp.C].permute(0, 3, 1, 2).contiguous(), pad_ok


class DecoderShadow:
    """``records``: one dict per unit visit (name, images, devs, spread, in_shape, out_shape, pad_ok, fwd); ``current``: the unit
    that is running (None between units); ``enabled`` = False lets a forward pass through unobserved; ``fwd``: a tag the caller
    sets (which forward of a case a record belongs to)."""

    def __init__(self, decoder, head=None, mvit=None):
        self.decoder = decoder
        self.ref = copy.deepcopy(decoder).to("cpu", torch.float64).eval()
        self.head_ref = None if head is None else copy.deepcopy(head).to("cpu", torch.float64).eval()
        self.ref32 = copy.deepcopy(decoder).to("cpu", torch.float32).eval()      # d32: the same unit in float32 on the CPU
        self.d32_units = set()              # units whose records also get ``d32`` (the float32 CPU evaluation against float64)
        self.mvit = mvit
        self.role = {id(decoder._split3): ("conv3", 0)}
        for k in STAGES:
            up = getattr(decoder, k, None)
            if up is not None:
                self.role[id(up._split1)] = (k, 1)
                self.role[id(up._split2)] = (k, 2)
        self.stage_name = {id(getattr(decoder, k)): k for k in STAGES if getattr(decoder, k, None) is not None}
        if mvit is not None:
            self.conv3x3_ref = copy.deepcopy(mvit.conv3x3).to("cpu", torch.float64)
            self.conv3x3_ref32 = copy.deepcopy(mvit.conv3x3).to("cpu", torch.float32)
            if mvit.__dict__.get("_split3x3") is None:
                mvit.__dict__["_split3x3"] = dfe.SplitConv3x3(mvit.conv3x3)
            self.role[id(mvit.__dict__["_split3x3"])] = ("heads.conv3x3", 0)
        self.records, self.taken = [], []
        self.current, self.enabled, self.fwd = None, True, 0
        self.defect = None                  # (stage name, fn(y) -> y): replaces that whole-stage unit's output, for the stages behind it too
        self._ctx = None
        self._undo = []

    # -- float64 references ------------------------------------------------------------------------------------------------------
    def _stage_in(self, name, x, skip, affine, ref=None):
        """cat([up(x), skip]) in float64 for the sampled images; for up1 behind ``affine_of``, x = conv2([conv_head](x0))."""
        if affine:
            if x.shape[1] != self.ref.conv2.in_channels:
                x = self.head_ref(x)
            x = (ref or self.ref).conv2(x)
        up = F.interpolate(x, size=skip.shape[-2:], mode="bilinear", align_corners=True)
        return torch.cat([up, skip], dim=1)

    def _record(self, name, idx, in_shape, y, ref):
        yv, pad_ok = read(y, idx)
        spread = float((ref.amax(0) - ref.amin(0)).abs().max() / ref.abs().max()) if len(idx) > 1 else None
        self.records.append(dict(name=name, images=idx, devs=branch_dev(yv, ref), spread=spread, in_shape=tuple(in_shape),
                                 out_shape=tuple(ref.shape[1:]), pad_ok=pad_ok, fwd=self.fwd))

    # -- wrappers ----------------------------------------------------------------------------------------------------------------
    def _stage(self, orig, up, x, skip, kw):
        name = self.stage_name.get(id(up))
        if name is None or not self.enabled or self._ctx is not None:
            return orig(up, x, skip, **kw)                          # (not this decoder's, switched off, or the inner call of a stage)
        affine = kw.get("affine_of")
        self._ctx = dict(name=name, x=affine[0] if affine is not None else x, skip=skip, affine=affine is not None, done=False)
        self.current = name + ".conv1"
        try:
            y = orig(up, x, skip, **kw)
            ctx = self._ctx
            if not ctx["done"]:                                     # the plain module path: the whole stage is one unit
                if self.defect is not None and self.defect[0] == name:
                    y = self.defect[1](y)
                idx = sample_images(skip.shape[0])
                with torch.no_grad():
                    cat = self._stage_in(name, read(ctx["x"], idx)[0], read(skip, idx)[0], ctx["affine"])
                    self._record(name, idx, ctx["x"].shape, y, getattr(self.ref, name)._net(cat))
            return y
        finally:
            self._ctx, self.current = None, None

    def _conv(self, method, orig, plan, args, kw):
        role = self.role.get(id(plan)) if self.enabled else None
        if role is None or (role[1] == 2 and (self._ctx is None or self._ctx["name"] != role[0] or self._ctx["done"])) or role[1] == 1:
            return orig(plan, *args, **kw)
        name, which = role
        x = args[0]
        idx = sample_images(x.shape[0])
        xv = read(x, idx)[0]
        if method != "run_split" and len(args) > 1 and args[1] is not None:
            xv = torch.cat([xv, read(args[1], idx)[0]], dim=1)
        if which == 2:
            ctx = self._ctx
            with torch.no_grad():
                cat = self._stage_in(name, read(ctx["x"], idx)[0], read(ctx["skip"], idx)[0], ctx["affine"])
                self._record(name + ".conv1", idx, ctx["x"].shape, x, getattr(self.ref, name)._net[:3](cat))
                if name + ".conv1" in self.d32_units and not ctx["affine"]:
                    cat32 = self._stage_in(name, read(ctx["x"], idx)[0].float(), read(ctx["skip"], idx)[0].float(), False)
                    self.records[-1]["d32"] = branch_dev(getattr(self.ref32, name)._net[:3](cat32), getattr(self.ref, name)._net[:3](cat))
            ctx["done"] = True
            unit, ref_mod, ref32_mod = name + ".conv2", getattr(self.ref, name)._net[3:], getattr(self.ref32, name)._net[3:]
        else:
            unit, ref_mod, ref32_mod = (name, self.ref.conv3, self.ref32.conv3) if name == "conv3" else \
                (name, self.conv3x3_ref, self.conv3x3_ref32)
        self.current = unit
        try:
            y = orig(plan, *args, **kw)
        finally:
            self.current = None
        with torch.no_grad():
            ref = ref_mod(xv)
        for out in (y if isinstance(y, tuple) else (y,)):           # (fp32 and split copy of one result: both are what someone reads)
            self._record(unit, idx, x.shape, out, ref)
        if isinstance(y, tuple):                                    # one visit: keep the worse of the two
            a, b = self.records.pop(), self.records.pop()
            a["devs"] = [max(p, q) for p, q in zip(a["devs"], b["devs"])]
            a["pad_ok"] = a["pad_ok"] and b["pad_ok"]
            self.records.append(a)
        if unit in self.d32_units:
            with torch.no_grad():
                self.records[-1]["d32"] = branch_dev(ref32_mod(xv.float()), ref)
        return y

    def _conv2(self, orig, dec, b4):
        if dec is not self.decoder or not self.enabled:
            return orig(dec, b4)
        self.current = "conv2"
        try:
            y = orig(dec, b4)
        finally:
            self.current = None
        idx = sample_images(b4.shape[0])
        with torch.no_grad():
            self._record("conv2", idx, b4.shape, y, self.ref.conv2(read(b4, idx)[0]))
        return y

    def _conv3_hook(self, mod, args, y):
        if self.enabled:                                            # (the module call: CPU / training path only)
            idx = sample_images(args[0].shape[0])
            with torch.no_grad():
                self._record("conv3", idx, args[0].shape, y, self.ref.conv3(read(args[0], idx)[0]))

    def _patch_embed(self, orig, fmap, weight, bias, pos, *a, **kw):
        if not self.enabled or self.mvit is None or weight.data_ptr() != self.mvit.patch_transformer.embedding_convPxP.weight.data_ptr():
            return orig(fmap, weight, bias, pos, *a, **kw)
        self.current = "heads.patch_embed"
        try:
            tok = orig(fmap, weight, bias, pos, *a, **kw)
        finally:
            self.current = None
        idx = sample_images(fmap.shape[0])
        with torch.no_grad():
            w, b, p = (t.detach().to("cpu", torch.float64) for t in (weight, bias, pos))
            ref = F.conv2d(read(fmap, idx)[0], w, b, stride=16).flatten(2).transpose(1, 2) + (p if p.dim() == 2 else p[idx])
        self._record("heads.patch_embed", idx, fmap.shape, tok, ref)
        return tok

    def _skip_part(self, orig, up, *a, **kw):
        """A skip part issued beside the encoder (SkipPrepass) belongs to its stage's first convolution."""
        name = self.stage_name.get(id(up))
        if name is None or self.current is not None or not self.enabled:
            return orig(up, *a, **kw)
        self.current = name + ".conv1"
        try:
            return orig(up, *a, **kw)
        finally:
            self.current = None

    def _take(self, orig, pre, up, f16):
        sk = orig(pre, up, f16)
        if sk is not None and id(up) in self.stage_name and self.enabled:
            self.taken.append((self.fwd, self.stage_name[id(up)]))
        return sk

    def __enter__(self):
        def patch(obj, attr, make):
            orig = getattr(obj, attr)
            setattr(obj, attr, make(orig))
            self._undo.append((obj, attr, orig))

        U, S = dfe.UpSampleWithSkip, dfe.SplitConv3x3
        patch(U, "forward_split", lambda o: lambda up, x, skip, **kw: self._stage(o, up, x, skip, kw))
        patch(U, "forward", lambda o: lambda up, x, skip: self._stage(o, up, x, skip, {}))
        patch(U, "skip_part", lambda o: lambda up, *a, **kw: self._skip_part(o, up, *a, **kw))
        for m in ("run_split", "__call__", "exact"):
            patch(S, m, lambda o, _m=m: lambda plan, *a, **kw: self._conv(_m, o, plan, a, kw))
        patch(dfe.Decoder, "_conv2_padded_1x1", lambda o: lambda dec, b4: self._conv2(o, dec, b4))
        patch(dfe.SkipPrepass, "take", lambda o: lambda pre, up, f16: self._take(o, pre, up, f16))
        patch(hip_ops, "patch_embed_auto", lambda o: lambda *a, **kw: self._patch_embed(o, *a, **kw))
        self._hook = self.decoder.conv3.register_forward_hook(self._conv3_hook)
        return self

    def __exit__(self, *exc):
        for obj, attr, orig in reversed(self._undo):
            setattr(obj, attr, orig)
        self._undo = []
        self._hook.remove()
        self._ctx, self.current = None, None

    def visits(self, fwd=None):
        return Counter(r["name"] for r in self.records if fwd is None or r["fwd"] == fwd)

    def failures(self, bar_of, fwd=None):
        """[(dev, unit, image, bar)] of every (unit, image) above ``bar_of(unit name)``, worst first."""
        bad = [(d, r["name"], i, bar_of(r["name"])) for r in self.records if fwd is None or r["fwd"] == fwd
               for i, d in zip(r["images"], r["devs"]) if not d <= bar_of(r["name"])]
        return sorted(bad, reverse=True)
