"""-m gpu: every block of the four encoders on the HIP path against a float64 CPU copy of that block, on the block's own input.

The skip-level tests (test_hip_encoders.py, G8 in test_hip_models.py) compare the encoders after up to 57 blocks of accumulated
rounding.  Here tests/block_shadow.py hooks every block of ``m.encoder`` (the product's launch plan: for the B family ``keep`` =
3 .. 11 as in G8, so the stem stays fused) and compares images {0, B // 2, B - 1} of each block's GPU output with the float64
copy of that block run on the same images of its GPU input: max |y - ref| / max |ref - x| (the residual branch) for residual
blocks, / max |ref| for the rest (tests/util.branch_dev).  Bars: 5e-5 (KERNEL_TOL) on the default route, 5e-6 with OCV_PW=fp32.

Every case also counts the hip_ops entry points each block calls (and whether its 1x1 launches got a split-K workspace) and
asserts that they equal what the dispatch policy predicts for that (B, H, W): expand_depthwise_fusable,
pointwise_hl_project_pays, ocv_pointwise_split_workspace_bytes.  Every route is covered (blocks per case; B x H x W):

    route                                   B5                              B1              V2-S            V2-M
    fused expand+depthwise (3 launches)     6 (1.*, 3.0), every default     3 (1.1, 1.2,    1 (4.0)         --
                                                                            3.0)
    per-image project (pointwise_hl)        6 (4.1-4.6) at B >= 4           --              --              13 (5.1-5.13) at B >= 4
    plain four-launch plan                  every case                      every           every           every
    split-K 1x1 + its finish launch         B <= 4 (9-18 blocks) *          B 1, 4 *        B 1, 4 *        B 1, 4 and 2 x 192 x 208
    DS block                                3 (0.*)                         2 (0.*)         --              --
    FusedMBConv expand 1 + residual         --                              --              2 (1.*)         3 (1.*)
    FusedMBConv expand 4, stride 2          --                              --              2 (2.0, 3.0)    2 (2.0, 3.0)
    V2 MBConv                               --                              --              fused, four,    per-image, four,
                                                                                            split-K         split-K
    fused stem (pushed activation 3)        every case                      every           --              --
    stem / head                             conv_head                       conv_head       both            both
    (* at 480 x 640; also B5 at 1 x 352 x 1216 and 2 x 192 x 208, B1 and V2-S at 4 x 352 x 1216)

B 9 and 14 are the ragged last batches of a bs-16 pass over the reference's KITTI Eigen (697) and NYU-v2 (654) test lists; 192 x
208 makes stride-2 layers see odd inputs (13 -> 7).  test_squeeze_excite_blocks_on_distinct_images runs every gated block again
on inputs whose images differ, which the seeded B5 weights otherwise make indistinguishable to the squeeze-excite gate."""
import sys
from collections import Counter, defaultdict

import pytest
import torch

import gen
from block_shadow import Shadow
from objcavit_amd import _lib, hip_ops
from objcavit_amd.config import make_args
from objcavit_amd.modules.efficientnet import DepthwiseSeparableConv, InvertedResidual
from objcavit_amd.modules.efficientnet_v2 import EfficientNetV2, FusedMBConv, MBConv

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KERNEL_TOL = 5e-5
FP32_TOL = 5e-6
ENTRY_POINTS = ("pointwise_nhwc", "pointwise_hl", "expand_depthwise_se_gate", "depthwise_se_gate", "depthwise_se_gate_weights",
                "conv3x3_strided", "stem_conv_same")


def _cases():
    """Grouped by (encoder, route) so that each model is built once."""
    at = {"efficientnet-b5": [(B, 480, 640) for B in (1, 2, 3, 4, 9, 14, 16)] + [(B, 352, 1216) for B in (1, 4, 9)] + [(2, 192, 208)]}
    for e in ("efficientnet-b1", "efficientnet-v2-s", "efficientnet-v2-m"):
        at[e] = [(B, 480, 640) for B in (1, 4, 14)] + [(4, 352, 1216)] + ([(2, 192, 208)] if e.endswith("v2-m") else [])
    cases = []
    for e, sizes in at.items():
        cases += [(e, B, H, W, "default") for B, H, W in sizes]
        if e in ("efficientnet-b5", "efficientnet-b1"):
            cases.append((e, 1, 480, 640, "pw_fp32"))
    return cases


CASES = _cases()

_MODELS = {}


def _model(enc, route):
    """(extractor on the GPU, Shadow) per (encoder, route), built once; the fp32 route gets its own model because the folded
    weight caches do not follow OCV_PW."""
    if (enc, route) not in _MODELS:
        from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
        _MODELS.clear()
        m = DenseFeatureExtractor(make_args(model="adabins", encoder_name=enc)).eval()
        gen.load_into(m, 71)
        sh = Shadow(m.encoder.original_model)
        _MODELS[(enc, route)] = (m.cuda(), sh)
    return _MODELS[(enc, route)]


def _cdiv(a, b):
    return -(-a // b)


def predicted_plan(backbone, B, H, W):
    """({block name: Counter of hip_ops entry points (+ "splitk": 1x1 launches given a split-K workspace)} that the encoder's
    dispatch policy gives a B x 3 x H x W image, {block name: its input shape}), walked from the module tree alone.  Every
    3 x 3 / 5 x 5 layer of both families produces ceil(H / stride) rows (TF "SAME", or symmetric (k - 1) // 2 at k = 3)."""
    lib = _lib.load()
    probe = hip_ops.pointwise_weight(torch.zeros(8, 8))           # the 1x1 weight form this route builds (OCV_PW)
    split = isinstance(probe, hip_ops.SplitWeight)

    def pw(M, cin, cout):
        c = Counter(pointwise_nhwc=1)
        if split and lib.ocv_pointwise_split_workspace_bytes(M, cin, cout) > 0:
            c["splitk"] += 1
        return c

    v2 = isinstance(backbone, EfficientNetV2)
    plan = {"features.0" if v2 else "stem": Counter(stem_conv_same=1)}
    shapes = {"features.0" if v2 else "stem": (B, 3, H, W)}
    h, w = _cdiv(H, 2), _cdiv(W, 2)
    for name, mod in backbone.named_modules():
        if isinstance(mod, (DepthwiseSeparableConv, InvertedResidual, MBConv, FusedMBConv)):
            cin = mod.conv_dw.in_channels if isinstance(mod, DepthwiseSeparableConv) else \
                mod.conv_pw.in_channels if isinstance(mod, InvertedResidual) else mod.block[0][0].in_channels
            shapes[name] = (B, cin, h, w)
        if isinstance(mod, DepthwiseSeparableConv):
            s = mod.conv_dw.stride[0]
            h, w = _cdiv(h, s), _cdiv(w, s)
            plan[name] = Counter(depthwise_se_gate=1) + pw(B * h * w, mod.conv_pw.in_channels, mod.conv_pw.out_channels)
        elif isinstance(mod, (InvertedResidual, MBConv)):
            e, d, p = (mod.conv_pw, mod.conv_dw, mod.conv_pwl) if isinstance(mod, InvertedResidual) else \
                (mod.block[0][0], mod.block[1][0], mod.block[3][0])
            k, s, cin, mid, cout = d.kernel_size[0], d.stride[0], e.in_channels, e.out_channels, p.out_channels
            rows_in = B * h * w
            h, w = _cdiv(h, s), _cdiv(w, s)
            if hip_ops.expand_depthwise_fusable(cin, probe, k):
                c = Counter(expand_depthwise_se_gate=1)
            elif split and hip_ops.pointwise_hl_project_pays(B, h * w, mid, cout):
                c = pw(rows_in, cin, mid) + Counter(depthwise_se_gate_weights=1, pointwise_hl=1)
                plan[name] = c
                continue
            else:
                c = pw(rows_in, cin, mid) + Counter(depthwise_se_gate=1)
            plan[name] = c + pw(B * h * w, mid, cout)
        elif isinstance(mod, FusedMBConv):
            c0 = mod.block[0][0]
            h, w = _cdiv(h, c0.stride[0]), _cdiv(w, c0.stride[0])
            plan[name] = Counter(conv3x3_strided=1)
            if len(mod.block) == 2:
                plan[name] += pw(B * h * w, c0.out_channels, mod.out_channels)
    head = backbone.features[-1][0] if v2 else backbone.conv_head
    name = f"features.{len(backbone.features) - 1}" if v2 else "conv_head"
    plan[name] = pw(B * h * w, head.in_channels, head.out_channels)
    shapes[name] = (B, head.in_channels, h, w)
    return plan, shapes


def route_name(backbone, name, calls):
    """A readable route for one block from the entry points it called."""
    mod = dict(backbone.named_modules()).get(name)
    sk = " +split-K" if calls.get("splitk") else ""
    if name in ("stem", "features.0"):
        return "fused stem" if name == "stem" else "v2 stem"
    if name == "conv_head" or not isinstance(mod, (DepthwiseSeparableConv, InvertedResidual, FusedMBConv, MBConv)):
        return "head" + sk
    if isinstance(mod, DepthwiseSeparableConv):
        return "ds" + sk
    if isinstance(mod, FusedMBConv):
        e = "e1" if len(mod.block) == 1 else "e4"
        return f"fused-mb {e} s{mod.block[0][0].stride[0]}{' res' if mod.use_res_connect else ''}" + sk
    pre = "mb " if isinstance(mod, MBConv) else ""
    if calls.get("expand_depthwise_se_gate"):
        return pre + "fused expand+dw" + sk
    if calls.get("pointwise_hl"):
        return pre + "per-image project" + sk
    return pre + "four-launch" + sk


class Ledger:
    """Counts the hip_ops entry points per running block (Shadow.current; the B family's fused stem runs outside any block and
    is booked as "stem") and the split-K workspaces pointwise_nhwc asks for."""

    def __init__(self, monkeypatch, shadow):
        self.calls = defaultdict(Counter)
        self.shadow = shadow
        for n in ENTRY_POINTS:
            monkeypatch.setattr(hip_ops, n, self._wrap(n, getattr(hip_ops, n)))
        enc_mod = sys.modules["objcavit_amd.hip_ops.encoder"]
        ws = enc_mod.workspace

        def workspace(nbytes, device, tag="default", zero=False):
            if tag == "pw_splitk" and nbytes > 0:
                self.calls[self.shadow.current or "stem"]["splitk"] += 1
            return ws(nbytes, device, tag, zero)

        monkeypatch.setattr(enc_mod, "workspace", workspace)

    def _wrap(self, n, f):
        def counted(*a, **kw):
            self.calls[self.shadow.current or "stem"][n] += 1
            return f(*a, **kw)
        return counted


@pytest.mark.parametrize("enc,B,H,W,route", CASES)
def test_encoder_blocks(monkeypatch, enc, B, H, W, route):
    """Measured worst block deviation per (encoder, route) on an MI355X over the cases (bar 5e-5; OCV_PW=fp32 5e-6):
      B5    ds 1.1e-5, four-launch 8.1e-6, fused expand+dw 8.4e-6, per-image project 7.8e-6, head 7.1e-6, stem 3.3e-7;
            fp32: ds 3.0e-7, four-launch 1.3e-6, head 1.1e-6
      B1    ds 1.0e-5, four-launch 9.7e-6, fused expand+dw 8.1e-6, head 8.9e-6, stem 2.7e-7;
            fp32: ds 3.1e-7, four-launch 1.1e-6, head 1.1e-6
      V2-S  fused-mb e1 5.8e-6, e4 s1 1.0e-5, e4 s2 1.2e-5, mb fused expand+dw 9.7e-6, mb four-launch 7.9e-6, head 8.6e-6,
            stem 4.0e-7
      V2-M  fused-mb e1 7.0e-6, e4 s1 1.0e-5, e4 s2 1.0e-5, mb per-image project 9.8e-6, mb four-launch 1.1e-5, head 6.9e-6,
            stem 4.0e-7
    The split-K blocks are within these (<= 9.7e-6)."""
    if route == "pw_fp32":
        monkeypatch.setenv("OCV_PW", "fp32")
    bar = FP32_TOL if route == "pw_fp32" else KERNEL_TOL
    m, sh = _model(enc, route)
    backbone = m.encoder.original_model
    v2 = isinstance(backbone, EfficientNetV2)
    if not v2:
        m.encoder.keep = tuple(range(3, 12))
    img = gen.randn("img", (B, 3, H, W), 71 + B + H)
    sh.records.clear()
    ledger = Ledger(monkeypatch, sh)
    with sh:
        feats = m.encoder(img.cuda())
        if not v2:
            assert feats[1] is None and feats[2] is None          # the stem ran fused
            sh.check_stem(img, feats[3])
    torch.cuda.synchronize()

    want, shapes = predicted_plan(backbone, B, H, W)
    got = {k: +v for k, v in ledger.calls.items()}
    routes = {n: route_name(backbone, n, got.get(n, Counter())) for n in want}
    visits = sh.visits()
    assert set(visits.values()) == {1} and set(visits) == set(want), (set(visits) ^ set(want))
    for r in sh.records:
        assert r["in_shape"] == shapes[r["name"]], (r["name"], r["in_shape"], shapes[r["name"]])
    for n in want:
        assert got.get(n, Counter()) == want[n], (enc, B, f"{H}x{W}", n, routes[n], dict(got.get(n, {})), dict(want[n]))
    assert set(got) == set(want), set(got) ^ set(want)

    worst = defaultdict(float)
    for r in sh.records:
        worst[routes[r["name"]]] = max(worst[routes[r["name"]]], max(r["devs"]))
    count = Counter(routes.values())
    print(f"\n[{enc} B{B} {H}x{W} {route}] {len(sh.records)} blocks; " +
          "; ".join(f"{k} x{count[k]} {worst[k]:.1e}" for k in sorted(count)))
    bad = sh.failures(bar, lambda n: routes[n])
    assert not bad, f"{enc} B={B} {H}x{W} {route}: {len(bad)} (block, image) above {bar:g}; worst " + \
        ", ".join(f"{n} [{rt}] image {i}: {d:.2e}" for d, n, rt, i in bad[:6])


def _se_of(block):
    return block.se if hasattr(block, "se") else block.block[2]


@pytest.mark.parametrize("enc,B", [("efficientnet-b5", 4), ("efficientnet-b5", 9), ("efficientnet-b1", 4),
                                   ("efficientnet-v2-s", 4), ("efficientnet-v2-m", 4), ("efficientnet-v2-m", 9)])
def test_squeeze_excite_blocks_on_distinct_images(monkeypatch, enc, B):
    """Every block with a squeeze-excite gate (DS, IR, MBConv) at its 480 x 640 geometry, on an input whose images differ
    (per-image channel offsets and scale 0.5 .. 1.5), against the float64 block: the same bar and route ledger as above.

    Why: through the encoder, the seeded B5 weights wash out what tells the images apart; in blocks.4.3 the images'
    gates agree to 1e-6, so a block that applied image b - 1's gate (or folded it into image b's project weights) to image b
    would pass test_encoder_blocks.  Here the float64 gates of the sampled images differ by >= 0.05 in every block (asserted;
    smallest measured 0.12, B5 B 4).  Measured worst deviation: B5 1.4e-5 (four-launch), B1 1.2e-5, V2-S 9.7e-6,
    V2-M 9.8e-6 (per-image project)."""
    H, W = 480, 640
    m, sh = _model(enc, "default")
    backbone = m.encoder.original_model
    want, shapes = predicted_plan(backbone, B, H, W)
    blocks = [(n, mod, ref) for n, mod, ref in sh.targets if isinstance(mod, (DepthwiseSeparableConv, InvertedResidual, MBConv))]
    gates, handles = {}, []
    for n, _, ref in blocks:
        # least-squares gate per (image, channel) of the float64 block's squeeze-excite: y = x * g
        handles.append(_se_of(ref).register_forward_hook(
            lambda mod, a, y, _n=n: gates.__setitem__(_n, (a[0] * y).sum((2, 3)) / (a[0] * a[0]).sum((2, 3)))))
    sh.records.clear()
    ledger = Ledger(monkeypatch, sh)
    scale = torch.linspace(0.5, 1.5, B).view(B, 1, 1, 1)
    try:
        with sh:
            for i, (n, mod, _) in enumerate(blocks):
                _, cin, h, w = shapes[n]
                g = torch.Generator().manual_seed(1000 * B + i)
                x = (torch.randn(B, cin, h, w, generator=g) + torch.randn(B, cin, 1, 1, generator=g)) * scale
                mod(x.cuda().contiguous(memory_format=torch.channels_last))
        torch.cuda.synchronize()
    finally:
        for hd in handles:
            hd.remove()

    assert [r["name"] for r in sh.records] == [n for n, _, _ in blocks]
    got = {k: +v for k, v in ledger.calls.items()}
    routes = {n: route_name(backbone, n, got.get(n, Counter())) for n, _, _ in blocks}
    for n, _, _ in blocks:
        assert got.get(n, Counter()) == want[n], (enc, B, n, routes[n], dict(got.get(n, {})), dict(want[n]))
    spread = {n: float((gt.amax(0) - gt.amin(0)).max()) for n, gt in gates.items()}
    assert min(spread.values()) >= 0.05, sorted(spread.items(), key=lambda t: t[1])[:3]

    worst = defaultdict(float)
    for r in sh.records:
        worst[routes[r["name"]]] = max(worst[routes[r["name"]]], max(r["devs"]))
    count = Counter(routes.values())
    print(f"\n[{enc} B{B} distinct images] {len(sh.records)} blocks, gate spread >= {min(spread.values()):.2f}; " +
          "; ".join(f"{k} x{count[k]} {worst[k]:.1e}" for k in sorted(count)))
    bad = sh.failures(KERNEL_TOL, lambda n: routes[n])
    assert not bad, f"{enc} B={B} distinct images: {len(bad)} (block, image) above {KERNEL_TOL:g}; worst " + \
        ", ".join(f"{n} [{rt}] image {i}: {d:.2e}" for d, n, rt, i in bad[:6])
