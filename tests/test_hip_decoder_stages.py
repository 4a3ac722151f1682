"""-m gpu: every unit of the four UNet decoders and the two head consumers of their output on the HIP path against float64, each
on the input it actually read (tests/decoder_shadow.py), with a ledger of the kernel routes taken.

The end-to-end decoder tests (test_encoder_fast_path_vs_oracle, G8, G9 / G10) compare the decoder OUTPUT at 1e-4 after ten
convolutions; the kernel tests use random tensors at a handful of shapes.  Here the product's own forward runs -- AdaBins, so the
decoder is called with ``_split_only`` and ``SkipPrepass`` -- TWICE per case: the first forward calibrates the fp16-pair route
and records the skip plans, the second is the settled one whose three skip parts come from the side stream.  Every unit of the
second forward (and of the first in each model's first case) is compared per image {0, B // 2, B - 1} as max |y - ref| / max |ref|
with the bar of the kernel route it took (decoder_shadow.bar_of), and the hip_ops entry points each unit called -- plus the
split-K workspaces ``conv_nhwc_split`` asked for -- must equal ``predicted_plan``, which walks the module tree with the library's
own policy functions (lowres_ready / tap_interp_supported, winograd_pays, packed_taps_pay, ocv_conv_nhwc_split_workspace_bytes,
Decoder._up1_affine, split_ready, usable).  Routes (asserted covered by test_every_route_is_covered):

    route                                     where
    composed up1 (conv_head + conv2 + taps)   B5, B1: every default case; V2: conv2 + taps (no deferred head)
    un-composed up1, conv2 its own launch     OCV_UPCONV_FOLD=0 (B5, V2-M), OCV_UPCONV=direct, OCV_CONV=exact, per-stage route
    low-resolution first convolution          every default case; tap interpolation with 2 and 3 staging rounds
    skip part: packed taps 16 / 24 / 40 / 48  B1 up4 / B5, V2 up4, B1 up3 / B5 up3, B1 up2 / V2 up3;  direct: 64 .. 176
    skip parts from the side stream           second forward of every all-split case (up2, up3, up4)
    Winograd F(4x4, 3x3)                      second convolutions of up1 (all) and up2 (B5); direct route: first ones (2224, 1440 in)
    direct 3x3 on 320 -> 320                  1280-feature up2 second convolution
    Cout % 32 != 0 split output (80)          1280-feature up4, conv3 reading Cp = 96
    resize + concat + direct 3x3, split-K     OCV_UPCONV=direct only: B5 B 2 (up3 552 -> 256), V2-S B 14 (up2 704 -> 320)
    bf16 pairs                                OCV_CONV_SPLIT=bf16
    exact fp32                                OCV_CONV=exact; final_upscale over 83 channels on the per-stage route
    fifth stage (do_final_upscale)            B5: tap GEMM at half resolution + conv3x3_few_channels; V2-S: per-stage route
    per-stage route (fp32 hand-over)          V2-S + do_final_upscale (80 up-sampled channels are no whole 32-blocks)

On the default route no decoder or head convolution of any model gets a split-K workspace (asserted): every convolution long
enough is a Winograd one.  test_stages_on_distinct_images runs every stage again on inputs whose images differ: through the
seeded encoders the images of a batch are indistinguishable at the deep stages, while the 256-row tiles of the convolutions
straddle two images wherever H W is no multiple of 256."""
import sys
from collections import Counter, defaultdict

import pytest
import torch

import gen
from block_shadow import sample_images
from decoder_shadow import EXACT_TOL, STAGES, DecoderShadow, bar_of
from objcavit_amd import _lib, hip_ops
from objcavit_amd.config import make_args
from objcavit_amd.modules import DenseFeatureExtractor as dfe

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

B5, B1, V2S, V2M = "efficientnet-b5", "efficientnet-b1", "efficientnet-v2-s", "efficientnet-v2-m"
ROUTES = {"default": {}, "direct": {"OCV_UPCONV": "direct"}, "nofold": {"OCV_UPCONV_FOLD": "0"}, "bf16": {"OCV_CONV_SPLIT": "bf16"},
          "exact": {"OCV_CONV": "exact"}, "final": {}}
ENTRY_POINTS = ("conv3x3_split_packed_taps", "conv3x3_winograd43_split", "tap_interp_combine", "upsample_concat_split",
                "conv3x3_few_channels", "conv_nhwc", "conv_nhwc_exact", "pointwise_nhwc")


def _cases():
    """Grouped by (encoder, route) so that each model is built once; each model's first case is its B = 1 one where it has one."""
    cases = [(B5, B, 480, 640, "default") for B in (1, 2, 3, 9, 16)] + [(B5, 1, 352, 1216, "default"), (B5, 4, 352, 1216, "default"),
                                                                         (B5, 2, 192, 208, "default")]
    for e in (B1, V2S, V2M):
        cases += [(e, 1, 480, 640, "default"), (e, 14, 480, 640, "default"), (e, 4, 352, 1216, "default")]
        if e == V2M:
            cases.append((e, 2, 192, 208, "default"))
    cases += [(B5, 2, 480, 640, "direct"), (V2S, 14, 480, 640, "direct"), (B5, 2, 480, 640, "nofold"), (V2M, 2, 480, 640, "nofold"),
              (B5, 2, 480, 640, "bf16"), (B5, 2, 192, 208, "exact"),
              (B5, 1, 480, 640, "final"), (B5, 2, 192, 208, "final"), (V2S, 1, 480, 640, "final"), (V2S, 2, 192, 208, "final")]
    return cases


CASES = _cases()
_MODELS = {}
SEEN = defaultdict(set)          # "worst <route>" -> what the cases of this run measured (printed by test_every_route_is_covered)


def _model(enc, route):
    """(AdaBins on the GPU, DecoderShadow) per (encoder, route), built once: the prepared weights follow the route."""
    if (enc, route) not in _MODELS:
        from objcavit_amd.modules.AdaBins import AdaBins
        _MODELS.clear()
        m = AdaBins(make_args(model="adabins", encoder_name=enc, do_final_upscale=route == "final")).eval()
        gen.load_into(m, 61)
        ext = m.dense_feature_extractor
        sh = DecoderShadow(ext.decoder, head=getattr(ext.encoder.original_model, "conv_head", None), mvit=m.adaptive_bins_layer)
        _MODELS[(enc, route)] = (m.cuda(), sh)
    return _MODELS[(enc, route)]


def _cdiv(a, b):
    return -(-a // b)


def _forward(m, img):
    """AdaBins' forward -- or, where the decoded map has fewer than the 129 patches its bin head needs (192 x 208 without
    do_final_upscale: 6 x 6), the extractor as AdaBins calls it and the two head consumers on its output."""
    ext, mvit = m.dense_feature_extractor, m.adaptive_bins_layer
    h, w = img.shape[2:] if ext.decoder.final_upscale is not None else (_cdiv(img.shape[2], 2), _cdiv(img.shape[3], 2))
    if (h // 16) * (w // 16) > mvit.n_query_channels:
        assert bool(torch.isfinite(m(img).depth_pred).all())
        return
    fmap = ext(img, _split_only=True)
    assert bool(torch.isfinite(mvit.patch_transformer.forward_batch_first(fmap)).all())
    assert bool(torch.isfinite(mvit._conv3x3_nhwc(fmap)).all())


class _Like:
    """Shape / device / dtype of a tensor that does not exist (what the policy functions consult)."""

    def __init__(self, *shape):
        self.shape, self.device, self.dtype = torch.Size(shape), torch.device("cuda"), torch.float32


def predicted_plan(decoder, head, B, H, W):
    """{unit: Counter of hip_ops entry points (conv_nhwc_split by kernel size; "splitk": launches given a split-K workspace)} that
    the dispatch policy gives a B x 3 x H x W image under the current environment, walked from the module tree and the library's
    policy functions alone, + facts about the walk (route name -> units).  Every stride-2 layer of both encoder families produces
    ceil(size / 2) rows."""
    lib = _lib.load()
    facts = defaultdict(list)

    def direct(b, h, w, cin, cout, k):
        c = Counter({f"conv_nhwc_split_{k}": 1})
        if lib.ocv_conv_nhwc_split_workspace_bytes(b, h, w, cin, cout, k) > 0:
            c["splitk"] += 1
        return c

    def conv3x3(b, h, w, cin, cout):
        if hip_ops.winograd_pays(b, h, w, cin, cout):
            return Counter(conv3x3_winograd43_split=1)
        return direct(b, h, w, cin, cout, 3)

    hw = [(H, W)]
    for _ in range(5):
        hw.append((_cdiv(hw[-1][0], 2), _cdiv(hw[-1][1], 2)))
    names = [k for k in STAGES if getattr(decoder, k, None) is not None]
    ups = [getattr(decoder, k) for k in names]
    f = decoder.conv2.out_channels
    c3 = decoder.conv3.in_channels
    skips, c1 = [], f
    for i, up in enumerate(ups):
        skips.append(_Like(B, up._net[0].in_channels - c1, *hw[4 - i]))
        c1 = up._net[0].out_channels
    h4, w4 = hw[5]
    x = _Like(B, f, h4 + 2, w4 + 2)
    fin = decoder.final_upscale
    split3 = decoder._split3.usable(c3) and c3 % 8 == 0
    all_split = bool(decoder.up1.split_ready(x, skips[0]) and split3
                     and (fin is None or fin.split_ready(_Like(B, decoder.up4._net[3].out_channels, *hw[1]), skips[4])))
    b4 = _Like(B, decoder.conv2.in_channels, h4, w4)
    deferred = head is not None                       # (the B family's bias-free conv_head is handed over un-applied)
    if deferred:
        b4 = dfe.DeferredConv1x1(_Like(B, head.in_channels, h4, w4), head)
    affine = decoder._up1_affine(b4, skips[0]) if all_split else None
    plan = {}
    if affine is None:
        plan["conv2"] = Counter(pointwise_nhwc=1)
        facts["conv2 own launch"].append("conv2")
    xs = x
    for i, (name, up, skip) in enumerate(zip(names, ups, skips)):
        cin1, cout = xs.shape[1], up._net[0].out_channels
        c2, (hs, ws) = skip.shape[1], skip.shape[2:]
        if all_split or up.split_ready(xs, skip):
            if (i == 0 and affine is not None) or up.lowres_ready(xs, skip):
                if i == 0 and affine is not None:
                    x0 = affine[1][0]
                    c = direct(B, x0.shape[2], x0.shape[3], x0.shape[1], 9 * cout, 1)
                    facts["composed up1" + (" behind conv_head" if deferred else "")].append(name)
                else:
                    c = direct(B, xs.shape[2], xs.shape[3], cin1, 9 * cout, 1)
                c["tap_interp_combine"] += 1
                facts[f"tap interpolation nj {hip_ops.tap_interp_staging_rounds(xs.shape[2], xs.shape[3], hs, ws)}"].append(name)
                if c2 <= 4:
                    c["conv3x3_few_channels"] += 1
                    facts["few-channel skip"].append(name)
                elif hip_ops.packed_taps_pay(c2):
                    c["conv3x3_split_packed_taps"] += 1
                    facts[f"packed taps {c2}"].append(name)
                else:
                    c += direct(B, hs, ws, c2, cout, 3)
                    facts["direct skip part"].append(name)
            else:
                c = Counter(upsample_concat_split=1) + conv3x3(B, hs, ws, cin1 + c2, cout)
                facts["resize + concat + 3x3"].append(name)
                if cin1 + c2 > 1024 and c.get("conv3x3_winograd43_split"):
                    facts["Winograd Cp > 1024"].append(name)
            plan[name + ".conv1"] = c
            plan[name + ".conv2"] = conv3x3(B, hs, ws, cout, cout)
            if cout % 32:
                facts["Cout % 32 != 0 split output"].append(name)
            if not plan[name + ".conv2"].get("conv3x3_winograd43_split") and cout >= 320:
                facts["direct 3x3 on >= 320 channels"].append(name)
        else:
            plan[name + ".conv1"] = Counter(conv_nhwc=1) if up._split1.usable(cin1, c2) else Counter(conv_nhwc_exact=1)
            plan[name + ".conv2"] = Counter(conv_nhwc=1) if up._split2.usable(cout) else Counter(conv_nhwc_exact=1)
            facts["stage on fp32 operands"].append(name)
        xs = _Like(B, cout, hs, ws)
    if all_split:
        plan["conv3"] = conv3x3(B, xs.shape[2], xs.shape[3], c3, decoder.conv3.out_channels)
        plan["heads.conv3x3"] = conv3x3(B, xs.shape[2], xs.shape[3], 128, 128)
        split_pe = hip_ops.split_only_enabled() and hip_ops.patch_embed_split_supported(B, 128, xs.shape[2], xs.shape[3], 128)
        plan["heads.patch_embed"] = Counter(patch_embed_split=1) if split_pe else Counter(patch_embed=1)
    else:
        facts["per-stage route"].append("decoder")
        plan["conv3"] = Counter(conv_nhwc=1) if decoder._split3.usable(c3) else Counter(conv_nhwc_exact=1)
        plan["heads.conv3x3"] = Counter(conv_nhwc=1) if dfe.split_bf16_convs_enabled() else Counter(conv_nhwc_exact=1)
        plan["heads.patch_embed"] = Counter(patch_embed=1)
    for u, c in plan.items():
        for k in ("conv3x3_winograd43_split", "splitk", "conv_nhwc_exact"):
            if c.get(k):
                facts[{"conv3x3_winograd43_split": "Winograd", "splitk": "split-K", "conv_nhwc_exact": "exact fp32"}[k]].append(u)
    return plan, dict(facts), all_split


def route_name(calls):
    """A readable route for one unit from the entry points it called."""
    if calls.get("pointwise_nhwc"):
        return "1x1"
    if calls.get("patch_embed_split") or calls.get("patch_embed"):
        return "patch embed" + (" exact" if calls.get("patch_embed") else "")
    sk = " +split-K" if calls.get("splitk") else ""
    if calls.get("tap_interp_combine"):
        tail = "packed skip" if calls.get("conv3x3_split_packed_taps") else "few-channel skip" if calls.get("conv3x3_few_channels") else "direct skip"
        return "lowres + " + tail + sk
    pre = "resize+concat + " if calls.get("upsample_concat_split") else ""
    if calls.get("conv3x3_winograd43_split"):
        return pre + "winograd"
    if calls.get("conv_nhwc_exact"):
        return "exact"
    if calls.get("conv_nhwc"):
        return "bf16 on fp32"
    return pre + "direct" + sk


class Ledger:
    """Counts the hip_ops entry points per running unit (DecoderShadow.current; launches outside any unit -- the encoder's -- are
    not booked) and the split-K workspaces conv_nhwc_split asks for."""

    def __init__(self, monkeypatch, shadow):
        self.calls = defaultdict(Counter)
        self.shadow = shadow
        for n in ENTRY_POINTS:
            monkeypatch.setattr(hip_ops, n, self._wrap(n, getattr(hip_ops, n)))
        heads = sys.modules["objcavit_amd.hip_ops.heads"]          # (patch_embed_auto calls its two forms inside its own module)
        for n in ("patch_embed_split", "patch_embed"):
            monkeypatch.setattr(heads, n, self._wrap(n, getattr(heads, n)))
        split = hip_ops.conv_nhwc_split

        def conv_nhwc_split(x, w_hi, w_lo, bias, ksize, *a, **kw):
            self.book(f"conv_nhwc_split_{ksize}")
            return split(x, w_hi, w_lo, bias, ksize, *a, **kw)

        monkeypatch.setattr(hip_ops, "conv_nhwc_split", conv_nhwc_split)
        conv = sys.modules["objcavit_amd.hip_ops.conv"]
        ws = conv.workspace

        def workspace(nbytes, device, tag="default", zero=False):
            if tag == "conv_splitk" and nbytes > 0:
                self.book("splitk")
            return ws(nbytes, device, tag, zero)

        monkeypatch.setattr(conv, "workspace", workspace)

    def book(self, n):
        if self.shadow.current is not None and self.shadow.enabled:
            self.calls[(self.shadow.fwd, self.shadow.current)][n] += 1

    def _wrap(self, n, f):
        def counted(*a, **kw):
            self.book(n)
            return f(*a, **kw)
        return counted

    def of(self, fwd):
        return {u: +c for (fw, u), c in self.calls.items() if fw == fwd}


def _report(tag, sh, got, fwd, f16):
    """Print one line for a forward, return its failures; every unit's bar follows the route it took.  One bar is not the
    project's own: ``final_upscale.conv1`` on the per-stage route (V2-S + do_final_upscale) is ATen's float32 bilinear resize in
    front of the exact-fp32 kernel, and float32 resize coordinates alone put the float32 CPU evaluation of that unit (d32)
    at 2.1e-6 (2 x 192 x 208) and 7.4e-6 (1 x 480 x 640) of max |ref| -- the float64 convolution of the float32 resize gives
    the same figures on the CPU.  The HIP path measured 2.04e-6 and 7.5e-6 there against the exact kernel's 2e-6: at d32's
    level, rounding of the reference arithmetic itself, so that unit's bar is 2 x max(2e-6, d32), d32 measured on the unit's
    own input in the same run (DecoderShadow.d32_units), and never above 2e-5 (4.3e-6 and 1.5e-5 in those two cases)."""
    routes = {u: route_name(c) for u, c in got.items()}
    bars = {u: bar_of(c, f16) for u, c in got.items()}
    for r in sh.records:
        if r["fwd"] == fwd and r.get("d32") and got[r["name"]].get("conv_nhwc_exact") and r["name"] == "final_upscale.conv1":
            bars[r["name"]] = min(2e-5, 2 * max(EXACT_TOL, max(r["d32"])))
            print(f"\n    {r['name']}: d32 {max(r['d32']):.1e}, bar {bars[r['name']]:.1e}")
    worst = defaultdict(float)
    for r in sh.records:
        if r["fwd"] == fwd:
            worst[routes[r["name"]]] = max(worst[routes[r["name"]]], max(r["devs"]))
            SEEN["worst " + routes[r["name"]] + ("" if f16 else " (bf16 pairs)")].add(f"{tag} {r['name']}: {max(r['devs']):.1e} of {bars[r['name']]:g}")
    count = Counter(routes[r["name"]] for r in sh.records if r["fwd"] == fwd)
    print(f"\n[{tag} forward {fwd}] {sum(count.values())} units; " + "; ".join(f"{k} x{count[k]} {worst[k]:.1e}" for k in sorted(count)))
    print("    " + ", ".join(f"{r['name']} {max(r['devs']):.1e}/{bars[r['name']]:g}" + (f" (d32 {max(r['d32']):.1e})" if r.get("d32") else "")
                             for r in sh.records if r["fwd"] == fwd))
    return sh.failures(lambda n: bars[n], fwd)


@pytest.mark.parametrize("enc,B,H,W,route", CASES)
def test_decoder_stages(monkeypatch, enc, B, H, W, route):
    """Measured worst unit deviation per (encoder, route) on an MI355X over the cases, as a share of max |ref| (bar):
      B5    default: low-resolution conv1 8.3e-7 (direct skip) / 1.4e-6 (packed skip), direct 3x3 2.2e-6 (up3.conv2) (4e-6),
            Winograd 1.6e-6 (1e-5), patch embedding 4.9e-7, heads' 3x3 1.5e-6 (4e-6); first and second forward agree
            OCV_UPCONV=direct: resize + concat + Winograd 2.8e-6 (1e-5), + direct 8.5e-7, + split-K 1.4e-6, conv2 5.7e-6 (5e-5)
            OCV_UPCONV_FOLD=0: as default, conv2 5.7e-6;  OCV_CONV_SPLIT=bf16: 7.0e-6 .. 9.4e-6 (2e-5), Winograd 7.6e-6 (1e-5)
            OCV_CONV=exact: 4.7e-7 .. 8.5e-7 (2e-6) beside d32 4.1e-7 .. 7.3e-7 -- before the exact kernel summed per block of 32
            channels (csrc/conv_exact.hip) its single chain gave up1.conv1 6.6e-6, up1.conv2 3.9e-6, ... conv3 1.9e-6
            do_final_upscale: final_upscale.conv1 1.6e-6 (tap GEMM + conv3x3_few_channels), .conv2 1.0e-6
      B1    low-resolution conv1 5.4e-7 / 1.6e-6, direct 1.8e-6, Winograd 1.3e-6, patch embedding 4.2e-7
      V2-S  low-resolution conv1 8.7e-7 / 2.7e-6, direct 1.7e-6, Winograd 1.4e-6; direct route: split-K 8.3e-7, Winograd conv1 2.7e-6
            do_final_upscale (per-stage route): up1 .. up4 as default, final_upscale.conv1 (exact) 7.5e-6 at 1 x 480 x 640
            (d32 7.4e-6, bar 1.5e-5) and 2.0e-6 at 2 x 192 x 208 (d32 2.1e-6, bar 4.3e-6: see _report), final_upscale.conv2 /
            conv3 / heads' 3x3 on conv_nhwc 6.8e-6 (2e-5), patch embedding (exact kernel) 4.4e-7
      V2-M  low-resolution conv1 1.3e-6 / 3.7e-6 (up4.conv1 at 4 x 352 x 1216), direct 2.1e-6, Winograd 1.3e-6, conv2 6.1e-6
    Wall time of the file: 4 min 21 s beside 1 min 20 s for test_hip_encoder_blocks.py on the same machine."""
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    m, sh = _model(enc, route)
    dec = m.dense_feature_extractor.decoder
    head = getattr(m.dense_feature_extractor.encoder.original_model, "conv_head", None)
    first_case = B == 1 and dec.settled_f16() is None and not dec.__dict__.get("_seen_case")      # (its first forward calibrates)
    dec.__dict__["_seen_case"] = True
    img = gen.randn("img", (B, 3, H, W), 61 + B + H).cuda()
    want, facts, all_split = predicted_plan(dec, head, B, H, W)
    hip_ops.ROUTE_REPORT.pop("Decoder", None)
    sh.records.clear()
    sh.taken.clear()
    ledger = Ledger(monkeypatch, sh)
    tag = f"{enc} B{B} {H}x{W} {route}"
    sh.d32_units = {u for u, c in want.items() if c.get("conv_nhwc_exact")}      # (printed beside the exact kernel's own figure)
    with sh:
        for fwd in (1, 2):
            sh.fwd, sh.enabled = fwd, fwd == 2 or first_case
            _forward(m, img)
            torch.cuda.synchronize()
    f16 = hip_ops.conv_split_f16()
    if all_split:
        assert dec.settled_f16() is f16 and "Decoder" not in hip_ops.ROUTE_REPORT, (dec.settled_f16(), hip_ops.ROUTE_REPORT)
        lowres = [n for n in ("up2", "up3", "up4") if want[n + ".conv1"].get("tap_interp_combine")]
        assert sorted(n for fw, n in sh.taken if fw == 2) == lowres and not [n for fw, n in sh.taken if fw == 1], sh.taken
    else:
        assert not sh.taken

    bad = []
    for fwd in (1, 2) if first_case else (2,):
        got = ledger.of(fwd)
        visits = sh.visits(fwd)
        assert set(visits.values()) == {1} and set(visits) == set(want), (fwd, set(visits) ^ set(want), visits)
        for u in want:
            assert got.get(u, Counter()) == want[u], (tag, fwd, u, dict(got.get(u, {})), dict(want[u]))
        assert set(got) == set(want), set(got) ^ set(want)
        assert all(r["pad_ok"] for r in sh.records), [r["name"] for r in sh.records if not r["pad_ok"]]
        bad += [(fwd,) + b for b in _report(tag, sh, got, fwd, f16)]
    if route == "default" or route == "final":
        assert not facts.get("split-K"), facts["split-K"]            # a policy fact: every long convolution is a Winograd one
    assert not bad, f"{tag}: {len(bad)} (unit, image) above their bars; worst " + \
        ", ".join(f"forward {fw} {n} image {i}: {d:.2e} > {b:g}" for fw, d, n, i, b in sorted(bad, key=lambda t: -t[1] / t[4])[:8])


def _distinct(shape, seed, B):
    """randn + a per-(image, channel) offset, scaled 0.5 .. 1.5 across the batch: dense at the image borders, every image its own
    (largest magnitude ~ 8: inside the fp16 calibration window [2^-6, 4094])."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.linspace(0.5, 1.5, B).view(B, 1, 1, 1)
    x = (torch.randn(*shape, generator=g) + torch.randn(shape[0], shape[1], 1, 1, generator=g)) * scale
    return x.cuda().contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("enc,B", [(B5, 2), (B5, 9), (B1, 4), (V2S, 4), (V2M, 4)])
def test_stages_on_distinct_images(monkeypatch, enc, B):
    """Every stage of the decoder, conv3 and the two head consumers called as Decoder._forward / the heads call them (affine_of for
    up1, the split hand-over of the pipeline, the split-only output) at the 480 x 640 geometry, each on synthetic inputs whose
    images differ: the float64 references of the sampled images differ by >= 0.05 of max |ref| in every unit (asserted; the run
    prints the smallest: 0.87 .. 0.95).  Same bars, same ledger as test_decoder_stages.  Measured worst deviations on an MI355X:
    low-resolution conv1 3.9e-6 (B5 B 2 up4.conv1: the closest any unit of this file comes to its bar, 4e-6 -- white noise at
    120 x 160 -> 240 x 320 makes the float32 interpolation coordinates count; 3.1e-6 .. 3.3e-6 in the other cases), Winograd 3.5e-6
    (1e-5), direct 3x3 1.5e-6, patch embedding 5.1e-7."""
    H, W = 480, 640
    m, sh = _model(enc, "default")
    dec, mvit = m.dense_feature_extractor.decoder, m.adaptive_bins_layer
    head = getattr(m.dense_feature_extractor.encoder.original_model, "conv_head", None)
    want, facts, all_split = predicted_plan(dec, head, B, H, W)
    assert all_split and "conv2" not in want
    f16 = hip_ops.conv_split_f16()
    hw = [(H, W)]
    for _ in range(5):
        hw.append((_cdiv(hw[-1][0], 2), _cdiv(hw[-1][1], 2)))
    sh.records.clear()
    sh.fwd = sh.enabled = 1
    ledger = Ledger(monkeypatch, sh)
    stages = [dec.up1, dec.up2, dec.up3, dec.up4]
    with sh:
        c1 = dec.conv2.out_channels
        for i, up in enumerate(stages):
            cout = up._net[0].out_channels
            skip = _distinct((B, up._net[0].in_channels - c1, *hw[4 - i]), 100 * B + 2 * i, B)
            nxt_lowres = i == 3 or stages[i + 1].lowres_ready(_Like(B, cout, *hw[4 - i]), _Like(B, 1, *hw[3 - i]))
            kw = dict(out_fp32=not nxt_lowres, out_split=nxt_lowres, f16=f16)
            if i == 0:
                x0 = _distinct((B, head.in_channels if head is not None else dec.conv2.in_channels, *hw[5]), 100 * B + 1, B)
                shape, aff = dec._up1_affine(dfe.DeferredConv1x1(x0, head) if head is not None else x0, skip)
                up.forward_split(shape, skip, affine_of=aff, **kw)
            else:
                x = _distinct((B, c1, *hw[5 - i]), 100 * B + 2 * i + 1, B)
                if up.lowres_ready(x, skip):
                    x = hip_ops.split_act(x, f16=f16)                # (the pipeline hands a low-resolution stage its input split)
                up.forward_split(x, skip, **kw)
            c1 = cout
        xs = hip_ops.split_act(_distinct((B, c1, *hw[1]), 100 * B + 9, B), f16=f16)
        sp = dec._split3.run_split(xs, hip_ops.ACT_NONE, out_fp32=False, out_split=True)
        fmap = hip_ops.map_placeholder(hip_ops.split_act(_distinct((B, 128, *hw[1]), 100 * B + 10, B), f16=f16))
        assert tuple(sp.shape) == tuple(fmap.shape)
        mvit._conv3x3_nhwc(fmap)
        pt = mvit.patch_transformer
        S = (hw[1][0] // 16) * (hw[1][1] // 16)
        hip_ops.patch_embed_auto(fmap, pt.embedding_convPxP.weight.detach(), pt.embedding_convPxP.bias.detach(),
                                 pt.positional_encodings.detach()[:S], pt._w_cl, pt._w_pe)
        torch.cuda.synchronize()

    got = ledger.of(1)
    visits = sh.visits(1)
    assert set(visits.values()) == {1} and set(visits) == set(want), (set(visits) ^ set(want), visits)
    for u in want:
        assert got.get(u, Counter()) == want[u], (enc, B, u, dict(got.get(u, {})), dict(want[u]))
    assert all(r["images"] == sample_images(B) and r["pad_ok"] for r in sh.records)
    spread = {r["name"]: r["spread"] for r in sh.records}
    print(f"\n[{enc} B{B} distinct images] smallest reference spread {min(spread.values()):.2f} ({min(spread, key=spread.get)})")
    assert min(spread.values()) >= 0.05, sorted(spread.items(), key=lambda t: t[1])[:3]
    bad = _report(f"{enc} B{B} distinct images", sh, got, 1, f16)
    assert not bad, f"{enc} B={B} distinct images: {len(bad)} (unit, image) above their bars; worst " + \
        ", ".join(f"{n} image {i}: {d:.2e} > {b:g}" for d, n, i, b in bad[:8])


REQUIRED = ["composed up1 behind conv_head", "composed up1", "conv2 own launch", "tap interpolation nj 2", "tap interpolation nj 3",
            "packed taps 16", "packed taps 24", "packed taps 40", "packed taps 48", "direct skip part", "few-channel skip",
            "Winograd", "Winograd Cp > 1024", "direct 3x3 on >= 320 channels", "Cout % 32 != 0 split output", "resize + concat + 3x3",
            "split-K", "exact fp32", "stage on fp32 operands", "per-stage route", "Winograd (bf16 pairs)", "packed taps 24 (bf16 pairs)"]


def test_every_route_is_covered(monkeypatch):
    """Every route of the table in this file's docstring is taken by at least one case of CASES, as stated by ``predicted_plan``
    (which every case asserts equal to what the kernels' entry points were called with), and split-K only under
    OCV_UPCONV=direct.  Also prints the worst deviation per route that the cases of this run saw."""
    from objcavit_amd.modules.DenseFeatureExtractor import DenseFeatureExtractor
    models, hit = {}, defaultdict(set)
    for enc, B, H, W, route in CASES:
        with monkeypatch.context() as mp:
            for k, v in ROUTES[route].items():
                mp.setenv(k, v)
            if (enc, route == "final") not in models:
                models[(enc, route == "final")] = DenseFeatureExtractor(make_args(model="adabins", encoder_name=enc,
                                                                                  do_final_upscale=route == "final")).eval()
            ext = models[(enc, route == "final")]
            _, facts, _ = predicted_plan(ext.decoder, getattr(ext.encoder.original_model, "conv_head", None), B, H, W)
            for k in facts:
                hit[k + ("" if hip_ops.conv_split_f16() else " (bf16 pairs)")].add((enc, B, H, W, route))
    missing = [k for k in REQUIRED if not hit.get(k)]
    assert not missing, (missing, sorted(hit))
    assert {c[4] for c in hit["split-K"]} == {"direct"}, hit["split-K"]
    print()
    for k in sorted(SEEN):
        if k.startswith("worst "):
            print(f"{k}: " + max(SEEN[k], key=lambda t: float(t.rsplit(": ", 1)[1].split(" of ")[0])))
