"""-m gpu: the validation loss on the device (csrc/metrics.hip: ocv_depth_metrics_loss_fwd) -- per-image SILog sums and 1-D
Chamfer terms from the same pass over the ground truth as the metric record -- against the float64 restatement tests/loss_ref.py
(pinned to the reference's own loss classes by the G11 fixtures, tests/test_val_loss_host.py), through the C ABI wrapper,
``ValidationStep(loss=True)`` and ``PipelinedValidation(loss=True)``.

Every comparison prints its worst deviation per field before it asserts (``pytest -s`` shows them; profiles/val_loss.txt keeps the
figures of one run)."""
import collections
import math

import numpy as np
import pytest
import torch

import gen
import loss_ref as lr
from objcavit_amd.config import make_args
from objcavit_amd.dp import LOSS_FIELDS, RECORD_FIELDS
from util import load_golden, rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TOL = 2e-5          # tests/test_hip_validation.py:12 -- fp32 per-pixel arithmetic; logf differs from the CPU's log by ulps
FLOAT_FIELDS = (0, 1, 3, 4)                      # mean_g, mean_g2, cham_x, cham_y (n_mask and image_id are exact)


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def dev(t):
    return None if t is None else t.to("cuda")


def field_devs(got, ref, note):
    """Worst relative deviation per loss field of a device table [B, 6] from the float64 one; counts and ids must be exact, and
    a field that is exactly 0 in the reference (an image without targets) must be exactly 0."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape == (ref.shape[0], len(LOSS_FIELDS)), (got.shape, ref.shape)
    assert torch.equal(got[:, 2], ref[:, 2]), (note, got[:, 2], ref[:, 2])
    assert torch.equal(got[:, 5], ref[:, 5]), (note, got[:, 5], ref[:, 5])
    out = {}
    for i in FLOAT_FIELDS:
        zero = ref[:, i] == 0
        assert torch.equal(got[zero, i], ref[zero, i]), (note, LOSS_FIELDS[i])
        d = ((got[~zero, i] - ref[~zero, i]).abs() / ref[~zero, i].abs())
        out[LOSS_FIELDS[i]] = float(d.max()) if d.numel() else 0.0
    print(f"[val_loss] {note}: " + "  ".join(f"{k} {v:.2e}" for k, v in out.items()))
    return out


def wide(rec, lrec):
    return torch.cat([rec, lrec], 1)


def brute_force_records(pred, mirror, gt, edges, dmin, dmax, first_image_id=0):
    """loss_ref's records with the Chamfer terms replaced by the float64 distance matrix (small cases only)."""
    ref = lr.loss_records(pred, mirror, gt, edges, dmin, dmax, first_image_id)
    c = lr.centres_of(edges).numpy()
    mask = lr.depth_mask(gt, dmin, dmax)
    for b in range(gt.shape[0]):
        t = gt[b].double()[mask[b]].numpy()
        if t.size:
            d = (c[b][:, None] - t[None, :]) ** 2
            ref[b, 3], ref[b, 4] = float(d.min(1).mean()), float(d.min(0).sum() / t.size)
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(lr.LOSS_CASES))
def test_g11_cases_vs_reference_classes(ops, tag):
    from objcavit_amd.validation import val_loss
    meta, z = load_golden(f"g11_val_loss_{tag}")
    gt, pa, pb, edges, dmin, dmax = lr.case_inputs(tag)
    B, H, W = meta["B"], meta["H"], meta["W"]
    box = (int(0.1 * H), int(0.9 * H), int(0.05 * W), int(0.95 * W))
    rec, lrec = ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges), dmin, dmax, crop=box, pred_mirror=dev(pb), first_image_id=7)
    assert rec.shape == (B, 10) and lrec.shape == (B, 6)
    pc = torch.from_numpy(z["pieces"])
    n = pc[:, 2].clamp(min=1.0)
    ref = torch.stack([pc[:, 0] / n, pc[:, 1] / n, pc[:, 2], pc[:, 3], pc[:, 4], torch.arange(7, 7 + B, dtype=torch.float64)], 1)
    devs = field_devs(lrec, ref, f"g11 {tag}")
    args = make_args()
    table = wide(rec, lrec)
    got_b, got_1 = val_loss(table, args, group=B), val_loss(table, args, group=1)
    lines = []
    for i, k in enumerate(("val/loss", "silog", "bins_chamfer")):
        want_b, want_1 = float(z["batch"][i]), float(z["single"][:, i].mean())
        lines.append((k, abs(got_b[k] - want_b) / want_b, abs(got_1[k] - want_1) / want_1))
    print(f"[val_loss] g11 {tag} recomposed (B-image call, mean of bs-1 calls): " + "  ".join(f"{k} {a:.2e} {b:.2e}" for k, a, b in lines)
          + "; the reference classes' own fp32 vs float64: " +
          "  ".join(f"{k} {abs(float(z['batch_fp32'][i]) - float(z['batch'][i])) / float(z['batch'][i]):.2e}"
                    for i, k in enumerate(("val/loss", "silog", "bins_chamfer"))))
    assert max(devs.values()) < TOL, devs
    assert all(a < TOL and b < TOL for _, a, b in lines), lines
    # metric half: bit-identical to the metric-only entry point, crop included; the whole call repeated is bit-equal
    assert torch.equal(rec, ops.depth_metrics(dev(pa), dev(gt), dmin, dmax, crop=box, pred_mirror=dev(pb), first_image_id=7))
    rec2, lrec2 = ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges), dmin, dmax, crop=box, pred_mirror=dev(pb), first_image_id=7)
    assert torch.equal(rec, rec2) and torch.equal(lrec, lrec2)
    # the crop is the metrics' alone
    _, lrec3 = ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges), dmin, dmax, crop=None, pred_mirror=dev(pb), first_image_id=7)
    assert torch.equal(lrec, lrec3)


@pytest.mark.parametrize("B,h,w,H,W,mirror,n_bins", [(1, 1, 1, 1, 1, False, 1), (2, 5, 7, 5, 7, True, 7), (3, 11, 13, 37, 29, True, 256),
                                                     (16, 240, 320, 480, 640, False, 256), (2, 30, 40, 31, 300, True, 1024),
                                                     (2, 176, 608, 352, 1216, True, 100)])
def test_depth_metrics_loss_vs_loss_ref(ops, B, h, w, H, W, mirror, n_bins):
    """Uniform noise on both sides (every interval between centres filled: the easy Chamfer case, all sizes); the prediction sits
    lower than the ground truth so that mean_g is well away from 0 and its relative deviation means something."""
    g = torch.Generator().manual_seed(B * 1000 + H)
    gt = torch.rand(B, 1, H, W, generator=g) * 12.0 - 1.0
    pa = torch.rand(B, 1, h, w, generator=g) * 4.0 + 0.1
    pb = torch.rand(B, 1, h, w, generator=g) * 4.0 + 0.1 if mirror else None
    if H == 1:
        gt[:] = 7.25
    if B > 1:
        gt[1] = -1.0                                   # an image without a single valid pixel
    edges = lr.clustered_edges(B, n_bins, 0.001, 10.0, H)
    box = (H // 4, H - H // 8, W // 8, W) if H > 8 else None
    rec, lrec = ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges), 0.001, 10.0, crop=box, pred_mirror=dev(pb), first_image_id=3)
    ref = lr.loss_records(pa, pb, gt, edges, 0.001, 10.0, first_image_id=3)
    devs = field_devs(lrec, ref, f"sweep B{B} {h}x{w}->{H}x{W} bins {n_bins}")
    assert max(devs.values()) < TOL, devs
    if B > 1:
        assert lrec[1, :5].tolist() == [0.0] * 5
    assert torch.equal(rec, ops.depth_metrics(dev(pa), dev(gt), 0.001, 10.0, crop=box, pred_mirror=dev(pb), first_image_id=3))
    again = ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges), 0.001, 10.0, crop=box, pred_mirror=dev(pb), first_image_id=3)
    assert torch.equal(again[0], rec) and torch.equal(again[1], lrec)


@pytest.mark.parametrize("how", ["shuffled", "equal_neighbours", "non_monotone"])
@pytest.mark.parametrize("tag", ["odd", "equal"])
def test_edges_in_any_order(ops, tag, how):
    """The ABI takes the edges as they come: the centres are the midpoints of CONSECUTIVE edges, then sorted on the device."""
    gt, pa, pb, edges, dmin, dmax = lr.case_inputs(tag)
    rs = np.random.RandomState(11)
    e = edges.clone()
    if how == "shuffled":
        for b in range(e.shape[0]):
            e[b] = e[b][torch.from_numpy(rs.permutation(e.shape[1]))]
    elif how == "equal_neighbours":
        e[:, 40:60] = e[:, 40:41]                      # twenty equal edges: nineteen equal centres
        e[:, 200] = e[:, 199]
    else:
        e[:, 1:-1] += torch.from_numpy(rs.uniform(-3e-2, 3e-2, (e.shape[0], e.shape[1] - 2)).astype(np.float32))
        assert bool((e[:, 1:] < e[:, :-1]).any())
    _, lrec = ops.depth_metrics_loss(dev(pa), dev(gt), dev(e), dmin, dmax, pred_mirror=dev(pb))
    ref = brute_force_records(pa, pb, gt, e, dmin, dmax)
    assert float(((ref - lr.loss_records(pa, pb, gt, e, dmin, dmax)).abs() / ref.abs().clamp(min=1e-300)).max()) < 1e-9
    devs = field_devs(lrec, ref, f"edges {how} {tag}")
    assert max(devs.values()) < TOL, devs


def test_nan_prediction_reaches_silog_of_its_image_only(ops):
    gt, pa, pb, edges, dmin, dmax = lr.case_inputs("nyu")
    rec0, lrec0 = ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges), dmin, dmax, pred_mirror=dev(pb))
    bad = pa.clone()
    bad[1, 0, 100, 100] = float("nan")
    assert bool(lr.depth_mask(gt, dmin, dmax)[1, 0, 200, 200])
    rec1, lrec1 = ops.depth_metrics_loss(dev(bad), dev(gt), dev(edges), dmin, dmax, pred_mirror=dev(pb))
    assert math.isnan(float(lrec1[1, 0])) and math.isnan(float(lrec1[1, 1]))           # no nan_to_num on the loss path
    assert torch.equal(lrec1[1, 2:], lrec0[1, 2:])                                     # its count and Chamfer fields untouched
    assert torch.equal(lrec1[[0, 2]], lrec0[[0, 2]])                                   # the other images untouched
    assert torch.equal(rec1, ops.depth_metrics(dev(bad), dev(gt), dmin, dmax, pred_mirror=dev(pb)))   # the metrics' nan -> min_depth
    assert not bool(torch.isnan(rec1).any())


def test_nan_edge_is_a_centre_at_infinity(ops):
    """A NaN edge (a diverged bin head) makes two NaN centres; they are taken as +inf: cham_x of that image is inf, its cham_y is
    that of the remaining centres, the other image is untouched and the call still repeats bit for bit."""
    gt, pa, pb, edges, dmin, dmax = lr.case_inputs("odd")
    _, lrec0 = ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges), dmin, dmax, pred_mirror=dev(pb))
    bad = edges.clone()
    bad[0, 100] = float("nan")
    _, lrec1 = ops.depth_metrics_loss(dev(pa), dev(gt), dev(bad), dmin, dmax, pred_mirror=dev(pb))
    _, lrec2 = ops.depth_metrics_loss(dev(pa), dev(gt), dev(bad), dmin, dmax, pred_mirror=dev(pb))
    assert torch.equal(lrec1, lrec2)
    assert torch.equal(lrec1[1], lrec0[1]) and torch.equal(lrec1[0, :3], lrec0[0, :3])
    assert math.isinf(float(lrec1[0, 3])) and float(lrec1[0, 3]) > 0
    c = lr.centres_of(edges)[0]
    keep = torch.ones(c.numel(), dtype=torch.bool)
    keep[99:101] = False                                                   # the centres on either side of edge 100
    t = gt[0].double()[lr.depth_mask(gt, dmin, dmax)[0]].numpy()
    want = lr.chamfer_1d(c[keep].numpy(), t)[1]
    assert abs(float(lrec1[0, 4]) - want) <= TOL * want


def test_argument_checks(ops):
    gt, pa, pb, edges, dmin, dmax = lr.case_inputs("odd")
    with pytest.raises(ValueError):
        ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges[:1]), dmin, dmax)
    with pytest.raises(ValueError):
        ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges[:, :1]), dmin, dmax)
    with pytest.raises(ValueError):
        ops.depth_metrics_loss(dev(pa), dev(gt), dev(lr.clustered_edges(2, 1025, dmin, dmax, 1)), dmin, dmax)
    with pytest.raises(ValueError):
        ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges), -0.5, dmax)
    with pytest.raises(TypeError):
        ops.depth_metrics_loss(dev(pa), dev(gt), dev(edges.double()), dmin, dmax)
    with pytest.raises(Exception):
        ops.depth_metrics_loss(dev(pa), dev(gt), edges, dmin, dmax)                   # edges on the CPU


# ---------------------------------------------------------------------------------------------------------------------------------
Out = collections.namedtuple("Out", ["depth_pred", "bin_edges"])


class Toy(torch.nn.Module):
    """The stand-in of tests/test_hip_validation.py with bin edges that follow from the image (the mirror's differ)."""

    def __init__(self, with_edges=True):
        super().__init__()
        self.with_edges = with_edges

    def forward(self, image):
        d = image[:, :1, ::2, ::2].abs() * 3.0 + torch.linspace(0.5, 4.0, image.shape[3] // 2, device=image.device)
        if not self.with_edges:
            return Out(d.contiguous(), None)
        wdt = image[:, 0, 0, :32].abs() + 0.05
        wdt = wdt / wdt.sum(1, keepdim=True)
        e = torch.cat([torch.full_like(wdt[:, :1], 0.001), 0.001 + torch.cumsum((10.0 - 0.001) * wdt, 1)], 1)
        return Out(d.contiguous(), e.contiguous())


def _check_step(model, args, img, gt, note, **kw):
    """ValidationStep(loss=True) against loss_ref on the step's OWN device outputs (copied to the CPU), and against loss=False."""
    from objcavit_amd.validation import ValidationStep
    on, off = ValidationStep(model, args, loss=True, **kw), ValidationStep(model, args, loss=False, **kw)
    rec, out = on(img, gt, first_image_id=10)
    edges = out.bin_edges.clone()
    assert rec.shape == (img.shape[0], len(RECORD_FIELDS) + len(LOSS_FIELDS))
    rec_off, _ = off(img, gt, first_image_id=10)
    assert rec_off.shape == (img.shape[0], 10) and torch.equal(rec[:, :10], rec_off)
    if kw.get("flip_tta", True):
        o, mirror = on._forward_pair(img)
        pred, mirror = o.depth_pred.clone().cpu(), mirror.clone().cpu()
    else:
        pred, mirror = on._call(img).depth_pred.clone().cpu(), None
    ds = args[args.basic.dataset]
    ref = lr.loss_records(pred, mirror, gt.cpu(), edges.cpu(), float(ds.min_depth), float(ds.max_depth), first_image_id=10)
    devs = field_devs(rec[:, 10:], ref, note)
    assert max(devs.values()) < TOL, devs
    return rec


@pytest.mark.parametrize("flip_tta", [True, False])
def test_validation_step_loss_on_the_toy_model(flip_tta):
    from objcavit_amd.validation import ValidationStep, val_loss
    args = make_args()
    img = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda()
    gt = (torch.rand(2, 1, 64, 96, generator=torch.Generator().manual_seed(2)) * 9.0 + 0.5).cuda()
    gt[:, :, :3] = 0.0
    m = Toy()
    assert not torch.equal(m(img).bin_edges, m(img.flip(dims=[3])).bin_edges)
    rec = _check_step(m, args, img, gt, f"toy flip_tta={flip_tta}", flip_tta=flip_tta)
    assert math.isfinite(val_loss(rec, args)["val/loss"])
    with pytest.raises(ValueError, match="bin_edges"):
        ValidationStep(Toy(with_edges=False), args, flip_tta=flip_tta, loss=True)(img, gt)


@pytest.mark.parametrize("joint", [True, False])
@pytest.mark.parametrize("model", ["adabins", "graphbins"])
def test_validation_step_loss_on_a_mini_model(model, joint):
    from objcavit_amd.modules.AdaBins import AdaBins
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    H, W, B, seed = 352, 384, 2, 41
    args = make_args(model=model, language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    m = (AdaBins(args) if model == "adabins" else GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5))).eval()
    gen.load_into(m, seed, gen.PEAKY)
    m = m.cuda()
    img = gen.randn("img", (B, 3, H, W), seed).cuda()
    gt = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(6)) * 3.0 + 0.5).cuda()
    gt[:, :, ::7] = 0.0
    _check_step(m, args, img, gt, f"mini {model} joint={joint}", joint=joint)


def test_pipelined_validation_with_the_loss():
    """Four slots, eight bs-1 steps on distinct images: the metric columns do not move when the loss is switched on, and the loss
    columns follow the sequential step's exactly as far as the metric columns do -- a slot whose static bin_edges were overwritten
    by its next replay before the loss launch read them would carry another image's Chamfer fields."""
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    from objcavit_amd.validation import PipelinedValidation, ValidationStep
    H, W, B, N = 352, 384, 1, 8
    args = make_args(language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    m = GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=5)).eval()
    gen.load_into(m, 29, gen.PEAKY)
    m = m.cuda()
    imgs = [gen.randn(f"im{i}", (B, 3, H, W), 300 + i).cuda() for i in range(N)]
    gts = [(torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(i)) * 3.0 + 0.5).cuda() for i in range(N)]
    seq = ValidationStep(m, args, joint=True, loss=True)
    ref = torch.cat([seq(imgs[i], gts[i], first_image_id=i)[0] for i in range(N)], 0)
    cham = ref[:, 13:15].cpu()
    assert len({tuple(r.tolist()) for r in cham}) == N                     # distinct images: distinct Chamfer fields
    pv = PipelinedValidation(m, args, imgs[0])
    assert len(pv.graphs) == 4 and pv.loss is False
    for i in range(N):
        pv.submit(imgs[i], gts[i], first_image_id=i)
    off = pv.collect()
    assert off.shape == (N, 10)
    pv.loss = True                                                         # the same pipeline, the same captured graphs
    for i in range(N):
        pv.submit(imgs[i], gts[i], first_image_id=i)
    on = pv.collect()
    assert on.shape == (N, 16) and pv.collect().shape == (0, 16)
    assert torch.equal(on[:, :10], off)
    assert torch.equal(on[:, [8, 9, 12, 15]], ref[:, [8, 9, 12, 15]])      # counts and ids exact
    same = [bool(torch.equal(on[i, :10], ref[i, :10])) for i in range(N)]
    print(f"[val_loss] pipelined vs sequential: metric columns bit-equal in {sum(same)} of {N} rows; "
          f"loss columns rel dev {max(rel_dev(on[:, c], ref[:, c]) for c in (10, 11, 13, 14)):.2e}, "
          f"metric columns {rel_dev(on[:, :8], ref[:, :8]):.2e}")
    for i in range(N):
        if same[i]:
            assert torch.equal(on[i], ref[i]), i
    assert rel_dev(on[:, :8], ref[:, :8]) < 1e-5                           # the bar of test_pipelined_validation_equals_the_sequential_step
    for c in (10, 11, 13, 14):
        assert rel_dev(on[:, c], ref[:, c]) < 1e-5, LOSS_FIELDS[c - 10]
    pv2 = PipelinedValidation(m, args, imgs[0], slots=2, loss=True)        # the constructor's switch
    pv2.submit(imgs[0], gts[0], first_image_id=0)
    one = pv2.collect()
    assert one.shape == (1, 16) and torch.equal(one[:, [8, 9, 12, 15]], on[:1, [8, 9, 12, 15]])
    assert all(rel_dev(one[:, c], on[:1, c]) < 1e-5 for c in (10, 11, 13, 14))
