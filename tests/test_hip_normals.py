"""-m gpu: csrc/surface_normals.hip against Statement N in torch (tests/normals_ref.py) -- the validity mask EQUAL element for element
(the statement fixes every rounding of the predicate), the normals within an angle bar of the fp64 normals, the picture within one
LSB -- the gather against plain indexing, both launches between poisoned guards and inside a captured graph, and the predict path
that carries them."""
import os
import subprocess
import sys

import pytest
import torch

import mem_guard
import normals_ref as ref
import point_cloud_ref
import test_hip_memory_bounds as bounds

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
POISON = 0x7FC0DEAD                       # a NaN payload no computation produces
ALL = ("normals", "rgb8", "valid")

# The largest angle between the kernel's normal and the fp64 statement over the maps of this file (every shape of SHAPES, every radius,
# every choice of the bad camera), measured on an MI355X by tools/normals_measure.py (profiles/normals.txt (a)); the bar is 8 x that --
# the margin covers another summation order and the fp32 normalisation -- and may never exceed 1e-3 rad: each planted error of
# tests/test_normals_host.py moves at least 1 % of the pixels by more than 1e-2 rad.
ANGLE_MEASURED = 3.182e-05          # rad: 37 x 131, r = 1 (profiles/normals.txt (a)); the bar is 2.546e-04
ANGLE_BAR = 8.0 * ANGLE_MEASURED
assert 0.0 < ANGLE_BAR <= 1e-3
LENGTH_TOL = 1e-6

SHAPES = ref.CASE_SHAPES + ref.VECTOR_SHAPES


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


_CASES = {}


def case(H, W, r, bad="rotate"):
    """(depth, K, the reference's Normals) on the host, made once per (shape, radius, bad camera).  "rotate": image r % 3 has the bad
    camera, so over the four radii every image is seen with a good camera at least twice."""
    bad = r % 3 if bad == "rotate" else bad
    key = (H, W, r, bad)
    if key not in _CASES:
        depth, K = ref.case(H, W, bad_camera=bad)
        _CASES[key] = (depth, K, ref.normals(depth, K, r))
    return _CASES[key]


def poisoned(n, H, W, names=ALL, byte=0xAB):
    out = {}
    if "normals" in names:
        out["normals"] = torch.full((n, 3, H, W), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    if "rgb8" in names:
        out["rgb8"] = torch.full((n, H, W, 3), byte, dtype=torch.uint8, device="cuda")
    if "valid" in names:
        out["valid"] = torch.full((n, H, W), byte, dtype=torch.uint8, device="cuda")
    return out


def check(got, want, what=""):
    """``got``: the wrapper's dict (any subset of the outputs), ``want``: the reference's Normals.  -> the largest angle seen."""
    v = want.valid
    worst = 0.0
    if "valid" in got:
        mask = got["valid"].cpu()
        assert mask.dtype == torch.uint8 and torch.equal(mask, v.to(torch.uint8)), (what, "valid differs from the reference")
    if "normals" in got:
        raw = got["normals"].cpu()
        assert not bool((raw.view(torch.int32) == POISON).any()), (what, "elements of normals never written")
        n = raw.double()
        assert not raw.permute(0, 2, 3, 1)[~v].view(torch.int32).any(), (what, "an invalid pixel's normal is not (+0, +0, +0)")
        if bool(v.any()):
            ang = ref.angle(n, want.normals)[v]
            length = (n.norm(dim=1) - 1).abs()[v]
            worst = float(ang.max())
            print(f"{what}: {int(v.sum())} valid, max angle {worst:.3e} rad (bar {ANGLE_BAR:.3e}), max ||n| - 1| {float(length.max()):.3e}")
            assert worst < ANGLE_BAR, (what, worst)
            assert float(length.max()) <= LENGTH_TOL, (what, float(length.max()))
    if "rgb8" in got:
        pic = got["rgb8"].cpu()
        assert pic.dtype == torch.uint8 and not pic[~v].any(), (what, "an invalid pixel's colour is not (0, 0, 0)")
        diff = (pic.int() - want.rgb8.int()).abs()
        assert int(diff.max()) <= 1, (what, int(diff.max()))
        if bool(v.any()):
            assert bool((pic[v].int().sum(-1) > 0).all()), (what, "a valid pixel's colour is (0, 0, 0)")       # 127.5 (n + 1) is 0 for n = -1 only
    return worst


# ---------------------------------------------------------------------------
# the dense launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("r", ref.RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_outputs_equal_the_reference(ops, shape, r):
    """B = 3: a step / plane, a model-like map with NaN, +-inf and out-of-range cells, a sphere; one image with a bad camera.  8 x 8 has no
    valid pixel at r = 4, 9 x 9 exactly one (image 0); 19 x 70 and 37 x 131 cross tile edges in both axes (131 = 2 x 64 + 3), W % 4 != 0:
    the scalar stores; 21 x 132: the vector stores over three tiles, the last four columns wide."""
    H, W = shape
    depth, K, want = case(H, W, r)
    bad = r % 3
    assert not want.valid[bad].any()
    if shape == (8, 8) and r == 4:
        assert not want.valid.any()
    if shape == (9, 9) and r == 4:
        assert int(want.valid[0].sum()) == 1 and bool(want.valid[0, 4, 4])
    out = poisoned(ref.CASE_B, H, W)
    got = ops.depth_normals(depth.cuda(), K.cuda(), radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE, want=ALL, out=out)
    assert all(got[k] is out[k] for k in ALL)
    check(got, want, (shape, r))
    # every element is written: a second call over another poison gives the same bytes
    again = ops.depth_normals(depth.cuda(), K.cuda(), radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE, want=ALL,
                              out=poisoned(ref.CASE_B, H, W, byte=0x54))
    for k in ALL:
        a, b = got[k], again[k]
        assert torch.equal(a.view(torch.int32) if k == "normals" else a, b.view(torch.int32) if k == "normals" else b), (shape, r, k)


@pytest.mark.parametrize("bad", [None, 0, 1, 2])
def test_every_choice_of_the_bad_camera(ops, bad):
    H, W, r = 19, 70, 2
    depth, K, want = case(H, W, r, bad)
    assert [bool(want.valid[i].any()) for i in range(3)] == [i != bad for i in range(3)]
    check(ops.depth_normals(depth.cuda(), K.cuda(), radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE, want=ALL,
                            out=poisoned(3, H, W)), want, ("bad camera", bad))
    for i, v in ((1, -2.0), (1, float("inf")), (2, float("nan")), (3, float("-inf")), (0, 0.0)):
        k = ref.intrinsics(H, W)
        k[0, i] = v
        got = ops.depth_normals(depth.cuda(), k.cuda(), radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE, want=("valid", "normals"))
        assert not got["valid"][0].any() and not got["normals"][0].any(), (i, v)


COMBOS = [("normals",), ("rgb8",), ("valid",), ("normals", "rgb8"), ("normals", "valid"), ("rgb8", "valid")]          # (all three: ``full``)


@pytest.mark.parametrize("shape,r", [((19, 70), 4), ((37, 131), 2), ((21, 132), 3)], ids=lambda v: str(v))
def test_every_combination_of_outputs(ops, shape, r):
    H, W = shape
    depth, K, want = case(H, W, r)
    d, k = depth.cuda(), K.cuda()
    kw = dict(radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE)
    full = ops.depth_normals(d, k, want=ALL, out=poisoned(3, H, W), **kw)
    for names in COMBOS:
        out = poisoned(3, H, W, names)
        got = ops.depth_normals(d, k, want=names, out=out, **kw)
        assert set(got) == set(names)
        check(got, want, (shape, r, names))
        for n in names:
            assert torch.equal(got[n].view(torch.uint8), full[n].view(torch.uint8)), (shape, r, names, n)
    with pytest.raises(ValueError):
        ops.depth_normals(d, k, want=(), **kw)
    with pytest.raises(ValueError):
        ops.depth_normals(d, k, want=("normals", "depth"), **kw)
    with pytest.raises(ValueError):
        ops.depth_normals(d, k, radius=5)


def test_thresholds_are_inclusive_and_the_defaults_take_every_finite_depth(ops):
    """z exactly at near / far passes, the next fp32 beyond fails; near = 0, far = inf (the wrapper's defaults) take any finite depth."""
    H, W, r = 12, 16, 1
    base = ref.plane(H, W, 1e-5, 1e-5, 0.5)                                     # ~2 m
    z = base.clone()
    z[3, 3], z[3, 9], z[8, 4], z[8, 11] = 1.9, float(torch.nextafter(torch.tensor(1.9), torch.tensor(0.0))), 2.05, \
        float(torch.nextafter(torch.tensor(2.05), torch.tensor(9.0)))
    depth = z.view(1, 1, H, W)
    K = ref.intrinsics(H, W, 1)
    want = ref.normals(depth, K, r, near=1.9, far=2.05, edge_ratio=0.2)
    assert bool(want.valid[0, 3, 3]) and not bool(want.valid[0, 3, 9]) and bool(want.valid[0, 8, 4]) and not bool(want.valid[0, 8, 11])
    check(ops.depth_normals(depth.cuda(), K.cuda(), radius=r, near=1.9, far=2.05, edge_ratio=0.2, want=ALL), want, "inclusive")
    wide = depth.clone()
    wide[0, 0, 5, 5] = 3.0e4
    want = ref.normals(wide, K, r, near=0.0, far=float("inf"), edge_ratio=1e9)
    assert int(want.valid.sum()) == (H - 2) * (W - 2)
    got = ops.depth_normals(wide.cuda(), K.cuda(), radius=r, edge_ratio=1e9, want=("valid",))
    assert torch.equal(got["valid"].cpu().bool(), want.valid)


def test_two_calls_are_bit_equal_and_image_index_fills_a_batch(ops):
    H, W, r = 37, 131, 3
    depth, K, want = case(H, W, r, None)
    d, k = depth.cuda(), K.cuda()
    kw = dict(radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE, want=ALL)
    a = ops.depth_normals(d, k, out=poisoned(3, H, W), **kw)
    b = ops.depth_normals(d, k, out=poisoned(3, H, W), **kw)
    for n in ALL:
        assert torch.equal(a[n].view(torch.uint8), b[n].view(torch.uint8)), n
    # a batch of three filled by three calls, in another order: image i of the case lands in slot pick.index(i)
    pick = [2, 0, 1]
    out = poisoned(3, H, W)
    for slot, i in enumerate(pick):
        got = ops.depth_normals(d[i:i + 1], k[i:i + 1], out=out, image_index=slot, **kw)
        assert got["normals"] is out["normals"]
    for n in ALL:
        assert torch.equal(out[n].view(torch.uint8), a[n][pick].contiguous().view(torch.uint8)), n
    with pytest.raises(ValueError):
        ops.depth_normals(d[:1], k[:1], out=out, image_index=3, **kw)
    with pytest.raises(ValueError):
        ops.depth_normals(d, k, out={"normals": out["normals"]}, **kw)           # rgb8 and valid are wanted too
    fresh = ops.depth_normals(d, k, **kw)                                        # without ``out`` the buffers are new
    for n in ALL:
        assert torch.equal(fresh[n].view(torch.uint8), a[n].view(torch.uint8)), n


# ---------------------------------------------------------------------------
# the gather
# ---------------------------------------------------------------------------
def _cloud(ops, depth, K, cap, stride):
    return ops.depth_unproject(depth, K, cap, stride=stride, near=ref.NEAR, far=ref.FAR, want_pixel=True)


@pytest.mark.parametrize("stride,cap", [((1, 1), 37 * 131), ((2, 3), 900), ((1, 1), 300), ((3, 2), 1)])
def test_gather_equals_indexing_and_leaves_the_tail_alone(ops, stride, cap):
    """Capacities above the total, below it (the cloud is cut: counts = cap), 300 (two workgroups, the second ragged) and 1."""
    H, W, r = 37, 131, 2
    depth, K, want = case(H, W, r, None)
    d, k = depth.cuda(), K.cuda()
    normals = ops.depth_normals(d, k, radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE)["normals"]
    cloud = _cloud(ops, d, k, cap, stride)
    counts = cloud["counts"].tolist()
    assert max(counts) > 0 and (cap >= 900 or min(cloud["total"].tolist()) > cap)
    out = torch.full((3, cap, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    got = ops.normals_gather(normals, cloud["pixel"], cloud["counts"], out=out)
    assert got is out
    flat = normals.flatten(2).cpu()
    res, pixel = out.cpu(), cloud["pixel"].cpu()
    seen_valid = seen_invalid = 0
    for b, n in enumerate(counts):
        idx = pixel[b, :n].long()
        assert torch.equal(res[b, :n, :3].view(torch.int32), flat[b][:, idx].t().contiguous().view(torch.int32)), (b, "rows differ")
        assert not res[b, :n, 3].view(torch.int32).any(), (b, "the fourth component is not +0")
        assert bool((res[b, n:].view(torch.int32) == POISON).all()), (b, "rows beyond counts were written")
        hit = want.valid[b].flatten()[idx]
        seen_valid += int(hit.sum())
        seen_invalid += int((~hit).sum())
        assert not res[b, :n][~hit].any()                                      # a kept point at an invalid pixel carries zeros
    if cap > 1:
        assert seen_valid > 0 and seen_invalid > 0
    again = ops.normals_gather(normals, cloud["pixel"], cloud["counts"])
    for b, n in enumerate(counts):
        assert torch.equal(again[b, :n].view(torch.int32), out[b, :n].view(torch.int32))


def test_gather_takes_counts_above_the_capacity_and_bad_indices(ops):
    H, W = 9, 9
    normals = torch.arange(2 * 3 * H * W, dtype=torch.float32).view(2, 3, H, W).cuda() + 1.0
    pixel = torch.tensor([[0, 80, 81, -1, 40], [7, 7, 2 ** 31 - 1, 3, 0]], dtype=torch.int32).cuda()
    counts = torch.tensor([9, -3], dtype=torch.int32).cuda()                      # above the capacity: clamped; negative: nothing
    out = torch.full((2, 5, 4), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    ops.normals_gather(normals, pixel, counts, out=out)
    res = out.cpu()
    flat = normals.flatten(2).cpu()
    assert torch.equal(res[0, 0, :3], flat[0][:, 0]) and torch.equal(res[0, 1, :3], flat[0][:, 80]) and torch.equal(res[0, 4, :3], flat[0][:, 40])
    assert not res[0, 2].any() and not res[0, 3].any()                            # an index outside the map: zeros
    assert bool((res[1].view(torch.int32) == POISON).all())
    with pytest.raises(ValueError):
        ops.normals_gather(normals, pixel[:1], counts)
    with pytest.raises(ValueError):
        ops.normals_gather(normals[:, :2], pixel, counts)


# ---------------------------------------------------------------------------
# guarded memory: rows of tests/test_hip_memory_bounds.py's table (its accounting test wants every *_fwd entry point in a row)
# ---------------------------------------------------------------------------
def _normals_row(c):
    """19 x 70, r = 4, B = 3: 2 x 2 tiles, both ragged.  Every element of every output is written (``c.out``)."""
    H, W, r = 19, 70, 4
    depth, K, want = case(H, W, r)
    got = c.ops.depth_normals(c.put(depth), c.put(K), radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE, want=ALL)
    assert torch.equal(got["valid"].cpu().bool(), want.valid)
    assert float(ref.angle(got["normals"].cpu().double(), want.normals)[want.valid].max()) < ANGLE_BAR
    assert int((got["rgb8"].cpu().int() - want.rgb8.int()).abs().max()) <= 1
    c.out(got["normals"], got["rgb8"], got["valid"])
    alone = c.ops.depth_normals(c.put(depth), c.put(K), radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE, want=("rgb8",))
    c.out(alone["rgb8"])


def _gather_row(c):
    """The gather behind a cloud of the same 19 x 70 map, capacities above and below the totals; rows at or beyond counts[b] are
    documented as NOT written: they must still hold the harness's pattern."""
    H, W, r = 19, 70, 4
    depth, K, _ = case(H, W, r, None)
    dg, kg = c.put(depth), c.put(K)
    normals = c.ops.depth_normals(dg, kg, radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE)["normals"]
    c.out(normals)
    for cap in (H * W, 257):
        cloud = c.ops.depth_unproject(dg, kg, cap, near=ref.NEAR, far=ref.FAR, want_pixel=True)
        got = c.ops.normals_gather(normals, cloud["pixel"], cloud["counts"]).cpu()
        flat, pixel = normals.flatten(2).cpu(), cloud["pixel"].cpu()
        for b, n in enumerate(cloud["counts"].tolist()):
            assert torch.equal(got[b, :n, :3].view(torch.int32), flat[b][:, pixel[b, :n].long()].t().contiguous().view(torch.int32))
            assert bool((got[b, n:].view(torch.int32) == mem_guard._PATTERN_I32).all())
        c.out(cloud["counts"], cloud["total"])


for _name, _fn in (("depth_normals|19x70 r4", _normals_row), ("normals_gather|19x70", _gather_row)):
    if _name not in bounds.ROWS:
        bounds.row(_name)(_fn)


@pytest.mark.parametrize("name", ["depth_normals|19x70 r4", "normals_gather|19x70"])
def test_both_launches_between_poisoned_guards(name):
    bounds.run_row(name)
    assert {"depth_normals|19x70 r4": "ocv_depth_normals_fwd", "normals_gather|19x70": "ocv_normals_gather_fwd"}[name] in bounds.RAN[name]


def test_captured_graph_replays_with_a_new_map_and_new_cameras():
    """In a fresh child process (tests/normals_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "normals_graph_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


# ---------------------------------------------------------------------------
# the predict path
# ---------------------------------------------------------------------------
from test_hip_point_cloud import PH, PW, _frames, _model_of  # noqa: E402


@pytest.fixture(scope="module")
def model():
    return _model_of("nyu", PH, PW, 29)


def _same(a, b, what=""):
    """Two SurfaceNormals on the device: every tensor equal bit for bit (points: the rows the caller names)."""
    for name in ("normals", "rgb8", "valid"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, name)


def _against_reference(res, K_window, opts, what):
    """``res.normals`` against Statement N applied to the result's own depth with the window's K."""
    want = ref.normals(res.depth.cpu(), K_window, opts["radius"], near=opts["near"], far=opts["far"], edge_ratio=opts["edge_ratio"])
    got = {"normals": res.normals.normals, "rgb8": res.normals.rgb8, "valid": res.normals.valid}
    check({k: v for k, v in got.items() if v is not None}, want, what)
    return want


def test_predictor_normals_of_its_own_map(ops, model):
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import Predictor, PredictResult
    from objcavit_amd.surface_normals import SurfaceNormals, surface_normals
    m, args = model
    ds = args[args.basic.dataset]
    frames = _frames(81, 2).cuda()
    K = intrinsics_from_focal([518.8579, 300.25], PH, PW)
    K[1, 2] += 3.25
    opts = dict(radius=3, edge_ratio=0.2, near=float(ds.min_depth), far=float(ds.max_depth))
    pr = Predictor(m, args, surface_normals=dict(radius=3, edge_ratio=0.2, picture=True, valid=True))
    res = pr(frames, intrinsics=K.cuda())
    assert isinstance(res, PredictResult) and isinstance(res.normals, SurfaceNormals) and res.points is None and res.objects is None
    assert tuple(res.normals.normals.shape) == (2, 3, PH, PW) and tuple(res.normals.rgb8.shape) == (2, PH, PW, 3)
    assert tuple(res.normals.valid.shape) == (2, PH, PW) and res.normals.points is None
    want = _against_reference(res, K, opts, "nyu window")
    assert 0 < int(want.valid.sum()) and not want.valid[:, :3].any() and not want.valid[:, :, -3:].any()
    # the stand-alone function on the same map gives the same bits
    alone = surface_normals(res.depth, K.cuda(), picture=True, valid=True, **opts)
    _same(res.normals, alone)
    # the map is made for the normals even when it is not wanted -- and then not handed out; without the mask / picture they are None
    u16 = Predictor(m, args, surface_normals=dict(radius=3, edge_ratio=0.2))(frames, want=("depth_u16",), intrinsics=[K[0].tolist(), K[1]])
    assert u16.depth is None and u16.depth_u16 is not None and u16.normals.rgb8 is None and u16.normals.valid is None
    assert torch.equal(u16.normals.normals.view(torch.int32), res.normals.normals.view(torch.int32))
    # without intrinsics, or without the keyword, there are no normals and the result is the plain tuple
    assert type(pr(frames)) is PredictResult and Predictor(m, args)(frames, intrinsics=K.cuda()).normals is None
    with pytest.raises(ValueError):
        pr(frames, intrinsics=K[:1].cuda())


def test_predictor_cloud_rows_carry_their_normals(ops, model):
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import Predictor
    m, args = model
    frames = _frames(83, 2).cuda()
    K = intrinsics_from_focal([450.0, 380.5], PH, PW).cuda()
    stride = (2, 3)
    pr = Predictor(m, args, point_cloud=dict(normals=True, stride=stride), surface_normals=dict(edge_ratio=0.2))
    res = pr(frames, intrinsics=K)
    gh, gw = ops.unproject_grid(PH, PW, stride)
    cap = gh * gw
    assert res.points.pixel is None and tuple(res.points.points.shape) == (2, cap, 4) and tuple(res.normals.points.shape) == (2, cap, 4)
    # the cloud is what it is without the normals; its pixel index (asked for) addresses the rows' normals
    plain = Predictor(m, args, point_cloud=dict(stride=stride, pixel=True))(frames, intrinsics=K)
    assert torch.equal(plain.points.counts, res.points.counts) and plain.normals is None
    flat = res.normals.normals.flatten(2)
    hits = 0
    for b, n in enumerate(res.points.counts.tolist()):
        assert n > 0 and torch.equal(plain.points.points[b, :n].view(torch.int32), res.points.points[b, :n].view(torch.int32))
        rows = flat[b][:, plain.points.pixel[b, :n].long()].t().contiguous()
        assert torch.equal(res.normals.points[b, :n, :3].view(torch.int32), rows.view(torch.int32)), b
        assert not res.normals.points[b, :n, 3].any()
        hits += int((rows.abs().sum(1) > 0).sum())
    assert hits > 0
    # normals=True alone implies the keyword's defaults; pixel=True hands the index out as well
    implied = Predictor(m, args, point_cloud=dict(normals=True, stride=stride, pixel=True))(frames, intrinsics=K)
    assert implied.normals is not None and implied.normals.points is not None and torch.equal(implied.points.pixel, plain.points.pixel)
    ds = args[args.basic.dataset]
    direct = ops.depth_normals(implied.depth, K, radius=2, near=float(ds.min_depth), far=float(ds.max_depth), edge_ratio=0.05)["normals"]
    assert torch.equal(implied.normals.normals.view(torch.int32), direct.view(torch.int32))


def test_predictor_takes_kitti_frames_of_different_sizes(ops):
    """Two frames of different sizes, each cropped to 352 x 1216 by its own origin: one launch per frame, the principal point of each
    shifted by ITS origin."""
    from objcavit_amd.predict import Predictor, kb_crop_origin
    KH, KW = 352, 1216
    m, args = _model_of("kitti", KH, KW, 27)
    ds = args[args.basic.dataset]
    frames = [_frames(31, 1, 375, 1242)[0].cuda(), _frames(32, 1, 370, 1224)[0].cuda()]
    K = torch.tensor([[721.5377, 721.5377, 609.5593, 172.854], [718.856, 718.856, 607.1928, 185.2157]])
    opts = dict(radius=2, edge_ratio=0.3, near=float(ds.min_depth), far=float(ds.max_depth))
    pr = Predictor(m, args, surface_normals=dict(radius=2, edge_ratio=0.3, valid=True))
    ops.enable_timing(True)
    res = pr(frames, intrinsics=K.cuda())
    timings = ops.timing_results()
    ops.enable_timing(False)
    assert timings["depth_normals"][0] == 2                                        # one launch per frame
    shifted = torch.stack([point_cloud_ref.shift_intrinsics(K[i:i + 1], *kb_crop_origin(*f.shape[:2]))[0] for i, f in enumerate(frames)], 0)
    assert not torch.equal(shifted[0, 2:] - K[0, 2:], shifted[1, 2:] - K[1, 2:])
    want = _against_reference(res, shifted, opts, "kitti list")
    assert all(int(want.valid[i].sum()) > 0 for i in range(2))


def test_predictor_with_a_resize_window(ops):
    from objcavit_amd.predict import Predictor, fit_window
    from test_hip_resize_ingest import MH, MW, _model, _rand_frames
    m, args = _model()
    ds = args[args.basic.dataset]
    frames = _rand_frames(61, 2, 250, 300).cuda()
    top, left, Hw, Ww = fit_window(250, 300, MH, MW)
    K = torch.tensor([[280.0, 285.0, 149.5, 124.5], [300.0, 300.0, 140.0, 130.0]])                         # of the 250 x 300 frames
    opts = dict(radius=4, edge_ratio=0.25, near=float(ds.min_depth), far=float(ds.max_depth))
    pr = Predictor(m, args, crop=(top, left, Hw, Ww), resize=(MH, MW), surface_normals=dict(radius=4, edge_ratio=0.25, picture=True, valid=True))
    res = pr(frames, intrinsics=K)
    assert tuple(res.depth.shape) == (2, 1, Hw, Ww) and tuple(res.normals.normals.shape) == (2, 3, Hw, Ww)
    want = _against_reference(res, point_cloud_ref.shift_intrinsics(K, top, left), opts, "resize window")
    assert int(want.valid.sum()) > 0


def test_pipelined_predictor_normals_equal_the_sequential_predictors(ops, model):
    """Four bs-1 steps over TWO slots: every step's normals (and the normals of its cloud's rows) are bit-equal to the sequential
    ``Predictor``'s on a captured graph of the same shape; a step without intrinsics has none."""
    import predict_ref
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args = model
    N = 4
    frames = [_frames(90 + i, 1).cuda() for i in range(N)]
    Ks = [intrinsics_from_focal(400.0 + 25.0 * i, PH, PW).cuda() for i in range(N)]
    cloud = dict(stride=(2, 2), near=0.5, far=7.0, normals=True)
    opts = dict(radius=2, edge_ratio=0.2, picture=True, valid=True)
    pp = PipelinedPredictor(m, args, frames[0], slots=2, want=("depth",), point_cloud=cloud, surface_normals=opts)
    example = predict_ref.frames_to_input(frames[0].cpu(), args, 0, 0, PH, PW)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_group=1, in_flight=2)
    seq = Predictor(g, args, point_cloud=cloud, surface_normals=opts)
    refs = []
    for i in range(N):
        r = seq(frames[i], intrinsics=Ks[i])
        refs.append((r.depth.clone(), type(r.normals)(*(t.clone() for t in r.normals)), r.points.counts.clone()))
    for i in range(N):
        pp.submit(frames[i], intrinsics=Ks[i] if i % 2 else [Ks[i][0].cpu()])
    pp.submit(frames[0])
    got = pp.collect()
    assert len(got) == N + 1 and pp.rerun_steps == 0 and got[N].normals is None and got[N].points is None
    for i in range(N):
        assert torch.equal(got[i].depth.view(torch.int32), refs[i][0].view(torch.int32)), i
        _same(got[i].normals, refs[i][1], i)
        n = int(refs[i][2][0])
        assert torch.equal(got[i].points.counts, refs[i][2]) and n > 0
        assert torch.equal(got[i].normals.points[0, :n].view(torch.int32), refs[i][1].points[0, :n].view(torch.int32)), i
        assert bool(got[i].normals.valid.any())
