"""-m gpu: csrc/ground_plane.hip against Statement E on the CPU (tests/ground_plane_ref.py) -- the counts of every hypothesis, the nine
moments and the stats EQUAL, the pose within one fp32 step (equal bits expected; fallback rows and the exact zeros bit-equal) -- at
ragged shapes, with T = 1, 70, 256 and 1024, strides and filters, between poisoned guards, chained into the ground grid, inside a
captured graph, and (in a child process) through the predict path that carries it."""
import os
import subprocess
import sys

import pytest
import torch

import ground_grid_ref
import ground_plane_ref as ref
import test_hip_memory_bounds as bounds

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
POISON = 0x7FC0DEAD                       # a NaN payload no computation produces
FILTER = dict(near=ref.NEAR, far=ref.FAR)


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


_SCENES, _WANT = {}, {}


def scene(H, W, **kw):
    key = (H, W, tuple(sorted(kw.items())))
    if key not in _SCENES:
        _SCENES[key] = ref.scene(H, W, **kw)
    return _SCENES[key]


def reference(tag, sc, triples, prior, **kw):
    """The statement on a case, made once per ``tag`` and left unchanged."""
    if tag not in _WANT:
        _WANT[tag] = ref.ground_plane(sc.depth, sc.K, triples, prior, **kw)
    return _WANT[tag]


def poisoned(n, byte=0xAB):
    return {"pose": torch.full((n, 12), POISON, dtype=torch.int32, device="cuda").view(torch.float32),
            "stats": torch.full((n, 4), POISON ^ byte, dtype=torch.int32, device="cuda")}


def run(ops, sc, triples, prior, out=None, want=("pose", "stats", "count", "moments"), **kw):
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    return ops.ground_plane(sc.depth.cuda(), sc.K.cuda(), triples.cuda(), prior.cuda(), want=want, out=out, **dict(FILTER, **dev))


def fp32_steps(a, b):
    """The distance of two fp32 tensors in representable values (0: equal bits, or -0 against +0)."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


def check(got, want, prior, what=""):
    """``got``: the wrapper's dict against the reference's ``Plane``."""
    for name in ("count", "moments", "stats"):
        if name in got:
            g, w = got[name].cpu(), getattr(want, name)
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, tuple(g.shape))
            assert torch.equal(g, w), (what, name, int((g != w).sum()), "elements differ", g[g != w][:8].tolist(), w[g != w][:8].tolist())
    pose = got["pose"].cpu()
    assert not bool((pose.view(torch.int32) == POISON).any()), (what, "pose elements never written")
    steps = fp32_steps(pose, want.pose)
    print(what, "pose: entries that are not bit-equal", int((steps > 0).sum()), "worst distance in fp32 steps", int(steps.max()))
    assert int(steps.max()) <= 1, (what, "pose", int(steps.max()), "fp32 steps")
    ok = want.stats[:, 3] == 1
    assert torch.equal(pose[~ok].view(torch.int32), prior[~ok].view(torch.int32)), (what, "a fallback row is not the prior's bytes")
    assert torch.equal(pose[:, [3, 7]].view(torch.int32), want.pose[:, [3, 7]].view(torch.int32)), (what, "the exact zeros")


# ---------------------------------------------------------------------------
# equality with the statement
# ---------------------------------------------------------------------------
TABLES = ((70, (2, 3)), (256, (1, 1)))        # (T, stride): 70 is no multiple of 64 and goes with a stride, 256 with every pixel


@pytest.mark.parametrize("table", TABLES, ids=lambda t: f"T{t[0]}-stride{t[1][0]}x{t[1][1]}")
@pytest.mark.parametrize("shape", ref.CASE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counts_moments_stats_and_pose_equal_the_statement(ops, shape, table):
    """B = 3 scenes with 2 % noise; one image with a bad camera, NaN patches or no ground at all, rotating with the case.  Every output
    is poisoned first; a second call over another poison gives the same bytes."""
    (H, W), (T, stride) = shape, table
    n = ref.CASE_SHAPES.index(shape) * 2 + (T == 256)
    bad, kind = n % 3, ("camera", "nan", "wall")[(n // 2) % 3]
    sc = scene(H, W, noise=0.02, bad=bad, kind=kind, seed=n)
    triples, prior = ref.triples_of(H, W, T, seed=n), ref.level_prior()
    want = reference(("plain", shape, table), sc, triples, prior, stride=stride)
    assert int(want.stats[:, 3].sum()) >= 2 and int(want.count.max()) >= 64 and bool((want.valid.sum(1) > 0).sum() >= 2)
    if kind != "nan":
        assert want.stats[bad].tolist() == [-1, 0, 0, 0]
    out = poisoned(ref.CASE_B)
    got = run(ops, sc, triples, prior, out=out, stride=stride)
    assert got["pose"] is out["pose"] and got["stats"] is out["stats"] and tuple(got["count"].shape) == (ref.CASE_B, T)
    check(got, want, prior, (shape, table))
    first = {k: v.clone() for k, v in got.items()}
    again = run(ops, sc, triples, prior, out=poisoned(ref.CASE_B, byte=0x54), stride=stride)
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), again[k].view(torch.uint8)), (shape, table, k)


@pytest.mark.parametrize("table", TABLES, ids=lambda t: f"T{t[0]}-stride{t[1][0]}x{t[1][1]}")
@pytest.mark.parametrize("shape", ref.CASE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_confidence_and_std_filters(ops, shape, table):
    """Every shape x table of the plain test again, with the ``confidence`` map, the ``depth_std`` map and both: the hypotheses launch
    and the candidates read the maps.  The filters thin the triples' pixels too (a triple needs all three kept), hence min_inliers = 16."""
    (H, W), (T, stride) = shape, table
    sc = scene(H, W, noise=0.02, seed=5)
    triples, prior = ref.triples_of(H, W, T, seed=5), ref.level_prior()
    conf, std = ref.confidence_map(H, W), ref.confidence_map(H, W, seed=9)
    plain = reference(("unfiltered", shape, table), sc, triples, prior, stride=stride, min_inliers=16)
    for tag, kw in (("confidence", dict(confidence=conf, min_confidence=0.5)), ("std", dict(depth_std=std, max_std=0.5)),
                    ("both", dict(confidence=conf, min_confidence=0.25, depth_std=std, max_std=0.75))):
        kw = dict(dict(stride=stride, min_inliers=16), **kw)
        want = ref.ground_plane(sc.depth, sc.K, triples, prior, **kw)
        assert not torch.equal(want.count, plain.count) and int(want.stats[:, 3].sum()) >= 2, tag           # the filter matters here
        assert int(want.valid.sum()) < int(plain.valid.sum()), tag                                            # ... in the hypotheses too
        check(run(ops, sc, triples, prior, out=poisoned(ref.CASE_B), **kw), want, prior, (shape, table, tag))


@pytest.mark.parametrize("T,shape", [(1, (19, 70)), (1024, (37, 131))], ids=["T1", "T1024"])
def test_one_hypothesis_and_the_most_the_entry_point_takes(ops, T, shape):
    """T = 1: the table's only triple is planted on the ground of image 0, so the consensus has exactly one plane to score (and the
    padding hypotheses of the workspace stay out).  T = 1024: sixteen rounds of the on-chip count table."""
    H, W = shape
    sc = scene(H, W, noise=0.0, seed=3)
    triples = ref.triples_of(H, W, T, seed=8)
    if T == 1:
        triples = torch.tensor([[(H - 1) * W + 2, (H - 1) * W + W - 3, (H - 5) * W + W // 5]], dtype=torch.int32)
    prior = ref.level_prior()
    want = reference(("T", T), sc, triples, prior, min_inliers=16)
    assert int(want.stats[:, 3].sum()) >= 1 and int(want.valid.sum()) >= 1
    check(run(ops, sc, triples, prior, out=poisoned(ref.CASE_B), min_inliers=16), want, prior, ("T", T))
    with pytest.raises(ValueError):
        run(ops, sc, ref.triples_of(H, W, 1024).repeat(2, 1)[:1025], prior)


def test_points_beyond_256_metres_stay_out_of_the_moments(ops):
    """The scene ten times as large: the wall stands at 300 m and the far ground beyond 256 m, so inliers of the best plane are dropped
    from the integer moments (N < count) -- and the refit still finds the camera 16.5, 12 and 19 m up."""
    H, W = 37, 131
    sc = scene(H, W, noise=0.0, seed=9)
    big = ref.Scene((sc.depth * 10).contiguous(), sc.K, sc.truth)
    triples, prior = ref.triples_of(H, W, 70, seed=9), ref.level_prior(height=15.0)
    kw = dict(tol=0.5, rel_tol=0.01, height_range=(5.0, 40.0), near=0.5, far=1e4)
    want = ref.ground_plane(big.depth, big.K, triples, prior, **kw)
    assert want.stats[:, 3].tolist() == [1, 1, 1] and bool((want.stats[:, 2] < want.stats[:, 1]).all())
    assert float((ref.angles(want.pose)[0] - 10 * ref.angles(sc.truth)[0]).abs().max()) < 0.05
    check(run(ops, big, triples, prior, out=poisoned(ref.CASE_B), **kw), want, prior, "beyond 256 m")


def test_triples_outside_the_map_are_invalid_and_read_nothing(ops):
    H, W = 19, 70
    sc = scene(H, W, noise=0.0, seed=3)
    triples = ref.triples_of(H, W, 70, seed=2)
    triples[0, 1], triples[5, 0], triples[9, 2] = -1, H * W, 2 ** 31 - 1
    prior = ref.level_prior()
    want = ref.ground_plane(sc.depth, sc.K, triples, prior)
    assert not want.valid[:, [0, 5, 9]].any() and int(want.stats[:, 3].sum()) == 3
    check(run(ops, sc, triples, prior, out=poisoned(ref.CASE_B)), want, prior, "outside")


def test_a_duplicated_triple_picks_the_lower_index(ops):
    """The tie rule: the best triple of the plain run is copied to a LATER row and to an EARLIER one; the earlier copy must win."""
    H, W = 37, 131
    sc = scene(H, W, noise=0.02, seed=1)
    triples, prior = ref.triples_of(H, W, 70, seed=1), ref.level_prior()
    plain = ref.ground_plane(sc.depth, sc.K, triples, prior)
    best = int(plain.stats[0, 0])
    late, early = (best + 17) % 70, max(best - 1, 0) if best > 0 else None
    tied = triples.clone()
    tied[late] = triples[best]
    expect = min(best, late)
    if early is not None and early != best:
        tied[early] = triples[best]
        expect = min(expect, early)
    want = ref.ground_plane(sc.depth, sc.K, tied, prior)
    assert int(want.stats[0, 0]) == expect and int((want.count[0] == want.count[0].max()).sum()) >= 2
    got = run(ops, sc, tied, prior, out=poisoned(ref.CASE_B))
    check(got, want, prior, "tie")
    assert int(got["stats"][0, 0]) == expect


def test_too_few_inliers_gives_the_prior(ops):
    H, W = 21, 132
    sc = scene(H, W, noise=0.02, seed=2)
    triples, prior = ref.triples_of(H, W, 70, seed=2), ref.level_prior(height=1.4)
    free = ref.ground_plane(sc.depth, sc.K, triples, prior, stride=(2, 3))
    top = sorted(int(v) for v in free.stats[:, 1])
    floor = top[1] + 1                                                         # above two of the images' best counts, not the third's
    want = ref.ground_plane(sc.depth, sc.K, triples, prior, stride=(2, 3), min_inliers=floor)
    assert sorted(want.stats[:, 3].tolist()) == [0, 0, 1]
    got = run(ops, sc, triples, prior, out=poisoned(ref.CASE_B), stride=(2, 3), min_inliers=floor)
    check(got, want, prior, "min_inliers")
    lost = want.stats[:, 3] == 0
    assert torch.equal(got["pose"].cpu()[lost].view(torch.int32), prior[lost].view(torch.int32))
    assert got["stats"].cpu()[lost].tolist() == [[-1, 0, 0, 0]] * 2


def test_image_index_fills_a_batch_and_the_workspace_may_be_the_callers(ops):
    from objcavit_amd import _lib
    H, W = 21, 132
    sc = scene(H, W, noise=0.02, seed=4)
    triples, prior = ref.triples_of(H, W, 70, seed=4), ref.level_prior()
    d, k, t, p = sc.depth.cuda(), sc.K.cuda(), triples.cuda(), prior.cuda()
    whole = ops.ground_plane(d, k, t, p, out=poisoned(3), **FILTER)
    check(whole, reference("index", sc, triples, prior), prior, "whole batch")
    pick = [2, 0, 1]
    out = poisoned(3)
    need = int(_lib.load().ocv_ground_plane_workspace_bytes(1, 70))
    assert need == 16 * 72 + 72 + 4 * 70                                       # the header's layout: hypotheses, moments, counts
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for slot, i in enumerate(pick):
        got = ops.ground_plane(d[i:i + 1], k[i:i + 1], t, p[i:i + 1], out=out, image_index=slot, workspace=ws, want=("pose", "count"), **FILTER)
        assert got["pose"] is out["pose"] and "stats" not in got
        assert got["count"].untyped_storage().data_ptr() == ws.untyped_storage().data_ptr()
        assert torch.equal(got["count"].cpu()[0], _WANT["index"].count[i])
    for n in ("pose", "stats"):
        assert torch.equal(out[n].view(torch.uint8), whole[n][pick].contiguous().view(torch.uint8)), n
    with pytest.raises(ValueError):
        ops.ground_plane(d[:1], k[:1], t, p[:1], out=out, image_index=3, **FILTER)
    with pytest.raises(ValueError):
        ops.ground_plane(d, k, t, p, out={"pose": out["pose"]}, **FILTER)
    before = out["pose"].clone()
    with pytest.raises(_lib.HipLibraryError):
        ops.ground_plane(d, k, t, p, out=out, workspace=ws, **FILTER)         # too small for three images: refused, no launch
    torch.cuda.synchronize()
    assert torch.equal(out["pose"].view(torch.int32), before.view(torch.int32))


def test_bad_options_are_refused(ops):
    sc = scene(19, 70, noise=0.0, seed=3)
    d, k, t, p = sc.depth.cuda(), sc.K.cuda(), ref.triples_of(19, 70, 70).cuda(), ref.level_prior().cuda()
    for kw in (dict(want=()), dict(want=("pose", "depth")), dict(tol=-0.1), dict(rel_tol=float("nan")), dict(height_range=(2.0, 1.0)),
               dict(cos_tilt=0.0), dict(cos_tilt=1.5), dict(min_cross=0.0), dict(min_inliers=2), dict(stride=(0, 1)), dict(near=2.0, far=1.0)):
        with pytest.raises(ValueError):
            ops.ground_plane(d, k, t, p, **kw)
    with pytest.raises(ValueError):
        ops.ground_plane(d, k, t[:, :2].contiguous(), p)
    with pytest.raises(ValueError):
        ops.ground_plane(d, k, t, p[:, :9].contiguous())
    with pytest.raises(TypeError):
        ops.ground_plane(d, k, t.long(), p)
    with pytest.raises(ValueError):
        ops.ground_plane(torch.empty((1, 1, 2049, 2049), device="cuda"), k[:1], t, p[:1])        # more than 2^22 candidates


# ---------------------------------------------------------------------------
# guarded memory: a row of tests/test_hip_memory_bounds.py's table (its accounting test wants every *_fwd entry point in a row)
# ---------------------------------------------------------------------------
ROW = "ground_plane|19x70 T70"


def _plane_row(c):
    """19 x 70 (two candidate tiles, the second ragged; 70 hypotheses: two rounds of the count table, the second ragged), B = 3 with a
    bad camera, once at stride (1, 1) and once at (2, 3).  Every element of the outputs and every byte of the workspace is written."""
    H, W = 19, 70
    sc = scene(H, W, noise=0.02, bad=1, kind="camera", seed=6)
    triples, prior = ref.triples_of(H, W, 70, seed=6), ref.level_prior()
    d, k, t, p = c.put(sc.depth), c.put(sc.K), c.put(triples), c.put(prior)
    need = int(c.lib.ocv_ground_plane_workspace_bytes(ref.CASE_B, 70))
    for stride in ((1, 1), (2, 3)):
        want = reference(("guarded", stride), sc, triples, prior, stride=stride)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        ws.view(torch.int32).fill_(POISON)                                      # (a NaN payload: an invalid hypothesis is 0x7fc00000, not this)
        got = c.ops.ground_plane(d, k, t, p, stride=stride, workspace=ws, want=("pose", "stats", "count", "moments"), **FILTER)
        check(got, want, prior, ("guarded", stride))
        left = int((ws.view(torch.int32) == POISON).sum())
        assert left == 0, f"{left} word(s) of the workspace were never written (hypotheses, their padding, moments, counts)"
        views = c.ops.ground_plane_workspace_views(ws, ref.CASE_B, 70)
        hyp = views["hypotheses"].cpu()
        assert tuple(hyp.shape) == (ref.CASE_B, 72, 4) and bool(torch.isnan(hyp[:, 70:, 3]).all()) and not hyp[:, 70:, :3].any()
        assert torch.equal(torch.isnan(hyp[:, :70, 3]), ~want.valid), "the hypotheses marked invalid are the statement's"
        c.out(ws, got["pose"], got["stats"])


if ROW not in bounds.ROWS:
    bounds.row(ROW)(_plane_row)


def test_launches_between_poisoned_guards():
    bounds.run_row(ROW)
    assert "ocv_ground_plane_fwd" in bounds.RAN[ROW]


# ---------------------------------------------------------------------------
# the chain: the grid posed by the device's estimate
# ---------------------------------------------------------------------------
def test_ground_grid_fed_the_devices_pose_equals_statement_g_on_that_pose(ops):
    H, W = 37, 131
    sc = scene(H, W, noise=0.02, bad=2, kind="wall", seed=7)
    triples, prior = ref.triples_of(H, W, 256, seed=7), ref.level_prior()
    d, k = sc.depth.cuda(), sc.K.cuda()
    plane = ops.ground_plane(d, k, triples.cuda(), prior.cuda(), **FILTER)
    spec = ground_grid_ref.Spec(-7.9, 1.1, 0.25, 64, 48)
    got = ops.ground_grid(d, k, plane["pose"], tuple(spec), min_obstacle_points=1, **FILTER)          # no host read in between
    pose = plane["pose"].cpu()
    assert plane["stats"].cpu()[:, 3].tolist() == [1, 1, 0] and torch.equal(pose[2].view(torch.int32), prior[2].view(torch.int32))
    want = ground_grid_ref.ground_grid(sc.depth, sc.K, pose, spec, near=ref.NEAR, far=ref.FAR)
    assert int((want.state == 1).sum()) > 50 and int((want.state == 2).sum()) > 0
    for name in ground_grid_ref.OUTPUTS:
        g, w = got[name].cpu(), getattr(want, name)
        assert g.dtype == w.dtype and bool((g == w).all()), (name, int((g != w).sum()), "elements differ")


def test_captured_graph_replays_with_a_new_map_camera_and_prior():
    """In a fresh child process (tests/ground_plane_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "ground_plane_graph_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


def test_predict_path_carries_the_plane_and_poses_the_grid_with_it():
    """``Predictor`` and ``PipelinedPredictor`` with the keywords, in a fresh child process (tests/ground_plane_predict_child.py, which
    says what it checks) started with GPU_MAX_HW_QUEUES=4."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "ground_plane_predict_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
