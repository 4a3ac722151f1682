"""-m "not gpu": Statement E itself (tests/ground_plane_ref.py) -- does the consensus and its one refit recover the pose the scenes were
rendered from --, the host half of objcavit_amd/ground_plane.py (``plane_triples``, ``pose_angles``), and what the ``ground_plane`` /
``ground_grid=dict(pose="plane")`` keywords ask of ``hip_ops``, pinned with recorders in the wrappers' place as
tests/test_predict_steps_host.py does."""
import math

import pytest
import torch

import ground_plane_ref as ref
from objcavit_amd import hip_ops, predict
from objcavit_amd.config import make_args
from objcavit_amd.ground_grid import ground_pose
from objcavit_amd.ground_plane import cos_of_tilt, plane_triples, pose_angles
from test_predict_steps_host import H, W, K_SRC, _drive, _Recorder, _shifted, _step_inputs

# (T, stride) of the issue: 70 is no multiple of 64 and goes with a stride, 256 with every pixel
TABLES = ((70, (2, 3)), (256, (1, 1)))
SEEDS = (0, 1, 2)


def _errors(noise, **kw):
    """The worst |height|, |pitch|, |roll| error over the shapes x tables x seeds, every image of every scene."""
    worst = [0.0, 0.0, 0.0]
    for Hc, Wc in ref.CASE_SHAPES:
        for T, stride in TABLES:
            for seed in SEEDS:
                sc = ref.scene(Hc, Wc, noise=noise, seed=seed)
                got = ref.ground_plane(sc.depth, sc.K, ref.triples_of(Hc, Wc, T, seed), ref.level_prior(), stride=stride, **kw)
                assert got.stats[:, 3].tolist() == [1, 1, 1], (Hc, Wc, T, seed, got.stats.tolist())
                assert int(got.valid.sum(1).min()) >= T // 2                   # nothing is degenerate: most triples span a usable plane
                for i, (a, b) in enumerate(zip(ref.angles(got.pose), ref.angles(sc.truth))):
                    worst[i] = max(worst[i], float((a - b).abs().max()))
    return worst


def test_noise_free_scenes_recover_the_pose():
    """tol = 0.02, rel_tol = 0: height within 5 mm, pitch and roll within 5e-4 rad.  Measured on this statement over the three shapes x
    two tables x three seeds: 3.5 mm, 2.6e-4 rad, 4.2e-5 rad (the coordinates are quantised to 1 / 128 m for the integer moments, and
    the smallest case fits 150 points)."""
    h, p, r = _errors(0.0, tol=0.02, rel_tol=0.0)
    print("noise-free: height", h, "pitch", p, "roll", r)
    assert h <= 5e-3 and p <= 5e-4 and r <= 5e-4, (h, p, r)


def test_two_percent_noise_recovers_the_pose_with_the_default_tolerances():
    """2 % multiplicative noise, tol = 0.05, rel_tol = 0.01: height within 0.15 m, pitch and roll within 0.015 rad.  Measured on this
    statement over the same cases: 0.079 m, 8.4e-3 rad, 4.0e-3 rad."""
    h, p, r = _errors(0.02)
    print("2 % noise: height", h, "pitch", p, "roll", r)
    assert h <= 0.15 and p <= 0.015 and r <= 0.015, (h, p, r)


def test_on_a_perfect_plane_the_pose_is_ground_poses():
    """Rows 0 and 1 follow ``ground_pose``'s convention: the refit of a noise-free scene is that matrix, not merely its plane."""
    sc = ref.scene(37, 131)
    got = ref.ground_plane(sc.depth, sc.K, ref.triples_of(37, 131, 256), ref.level_prior(), tol=0.02, rel_tol=0.0)
    assert float((got.pose - sc.truth).abs().max()) <= 5e-3
    assert bool((got.pose[:, 3] == 0).all()) and bool((got.pose[:, 7] == 0).all())


def test_pose_angles_is_the_inverse_of_ground_pose():
    h, p, r = [1.65, 0.8, 2.5, 1.0], [0.0, 0.3, -0.2, 0.07], [0.0, -0.1, 0.25, -0.03]
    gh, gp, gr = pose_angles(ground_pose(h, p, r))
    assert gh.dtype == torch.float64 and tuple(gh.shape) == (4,)
    for got, want in ((gh, h), (gp, p), (gr, r)):
        assert float((got - torch.tensor(want, dtype=torch.float64)).abs().max()) <= 1e-6          # the pose is fp32
    one = pose_angles(ground_pose(1.2, 0.1, 0.0)[0])
    assert all(tuple(v.shape) == (1,) for v in one) and abs(float(one[1]) - 0.1) <= 1e-6
    # and the test's own inverse agrees with the package's
    for a, b in zip(ref.angles(ground_pose(h, p, r)), (gh, gp, gr)):
        assert torch.equal(a, b)


def test_plane_triples_is_a_function_of_its_arguments_and_stays_inside_its_rows():
    a, b = plane_triples(37, 131, 70, seed=4), plane_triples(37, 131, 70, seed=4)
    assert a.dtype == torch.int32 and tuple(a.shape) == (70, 3) and torch.equal(a, b) and a.device.type == "cpu"
    assert not torch.equal(a, plane_triples(37, 131, 70, seed=5))
    assert tuple(plane_triples(480, 640).shape) == (256, 3)
    y = a // 131
    assert int(y.min()) >= 37 // 2 and int(y.max()) < 37 and int((a % 131).max()) < 131 and int(a.min()) >= 0
    assert len(set(y.view(-1).tolist())) == 37 - 37 // 2                              # every row of the lower half is drawn from
    rows = plane_triples(37, 131, 256, rows=(5, 9), seed=1) // 131
    assert int(rows.min()) == 5 and int(rows.max()) == 8
    for bad in (dict(T=0), dict(T=1025), dict(rows=(9, 9)), dict(rows=(0, 38)), dict(rows=(-1, 4))):
        with pytest.raises(ValueError):
            plane_triples(37, 131, **bad)
    with pytest.raises(ValueError):
        plane_triples(0, 131)


def test_an_all_wall_scene_gives_the_priors_bytes():
    """No ground in sight: every hypothesis is vertical (beyond max_tilt) or none has min_inliers -> ok = 0, the pose is the prior bit
    for bit; the other two images are estimated as ever."""
    sc = ref.scene(21, 132, bad=1, kind="wall")
    prior = ref.level_prior(height=1.5)
    got = ref.ground_plane(sc.depth, sc.K, ref.triples_of(21, 132, 70), prior)
    assert got.stats[1].tolist() == [-1, 0, 0, 0] and got.stats[:, 3].tolist() == [1, 0, 1]
    assert torch.equal(got.pose[1].view(torch.int32), prior[1].view(torch.int32))
    assert not torch.equal(got.pose[0], prior[0])
    # a non-finite prior: no hypothesis is valid, and the output is that prior (NaN included), bit for bit
    broken = prior.clone()
    broken[2, 3] = float("nan")
    got = ref.ground_plane(sc.depth, sc.K, ref.triples_of(21, 132, 70), broken)
    assert got.stats[2].tolist() == [-1, 0, 0, 0] and not got.valid[2].any()
    assert torch.equal(got.pose[2].view(torch.int32), broken[2].view(torch.int32))


# ---------------------------------------------------------------------------
# the keywords
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def args():
    return make_args(dataset="kitti")


def test_bad_options_are_refused(args):
    for bad in (dict(hypotheses=0), dict(hypotheses=1025), dict(hypotheses=2.5), dict(rows=(4, 4)), dict(tol=-1.0), dict(rel_tol=float("inf")),
                dict(max_tilt=2.0), dict(max_tilt=-0.1), dict(height_range=(2.0, 1.0)), dict(min_cross=0.0), dict(min_inliers=2),
                dict(height=float("nan")), dict(stride=0), dict(near=3.0, far=1.0), dict(cell=0.1)):
        with pytest.raises(ValueError):
            predict._Ends(args, ground_plane=bad)
    with pytest.raises(ValueError):
        cos_of_tilt(math.pi / 2)
    o = predict._Ends(args, ground_plane={}).plane
    assert o["hypotheses"] == 256 and o["rows"] is None and o["seed"] == 0 and (o["tol"], o["rel_tol"]) == (0.05, 0.01)
    assert o["cos_tilt"] == math.cos(0.35) and o["height_range"] == (0.5, 4.0) and o["min_inliers"] == 64 and o["stride"] == (1, 1)
    assert torch.equal(o["prior"], ground_pose(1.65, 0.0, 0.0))


def test_pose_plane_needs_the_ground_plane_keyword(args):
    with pytest.raises(ValueError, match="ground_plane"):
        predict._Ends(args, ground_grid={"pose": "plane"})
    with pytest.raises(ValueError):
        predict._Ends(args, ground_grid={"pose": "imu"}, ground_plane={})
    ends = predict._Ends(args, ground_grid={"pose": "plane"}, ground_plane={})
    assert ends.ground["pose_from"] == "plane" and predict._Ends(args, ground_grid={}, ground_plane={}).ground["pose_from"] is None
    assert [r.keyword for r in predict.READOUTS][-2:] == ["ground_plane", "ground_grid"] and len(predict.READOUTS) == 6


class _PlaneRecorder(_Recorder):
    """tests/test_predict_steps_host.py's recorder, with a stand-in for ``hip_ops.ground_plane`` as well."""

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        monkeypatch.setattr(hip_ops, "ground_plane", self.ground_plane)

    def ground_plane(self, depth, K, triples, prior, confidence=None, depth_std=None, out=None, image_index=0, **kw):
        self.calls.append(("ground_plane", dict(self._per_frame(depth, K, confidence, depth_std, image_index), triples=triples,
                                                prior=prior.tolist(), prior_storage=prior.untyped_storage().data_ptr(),
                                                names=tuple(sorted(out)), options=kw)))
        self.plane = out
        return out

    def ground_grid(self, depth, K, pose, grid, **kw):
        self.grid_pose = getattr(self, "grid_pose", []) + [pose]
        return super().ground_grid(depth, K, pose, grid, **kw)


def test_the_plane_runs_in_front_of_the_grid_and_hands_it_its_pose_tensor(args, monkeypatch):
    rec = _PlaneRecorder(monkeypatch)
    frames, out, mirror = _step_inputs(stats=True)
    kw = dict(surface_normals={}, ground_plane={"hypotheses": 70, "seed": 3, "max_std": 2.0, "stride": (2, 3), "pitch": 0.05},
              ground_grid={"pose": "plane", "want": ("state",)})
    ends, res = _drive(args, kw, out, mirror, frames, ("depth",), intrinsics=K_SRC)
    assert rec.names() == ["depth_finalize", "depth_normals", "depth_normals", "ground_plane", "ground_plane", "ground_grid", "ground_grid"]
    assert rec.of("depth_finalize")[0]["want"] == ("depth", "depth_std")               # the plane's finite max_std makes that map
    table = plane_triples(H, W, 70, seed=3)
    prior = ground_pose(1.65, 0.05, 0.0)
    for i in range(2):
        c = rec.of("ground_plane")[i]
        assert (c["image_index"], c["depth"], c["K"], c["confidence"], c["depth_std"]) == (i, (i, 1), _shifted(i), None, (i, 1))
        assert torch.equal(c["triples"], table) and c["prior"] == prior.tolist() and c["names"] == ("pose", "stats")
        o = c["options"]
        assert (o["tol"], o["rel_tol"], o["stride"], o["min_inliers"], o["max_std"]) == (0.05, 0.01, (2, 3), 64, 2.0)
        assert o["cos_tilt"] == math.cos(0.35) and o["height_range"] == (0.5, 4.0) and o["near"] == ends.min_depth
        # the grid reads the plane's OWN tensor: image i's rows of the buffer the plane's launches write
        g = rec.grid_pose[i]
        assert g.untyped_storage().data_ptr() == rec.plane["pose"].untyped_storage().data_ptr()
        assert (g.storage_offset(), tuple(g.shape)) == (12 * i, (1, 12))
    assert res.plane.pose is rec.plane["pose"] and tuple(res.plane.pose.shape) == (2, 12)
    assert res.plane.stats is rec.plane["stats"] and res.plane.stats.dtype == torch.int32 and tuple(res.plane.stats.shape) == (2, 4)
    assert res.ground.state is not None and res.points is None
    assert res._replace(bin_edges=None).plane is res.plane
    # the table of triples (per device and map size) and the prior (per device and batch size) are made once per ``_Ends`` and kept:
    # a second step of the SAME ends hands the wrapper the same two tensors, and new output buffers
    first = rec.of("ground_plane")
    rec.calls.clear()
    step = ends.step(ends.frames_of(frames, "frames_u8"), intrinsics=K_SRC)
    again = ends.finish(out, mirror, step, 0, ("depth",))
    second = rec.of("ground_plane")
    assert len(second) == 2 and all(c["triples"] is first[0]["triples"] for c in first + second)
    assert second[0]["prior_storage"] == first[0]["prior_storage"] and again.plane.pose is not res.plane.pose
    assert [k for k in ends._on(torch.device("cpu"), False) if k[0] in ("plane_triples", "plane_prior")] == [("plane_triples", H, W), ("plane_prior", 2)]


def test_camera_pose_wins_and_without_the_option_the_grid_keeps_its_own_pose(args, monkeypatch):
    rec = _PlaneRecorder(monkeypatch)
    frames, out, mirror = _step_inputs(stats=False)
    pose = torch.arange(24, dtype=torch.float32).reshape(2, 12)
    kw = dict(ground_plane={}, ground_grid={"pose": "plane"})
    _drive(args, kw, out, mirror, frames, (), intrinsics=K_SRC, camera_pose=pose)
    assert rec.names() == ["depth_finalize", "ground_plane", "ground_plane", "ground_grid", "ground_grid"]
    assert [c["pose"] for c in rec.of("ground_grid")] == [pose[i:i + 1].tolist() for i in range(2)]
    rec.calls.clear()
    ends, res = _drive(args, dict(ground_plane={}, ground_grid={"height": 1.2}), out, mirror, frames, (), intrinsics=K_SRC)
    assert [c["pose"] for c in rec.of("ground_grid")] == [ends.ground["pose"].reshape(1, 12).tolist()] * 2 and res.plane is not None
    # the plane alone: intrinsics are kept for it, and without them nothing runs
    rec.calls.clear()
    ends, res = _drive(args, dict(ground_plane={}), out, mirror, frames, ("depth_u16",), intrinsics=K_SRC)
    assert rec.names() == ["depth_finalize", "ground_plane", "ground_plane"] and res.ground is None and res.depth is None
    rec.calls.clear()
    ends, res = _drive(args, kw, out, mirror, frames, ("depth_u16",))
    assert rec.names() == ["depth_finalize"] and res.plane is None and res.ground is None
