"""Child process of tests/test_hip_ground_plane.py: the ground plane through the predict path -- ``Predictor`` and ``PipelinedPredictor``
with ``ground_plane={...}, ground_grid={"pose": "plane"}`` on the small model the point cloud's predict test uses.  ``result.plane``
equals the direct call on ``result.depth`` (and Statement E on it), ``result.ground`` equals the direct grid call on that pose (and
Statement G on it, read back), ``camera_pose=`` still wins, and every other field is the bytes it is without the keyword.  A process of
its own for the reason tests/ground_grid_predict_child.py gives (pipelines draw streams from torch's per-process pool).  Started fresh so
that the HIP runtime reads GPU_MAX_HW_QUEUES=4 at ITS start.  Prints OK when every part passed.

The small model's maps are no road scene (they lie around 2.5 m, bent), so the options are wide -- triples from every row, a tolerance
of 0.3 m + 10 %, any tilt below 1.5 rad -- for a plane to be found at all; what is checked is equality, not the plane's meaning."""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), HERE]

import torch  # noqa: E402

import ground_grid_ref  # noqa: E402
import ground_plane_ref as ref  # noqa: E402
from test_hip_point_cloud import PH, PW, _frames, _model_of  # noqa: E402

torch.set_grad_enabled(False)
PLANE = dict(hypotheses=70, rows=(0, PH), seed=2, tol=0.3, rel_tol=0.1, max_tilt=1.5, height_range=(-20.0, 20.0), min_inliers=32,
             height=1.2, pitch=0.3, stride=(4, 4))
GROUND = dict(cell=0.5, x_range=(-8.0, 8.0), y_range=(0.0, 16.0), band=(-6.0, 6.0), obstacle_height=0.1, min_points=2,
              min_obstacle_points=2, pose="plane")
ALL = ground_grid_ref.OUTPUTS


def _direct(ops, depth, K, args, B):
    """(the direct plane call on a map, the direct grid call posed by it): the package's own functions with the keywords' options."""
    from objcavit_amd.ground_grid import ground_grid
    from objcavit_amd.ground_plane import ground_plane
    ds = args[args.basic.dataset]
    rng = dict(near=float(ds.min_depth), far=float(ds.max_depth))
    plane = ground_plane(depth, K, **PLANE, **rng)
    grid = ground_grid(depth, K, plane.pose, **{k: v for k, v in GROUND.items() if k != "pose"}, **rng)
    return plane, grid


def _same_plane(a, b, what):
    assert torch.equal(a.pose.view(torch.int32), b.pose.view(torch.int32)), (what, "pose")
    assert torch.equal(a.stats, b.stats), (what, "stats")


def _same_grid(a, b, what):
    for n in ALL:
        assert torch.equal(getattr(a, n).view(torch.uint8), getattr(b, n).view(torch.uint8)), (what, n)


def _same_fields(a, b, what):
    for name in type(b)._fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if isinstance(x, torch.Tensor):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, name)


def predictor_plane_of_its_own_map(ops, model):
    from objcavit_amd.ground_grid import GroundGrid, ground_pose
    from objcavit_amd.ground_plane import GroundPlane, plane_triples
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import Predictor, PredictResult
    m, args = model
    ds = args[args.basic.dataset]
    frames = _frames(81, 2).cuda()
    K = intrinsics_from_focal([200.0, 150.25], PH, PW)
    K[1, 2] += 3.25
    want = ("depth", "depth_u16")
    plain = Predictor(m, args)(frames, want=want)
    pr = Predictor(m, args, ground_plane=PLANE, ground_grid=GROUND)
    res = pr(frames, intrinsics=K.cuda(), want=want)
    assert isinstance(res, PredictResult) and isinstance(res.plane, GroundPlane) and isinstance(res.ground, GroundGrid) and res.points is None
    assert tuple(res.plane.pose.shape) == (2, 12) and tuple(res.plane.stats.shape) == (2, 4) and res.plane.stats.dtype == torch.int32
    stats = res.plane.stats.cpu()
    print("stats through the predictor", stats.tolist())
    assert bool((stats[:, 3] == 1).any()), "no plane found on the small model's maps: the chain would be checked with the prior alone"
    # the direct calls on the same map: equal bytes
    plane, grid = _direct(ops, res.depth, K.cuda(), args, 2)
    _same_plane(res.plane, plane, "predictor / direct")
    _same_grid(res.ground, grid, "predictor / direct")
    # Statement E on the map, Statement G on the pose read back
    triples = plane_triples(PH, PW, PLANE["hypotheses"], PLANE["rows"], PLANE["seed"])
    prior = ground_pose(PLANE["height"], PLANE["pitch"], 0.0).expand(2, 12).contiguous()
    e = ref.ground_plane(res.depth.cpu(), K, triples, prior, tol=PLANE["tol"], rel_tol=PLANE["rel_tol"], height_range=PLANE["height_range"],
                         cos_tilt=math.cos(PLANE["max_tilt"]), min_inliers=PLANE["min_inliers"],
                         stride=PLANE["stride"], near=float(ds.min_depth), far=float(ds.max_depth))
    assert torch.equal(stats, e.stats), (stats.tolist(), e.stats.tolist())
    pose = res.plane.pose.cpu()
    steps = (pose.view(torch.int32).long() - e.pose.view(torch.int32).long()).abs()
    assert int(steps.max()) <= 1, ("pose against the statement", int(steps.max()))
    g = ground_grid_ref.ground_grid(res.depth.cpu(), K, pose, ground_grid_ref.Spec(-8.0, 0.0, 0.5, 32, 32), band=GROUND["band"],
                                    obstacle_height=0.1, min_points=2, min_obstacle_points=2, near=float(ds.min_depth), far=float(ds.max_depth))
    assert int(g.count.sum()) > 0
    for n in ALL:
        assert bool((getattr(res.ground, n).cpu() == getattr(g, n)).all()), ("grid against Statement G on the device's pose", n)
    # every other field is the bytes it is without the keywords
    _same_fields(res, plain, "with / without the keywords")
    # camera_pose= still wins over pose="plane"; the plane is estimated all the same
    other = ground_pose([1.0, 1.4], [0.35, 0.25], [0.0, -0.05])
    posed = pr(frames, intrinsics=K.cuda(), camera_pose=other, want=want)
    _same_plane(posed.plane, res.plane, "camera_pose")
    only_grid = Predictor(m, args, ground_grid={k: v for k, v in GROUND.items() if k != "pose"})(frames, intrinsics=K.cuda(), camera_pose=other)
    _same_grid(posed.ground, only_grid.ground, "camera_pose wins")
    # the plane alone; without intrinsics neither runs and the result is the plain tuple
    alone = Predictor(m, args, ground_plane=PLANE)(frames, intrinsics=K.cuda(), want=("depth_u16",))
    assert alone.depth is None and alone.ground is None
    _same_plane(alone.plane, res.plane, "plane alone")
    assert type(pr(frames)) is PredictResult


def pipelined_predictor_planes_equal_the_sequential_predictors(ops, model):
    """Four bs-1 steps over TWO slots: every step's plane and grid are bit-equal to the sequential ``Predictor``'s on a captured graph of
    the same shape, a step without intrinsics has neither, and the map is the bytes it is without the keywords."""
    import predict_ref
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args = model
    N = 4
    frames = [_frames(90 + i, 1).cuda() for i in range(N)]
    Ks = [intrinsics_from_focal(180.0 + 15.0 * i, PH, PW).cuda() for i in range(N)]
    pp = PipelinedPredictor(m, args, frames[0], slots=2, want=("depth",), ground_plane=PLANE, ground_grid=GROUND)
    example = predict_ref.frames_to_input(frames[0].cpu(), args, 0, 0, PH, PW)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_group=1, in_flight=2)
    seq = Predictor(g, args, ground_plane=PLANE, ground_grid=GROUND)
    off = Predictor(g, args)
    refs = []
    for i in range(N):
        r = seq(frames[i], intrinsics=Ks[i])
        refs.append((r.depth.clone(), r.plane.pose.clone(), r.plane.stats.clone(), {n: getattr(r.ground, n).clone() for n in ALL},
                     off(frames[i], intrinsics=Ks[i]).depth.clone()))
    for i in range(N):
        pp.submit(frames[i], intrinsics=Ks[i] if i % 2 else [Ks[i][0].cpu()])
    pp.submit(frames[0])
    got = pp.collect()
    assert len(got) == N + 1 and pp.rerun_steps == 0 and got[N].plane is None and got[N].ground is None
    for i in range(N):
        assert torch.equal(got[i].depth.view(torch.int32), refs[i][0].view(torch.int32)), i
        assert torch.equal(got[i].depth.view(torch.int32), refs[i][4].view(torch.int32)), i      # the keywords change no byte of the map
        assert torch.equal(got[i].plane.pose.view(torch.int32), refs[i][1].view(torch.int32)), i
        assert torch.equal(got[i].plane.stats, refs[i][2]), i
        for n in ALL:
            assert torch.equal(getattr(got[i].ground, n).view(torch.uint8), refs[i][3][n].view(torch.uint8)), (i, n)
    print("stats through the pipeline", [got[i].plane.stats.cpu().tolist() for i in range(N)])
    plane, grid = _direct(ops, got[1].depth, Ks[1], args, 1)
    _same_plane(got[1].plane, plane, "pipelined / direct")
    _same_grid(got[1].ground, grid, "pipelined / direct")


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    from objcavit_amd import hip_ops
    model = _model_of("nyu", PH, PW, 29)
    predictor_plane_of_its_own_map(hip_ops, model)
    pipelined_predictor_planes_equal_the_sequential_predictors(hip_ops, model)
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
