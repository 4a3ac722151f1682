"""Child process of tests/test_hip_ground_grid.py: the ground grid through the predict path -- ``Predictor`` and ``PipelinedPredictor``
with the ``ground_grid`` keyword on the small model the normals' predict test uses.  ``result.ground`` equals Statement G
(tests/ground_grid_ref.py) applied to ``result.depth``; ``camera_pose=`` overrides the keyword's pose; without ``intrinsics=`` there is
no grid; with the keyword absent the results are the bytes they were.  A process of its own, because these steps build pipelines:
slots, captured graphs and streams drawn from torch's per-process stream pool.  Which pool stream (and so which hardware queue) a later
``torch.cuda.Stream()`` of the suite's process gets depends on how many were drawn before it, and the suite's forked-graph replays on
two streams (tests/test_hip_models.py) have only ever run with the pool as the earlier files leave it.  Started fresh so that the HIP
runtime reads GPU_MAX_HW_QUEUES=4 at ITS start.  Prints OK when every part passed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), HERE]

import pytest  # noqa: E402
import torch  # noqa: E402

import ground_grid_ref as ref  # noqa: E402
import point_cloud_ref  # noqa: E402
from test_hip_point_cloud import PH, PW, _frames, _model_of  # noqa: E402

torch.set_grad_enabled(False)
POISON = 0x7FC0DEAD
ALL = ref.OUTPUTS
INT = ("count", "obstacle", "state")


def check(got, want, what=""):
    """``got``: the wrapper's dict (any subset of the outputs) against the reference's Grid: EQUAL."""
    for name, t in got.items():
        g, w = t.cpu(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, tuple(g.shape))
        if name in INT:
            assert torch.equal(g, w), (what, name, int((g != w).sum()), "elements differ")
        else:
            assert not bool((g.view(torch.int32) == POISON).any()), (what, name, "elements never written")
            assert bool((g == w).all()), (what, name, int((g != w).sum()), "elements differ")      # by value: -0 == +0, inf == inf, no NaN


# the small model's maps lie within nyu's 10 m: a coarse grid that covers them, a wide band, the camera pitched down
GROUND = dict(cell=0.5, x_range=(-8.0, 8.0), y_range=(0.0, 16.0), height=1.2, pitch=0.3, roll=0.02, band=(-6.0, 6.0), obstacle_height=0.1,
              min_points=2, min_obstacle_points=2)


def _statement(res, K_window, pose, args, **kw):
    from objcavit_amd.ground_grid import grid_of as host_grid
    ds = args[args.basic.dataset]
    o = dict(GROUND, **kw)
    spec = ref.Spec(*host_grid(o["cell"], o["x_range"], o["y_range"]))
    return ref.ground_grid(res.depth.cpu(), K_window, pose, spec, band=o["band"], obstacle_height=o["obstacle_height"],
                           min_points=o["min_points"], min_obstacle_points=o["min_obstacle_points"], near=float(ds.min_depth),
                           far=float(ds.max_depth), stride=o.get("stride", (1, 1)))


def _as_dict(g):
    return {n: getattr(g, n) for n in ALL if getattr(g, n) is not None}


def predictor_grid_of_its_own_map(ops, model):
    from objcavit_amd.ground_grid import GroundGrid, ground_grid, ground_pose
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import Predictor, PredictResult
    m, args = model
    frames = _frames(81, 2).cuda()
    K = intrinsics_from_focal([200.0, 150.25], PH, PW)
    K[1, 2] += 3.25
    plain = Predictor(m, args)(frames)
    pr = Predictor(m, args, ground_grid=GROUND)
    res = pr(frames, intrinsics=K.cuda())
    assert isinstance(res, PredictResult) and isinstance(res.ground, GroundGrid) and res.points is None and res.normals is None
    assert (res.ground.x0, res.ground.y0, res.ground.cell) == (-8.0, 0.0, 0.5) and tuple(res.ground.count.shape) == (2, 32, 32)
    assert tuple(res.ground.first_occupied.shape) == (2, 32)
    pose = ground_pose(GROUND["height"], GROUND["pitch"], GROUND["roll"]).expand(2, 12).contiguous()
    want = _statement(res, K, pose, args)
    print("points in the grid", int(want.count.sum()), "occupied cells", int((want.state == 2).sum()))
    assert int(want.count.sum()) > 0
    check(_as_dict(res.ground), want, "keyword's pose")
    # with the keyword the map is the bytes it was without it
    assert torch.equal(res.depth.view(torch.int32), plain.depth.view(torch.int32))
    # the stand-alone function on the same map gives the same bits
    ds = args[args.basic.dataset]
    alone = ground_grid(res.depth, K.cuda(), pose, cell=0.5, x_range=(-8.0, 8.0), y_range=(0.0, 16.0), band=GROUND["band"],
                        obstacle_height=0.1, min_points=2, min_obstacle_points=2, near=float(ds.min_depth), far=float(ds.max_depth))
    for n in ALL:
        assert torch.equal(getattr(alone, n).view(torch.uint8), getattr(res.ground, n).view(torch.uint8)), n
    # camera_pose= overrides the keyword's pose, per image
    other = ground_pose([1.0, 1.4], [0.35, 0.25], [0.0, -0.05])
    posed = pr(frames, intrinsics=K.cuda(), camera_pose=other)
    want_posed = _statement(posed, K, other, args)
    check(_as_dict(posed.ground), want_posed, "camera_pose")
    assert not torch.equal(want_posed.count, want.count)
    listed = pr(frames, intrinsics=K.cuda(), camera_pose=[other[0].view(3, 4), other[1].tolist()])
    assert torch.equal(listed.ground.count, posed.ground.count)
    # a subset of the outputs, a stride; the map is made for the grid even when it is not wanted -- and then not handed out
    sub = Predictor(m, args, ground_grid=dict(GROUND, want=("state", "first_occupied"), stride=(2, 2)))(frames, want=("depth_u16",),
                                                                                                       intrinsics=K.cuda())
    assert sub.depth is None and sub.depth_u16 is not None and sub.ground.count is None and sub.ground.h_mean is None
    check(_as_dict(sub.ground), _statement(res, K, pose, args, stride=(2, 2)), "subset")
    # without intrinsics, or without the keyword, there is no grid and the result is the plain tuple
    assert type(pr(frames)) is PredictResult and type(pr(frames, camera_pose=other)) is PredictResult
    assert Predictor(m, args)(frames, intrinsics=K.cuda(), camera_pose=other).ground is None
    with pytest.raises(ValueError):
        pr(frames, intrinsics=K.cuda(), camera_pose=other[:1])


def predictor_shifts_the_camera_by_each_frames_window(ops):
    """Two KITTI frames of different sizes, each cropped by its own origin: one call per frame, the principal point of each shifted by
    ITS origin, exactly as the cloud's."""
    from objcavit_amd.ground_grid import ground_pose
    from objcavit_amd.predict import Predictor, kb_crop_origin
    KH, KW = 352, 1216
    m, args = _model_of("kitti", KH, KW, 27)
    ds = args[args.basic.dataset]
    frames = [_frames(31, 1, 375, 1242)[0].cuda(), _frames(32, 1, 370, 1224)[0].cuda()]
    K = torch.tensor([[721.5377, 721.5377, 609.5593, 172.854], [718.856, 718.856, 607.1928, 185.2157]])
    opts = dict(cell=0.5, x_range=(-10.0, 10.0), y_range=(0.0, 40.0), height=1.65, pitch=0.05, band=(-3.0, 3.0), obstacle_height=0.3)
    pr = Predictor(m, args, ground_grid=opts)
    ops.enable_timing(True)
    res = pr(frames, intrinsics=K.cuda())
    timings = ops.timing_results()
    ops.enable_timing(False)
    assert timings["ground_grid"][0] == 2                                          # one call per frame
    shifted = torch.stack([point_cloud_ref.shift_intrinsics(K[i:i + 1], *kb_crop_origin(*f.shape[:2]))[0] for i, f in enumerate(frames)], 0)
    pose = ground_pose(1.65, 0.05).expand(2, 12).contiguous()
    want = ref.ground_grid(res.depth.cpu(), shifted, pose, ref.Spec(-10.0, 0.0, 0.5, 40, 80), band=(-3.0, 3.0), obstacle_height=0.3,
                           min_points=1, min_obstacle_points=3, near=float(ds.min_depth), far=float(ds.max_depth))
    assert all(int(want.count[i].sum()) > 0 for i in range(2))
    check(_as_dict(res.ground), want, "kitti list")


def pipelined_predictor_grids_equal_the_sequential_predictors(ops, model):
    """Four bs-1 steps over TWO slots: every step's grid is bit-equal to the sequential ``Predictor``'s on a captured graph of the same
    shape -- with the keyword's pose and with a pose per step --, a step without intrinsics has none, and with the keyword absent the
    results are the bytes they were."""
    import predict_ref
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.ground_grid import ground_pose
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args = model
    N = 4
    frames = [_frames(90 + i, 1).cuda() for i in range(N)]
    Ks = [intrinsics_from_focal(180.0 + 15.0 * i, PH, PW).cuda() for i in range(N)]
    poses = [None if i % 2 == 0 else ground_pose(1.0 + 0.1 * i, 0.3 - 0.02 * i, 0.01 * i) for i in range(N)]
    pp = PipelinedPredictor(m, args, frames[0], slots=2, want=("depth",), ground_grid=GROUND)
    example = predict_ref.frames_to_input(frames[0].cpu(), args, 0, 0, PH, PW)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_group=1, in_flight=2)
    seq = Predictor(g, args, ground_grid=GROUND)
    off = Predictor(g, args)
    refs = []
    for i in range(N):
        r = seq(frames[i], intrinsics=Ks[i], camera_pose=poses[i])
        refs.append((r.depth.clone(), {n: t.clone() for n, t in _as_dict(r.ground).items()}, off(frames[i], intrinsics=Ks[i]).depth.clone()))
    for i in range(N):
        pp.submit(frames[i], intrinsics=Ks[i] if i % 2 else [Ks[i][0].cpu()], camera_pose=None if poses[i] is None else poses[i].cuda())
    pp.submit(frames[0])
    got = pp.collect()
    assert len(got) == N + 1 and pp.rerun_steps == 0 and got[N].ground is None
    for i in range(N):
        assert torch.equal(got[i].depth.view(torch.int32), refs[i][0].view(torch.int32)), i
        assert torch.equal(got[i].depth.view(torch.int32), refs[i][2].view(torch.int32)), i      # the keyword changes no byte of the map
        for n in ALL:
            assert torch.equal(getattr(got[i].ground, n).view(torch.uint8), refs[i][1][n].view(torch.uint8)), (i, n)
        assert int(got[i].ground.count.sum()) > 0
    assert not torch.equal(got[1].ground.count, got[0].ground.count)
    want = _statement(got[1], Ks[1].cpu(), poses[1], args)
    check(_as_dict(got[1].ground), want, "pipelined, posed step")


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    from objcavit_amd import hip_ops
    model = _model_of("nyu", PH, PW, 29)
    predictor_grid_of_its_own_map(hip_ops, model)
    predictor_shifts_the_camera_by_each_frames_window(hip_ops)
    pipelined_predictor_grids_equal_the_sequential_predictors(hip_ops, model)
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
