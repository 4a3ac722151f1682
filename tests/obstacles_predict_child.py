"""Child process of tests/test_hip_obstacles.py: the obstacle list through the predict path -- ``Predictor`` and ``PipelinedPredictor``
with the ``ground_grid`` and ``obstacles`` keywords on the small model the grid's predict test uses, with the keyword's pose and with
``ground_plane=`` / ``pose="plane"``.  ``result.obstacles`` equals Statement O (tests/obstacles_ref.py) applied to ``result.ground``; the
grid's buffers are made for it even when the grid's ``want`` leaves them out, and are then not handed out; without the keyword there is no
list and the results are the bytes they were; ``PredictResult``'s fields are what they were.  A process of its own for the reasons
tests/ground_grid_predict_child.py gives (pipelines draw streams from torch's per-process pool); started fresh so that the HIP runtime
reads GPU_MAX_HW_QUEUES=4 at ITS start.  Prints OK when every part passed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), HERE]

import pytest  # noqa: E402
import torch  # noqa: E402

import obstacles_ref as ref  # noqa: E402
from ground_grid_predict_child import GROUND  # noqa: E402
from test_hip_point_cloud import PH, PW, _frames, _model_of  # noqa: E402

torch.set_grad_enabled(False)
ALL = ref.OUTPUTS
LIST = dict(link=2, min_cells=2, min_obstacle_points=3, capacity=24, labels=True)
PLANE = dict(hypotheses=64, min_inliers=16, height=1.2, pitch=0.3, roll=0.02, height_range=(0.2, 6.0), max_tilt=0.8)
FIELDS = ("depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence")


def statement(ground, **kw):
    """Statement O on a ``GroundGrid`` of the device, with the options of ``LIST`` (``kw`` on top)."""
    o = dict(LIST, **kw)
    GY, GX = (int(v) for v in ground.state.shape[1:])
    return ref.obstacles(ground.state.cpu().numpy(), (ground.x0, ground.y0, ground.cell, GX, GY), ground.count.cpu().numpy(),
                         ground.obstacle.cpu().numpy(), ground.h_max.cpu().numpy(), link=o["link"], min_cells=o["min_cells"],
                         min_obstacle_points=o["min_obstacle_points"], cap=o["capacity"])


def check(got, want, what):
    for n in ALL:
        t = getattr(got, n)
        if t is None:
            continue
        assert torch.equal(t.cpu().view(torch.int32), getattr(want, n).view(torch.int32)), (what, n)


def predictor_lists_the_obstacles_of_its_own_grid(model):
    from objcavit_amd.obstacles import Obstacles, obstacles
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import Predictor, PredictResult
    m, args = model
    assert PredictResult._fields == FIELDS
    frames = _frames(81, 2).cuda()
    K = intrinsics_from_focal([200.0, 150.25], PH, PW).cuda()
    plain = Predictor(m, args, ground_grid=GROUND)(frames, intrinsics=K)
    assert plain.obstacles is None
    res = Predictor(m, args, ground_grid=GROUND, obstacles=LIST)(frames, intrinsics=K)
    assert isinstance(res, PredictResult) and isinstance(res.obstacles, Obstacles) and len(tuple(res)) == len(FIELDS)
    assert (res.obstacles.x0, res.obstacles.y0, res.obstacles.cell) == (res.ground.x0, res.ground.y0, res.ground.cell)
    assert tuple(res.obstacles.cells.shape) == (2, 24, 8) and tuple(res.obstacles.labels.shape) == tuple(res.ground.state.shape)
    want = statement(res.ground)
    print("obstacles kept", want.total.tolist(), "occupied cells", int((res.ground.state == 2).sum()))
    assert int(want.total.sum()) > 0
    check(res.obstacles, want, "keyword's pose")
    # the keyword changes no byte of the map or of the grid
    assert torch.equal(res.depth.view(torch.int32), plain.depth.view(torch.int32))
    for n, t in plain.ground._asdict().items():
        if isinstance(t, torch.Tensor):
            assert torch.equal(t.view(torch.uint8), getattr(res.ground, n).view(torch.uint8)), n
    # the stand-alone function on the same grid gives the same bits, and rows() the same numbers
    alone = obstacles(res.ground, link=2, min_cells=2, min_obstacle_points=3, capacity=24)
    check(alone, want, "stand-alone")
    rows = alone.rows(0)
    assert len(rows) == int(want.counts[0]) and [r["root"] for r in rows] == want.cells[0, :len(rows), 7].tolist()
    assert all(r["x_min"] < r["x_mean"] < r["x_max"] and r["n"] >= 2 for r in rows)
    # the grid's buffers are made for the list even when the grid's ``want`` leaves them out -- and are then not handed out
    sub = Predictor(m, args, ground_grid=dict(GROUND, want=("first_occupied",)), obstacles=dict(LIST, labels=False))(
        frames, want=("depth_u16",), intrinsics=K)
    assert sub.depth is None and sub.ground.state is None and sub.ground.count is None and sub.ground.h_max is None
    assert sub.ground.first_occupied is not None and sub.obstacles.labels is None
    check(sub.obstacles, want, "grid buffers made for the list")
    # the defaults of the keyword; without intrinsics there is neither a grid nor a list
    dflt = Predictor(m, args, ground_grid=GROUND, obstacles={})
    check(dflt(frames, intrinsics=K).obstacles, statement(res.ground, link=1, min_cells=2, min_obstacle_points=0, capacity=64), "defaults")
    assert type(dflt(frames)) is PredictResult
    with pytest.raises(ValueError):
        Predictor(m, args, obstacles={})
    # posed by the plane of the same step
    posed = Predictor(m, args, ground_plane=PLANE, ground_grid=dict(GROUND, pose="plane"), obstacles=LIST)(frames, intrinsics=K)
    assert posed.plane is not None and posed.obstacles is not None
    check(posed.obstacles, statement(posed.ground), "pose='plane'")


def pipelined_predictor_lists_equal_the_statement(model):
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import PipelinedPredictor
    m, args = model
    N = 4
    frames = [_frames(90 + i, 1).cuda() for i in range(N)]
    Ks = [intrinsics_from_focal(180.0 + 15.0 * i, PH, PW).cuda() for i in range(N)]
    for kw in (dict(ground_grid=GROUND), dict(ground_plane=PLANE, ground_grid=dict(GROUND, pose="plane"))):
        off = PipelinedPredictor(m, args, frames[0], slots=2, want=("depth",), **kw)
        pp = PipelinedPredictor(m, args, frames[0], slots=2, want=("depth",), obstacles=LIST, **kw)
        for p in (off, pp):
            for i in range(N):
                p.submit(frames[i], intrinsics=Ks[i])
            p.submit(frames[0])
        base, got = off.collect(), pp.collect()
        assert len(got) == N + 1 and pp.rerun_steps == 0 and got[N].obstacles is None and got[N].ground is None
        totals = []
        for i in range(N):
            assert base[i].obstacles is None and len(tuple(got[i])) == len(FIELDS)
            assert torch.equal(got[i].depth.view(torch.int32), base[i].depth.view(torch.int32)), i      # the keyword changes no byte
            assert torch.equal(got[i].ground.state, base[i].ground.state) and torch.equal(got[i].ground.count, base[i].ground.count), i
            want = statement(got[i].ground)
            check(got[i].obstacles, want, ("pipelined", sorted(kw), i))
            totals.append(int(want.total[0]))
        print("pipelined", sorted(kw), "obstacles kept", totals)
        assert sum(totals) > 0


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    model = _model_of("nyu", PH, PW, 29)
    predictor_lists_the_obstacles_of_its_own_grid(model)
    pipelined_predictor_lists_equal_the_statement(model)
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
