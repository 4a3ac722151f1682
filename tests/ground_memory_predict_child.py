"""Child process of tests/test_hip_ground_memory.py: the ground memory through the predict path -- ``Predictor`` and
``PipelinedPredictor`` with the ``ground_grid`` and ``ground_memory`` keywords on the small model the grid's predict test uses.
``result.ground_memory`` over consecutive calls equals the manual chain of ``hip_ops.ground_fuse`` over each call's ``result.ground``
(and Statement F, tests/ground_memory_ref.py, on the host copies); ``reset=True`` equals a fresh predictor; with ``obstacles=True`` the
list is that of the fused map; every other field and attribute is what it is without the keyword; and six bs-1 steps over FOUR slots --
the slots wrap, every step's fuse launch runs on another stream than the one before -- equal the sequential ``Predictor`` bit for bit,
which they do only if each fuse launch waits for the previous step's.  A process of its own for the reasons
tests/ground_grid_predict_child.py gives; started fresh so that the HIP runtime reads GPU_MAX_HW_QUEUES=4 at ITS start.  Prints OK when
every part passed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), HERE]

import pytest  # noqa: E402
import torch  # noqa: E402

import ground_memory_ref as ref  # noqa: E402
from ground_grid_predict_child import GROUND  # noqa: E402
from test_hip_point_cloud import PH, PW, _frames, _model_of  # noqa: E402

torch.set_grad_enabled(False)
ALL = ref.OUTPUTS
MEMORY = dict(free=2, occupied=4, decay=1, limit=8, free_at=3, occupied_at=6)
LIST = dict(link=2, min_cells=2, min_obstacle_points=0, capacity=24, labels=True)
FIELDS = ("depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence")
# (dx, dy, dyaw) per call and stream: about a cell of the 0.5 m grid per step, a slight turn; stream 0 stands for the first three calls
EGO = [None, [[0.0, 0.0, 0.0], [0.0, 0.5, 0.0]], [[0.0, 0.0, 0.0], [0.5, 0.0, 0.1]], [[0.0, 1.0, 0.0], [0.0, 0.0, 0.0]],
       [[0.1, 0.45, 0.01], [-0.5, 0.5, -0.05]], [[0.0, 0.5, 0.0], [0.25, 0.25, 0.0]]]


def bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def spec_of(g):
    GY, GX = (int(v) for v in g.state.shape[1:])
    return (g.x0, g.y0, g.cell, GX, GY)


def motion_of(ego, B):
    from objcavit_amd.ground_memory import ego_motion
    if ego is None:
        return ego_motion().expand(B, 4).contiguous()
    t = torch.tensor(ego, dtype=torch.float64)[:B]
    return ego_motion(t[:, 0], t[:, 1], t[:, 2])


def chain_step(ops, ground, motion, prev):
    """One manual step: ``hip_ops.ground_fuse`` on a result's grid; checked against the statement on the host copies."""
    spec = spec_of(ground)
    got = ops.ground_fuse(ground.state, spec, motion.cuda(), prev_evidence=prev[0], h_max=ground.h_max, prev_h=prev[1], **MEMORY)
    want = ref.fuse(ground.state.cpu().numpy(), ref.Spec(*spec), motion.numpy(), None if prev[0] is None else prev[0].cpu().numpy(),
                    ground.h_max.cpu().numpy(), None if prev[1] is None else prev[1].cpu().numpy(), **MEMORY)
    for n in ALL:
        assert ref.same_bytes(got[n].cpu().numpy(), getattr(want, n)), ("manual step against the statement", n)
    return got


def predictor_carries_the_memory_from_call_to_call(ops, model):
    from objcavit_amd.ground_memory import FusedGrid
    from objcavit_amd.obstacles import Obstacles
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import Predictor, PredictResult
    m, args = model
    assert PredictResult._fields == FIELDS
    first = _frames(81, 2).cuda()
    frames = [first, first, first] + [_frames(82 + i, 2).cuda() for i in range(3)]       # three calls see the same frames: the clamp is reached
    K = intrinsics_from_focal([200.0, 150.25], PH, PW).cuda()
    pr = Predictor(m, args, ground_grid=GROUND, obstacles=LIST, ground_memory=MEMORY)
    plain = Predictor(m, args, ground_grid=GROUND, obstacles=LIST)
    prev, seen, results = (None, None), set(), []
    for i in range(5):
        res = pr(frames[i], intrinsics=K, ego_motion=EGO[i])
        f = res.ground_memory
        assert isinstance(res, PredictResult) and isinstance(f, FusedGrid) and len(tuple(res)) == len(FIELDS)
        assert (f.x0, f.y0, f.cell) == (res.ground.x0, res.ground.y0, res.ground.cell)
        want = chain_step(ops, res.ground, motion_of(EGO[i], 2), prev)
        for n in ALL:
            assert bits(getattr(f, n), want[n]), ("call", i, n)
        prev = (want["evidence"], want["h_max"])
        seen.update(f.state.unique().tolist())
        results.append(res)
        # every other field and attribute is what it is without the keyword (the list reads the frame's grid)
        base = plain(frames[i], intrinsics=K)
        assert base.ground_memory is None and bits(res.depth, base.depth), i
        for name in ("ground", "obstacles"):
            for n, t in getattr(base, name)._asdict().items():
                if isinstance(t, torch.Tensor):
                    assert bits(getattr(getattr(res, name), n), t), (i, name, n)
    ev = torch.stack([r.ground_memory.evidence for r in results]).int()
    print("fused states seen", sorted(seen), "evidence range", int(ev.min()), int(ev.max()), "occupied cells per call",
          [int((r.ground_memory.state == 2).sum()) for r in results])
    assert seen == {0, 1, 2} and int(ev.max()) == MEMORY["limit"]
    # a result handed out is never overwritten: the first call's tensors are still the first manual step's
    first = chain_step(ops, results[0].ground, motion_of(None, 2), (None, None))
    assert all(bits(getattr(results[0].ground_memory, n), first[n]) for n in ALL)
    # reset=True forgets before that call: a fresh predictor's first call
    again = pr(frames[5], intrinsics=K, ego_motion=EGO[5], reset=True)
    fresh = Predictor(m, args, ground_grid=GROUND, ground_memory=MEMORY)(frames[5], intrinsics=K, ego_motion=EGO[5])
    assert all(bits(getattr(again.ground_memory, n), getattr(fresh.ground_memory, n)) for n in ALL)
    assert not bits(again.ground_memory.evidence, pr(frames[5], intrinsics=K, ego_motion=EGO[5]).ground_memory.evidence)    # and remembers after it
    # the grid's buffers are made for the memory even when the grid's ``want`` leaves them out; ``want`` of the memory selects
    sub = Predictor(m, args, ground_grid=dict(GROUND, want=("first_occupied",)), ground_memory=dict(MEMORY, want=("state",)))(frames[0], intrinsics=K)
    assert sub.ground.state is None and sub.ground.h_max is None and sub.ground_memory.evidence is None and sub.ground_memory.h_max is None
    assert bits(sub.ground_memory.state, results[0].ground_memory.state)
    # without intrinsics there is neither a grid nor a memory step
    assert type(pr(frames[0])) is PredictResult
    with pytest.raises(ValueError):
        Predictor(m, args, ground_memory={})

    # obstacles=True: the list of the FUSED map
    po = Predictor(m, args, ground_grid=GROUND, obstacles=LIST, ground_memory=dict(MEMORY, obstacles=True))
    total = 0
    for i in range(3):
        res = po(frames[i], intrinsics=K, ego_motion=EGO[i])
        f = res.ground_memory
        assert all(bits(getattr(f, n), getattr(results[i].ground_memory, n)) for n in ALL), i        # the option changes no byte of the map
        want = ops.obstacles(f.state, spec_of(f), h_max=f.h_max, link=LIST["link"], min_cells=LIST["min_cells"],
                             min_obstacle_points=LIST["min_obstacle_points"], capacity=LIST["capacity"])
        assert isinstance(res.obstacles, Obstacles)
        for n in ops.OBSTACLES_WANT:
            assert bits(getattr(res.obstacles, n), want[n]), (i, n)
        assert not res.obstacles.cells[:, :, 5:7].any()                                              # count / obstacle are null
        total += int(want["total"].sum())
        if i == 0:                                                                                   # one frame is no obstacle yet: not the frame's list
            assert int(want["total"].sum()) == 0 and int(results[0].obstacles.total.sum()) > 0
    print("obstacles of the fused maps", total)
    assert total > 0


def pipelined_predictor_fuses_in_submission_order(ops, model):
    """Six bs-1 steps over FOUR slots against the sequential ``Predictor`` on a captured graph of the same shape."""
    import predict_ref
    from objcavit_amd.graph import GraphedGraphBins
    from objcavit_amd.point_cloud import intrinsics_from_focal
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args = model
    N = 6
    frames = [_frames(90 + i, 1).cuda() for i in range(N)]
    Ks = [intrinsics_from_focal(180.0 + 15.0 * i, PH, PW).cuda() for i in range(N)]
    egos = [None if e is None else e[:1] for e in EGO]
    example = predict_ref.frames_to_input(frames[0].cpu(), args, 0, 0, PH, PW)
    g = GraphedGraphBins(m, torch.cat([example, example.flip(3)], 0).cuda(), object_group=1, in_flight=4)
    for extra in ({}, {"obstacles": True}):
        memory = dict(MEMORY, **extra)
        seq = Predictor(g, args, ground_grid=GROUND, obstacles=LIST, ground_memory=memory)
        refs = []
        for i in range(N):
            r = seq(frames[i], intrinsics=Ks[i], ego_motion=egos[i], reset=(i == 4))
            refs.append(({n: getattr(r.ground_memory, n).clone() for n in ALL}, r.ground.state.clone(), r.obstacles.cells.clone(), r.depth.clone()))
        pp = PipelinedPredictor(m, args, frames[0], slots=4, want=("depth",), ground_grid=GROUND, obstacles=LIST, ground_memory=memory)
        off = PipelinedPredictor(m, args, frames[0], slots=4, want=("depth",), ground_grid=GROUND, obstacles=LIST)
        for i in range(N):
            pp.submit(frames[i], intrinsics=Ks[i], ego_motion=egos[i], reset=(i == 4))
            off.submit(frames[i], intrinsics=Ks[i])
        pp.submit(frames[0])
        got, base = pp.collect(), off.collect()
        assert len(got) == N + 1 and pp.rerun_steps == 0 and got[N].ground_memory is None and got[N].ground is None
        for i in range(N):
            assert base[i].ground_memory is None and len(tuple(got[i])) == len(FIELDS)
            assert bits(got[i].depth, refs[i][3]) and bits(got[i].depth, base[i].depth), i               # the keyword changes no byte of the map
            assert bits(got[i].ground.state, refs[i][1]) and bits(got[i].ground.state, base[i].ground.state), i
            for n in ALL:
                assert bits(getattr(got[i].ground_memory, n), refs[i][0][n]), ("pipelined", sorted(extra), i, n)
            assert bits(got[i].obstacles.cells, refs[i][2]), i
            if not extra:
                assert bits(got[i].obstacles.cells, base[i].obstacles.cells), i
        ev = [int(got[i].ground_memory.evidence.int().abs().sum()) for i in range(N)]
        print("pipelined", sorted(extra), "sum |evidence| per step", ev)
        assert ev[0] > 0
        assert not bits(got[1].ground_memory.evidence, got[0].ground_memory.evidence)


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    from objcavit_amd import hip_ops
    model = _model_of("nyu", PH, PW, 29)
    predictor_carries_the_memory_from_call_to_call(hip_ops, model)
    pipelined_predictor_fuses_in_submission_order(hip_ops, model)
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
