"""Child process of tests/test_hip_ground_grid.py: a ``torch.cuda.graph`` that holds the ground grid's launches only -- clear,
accumulate, finalize: one linear chain, no parallel branch --, replayed after the map, the cameras and the poses were overwritten in
place; in the second round one pose is non-finite.  Started fresh so that the HIP runtime reads GPU_MAX_HW_QUEUES=4 (what
tests/conftest.py sets for the suite) at ITS start.  Nothing is read on the host between the start of the capture and the replays.
Prints OK when the replay gives the new inputs' grid."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import ground_grid_ref as ref  # noqa: E402
from objcavit_amd import _lib, hip_ops  # noqa: E402

INT = ("count", "obstacle", "state")


def same(out, c, spec):
    want = ref.ground_grid(c.depth, c.K, c.pose, spec, **c.options)
    for name in ref.OUTPUTS:
        g, w = out[name].cpu(), getattr(want, name)
        if not (torch.equal(g, w) if name in INT else bool((g == w).all())):
            return False
    return True


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    (H, W), spec = ref.CASE_SHAPES[2], ref.GRIDS[3]
    B = ref.CASE_B
    c = ref.case(H, W)
    depth, K, pose = c.depth.cuda(), c.K.cuda(), c.pose.cuda()
    dtypes = {"count": torch.int32, "obstacle": torch.int32, "state": torch.uint8}
    out = {n: torch.empty((B, spec.GX) if n == "first_occupied" else (B, spec.GY, spec.GX), dtype=dtypes.get(n, torch.float32), device="cuda")
           for n in ref.OUTPUTS}
    ws = torch.empty(int(_lib.load().ocv_ground_grid_workspace_bytes(B, spec.GX, spec.GY)), dtype=torch.uint8, device="cuda")

    def chain():
        hip_ops.ground_grid(depth, K, pose, tuple(spec), near=ref.NEAR, far=ref.FAR, min_obstacle_points=1, out=out, workspace=ws, **c.options)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for t in out.values():
        t.view(torch.uint8).fill_(0xAB)
    graph.replay()
    torch.cuda.synchronize()
    first = out["count"].cpu().clone()
    assert same(out, c, spec), "replay on the captured inputs"
    assert all(int(first[b].sum()) > 0 for b in range(B))
    # new inputs, in place: another map, other cameras, other poses (one of them non-finite now); the thresholds are the captured ones
    n = ref.case(H, W, bad=0, kind="pose", seed=7)
    new = ref.Case(n.depth, n.K.flip(0).contiguous(), n.pose, c.options)
    depth.copy_(new.depth.cuda())
    K.copy_(new.K.cuda())
    pose.copy_(new.pose.cuda())
    for t in out.values():
        t.view(torch.uint8).fill_(0x54)
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, new, spec), "replay on the new inputs"
    now = out["count"].cpu()
    assert not torch.equal(now, first) and not now[0].any() and bool(now[1].any()) and bool(torch.isinf(out["first_occupied"][0]).all())
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
