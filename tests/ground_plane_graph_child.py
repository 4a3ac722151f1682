"""Child process of tests/test_hip_ground_plane.py: a ``torch.cuda.graph`` that holds the ground plane's launches and the ground grid's
behind them -- hypotheses, consensus, moments, solve, then clear, accumulate, finalize reading the pose the solve wrote: one linear
chain, no parallel branch --, replayed after the map, the cameras and the prior were overwritten in place; in the second round one image
has no ground in sight and gets its (new) prior.  Started fresh so that the HIP runtime reads GPU_MAX_HW_QUEUES=4 (what tests/conftest.py
sets for the suite) at ITS start.  Nothing is read on the host between the start of the capture and the replays.  Prints OK when the
replay gives the new inputs' plane and grid."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import ground_grid_ref  # noqa: E402
import ground_plane_ref as ref  # noqa: E402
from objcavit_amd import _lib, hip_ops  # noqa: E402

T, STRIDE = 70, (2, 3)
SPEC = ground_grid_ref.Spec(-7.9, 1.1, 0.25, 64, 48)


def same(out, grid, ws_views, sc, triples, prior):
    want = ref.ground_plane(sc.depth, sc.K, triples, prior, stride=STRIDE)
    pose = out["pose"].cpu()
    if not (torch.equal(out["stats"].cpu(), want.stats) and torch.equal(ws_views["count"].cpu(), want.count)
            and torch.equal(ws_views["moments"].cpu(), want.moments)):
        return False
    i, w = pose.view(torch.int32).long(), want.pose.view(torch.int32).long()
    if int((i - w).abs().max()) > 1:                                               # (same sign where they differ: one fp32 step)
        return False
    g = ground_grid_ref.ground_grid(sc.depth, sc.K, pose, SPEC, near=ref.NEAR, far=ref.FAR)
    return all(bool((grid[n].cpu() == getattr(g, n)).all()) for n in ground_grid_ref.OUTPUTS)


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    H, W = ref.CASE_SHAPES[1]
    B = ref.CASE_B
    sc = ref.scene(H, W, noise=0.02, seed=11)
    triples_host, prior_host = ref.triples_of(H, W, T, seed=11), ref.level_prior()
    depth, K, triples, prior = sc.depth.cuda(), sc.K.cuda(), triples_host.cuda(), prior_host.cuda()
    out = {"pose": torch.empty((B, 12), device="cuda"), "stats": torch.empty((B, 4), dtype=torch.int32, device="cuda")}
    dtypes = {"count": torch.int32, "obstacle": torch.int32, "state": torch.uint8}
    grid = {n: torch.empty((B, SPEC.GX) if n == "first_occupied" else (B, SPEC.GY, SPEC.GX), dtype=dtypes.get(n, torch.float32), device="cuda")
            for n in ground_grid_ref.OUTPUTS}
    lib = _lib.load()
    ws = torch.empty(int(lib.ocv_ground_plane_workspace_bytes(B, T)), dtype=torch.uint8, device="cuda")
    ws_grid = torch.empty(int(lib.ocv_ground_grid_workspace_bytes(B, SPEC.GX, SPEC.GY)), dtype=torch.uint8, device="cuda")
    views = {}

    def chain():
        got = hip_ops.ground_plane(depth, K, triples, prior, stride=STRIDE, near=ref.NEAR, far=ref.FAR, out=out, workspace=ws,
                                   want=("pose", "stats", "count", "moments"))
        views.update(count=got["count"], moments=got["moments"])
        hip_ops.ground_grid(depth, K, out["pose"], tuple(SPEC), near=ref.NEAR, far=ref.FAR, min_obstacle_points=1, out=grid, workspace=ws_grid)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for t in list(out.values()) + list(grid.values()) + [ws]:
        t.view(torch.uint8).fill_(0xAB)
    graph.replay()
    torch.cuda.synchronize()
    first = out["pose"].cpu().clone()
    assert same(out, grid, views, sc, triples_host, prior_host), "replay on the captured inputs"
    assert out["stats"].cpu()[:, 3].tolist() == [1, 1, 1]
    # new inputs, in place: another map (image 1 all wall), other cameras, another prior; the table and the options are the captured ones
    new = ref.scene(H, W, noise=0.02, bad=1, kind="wall", seed=12)
    new = ref.Scene(new.depth.flip(0).contiguous(), new.K.flip(0).contiguous(), new.truth.flip(0))
    new_prior = ref.level_prior(height=1.8)
    depth.copy_(new.depth.cuda())
    K.copy_(new.K.cuda())
    prior.copy_(new_prior.cuda())
    for t in list(out.values()) + list(grid.values()) + [ws]:
        t.view(torch.uint8).fill_(0x54)
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, grid, views, new, triples_host, new_prior), "replay on the new inputs"
    now = out["pose"].cpu()
    assert out["stats"].cpu()[:, 3].tolist() == [1, 0, 1] and not torch.equal(now, first)
    assert torch.equal(now[1].view(torch.int32), new_prior[1].view(torch.int32))
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
