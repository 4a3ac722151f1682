"""Child process of tests/test_hip_point_cloud.py: a ``torch.cuda.graph`` that holds ONLY the point cloud's two launches -- one linear
chain, no parallel branch --, replayed after the map, the confidence and the cameras were overwritten in place.  Started fresh so that the
HIP runtime reads GPU_MAX_HW_QUEUES=4 (what tests/conftest.py sets for the suite) at ITS start.  Nothing is read on the host between the
start of the capture and the replays.  Prints OK when the replay gives the new inputs' cloud."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import point_cloud_ref as ref  # noqa: E402
from objcavit_amd import _lib, hip_ops  # noqa: E402

POISON = 0x7FC0DEAD


def same(got, want, cap):
    points, counts, total, pixel = (got[k].cpu() for k in ("points", "counts", "total", "pixel"))
    for b, c in enumerate(want):
        n = c.records.shape[0]
        k = min(n, cap)
        if int(total[b]) != n or int(counts[b]) != k:
            return False
        if not torch.equal(points[b, :k].view(torch.int32), c.records[:k].view(torch.int32)) or not torch.equal(pixel[b, :k], c.pixel[:k]):
            return False
        if not bool((points[b, k:].view(torch.int32) == POISON).all()):
            return False
    return True


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    B, H, W, cap = ref.CASE_B, ref.CASE_H, ref.CASE_W, 2600
    depth_h, conf_h, K_h = ref.case_depth("checkerboard"), ref.case_confidence(), ref.case_intrinsics()
    frames_h = ref.case_frames(5, B, H + 2, W + 3)
    depth, conf, K, frames = depth_h.cuda(), conf_h.cuda(), K_h.cuda(), frames_h.cuda()
    out = {"points": torch.empty((B, cap, 4), dtype=torch.float32, device="cuda"), "counts": torch.empty(B, dtype=torch.int32, device="cuda"),
           "total": torch.empty(B, dtype=torch.int32, device="cuda"), "pixel": torch.empty((B, cap), dtype=torch.int32, device="cuda")}
    ws = torch.empty(int(_lib.load().ocv_depth_unproject_workspace_bytes(B, H, W, 1, 1)), dtype=torch.uint8, device="cuda")
    kw = dict(near=ref.NEAR, far=ref.FAR, confidence=conf, min_confidence=0.25, frames=frames, top=1, left=2, want_pixel=True, out=out,
              workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_ops.depth_unproject(depth, K, cap, **kw)                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip_ops.depth_unproject(depth, K, cap, **kw)
    rkw = dict(near=ref.NEAR, far=ref.FAR, min_confidence=0.25, frames=frames_h, top=1, left=2)
    out["points"].view(torch.int32).fill_(POISON)
    graph.replay()
    torch.cuda.synchronize()
    first = out["total"].cpu().clone()
    assert same(out, ref.unproject(depth_h, K_h, confidence=conf_h, **rkw), cap), "replay on the captured inputs"
    # new inputs, in place: another map (more keepers than the capacity), another confidence, other cameras
    depth_h, conf_h, K_h = ref.case_depth("all", seed=3), ref.case_confidence(seed=2), ref.case_intrinsics().flip(0).contiguous()
    depth.copy_(depth_h.cuda())
    conf.copy_(conf_h.cuda())
    K.copy_(K_h.cuda())
    out["points"].view(torch.int32).fill_(POISON)
    graph.replay()
    torch.cuda.synchronize()
    want = ref.unproject(depth_h, K_h, confidence=conf_h, **rkw)
    assert max(c.records.shape[0] for c in want) > cap, "the second map overflows the capacity"
    assert same(out, want, cap), "replay on the new inputs"
    assert not torch.equal(out["total"].cpu(), first)
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
