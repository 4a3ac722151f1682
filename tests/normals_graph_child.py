"""Child process of tests/test_hip_normals.py: a ``torch.cuda.graph`` that holds the point cloud's two launches, the dense normals launch
and the gather -- one linear chain, no parallel branch --, replayed after the map and the cameras were overwritten in place.  Started
fresh so that the HIP runtime reads GPU_MAX_HW_QUEUES=4 (what tests/conftest.py sets for the suite) at ITS start.  Nothing is read on the
host between the start of the capture and the replays.  Prints OK when the replay gives the new inputs' normals."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import normals_ref as ref  # noqa: E402
from objcavit_amd import _lib, hip_ops  # noqa: E402

POISON = 0x7FC0DEAD
ANGLE_BAR = 1e-3                          # the ceiling of tests/test_hip_normals.py's bar: this file checks the replay, that one the kernel


def same(out, cloud, rows, depth_h, K_h, r):
    want = ref.normals(depth_h, K_h, r)
    n = out["normals"].cpu()
    if not torch.equal(out["valid"].cpu().bool(), want.valid) or bool(n.permute(0, 2, 3, 1)[~want.valid].any()):
        return False
    if float(ref.angle(n.double(), want.normals)[want.valid].max()) >= ANGLE_BAR:
        return False
    if int((out["rgb8"].cpu().int() - want.rgb8.int()).abs().max()) > 1:
        return False
    flat, pixel, res = n.flatten(2), cloud["pixel"].cpu(), rows.cpu()
    for b, k in enumerate(cloud["counts"].tolist()):
        if not torch.equal(res[b, :k, :3].view(torch.int32), flat[b][:, pixel[b, :k].long()].t().contiguous().view(torch.int32)):
            return False
        if not bool((res[b, k:].view(torch.int32) == POISON).all()):
            return False
    return True


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    (H, W), r, cap = ref.CASE_SHAPES[3], 3, 2600
    B = ref.CASE_B
    depth_h, K_h = ref.case(H, W)
    depth, K = depth_h.cuda(), K_h.cuda()
    out = {"normals": torch.empty((B, 3, H, W), dtype=torch.float32, device="cuda"),
           "rgb8": torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda"), "valid": torch.empty((B, H, W), dtype=torch.uint8, device="cuda")}
    cloud = {"points": torch.empty((B, cap, 4), dtype=torch.float32, device="cuda"), "counts": torch.empty(B, dtype=torch.int32, device="cuda"),
             "total": torch.empty(B, dtype=torch.int32, device="cuda"), "pixel": torch.empty((B, cap), dtype=torch.int32, device="cuda")}
    rows = torch.empty((B, cap, 4), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(_lib.load().ocv_depth_unproject_workspace_bytes(B, H, W, 1, 1)), dtype=torch.uint8, device="cuda")

    def chain():
        hip_ops.depth_unproject(depth, K, cap, near=ref.NEAR, far=ref.FAR, want_pixel=True, out=cloud, workspace=ws)
        hip_ops.depth_normals(depth, K, radius=r, near=ref.NEAR, far=ref.FAR, edge_ratio=ref.EDGE, want=("normals", "rgb8", "valid"), out=out)
        hip_ops.normals_gather(out["normals"], cloud["pixel"], cloud["counts"], out=rows)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    rows.view(torch.int32).fill_(POISON)
    graph.replay()
    torch.cuda.synchronize()
    first = out["valid"].cpu().clone()
    assert same(out, cloud, rows, depth_h, K_h, r), "replay on the captured inputs"
    # new inputs, in place: another map, other cameras (one of them unusable now)
    depth_h, K_h = ref.case(H, W, bad_camera=0, seed=7)
    K_h = K_h.flip(0).contiguous()
    depth.copy_(depth_h.cuda())
    K.copy_(K_h.cuda())
    rows.view(torch.int32).fill_(POISON)
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, cloud, rows, depth_h, K_h, r), "replay on the new inputs"
    assert not torch.equal(out["valid"].cpu(), first) and not out["valid"][2].any() and bool(out["valid"][0].any())
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
