"""Child process of tests/test_hip_object_depth.py: a ``torch.cuda.graph`` that holds ONLY the object-depth call -- one linear chain,
no parallel branch --, replayed after counts, boxes and the map were overwritten in place.  Started fresh so that the HIP runtime reads
GPU_MAX_HW_QUEUES=4 (what tests/conftest.py sets for the suite) at ITS start.  Prints OK when the replay gives the new inputs' records."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import object_depth_ref as ref  # noqa: E402
from objcavit_amd import hip_ops  # noqa: E402


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    q = (0.1, 0.5, 0.9)
    depth = ref.case_map("uniform").cuda()
    std = ref.case_map("uniform", seed=3).cuda()
    xywh_h, counts_h = ref.case_boxes("inside", width=6)
    xywh, counts = xywh_h.cuda(), counts_h.cuda()
    out = torch.full((3, 6, 8), float("nan"), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_ops.object_depth(depth, xywh, counts, depth_std=std, quantiles=q, out=out)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip_ops.object_depth(depth, xywh, counts, depth_std=std, quantiles=q, out=out)
    graph.replay()
    torch.cuda.synchronize()
    first = out.cpu().clone()
    assert torch.equal(first, ref.object_depth(depth, xywh, counts_h, std, q)), "replay on the captured inputs"
    # new inputs, in place: another map, another box set, other counts
    depth.copy_(ref.case_map("special").cuda())
    std.copy_(ref.case_map("uniform", seed=4).cuda())
    new_xywh, _ = ref.case_boxes("small", width=6)
    new_counts = torch.tensor([4, 0, 2], dtype=torch.int32)
    xywh.copy_(new_xywh.cuda())
    counts.copy_(new_counts.cuda())
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.object_depth(depth, xywh, new_counts, std, q)
    got = out.cpu()
    exact = [0, 1, 2, 5, 6, 7]
    assert not torch.isnan(got[..., exact]).any() and torch.equal(got[..., exact], want[..., exact]), "replay on the new inputs"
    assert ref.within_one_ulp(got[..., 3:5], want[..., 3:5]), "replay on the new inputs: means"
    assert not torch.equal(got.nan_to_num(), first.nan_to_num())
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
