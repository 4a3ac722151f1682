"""Child process of tests/test_hip_object_metrics.py: a ``torch.cuda.graph`` that holds ONLY the object-metrics call -- one linear chain
of three launches, no parallel branch --, replayed after boxes, counts, ground truth and prediction were overwritten in place.  Started
fresh so that the HIP runtime reads GPU_MAX_HW_QUEUES=4 (what tests/conftest.py sets for the suite) at ITS start.  Prints OK when the
replay gives the new inputs' records."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import object_depth_ref as odr  # noqa: E402
import object_metrics_ref as ref  # noqa: E402
from objcavit_amd import hip_ops  # noqa: E402

TOL = 2e-5


def rel_dev(a, b) -> float:
    """max |a - b| / max |b| in float64 (tests/util.py's)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def close(got, want) -> bool:
    got = got.cpu()
    exact = torch.equal(got[..., 8].double(), want[..., 8]) and torch.equal(ref.delta_counts(got), ref.delta_counts(want))
    return exact and all(rel_dev(got[..., c], want[..., c]) < TOL for c in range(ref.FIELDS))


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    pred_h, mirror_h, gt_h = ref.case_maps(seed=11)
    xywh_h, counts_h = odr.case_boxes("inside", width=6)
    pred, mirror, gt, xywh, counts = pred_h.cuda(), mirror_h.cuda(), gt_h.cuda(), xywh_h.cuda(), counts_h.cuda()
    out = torch.full((3, 6, 10), float("nan"), device="cuda")
    call = lambda: hip_ops.object_metrics(pred, gt, xywh, counts, ref.MIN_DEPTH, ref.MAX_DEPTH, pred_mirror=mirror, shrink=0.7, out=out)   # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                  # warm-up outside the capture: this stream's workspace is made here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                                  # captured on the warmed-up stream: the workspace store is per stream
        _, regions = call()
    graph.replay()
    torch.cuda.synchronize()
    first_b, first_r = out.cpu().clone(), regions.cpu().clone()
    want_b, want_r = ref.object_metrics(pred_h, gt_h, xywh_h[..., :4], counts_h, pred_mirror=mirror_h, shrink=0.7)
    assert close(first_b, want_b) and close(first_r, want_r), "replay on the captured inputs"
    # new inputs, in place: other maps, another box set, other counts
    pred_n, mirror_n, gt_n = ref.case_maps(seed=12, special=True)
    xywh_n, _ = odr.case_boxes("small", width=6)
    counts_n = torch.tensor([4, 0, 2], dtype=torch.int32)
    pred.copy_(pred_n.cuda()); mirror.copy_(mirror_n.cuda()); gt.copy_(gt_n.cuda()); xywh.copy_(xywh_n.cuda()); counts.copy_(counts_n.cuda())
    out.fill_(float("nan"))
    regions.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    want_b, want_r = ref.object_metrics(pred_n, gt_n, xywh_n[..., :4], counts_n, pred_mirror=mirror_n, shrink=0.7)
    assert not torch.isnan(out).any() and not torch.isnan(regions).any(), "replay on the new inputs: every element written"
    assert close(out, want_b) and close(regions, want_r), "replay on the new inputs"
    assert not out[1].any() and not regions[1, 0].any() and not torch.equal(out.cpu(), first_b) and not torch.equal(regions.cpu(), first_r)
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
