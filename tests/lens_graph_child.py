"""Child process of tests/test_hip_lens.py: a ``torch.cuda.graph`` that holds the fused lens launch (nv12 frames, three maps, the VEC form
with the mirror) and the rgb24 launch behind it, replayed after the frames' bytes AND the map's entries were overwritten in place.
Started fresh so that the HIP runtime reads GPU_MAX_HW_QUEUES=4 (what tests/conftest.py sets for the suite) at ITS start.  Nothing is
read on the host between the start of the capture and the replays.  Prints OK when each replay gives its inputs' bytes."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(HERE, "golden"), HERE]

import torch  # noqa: E402

import lens_ref as ref  # noqa: E402
import test_hip_lens as t  # noqa: E402
from objcavit_amd import hip_ops  # noqa: E402
from objcavit_amd.pixel_formats import PlanarFrames  # noqa: E402

POISON = 0x7FC0DEAD


def same(out, rgb, planes, fmt, map_host, table):
    rect = ref.rectified_rgb([p.numpy() for p in planes], fmt, map_host.numpy())
    want = torch.from_numpy(ref.ingest(rect, table.numpy(), True))
    return torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)) and torch.equal(rgb.cpu(), torch.from_numpy(rect))


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    fmt, window = t.FORMATS[4], t.VEC
    Hw, Ww = window
    planes = t.host_planes(fmt.name, t.B, t.HS, t.WS, 901)
    dev = [p.cuda() for p in planes]
    frames = PlanarFrames(fmt.name, dev, t.HS, t.WS)
    map_host = t.maps(window)["three"].map.clone()
    m = map_host.cuda()
    table_host = t._table()
    table = table_host.cuda()
    yuv = hip_ops.frame_yuv_tables("cuda", fmt)
    out = torch.empty((2 * t.B, 3, Hw, Ww), dtype=torch.float32, device="cuda")
    rgb = torch.empty((t.B, Hw, Ww, 3), dtype=torch.uint8, device="cuda")

    def chain():
        hip_ops.frame_remap_ingest(frames, table, m, fmt, mirror_too=True, out=out, yuv_tables=yuv)
        hip_ops.frames_remap_rgb24(frames, m, fmt, out=rgb, yuv_tables=yuv)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    out.view(torch.int32).fill_(POISON)
    rgb.fill_(0x5A)
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, rgb, planes, fmt, map_host, table_host), "replay on the captured inputs"
    first = out.cpu().clone()
    # new inputs, in place: other frame bytes, the three maps in another order
    planes = t.host_planes(fmt.name, t.B, t.HS, t.WS, 902)
    for d, p in zip(dev, planes):
        d.copy_(p.cuda())
    map_host = map_host[[2, 0, 1]].contiguous()
    m.copy_(map_host.cuda())
    out.view(torch.int32).fill_(POISON)
    rgb.fill_(0x5A)
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, rgb, planes, fmt, map_host, table_host), "replay on the new inputs"
    assert not torch.equal(out.cpu(), first)
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
