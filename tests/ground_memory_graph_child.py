"""Child process of tests/test_hip_ground_memory.py: a ``torch.cuda.graph`` that holds ONE ground-memory step (``hip_ops.ground_fuse``
into the caller's buffers), replayed after the state, the heights, the previous map and the motions were overwritten in place.  Started
fresh so that the HIP runtime reads GPU_MAX_HW_QUEUES=4 (what tests/conftest.py sets for the suite) at ITS start.  Nothing is read on
the host between the start of the capture and the replays.  Prints OK when the replay gives the new inputs' map: Statement F
(tests/ground_memory_ref.py)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ground_memory_ref as ref  # noqa: E402
from objcavit_amd import hip_ops  # noqa: E402

B, LIMIT = 3, 8


def same(out, c, spec, motion):
    want = ref.fuse(c.state, spec, motion, c.prev_evidence, c.h_max, c.prev_h, limit=LIMIT)
    return all(ref.same_bytes(out[n].cpu().numpy(), getattr(want, n)) for n in ref.OUTPUTS), want


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    spec = ref.GRIDS[2]
    m = ref.motions(spec)
    c = ref.case(spec, B, seed=11, limit=LIMIT)
    motion = np.stack([m["small"], m["yaw"], m["shift"]], 0)
    state, h_max, prev_e, prev_h, mot = (torch.from_numpy(a).cuda() for a in (c.state, c.h_max, c.prev_evidence, c.prev_h, motion))
    dtypes = {"evidence": torch.int16, "state": torch.uint8}
    out = {n: torch.empty((B, spec.GX) if n == "first_occupied" else (B, spec.GY, spec.GX), dtype=dtypes.get(n, torch.float32), device="cuda")
           for n in ref.OUTPUTS}

    def step():
        hip_ops.ground_fuse(state, tuple(spec), mot, prev_evidence=prev_e, h_max=h_max, prev_h=prev_h, limit=LIMIT, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in out.values():
        t.view(torch.uint8).fill_(0xAB)
    graph.replay()
    torch.cuda.synchronize()
    ok, want = same(out, c, spec, motion)
    assert ok, "replay on the captured inputs"
    first = out["evidence"].cpu().clone()
    assert want.inside.any() and not want.inside.all()
    # new inputs, in place: another state, other heights, another previous map, other motions (one of them NaN now: its image forgets)
    n = ref.case(spec, B, seed=12, limit=LIMIT)
    new_motion = np.stack([m["nan"], m["half"], m["small"]], 0)
    for t, a in ((state, n.state), (h_max, n.h_max), (prev_e, n.prev_evidence), (prev_h, n.prev_h), (mot, new_motion)):
        t.copy_(torch.from_numpy(a).cuda())
    for t in out.values():
        t.view(torch.uint8).fill_(0x54)
    graph.replay()
    torch.cuda.synchronize()
    ok, want = same(out, n, spec, new_motion)
    assert ok, "replay on the new inputs"
    assert not torch.equal(out["evidence"].cpu(), first) and not want.inside[0].any() and want.inside[1:].any()
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
