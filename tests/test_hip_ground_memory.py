"""-m gpu: csrc/ground_fuse.hip against Statement F in numpy (tests/ground_memory_ref.py) -- EQUAL, not close: every output byte for
byte -- on every grid and motion that can break the warp or the column scan, over sequences fed forward on the device, with the null
inputs, output subsets and batches filled image by image, between poisoned guards, inside a captured graph, and (in a child process)
through the predict path that carries it from step to step."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ground_memory_ref as ref
import test_hip_memory_bounds as bounds
from test_ground_memory_host import BASE, N, POINTERS, REFUSALS, call_entry

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = ref.OUTPUTS
B = 3
DTYPES = {"evidence": torch.int16, "state": torch.uint8}


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


def poisoned(n, spec, names=ALL, byte=0xAB):
    """Output buffers for ``n`` images filled with a byte pattern no result consists of (as fp32 a NaN with a payload, as int16 -21589)."""
    shapes = {name: (n, spec.GX) if name == "first_occupied" else (n, spec.GY, spec.GX) for name in ALL}
    out = {}
    for name in names:
        t = torch.empty(shapes[name], dtype=DTYPES.get(name, torch.float32), device="cuda")
        t.view(torch.uint8).fill_(byte)
        out[name] = t
    return out


def check(got, want, what=""):
    """``got``: the wrapper's dict (any subset of the outputs) against the reference's Result: EQUAL, byte for byte."""
    for name, t in got.items():
        g, w = t.cpu().numpy(), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        if not ref.same_bytes(g, w):
            bad = g.view(np.uint8).reshape(g.shape + (-1,)) != np.ascontiguousarray(w).view(np.uint8).reshape(w.shape + (-1,))
            bad = bad.any(-1)
            at = np.argwhere(bad)[:4].tolist()
            raise AssertionError((what, name, int(bad.sum()), "elements differ", at, [g[tuple(i)] for i in at], [w[tuple(i)] for i in at]))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ops, spec, c, motion, names=ALL, out=None, nulls=(), **kw):
    given = {n: (None if n in nulls else dev(getattr(c, n))) for n in ("prev_evidence", "h_max", "prev_h")}
    return ops.ground_fuse(dev(c.state), tuple(spec), dev(motion), want=names, out=out, **given, **kw)


_WANT = {}


def reference(spec, triple, nulls=(), seed=0, **kw):
    """(the case, its motions [3, 4], the statement on them), made once per (case, options) and left unchanged."""
    key = (spec, triple, tuple(nulls), seed, tuple(sorted(kw.items())))
    if key not in _WANT:
        c = ref.case(spec, B, seed)
        m = ref.motions(spec)
        motion = np.stack([m[n] for n in triple], 0)
        given = {n: (None if n in nulls else getattr(c, n)) for n in ("prev_evidence", "h_max", "prev_h")}
        _WANT[key] = (c, motion, ref.fuse(c.state, spec, motion, **given, **kw))
    return _WANT[key]


# ---------------------------------------------------------------------------
# equality with the statement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ref.GRIDS, ids=lambda s: f"{s.GX}x{s.GY}")
def test_outputs_equal_the_statement(ops, spec):
    """Every motion, three to a batch (one batch has a NaN motion between two others), into poisoned buffers.  A second call over
    another poison gives the same bytes: every element is written, and nothing depends on what the buffers held."""
    carried = 0
    for triple in ref.TRIPLES:
        c, motion, want = reference(spec, triple)
        out = poisoned(B, spec)
        got = run(ops, spec, c, motion, out=out)
        assert all(got[k] is out[k] for k in ALL)
        check(got, want, (spec, triple))
        again = run(ops, spec, c, motion, out=poisoned(B, spec, byte=0x54))
        for k in ALL:
            assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), (spec, triple, k)
        carried += int(want.inside.sum())
        for i, name in enumerate(triple):
            if name in ("nan", "far"):
                assert not want.inside[i].any()
    assert carried > 0
    if spec.GX * spec.GY > 64:
        _, _, want = reference(spec, ref.TRIPLES[1])
        assert set(np.unique(want.state).tolist()) == {0, 1, 2} and np.isfinite(want.first_occupied).any()


def test_the_default_grid_once(ops):
    """200 x 400 at 0.1 m: 13 x 25 tiles and 25 column groups per image, the yaw among the motions."""
    spec = ref.DEFAULT_GRID
    c, motion, want = reference(spec, ref.TRIPLES[1])
    assert want.inside[0].any() and not want.inside[0].all()
    check(run(ops, spec, c, motion, out=poisoned(B, spec)), want, "200x400")


@pytest.mark.parametrize("limit", (8, 32))
@pytest.mark.parametrize("spec", ref.GRIDS[2:], ids=lambda s: f"{s.GX}x{s.GY}")
def test_sequences_fed_forward_on_the_device(ops, spec, limit):
    """Twelve steps of four streams, each step's evidence and fused h_max handed to the next on the device; steps 9 to 12 see nothing,
    so that the evidence fades (tests/test_ground_memory_host.py asserts what these sequences reach)."""
    steps = ref.sequence(spec)
    want = ref.run_sequence(spec, steps, **dict(ref.DEFAULTS, limit=limit))
    prev_e = prev_h = None
    for t, (state, h_max, motion) in enumerate(steps):
        got = ops.ground_fuse(dev(state), tuple(spec), dev(motion), prev_evidence=prev_e, h_max=dev(h_max), prev_h=prev_h, limit=limit,
                              out=poisoned(ref.SEQ_B, spec, byte=0xAB if t % 2 else 0x54))
        check(got, want[t], (spec, limit, "step", t + 1))
        prev_e, prev_h = got["evidence"], got["h_max"]


def test_null_previous_evidence_equals_a_zero_tensor_and_the_null_inputs(ops):
    spec = ref.GRIDS[2]
    c, motion, _ = reference(spec, ref.TRIPLES[2])
    zero = c._replace(prev_evidence=np.zeros_like(c.prev_evidence))
    a = run(ops, spec, zero, motion, out=poisoned(B, spec))
    b = run(ops, spec, c, motion, out=poisoned(B, spec), nulls=("prev_evidence",))
    for k in ALL:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    for r in range(3):
        for nulls in itertools.combinations(("prev_evidence", "h_max", "prev_h"), r + 1):
            _, _, want = reference(spec, ref.TRIPLES[2], nulls=nulls)
            check(run(ops, spec, c, motion, out=poisoned(B, spec), nulls=nulls), want, nulls)
    _, _, full = reference(spec, ref.TRIPLES[2])
    _, _, no_h = reference(spec, ref.TRIPLES[2], nulls=("h_max", "prev_h"))
    assert full.h_max.any() and not no_h.h_max.any()


@pytest.mark.parametrize("names", [c for r in range(1, 4) for c in itertools.combinations(ALL, r)], ids=lambda v: "+".join(v))
def test_subsets_of_the_outputs(ops, names):
    spec = ref.GRIDS[2]
    c, motion, want = reference(spec, ref.TRIPLES[1])
    got = run(ops, spec, c, motion, names=names, out=poisoned(B, spec, names))
    assert set(got) == set(names)
    check(got, want, names)


def test_other_options_than_the_defaults(ops):
    spec = ref.GRIDS[3]
    for kw in (dict(free=0, occupied=1, decay=0, limit=1, free_at=1, occupied_at=1), dict(free=7, occupied=3, decay=5, limit=16383, free_at=9, occupied_at=2),
               dict(free=16383, occupied=16383, decay=16383, limit=16383, free_at=16383, occupied_at=16383)):
        c, motion, want = reference(spec, ref.TRIPLES[0], **kw)
        check(run(ops, spec, c, motion, out=poisoned(B, spec), **kw), want, kw)
    # a previous map a caller made up: the whole int16 range is carried without overflow
    c, motion, _ = reference(spec, ref.TRIPLES[0])
    wild = c._replace(prev_evidence=np.random.default_rng(5).integers(-32768, 32768, c.prev_evidence.shape).astype(np.int16))
    want = ref.fuse(wild.state, spec, motion, wild.prev_evidence, wild.h_max, wild.prev_h, limit=16383, decay=0)
    check(run(ops, spec, wild, motion, out=poisoned(B, spec), limit=16383, decay=0), want, "int16 range")


def test_image_index_fills_a_batch_out_of_order(ops):
    spec = ref.GRIDS[2]
    c, motion, want = reference(spec, ref.TRIPLES[1])
    state, motion_d = dev(c.state), dev(motion)                                        # (a row of the motions is 16 bytes: every slice stays aligned)
    pe, h, ph = dev(c.prev_evidence), dev(c.h_max), dev(c.prev_h)
    whole = run(ops, spec, c, motion, out=poisoned(B, spec))
    check(whole, want, "whole batch")
    pick = [2, 0, 1]
    out = poisoned(B, spec)
    for slot, i in enumerate(pick):
        got = ops.ground_fuse(state[i:i + 1], tuple(spec), motion_d[i:i + 1], prev_evidence=pe[i:i + 1], h_max=h[i:i + 1], prev_h=ph[i:i + 1],
                              out=out, image_index=slot)
        assert got["evidence"] is out["evidence"]
    for n in ALL:
        assert torch.equal(out[n].view(torch.uint8), whole[n][pick].contiguous().view(torch.uint8)), n
    with pytest.raises(ValueError):
        ops.ground_fuse(state[:1], tuple(spec), motion_d[:1], out=out, image_index=3)
    with pytest.raises(ValueError):
        ops.ground_fuse(state, tuple(spec), motion_d, out={"evidence": out["evidence"]})
    fresh = ops.ground_fuse(state, tuple(spec), motion_d, prev_evidence=pe, h_max=h, prev_h=ph)
    for n in ALL:
        assert torch.equal(fresh[n].view(torch.uint8), whole[n].view(torch.uint8)), n


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_bad_options_are_refused(ops):
    spec = ref.GRIDS[1]
    state = torch.zeros(1, spec.GY, spec.GX, dtype=torch.uint8, device="cuda")
    motion = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device="cuda")
    for kw in (dict(want=()), dict(want=("evidence", "count")), dict(limit=0), dict(limit=16384), dict(free=-1), dict(decay=1.5),
               dict(occupied=True), dict(free_at=0), dict(occupied_at=0), dict(prev_evidence=state.short()[:, :2].contiguous()),
               dict(h_max=state.float()[:, :, :3].contiguous())):
        with pytest.raises(ValueError):
            ops.ground_fuse(state, tuple(spec), motion, **kw)
    for bad in ((0.0, 0.0, 0.0, 7, 5), (0.0, 0.0, 1.0, 5, 7), (0.0, 0.0, 1.0, 7), (float("nan"), 0.0, 1.0, 7, 5), (0.0, float("inf"), 1.0, 7, 5)):
        with pytest.raises(ValueError):
            ops.ground_fuse(state, bad, motion)
    with pytest.raises(ValueError):
        ops.ground_fuse(state, tuple(spec), motion.expand(2, 4).contiguous())
    for kw in (dict(prev_evidence=state.int()), dict(prev_h=state.double()), dict(h_max=state)):
        with pytest.raises(TypeError):
            ops.ground_fuse(state, tuple(spec), motion, **kw)
    with pytest.raises(TypeError):
        ops.ground_fuse(state.int(), tuple(spec), motion)


def _real_buffers():
    """Real device buffers for the base case of the refusal table, inputs valid, everything the entry point could write poisoned."""
    GX, GY = BASE["GX"], BASE["GY"]
    t = {"state": torch.full((1, GY, GX), 2, dtype=torch.uint8, device="cuda"), "h_max": torch.ones((1, GY, GX), device="cuda"),
         "prev_e": torch.full((1, GY, GX), 3, dtype=torch.int16, device="cuda"), "prev_h": torch.ones((1, GY, GX), device="cuda"),
         "motion": torch.tensor([[1.0, 0.0, 0.0, 0.0]], device="cuda")}
    t.update({"evidence": torch.full((1, GY, GX), -21589, dtype=torch.int16, device="cuda"), "fstate": torch.full((1, GY, GX), 0xAB, dtype=torch.uint8, device="cuda"),
              "fh": torch.full((1, GY, GX), float("nan"), device="cuda"), "first": torch.full((1, GX), float("nan"), device="cuda")})
    assert set(t) == set(POINTERS) and GX * GY == N
    return t


@pytest.mark.parametrize("kw,word", REFUSALS)
def test_entry_point_refuses_before_any_launch(kw, word):
    """The entry point on real device buffers, every refusal of the table tests/test_ground_memory_host.py runs without a GPU: -1, the
    message, and no byte of any output (or input) touched."""
    from objcavit_amd import _lib
    lib = _lib.load()
    t = _real_buffers()
    before = {n: v.clone() for n, v in t.items()}
    rc = call_entry(lib, {n: v.data_ptr() for n, v in t.items()}, kw, torch.cuda.current_stream().cuda_stream)
    msg = lib.ocv_last_error().decode()
    assert rc == -1 and msg.startswith("ocv_ground_fuse_fwd:") and word in msg, (rc, msg)
    torch.cuda.synchronize()
    for n, v in t.items():
        assert torch.equal(v.view(torch.uint8), before[n].view(torch.uint8)), n


def test_evidence_over_the_previous_evidence_is_refused(ops):
    """The wrapper, handed the previous step's tensors as ``out``: a ping-pong in place is refused, by name, and nothing is written."""
    from objcavit_amd._lib import HipLibraryError
    spec = ref.GRIDS[2]
    c, motion, want = reference(spec, ref.TRIPLES[0])
    pe, ph = dev(c.prev_evidence), dev(c.prev_h)
    state, mot, h = dev(c.state), dev(motion), dev(c.h_max)
    with pytest.raises(HipLibraryError, match="evidence overlaps the input prev_evidence"):
        ops.ground_fuse(state, tuple(spec), mot, prev_evidence=pe, h_max=h, prev_h=ph, want=("evidence",), out={"evidence": pe})
    with pytest.raises(HipLibraryError, match="h_max overlaps the input prev_h"):
        ops.ground_fuse(state, tuple(spec), mot, prev_evidence=pe, h_max=h, prev_h=ph, want=("h_max",), out={"h_max": ph})
    with pytest.raises(HipLibraryError, match="evidence overlaps the input prev_evidence"):      # two images written over images 1 and 2
        ops.ground_fuse(state[:2], tuple(spec), mot[:2], prev_evidence=pe[:2], prev_h=ph[:2], want=("evidence",), out={"evidence": pe[1:]})
    torch.cuda.synchronize()
    assert torch.equal(pe.cpu(), torch.from_numpy(c.prev_evidence)) and torch.equal(ph.cpu().view(torch.int32), torch.from_numpy(c.prev_h).view(torch.int32))
    check(run(ops, spec, c, motion), want, "fresh outputs")


# ---------------------------------------------------------------------------
# guarded memory: a row of tests/test_hip_memory_bounds.py's table (its accounting test wants every *_fwd entry point in a row)
# ---------------------------------------------------------------------------
ROW = "ground_fuse|33x129"


def _ground_fuse_row(c):
    """(33, 129) -- three tiles by nine and five column groups, all ragged --, B = 3 with the yaw among the motions; once with every
    output, once with ``state`` alone.  Every element of every output is written (``c.out``)."""
    spec, triple = ref.GRIDS[2], ref.TRIPLES[1]
    case, motion, want = reference(spec, triple)
    assert triple[0] == "yaw" and want.inside[0].any()
    state, h_max, prev_e, prev_h, mot = (c.put(torch.from_numpy(np.ascontiguousarray(a))) for a in
                                         (case.state, case.h_max, case.prev_evidence, case.prev_h, motion))
    for names in (ALL, ("state",)):
        got = c.ops.ground_fuse(state, tuple(spec), mot, prev_evidence=prev_e, h_max=h_max, prev_h=prev_h, want=names)
        check(got, want, ("guarded", names))
        c.out(*got.values())


if ROW not in bounds.ROWS:
    bounds.row(ROW)(_ground_fuse_row)


def test_launch_between_poisoned_guards():
    bounds.run_row(ROW)
    assert "ocv_ground_fuse_fwd" in bounds.RAN[ROW]


def _child(name):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, name)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


def test_captured_graph_replays_with_a_new_state_and_motion():
    """In a fresh child process (tests/ground_memory_graph_child.py) started with GPU_MAX_HW_QUEUES=4."""
    _child("ground_memory_graph_child.py")


def test_predict_path_carries_the_memory():
    """``Predictor`` and ``PipelinedPredictor`` with the keyword, in a fresh child process (tests/ground_memory_predict_child.py, which
    says what it checks) started with GPU_MAX_HW_QUEUES=4."""
    _child("ground_memory_predict_child.py")
