"""-m "not gpu": the per-object depth readout's host side -- the new symbol and its argument checks (no launch happens), the torch
statement of tests/object_depth_ref.py against a brute-force pixel loop, box padding, and the pinned predict interface."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import object_depth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


def test_symbol_is_declared_bound_and_exported(lib):
    from objcavit_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_object_depth_fwd\s*\(", header)
    assert re.search(r"#define\s+OCV_ABI_VERSION\s+5\b", header)
    assert "ocv_object_depth_fwd" in _lib.PROTOTYPES and "object_depth.hip" in build.SOURCES
    assert hasattr(lib, "ocv_object_depth_fwd")
    assert lib.ocv_abi_version() == 5 and _lib.ABI_VERSION == 5


def _call(lib, depth=64, xywh=64, counts=64, out=64, B=1, cap=1, H=8, W=8, half=0.5, q=(0.5,), Q=None, quantiles="array"):
    """The entry point with made-up (never dereferenced) device addresses: every call here must be refused before any launch."""
    arr = (C.c_double * max(len(q), 1))(*q)
    return lib.ocv_object_depth_fwd(depth, None, xywh, 4, counts, B, cap, H, W, half, arr if quantiles == "array" else None,
                                    len(q) if Q is None else Q, out, None)


@pytest.mark.parametrize("kw,word", [
    (dict(depth=None), "null pointer"), (dict(xywh=None), "null pointer"), (dict(counts=None), "null pointer"),
    (dict(out=None), "null pointer"), (dict(quantiles=None), "null pointer"),
    (dict(Q=0), "quantiles"), (dict(q=(0.5,) * 9), "quantiles"),
    (dict(q=(0.5, 1.5)), "outside [0, 1]"), (dict(q=(-0.1,)), "outside [0, 1]"), (dict(q=(float("nan"),)), "outside [0, 1]"),
    (dict(half=0.0), "half"), (dict(half=0.6), "half"), (dict(half=float("nan")), "half"),
    (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"), (dict(B=0), "bad sizes"), (dict(cap=0), "bad sizes"),
])
def test_bad_arguments_are_refused_with_a_message_before_any_launch(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.ocv_last_error().decode()
    assert msg.startswith("ocv_object_depth_fwd:") and word in msg, msg


def test_wrapper_refuses_host_tensors_and_bad_operands():
    from objcavit_amd import hip_ops
    from objcavit_amd._lib import HipLibraryError
    d, x, c = torch.zeros(1, 1, 4, 4), torch.zeros(1, 2, 4), torch.ones(1, dtype=torch.int32)
    with pytest.raises(HipLibraryError):
        hip_ops.object_depth(d, x, c)
    assert hip_ops.object_depth.__defaults__ == (None, (0.1, 0.5, 0.9), 1.0, None)


@pytest.mark.parametrize("name", sorted(ref.BOX_SETS))
@pytest.mark.parametrize("shrink", [1.0, 0.3])
def test_reference_agrees_with_a_brute_force_pixel_loop(name, shrink):
    q = (0.0, 0.1, 0.5, 0.9, 1.0)
    depth, std = ref.case_map("special"), ref.case_map("uniform", seed=1)
    xywh, counts = ref.case_boxes(name)
    got = ref.object_depth(depth, xywh, counts, depth_std=std, quantiles=q, shrink=shrink)
    assert tuple(got.shape) == (3, 6, 10)
    for b in range(3):
        for r in range(6):
            want = [0.0] * 10 if r >= int(counts[b]) else ref.brute_force(depth[b, 0], xywh[b, r].tolist(), q, shrink, std[b, 0])
            row = got[b, r].tolist()
            assert len(row) == len(want)
            for a, e in zip(row, want):
                assert a == e or (math.isnan(a) and math.isnan(e)), (name, b, r, row, want)


def test_pixel_counts_of_the_rules():
    """The counts worked out by hand for the centre rule, and the degenerate boxes: empty or the whole map."""
    H, W = ref.CASE_H, ref.CASE_W
    n = lambda box, s=1.0: 0 if ref.box_pixels(torch.tensor(box), H, W, s) is None else (   # noqa: E731
        lambda p: (p[1] - p[0]) * (p[3] - p[2]))(ref.box_pixels(torch.tensor(box), H, W, s))
    assert n((10.3, 7.7, 4.6, 3.2)) == 15 and n((10.0, 7.0, 2.0, 2.0)) == 4 and n((0.2, 0.2, 1.0, 1.0)) == 1
    assert ref.box_pixels(torch.tensor((10.0, 7.0, 1.0, 1.0)), H, W) == (9, 10, 6, 7)          # lower edge on a centre: in; upper: out
    nan, inf = float("nan"), float("inf")
    for box in ((-1.0, -1.0, -1.0, -1.0), (10.0, 10.0, 0.0, 0.0), (10.0, 10.0, 0.0, 5.0), (100.0, 100.0, 5.0, 5.0), (-9.0, 5.0, 4.0, 4.0),
                (nan, 5.0, 3.0, 3.0), (5.0, 5.0, 3.0, nan), (inf, 5.0, 3.0, 3.0), (5.0, 5.0, inf, 3.0), (5.0, -inf, 3.0, 3.0)):
        assert n(box) == 0, box
    assert n((3.0, 4.0, 1e30, 1e30)) == H * W and n((26.5, 18.5, 53.0, 37.0)) == H * W
    assert n((26.5, 18.5, 53.0, 37.0), 0.5) == 27 * 19          # centres in [13.25, 39.75) x [9.25, 27.75): columns 13 .. 39, rows 9 .. 27


def test_object_depths_pads_lists_like_padded_objects():
    from objcavit_amd.modules.ObjCAViT import PaddedObjects
    from objcavit_amd.object_depth import OBJECT_FIELDS, object_fields, pad_boxes
    dev = torch.device("cpu")
    lists = [None, torch.arange(15.0).view(3, 5), torch.arange(8.0).view(2, 4)]
    xywh, counts = pad_boxes(lists, dev)
    feats = [torch.zeros(1, 7), torch.zeros(3, 7), torch.zeros(2, 7)]
    po = PaddedObjects.from_lists(feats, lists, dev)
    assert torch.equal(xywh, po.xywh) and torch.equal(counts, po.counts) and counts.dtype == torch.int32
    assert counts.tolist() == [1, 3, 2] and xywh[0, 0].tolist() == [-1.0] * 4 and tuple(xywh.shape) == (3, 3, 4)
    assert pad_boxes(po, dev)[0] is po.xywh and pad_boxes((po.xywh, po.counts), dev)[1] is po.counts
    with pytest.raises(TypeError):
        pad_boxes(torch.zeros(3, 4), dev)
    assert OBJECT_FIELDS == ("n", "min", "max", "mean", "std_mean")
    assert object_fields() == OBJECT_FIELDS + ("q0.1", "q0.5", "q0.9") and object_fields((0.0, 1.0, 0.25)) == OBJECT_FIELDS + ("q0", "q1", "q0.25")


def test_predict_interface_is_unchanged_and_objects_is_an_attribute():
    import inspect
    from objcavit_amd.predict import WANT, PipelinedPredictor, Predictor, PredictResult, _ObjectsResult
    assert PredictResult._fields == ("depth", "depth_u16", "rgb8", "records", "bin_edges", "depth_std", "confidence")
    assert WANT == ("depth", "depth_u16", "rgb8", "depth_std", "confidence")
    r = PredictResult(1, 2, 3, 4, 5)
    assert r.objects is None and len(r) == 7
    o = _ObjectsResult(*r, objects="table")
    assert isinstance(o, PredictResult) and o == r and o._fields == r._fields and o.objects == "table"
    assert o._replace(bin_edges=None).objects == "table" and o._replace(bin_edges=None).bin_edges is None
    for fn, name in ((Predictor.__init__, "object_depth"), (PipelinedPredictor.__init__, "object_depth"), (Predictor.__call__, "boxes"),
                     (PipelinedPredictor.submit, "boxes")):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == name and params[name].default is None          # added at the end: positional callers are unaffected
    with pytest.raises(ValueError):
        Predictor(None, __import__("objcavit_amd.config", fromlist=["make_args"]).make_args(), object_depth={"quantile": (0.5,)})
