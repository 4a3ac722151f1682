"""-m "not gpu": host side of the predict path (objcavit_amd/predict.py, the three new C entry points' declarations and argument
checks, the reference statements of tests/predict_ref.py).  No kernel runs."""
import os
import re

import pytest
import torch

import predict_ref
from objcavit_amd import _lib
from objcavit_amd.config import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ocv_frame_ingest_fwd", "ocv_depth_ingest_fwd", "ocv_depth_finalize_fwd")


def test_new_entry_points_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    declared = set(re.findall(r"\b(ocv_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES, name
    if not os.path.exists(_lib.LIB_PATH):
        from objcavit_amd.build import build
        build()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.ocv_abi_version() == _lib.ABI_VERSION == 5                  # symbols are only added
    # bad arguments: -1 and a message, before any launch (there is no GPU here: a launch would fail differently)
    assert lib.ocv_frame_ingest_fwd(None, 0, 0, 8, 8, 0, 0, None, None, 1, 8, 8, 0, 0, None) == -1
    assert b"ocv_frame_ingest_fwd: null pointer" in lib.ocv_last_error()
    assert lib.ocv_depth_ingest_fwd(None, 0, 0, 8, 8, 0, 0, 1000.0, None, 1, 8, 8, None) == -1
    assert b"ocv_depth_ingest_fwd: null pointer" in lib.ocv_last_error()
    assert lib.ocv_depth_finalize_fwd(None, None, 4, 4, 0.001, 10.0, 8, 8, None, None, 1000.0, None, None, 0.0, 1.0, 1, None) == -1
    assert b"ocv_depth_finalize_fwd: null pointer" in lib.ocv_last_error()
    p = 4096                                                               # any non-null, aligned address: it is never dereferenced
    assert lib.ocv_frame_ingest_fwd(p, 24 * 8, 24, 8, 8, 0, 0, p, p, 1, 8, 0, 0, 0, None) == -1
    assert b"bad sizes" in lib.ocv_last_error()
    assert lib.ocv_frame_ingest_fwd(p, 24 * 8, 24, 8, 8, 0, 0, p, p, 1, 8, -4, 0, 0, None) == -1
    assert lib.ocv_frame_ingest_fwd(p, 24 * 8, 24, 8, 8, 1, 0, p, p, 1, 8, 8, 0, 0, None) == -1
    assert b"crop window" in lib.ocv_last_error()
    assert lib.ocv_frame_ingest_fwd(p, 24 * 8, 24, 8, 8, 0, 0, p, p, 2, 8, 8, 1, 8, None) == -1      # the mirrors would land inside the batch
    assert b"mirror" in lib.ocv_last_error()
    assert lib.ocv_depth_ingest_fwd(p, 64, 8, 8, 8, 0, 0, 1000.0, p, 1, 8, 0, None) == -1
    assert b"bad sizes" in lib.ocv_last_error()
    assert lib.ocv_depth_ingest_fwd(p, 64, 8, 8, 8, 0, 0, 0.0, p, 1, 8, 8, None) == -1
    assert b"factor" in lib.ocv_last_error()
    assert lib.ocv_depth_finalize_fwd(p, None, 4, 4, 0.001, 10.0, 8, 0, p, None, 1000.0, None, None, 0.0, 1.0, 1, None) == -1
    assert b"bad sizes" in lib.ocv_last_error()
    assert lib.ocv_depth_finalize_fwd(p, None, 4, 4, 0.001, 10.0, 8, 8, None, None, 1000.0, p, None, 0.0, 1.0, 1, None) == -1
    assert b"colour table" in lib.ocv_last_error()
    assert lib.ocv_depth_finalize_fwd(p, None, 4, 4, 10.0, 0.001, 8, 8, p, None, 1000.0, None, None, 0.0, 1.0, 1, None) == -1
    assert b"min_depth" in lib.ocv_last_error()


def test_kb_crop_origin():
    from objcavit_amd.predict import kb_crop_origin
    assert kb_crop_origin(376, 1241) == (24, 12)
    assert kb_crop_origin(375, 1242) == (23, 13)
    assert kb_crop_origin(370, 1224) == (18, 4)
    assert kb_crop_origin(352, 1216) == (0, 0)
    for Hs, Ws in [(351, 1241), (376, 1215), (100, 100)]:
        with pytest.raises(ValueError):
            kb_crop_origin(Hs, Ws)


@pytest.mark.parametrize("dataset", ["nyu", "kitti"])
def test_normalisation_table_is_the_reference_statement_bit_for_bit(dataset):
    from objcavit_amd.predict import normalisation_table
    args = make_args(dataset=dataset)
    t = normalisation_table(args)
    assert tuple(t.shape) == (3, 256) and t.dtype == torch.float32
    # every value in every channel through the restated reference pipeline: a 16 x 16 frame whose three channels each hold 0 .. 255
    v = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    ref = predict_ref.frames_to_input(v, args, 0, 0, 16, 16)
    assert torch.equal(t, ref.view(3, 256))
    assert float(t[0, 0]) == pytest.approx(-0.485 / 0.229, rel=1e-6) and float(t[2, 255]) == pytest.approx((1 - 0.406) / 0.225, rel=1e-6)


def test_reference_u16_and_rgb8_statements():
    table = torch.arange(256 * 3, dtype=torch.int64).view(256, 3).remainder(251).to(torch.uint8)
    vmin, vmax = 0.5, 8.5
    d = torch.tensor([vmin, vmax, vmin - 1.0, vmax + 3.0, 0.5 + 8.0 / 256 * 17.5, float(torch.nextafter(torch.tensor(8.5), torch.tensor(0.0)))])
    rgb = predict_ref.to_rgb8(d, table, vmin, vmax)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (6, 3)
    for i, row in enumerate([0, 255, 0, 255, 17, 255]):
        assert torch.equal(rgb[i], table[row]), i
    u = predict_ref.to_u16(torch.tensor([0.0, 0.5 / 256, 1.5 / 256, 2.5 / 256, 80.0, 255.998, 300.0]), 256.0)
    assert u.tolist() == [0, 0, 2, 2, 20480, 65535, 65535]               # exact ties go to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2; saturated
    assert predict_ref.to_u16(torch.tensor([0.001, 10.0, 65.5354, 70.0]), 1000.0).tolist() == [1, 10000, 65535, 65535]


def test_colormap_table_is_matplotlibs_normalize_and_colormap_call():
    """The index rule of ``to_rgb8`` against matplotlib itself.  matplotlib evaluates ((d - vmin) / (vmax - vmin)) * 256 in fp32 (a
    division, then a product), the device one product with s = 256 / (vmax - vmin): the two agree in every bit when vmax - vmin is
    a power of two (both are then exact scalings of d - vmin), which is what this comparison uses; for another span a value within
    an ulp of a colour boundary may fall on either side."""
    matplotlib = pytest.importorskip("matplotlib")
    import numpy as np
    from matplotlib.colors import Normalize
    from objcavit_amd.predict import colormap_table
    table = colormap_table("inferno_r")
    assert tuple(table.shape) == (256, 3) and table.dtype == torch.uint8
    assert torch.equal(table, colormap_table("inferno").flip(0))           # a reversed map is its base table read backwards
    vmin, vmax = 0.5, 8.5
    d = torch.rand(97, 131, generator=torch.Generator().manual_seed(7)) * 10.0 - 0.5        # below vmin and above vmax included
    d[0, :4] = torch.tensor([vmin, vmax, -3.0, 40.0])
    try:
        cmap = matplotlib.colormaps["inferno_r"]                           # the registry: what cm.get_cmap returns, without its deprecation
    except AttributeError:                                                 # matplotlib < 3.5
        cmap = matplotlib.cm.get_cmap("inferno_r")
    ref = cmap(Normalize(vmin, vmax)(d.numpy()), bytes=True)[..., :3]
    got = predict_ref.to_rgb8(d, table, vmin, vmax)
    assert np.array_equal(got.numpy(), np.asarray(ref))


def test_predictor_rejects_cpu_tensors():
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    args = make_args()
    frames = torch.zeros(1, 48, 64, 3, dtype=torch.uint8)
    with pytest.raises(_lib.HipLibraryError):
        Predictor(None, args)(frames)
    with pytest.raises(_lib.HipLibraryError):
        Predictor(None, make_args(dataset="kitti"))([torch.zeros(376, 1241, 3, dtype=torch.uint8)])
    with pytest.raises(_lib.HipLibraryError):
        PipelinedPredictor(None, args, frames, slots=1)
    from objcavit_amd import hip_ops
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.frame_ingest(frames, torch.zeros(3, 256))
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.depth_ingest(torch.zeros(1, 8, 8, dtype=torch.uint16), 1000.0)
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.depth_finalize(torch.zeros(1, 1, 4, 4), 0.001, 10.0, (8, 8))
