"""Child process of tests/test_hip_lens.py: the lens through the predict path.  ``Predictor(lens=...)`` and ``PipelinedPredictor(lens=...)``
on DISTORTED frames give, tensor for tensor, the bytes of the same predictors without ``lens`` on frames rectified by Statement L on the
CPU (tests/lens_ref.py): depth, depth_u16, the point cloud with its colour, the normals and the ground grid -- ``intrinsics`` left to
default to the map's ``new_K`` in the lens run and given as ``new_K`` in the other.  Once with rgb24 frames, once with nv12, once with
``resize``.  On the small model and frame sizes of tests/ground_grid_predict_child.py, and a process of its own for the reason that file
gives: these steps build pipelines (slots, captured graphs, streams of torch's per-process pool).  Started fresh so that the HIP
runtime reads GPU_MAX_HW_QUEUES=4 at ITS start.  Prints OK when every part passed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), HERE]

import torch  # noqa: E402

import lens_ref as ref  # noqa: E402
from ground_grid_predict_child import GROUND  # noqa: E402
from test_hip_lens import host_planes  # noqa: E402
from test_hip_point_cloud import PH, PW, _frames, _model_of  # noqa: E402

torch.set_grad_enabled(False)
HS, WS = 372, 408                                # the distorted frames
WANT = ("depth", "depth_u16")
READOUTS = dict(point_cloud=dict(stride=(2, 2), pixel=True), surface_normals=dict(radius=2, edge_ratio=0.2, valid=True), ground_grid=GROUND)


def lens_of(window):
    """A moderate barrel whose rectified window looks a little past the frame's corners (black border pixels are image, as documented)."""
    from objcavit_amd.lens import LensMap
    Hw, Ww = window
    return LensMap.brown((230.0, 228.0, 203.1, 186.4), (-0.24, 0.07, 0.0008, -0.0005, -0.008), (HS, WS), window_size=window,
                         new_K=(200.0, 150.25, (Ww - 1) / 2 + 1.5, (Hw - 1) / 2 - 2.25))


def same(a, b, what):
    """Two results of the predict path: every tensor equal byte for byte (a cloud's rows up to its counts: the rest is never written)."""
    for name in WANT:
        x, y = getattr(a, name), getattr(b, name)
        assert x is not None and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, name)
    assert a.points is not None and torch.equal(a.points.counts, b.points.counts) and torch.equal(a.points.total, b.points.total), what
    seen = 0
    for i, n in enumerate(a.points.counts.tolist()):
        assert n > 0 and torch.equal(a.points.points[i, :n].view(torch.int32), b.points.points[i, :n].view(torch.int32)), (what, "points", i)
        assert torch.equal(a.points.pixel[i, :n], b.points.pixel[i, :n]), (what, "pixel", i)
        seen += int((a.points.points[i, :n, 3].view(torch.int32) & 0xFFFFFF).ne(0).sum())
    assert seen > 0, (what, "no point carries a colour")
    for name in ("normals", "valid"):
        x, y = getattr(a.normals, name), getattr(b.normals, name)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, "normals", name)
    assert bool(a.normals.valid.any()), what
    for name in ("count", "obstacle", "h_min", "h_max", "h_mean", "state", "first_occupied"):
        x, y = getattr(a.ground, name), getattr(b.ground, name)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, "ground", name)
    assert int(a.ground.count.sum()) > 0, what


def cases():
    """name -> (keywords of the lens run, the distorted frames on the device, keywords of the other run, the rectified RGB frames on the
    device, the map)."""
    from objcavit_amd.pixel_formats import PixelFormat, PlanarFrames
    out = {}
    full = lens_of((PH, PW))
    rgb = _frames(71, 2, HS, WS)
    out["rgb24"] = (dict(lens=full), rgb.cuda(), {}, torch.from_numpy(ref.remap_rgb(rgb.numpy(), full.map.numpy())).cuda(), full)
    nv = PixelFormat("nv12", "bt709", "limited")
    planes = [p[:2] for p in host_planes("nv12", 2, HS, WS, 73)]
    rect = ref.rectified_rgb([p.numpy() for p in planes], nv, full.map.numpy())
    out["nv12"] = (dict(lens=full, pixel_format=nv), PlanarFrames("nv12", [p.cuda() for p in planes], HS, WS), {},
                   torch.from_numpy(rect).cuda(), full)
    small = lens_of((320, 352))                                                    # another window, resized to the model's 352 x 384
    rect = ref.rectified_rgb([p.numpy() for p in planes], nv, small.map.numpy())
    out["nv12 + resize"] = (dict(lens=small, pixel_format=nv, resize=(PH, PW)), PlanarFrames("nv12", [p.cuda() for p in planes], HS, WS),
                            dict(resize=(PH, PW)), torch.from_numpy(rect).cuda(), small)
    rect = ref.remap_rgb(rgb.numpy(), small.map.numpy())
    out["resize"] = (dict(lens=small, resize=(PH, PW)), rgb.cuda(), dict(resize=(PH, PW)), torch.from_numpy(rect).cuda(), small)
    return out


def one(frames, i):
    return frames[i] if not isinstance(frames, torch.Tensor) else frames[i:i + 1]


def main() -> int:
    assert os.environ.get("GPU_MAX_HW_QUEUES") == "4"
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    m, args = _model_of("nyu", PH, PW, 29)
    made = cases()
    for name in ("rgb24", "nv12", "resize"):
        with_lens, distorted, without, rectified, lm = made[name]
        K = torch.tensor([lm.new_K] * 2, dtype=torch.float32).cuda()
        a = Predictor(m, args, **with_lens, **READOUTS)(distorted, want=WANT)                       # intrinsics default to lens.new_K
        b = Predictor(m, args, **without, **READOUTS)(rectified, want=WANT, intrinsics=K)
        assert tuple(a.depth.shape) == (2, 1) + lm.window_size
        same(a, b, ("Predictor", name))
        # a call's own intrinsics win over the default
        other = K * torch.tensor([1.1, 0.9, 1.0, 1.0], device="cuda")
        c = Predictor(m, args, **with_lens, **READOUTS)(distorted, want=WANT, intrinsics=other)
        assert torch.equal(c.depth, a.depth) and not torch.equal(c.normals.normals, a.normals.normals)
        print("Predictor", name, "equal; valid map pixels", int(lm.valid.sum()), "of", lm.valid.numel())
    for name in ("rgb24", "nv12 + resize"):
        with_lens, distorted, without, rectified, lm = made[name]
        K = torch.tensor([lm.new_K], dtype=torch.float32).cuda()
        pa = PipelinedPredictor(m, args, one(distorted, 0), slots=2, want=WANT, **with_lens, **READOUTS)
        pb = PipelinedPredictor(m, args, rectified[:1], slots=2, want=WANT, **without, **READOUTS)
        for i in (0, 1, 0):
            pa.submit(one(distorted, i))
            pb.submit(rectified[i:i + 1], intrinsics=K)
        ra, rb = pa.collect(), pb.collect()
        assert len(ra) == len(rb) == 3 and pa.rerun_steps == pb.rerun_steps == 0
        for i in range(3):
            same(ra[i], rb[i], ("PipelinedPredictor", name, i))
        assert not torch.equal(ra[0].depth, ra[1].depth) and torch.equal(ra[0].depth, ra[2].depth)
        print("PipelinedPredictor", name, "equal")
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
