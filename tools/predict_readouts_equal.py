"""Bit-equality of the predict path across a change of its Python layer -> profiles/predict_readouts_refactor.txt, section (2).

    python tools/predict_readouts_equal.py --save A.pt [--package-root DIR]      # one fresh process per side
    python tools/predict_readouts_equal.py --compare A.pt B.pt

``--save`` runs ``Predictor`` (on the module) and ``PipelinedPredictor`` (two slots, four steps, step 1 without ground truth, step 2
without boxes, step 3 with a camera pose of its own) over the cases below on the seeded synthetic GraphBins, at bs 1 and on a list of two
frames of different size under one ``crop``, at the smallest window the predict tests use (352 x 384), and saves every tensor of every
result; cloud rows and gathered normals only up to ``counts[b]`` (rows beyond are unwritten by contract).  ``--package-root``: a
directory holding another copy of ``objcavit_amd`` (the parent commit's ``predict.py`` / ``hip_ops`` put into it) to import instead of
this tree's.  ``--compare`` compares two such files entry by entry on their bytes (shape, dtype, the uint8 view) and prints the list.
Only the public interface is used, so one script serves both sides.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 352, 384
ALL = dict(object_depth={"shrink": 0.8}, object_metrics={}, surface_normals={"picture": True, "valid": True},
           point_cloud={"stride": 2, "min_confidence": 0.05, "max_std": 5.0, "normals": True, "pixel": True},
           ground_grid={"pitch": 0.07, "band": (-5.0, 5.0), "min_confidence": 0.02, "cell": 0.25})
CASES = [("all", ALL, {})]
CASES += [(k, {k: v}, {}) for k, v in ALL.items()]
CASES += [("cloud-plain", dict(point_cloud={"capacity": 5000}), {}), ("all,tta=False", ALL, dict(flip_tta=False)),
          ("plain,maps", {}, dict(want=("depth", "depth_u16"))),
          ("plain,stats,edges", {}, dict(want=("depth", "depth_std", "confidence"), edges=True))]
CASES += [(f"{fmt}{',resize' if rs else ''}", dict(point_cloud={"stride": 3}, object_depth={}), dict(pixel_format=fmt, resize=rs))
          for fmt in ("nv12", "bgra32") for rs in (False, True)]


def _frames(torch, g, sizes, fmt):
    """One step's frames: a batch tensor for one size, a list of single frames for several."""
    from objcavit_amd.pixel_formats import PlanarFrames

    def one(Hs, Ws, batch):
        lead = (1,) if batch else ()
        rnd = lambda *s: torch.randint(0, 256, lead + s, dtype=torch.uint8, generator=g).cuda()          # noqa: E731
        if fmt == "nv12":
            planes = (rnd(Hs, Ws), rnd(-(-Hs // 2), -(-Ws // 2), 2))
            return PlanarFrames("nv12", planes if batch else tuple(p.unsqueeze(0) for p in planes), Hs, Ws)
        return rnd(Hs, Ws, 4 if fmt == "bgra32" else 3)
    return one(*sizes[0], True) if len(sizes) == 1 else [one(Hs, Ws, False) for Hs, Ws in sizes]


def _tensors(torch, name, res):
    """{key: cpu tensor} of one result: its fields and, per readout attribute, that result's tensors."""
    out = {}
    for f in res._fields:
        if isinstance(getattr(res, f), torch.Tensor):
            out[f"{name}.{f}"] = getattr(res, f)
    counts = None if res.points is None else res.points.counts.cpu().tolist()
    for attr in ("objects", "points", "object_metrics", "normals", "ground"):
        part = getattr(res, attr)
        for f in (() if part is None else part._fields):
            t = getattr(part, f)
            if not isinstance(t, torch.Tensor):
                continue
            if (attr, f) in (("points", "points"), ("points", "pixel"), ("normals", "points")):
                for b, n in enumerate(counts):
                    out[f"{name}.{attr}.{f}[{b},:{n}]"] = t[b, :n]
            else:
                out[f"{name}.{attr}.{f}"] = t
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def save(path: str) -> None:
    import torch
    from objcavit_amd import synth as gen
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.GraphBins import GraphBins, SyntheticObjectProvider
    from objcavit_amd.predict import PipelinedPredictor, Predictor
    torch.set_grad_enabled(False)
    print(f"package: {os.path.relpath(os.path.dirname(sys.modules['objcavit_amd'].__file__), ROOT)}", flush=True)
    args = make_args(strategy="learned", language="clip", dimensions_train=[H, W], dimensions_test=[H, W])
    model = GraphBins(args, object_provider=SyntheticObjectProvider(12, "clip", seed=42)).eval()
    gen.load_into(model, 42, gen.PEAKY)
    model = model.cuda()
    saved = {}
    for label, keywords, opt in CASES:
        for shape in ("bs1", "list2"):
            t0 = time.time()
            rs = opt.get("resize", False)
            Hw, Ww = (380, 420) if rs else (H, W)
            sizes = [(Hw + 20, Ww + 20), (Hw + 30, Ww + 35)][:1 if shape == "bs1" else 2]
            B = len(sizes)
            kw = dict(keywords, crop=(6, 10, Hw, Ww), flip_tta=opt.get("flip_tta", True), pixel_format=opt.get("pixel_format"),
                      resize=(H, W) if rs else None)
            want = opt.get("want", ("depth_u16",))
            g = torch.Generator().manual_seed(7)
            steps = []
            for i in range(4):
                gt = None if i == 1 else (torch.rand(B, 1, Hw, Ww, generator=g) * 9.0 + 0.5).cuda()
                boxes = None if i == 2 else [torch.tensor([[60.0 + 20 * i + 7 * b, 90.0, 50.0, 70.0, 1.0], [200.0, 150.0 + 5 * b, 120.0, 90.0, 2.0]])
                                             .cuda() for b in range(B)]
                K = torch.tensor([[518.9 + b, 519.5, Ww / 2 + 10.0 + i, Hw / 2 + 6.0] for b in range(B)])
                pose = torch.eye(3, 4).reshape(1, 12).repeat(B, 1) + 0.01 * (torch.rand(B, 12, generator=g) - 0.5) if i == 3 else None
                steps.append(dict(frames=_frames(torch, g, sizes, opt.get("pixel_format")), depth_gt=gt, boxes=boxes, intrinsics=K,
                                  camera_pose=pose))
            name = f"[{label},{shape}]"
            seq = Predictor(model, args, **kw)
            for i, s in enumerate(steps):
                saved.update(_tensors(torch, f"Predictor{name}[{i}]", seq(s["frames"], s["depth_gt"], first_image_id=i, want=want,
                                                                          camera_pose=s["camera_pose"], intrinsics=s["intrinsics"],
                                                                          boxes=s["boxes"])))
            pp = PipelinedPredictor(model, args, steps[0]["frames"], slots=2, want=want + (("bin_edges",) if opt.get("edges") else ()), **kw)
            for i, s in enumerate(steps):
                pp.submit(s["frames"], s["depth_gt"], first_image_id=i, camera_pose=s["camera_pose"], intrinsics=s["intrinsics"],
                          boxes=s["boxes"])
            results = pp.collect()
            for i, r in enumerate(results):
                saved.update(_tensors(torch, f"PipelinedPredictor{name}[{i}]", r))
            saved[f"PipelinedPredictor{name}.records"] = pp.records(results).cpu()
            del pp, seq
            print(f"{name}: {time.time() - t0:.1f} s, {len(saved)} tensors so far", flush=True)
    torch.save(saved, path)
    print(f"saved {len(saved)} tensors to {path}")


def compare(a: str, b: str) -> int:
    import torch
    A, Bt = torch.load(a), torch.load(b)
    lines, same = [], 0
    for k in sorted(set(A) | set(Bt)):
        x, y = A.get(k), Bt.get(k)
        ok = x is not None and y is not None and x.shape == y.shape and x.dtype == y.dtype and \
            torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
        same += ok
        t = x if x is not None else y
        lines.append(f"    {'equal    ' if ok else 'DIFFERENT'} {k} {tuple(t.shape)} {str(t.dtype).replace('torch.', '')}")
    print(f"    {len(lines)} tensors compared, {same} bit-equal, {len(lines) - same} different\n")
    print("\n".join(lines))
    return 0 if same == len(lines) else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--save")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")              # before torch initialises HIP
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    if not torch.cuda.is_available():
        print("predict_readouts_equal: no GPU -- nothing runs without one", file=sys.stderr)
        return 2
    save(a.save)
    return 0


if __name__ == "__main__":
    sys.exit(main())
