"""Resampler benchmark: the cubic B-spline prefilter and evaluate and the label-Gaussian vote
(csrc/resample_hq.hip) against the linear and nearest kernels (csrc/image.hip), on the same build, for a 2x
upsampling of a seeded --size^3 volume to (2 size)^3.

Device events around each call, the median of --repeats runs after one warm-up, one process.  The image is f32
noise; the label map is u8, --labels labels in blocks of --block voxels (so most windows hold one label, as in a
segmentation).  GB/s are model bytes over time, the model counting every array once per kernel that must read
or write it:

    prefilter        read the pixels + 3 passes x (read + write) of the float64 coefficients
    bspline_eval     read the float64 coefficients + write the output pixels
    linear, nearest, label_gaussian
                     read the input pixels + write the output pixels

    python scripts/resample_bench.py [--size 256] [--repeats 5] [--labels 5] [--block 16] [--sigma 1] [--alpha 2]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def _timed(fn, repeats: int):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(repeats + 1):                   # the first run is the warm-up
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms[1:])), "ms_all": [round(float(v), 3) for v in ms[1:]]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--labels", type=int, default=5)
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--alpha", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 timed runs")
    import torch
    from segmantic_amd import ops
    assert torch.cuda.is_available(), "resample_bench needs an MI355X"
    dev = torch.device("cuda:0")
    n, o = args.size, 2 * args.size
    g = torch.Generator(device=dev).manual_seed(args.seed)
    image = torch.randn((n, n, n), generator=g, device=dev)
    nb = -(-n // args.block)
    blocks = torch.randint(0, args.labels, (nb, nb, nb), generator=g, device=dev, dtype=torch.uint8)
    label = blocks.repeat_interleave(args.block, 0).repeat_interleave(args.block, 1).repeat_interleave(args.block, 2)
    label = label[:n, :n, :n].contiguous()
    m = np.zeros((3, 4))
    m[:, :3] = np.eye(3) * 0.5
    m[:, 3] = -0.25                                # output voxel centres at the quarter points, as ITK places them
    out = (o, o, o)
    nin, nout = n ** 3, o ** 3
    coef = ops.bspline_coefficients(image)
    runs = {
        "linear": (lambda: ops.resample3d(image, out, m), 4 * nin + 4 * nout),
        "nearest_u8": (lambda: ops.resample3d(label, out, m, nearest=True), nin + nout),
        "prefilter": (lambda: ops.bspline_coefficients(image), 4 * nin + 3 * 16 * nin),
        "bspline_eval": (lambda: ops.resample3d_bspline(image, out, m, coef=coef), 8 * nin + 4 * nout),
        "label_gaussian_u8": (lambda: ops.resample3d_label_gaussian(label, out, m, sigma=args.sigma, alpha=args.alpha),
                              nin + nout),
    }
    res = {"size": n, "out_size": o, "repeats": args.repeats, "labels": args.labels, "block": args.block,
           "sigma": args.sigma, "alpha": args.alpha}
    for name, (fn, model) in runs.items():
        t = _timed(fn, args.repeats)
        t["model_bytes"] = model
        t["model_GBps"] = model / (t["ms_median"] * 1e-3) / 1e9
        res[name] = t
    res["bspline_over_linear"] = (res["prefilter"]["ms_median"] + res["bspline_eval"]["ms_median"]) / res["linear"]["ms_median"]
    res["label_gaussian_over_nearest"] = res["label_gaussian_u8"]["ms_median"] / res["nearest_u8"]["ms_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
