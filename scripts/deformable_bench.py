"""Timing of the deformable-registration kernels on one MI355X.

    python scripts/deformable_bench.py [--size 256] [--reps 5] [--bins 32] [--grid-spacing 16]

A seeded analytic pair of SIZE^3 float32 voxels at 1 mm (the phantom of scripts/registration_bench.py): the moving
image is the phantom through a non-monotone intensity map, the fixed image the phantom under a known smooth
B-spline field of 7^3 control points; both with noise.  On the full-resolution level, with the control grid that
``--grid-spacing`` gives, it times (median of REPS launches between device events after a warm-up) the 4-candidate
``ops.ffd_joint_histogram`` launch of one search iteration, ``ops.ffd_gradient``, ``ops.ffd_jacobian`` and
``ops.ffd_warp``.  The comparator is plain torch on the same GPU: per candidate ``grid_sample`` over a precomputed
dense coordinate volume plus a ``bincount`` of the hard joint bin (no B-spline evaluation, no float64), and one
``grid_sample`` for the warp.  Then it times the whole registration and measures the mean displacement error over
the foreground before and after.  One JSON line at the end.
"""
from __future__ import annotations

import importlib.util
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.image import processing, registration  # noqa: E402

_spec = importlib.util.spec_from_file_location("registration_bench", ROOT / "scripts" / "registration_bench.py")
rb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rb)


def make_pair(size: int, truth: registration.DeformableResult, dev, seed: int = 0):
    """(fixed, moving, u): fixed(p) = phantom(p + u(p)), moving(q) = remap(phantom(q)), u float32 [3, z, y, x] in mm"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = registration.displacement_field(truth, device=dev)
    ax = torch.arange(size, dtype=torch.float64, device=dev) - 0.5 * (size - 1)
    fixed = torch.empty((size,) * 3, dtype=torch.float32, device=dev)
    moving = torch.empty((size,) * 3, dtype=torch.float32, device=dev)
    for z in range(size):                                  # plane by plane: the float64 temporaries stay small
        zz, yy, xx = torch.meshgrid(ax[z:z + 1], ax, ax, indexing="ij")
        p = torch.stack([xx, yy, zz], -1)[0]
        fixed[z] = rb.phantom(p + u[:, z].permute(1, 2, 0).double(), float(size)).float()
        v = rb.phantom(p, float(size))
        moving[z] = (1.0 - v * v + 0.15 * torch.sin(9.0 * v)).float()
    fixed += 0.01 * torch.randn(fixed.shape, generator=g).to(dev)
    moving += 0.01 * torch.randn(moving.shape, generator=g).to(dev)
    origin = (-0.5 * (size - 1),) * 3
    return processing.Image(fixed, origin=origin), processing.Image(moving, origin=origin), u


def torch_histograms(fbin, mimg, grids, bins, mlo, mscale):
    """plain torch: per candidate grid_sample (trilinear) at precomputed normalised coordinates + hard bin + bincount"""
    fb = fbin.reshape(-1).long()
    keep = fb != 255
    out = []
    for grid in grids:
        val = torch.nn.functional.grid_sample(mimg[None, None], grid, mode="bilinear", padding_mode="zeros",
                                              align_corners=True).reshape(-1)
        mb = ((val - mlo) * mscale + 0.5).floor().clamp(0, bins - 1).long()
        out.append(torch.bincount((fb * bins + mb)[keep], minlength=bins * bins).reshape(bins, bins))
    return torch.stack(out)


def main(size: int = typer.Option(256, "--size"), reps: int = typer.Option(5, "--reps"),
         bins: int = typer.Option(32, "--bins"), grid_spacing: float = typer.Option(16.0, "--grid-spacing")) -> None:
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    geometry = registration._Geometry((size,) * 3, (1.0,) * 3, (-0.5 * (size - 1),) * 3, np.eye(3).reshape(-1))
    truth = registration.DeformableResult(rng.uniform(-0.035 * size, 0.035 * size, (3, 7, 7, 7)), np.eye(4), geometry, "nmi", 0.0)
    fixed, moving, u_true = make_pair(size, truth, dev)
    full = tuple(fixed.data.shape)
    spans = registration.control_spans(fixed.GetSize(), fixed.spacing, grid_spacing, 3)[-1]
    n_zyx = tuple(s + 3 for s in reversed(spans))
    fimg, mimg = ops.bin_shrink(fixed.data, (1, 1, 1)), moving.data
    flo, fhi, mlo, mhi = float(fimg.min()), float(fimg.max()), float(mimg.min()), float(mimg.max())
    fbin = ops.fixed_bins(fimg, flo, fhi, bins)
    mscale = (bins - 1) / (mhi - mlo)
    m = processing._index_map(moving, fixed.spacing, fixed.origin, fixed.direction, None)
    r = np.eye(3)
    gscale = 1.0 / (mhi - mlo)
    h = [(size - 1) / float(s) for s in spans]
    grids = torch.from_numpy(rng.uniform(-2.0, 2.0, (4, 3) + n_zyx)).to(dev)
    hist = ops.ffd_joint_histogram(fbin, mimg, grids, full, (1, 1, 1), m, r, bins, mlo, mscale)
    dmax, qd = registration.derivative_table(hist[0].cpu().numpy(), "nmi")
    qd = torch.from_numpy(qd).to(dev)
    # the comparator's dense coordinates, normalised for grid_sample: the identity shifted by a constant per candidate
    ax = torch.linspace(-1, 1, size, device=dev)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    dense = [torch.stack([xx, yy, zz], -1)[None] + 0.01 * k for k in range(4)]
    t = {"hist4": rb.gpu_ms(lambda: ops.ffd_joint_histogram(fbin, mimg, grids, full, (1, 1, 1), m, r, bins, mlo, mscale), reps),
         "gradient": rb.gpu_ms(lambda: ops.ffd_gradient(fbin, mimg, grids[0], full, (1, 1, 1), m, r, bins, mlo, mscale, gscale, qd), reps),
         "jacobian": rb.gpu_ms(lambda: ops.ffd_jacobian(grids[0], full, full, (1, 1, 1), [1.0 / v for v in h]), reps),
         "warp": rb.gpu_ms(lambda: ops.ffd_warp(mimg, grids[0], full, m, r), reps),
         "torch_hist4": rb.gpu_ms(lambda: torch_histograms(fbin, mimg, dense, bins, mlo, mscale), reps),
         "torch_warp": rb.gpu_ms(lambda: torch.nn.functional.grid_sample(mimg[None, None], dense[1], mode="bilinear",
                                                                          padding_mode="zeros", align_corners=True), reps)}
    del dense, zz, yy, xx
    for k, v in t.items():
        print(f"{k}: {v:.3f} ms")
    print(f"control grid {n_zyx} (z, y, x), {fbin.numel()} voxels; histogram {t['torch_hist4'] / t['hist4']:.2f}x, "
          f"warp {t['torch_warp'] / t['warp']:.2f}x the torch comparator's speed")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = registration.register_deformable(fixed, moving, grid_spacing=grid_spacing, bins=bins)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    got = registration.displacement_field(res, device=dev)
    fg = fixed.data > 0.2 * float(fixed.data.max())
    before = float(u_true.double().pow(2).sum(0).sqrt()[fg].mean())
    after = float((u_true - got).double().pow(2).sum(0).sqrt()[fg].mean())
    result = {"size": size, "bins": bins, "grid": list(n_zyx), "ms": {k: round(v, 4) for k, v in t.items()},
              "register": {"seconds": round(wall, 3), "iterations": res.iterations, "evaluations": res.evaluations,
                           "spans": [list(s) for s in res.spans], "values": res.level_values, "converged": res.converged,
                           "folded": res.folded, "min_jacobian": res.min_jacobian, "error_before_mm": round(before, 4),
                           "error_after_mm": round(after, 4)}}
    print(f"registration, levels 4,2,1: {wall:.3f} s, iterations {res.iterations}, mean foreground displacement error "
          f"{before:.3f} -> {after:.3f} mm, folded {res.folded}, min Jacobian {res.min_jacobian:.3f}")
    print(json.dumps(result))


if __name__ == "__main__":
    typer.run(main)
