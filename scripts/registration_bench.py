"""Timing of the registration kernels on one MI355X.

    python scripts/registration_bench.py [--size 256] [--reps 5] [--bins 32]

A seeded analytic pair (Gaussian blobs + an ellipsoid; the moving image under a known rigid transform and a
non-monotone intensity map, both with noise) of SIZE^3 voxels.  Per pyramid level 4, 2, 1 it times one
12-candidate ``ops.joint_histogram`` call (the 2 P candidates of a rigid iteration) against plain torch on the same
GPU: per candidate ``grid_sample`` of the moving level image at the fixed voxels plus a ``bincount`` of the hard
(nearest-bin) joint index.  Then it times the whole rigid registration, and prints the time that went into the
read-backs of the tables.  One JSON line at the end.
"""
from __future__ import annotations

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

BLOBS = (((-0.19, -0.13, -0.10), 0.10, 0.55), ((0.17, 0.15, 0.06), 0.08, 0.45), ((0.06, -0.19, 0.17), 0.07, 0.40),
         ((-0.13, 0.19, -0.17), 0.09, 0.35), ((0.21, -0.06, -0.19), 0.06, 0.30))   # centre, sigma, amplitude (box units)
ELLIPSOID = ((0.02, -0.02, 0.01), (0.35, 0.29, 0.25), 0.30)


def phantom(p: torch.Tensor, extent: float) -> torch.Tensor:
    p = p / extent
    v = torch.zeros(p.shape[:-1], dtype=torch.float64, device=p.device)
    for c, s, a in BLOBS:
        v += a * torch.exp(-((p - torch.tensor(c, dtype=torch.float64, device=p.device)) ** 2).sum(-1) / (2 * s * s))
    c, ax, a = ELLIPSOID
    d = (((p - torch.tensor(c, dtype=torch.float64, device=p.device)) / torch.tensor(ax, dtype=torch.float64, device=p.device)) ** 2).sum(-1).sqrt()
    return (v + a * ((1.0 - d) * 6.0).clamp(0, 1)).clamp(0, 1)


def make_pair(size: int, truth: np.ndarray, dev, seed: int = 0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ax = torch.arange(size, dtype=torch.float64, device=dev) - 0.5 * (size - 1)
    origin = (-0.5 * (size - 1),) * 3
    inv = torch.tensor(np.linalg.inv(truth), dtype=torch.float64, device=dev)
    fixed = torch.empty((size,) * 3, dtype=torch.float32, device=dev)
    moving = torch.empty((size,) * 3, dtype=torch.float32, device=dev)
    for z in range(size):                                  # plane by plane: the float64 temporaries stay small
        zz, yy, xx = torch.meshgrid(ax[z:z + 1], ax, ax, indexing="ij")
        p = torch.stack([xx, yy, zz], -1)[0]
        fixed[z] = phantom(p, float(size)).float()
        v = phantom(p @ inv[:3, :3].T + inv[:3, 3], float(size))
        moving[z] = (1.0 - v * v + 0.15 * torch.sin(9.0 * v)).float()
    fixed += 0.01 * torch.randn(fixed.shape, generator=g).to(dev)
    moving += 0.01 * torch.randn(moving.shape, generator=g).to(dev)
    return processing.Image(fixed, origin=origin), processing.Image(moving, origin=origin)


def gpu_ms(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def torch_joint_histogram(fbin, mimg, maps, bins, mlo, mscale):
    """plain torch: per candidate grid_sample (trilinear, zeros outside) + hard joint bin + bincount"""
    dz, dy, dx = fbin.shape
    mz, my, mx = mimg.shape
    dev = fbin.device
    zz, yy, xx = torch.meshgrid(torch.arange(dz, device=dev, dtype=torch.float32), torch.arange(dy, device=dev, dtype=torch.float32),
                                torch.arange(dx, device=dev, dtype=torch.float32), indexing="ij")
    fb = fbin.reshape(-1).long()
    src = mimg[None, None]
    out = []
    for m in maps:
        m = torch.tensor(m, dtype=torch.float32, device=dev)
        c = [m[r, 0] * xx + m[r, 1] * yy + m[r, 2] * zz + m[r, 3] for r in range(3)]
        inside = ((c[0] >= 0) & (c[0] <= mx - 1) & (c[1] >= 0) & (c[1] <= my - 1) & (c[2] >= 0) & (c[2] <= mz - 1)).reshape(-1)
        grid = torch.stack([2 * c[0] / (mx - 1) - 1, 2 * c[1] / (my - 1) - 1, 2 * c[2] / (mz - 1) - 1], -1)[None]
        val = torch.nn.functional.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(-1)
        mb = ((val - mlo) * mscale + 0.5).floor().clamp(0, bins - 1).long()
        keep = inside & (fb != 255)
        out.append(torch.bincount((fb * bins + mb)[keep], minlength=bins * bins).reshape(bins, bins))
    return torch.stack(out)


def main(size: int = typer.Option(256, "--size"), reps: int = typer.Option(5, "--reps"),
         bins: int = typer.Option(32, "--bins")) -> None:
    dev = torch.device("cuda:0")
    angles = np.deg2rad([6.0, -4.0, 8.0])
    truth = np.eye(4)
    truth[:3, :3] = registration._rot(2, angles[2]) @ registration._rot(1, angles[1]) @ registration._rot(0, angles[0])
    truth[:3, 3] = np.array([3.0, -2.0, 4.0]) * size / 48.0
    fixed, moving = make_pair(size, truth, dev)
    gf = registration._Geometry.of(fixed)
    centre, radius = registration.grid_centre(gf), registration.grid_radius(gf)
    result = {"size": size, "bins": bins, "levels": {}}
    for lv in (4, 2, 1):
        ff = ops.shrink_factors(fixed.data.shape, lv)
        fimg = ops.bin_shrink(fixed.data, ff)
        mimg = moving.data if lv == 1 else ops.bin_shrink(moving.data, ff)
        flo, fhi, mlo, mhi = float(fimg.min()), float(fimg.max()), float(mimg.min()), float(mimg.max())
        fbin = ops.fixed_bins(fimg, flo, fhi, bins)
        mscale = (bins - 1) / (mhi - mlo)
        lg = registration.level_geometry(gf, tuple(reversed(ff)))
        step = 2.0 * min(lg.spacing)
        cands = []
        for k in range(6):
            for sign in (1.0, -1.0):
                q = np.zeros(6)
                q[k] = sign * step
                cands.append(processing._index_map(lg, lg.spacing, lg.origin, lg.direction,
                                                   registration.parameters_to_matrix("rigid", 3, q, centre, radius)))
        maps = np.stack(cands)
        t_hip = gpu_ms(lambda: ops.joint_histogram(fbin, mimg, maps, bins, mlo, mscale), reps)
        t_torch = gpu_ms(lambda: torch_joint_histogram(fbin, mimg.float(), maps, bins, mlo, mscale), max(1, reps // 2))
        h = ops.joint_histogram(fbin, mimg, maps, bins, mlo, mscale)
        torch.cuda.synchronize()                           # time the copy alone, not the wait for the launch
        t0 = time.perf_counter()
        h.cpu()
        t_read = (time.perf_counter() - t0) * 1e3
        samples = fbin.numel() * len(maps)
        result["levels"][str(lv)] = {"fixed_voxels": fbin.numel(), "hip_ms": round(t_hip, 4), "torch_ms": round(t_torch, 4),
                                     "readback_ms": round(t_read, 4),
                                     "hip_gsamples_per_s": round(samples / t_hip / 1e6, 2)}
        print(f"level {lv}: {fbin.numel()} fixed voxels x 12 candidates: joint_histogram {t_hip:.3f} ms, torch grid_sample + "
              f"bincount {t_torch:.3f} ms ({t_torch / t_hip:.1f}x), read-back of the table {t_read:.3f} ms")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = registration.register(fixed, moving, transform="rigid", bins=bins)
    wall = time.perf_counter() - t0
    err = 0.0
    n = np.asarray(gf.size, np.float64) - 1.0
    for k in range(8):
        p = np.asarray(gf.origin) + np.array([n[d] if (k >> d) & 1 else 0.0 for d in range(3)])
        err = max(err, float(np.linalg.norm((truth[:3, :3] - r.transform[:3, :3]) @ p + truth[:3, 3] - r.transform[:3, 3])))
    result["register"] = {"seconds": round(wall, 3), "evaluations": r.evaluations, "iterations": r.iterations,
                          "readback_seconds": round(r.readback_seconds, 3), "tre_mm": round(err, 4), "value": r.value,
                          "converged": r.converged}
    print(f"rigid registration, levels 4,2,1: {wall:.3f} s, {sum(r.evaluations)} evaluations in {sum(r.iterations) + 3} "
          f"launches, {r.readback_seconds:.3f} s in read-backs, TRE {err:.3f} mm")
    print(json.dumps(result))


if __name__ == "__main__":
    typer.run(main)
