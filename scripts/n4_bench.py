"""N4 bias-field correction and CT scaling on one MI355X (DESIGN §12 records the figures).

    python scripts/n4_bench.py [--size 512] [--shrink 4] [--levels 4] [--iterations 50] [--reps 5]
                               [--oracle-size 96]

Input: a seeded phantom (three ellipsoid classes, 100 / 200 / 300 + noise, times exp(b) with a smooth b of
amplitude 0.3), f32 [size]^3 on the device.  The N4 run uses the convergence threshold 0, so every level
runs its full iteration count.  Times are medians of --reps timed calls after one warm-up, from device
events.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.image import modality  # noqa: E402

HBM_PEAK = 8.0e12


def phantom_gpu(n: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator(device="cuda").manual_seed(seed)
    ax = torch.linspace(-1, 1, n, device="cuda", dtype=torch.float32)
    z, y, x = ax.view(n, 1, 1), ax.view(1, n, 1), ax.view(1, 1, n)
    cls = torch.zeros((n, n, n), dtype=torch.float32, device="cuda")
    cls = torch.where(z ** 2 / 0.81 + y ** 2 / 0.7225 + x ** 2 / 0.64 < 1, 1.0, cls)
    cls = torch.where((z - 0.1) ** 2 / 0.3025 + (y + 0.1) ** 2 / 0.25 + (x - 0.1) ** 2 / 0.2025 < 1, 2.0, cls)
    cls = torch.where((z + 0.2) ** 2 / 0.09 + (y + 0.15) ** 2 / 0.0625 + (x + 0.2) ** 2 / 0.09 < 1, 3.0, cls)
    noise = torch.randn((n, n, n), generator=g, device="cuda") * 5.0
    b = 0.3 * torch.sin(1.3 * x + 0.4) * torch.cos(0.9 * y - 0.2) + 0.15 * z
    return ((100.0 * cls + (cls > 0) * noise) * torch.exp(b)).contiguous()


def timed(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--shrink", type=int, default=4)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-size", type=int, default=96)
    a = ap.parse_args()
    n = a.size
    x = phantom_gpu(n)
    nbytes = x.numel() * 4
    its = [a.iterations] * a.levels

    def n4_end_to_end():
        _, stats = ops.otsu(x, 200)
        _, _, lg = ops.n4_shrink(x, [a.shrink] * 3, otsu_stats=stats, want_image=False, want_mask=False,
                                 want_log=True)
        lat, _, _, _ = ops.n4_fit(lg, its, threshold=0.0)
        return ops.n4_evaluate(lat, x.shape, x)

    _, stats = ops.otsu(x, 200)
    _, _, lg = ops.n4_shrink(x, [a.shrink] * 3, otsu_stats=stats, want_image=False, want_mask=False, want_log=True)
    lat, _, elapsed, _ = ops.n4_fit(lg, its, threshold=0.0)
    fit_set = int(torch.isfinite(lg).sum())
    t_e2e = timed(n4_end_to_end, a.reps)
    t_otsu = timed(lambda: ops.otsu(x, 200), max(a.reps, 20))
    t_shrink = timed(lambda: ops.n4_shrink(x, [a.shrink] * 3, otsu_stats=stats, want_image=False, want_mask=False,
                                           want_log=True), max(a.reps, 20))
    t_fit = timed(lambda: ops.n4_fit(lg, its, threshold=0.0), a.reps)
    t_eval = timed(lambda: ops.n4_evaluate(lat, x.shape, x), max(a.reps, 20))
    t_ct = timed(lambda: ops.ct_scale(x), max(a.reps, 20))
    # the public entry point with its default threshold, for reference
    t_api = timed(lambda: modality.bias_correct(modality.Image(x), shrink_factor=a.shrink,
                                                num_fitting_levels=a.levels, num_iterations=a.iterations), a.reps)
    # numpy f64 oracle (not ITK) on a smaller volume
    from tests.helpers import n4_ref as ref
    m = a.oracle_size
    img_o, _, _ = ref.phantom((m, m, m), seed=0)
    t0 = time.perf_counter()
    mask_o, _, _ = ref.otsu_threshold(img_o)
    lat_o, _, _, _ = ref.n4(ref.shrink(img_o, a.shrink), ref.shrink(mask_o, a.shrink), iterations=its, threshold=0.0)
    _ = img_o / np.exp(ref.evaluate(lat_o, img_o.shape))
    t_oracle = time.perf_counter() - t0
    n_iter = sum(elapsed)
    res = {
        "size": n, "shrink": a.shrink, "levels": a.levels, "iterations": elapsed, "fit_set_voxels": fit_set,
        "end_to_end_s": t_e2e, "bias_correct_default_threshold_s": t_api,
        "otsu_ms": t_otsu * 1e3, "otsu_TBps": 2 * nbytes / t_otsu / 1e12,
        "shrink_gather_ms": t_shrink * 1e3,
        "fit_ms": t_fit * 1e3, "per_iteration_us": t_fit / n_iter * 1e6,
        "eval_divide_ms": t_eval * 1e3, "eval_divide_TBps": 2 * nbytes / t_eval / 1e12,
        "eval_divide_hbm_frac": 2 * nbytes / t_eval / HBM_PEAK,
        "ct_scale_ms": t_ct * 1e3, "ct_scale_TBps": 2 * nbytes / t_ct / 1e12,
        "numpy_f64_oracle_size": m, "numpy_f64_oracle_s": t_oracle,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
