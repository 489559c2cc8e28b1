"""Nyul standardisation benchmark: landmarks (segmented multi-rank radix select) and the piecewise map on a
seeded 512^3 f32 single-channel volume with 11 landmarks (0.01, 0.1 ... 0.9, 0.99).

Volumes: `random` (normal intensities) and `background` (the same with half the voxels set to a constant 0,
as zero padding: with nonzero off they all fall into one histogram bin, the case the per-wave aggregation
is for; with nonzero on they are masked out).  Each runs with nonzero off and on.  Reports device-event
times of the landmark call and of the map, the bytes each moves by the model below, GB/s and the share of
the 8 TB/s HBM peak, and (unless --no-host) the host time of np.quantile + the piecewise map in numpy on
the same volume.

    python scripts/nyul_bench.py [--size 512] [--repeats 10] [--no-host]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd import ops  # noqa: E402

PEAK = 8.0e12
QUANTILES = np.array([0.01, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.99])
SCALE = np.linspace(0.0, 100.0, QUANTILES.size)


def byte_model(nvox: int) -> dict:
    """landmarks: three reading passes (A, B, C); map: one read and one write"""
    return {"landmarks": 3 * 4 * nvox, "map": 2 * 4 * nvox}


def volume(kind: str, size: int, dev) -> torch.Tensor:
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x = torch.randn((1, size, size, size), generator=g, device=dev) * 300.0 + 40.0
    if kind == "background":
        x[:, : size // 2] = 0.0
    return x


def timed(fn, repeats: int, before=None):
    ts = []
    for _ in range(repeats):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(np.min(ts))


def host_baseline(x: np.ndarray, nonzero: bool) -> float:
    t0 = time.perf_counter()
    m = x != 0 if nonzero else np.ones(x.shape, bool)
    v = x[m]
    lm = np.quantile(v, QUANTILES)
    i = np.clip(np.searchsorted(lm, v) - 1, 0, lm.size - 2)
    slope = (SCALE[1:] - SCALE[:-1]) / (lm[1:] - lm[:-1])
    y = x.copy()
    y[m] = slope[i] * v + (SCALE[:-1] - slope * lm[:-1])[i]
    return time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nyul_bench needs an MI355X")
    dev = torch.device("cuda:0")
    n = args.size ** 3
    bm = byte_model(n)
    for kind in ("random", "background"):
        x = volume(kind, args.size, dev)
        y = torch.empty_like(x)
        host_x = None if args.no_host else x.cpu().numpy()
        for nonzero in (False, True):
            lm = torch.empty(1, QUANTILES.size, dtype=torch.float32, device=dev)
            cnt = torch.empty(1, dtype=torch.int64, device=dev)
            ws = torch.empty(ops.nyul_workspace_bytes(1, QUANTILES.size), dtype=torch.uint8, device=dev)

            def landmarks():
                ops.nyul_landmarks(x, 1, nonzero, QUANTILES, lm, cnt, ws)

            def apply():
                ops.nyul_apply_(y, 1, nonzero, lm, cnt, SCALE)

            for _ in range(2):                                   # warm-up
                landmarks()
                y.copy_(x)
                apply()
            torch.cuda.synchronize()
            t_lm, t_lm_min = timed(landmarks, args.repeats)
            t_map, t_map_min = timed(apply, args.repeats, before=lambda: y.copy_(x))
            row = {
                "volume": kind, "size": args.size, "nonzero": nonzero, "landmarks": QUANTILES.size,
                "landmarks_s": t_lm, "landmarks_min_s": t_lm_min, "map_s": t_map, "map_min_s": t_map_min,
                "landmarks_bytes": bm["landmarks"], "map_bytes": bm["map"],
                "landmarks_GBps": bm["landmarks"] / t_lm / 1e9, "map_GBps": bm["map"] / t_map / 1e9,
                "landmarks_peak_share": bm["landmarks"] / t_lm / PEAK, "map_peak_share": bm["map"] / t_map / PEAK,
                "total_s": t_lm + t_map,
            }
            if host_x is not None:
                row["host_numpy_s"] = host_baseline(host_x, nonzero)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
