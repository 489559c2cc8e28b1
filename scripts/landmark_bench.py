"""Vertebra-landmark passes on one MI355X: centroid sums, heatmap, extract (max + first argmax) and the positive
bounding box, on a seeded 512^3 label volume with 25 ellipsoidal "vertebrae" (some cut by the border).

    python scripts/landmark_bench.py [--size 512] [--labels 25] [--iters 10] [--oracle-size 128] [--json OUT]

Each pass is timed with device events after a warm-up (median of --iters launches) and reported against a
byte model kept here: bytes each pass must move at least, TB/s, and the share of the 8 TB/s HBM peak.  The CPU
numpy oracle (tests/helpers/detect_ref.py's definitions, vectorised) is timed on a --oracle-size^3 volume.
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
from segmantic_amd.detect.transforms import VertHeatMap, _heatmap_params  # noqa: E402

PEAK_TBS = 8.0


def label_volume(n: int, k: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    lab = np.zeros((n, n, n), dtype=np.uint8)
    ax = np.arange(n, dtype=np.float32)
    for c in range(1, k + 1):
        ctr = rng.uniform(0.05, 0.95, 3) * n
        if c % 6 == 0:
            ctr[rng.integers(0, 3)] = 0.0 if c % 12 else n - 1.0   # cut by the border
        rad = rng.uniform(0.04, 0.09, 3) * n
        sl = [slice(max(int(ctr[a] - rad[a]), 0), min(int(ctr[a] + rad[a]) + 1, n)) for a in range(3)]
        z, y, x = np.meshgrid(ax[sl[0]], ax[sl[1]], ax[sl[2]], indexing="ij")
        m = ((z - ctr[0]) / rad[0]) ** 2 + ((y - ctr[1]) / rad[1]) ** 2 + ((x - ctr[2]) / rad[2]) ** 2 <= 1
        lab[sl[0], sl[1], sl[2]][m] = c
    return lab


def time_ms(fn, iters: int) -> float:
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def oracle_seconds(n: int, k: int) -> dict:
    """numpy on the host: per-label np.where centroids, the f64 heatmap, max + argmax, bbox"""
    from tests.helpers import detect_ref as ref
    lab = label_volume(n, k, seed=1)
    t0 = time.perf_counter()
    ctrs = {c: ref.centre(lab, c) for c in range(1, k + 1) if np.any(lab == c)}
    t1 = time.perf_counter()
    heat = ref.heatmap(lab, k, 1000.0, False).astype(np.float32)
    t2 = time.perf_counter()
    ref.extract(heat, 0.5)
    t3 = time.perf_counter()
    ref.bbox(heat)
    t4 = time.perf_counter()
    assert ctrs
    return {"size": n, "centroids_s": t1 - t0, "heatmap_s": t2 - t1, "extract_s": t3 - t2, "bbox_s": t4 - t3}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=25)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--oracle-size", type=int, default=128)
    ap.add_argument("--json", type=Path, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, k = a.size, a.labels
    lab = torch.from_numpy(label_volume(n, k)).to(dev)
    vox = n ** 3
    sums, flag = ops.label_centroids(lab, k)
    params = _heatmap_params(dev, k, 1000.0)
    heat = ops.vert_heatmap(params, k, sums, flag, lab.shape)
    keys, nan = ops.channel_argmax(heat[1:])
    box = ops.positive_bbox(heat)
    torch.cuda.synchronize()
    present = int((sums[1:, 0] > 0).sum())
    assert int(flag.item()) == 0 and not bool(nan.any())
    # byte model: the least each pass must move (labels u8, heatmap f32 [K + 1, n, n, n])
    model = {
        "centroids": vox * 1,
        "heatmap": (k + 1) * vox * 4,
        "extract": k * vox * 4,
        "bbox": (k + 1) * vox * 4,
    }
    passes = {
        "centroids": lambda: ops.label_centroids(lab, k, sums, flag),
        "heatmap": lambda: ops.vert_heatmap(params, k, sums, flag, lab.shape, out=heat),
        "extract": lambda: ops.channel_argmax(heat[1:], keys, nan),
        "bbox": lambda: ops.positive_bbox(heat, box),
    }
    res = {"size": n, "labels": k, "present": present, "passes": {}}
    for name, fn in passes.items():
        ms = time_ms(fn, a.iters)
        tbs = model[name] / (ms * 1e-3) / 1e12
        res["passes"][name] = {"ms": round(ms, 4), "bytes": model[name], "tb_s": round(tbs, 3),
                               "peak_share": round(tbs / PEAK_TBS, 3)}
        print(f"{name:10s} {ms:9.3f} ms  {model[name] / 1e9:7.3f} GB  {tbs:6.2f} TB/s  {100 * tbs / PEAK_TBS:5.1f} % of peak")
    # the transform end to end (two launches + the flag read-back)
    hm = VertHeatMap(keys="l", label_names=["v"] * k)
    res["vert_heatmap_transform_ms"] = round(time_ms(lambda: hm.heatmap(lab), max(3, a.iters // 2)), 3)
    print(f"VertHeatMap transform end to end: {res['vert_heatmap_transform_ms']:.3f} ms")
    if a.oracle_size > 0:
        res["numpy_oracle"] = oracle_seconds(a.oracle_size, k)
        o = res["numpy_oracle"]
        print(f"numpy oracle at {o['size']}^3: centroids {o['centroids_s']:.2f} s, heatmap {o['heatmap_s']:.2f} s, "
              f"extract {o['extract_s']:.2f} s, bbox {o['bbox_s']:.2f} s")
    print(json.dumps(res))
    if a.json:
        a.json.parent.mkdir(parents=True, exist_ok=True)
        a.json.write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
