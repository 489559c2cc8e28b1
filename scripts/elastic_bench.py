"""Elastic-gather benchmark: ``segmi_elastic_warp_crop_patches`` with a 7^3 control grid against
``segmi_warp_crop_patches`` with the same index map, on the same build, at the sampler's own shapes:
--patches patches of --roi^3 from a seeded --size^3 volume, one channel and then --channels channels, bf16 store.

Device events around each call, the median of --repeats runs after one warm-up, one process.  Byte model of
either gather, per patch voxel: 8 image reads per channel (f32) + 1 label read (f32) + the stores (C bf16 image
values + 1 f32 label) = 32 C + 4 + 2 C + 4 bytes; the control grid (4 KB at 7^3) is not counted.

    python scripts/elastic_bench.py [--size 256] [--roi 128] [--patches 8] [--channels 4] [--repeats 5]
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
    ap.add_argument("--roi", type=int, default=128)
    ap.add_argument("--patches", type=int, default=8)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--control-points", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 timed runs")
    import torch
    from segmantic_amd import ops
    from segmantic_amd.seg import augment as aug
    assert torch.cuda.is_available(), "elastic_bench needs an MI355X"
    dev = torch.device("cuda:0")
    n, r, P = args.size, args.roi, args.patches
    rng = np.random.RandomState(args.seed)
    seed = args.seed
    m = None
    while m is None:                               # the first seed whose spatial draw fires
        m = aug.draw_spatial(np.random.RandomState(seed), (n, n, n))
        seed += 1
    cfg = aug.elastic_config({"prob": 1.0, "control_points": args.control_points})
    ctrl = torch.from_numpy(aug.draw_elastic(rng, (n, n, n), cfg)).to(dev)
    starts = [[0] + [int(v) for v in rng.randint(0, n - r + 1, 3)] for _ in range(P)]
    flips = [int(v) for v in rng.randint(0, 8, P)]
    index_map = aug.to_index_map_xyz(m)
    g = torch.Generator(device=dev).manual_seed(args.seed)
    label = torch.randint(0, 4, (n, n, n), generator=g, device=dev).float()
    res = {"size": n, "roi": r, "patches": P, "control_points": args.control_points, "repeats": args.repeats,
           "store": "bf16"}
    for C in sorted({1, args.channels}):
        image = torch.randn((1, n, n, n, C), generator=g, device=dev)
        out = torch.empty((P, r, r, r, C), dtype=torch.bfloat16, device=dev)
        olab = torch.empty((P, r, r, r), dtype=torch.float32, device=dev)
        model = P * r ** 3 * (32 * C + 4 + 2 * C + 4)
        ela = _timed(lambda: ops.elastic_warp_crop_patches(image, label, starts, flips, index_map, ctrl, out, olab),
                     args.repeats)
        aff = _timed(lambda: ops.warp_crop_patches(image, label, starts, flips, index_map, out, olab), args.repeats)
        for t in (ela, aff):
            t["model_bytes"] = model
            t["model_GBps"] = model / (t["ms_median"] * 1e-3) / 1e9
        res[f"channels_{C}"] = {"elastic": ela, "affine": aff, "ratio": ela["ms_median"] / aff["ms_median"],
                                "added_ms": ela["ms_median"] - aff["ms_median"]}
        del image, out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
