"""Label clean-up benchmark: connected components and the transforms of seg/transforms.py on the
distance_bench.py volume (seeded 512^3, 16 ellipsoid labels, some on the border) with seeded specks (a few
thousand islands of 1-30 voxels) and a few enclosed cavities added, plus the two structural worst cases
(3-D checkerboard, serpentine path) at 256^3.

Reports, as median (min-max) of --repeats runs after a warm-up: the kernel groups (cc_label, cc_sizes,
cc_compact, cc_keep_largest, cc_fill_holes incl. its background labelling) timed with device events, GB/s
against the byte model below, the end-to-end time of each public transform (host clock around a device
synchronise) and, as context only, scipy.ndimage.label per class on the host when scipy is importable.

    python scripts/components_bench.py [--size 512] [--labels 16] [--repeats 5] [--no-scipy]
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
from segmantic_amd.seg import transforms  # noqa: E402


def byte_model(n: int) -> dict:
    """bytes per call for n voxels of uint8 labels and int32 parents / sizes; data-dependent traffic
    (neighbour labels served by the caches, seam atomics, find chains) is not charged, so the GB/s
    figures are lower bounds on what the hardware moved"""
    return {
        # tile: labels read, parents written; seam: labels read; flatten: parents read, roots written
        "cc_label": n * (1 + 4) + n * 1 + n * (4 + 4),
        "cc_sizes": n * 4 + n * 4,                       # memset of size, roots read (atomics on top)
        "cc_compact": n * 4 + n * 4 + n * (4 + 4),       # count, number, gather: roots read 3x, comp written
        "cc_keep_largest": n * (4 + 1) + n * (1 + 4 + 1),  # one round over the roots, apply
        "cc_fill_holes": n * (1 + 4) * 2 + n * (1 + 4 + 1),  # init, scan, apply (labelling charged apart)
    }


def bench_volume(size: int, labels: int, seed: int, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z, y, x = torch.meshgrid(*[torch.arange(size, device=dev, dtype=torch.float32)] * 3, indexing="ij")
    vol = torch.zeros((size, size, size), dtype=torch.uint8, device=dev)
    for c in range(1, labels + 1):          # the ellipsoids of distance_bench.py
        r = (torch.rand(3, generator=g) * 0.12 + 0.03) * size
        ctr = torch.rand(3, generator=g) * size
        if c % 5 == 0:
            ctr[c % 3] = 0.0 if c % 2 else size - 1.0
        inside = (((z - ctr[0]) / r[0]) ** 2 + ((y - ctr[1]) / r[1]) ** 2 + ((x - ctr[2]) / r[2]) ** 2) <= 1.0
        vol[inside] = c
        if c % 4 == 1:                      # an enclosed cavity at the centre of every fourth ellipsoid
            hole = (((z - ctr[0]) / (r[0] / 3)) ** 2 + ((y - ctr[1]) / (r[1] / 3)) ** 2 +
                    ((x - ctr[2]) / (r[2] / 3)) ** 2) <= 1.0
            vol[hole & (vol == c)] = 0
    del z, y, x
    rng = np.random.default_rng(seed)
    n_specks = 4000
    for _ in range(n_specks):               # islands of 1-30 voxels: a short run of a small box
        c = int(rng.integers(1, labels + 1))
        p = rng.integers(2, size - 8, 3)
        e = rng.integers(1, 4, 3)
        e[2] = min(int(e[2]) * int(rng.integers(1, 4)), 30 // int(e[0] * e[1]))
        vol[p[0]:p[0] + e[0], p[1]:p[1] + e[1], p[2]:p[2] + max(int(e[2]), 1)] = c
    return vol.contiguous()


def checkerboard(size: int, dev):
    i = torch.arange(size, device=dev)
    return ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2).to(torch.uint8).contiguous()


def serpentine(size: int, dev):
    vol = torch.zeros((size, size, size), dtype=torch.uint8, device=dev)
    vol[0::2, 0::2, :] = 1
    rows = torch.arange(0, size - 2, 2, device=dev)
    vol[0::2, rows[0::2] + 1, size - 1] = 1
    vol[0::2, rows[1::2] + 1, 0] = 1
    last = size - 2 if size % 2 == 0 else size - 1
    planes = torch.arange(0, size - 2, 2, device=dev)
    vol[planes[0::2] + 1, last, 0] = 1
    vol[planes[1::2] + 1, 0, 0] = 1
    return vol.contiguous()


def _stat(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def time_events(fn, reps: int):
    out = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return _stat(out)


def time_host(fn, reps: int):
    out = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i:
            out.append((time.perf_counter() - t) * 1e3)
    return _stat(out)


def kernel_times(vol, reps: int, connectivity=None):
    n = vol.numel()
    ws = torch.empty(ops.cc_workspace_bytes(vol.shape), dtype=torch.uint8, device=vol.device)
    root = torch.empty(vol.shape, dtype=torch.int32, device=vol.device)
    size = torch.empty_like(root)
    comp = torch.empty_like(root)
    n_comp = torch.empty(1, dtype=torch.int32, device=vol.device)
    out = torch.empty_like(vol)
    res = {"cc_label": time_events(lambda: ops.cc_label(vol, connectivity, False, root, ws), reps)}
    res["cc_sizes"] = time_events(lambda: ops.cc_sizes(root, size), reps)
    res["cc_compact"] = time_events(lambda: ops.cc_compact(root, comp, n_comp, ws), reps)
    res["cc_keep_largest"] = time_events(lambda: ops.cc_keep_largest(vol, root, size, None, True, 1, out, ws), reps)
    res["components"] = int(n_comp.item())
    ops.cc_label(vol, connectivity, True, root, ws)
    res["cc_fill_holes"] = time_events(lambda: ops.cc_fill_holes(vol, root, None, connectivity, out, ws), reps)
    model = byte_model(n)
    for k, b in model.items():
        res[k]["model_bytes"] = b
        res[k]["gb_per_s"] = b / (res[k]["median_ms"] * 1e-3) / 1e9
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--worst-size", type=int, default=256)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_bench needs an MI355X; a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    vol = bench_volume(args.size, args.labels, args.seed, dev)
    result = {"size": args.size, "labels": args.labels, "voxels": vol.numel(),
              "foreground": int((vol != 0).sum().item()), "kernels": kernel_times(vol, args.repeats)}
    result["end_to_end"] = {
        "connected_components": time_host(lambda: transforms.connected_components(vol), args.repeats),
        "keep_largest": time_host(lambda: transforms.keep_largest_connected_component(vol), args.repeats),
        "remove_small_objects": time_host(lambda: transforms.remove_small_objects(vol, 64), args.repeats),
        "fill_holes": time_host(lambda: transforms.fill_holes(vol), args.repeats),
    }
    cleaned = transforms.fill_holes(transforms.keep_largest_connected_component(vol))
    result["components_after_clean_up"] = transforms.connected_components(cleaned)[1]
    result["voxels_filled"] = int(((cleaned != 0) & (vol == 0)).sum().item())
    worst = {}
    for name, make in (("checkerboard", checkerboard), ("serpentine", serpentine)):
        w = make(args.worst_size, dev)
        for c in (1, 3):
            k = kernel_times(w, args.repeats, c)
            worst[f"{name}_c{c}"] = {"components": k["components"], "cc_label": k["cc_label"]}
    result["worst_cases"] = {"size": args.worst_size, **worst}
    if not args.no_scipy:
        try:
            import scipy.ndimage as ndi
        except ImportError:
            result["scipy"] = "not importable on this host"
        else:
            host = vol.cpu().numpy()
            st = ndi.generate_binary_structure(3, 3)
            t = time.perf_counter()
            count = 0
            for c in range(1, args.labels + 1):
                count += ndi.label(host == c, st)[1]
            dt = (time.perf_counter() - t) * 1e3
            result["scipy"] = {"label_all_classes_ms_cpu": dt, "components": count,
                               "ratio_to_cc_label": dt / result["kernels"]["cc_label"]["median_ms"]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
