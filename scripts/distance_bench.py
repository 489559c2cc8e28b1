"""Evaluation benchmark: surface_distances on a seeded synthetic 512^3 label pair with 16 labels.

Labels are ellipsoids of varied size (some touch the volume border); the prediction is the reference
shifted by one voxel and dilated by one.  Reports the end-to-end time of surface_distances (warmed up,
device-synchronised, repeated), the EDT and sampler kernel times of the largest label's box against the
byte model below, and the CPU time of the test oracle on one label's box (labelled CPU).

    python scripts/distance_bench.py [--size 512] [--labels 16] [--repeats 5] [--once]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.seg.evaluation import surface_distances  # noqa: E402


def byte_model(nvox: int, n_query: int) -> dict:
    """bytes each pass moves for a box of nvox voxels (uint8 labels, f32 maps, i32 + f32 stack entries;
    the envelope passes are charged a full stack: one entry written and read per voxel)"""
    return {
        "p1": nvox * (1 + 4 + 4 + 4),          # labels, forward write, backward read + write
        "p2": nvox * (4 + 8 + 8 + 4),          # f1 read, stack write + read, transposed write
        "p3": nvox * (4 + 8 + 8 + 4),          # in place: read, stack write + read, write
        "sample": nvox * 1 + n_query * 4,      # query test over the box, distances of the queries
    }


def synthetic_pair(size: int, labels: int, seed: int, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z, y, x = torch.meshgrid(*[torch.arange(size, device=dev, dtype=torch.float32)] * 3, indexing="ij")
    ref = torch.zeros((size, size, size), dtype=torch.uint8, device=dev)
    for c in range(1, labels + 1):
        r = (torch.rand(3, generator=g) * 0.12 + 0.03) * size
        ctr = torch.rand(3, generator=g) * size
        if c % 5 == 0:
            ctr[c % 3] = 0.0 if c % 2 else size - 1.0      # touches the border
        inside = (((z - ctr[0]) / r[0]) ** 2 + ((y - ctr[1]) / r[1]) ** 2 + ((x - ctr[2]) / r[2]) ** 2) <= 1.0
        ref[inside] = c
    del z, y, x
    pred = torch.roll(ref, shifts=(1, 0, 1), dims=(0, 1, 2))
    grown = torch.zeros_like(pred)
    for c in range(1, labels + 1):
        m = F.max_pool3d((pred == c).float()[None, None], 3, 1, 1)[0, 0] > 0
        grown[m & (grown == 0)] = c
    pred = torch.where(pred == 0, grown, pred)
    return pred.contiguous(), ref.contiguous()


def time_kernels(pred, ref, box, spacing, reps):
    """events around one edt_sq and one sampler on the given box"""
    nvox = int(np.prod(np.asarray(box[1::2]) - np.asarray(box[0::2])))
    dist = torch.empty(nvox, dtype=torch.float32, device=pred.device)
    ws = torch.empty(ops.edt_workspace_bytes(box), dtype=torch.uint8, device=pred.device)
    stats = torch.zeros(4, dtype=torch.float64, device=pred.device)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_edt, t_s = [], []
    for _ in range(reps + 1):
        e[0].record()
        ops.edt_sq(ref, 1, 1, box, spacing, dist, ws)
        e[1].record()
        ops.edt_sample(dist, pred, 1, 0, box, stats, ws)
        e[2].record()
        torch.cuda.synchronize()
        t_edt.append(e[0].elapsed_time(e[1]))
        t_s.append(e[1].elapsed_time(e[2]))
    return nvox, float(np.median(t_edt[1:])), float(np.median(t_s[1:])), int(stats[0].item())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--once", action="store_true", help="one call (for a profiler run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "distance_bench needs an MI355X"
    dev = torch.device("cuda:0")
    pred, ref = synthetic_pair(args.size, args.labels, args.seed, dev)
    spacing = (1.0, 1.0, 1.0)
    k = args.labels + 1
    torch.cuda.synchronize()
    if args.once:
        surface_distances(pred, ref, num_classes=k, spacing=spacing)
        torch.cuda.synchronize()
        print(json.dumps({"once": True, "size": args.size, "labels": args.labels}))
        return
    surface_distances(pred, ref, num_classes=k, spacing=spacing)      # warm-up
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        surface_distances(pred, ref, num_classes=k, spacing=spacing)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res = {"size": args.size, "labels": args.labels, "e2e_ms_median": 1e3 * float(np.median(times)),
           "e2e_ms_all": [round(1e3 * t, 3) for t in times]}
    # whole-volume box: the full 512^3 crop of the byte-model figures (label 1 of ref vs pred)
    one_p = (pred == 1).to(torch.uint8).contiguous()
    one_r = (ref == 1).to(torch.uint8).contiguous()
    s = args.size
    box = [0, s, 0, s, 0, s]
    nvox, t_edt, t_s, nq = time_kernels(one_p, one_r, box, spacing, 3)
    bm = byte_model(nvox, nq)
    res["full_box"] = {"nvox": nvox, "edt_ms": t_edt, "sample_ms": t_s,
                       "edt_model_GBps": (bm["p1"] + bm["p2"] + bm["p3"]) / (t_edt * 1e-3) / 1e9,
                       "sample_model_GBps": bm["sample"] / (t_s * 1e-3) / 1e9, "bytes": bm}
    # CPU oracle on the smallest label's box
    from tests.helpers import distance_ref as oracle
    counts = [(int((ref == c).sum()), c) for c in range(1, k)]
    c = min(cc for cc in counts if cc[0] > 0)[1]
    m = ((pred == c) | (ref == c)).nonzero()
    lo, hi = m.min(0).values.tolist(), (m.max(0).values + 1).tolist()
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    p_np, r_np = (pred[sl] == c).cpu().numpy(), (ref[sl] == c).cpu().numpy()
    t0 = time.perf_counter()
    oracle.metrics(p_np, r_np, spacing)
    res["cpu_oracle"] = {"label": c, "box": [b - a for a, b in zip(lo, hi)], "CPU_s": time.perf_counter() - t0}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
