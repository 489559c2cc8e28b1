"""Label-surface benchmark: discrete surface nets of the distance_bench.py volume (seeded 512^3 uint8, 16
ellipsoid labels, some on the border), all labels in one call, and one single-label case whose box is the whole
volume (the union of the ellipsoids plus two corner voxels).

Reports, as median (min-max) of --repeats runs after a warm-up: the kernel groups (boxes, count incl. the scan,
emit, relax = --smooth sweeps + the physical transform, measure) timed with device events, GB/s against the byte
model below, the end-to-end time of extract_surfaces (host clock around a device synchronise) with the number of
device-to-host copies it made for 1 and for all labels, and, as context only, the numpy oracle on one label's box.

With --decimate R the all-label meshes are also decimated (segmantic_amd.ops.decimate_meshes): rounds, the
device-event span of the whole decimation (it holds one live-count copy per round, so it includes the host's wait
between rounds), that span per round, its device-to-host copies, the byte model per round and the end-to-end
time of extract_surfaces with decimation.

    python scripts/surface_bench.py [--size 512] [--labels 16] [--repeats 5] [--smooth 5] [--no-oracle]
                                    [--decimate R]
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
from segmantic_amd.image import surfaces  # noqa: E402


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


def kernel_times(vol, selected, reps: int, smooth: int):
    """device-event times of the kernel groups and the byte model: labels are charged one byte per voxel or cell
    (the 2x2 rows a cell reads are shared with its neighbours through the caches), chunk records 16 bytes; the
    gathers of neighbour offsets (relax) and of face vertices (measure) are not charged, so those GB/s figures
    are lower bounds on what the hardware moved"""
    n = vol.numel()
    boxes = ops.surface_boxes(vol, selected).cpu().numpy()
    ws = torch.empty(ops.surface_workspace_bytes(vol.shape, selected, boxes), dtype=torch.uint8, device=vol.device)
    starts_dev = ops.surface_count(vol, selected, boxes, ws)
    starts = starts_dev.cpu().numpy()
    nv, nf = int(starts[-2, 0]), int(starts[-2, 1])
    grown = boxes[:, 1::2] - boxes[:, 0::2] + 1
    chunks = int((grown[:, 0] * grown[:, 1] * (boxes[:, 5] // 64 - boxes[:, 4] // 64 + 1)).sum())
    cells = chunks * 64
    offs, cell_xyz, nbr, faces = ops.surface_emit(vol, selected, boxes, ws, nv, nf, with_neighbours=True)
    geo = (np.zeros(3), np.eye(3), np.ones(3))
    verts = ops.surface_relax(offs.clone(), cell_xyz, nbr, 0, 0.5, *geo)
    res = {"vertices": nv, "faces": nf, "chunks": chunks, "box_cells": cells, "box_cells_over_voxels": cells / n}
    res["boxes"] = time_events(lambda: ops.surface_boxes(vol, selected), reps)
    res["count"] = time_events(lambda: ops.surface_count(vol, selected, boxes, ws), reps)
    res["emit"] = time_events(lambda: ops.surface_emit(vol, selected, boxes, ws, nv, nf, with_neighbours=True), reps)
    res["relax"] = time_events(lambda: ops.surface_relax(offs, cell_xyz, nbr, smooth, 0.5, *geo), reps)
    res["measure"] = time_events(lambda: ops.surface_measure(verts, faces, starts_dev), reps)
    model = {
        "boxes": n,
        "count": cells + chunks * 16 + chunks * 2 * (8 + 8),          # classify, then sum + apply of the scan
        "emit": cells + chunks * 16 + nv * (12 + 12 + 24) + nf * 12,
        "relax": smooth * nv * (12 + 24 + 12) + nv * (12 + 12 + 12),
        "measure": nf * 12,
    }
    for k, b in model.items():
        res[k]["model_bytes"] = int(b)
        res[k]["gb_per_s"] = b / (res[k]["median_ms"] * 1e-3) / 1e9
    res["kernel_total_ms"] = sum(res[k]["median_ms"] for k in model)
    return res


def decimate_times(vol, selected, reps: int, smooth: int, reduction: float):
    """decimation of the all-label meshes.  Byte model of one round over V vertices and F faces (stars hold 3 F
    entries): count 12 F, scan 16 V, fill 12 F + 12 F, classify 3 F * (4 + 12) + 4 * 3 F + 17 V, candidate
    3 F * 4 + 80 V + 6 * (3 F / V) rings and faces gathered per vertex (not charged), claim 8 V + 3 F * 4,
    apply 8 V + 3 F * 4: about 140 F + 130 V bytes charged, a lower bound as the gathers are left out"""
    boxes = ops.surface_boxes(vol, selected).cpu().numpy()
    ws = torch.empty(ops.surface_workspace_bytes(vol.shape, selected, boxes), dtype=torch.uint8, device=vol.device)
    starts_dev = ops.surface_count(vol, selected, boxes, ws)
    starts = starts_dev.cpu().numpy()
    nv, nf = int(starts[-2, 0]), int(starts[-2, 1])
    offs, cell_xyz, nbr, faces = ops.surface_emit(vol, selected, boxes, ws, nv, nf, with_neighbours=True)
    verts = ops.surface_relax(offs, cell_xyz, nbr, smooth, 0.5, np.zeros(3), np.eye(3), np.ones(3))
    stats = {}
    out = ops.decimate_meshes(verts, faces, starts_dev, starts, reduction, 128, stats)
    res = {"reduction": reduction, "vertices_in": nv, "faces_in": nf, "vertices_out": int(out[0].shape[0]),
           "faces_out": int(out[1].shape[0]), "rounds": stats["rounds"], "d2h_copies": stats["d2h_copies"],
           "model_bytes_per_round_first": 140 * nf + 130 * nv}
    res["total"] = time_events(lambda: ops.decimate_meshes(verts, faces, starts_dev, starts, reduction, 128), reps)
    res["per_round"] = {k: v / max(1, stats["rounds"]) for k, v in res["total"].items()}
    res["gb_per_s_first_round_model"] = res["model_bytes_per_round_first"] / (res["per_round"]["median_ms"] * 1e-3) / 1e9
    return res


def count_copies(fn) -> int:
    """device-to-host copies (Tensor.cpu / Tensor.tolist of a device tensor) made by fn: each one synchronises"""
    calls = [0]
    cpu, tolist = torch.Tensor.cpu, torch.Tensor.tolist

    def cpu_(self, *a, **k):
        calls[0] += int(self.is_cuda)
        return cpu(self, *a, **k)

    def tolist_(self, *a, **k):
        calls[0] += int(self.is_cuda)
        return tolist(self, *a, **k)

    torch.Tensor.cpu, torch.Tensor.tolist = cpu_, tolist_
    try:
        fn()
    finally:
        torch.Tensor.cpu, torch.Tensor.tolist = cpu, tolist
    return calls[0]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--smooth", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--decimate", type=float, default=0.0, help="also decimate the all-label meshes by this share")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench needs an MI355X; a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    vol = bench_volume(args.size, args.labels, args.seed, dev)
    present = [c for c in range(1, args.labels + 1) if bool((vol == c).any())]
    result = {"size": args.size, "labels": args.labels, "present": len(present), "voxels": vol.numel(),
              "smooth": args.smooth, "all_labels": kernel_times(vol, present, args.repeats, args.smooth)}
    one = (vol != 0).to(torch.uint8)
    one[0, 0, 0] = one[-1, -1, -1] = 1                 # the box of label 1 is the whole volume
    result["whole_volume_one_label"] = kernel_times(one.contiguous(), [1], args.repeats, args.smooth)
    result["all_labels_over_n_whole_volume_passes"] = result["all_labels"]["kernel_total_ms"] / (
        len(present) * result["whole_volume_one_label"]["kernel_total_ms"])
    result["end_to_end"] = {
        "all_labels": time_host(lambda: surfaces.extract_surfaces(vol, smooth_iterations=args.smooth), args.repeats),
        "one_label": time_host(lambda: surfaces.extract_surfaces(vol, [present[0]], smooth_iterations=args.smooth),
                               args.repeats),
    }
    # device-to-host copies: the range check (aminmax, run for every dtype: it also gives the largest label for
    # the default selection) + 3 results (boxes, totals, measures); the meshes themselves are copied only when
    # the input lived on the host
    result["device_to_host_copies"] = {
        "one_label": count_copies(lambda: surfaces.extract_surfaces(vol, [present[0]])),
        "all_labels": count_copies(lambda: surfaces.extract_surfaces(vol)),
    }
    if args.decimate > 0.0:
        result["decimate"] = decimate_times(vol, present, args.repeats, args.smooth, args.decimate)
        result["decimate"]["end_to_end_all_labels"] = time_host(
            lambda: surfaces.extract_surfaces(vol, smooth_iterations=args.smooth, decimate=args.decimate), args.repeats)
        result["decimate"]["end_to_end_d2h_copies"] = count_copies(
            lambda: surfaces.extract_surfaces(vol, smooth_iterations=args.smooth, decimate=args.decimate))
    if not args.no_oracle:
        from tests.helpers import surface_ref

        c = present[0]
        b = ops.surface_boxes(vol, [c]).cpu().numpy()[0]
        crop = vol[b[0]:b[1], b[2]:b[3], b[4]:b[5]].cpu().numpy()
        t = time.perf_counter()
        got = surface_ref.surface_nets(crop, c)
        result["numpy_oracle_one_label_box"] = {"label": c, "box": [int(v) for v in b], "vertices": int(got["index"].shape[0]),
                                                "ms_cpu": (time.perf_counter() - t) * 1e3}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
