"""Morphology benchmark: the feature transform and the label operations on a seeded synthetic 512^3 label map
with 16 ellipsoid labels (some touch the volume border).

Reports the median of --repeats device-synchronised runs of the whole-volume feature transform (events around
the three passes, against the byte model below), of expand_labels and of open_labels over all labels (host
clock, end to end from a device tensor), and beside them the CPU time of scipy's
distance_transform_edt(return_indices=True) on the same volume (labelled CPU).  Every GPU step runs in a child
process of its own under its own time limit; the first step that fails or overruns ends the benchmark.

    python scripts/morphology_bench.py [--size 512] [--labels 16] [--repeats 5] [--no-scipy]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

STEP_LIMIT_S = {"feature_transform": 240, "expand_labels": 240, "open_labels": 420}
EDT_SQ_MS_512 = 4.79          # segmi_edt_sq on a 512^3 box
EDT_SQ_BYTES = 13 + 24 + 24   # per voxel, its three passes


def byte_model(n: int) -> dict:
    """bytes each pass of the feature transform moves for n voxels (uint8 labels, one i32 per voxel in place,
    the stack charged in full: one (position, payload) entry written and read per voxel)"""
    return {
        "p1": n * (1 + 4 + 1 + 4 + 4),      # labels, left candidate written; labels again, read, final written
        "p2": n * (4 + 8 + 8 + 4),          # read, stack write + read, write
        "p3": n * (4 + 8 + 8 + 4),          # the same (+ 4 when distances are written; not timed here)
    }


def bench_volume(size: int, labels: int, seed: int, dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    z, y, x = torch.meshgrid(*[torch.arange(size, device=dev, dtype=torch.float32)] * 3, indexing="ij")
    vol = torch.zeros((size, size, size), dtype=torch.uint8, device=dev)
    for c in range(1, labels + 1):
        r = (torch.rand(3, generator=g) * 0.12 + 0.03) * size
        ctr = torch.rand(3, generator=g) * size
        if c % 5 == 0:
            ctr[c % 3] = 0.0 if c % 2 else size - 1.0      # touches the border
        inside = (((z - ctr[0]) / r[0]) ** 2 + ((y - ctr[1]) / r[1]) ** 2 + ((x - ctr[2]) / r[2]) ** 2) <= 1.0
        vol[inside] = c
    return vol.contiguous()


def _median(ms):
    return {"ms_median": float(np.median(ms)), "ms_all": [round(float(v), 3) for v in ms]}


def run_step(step: str, args) -> dict:
    import torch
    from segmantic_amd import ops
    from segmantic_amd.seg import morphology
    assert torch.cuda.is_available(), "morphology_bench needs an MI355X"
    dev = torch.device("cuda:0")
    vol = bench_volume(args.size, args.labels, args.seed, dev)
    n = vol.numel()
    torch.cuda.synchronize()
    if step == "feature_transform":
        index = torch.empty(vol.shape, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.feature_transform_workspace_bytes(vol.shape), dtype=torch.uint8, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.repeats + 1):
            e0.record()
            ops.feature_transform(vol, ops.FT_NONZERO, (1.0, 1.0, 1.0), index=index, workspace=ws)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        res = _median(ms[1:])
        bm = byte_model(n)
        total = sum(bm.values())
        res.update({"bytes": bm, "model_GBps": total / (res["ms_median"] * 1e-3) / 1e9,
                    "yardstick_ms": EDT_SQ_MS_512 * (n / 512 ** 3) * (total / n) / EDT_SQ_BYTES,
                    "feature_share": float((vol != 0).float().mean().item())})
        return res
    fn = {"expand_labels": lambda: morphology.expand_labels(vol, args.radius),
          "open_labels": lambda: morphology.open_labels(vol, args.radius)}[step]
    fn()                                                               # warm-up
    ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return _median(ms)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--radius", type=float, default=2.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-scipy", action="store_true", help="skip the CPU comparison")
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), help="run one GPU step in this process (internal)")
    args = ap.parse_args()
    if args.step:
        print("STEP_RESULT " + json.dumps(run_step(args.step, args)))
        return
    res = {"size": args.size, "labels": args.labels, "radius": args.radius, "repeats": args.repeats}
    for step in ("feature_transform", "expand_labels", "open_labels"):
        cmd = [sys.executable, __file__, "--step", step, "--size", str(args.size), "--labels", str(args.labels),
               "--repeats", str(args.repeats), "--radius", str(args.radius), "--seed", str(args.seed)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            res[step] = {"error": f"time limit of {STEP_LIMIT_S[step]} s"}
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if p.returncode != 0 or not lines:
            res[step] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            break                                                      # nothing more is started on the GPU
        res[step] = json.loads(lines[-1][len("STEP_RESULT "):])
    if not args.no_scipy and all("error" not in v for v in res.values() if isinstance(v, dict)):
        from scipy import ndimage
        import torch
        vol = bench_volume(args.size, args.labels, args.seed, torch.device("cpu")).numpy()
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(vol == 0, return_indices=True)
        res["scipy_edt_return_indices"] = {"CPU_s": time.perf_counter() - t0}
    print(json.dumps(res))
    if any(isinstance(v, dict) and "error" in v for v in res.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
