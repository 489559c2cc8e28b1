"""Patch-based label-fusion benchmark: a seeded 256^3 target of 16 ellipsoid labels (17 classes with the
background), 8 atlases made from it by shifts of up to two voxels, a gain of 0.9 .. 1.1 and Gaussian noise, fused with
the adaptive bandwidth at (patch radius, search radius) = (1, 2) and (2, 2).

Reports per setting ms per call (median of --repeats after a warm-up), candidate patches per second (voxels x
atlases x search offsets; the offsets that leave the volume at its faces are counted too, they are 2 % of them) and
GB/s against the byte model "the target read once; every atlas image and label map read once per sweep over the
candidates (two sweeps with the adaptive bandwidth, one with a fixed one); labels, best and total written once".
Beside it the comparator: the same fusion in plain torch on the same device -- per atlas and offset the squared
difference of the rolled image, avg_pool3d for the patch mean, the minimum over the candidates, then exp weights
scattered into a [K, N] score table -- in float32, so it is not bit-equal; its share of voxels that agree with the
HIP result is printed.  No threshold: the figures go into DESIGN.md section 25.

    python scripts/patch_fusion_bench.py [--size 256] [--atlases 8] [--labels 16] [--repeats 3] [--no-torch]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from itertools import product
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd import ops  # noqa: E402

SETTINGS = ((1, 2), (2, 2))


def bench_truth(size: int, labels: int, seed: int, dev) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(seed)
    z, y, x = torch.meshgrid(*[torch.arange(size, device=dev, dtype=torch.float32)] * 3, indexing="ij")
    vol = torch.zeros((size, size, size), dtype=torch.uint8, device=dev)
    for c in range(1, labels + 1):
        r = (torch.rand(3, generator=g) * 0.15 + 0.05) * size
        ctr = torch.rand(3, generator=g) * size
        inside = (((z - ctr[0]) / r[0]) ** 2 + ((y - ctr[1]) / r[1]) ** 2 + ((x - ctr[2]) / r[2]) ** 2) <= 1.0
        vol[inside] = c
    return vol.contiguous()


def bench_inputs(size: int, atlases: int, labels: int, seed: int, dev, noise: float = 8.0):
    """(target u8, atlas images u8, atlas labels u8), quantised over 0 .. 255"""
    truth = bench_truth(size, labels, seed, dev)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    gd = torch.Generator(device=dev).manual_seed(seed + 2)
    means = (20.0 + 215.0 * torch.randperm(labels + 1, generator=g).float() / labels).to(dev)
    draw = lambda lab, gain: (gain * means[lab.long()] +                                     # noqa: E731
                              noise * torch.randn(lab.shape, generator=gd, device=dev)).contiguous()
    tq = ops.quantise_u8(draw(truth, 1.0), 0.0, 255.0)
    iq, ls = [], []
    for _ in range(atlases):
        off = [int(v) for v in torch.randint(-2, 3, (3,), generator=g)]
        lab = torch.roll(truth, off, dims=(0, 1, 2)).contiguous()
        iq.append(ops.quantise_u8(draw(lab, float(torch.rand(1, generator=g)) * 0.2 + 0.9), 0.0, 255.0))
        ls.append(lab)
    return truth, tq, iq, ls


def timed(fn, reps: int):
    ms = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if i:
            ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms)), res


def torch_fusion(tq, iq, ls, K: int, rp: int, rs: int, beta: float = 1.0, min_h2: int = 4) -> torch.Tensor:
    """the comparator: adaptive patch fusion in plain float32 torch (borders by wrap-around and zero padding)"""
    npatch = (2 * rp + 1) ** 3
    t = tq.float()
    shape, n = tq.shape, tq.numel()
    offsets = list(product(range(-rs, rs + 1), repeat=3))

    def distance(img, o):
        moved = torch.roll(img, [-v for v in o], dims=(0, 1, 2))
        e = (t - moved) ** 2
        return torch.nn.functional.avg_pool3d(e[None, None], 2 * rp + 1, 1, rp, count_include_pad=True)[0, 0] * npatch

    dmin = torch.full(shape, float("inf"), device=tq.device)
    imgs = [q.float() for q in iq]
    for img in imgs:
        for o in offsets:
            dmin = torch.minimum(dmin, distance(img, o))
    den = torch.clamp_min(dmin, float(npatch * min_h2)) * beta
    scores = torch.zeros((K, n), device=tq.device)
    for img, lab in zip(imgs, ls):
        for o in offsets:
            w = torch.exp(-distance(img, o) / den)
            moved = torch.roll(lab, [-v for v in o], dims=(0, 1, 2))
            scores.scatter_add_(0, moved.reshape(1, n).long(), w.reshape(1, n))
    return scores.argmax(0).reshape(shape)


def note(msg: str) -> None:
    print(f"# {msg}", file=sys.stderr, flush=True)


def bench_setting(truth, tq, iq, ls, K: int, rp: int, rs: int, reps: int, with_torch: bool) -> dict:
    A, n = len(iq), tq.numel()
    table = torch.from_numpy(ops.patch_fusion_table(1.0).astype(np.int32)).to(tq.device)
    call = timed(lambda: ops.patch_fusion(tq, iq, ls, K, patch_radius=rp, search_radius=rs, table=table,
                                          return_confidence=True), reps)
    out = call[3][0]
    candidates = n * A * (2 * rs + 1) ** 3
    model = n + 2 * A * 2 * n + n + 8 * n                       # two sweeps; u8 images and u8 labels
    res = {"patch_radius": rp, "search_radius": rs, "atlases": A, "classes": K, "voxels": n,
           "variant": ops.patch_fusion_variant_name(K, rp, rs),
           "call_ms": {"median": call[0], "min": call[1], "max": call[2]},
           "candidates_per_s": candidates / (call[0] * 1e-3), "model_bytes": model,
           "model_gb_per_s": model / (call[0] * 1e-3) / 1e9,
           "wrong_share": float((out != truth).float().mean().item())}
    note(f"rp {rp} rs {rs}: {call[0]:.1f} ms per call, {res['candidates_per_s']:.3e} candidates/s, wrong "
         f"{res['wrong_share']:.5f}")
    if with_torch:
        small = tuple(slice(0, 16) for _ in range(3))
        torch_fusion(tq[small].contiguous(), [q[small].contiguous() for q in iq[:1]], [l[small].contiguous() for l in ls[:1]],
                     K, rp, rs)                                  # warm-up on a corner
        t = timed(lambda: torch_fusion(tq, iq, ls, K, rp, rs), 1)
        res["torch_ms"] = t[0]
        res["torch_over_hip"] = t[0] / call[0]
        res["torch_agreement"] = float((t[3] == out).float().mean().item())
        note(f"rp {rp} rs {rs}: plain torch {t[0]:.1f} ms, {res['torch_over_hip']:.1f} x the HIP call, agreement "
             f"{res['torch_agreement']:.5f}")
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--atlases", type=int, default=8)
    ap.add_argument("--labels", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patch_fusion_bench needs an MI355X; a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    truth, tq, iq, ls = bench_inputs(args.size, args.atlases, args.labels, args.seed, dev)
    result = {"size": args.size, "atlases": args.atlases, "labels": args.labels, "cases": []}
    for rp, rs in SETTINGS:
        result["cases"].append(bench_setting(truth, tq, iq, ls, args.labels + 1, rp, rs, args.repeats, not args.no_torch))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
