"""fp16 vs bf16 training step of the benchmark workload (UNet 16-32-64-128-256, 16 labels, batch 8 x 128^3,
Adam), in ONE process, timed as bench.py times it: K steps between two device-wide synchronisations.  The two
precisions are timed in alternating windows (``--reps`` each), so drift of the shared host hits both alike.

Also reported, after the timed windows: the share of fp16 Dice gradients (dlogits, scaled by the default 2^16
loss scale) that are subnormal / zero in fp16, the loss scale and the skipped-step count.

  python scripts/fp16_step_bench.py [--steps 10] [--warmup 3] [--reps 5] [--out DIR]
  python scripts/fp16_step_bench.py --only fp16 --steps 2 --warmup 1 --reps 1   # a short run for rocprofv3
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def synthetic(batch, size, classes, seed, device):
    """bench.py's synthetic batch: randn images, blob-like integer labels stored as float"""
    g = torch.Generator(device="cpu").manual_seed(1234 + seed)
    img = torch.randn((batch, 1, size, size, size), generator=g)
    ax = torch.arange(size, dtype=torch.float32)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    lab = torch.empty((batch, 1, size, size, size))
    for b in range(batch):
        c = [size * (0.35 + 0.3 * ((b * 7 + i * 3 + seed) % 5) / 4.0) for i in range(3)]
        r = torch.sqrt((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2)
        lab[b, 0] = torch.clamp(torch.floor(classes * (1.0 - r / (0.75 * size))), 0, classes - 1)
    return img.to(device), lab.to(device)


def make_net(classes, size, mode, device):
    from segmantic_amd.seg.monai_unet import Net
    torch.manual_seed(0)
    net = Net(num_classes=classes, num_channels=1, spatial_size=[size] * 3)
    net.mixed_precision = mode
    return net.to(device).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per precision (alternating)")
    ap.add_argument("--only", choices=("bf16", "fp16"), default=None)
    ap.add_argument("--out", default=None, help="directory for fp16_step_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp16_step_bench: needs an MI355X")
    dev = torch.device("cuda:0")
    img, lab = synthetic(args.batch, args.size, args.classes, 0, dev)
    batch = {"image": img, "label": lab}
    modes = [args.only] if args.only else ["bf16", "fp16"]
    nets = {m: make_net(args.classes, args.size, m, dev) for m in modes}
    for m in modes:
        for _ in range(args.warmup):
            nets[m].training_step(batch)
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    for _ in range(args.reps):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                nets[m].training_step(batch)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"batch": args.batch, "size": args.size, "classes": args.classes, "steps_per_window": args.steps,
           "reps": args.reps, "ms_per_step": ms,
           "median_ms": {m: statistics.median(v) for m, v in ms.items()}}
    if len(modes) == 2:
        out["fp16_over_bf16"] = out["median_ms"]["fp16"] / out["median_ms"]["bf16"]
    if "fp16" in nets:
        net = nets["fp16"]
        eng = net._engine
        dl = eng._bufs["dlogits"][..., :args.classes].float() if "dlogits" in eng._bufs else None
        if dl is not None:
            a = dl.abs()
            nz = a > 0
            sub = nz & (a < 2.0 ** -14)
            out["dlogits_fp16"] = {"subnormal_fraction": float(sub.float().mean()),
                                   "zero_fraction": float((~nz).float().mean()),
                                   "subnormal_fraction_of_nonzero": float(sub.sum() / nz.sum().clamp(min=1)),
                                   "max_abs": float(a.max()), "loss_scale": net.grad_scaler().get_scale()}
        out["fp16_skipped_steps"] = net.grad_scaler().skipped_steps()
        out["fp16_loss_scale"] = net.grad_scaler().get_scale()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        Path(args.out, "fp16_step_bench.json").write_text(line + "\n")


if __name__ == "__main__":
    main()
