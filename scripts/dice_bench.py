#!/usr/bin/env python3
"""Loss forward / backward kernels in isolation at the benchmark shape (B=8 x 128^3, K=16), cold caches:
Dice, Dice + cross-entropy, Tversky and Dice + focal, bf16 and f32, the backward with the fused bias gradient (as
``Net.training_step`` runs it).  The losses alternate inside every repetition, so all see the same machine state.

Byte model (what each pass has to move): forward = logits + labels read; backward = logits + labels read and
dlogits written.  The partial rows, coefficients and bias sums are a few hundred KB and are left out.

    python scripts/dice_bench.py [--reps 20] [--json] [--losses Dice,DiceCE]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from segmantic_amd.seg.losses import DiceCELoss, DiceFocalLoss, DiceLoss, TverskyLoss  # noqa: E402

DEV = "cuda:0"
N, S, K = 8, 128, 16


def bytes_moved(dtype, backward: bool) -> int:
    vox = N * S ** 3
    elem = torch.finfo(dtype).bits // 8
    return vox * K * elem * (2 if backward else 1) + vox * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", action="store_true", help="one JSON line per (dtype, loss, pass)")
    ap.add_argument("--losses", default="Dice,DiceCE,Tversky,DiceFocal", help="comma-separated subset, in this order")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dice_bench needs an MI355X")
    g = torch.Generator(device=DEV).manual_seed(0)
    lab = torch.randint(0, K, (N, 1, S, S, S), device=DEV, generator=g).float()
    flush = torch.empty(256 << 20, device=DEV)          # larger than the 256 MB last-level cache
    for dtype in (torch.bfloat16, torch.float32):
        lg = torch.randn((N, S, S, S, K), device=DEV, generator=g).to(dtype)
        out = torch.empty_like(lg)
        bias = torch.empty(K, device=DEV)
        weight = [0.5] + [1.0] * (K - 1)
        losses = {"Dice": DiceLoss(), "DiceCE": DiceCELoss(weight=weight),
                  "Tversky": TverskyLoss(exponent=0.75), "DiceFocal": DiceFocalLoss(gamma=2.0, weight=weight)}
        losses = {name: losses[name] for name in args.losses.split(",")}
        passes = {}
        for name, mod in losses.items():
            passes[name, "fwd"] = (lambda m=mod: m.forward_ndhwc(lg, lab), False)
            passes[name, "bwd"] = (lambda m=mod: m.backward_ndhwc(lg, 1.0, out, bias_grad=bias), True)
        times = {key: [] for key in passes}
        for fn, _ in passes.values():                   # warm-up: code objects, scratch buffers
            fn()
            fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for key, (fn, _) in passes.items():         # Dice fwd, Dice bwd, DiceCE fwd, DiceCE bwd, repeat
                flush.fill_(1.0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3)
        for (name, which), ts in times.items():
            ts = sorted(ts)
            med = statistics.median(ts)
            nbytes = bytes_moved(dtype, passes[name, which][1])
            row = {"dtype": str(dtype).replace("torch.", ""), "loss": name, "pass": which, "median_us": round(med, 1),
                   "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1), "reps": len(ts),
                   "model_bytes": nbytes, "tb_per_s": round(nbytes / med / 1e6, 3)}
            if args.json:
                print(json.dumps(row))
            else:
                print(f"{row['dtype']:>8} {name:>9} {which}: median {med:8.1f} us  [{ts[0]:8.1f} .. {ts[-1]:8.1f}]  "
                      f"{row['tb_per_s']:.2f} TB/s of the byte model")
        for name, mod in losses.items():
            print(f"{str(dtype).replace('torch.', ''):>8} {name:>9} loss {float(mod.forward_ndhwc(lg, lab)):.6f}")


if __name__ == "__main__":
    main()
