"""Test-time-augmentation benchmark: ``segmi_tta_accumulate`` and ``segmi_tta_finalize`` on a seeded
--size^3 x --classes volume, against their byte models and against the plain torch composition
``acc += softmax(flip(logits))`` on the same tensors.

Device events around each call, the median of --repeats runs after one warm-up, one process.  Byte models (f32):
accumulate = logits read + accumulator read and written = 3 K 4 bytes per voxel; finalize = scores read + label
(1 byte), confidence and entropy written = 4 K + 9 bytes per voxel.

    python scripts/tta_bench.py [--size 256] [--classes 16] [--repeats 5] [--mask 7]
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
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mask", type=int, default=7, help="axes mirrored in the timed pass (bit 0 = d, 1 = h, 2 = w)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from segmantic_amd import ops
    assert torch.cuda.is_available(), "tta_bench needs an MI355X"
    dev = torch.device("cuda:0")
    n, K = args.size, args.classes
    g = torch.Generator(device=dev).manual_seed(args.seed)
    logits = torch.randn((1, n, n, n, K), generator=g, device=dev) * 3.0
    acc = torch.empty((n, n, n, K), dtype=torch.float32, device=dev)
    ops.tta_accumulate(logits, 0, acc, True)
    nvox = n ** 3
    res = {"size": n, "classes": K, "mask": args.mask, "repeats": args.repeats}

    def rate(r, bytes_per_voxel):
        r["model_bytes"] = nvox * bytes_per_voxel
        r["model_GBps"] = r["model_bytes"] / (r["ms_median"] * 1e-3) / 1e9
        return r

    for name, mask in (("accumulate_identity", 0), ("accumulate_mirrored", args.mask)):
        res[name] = rate(_timed(lambda: ops.tta_accumulate(logits, mask, acc, False), args.repeats), 3 * K * 4)
    # the torch composition on the same tensors: flip (a copy), softmax (a copy), add in place
    dims = [1 + a for a in range(3) if args.mask & (1 << a)]
    acc5 = acc[None]
    res["torch_accumulate_mirrored"] = rate(
        _timed(lambda: acc5.add_(torch.softmax(torch.flip(logits, dims), dim=-1)), args.repeats), 3 * K * 4)
    res["torch_accumulate_identity"] = rate(
        _timed(lambda: acc5.add_(torch.softmax(logits, dim=-1)), args.repeats), 3 * K * 4)
    res["accumulate_speedup_vs_torch"] = (res["torch_accumulate_mirrored"]["ms_median"]
                                          / res["accumulate_mirrored"]["ms_median"])

    ops.tta_accumulate(logits, 0, acc, True)       # finalize a well-formed accumulator (2 passes)
    ops.tta_accumulate(logits, args.mask, acc, False)
    lab = torch.empty((1, n, n, n), dtype=torch.uint8, device=dev)
    conf = torch.empty((1, n, n, n), dtype=torch.float32, device=dev)
    ent = torch.empty((1, n, n, n), dtype=torch.float32, device=dev)
    res["finalize"] = rate(_timed(lambda: ops.tta_finalize(acc5, lab, conf, ent), args.repeats), 4 * K + 9)

    def torch_finalize():
        q = acc5 / acc5.sum(-1, keepdim=True)
        c, l = q.max(-1)
        e = -(torch.xlogy(q, q)).sum(-1) / float(np.log(K))
        return l.to(torch.uint8), c, e.clamp_(0, 1)
    res["torch_finalize"] = rate(_timed(torch_finalize, args.repeats), 4 * K + 9)
    res["finalize_speedup_vs_torch"] = res["torch_finalize"]["ms_median"] / res["finalize"]["ms_median"]
    res["finalize_probs_in_place"] = rate(
        _timed(lambda: ops.tta_finalize(acc5, lab, conf, ent, probs_out=acc5), args.repeats), 8 * K + 9)
    vals = ent.view(-1)
    res["label_means"] = rate(_timed(lambda: ops.label_means(lab.view(-1), vals, K), args.repeats), 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
