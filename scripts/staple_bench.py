"""STAPLE label-fusion benchmark: a seeded 512^3 uint8 volume of 16 ellipsoid labels (17 classes with the
background), 5 raters made from it by shifting or dilating single labels by one voxel, and a 16-rater case.

Reports per case the disputed share of the voxels, ms per iteration (the difference of a long and a short call at
tolerance 0, divided by the iterations between them), ms per call at the default settings with its iteration
count, and GB/s against the byte model "every rater volume read once per iteration, labels written once" (the
counting pass and the final pass read every volume once more each; the model charges them too for the call).
Beside it: the same loop in plain torch on the same device (float64 one-hot formulation, voxels in chunks), timed
per iteration, as the comparator.  No threshold: the figures go into DESIGN.md section 22.

    python scripts/staple_bench.py [--size 512] [--labels 16] [--repeats 3] [--raters 5 16] [--no-torch]
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


def bench_volume(size: int, labels: int, seed: int, dev) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(seed)
    z, y, x = torch.meshgrid(*[torch.arange(size, device=dev, dtype=torch.float32)] * 3, indexing="ij")
    vol = torch.zeros((size, size, size), dtype=torch.uint8, device=dev)
    for c in range(1, labels + 1):
        r = (torch.rand(3, generator=g) * 0.12 + 0.03) * size
        ctr = torch.rand(3, generator=g) * size
        inside = (((z - ctr[0]) / r[0]) ** 2 + ((y - ctr[1]) / r[1]) ** 2 + ((x - ctr[2]) / r[2]) ** 2) <= 1.0
        vol[inside] = c
    return vol.contiguous()


def make_raters(truth: torch.Tensor, raters: int, labels: int):
    """rater k redraws the labels c with c % raters == k: odd c shifted by one voxel along axis c % 3, even c
    dilated by one voxel (6-neighbourhood)"""
    out = []
    for k in range(raters):
        t = truth.clone()
        for c in range(1, labels + 1):
            if c % raters != k:
                continue
            m = truth == c
            if c % 2:
                moved = torch.roll(m, 1, dims=c % 3)
                t[m & ~moved] = 0
                t[moved] = c
            else:
                grown = m.clone()
                for d in range(3):
                    grown |= torch.roll(m, 1, dims=d) | torch.roll(m, -1, dims=d)
                t[grown] = c
        out.append(t.contiguous())
    return out


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


def torch_iteration(D, theta, prior, L: int, chunk: int = 1 << 22):
    """one E-step + M-step in plain torch: float64 probabilities, the M-step as one-hot^T @ W per rater"""
    R = len(D)
    S = torch.zeros((R, L, L), dtype=torch.float64, device=prior.device)
    flat = [d.reshape(-1) for d in D]
    for a in range(0, flat[0].numel(), chunk):
        idx = [f[a:a + chunk].long() for f in flat]
        p = prior[None, :].repeat(idx[0].numel(), 1)
        for r in range(R):
            p = p * theta[r][idx[r]]
        w = p / p.sum(1, keepdim=True)
        for r in range(R):
            S[r] += torch.nn.functional.one_hot(idx[r], L).to(torch.float64).T @ w
    T = S[0].sum(0)
    return torch.where(T > 0, S / T.clamp_min(1e-300), torch.zeros_like(S))


def note(msg: str) -> None:
    print(f"# {msg}", file=sys.stderr, flush=True)


def bench_case(D, L: int, reps: int, with_torch: bool) -> dict:
    R, n = len(D), D[0].numel()
    stack = torch.stack([d.reshape(-1) for d in D])
    disputed = float((stack != stack[0]).any(0).float().mean().item())
    del stack
    note(f"{R} raters: disputed share {disputed:.4f}")
    short, long_ = 2, 12
    t_short = timed(lambda: ops.staple(D, L, max_iterations=short, tolerance=0.0), reps)
    t_long = timed(lambda: ops.staple(D, L, max_iterations=long_, tolerance=0.0), reps)
    per_it = (t_long[0] - t_short[0]) / (long_ - short)
    note(f"{R} raters: {short} iterations {t_short[0]:.1f} ms, {long_} iterations {t_long[0]:.1f} ms")
    call = timed(lambda: ops.staple(D, L), reps)
    its = call[3][3]
    note(f"{R} raters: default call {call[0]:.1f} ms, {its} iterations")
    res = {"raters": R, "classes": L, "voxels": n, "table": ops.staple_table_name(R, L), "disputed_share": disputed,
           "ms_per_iteration": per_it, "iteration_model_bytes": R * n,
           "iteration_gb_per_s": R * n / (per_it * 1e-3) / 1e9 if per_it > 0 else None,
           "call_ms": {"median": call[0], "min": call[1], "max": call[2]}, "call_iterations": its,
           "call_converged": call[3][4], "call_model_bytes": (its + 2) * R * n + n,
           "call_gb_per_s": ((its + 2) * R * n + n) / (call[0] * 1e-3) / 1e9}
    if with_torch:
        prior = torch.full((L,), 1.0 / L, dtype=torch.float64, device=D[0].device)
        theta = (torch.eye(L, dtype=torch.float64, device=D[0].device) * 0.9 + 0.1 / L)[None].repeat(R, 1, 1)
        t = timed(lambda: torch_iteration(D, theta, prior, L), 1)
        res["torch_ms_per_iteration"] = t[0]
        res["torch_over_hip"] = t[0] / per_it if per_it > 0 else None
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--raters", type=int, nargs="+", default=[5, 16], help="rater counts to run")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("staple_bench needs an MI355X; a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    truth = bench_volume(args.size, args.labels, args.seed, dev)
    L = args.labels + 1
    result = {"size": args.size, "labels": args.labels, "cases": []}
    for raters in args.raters:
        D = make_raters(truth, raters, args.labels)
        result["cases"].append(bench_case(D, L, args.repeats, not args.no_torch))
        del D
    print(json.dumps(result))


if __name__ == "__main__":
    main()
