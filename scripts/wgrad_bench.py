#!/usr/bin/env python3
"""Cold-cache timings of the weight-gradient launches of the benchmark step (bf16, B=8, 128^3 net):
   python scripts/wgrad_bench.py [B]"""
import sys, torch
sys.path.insert(0, ".")
from segmantic_amd import ops
DEV = "cuda:0"
flush = torch.empty(256 << 20, device=DEV)

def run(name, xs, dys, k, s, tf=False, reps=6):
    x = torch.randn(xs, device=DEV).bfloat16()
    dy = torch.randn(dys, device=DEV).bfloat16()
    dw = torch.empty((dys[-1], xs[-1], k, k, k), device=DEV)
    ws = torch.empty(ops.conv3d_wgrad_workspace(x, dy, k, s), dtype=torch.uint8, device=DEV)
    in_tf = None
    if tf:
        c = xs[-1]
        in_tf = (torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV) * 0.1, torch.full((1,), 0.25, device=DEV))
    for _ in range(2):
        ops.conv3d_wgrad(x, dy, dw, None, k, s, ws, in_tf=in_tf)
    tot = 0.0
    for _ in range(reps):
        flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.conv3d_wgrad(x, dy, dw, None, k, s, ws, in_tf=in_tf)
        e1.record(); torch.cuda.synchronize()
        tot += e0.elapsed_time(e1)
    nbytes = (x.numel() + dy.numel()) * 2
    us = tot / reps * 1e3
    print(f"{name:34s} {us:8.1f} us  {nbytes / us / 1e6:6.2f} TB/s algorithmic (incl. slab reduce)")

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
run("top 16x16 s1 @128^3", (B, 128, 128, 128, 16), (B, 128, 128, 128, 16), 3, 1)
run("top 16x16 s1 @128^3 + in_tf", (B, 128, 128, 128, 16), (B, 128, 128, 128, 16), 3, 1, tf=True)
run("upconvT top: x16@128^3 dy32@64^3 s2", (B, 128, 128, 128, 16), (B, 64, 64, 64, 32), 3, 2)
run("L0 16x16 s1 @64^3", (B, 64, 64, 64, 16), (B, 64, 64, 64, 16), 3, 1)
run("L1 unit0 16->32 s2 (x@64^3)", (B, 64, 64, 64, 16), (B, 32, 32, 32, 32), 3, 2)
run("L1 unit1 32x32 s1 @32^3", (B, 32, 32, 32, 32), (B, 32, 32, 32, 32), 3, 1)
run("upconvT L1: x16@64^3 dy64@32^3 s2", (B, 64, 64, 64, 16), (B, 32, 32, 32, 64), 3, 2)
run("L2 unit0 32->64 s2 (x@32^3)", (B, 32, 32, 32, 32), (B, 16, 16, 16, 64), 3, 2)
run("L2 unit1 64x64 s1 @16^3", (B, 16, 16, 16, 64), (B, 16, 16, 16, 64), 3, 1)
run("upconvT L2: x32@32^3 dy128@16^3 s2", (B, 32, 32, 32, 32), (B, 16, 16, 16, 128), 3, 2)
run("L3 unit1 128x128 s1 @8^3", (B, 8, 8, 8, 128), (B, 8, 8, 8, 128), 3, 1)
run("bottom 256x256 s1 @8^3", (B, 8, 8, 8, 256), (B, 8, 8, 8, 256), 3, 1)
