#!/usr/bin/env python3
"""Records tests/golden/conv_plan_parent.json: what the convolution family's host-side queries answer for a table
of layers -- kernel name, statistics rows, fusion capabilities, weight-gradient workspace.  The table was recorded
from the commit BEFORE the launch decisions moved into csrc/conv_plan.h, and tests/test_conv_plan_host.py holds every
later build to it, so the file is regenerated only when a selection outcome is changed on purpose.

The queries are host arithmetic over fabricated views (tests/helpers/conv_plan_queries.py): no GPU is needed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_conv_plan_goldens.py
"""
import json
import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

if "SEGMI_WGRAD_CUS" in os.environ:
    sys.exit("SEGMI_WGRAD_CUS overrides the `cus` argument of the workspace query: unset it")

from segmantic_amd import _lib  # noqa: E402
from tests.helpers.conv_plan_queries import CASE_FIELDS, evaluate  # noqa: E402

F32, BF16, F16 = 0, 1, 2
CIN = (1, 3, 4, 5, 16, 32, 48, 64, 128, 256)
COUT = (3, 16, 32, 48, 64, 128, 256)
KS = ((3, 1), (3, 2), (1, 1))
# (n, d, h, w) of the input view.  w 8 / 9 / 16 / 17 (and their stride-2 images 4 / 5 / 8 / 9 from 8 / 9 / 16 / 17 / 18)
W_EXT = [(1, 8, 8, 8), (1, 8, 8, 9), (1, 8, 8, 16), (1, 8, 8, 17), (1, 8, 8, 18), (2, 8, 8, 20)]
# ring: columns = n * ceil(h/8) * ceil(w/16) at 255 / 256 and 128 x (15 | 16 steps of 4 planes), too few steps, the
# full-resolution layers
RING_EXT = [(1, 16, 128, 256), (1, 16, 120, 272), (4, 60, 64, 64), (4, 64, 64, 64), (8, 12, 64, 64), (8, 16, 64, 64),
            (8, 128, 128, 128), (2, 64, 64, 64), (1, 128, 128, 128), (1, 20, 24, 24)]
# the 512-workgroup rules of the tile, k-split and transposed kernels (deep levels), tiles per persistent workgroup
# 1 / 4 / 8 / 16
WG_EXT = [(8, 8, 8, 8), (8, 16, 16, 16), (1, 32, 32, 32), (2, 32, 32, 32), (8, 32, 32, 32), (8, 64, 64, 64), (2, 24, 24, 24)]
# non-cubic, depth 1 (the 2-D networks)
FLAT_EXT = [(4, 1, 64, 64), (2, 1, 128, 96), (1, 1, 256, 256), (1, 5, 37, 50), (3, 7, 9, 33)]
# one sample past each 32-bit limit: the ring's (d + 8) h w 4 cin 2 >= 2^31, ring3's output sample in 4-fold rows,
# the 416^3 sample of tests/test_ops_gpu.py, the weight gradient's 4 GiB batch split (8 x 160^3 in 96-wide rows; 64-wide
# rows stay just inside one descriptor)
BIG_EXT = [(1, 256, 256, 256), (1, 160, 160, 160), (1, 416, 416, 416), (8, 160, 160, 160)]
ALL_EXT = W_EXT + RING_EXT + WG_EXT + FLAT_EXT


def case(dt, ext, cin, cout, ks, ldi_mul=1, ioff=0, ldo_mul=1, ooff=0):
    return (dt, *ext, cin, cin * ldi_mul, ioff, cout, cout * ldo_mul, ooff, *ks)


cases, tags = [], {}


def add(c, tag=None):
    if c not in cases:
        cases.append(c)
    if tag:
        tags[tag] = cases.index(c)


# 1. every dtype x cin x cout x (k, s), the extent / row stride / pointer offset cycling through their lists
i = 0
for dt in (F32, BF16, F16):
    for cin in CIN:
        for cout in COUT:
            for ks in KS:
                ext = ALL_EXT[i % len(ALL_EXT)]
                add(case(dt, ext, cin, cout, ks, (1, 2, 4)[(i // 3) % 3], (0, 0, 8, 0, 16)[(i // 7) % 5], (1, 2, 4)[(i // 5) % 3]))
                i += 1
# 2. every threshold extent x the channel pairs that reach each family
PAIRS = [(16, 16), (32, 32), (32, 48), (64, 64), (16, 32), (32, 16), (4, 16), (5, 3)]
for dt in (F32, BF16):
    for ext in ALL_EXT:
        for cin, cout in PAIRS:
            for ks in KS:
                add(case(dt, ext, cin, cout, ks))
for ext in RING_EXT + W_EXT:
    for cin, cout in PAIRS[:4]:
        add(case(F16, ext, cin, cout, (3, 1)))
# 3. row strides c / 2c / 4c and pointer offsets 0 / 8 / 16 on the ring and k-split shapes
for dt in (BF16, F16, F32):
    for ext in [(8, 16, 64, 64), (8, 128, 128, 128), (8, 16, 16, 16)]:
        for cin, cout in [(16, 16), (32, 32), (16, 64), (128, 128)]:
            for ldm in (1, 2, 4):
                for ioff in (0, 8, 16):
                    add(case(dt, ext, cin, cout, (3, 1), ldm, ioff, ldm))
            add(case(dt, ext, cin, cout, (3, 1), 1, 0, 1, 8))      # the OUTPUT 8 bytes in
for dt in (F32, BF16, F16):
    for ooff in (8, 16):
        add(case(dt, (1, 32, 32, 32), 1, 16, (3, 2), 1, 0, 1, ooff))
# 4. past the 32-bit limits
for dt in (BF16, F16, F32):
    for ext in BIG_EXT:
        for cin, cout, ldi_mul, ldo_mul in [(16, 16, 1, 1), (16, 64, 1, 4), (32, 32, 2, 1), (32, 32, 3, 1), (32, 32, 1, 1), (16, 16, 4, 4)]:
            for ks in KS:
                add(case(dt, ext, cin, cout, ks, ldi_mul, 0, ldo_mul))
# 5. the named layers: one per kernel family and weight-gradient path (tests/test_conv_plan_gpu.py runs these)
add(case(BF16, (8, 16, 64, 64), 16, 16, (3, 1)), "fwd:ring3")
add(case(BF16, (8, 16, 64, 64), 32, 32, (3, 1)), "fwd:ring2 ck32 nt2")
add(case(BF16, (8, 16, 64, 64), 32, 48, (3, 1)), "fwd:ring2 ck32 nt1")
add(case(BF16, (8, 16, 64, 64), 16, 16, (3, 1), 2, 8), "fwd:ring2 ck16")
add(case(BF16, (1, 8, 8, 8), 64, 64, (3, 1)), "fwd:k-split")
add(case(F32, (2, 8, 8, 20), 128, 128, (3, 1)), "fwd:k-split wide")
add(case(BF16, (1, 20, 24, 24), 16, 16, (3, 1)), "fwd:tile k3 s1")
add(case(BF16, (1, 16, 16, 16), 32, 64, (3, 2)), "fwd:tile k3 s2")
add(case(BF16, (1, 8, 8, 20), 16, 16, (1, 1)), "fwd:tile k1")
add(case(F32, (1, 64, 64, 64), 1, 16, (3, 2)), "fwd:small-cin")
add(case(F32, (2, 24, 24, 24), 5, 7, (3, 1)), "fwd:direct")
add(case(BF16, (1, 8, 8, 16), 32, 16, (3, 2)), "convT:persistent")
add(case(BF16, (1, 8, 8, 8), 32, 16, (3, 2)), "convT:tile")
add(case(BF16, (8, 64, 64, 64), 32, 32, (3, 1)), "wgrad:wave-specialised")
add(case(F32, (2, 16, 16, 16), 32, 32, (3, 1)), "wgrad:mfma")
add(case(F32, (1, 64, 64, 64), 1, 16, (3, 2)), "wgrad:small-cin")
add(case(BF16, (8, 64, 64, 64), 32, 32, (3, 1), 1, 8), "wgrad:direct")
add(case(BF16, (8, 160, 160, 160), 32, 32, (3, 1), 3), "wgrad:batch parts")

names, rows = [], []
for c in cases:
    r = evaluate(_lib, c)
    if r[0] not in names:
        names.append(r[0])
    rows.append(list(c) + [names.index(r[0])] + r[1:])

out = Path(__file__).resolve().parent / "conv_plan_parent.json"
text = json.dumps({"fields": list(CASE_FIELDS), "names": names, "tags": tags, "rows": rows}, separators=(",", ":"))
out.write_text(text.replace("],[", "],\n[") + "\n")
print(f"{len(rows)} cases, {len(names)} kernel names, {out.stat().st_size} bytes -> {out}")
for nm in sorted(names):
    print("  ", nm)
