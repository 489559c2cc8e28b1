"""The host-side launch-decision queries of the convolution family, asked through the C ABI with fabricated views.

The queries (statistics rows, kernel name, fusion capabilities, weight-gradient workspace) are pure host arithmetic
over the fields of ``segmi_act``: they never touch the memory a view points to.  So the whole decision layer can be
called without a GPU, with views whose ``data`` is a made-up aligned address.  ``evaluate`` turns one case into the
row recorded in ``tests/golden/conv_plan_parent.json``; the generator (``tests/golden/make_conv_plan_goldens.py``)
and the test (``tests/test_conv_plan_host.py``) both go through it.
"""
from __future__ import annotations

import ctypes as C

IN_BASE = 0x10_0000_0000      # fabricated device addresses, 4 KiB aligned and far apart
OUT_BASE = 0x20_0000_0000
OUT2_BASE = 0x30_0000_0000
TOUT_BASE = 0x40_0000_0000
CUS = (0, 64, 128)

# one case: dtype code, input view (n, d, h, w, c, ld, pointer offset in bytes), output channels / row stride / pointer
# offset, ksize, stride.  The output extent follows from the input's.
CASE_FIELDS = ("dtype", "n", "d", "h", "w", "cin", "ldi", "ioff", "cout", "ldo", "ooff", "ksize", "stride")


def out_extent(i: int, ksize: int, stride: int) -> int:
    pad = (ksize - 1) // 2
    return (i + 2 * pad - ksize) // stride + 1


def pair_candidate(cin: int, cout: int, ksize: int) -> bool:
    return ksize == 3 and cin <= 4 and cout in (16, 32)


def views(_lib, case):
    """(in, out, second output of a pair, output of the transposed layer that reads `in`) of a case."""
    dt, n, d, h, w, cin, ldi, ioff, cout, ldo, ooff, k, s = case
    do, ho, wo = (out_extent(e, k, s) for e in (d, h, w))
    a_in = _lib.Act(IN_BASE + ioff, n, d, h, w, cin, ldi)
    a_out = _lib.Act(OUT_BASE + ooff, n, do, ho, wo, cout, ldo)
    a_out2 = _lib.Act(OUT2_BASE + ooff, n, do, ho, wo, cout, ldo)
    a_tout = _lib.Act(TOUT_BASE + ooff, n, 2 * d, 2 * h, 2 * w, cout, ldo)
    return a_in, a_out, a_out2, a_tout


def evaluate(_lib, case):
    """[kernel name, stats rows, in_affine | bn_bwd_sums << 1 | split_act << 2, pair_ok or -1, workspace x 3]
    and, for a stride-2 case, [+ transposed stats rows, transposed-layer workspace x 3]: the transposed layer reads
    the case's input view and writes twice its extent; its weight gradient is the (dy, x, 3, 2) convolution form."""
    lib = _lib.lib
    dt, n, d, h, w, cin, ldi, ioff, cout, ldo, ooff, k, s = case
    a_in, a_out, a_out2, a_tout = views(_lib, case)
    pi, po = C.byref(a_in), C.byref(a_out)
    name = lib.segmi_conv3d_fwd_kernel_name(dt, pi, po, k, s).decode()
    rows = lib.segmi_conv3d_stats_rows(dt, pi, po, k, s)
    flags = (int(lib.segmi_conv3d_in_affine_ok(dt, pi, po, k, s)) | int(lib.segmi_conv3d_bn_bwd_sums_ok(dt, pi, po, k, s)) << 1 |
             int(lib.segmi_conv3d_split_act_ok(dt, pi, po, k, s)) << 2)
    pair = int(lib.segmi_conv3d_pair_ok(dt, pi, po, C.byref(a_out2))) if pair_candidate(cin, cout, k) else -1
    row = [name, rows, flags, pair] + [lib.segmi_conv3d_wgrad_workspace(dt, pi, po, k, s, cus) for cus in CUS]
    if s == 2:
        pt = C.byref(a_tout)
        row.append(lib.segmi_convT3d_stats_rows(dt, pi, pt))
        row += [lib.segmi_conv3d_wgrad_workspace(dt, pt, pi, 3, 2, cus) for cus in CUS]
    return row
