"""What the size queries of the convolution family promise, checked on the device.

The engine allocates ``[rows][2|3][C]`` statistics tables and the weight-gradient slab workspace from
``conv3d_stats_rows`` / ``convT3d_stats_rows`` / ``conv3d_wgrad_workspace``; the kernels write ``grid.x`` rows or slabs
chosen by the launchers.  Each test allocates exactly what the query reports plus a guard filled with a sentinel bit
pattern, launches, and requires the guard bit-intact and the result within the bounds tests/test_ops_gpu.py holds the
same launch to.  One layer per kernel family, at the smallest extent that reaches the family.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from tests.test_ops_gpu import DEV, _fin_bufs, from_ndhwc, q, relerr, rnd, to_ndhwc, wgrad_bound  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload no kernel produces
GUARD_ROWS = 64
GUARD_BYTES = 64 * 1024


def sentinel_table(rows, width, c):
    t = torch.empty((rows + GUARD_ROWS, width, c), dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(SENTINEL)
    return t


def guard_intact(t, rows):
    return bool((t[rows:].view(torch.int32) == SENTINEL).all())


def reserve_rows():
    """rows every statistics table carries behind the workgroups' own (scratch of the finalisation): the k-split
    kernel's 1 x 8 x 8 x 8 layer is 4 workgroups"""
    a = torch.empty((1, 8, 8, 8, 64), dtype=BF16, device=DEV)
    return ops.conv3d_stats_rows(a, a, 3, 1) - 4


def out_view(shape, dtype, slice_bytes):
    """the output tensor, optionally as a channel slice that starts `slice_bytes` into a wider row"""
    if not slice_bytes:
        return torch.empty(shape, dtype=dtype, device=DEV)
    c, skip = shape[-1], slice_bytes // torch.empty((), dtype=dtype).element_size()
    wide = torch.zeros(shape[:-1] + (2 * c,), dtype=dtype, device=DEV)
    return wide[..., skip:skip + c]


# family substring of the kernel name, dtype, input (n, d, h, w), cin, cout, k, s, workgroups, output slice offset
FWD_CASES = [
    ("conv_ring3", BF16, (8, 16, 64, 64), 16, 16, 3, 1, 256, 0),
    ("conv_ring2_kernel<bf16, CK=32, NT=2>", BF16, (8, 16, 64, 64), 32, 32, 3, 1, 256, 0),
    ("conv_ring2_kernel<bf16, CK=32, NT=1>", BF16, (8, 16, 64, 64), 32, 48, 3, 1, 256, 0),
    # the ring3 shape written through a channel slice that starts 8 bytes in (the launch needs 16-byte aligned INPUT
    # rows whatever the kernel, so the view that moves it to ring2 is the output's)
    ("conv_ring2_kernel<bf16, CK=16, NT=1>", BF16, (8, 16, 64, 64), 16, 16, 3, 1, 256, 8),
    ("conv_fwd_ks", BF16, (1, 8, 8, 8), 64, 64, 3, 1, 4, 0),
    ("conv_fwd_ks", F32, (2, 8, 8, 20), 128, 128, 3, 1, 32, 0),
    ("conv_fwd_mfma_kernel<bf16, CK=16, k3 s1>", BF16, (1, 20, 24, 24), 16, 16, 3, 1, None, 0),
    ("conv_fwd_mfma_kernel<bf16, CK=32, k3 s2>", BF16, (1, 16, 16, 16), 32, 64, 3, 2, None, 0),
    ("conv_fwd_mfma_kernel<bf16, CK=16, k1 s1>", BF16, (1, 8, 8, 20), 16, 16, 1, 1, None, 0),
    ("conv_small_fwd", F32, (1, 64, 64, 64), 1, 16, 3, 2, None, 0),
    ("conv_direct", F32, (2, 24, 24, 24), 5, 7, 3, 1, None, 0),
    ("convT persistent", BF16, (1, 8, 8, 16), 32, 16, 3, 2, 16, 0),
    ("convT tile", BF16, (1, 8, 8, 8), 32, 16, 3, 2, 8, 0),
]


@pytest.mark.parametrize("case", FWD_CASES, ids=[f"{c[0].split('<')[0].replace(' ', '_')}-{c[3]}to{c[4]}-k{c[5]}s{c[6]}-{i}" for i, c in enumerate(FWD_CASES)])
def test_statistics_rows_stay_inside_the_table_the_query_sizes(case):
    family, dtype, (n, d, h, w), cin, cout, k, s, wgs, slice_bytes = case
    transposed = family.startswith("convT")
    x = rnd((n, cin, d, h, w), 21)
    xd = to_ndhwc(x, dtype)
    b = rnd((cout,), 23, 0.1)
    if transposed:
        wt = rnd((cin, cout, 3, 3, 3), 22, 1.0 / math.sqrt(cin * 27 / 8))
        ref = F.conv_transpose3d(q(x, dtype), q(wt, dtype), b, stride=2, padding=1, output_padding=1)
    else:
        wt = rnd((cout, cin, k, k, k), 22, 1.0 / math.sqrt(cin * k ** 3))
        ref = F.conv3d(q(x, dtype), q(wt, dtype) if family != "conv_direct" else wt, b, stride=s, padding=(k - 1) // 2)
    osp = tuple(ref.shape[2:])
    wd, bd = wt.to(DEV), b.to(DEV)
    packed = ops.wpack(dtype, 2 if transposed else 0, wd, cin, cout, 3 if transposed else k) if ops.mfma_ok(cin, cout) else None
    y = out_view((n,) + osp + (cout,), dtype, slice_bytes)
    rows = ops.convT3d_stats_rows(xd, y) if transposed else ops.conv3d_stats_rows(xd, y, k, s)
    if not transposed:
        assert family in ops.conv3d_fwd_kernel_name(xd, y, k, s)
    reserve = reserve_rows()
    if wgs is not None:
        assert rows == wgs + reserve
    count = n * osp[0] * osp[1] * osp[2]
    rs = ref.double().sum((0, 2, 3, 4)) / count
    rq = (ref.double() ** 2).sum((0, 2, 3, 4)) / count
    # the tolerances test_conv3d_fwd holds the fused statistics of the same launches to
    tol_mean = (1e-5 if dtype == F32 else 2e-2) * float(ref.abs().max())
    tol_sq = 1e-4 if dtype == F32 else 3e-2

    def launch(stats, fin):
        if transposed:
            ops.convT3d_fwd(xd, y, packed, wd, bd, stats=stats, stats_fin=fin)
        else:
            ops.conv3d_fwd(xd, y, packed, wd, 0, bd, k, s, stats=stats, stats_fin=fin)
        torch.cuda.synchronize()

    # statistics rows alone: the workgroups' rows hold the sums, nothing behind the table is touched
    stats = sentinel_table(rows, 2, cout)
    launch(stats, None)
    assert guard_intact(stats, rows)
    mean = stats[:rows - reserve, 0].double().sum(0).cpu() / count
    sq = stats[:rows - reserve, 1].double().sum(0).cpu() / count
    assert float((mean - rs).abs().max()) < tol_mean
    assert float(((sq - rq).abs() / rq).max()) < tol_sq
    assert relerr(from_ndhwc(y), ref) < (2e-5 if dtype == F32 else 1.5e-2)
    # ... and with the finalisation inside the launch (it uses the reserve rows as scratch)
    stats = sentinel_table(rows, 2, cout)
    gamma, beta = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    rm, rv, (mean_d, invstd_d, scale_d, shift_d) = _fin_bufs(cout)
    eps = 1e-5
    launch(stats, (count, gamma, beta, rm, rv, 0.1, eps, mean_d, invstd_d, scale_d, shift_d))
    assert guard_intact(stats, rows)
    mean, invstd = mean_d.double().cpu(), invstd_d.double().cpu()
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(invstd).all())
    assert float((mean - rs).abs().max()) < tol_mean
    sq = 1.0 / invstd ** 2 - eps + mean ** 2           # invstd = (E[y^2] - mean^2 + eps)^-1/2
    assert float(((sq - rq).abs() / rq).max()) < tol_sq


@pytest.mark.parametrize("c,slice_bytes", [(16, 0), (16, 8), (32, 0)], ids=["ring3-16", "ring2-16", "ring2-32"])
def test_bn_backward_sums_stay_inside_the_table_the_query_sizes(c, slice_bytes, dtype=BF16):
    """MODE 4 of the ring kernels (16 -> 16 on ring3 and ring2, 32 -> 32 as two tiles on grid.y): three rows per
    workgroup into a table sized by conv3d_stats_rows; sums equal to the separate reduce pass within the bound of
    test_bn_bwd_sums_in_the_input_gradient_epilogue_match_the_separate_pass."""
    n, d, h, w = 8, 16, 64, 64
    dyd = to_ndhwc(rnd((n, c, d, h, w), 401, 0.5), dtype)
    xd = to_ndhwc(rnd((n, c, d, h, w), 402, 2.0) + 0.3, dtype)
    pk = ops.wpack(dtype, 1, rnd((c, c, 3, 3, 3), 403, 0.08).to(DEV), c, c, 3)
    mean, invstd = (rnd((c,), 404) * 0.5).to(DEV), (rnd((c,), 405).abs() + 0.5).to(DEV)
    gamma, beta = (rnd((c,), 406) + 1.5).to(DEV), (rnd((c,), 407) * 0.3).to(DEV)
    alpha = torch.full((1,), 0.25, device=DEV)
    count = n * d * h * w
    dx = out_view(tuple(dyd.shape), dtype, slice_bytes)
    assert ops.conv3d_bn_bwd_sums_ok(dyd, dx, 3, 1)
    name = ops.conv3d_fwd_kernel_name(dyd, dx, 3, 1)
    assert ("ring3" in name) == (c == 16 and not slice_bytes) and "ring" in name
    rows = ops.conv3d_stats_rows(dyd, dx, 3, 1)
    assert rows == 256 + reserve_rows()

    def outs():
        return torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.empty(1, device=DEV), torch.empty((2, c), device=DEV)

    part = sentinel_table(rows, 3, c)
    ops.conv3d_fwd(dyd, dx, pk, None, 1, None, 3, 1, bn_bwd=(xd, mean, invstd, gamma, beta, alpha, part))
    torch.cuda.synchronize()
    assert guard_intact(part, rows)
    got = outs()
    ops.bn_act_bwd_finalize(part, rows, c, count, gamma, invstd, *got)
    # finalised inside the launch
    part2, fused = sentinel_table(rows, 3, c), outs()
    ops.conv3d_fwd(dyd, dx, pk, None, 1, None, 3, 1, bn_bwd=(xd, mean, invstd, gamma, beta, alpha, part2),
                   bn_bwd_fin=(count, *fused))
    torch.cuda.synchronize()
    assert guard_intact(part2, rows)
    # the separate pass over the stored gradient
    rows_a = ops.bn_act_bwd_rows(xd)
    part_a, ref = torch.empty((rows_a, 3, c), device=DEV), outs()
    ops.bn_act_bwd_reduce(dx.contiguous(), xd, mean, invstd, gamma, beta, alpha, part_a)
    ops.bn_act_bwd_finalize(part_a, rows_a, c, count, gamma, invstd, *ref)
    torch.cuda.synchronize()
    for a, b, f, what in zip(ref, got, fused, ("dgamma", "dbeta", "dalpha", "coef")):
        a, b, f = a.cpu(), b.cpu(), f.cpu()
        scale = float(a.abs().max()) + 1e-6
        assert float((a - b).abs().max()) < 2e-4 * scale + 1e-3 * float(a.abs().mean()), what
        assert float((a - f).abs().max()) < 2e-4 * scale + 1e-3 * float(a.abs().mean()), what + " (finalised in the launch)"


WGRAD_CASES = [
    # path, dtype, cin, cout, k, s, x (n, d, h, w), x read through a channel slice that starts this many bytes in
    ("wave-specialised", BF16, 32, 32, 3, 1, (2, 32, 32, 64), 0),     # 512 tiles of 2 x 8 x 16: 4 per workgroup of the 128-wide grid
    ("mfma", F32, 32, 32, 3, 1, (2, 16, 16, 16), 0),
    ("small-cin", F32, 1, 16, 3, 2, (1, 64, 64, 64), 0),
    ("direct", BF16, 16, 16, 3, 1, (1, 6, 6, 6), 8),                  # misaligned rows: no MFMA kernel takes them
]


@pytest.mark.parametrize("cus", [0, 128])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_weight_gradient_slabs_stay_inside_the_workspace_the_query_sizes(case, cus):
    path, dtype, cin, cout, k, s, (n, d, h, w), slice_bytes = case
    x = rnd((n, cin, d, h, w), 31)
    osp = tuple((e + 2 * ((k - 1) // 2) - k) // s + 1 for e in (d, h, w))
    dy = rnd((n, cout) + osp, 32)
    xd, dyd = to_ndhwc(x, dtype), to_ndhwc(dy, dtype)
    if slice_bytes:
        skip = slice_bytes // xd.element_size()
        wide = torch.zeros(xd.shape[:4] + (2 * cin,), dtype=dtype, device=DEV)
        wide[..., skip:skip + cin] = xd
        xd = wide[..., skip:skip + cin]
    nbytes = ops.conv3d_wgrad_workspace(xd, dyd, k, s, cus)
    # the four paths answer the query differently: slabs = workgroups (wave-specialised: sized by `cus`), tiles, ...
    if path == "wave-specialised":
        assert nbytes != ops.conv3d_wgrad_workspace(xd, dyd, k, s, 64)
    ws = torch.empty(nbytes + GUARD_BYTES, dtype=torch.uint8, device=DEV)
    ws[nbytes:].view(torch.int32).fill_(SENTINEL)
    dw = torch.empty((cout, cin, k, k, k), device=DEV)
    db = torch.empty((cout,), device=DEV)
    ops.conv3d_wgrad(xd, dyd, dw, db, k, s, ws, cus=cus)
    torch.cuda.synchronize()
    assert bool((ws[nbytes:].view(torch.int32) == SENTINEL).all())
    wgrad_bound(dtype, x, dy, k, s, dw, db)
