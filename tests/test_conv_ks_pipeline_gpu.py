"""conv_fwd_ks_kernel (csrc/conv_ks_impl.h) at the smallest shapes on which each of its paths can go wrong: the
single-chunk form and the chunk loop (1, 2, 3 and 8 channel chunks; an odd count too, so that a loop that alternates
LDS slots would end on either), one and two output tiles per workgroup, both tile shapes with ragged, part-empty, single and interior
tiles, every epilogue, strided operands, the three storage types, and the k-steps only wave 3 clamps.

Every case goes through ``ops.conv3d_fwd`` and asserts from ``ops.conv3d_fwd_kernel_name`` that the k-split kernel
took the layer.  Expected values are a float64 convolution of the rounded operands on the CPU; every output element
is held to the bound of tests/helpers/lowp_bounds.py for its storage type, through the helpers of tests/test_ops_gpu.py.

Statistics rows are f32 accumulator outputs taken BEFORE the store rounds: row t holds, per channel, the sum and the
sum of squares of conv + bias over the voxels of workgroup tile t.  They are compared row by row with the float64
sums of the float64 reference over the same voxels, at the accumulator bound (``rounded=False``: 2^-18 A) with
A_row = sum of the voxels' A for the sums.  For the squares, v = ref + e with |e| <= 2^-18 A and |ref| <= A gives
|v^2 - ref^2| <= 2 A |e| + e^2, so the companion is 2 * sum A^2 (+ the same chain of adds).  For f32 storage the
stored output IS the pre-rounding value, so there the rows are also compared with the float64 sums of the kernel's
own output.  (Sums of a 16-bit kernel's stored output differ from its rows by the store roundings themselves, up to
2^-9 per voxel, which no accumulation bound covers.)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from tests.helpers import lowp_bounds as lb  # noqa: E402
from tests.test_ops_gpu import DEV, F16, elem_bound, epilogue64, from_ndhwc, q, rnd, to_ndhwc  # noqa: E402
from tests.test_ops_gpu import _ratio_report  # noqa: E402,F401  (autouse: elem_bound reports its worst ratio)

BF16, F32 = torch.bfloat16, torch.float32
TYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="f16"), pytest.param(F32, id="f32")]
WIDE, NARROW = (2, 4, 16), (4, 4, 8)          # conv_ks_tile_shape(wide), wide = output row longer than 8
RAGGED_WIDE = (3, 6, 18)                      # 2 x 2 x 2 wide tiles, ragged on every axis, part-empty tiles
RAGGED_NARROW = (5, 5, 8)                     # 2 x 2 x 1 narrow tiles
FILL_WGS = 512                                # conv_plan.h kFillWgs


def ck_of(dtype):
    """channels per chunk: 32 in the 16-bit types, 16 in f32"""
    return 16 if dtype == F32 else 32


def plan(sp, n, cout):
    """(tile, tiles along z / y / x, workgroups on grid.x, output tiles per workgroup) as conv_plan() decides them"""
    t = WIDE if sp[2] > 8 else NARROW
    tz, ty, tx = (-(-e // s) for e, s in zip(sp, t))
    wgs, ntiles = n * tz * ty * tx, cout // 16
    nt = 2 if ntiles % 2 == 0 and wgs * (ntiles // 2) >= FILL_WGS else 1
    return t, (tz, ty, tx), wgs, nt


_REFS = {}


def operands(dtype, cin, cout, sp, n, only_tap=None):
    """rounded operands and their float64 reference, computed once per shape and left unchanged"""
    key = (dtype, cin, cout, sp, n, only_tap)
    if key not in _REFS:
        x = q(rnd((n, cin) + sp, 701), dtype)
        w = rnd((cout, cin, 3, 3, 3), 702, 1.0 / math.sqrt(cin * 27))
        if only_tap is not None:
            keep = torch.zeros(27)
            keep[only_tap] = 1.0
            w = w * keep.view(1, 1, 3, 3, 3) * math.sqrt(27)
        w = q(w, dtype)
        b = rnd((cout,), 703, 0.1)
        r = q(rnd((n, cout) + sp, 704), dtype)
        ref, absref = lb.conv_ref(x, w, None)
        b5 = b.double().view(1, -1, 1, 1, 1)
        _REFS[key] = (x, w, b, r, (ref, absref), (ref + b5, absref + b5.abs()))
    return _REFS[key]


def row_sums(v, sp, n, tile, tiles):
    """[rows][c] sums of an NCDHW float64 tensor over each workgroup tile, rows in blockIdx.x order"""
    tz, ty, tx = tiles
    pad = [tz * tile[0] - sp[0], ty * tile[1] - sp[1], tx * tile[2] - sp[2]]
    v = torch.nn.functional.pad(v, (0, pad[2], 0, pad[1], 0, pad[0]))
    c = v.shape[1]
    v = v.view(n, c, tz, tile[0], ty, tile[1], tx, tile[2]).sum((3, 5, 7))          # n c tz ty tx
    return v.permute(0, 2, 3, 4, 1).reshape(n * tz * ty * tx, c)


def run_ks(dtype, cin, cout, sp, n, want_nt, bias=False, alpha=None, residual=False, stats=False, in_view=False,
           only_tap=None):
    x, w, b, r, ref_nobias, ref_bias = operands(dtype, cin, cout, sp, n, only_tap)
    tile, tiles, wgs, nt = plan(sp, n, cout)
    assert nt == want_nt, (nt, want_nt)
    if in_view:          # the input is a channel slice of a wider buffer (row stride > channels)
        big = torch.full((n,) + sp + (cin + 48,), float("nan"), dtype=dtype, device=DEV)
        big[..., 16:16 + cin] = to_ndhwc(x, dtype)
        xd = big[..., 16:16 + cin]
    else:
        xd = to_ndhwc(x, dtype)
    yd = torch.full((n,) + sp + (cout,), float("nan"), dtype=dtype, device=DEV)
    name = ops.conv3d_fwd_kernel_name(xd, yd, 3, 1)
    assert "conv_fwd_ks_kernel" in name, name
    packed = ops.wpack(dtype, 0, w.to(DEV), cin, cout, 3)
    bd = b.to(DEV) if bias else None
    ad = torch.tensor([alpha], device=DEV) if alpha is not None else None
    rd = None
    if residual:         # read through a channel-slice view: ld = cout + 16 > c
        rbig = torch.full((n,) + sp + (cout + 16,), float("nan"), dtype=dtype, device=DEV)
        rbig[..., 16:] = to_ndhwc(r, dtype)
        rd = rbig[..., 16:]
    ref, absref = ref_bias if bias else ref_nobias
    want = epilogue64(ref, absref, alpha, r if residual else None)

    def check_out(y):
        got = from_ndhwc(y)
        assert bool(torch.isfinite(got).all())                      # every voxel written (the output started as NaN)
        elem_bound(dtype, got, *want)
        return got

    if not stats:
        ops.conv3d_fwd(xd, yd, packed, None, 0, bd, 3, 1, prelu_alpha=ad, residual=rd)
        torch.cuda.synchronize()
        check_out(yd)
        return
    # ---- statistics rows, then the same launch finalising them
    rows = ops.conv3d_stats_rows(xd, yd, 3, 1)
    assert rows >= wgs
    st = torch.zeros((rows, 2, cout), device=DEV)
    ops.conv3d_fwd(xd, yd, packed, None, 0, bd, 3, 1, prelu_alpha=ad, residual=rd, stats=st)
    torch.cuda.synchronize()
    got = check_out(yd)
    rows_got = st[:wgs].cpu()
    elem_bound(dtype, rows_got[:, 0], row_sums(ref, sp, n, tile, tiles), row_sums(absref, sp, n, tile, tiles),
               what="sum rows", rounded=False)
    elem_bound(dtype, rows_got[:, 1], row_sums(ref * ref, sp, n, tile, tiles),
               2 * row_sums(absref * absref, sp, n, tile, tiles), what="square rows", rounded=False)
    if dtype == F32 and alpha is None and not residual:
        own = got.double()
        elem_bound(dtype, rows_got[:, 0], row_sums(own, sp, n, tile, tiles), row_sums(absref, sp, n, tile, tiles),
                   what="sum rows (own output)", rounded=False)
        elem_bound(dtype, rows_got[:, 1], row_sums(own * own, sp, n, tile, tiles),
                   2 * row_sums(absref * absref, sp, n, tile, tiles), what="square rows (own output)", rounded=False)
    count = n * sp[0] * sp[1] * sp[2]
    gamma, beta = (1 + 0.2 * rnd((cout,), 705)).to(DEV), (0.1 * rnd((cout,), 706)).to(DEV)

    def fin_bufs():
        rm, rv = (rnd((cout,), 707) * 0.2).to(DEV), (rnd((cout,), 708).abs() + 0.5).to(DEV)
        return rm, rv, [torch.full((cout,), float("nan"), device=DEV) for _ in range(4)]

    rm0, rv0, outs0 = fin_bufs()
    ops.bn_finalize(st, rows, cout, count, gamma, beta, rm0, rv0, 0.1, 1e-5, *outs0)
    y1 = torch.full_like(yd, float("nan"))
    st1 = torch.zeros((rows, 2, cout), device=DEV)
    rm1, rv1, outs1 = fin_bufs()
    ops.conv3d_fwd(xd, y1, packed, None, 0, bd, 3, 1, prelu_alpha=ad, residual=rd, stats=st1,
                   stats_fin=(count, gamma, beta, rm1, rv1, 0.1, 1e-5, *outs1))
    torch.cuda.synchronize()
    assert torch.equal(y1, yd)
    # the bound of test_bn_statistics_finalised_by_the_producing_launch: f64 sums of the same f32 rows in another order
    for a, g_, what in zip(outs0 + [rm0, rv0], outs1 + [rm1, rv1],
                           ("mean", "invstd", "scale", "shift", "running_mean", "running_var")):
        assert bool(torch.isfinite(g_).all()), what
        assert float((a - g_).abs().max()) <= 1e-6 * float(a.abs().max()) + 1e-9, what


# ------------------------------------------------------------------ chunk counts x output tiles per workgroup x types
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("chunks,cout", [(1, 32), (2, 64), (3, 32), (8, 32)])
def test_chunk_counts_and_output_tiles_per_workgroup(chunks, cout, nt, dtype):
    """1 chunk: the form without a chunk loop.  2, 3, 8 chunks: the chunk loop, even and odd counts.  A batch of 2
    leaves the launch short of kFillWgs workgroups (NT = 1); the batch that reaches it gives NT = 2."""
    n = 2 if nt == 1 else FILL_WGS // 8 // (cout // 32)
    run_ks(dtype, chunks * ck_of(dtype), cout, RAGGED_WIDE, n, nt, bias=True)


# ------------------------------------------------------------------ tiles
@pytest.mark.parametrize("chunks", [1, 2, 3])
@pytest.mark.parametrize("sp,n", [(RAGGED_WIDE, 2), (RAGGED_NARROW, 2), (WIDE, 1), (NARROW, 1), ((6, 12, 48), 1),
                                  ((12, 12, 8), 1)])
def test_tile_shapes(sp, n, chunks, dtype=BF16):
    """ragged wide and narrow tiles; a volume of exactly one tile (every halo voxel is zero fill); 3 x 3 x 3 wide
    tiles (the middle tile's halo is all neighbours' data) and 3 x 3 x 1 narrow ones"""
    run_ks(dtype, chunks * 32, 32, sp, n, 1)


# ------------------------------------------------------------------ epilogues
EPILOGUES = {
    "plain": dict(),
    "bias": dict(bias=True),
    "prelu": dict(bias=True, alpha=0.2),
    "residual": dict(bias=True, alpha=0.2, residual=True),
    "stats": dict(bias=True, stats=True),
    "stats_prelu_residual": dict(bias=True, alpha=1.5, residual=True, stats=True),
}


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("mode", list(EPILOGUES))
def test_epilogues(mode, chunks, dtype):
    run_ks(dtype, chunks * ck_of(dtype), 32, RAGGED_WIDE, 2, 1, **EPILOGUES[mode])


@pytest.mark.parametrize("chunks,cout", [(1, 32), (2, 64)])
def test_epilogue_with_two_output_tiles_per_workgroup(chunks, cout, dtype=BF16):
    run_ks(dtype, chunks * 32, cout, RAGGED_WIDE, FILL_WGS // 8 // (cout // 32), 2, bias=True, alpha=0.2,
           residual=True, stats=True)


@pytest.mark.parametrize("sp", [RAGGED_NARROW, (12, 12, 8)])
def test_statistics_rows_of_narrow_tiles(sp, dtype=BF16):
    run_ks(dtype, 64, 32, sp, 2, 1, bias=True, stats=True)


# ------------------------------------------------------------------ strided input
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("chunks", [1, 3])
def test_input_is_a_channel_slice_of_a_wider_buffer(chunks, dtype):
    run_ks(dtype, chunks * ck_of(dtype), 32, RAGGED_WIDE, 2, 1, bias=True, in_view=True)


# ------------------------------------------------------------------ wave 3 owns 6 taps, the others 7
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("tap", [24, 26])
def test_last_k_steps(tap, chunks, dtype=BF16):
    """all weights zero except one tap.  Tap 26 is wave 2's last k-step and tap 24 wave 0's; wave 3's seventh step is
    clamped to tap 26 and must not run: run twice, or read from the wrong LDS row, it changes these outputs."""
    run_ks(dtype, chunks * 32, 32, RAGGED_WIDE, 2, 1, only_tap=tap)
    run_ks(dtype, chunks * 32, 32, (12, 12, 8), 1, 1, only_tap=tap)
