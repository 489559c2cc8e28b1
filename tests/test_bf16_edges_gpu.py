"""bf16 stores bit for bit, kernel family by kernel family: round to nearest even at every convolution store and in
the residual epilogue, the format-only kernels against torch's conversion (NaN, Inf, the overflow tie, signed zero)
and the weight packs.

The convolution tests use a one-hot weight (centre tap 1.0 from input channel ``co % Cin``): every other product is
an exact zero, so the f32 sum is exact in any order and the stored bf16 value is decided by the store's rounding
alone.  Inputs and bias are chosen so that ``x + b`` is exact in f32 and lies on a bf16 tie or one f32 ulp to either
side of one; a store that truncates, or rounds half away from zero, differs in the last bit.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from tests.helpers import unet_sweep as us  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16


def to_ndhwc(x_ncdhw, dtype=BF16):
    return x_ncdhw.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)


def from_ndhwc_bits(t):
    """NCDHW int16 view of a bf16 NDHWC device tensor"""
    return t.cpu().permute(0, 4, 1, 2, 3).contiguous().view(torch.int16)


def bits(t32):
    """torch's f32 -> bf16 conversion (round to nearest even) as int16"""
    return t32.bfloat16().contiguous().view(torch.int16)


def is_tie(t32):
    return (t32.contiguous().view(torch.int32) & 0xFFFF) == 0x8000


def exponent_of(ch):
    """binade of input channel ``ch``: 2^-2 .. 2^2"""
    return (ch % 5) - 2


def tie_operands(cin, cout, sp, n, seed):
    """bf16 x = ±2^e (1 + j 2^-7), e per input channel; f32 bias b = ±2^e (2^-8 + d), d in {0, ±2^-23} per output
    channel, e that of the channel the one-hot weight reads: x + b is exact in f32 and is a bf16 tie (d = 0) or one
    f32 ulp above / below one"""
    g = torch.Generator().manual_seed(seed)
    shape = (n, cin) + sp
    j = torch.randint(0, 128, shape, generator=g).float()
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    e = torch.tensor([exponent_of(c) for c in range(cin)]).float().view(1, -1, 1, 1, 1)
    x = sign * torch.exp2(e) * (1 + j / 128)
    assert torch.equal(x.bfloat16().float(), x)
    co = torch.arange(cout)
    d = torch.tensor([0.0, 2.0 ** -23, -2.0 ** -23])[(co + co // cin) % 3]
    bsign = torch.where((co // 3) % 2 == 0, 1.0, -1.0)
    b = bsign * torch.exp2(torch.tensor([exponent_of(int(c) % cin) for c in co]).float()) * (2.0 ** -8 + d)
    w = torch.zeros((cout, cin, 3, 3, 3))
    w[co, co % cin, 1, 1, 1] = 1.0
    return x, w, b


def one_hot_expected(x, cout, stride, b=None, r=None):
    """f32 value of the one-hot convolution (+ bias, + residual): exact, checked against float64"""
    cin = x.shape[1]
    v = x[:, torch.arange(cout) % cin][:, :, ::stride, ::stride, ::stride]
    want, want64 = v.float(), v.double()
    if b is not None:
        want, want64 = want + b.view(1, -1, 1, 1, 1), want64 + b.double().view(1, -1, 1, 1, 1)
    if r is not None:
        want, want64 = want + r.float(), want64 + r.double()
    assert torch.equal(want.double(), want64)                  # the f32 sum is exact: only the store rounds
    return want


def assert_bits(got_bits, want32, what):
    want = bits(want32)
    bad = got_bits != want
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} stored values differ from round-to-nearest-even "
                             f"({int((bad & is_tie(want32)).sum())} of them on exact ties), e.g. f32 "
                             f"{float(want32.flatten()[i])!r} stored as 0x{int(got_bits.flatten()[i]) & 0xFFFF:04x}, "
                             f"expected 0x{int(want.flatten()[i]) & 0xFFFF:04x}")


def run_conv(cin, cout, stride, sp, n, x, w, b, residual=None):
    xd = to_ndhwc(x)
    osp = tuple((d - 1) // stride + 1 for d in sp)
    yd = torch.full((n,) + osp + (cout,), float("nan"), dtype=BF16, device=DEV)
    name = ops.conv3d_fwd_kernel_name(xd, yd, 3, stride)
    assert "bf16" in name, name
    wd = w.to(DEV)
    packed = ops.wpack(BF16, 0, wd, cin, cout, 3) if ops.mfma_ok(cin, cout) else None
    ops.conv3d_fwd(xd, yd, packed, wd, 0, None if b is None else b.to(DEV), 3, stride,
                   residual=None if residual is None else to_ndhwc(residual))
    torch.cuda.synchronize()
    return from_ndhwc_bits(yd), name


# cin, cout, stride, spatial, batch: the smallest case of tests/test_ops_gpu.py's CONV_CASES that reaches each family
STORE_CASES = [
    (16, 3, 1, (6, 7, 9), 1),            # direct
    (1, 16, 2, (12, 12, 12), 2),         # small-Cin
    (2, 32, 1, (5, 9, 19), 2),           # small-Cin, stride 1
    (16, 16, 1, (8, 12, 20), 2),         # tile kernel CK=16 s1
    (16, 32, 2, (10, 12, 36), 1),        # tile kernel CK=16 s2
    (32, 64, 2, (8, 8, 16), 1),          # tile kernel CK=32 s2
    (128, 48, 1, (5, 6, 7), 2),          # k-split, narrow tiles
    (64, 64, 1, (9, 10, 40), 2),         # k-split, wide tiles
    (16, 16, 1, (33, 60, 120), 2),       # ring3
    (32, 32, 1, (33, 60, 120), 2),       # ring2 NT=2
    (32, 16, 1, (33, 60, 120), 2),       # ring2 NT=1 (one output tile)
]
_ids = lambda c: f"{c[0]}to{c[1]}s{c[2]}-{'x'.join(map(str, c[3]))}"


def _family(case):
    cin, cout, s, sp, n = case
    xd = torch.empty((n,) + sp + (cin,), dtype=BF16, device=DEV)
    yd = torch.empty((n,) + tuple((d - 1) // s + 1 for d in sp) + (cout,), dtype=BF16, device=DEV)
    return us.family_of(ops.conv3d_fwd_kernel_name(xd, yd, 3, s))


def test_store_cases_reach_every_reachable_forward_family():
    reached = {_family(c) for c in STORE_CASES}
    missing = [f for f in us.FAMILIES if f not in us.UNREACHABLE and f not in reached]
    assert not missing, (missing, sorted(reached))


@pytest.mark.parametrize("case", STORE_CASES, ids=_ids)
def test_conv_store_rounds_to_nearest_even(case, record_property):
    cin, cout, s, sp, n = case
    x, w, b = tie_operands(cin, cout, sp, n, 1)
    want = one_hot_expected(x, cout, s, b)
    ties = float(is_tie(want).float().mean())
    assert ties > 0.1 and float((~is_tie(want)).float().mean()) > 0.1        # ties and their f32 neighbours
    got, name = run_conv(cin, cout, s, sp, n, x, w, b)
    record_property("kernel", name)
    record_property("share of exact ties", round(ties, 3))
    assert_bits(got, want, name)


RESIDUAL_CASES = [
    (16, 16, 1, (8, 12, 20), 2),         # tile kernel
    (16, 32, 2, (10, 12, 36), 1),        # tile kernel, stride 2
    (128, 48, 1, (5, 6, 7), 2),          # k-split
    (16, 16, 1, (33, 60, 120), 2),       # ring3
    (32, 32, 1, (33, 60, 120), 2),       # ring2
]


@pytest.mark.parametrize("case", RESIDUAL_CASES, ids=_ids)
def test_residual_epilogue_rounds_the_exact_sum_once(case, record_property):
    """conv (one-hot, no bias, no PReLU) + a bf16 residual whose exponent lies within ±4 of x's: the f32 sum of two
    8-bit significands at most 4 binades apart is exact, and it ties wherever the bits below the result's 8th cancel
    to a half"""
    cin, cout, s, sp, n = case
    x, w, _ = tie_operands(cin, cout, sp, n, 2)
    osp = tuple((d - 1) // s + 1 for d in sp)
    g = torch.Generator().manual_seed(3)
    shape = (n, cout) + osp
    xe = torch.tensor([exponent_of(c % cin) for c in range(cout)]).float().view(1, -1, 1, 1, 1)
    re = xe + torch.randint(-4, 5, shape, generator=g).float()
    r = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0) * torch.exp2(re) * \
        (1 + torch.randint(0, 128, shape, generator=g).float() / 128)
    assert torch.equal(r.bfloat16().float(), r)
    want = one_hot_expected(x, cout, s, None, r)
    ties = float(is_tie(want).float().mean())
    assert ties > 0.02
    got, name = run_conv(cin, cout, s, sp, n, x, w, None, residual=r)
    record_property("kernel", name)
    record_property("share of exact ties", round(ties, 3))
    assert_bits(got, want, name + " + residual")


def test_convT_store_rounds_to_nearest_even(record_property):
    """ConvTranspose3d 32 -> 16: the centre tap lands on the even output voxels (y[2p] = x[p] + b), the others hold
    the bias alone"""
    cin, cout, sp, n = 32, 16, (6, 6, 20), 2
    x, wc, b = tie_operands(cin, cout, sp, n, 4)
    w = wc.permute(1, 0, 2, 3, 4).contiguous()                 # [cin][cout][taps]
    want64 = F.conv_transpose3d(x.double(), w.double(), b.double(), stride=2, padding=1, output_padding=1)
    want = want64.float()
    assert torch.equal(want.double(), want64)
    assert torch.equal(want[:, :, ::2, ::2, ::2], one_hot_expected(x, cout, 1, b))
    assert float(is_tie(want).float().mean()) > 0.02
    xd = to_ndhwc(x)
    yd = torch.full((n,) + tuple(want.shape[2:]) + (cout,), float("nan"), dtype=BF16, device=DEV)
    wd = w.to(DEV)
    ops.convT3d_fwd(xd, yd, ops.wpack(BF16, 2, wd, cin, cout, 3), wd, b.to(DEV))
    torch.cuda.synchronize()
    assert_bits(from_ndhwc_bits(yd), want, "convT 32->16")


def test_dectop_store_rounds_to_nearest_even():
    """the fused decoder top: one-hot up-convolution (scale 1, no bias, slope 1) gives h = x on the even voxels and 0
    elsewhere; the one-hot conv + bias + identity residual then stores 2 h + cb, exact in f32 in either order"""
    n, d, h, w = 1, 8, 16, 16
    x, wc, b = tie_operands(32, 16, (d, h, w), n, 5)
    wt = wc.permute(1, 0, 2, 3, 4).contiguous()                # [32][16][taps], ci = co
    w2 = torch.zeros((16, 16, 3, 3, 3))
    w2[torch.arange(16), torch.arange(16), 1, 1, 1] = 1.0
    cb = 2 * b                                                 # ±2^(e+1) (2^-8 + d): a tie of 2 h + cb
    h64 = F.conv_transpose3d(x.double(), wt.double(), None, stride=2, padding=1, output_padding=1)
    want64 = F.conv3d(h64, w2.double(), cb.double(), padding=1) + h64
    want = want64.float()
    assert torch.equal(want.double(), want64)
    assert torch.equal((h64.float() + cb.view(1, -1, 1, 1, 1)).double(), h64 + cb.double().view(1, -1, 1, 1, 1))
    assert float(is_tie(want).float().mean()) > 0.02
    xd = to_ndhwc(x)
    out = torch.full((n, 2 * d, 2 * h, 2 * w, 16), float("nan"), dtype=BF16, device=DEV)
    assert ops.dectop_ok(xd, out)
    ops.dectop_fwd(xd, out, ops.dectop_up_frag(wt.to(DEV), torch.ones(16, device=DEV), dtype=BF16),
                   torch.zeros(16, device=DEV), torch.ones(1, device=DEV), ops.wpack(BF16, 0, w2.to(DEV), 16, 16, 3),
                   cb.to(DEV), alpha_in_unit_range=True)
    torch.cuda.synchronize()
    assert_bits(from_ndhwc_bits(out), want, "dectop")


# ---------------------------------------------------------------------------------------------- weight packs
def _tie_weights(shape, seed):
    """f32 weights ±2^e (1 + j 2^-7 + 2^-8 + d), d in {0, ±2^-23}: bf16 ties and their f32 neighbours"""
    g = torch.Generator().manual_seed(seed)
    j = torch.randint(0, 128, shape, generator=g).float()
    d = torch.tensor([0.0, 2.0 ** -23, -2.0 ** -23])[torch.randint(0, 3, shape, generator=g)]
    e = torch.randint(-6, 2, shape, generator=g).float()
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    w = sign * torch.exp2(e) * (1 + j / 128 + 2.0 ** -8 + d)
    assert float(is_tie(w).float().mean()) > 0.2
    return w


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_wpack_rounds_f32_weights_to_nearest_even(kind):
    """ops.wpack(bfloat16, ...) read back through a convolution of unit impulses (sample i: 1.0 in channel i at the
    centre voxel): each output voxel holds exactly one packed weight, already bf16, so the store does not round again.
    kind 0: forward, 1: stride-1 input gradient (flipped, transposed), 2: transposed convolution"""
    c = 16
    w = _tie_weights((c, c, 3, 3, 3), 6 + kind)
    wd = w.to(DEV)
    packed = ops.wpack(BF16, kind, wd, c, c, 3)
    isp = (3, 5, 17) if kind == 2 else (6, 8, 20)            # shapes tests/test_ops_gpu.py runs these kernels at
    x = torch.zeros((c, c) + isp)
    x[torch.arange(c), torch.arange(c), 1, 1, 1] = 1.0
    xd = to_ndhwc(x)
    if kind == 2:
        yd = torch.full((c, 6, 10, 34, c), float("nan"), dtype=BF16, device=DEV)
        ops.convT3d_fwd(xd, yd, packed, wd, None)
        torch.cuda.synchronize()
        full = from_ndhwc_bits(yd)
        got, rest = full[:, :, 1:4, 1:4, 1:4], full.clone()    # y[i, co, 1 + t] = w[i, co, t]
        rest[:, :, 1:4, 1:4, 1:4] = 0
        want = w
    else:
        yd = torch.full((c,) + isp + (c,), float("nan"), dtype=BF16, device=DEV)
        ops.conv3d_fwd(xd, yd, packed, wd, kind, None, 3, 1)
        torch.cuda.synchronize()
        full = from_ndhwc_bits(yd)
        got, rest = full[:, :, :3, :3, :3], full.clone()
        rest[:, :, :3, :3, :3] = 0
        # kind 0: y[i, co, p] = w[co, i, 2 - p];  kind 1: dx[i, ci, p] = w[i, ci, p]
        want = w.permute(1, 0, 2, 3, 4).flip(2, 3, 4) if kind == 0 else w
    assert_bits(got.contiguous(), want.contiguous(), f"wpack kind {kind}")
    assert bool(((rest & 0x7FFF) == 0).all())                  # every voxel the impulse does not reach is ±0


# ---------------------------------------------------------------------------------------------- format-only kernels
SPECIALS = [  # f32 bits -> bf16 bits (None: any NaN)
    (0x7F800001, None),      # NaN whose payload lies in the low mantissa only: truncation would make it Inf
    (0xFFC00001, None),
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),                # ±Inf
    (0x7F7F8000, 0x7F80), (0xFF7F8000, 0xFF80),                # the tie above the largest finite bf16 -> Inf
    (0x7F7FFFFF, 0x7F80),                                      # FLT_MAX -> Inf
    (0x7F7F7FFF, 0x7F7F), (0xFF7F7FFF, 0xFF7F),                # just below the tie -> the largest finite bf16
    (0x00000000, 0x0000), (0x80000000, 0x8000),                # ±0
    (0x3F808000, 0x3F80), (0x3F818000, 0x3F82),                # ties to even, both directions
    (0x3F808001, 0x3F81), (0x3F817FFF, 0x3F81),
]


def _plant(t, start):
    """the special values into consecutive elements of ``t`` (flat, from ``start``); returns their flat indices"""
    vals = torch.tensor([s if s < 2 ** 31 else s - 2 ** 32 for s, _ in SPECIALS], dtype=torch.int32).view(torch.float32)
    idx = torch.arange(start, start + len(SPECIALS))
    t.view(-1)[idx] = vals
    return idx


def assert_same_bf16(got, want32, what):
    """got (bf16, cpu) equals torch's conversion of want32 bit for bit; NaN only has to stay NaN"""
    want = want32.bfloat16()
    nan = torch.isnan(want32)
    assert torch.equal(torch.isnan(got.float()), nan), f"{what}: NaN not kept"
    gb, wb = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    assert torch.equal(gb[~nan], wb[~nan]), f"{what}: {int((gb != wb)[~nan].sum())} values differ from torch's bf16"


def test_torchs_conversion_is_the_table():
    for s, want in SPECIALS:
        v = torch.tensor([s if s < 2 ** 31 else s - 2 ** 32], dtype=torch.int32).view(torch.float32)
        if want is None:
            assert bool(torch.isnan(v.bfloat16().float()))
        else:
            assert int(v.bfloat16().view(torch.int16)) & 0xFFFF == want, hex(s)


def test_format_kernels_are_bit_exact_in_bf16():
    """crop_patches, warp_crop_patches, nchw_to_ndhwc, sw_gather and ndhwc_to_nchw move or convert data only: the
    bf16 output equals the f32 kernel's output converted by torch, bit for bit (ndhwc_to_nchw: torch's bf16 -> f32),
    with NaN, ±Inf, the overflow tie, the largest finite value and ±0 among the sources"""
    from segmantic_amd.seg.augment import _rot, to_index_map_xyz
    g = torch.Generator().manual_seed(171)
    D, H, W = 20, 24, 28
    img = torch.randn((1, D, H, W, 1), generator=g) * torch.exp2(torch.randint(-20, 10, (1, D, H, W, 1), generator=g))
    planted = _plant(img, (8 * H + 10) * W + 9)                 # row (z 8, y 10), x 9 ..: inside both crops' source
    lab = torch.randint(0, 4, (D, H, W), generator=g).float()
    imd, lad = img.to(DEV), lab.to(DEV)
    roi = (8, 12, 16)
    starts, flips = [[0, 3, 5, 7], [0, -2, 15, 20]], [0, 5]
    o32 = torch.empty((2,) + roi + (1,), device=DEV)
    o16 = torch.empty((2,) + roi + (1,), dtype=BF16, device=DEV)
    l32, l16 = torch.empty((2,) + roi, device=DEV), torch.empty((2,) + roi, device=DEV)
    ops.crop_patches(imd, lad, starts, flips, o32, l32)
    ops.crop_patches(imd, lad, starts, flips, o16, l16)
    torch.cuda.synchronize()
    assert int(torch.isnan(o32).sum()) >= 2 and int(torch.isinf(o32).sum()) >= 2      # the crop holds the specials
    assert_same_bf16(o16.cpu(), o32.cpu(), "crop_patches")
    assert torch.equal(l16, l32)
    ctr = (np.array([D, H, W]) - 1) / 2.0
    to_c, from_c = np.eye(4), np.eye(4)
    to_c[:3, 3], from_c[:3, 3] = -ctr, ctr
    m = from_c @ _rot(0, -0.3) @ np.diag([1 / 1.2, 1 / 1.2, 1 / 1.2, 1.0]) @ to_c
    ops.warp_crop_patches(imd, lad, starts, flips, to_index_map_xyz(m), o32, l32)
    ops.warp_crop_patches(imd, lad, starts, flips, to_index_map_xyz(m), o16, l16)
    torch.cuda.synchronize()
    assert_same_bf16(o16.cpu(), o32.cpu(), "warp_crop_patches")
    assert torch.equal(l16, l32)
    src = img.permute(0, 4, 1, 2, 3).contiguous()
    s32 = torch.empty((1, D, H, W, 1), device=DEV)
    s16 = torch.empty((1, D, H, W, 1), dtype=BF16, device=DEV)
    ops.nchw_to_ndhwc(src.to(DEV), s32)
    ops.nchw_to_ndhwc(src.to(DEV), s16)
    torch.cuda.synchronize()
    assert torch.equal(s32.cpu().view(torch.int32), img.view(torch.int32))            # f32: a copy, payloads included
    assert_same_bf16(s16.cpu(), img, "nchw_to_ndhwc")
    stored = s16.cpu().view(torch.int16).view(-1)[planted]
    for (s, want), got in zip(SPECIALS, stored.tolist()):
        got &= 0xFFFF
        if want is None:
            assert (got & 0x7F80) == 0x7F80 and (got & 0x007F) != 0, f"f32 0x{s:08x} stored as 0x{got:04x}: not a NaN"
        else:
            assert got == want, f"f32 0x{s:08x} stored as 0x{got:04x}, expected 0x{want:04x}"
    back = torch.empty((1, 1, D, H, W), device=DEV)
    ops.ndhwc_to_nchw(s16, back)
    torch.cuda.synchronize()
    wantb = src.bfloat16().float()
    assert torch.equal(torch.isnan(back.cpu()), torch.isnan(wantb))
    assert torch.equal(back.cpu().view(torch.int32)[~torch.isnan(wantb)], wantb.view(torch.int32)[~torch.isnan(wantb)])
    wins = [(0, 0, 0), (4, 8, 8), (12, 16, 20)]                # the second window holds the planted values
    w16 = torch.empty((3, 8, 8, 8, 1), dtype=BF16, device=DEV)
    ops.sw_gather(s16, 0, wins, w16)
    torch.cuda.synchronize()
    for i, (z, y, x) in enumerate(wins):
        # a copy of bf16 elements: the very bits, NaN payloads included
        assert torch.equal(w16[i, ..., 0].cpu().view(torch.int16), s16[0, z:z + 8, y:y + 8, x:x + 8, 0].cpu().view(torch.int16))
        assert_same_bf16(w16[i, ..., 0].cpu(), img[0, z:z + 8, y:y + 8, x:x + 8, 0], "sw_gather")
