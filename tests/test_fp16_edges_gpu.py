"""fp16 at its edges, op by op: subnormal operands, overflow to Inf in every store path, Inf / NaN reaching the f32
gradients, the arena-wide finite check, and the format-only kernels bit for bit.

Every numeric check uses the elementwise bound of tests/helpers/lowp_bounds.py against a float64 reference on the
same fp16 operands (tests/test_fp16_host.py proves on CPU that the bound rejects flushed subnormal operands and a
store saturated to 65504).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from tests.helpers import lowp_bounds as lb  # noqa: E402

DEV = "cuda:0"
F16 = torch.float16
SUB_LO, SUB_HI = 2.0 ** -24, 2.0 ** -14          # the fp16 subnormal range
BIG = 65520.0 * (1 + 1e-3)                       # references above this must store as Inf
SMALL = 65504.0 * (1 - 1e-3)                     # ... and below this as finite values


def to_ndhwc(x_ncdhw, dtype=F16):
    return x_ncdhw.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)


def from_ndhwc(t):
    return t.float().cpu().permute(0, 4, 1, 2, 3).contiguous()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def q(x):
    return x.half().float()


def subnormal(shape, seed):
    """fp16 values of log-uniform magnitude in [2^-24, 2^-14) and random sign: every one an fp16 subnormal"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(-24 + 10 * torch.rand(shape, generator=g))
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    x = q(mag * sign)
    assert float((x.abs() < SUB_HI).float().mean()) > 0.5 and float((x == 0).float().mean()) < 0.01
    return x


def check_subnormal(got, ref, absref, ref_flushed, what, rounded=True):
    """the bound against the reference on the subnormal operands; on failure also report how the result
    compares with the reference computed on flushed operands, which tells a flush from another error"""
    if rounded:
        assert float((ref.abs() > SUB_LO).double().mean()) > 0.5, what        # not underflowing to zero
        assert float((ref.abs() < SUB_HI).double().mean()) > 0.05, what       # not all in the normal range
    r = lb.ratio(got, ref, absref, rounded)
    if float(r.max()) > 1.0:
        rf = float(lb.ratio(got, ref_flushed, absref, rounded).max())
        raise AssertionError(f"{what}: worst ratio {float(r.max()):.3g} against the reference, {rf:.3g} against "
                             f"the reference on flushed operands")


def assert_overflow(got, ref, what):
    """exactly ±Inf where |ref| > 65520 (1 + 1e-3), finite where |ref| < 65504 (1 - 1e-3); the band between is
    not checked"""
    got, ref = got.double().cpu(), ref.double().cpu()
    big, small = ref.abs() > BIG, ref.abs() < SMALL
    assert int(big.sum()) > 0 and int(small.sum()) > 0, what
    want = torch.where(ref > 0, float("inf"), float("-inf"))
    assert torch.equal(got[big], want[big]), f"{what}: {int((got[big] != want[big]).sum())} of {int(big.sum())} " \
        f"overflowing elements are not ±Inf (e.g. {got[big][got[big] != want[big]][:3].tolist()})"
    assert bool(torch.isfinite(got[small]).all()), f"{what}: non-finite values where the reference is finite"


# ---------------------------------------------------------------------------------------------- subnormal operands
SUB_CONV_CASES = [
    # cin, cout, stride, spatial, batch -- the kernel families of tests/test_fp16_gpu.py
    (16, 16, 1, (16, 64, 128), 1),     # ring3 (LDS-DMA ring)
    (32, 32, 1, (33, 60, 120), 1),     # ring2, 32 -> 32
    (128, 48, 1, (5, 6, 7), 2),        # K-split
    (16, 32, 2, (10, 12, 36), 1),      # stride-2 MFMA
    (1, 16, 2, (12, 12, 12), 2),       # small-Cin MFMA
    (16, 3, 1, (6, 7, 9), 1),          # direct
]


@pytest.mark.parametrize("case", SUB_CONV_CASES, ids=lambda c: f"{c[0]}to{c[1]}s{c[2]}")
def test_conv_fwd_keeps_subnormal_activations(case):
    cin, cout, s, sp, n = case
    x = subnormal((n, cin) + sp, 1)
    w = rnd((cout, cin, 3, 3, 3), 2, 2.0 / math.sqrt(cin * 27))
    packed = ops.wpack(F16, 0, w.to(DEV), cin, cout, 3) if ops.mfma_ok(cin, cout) else None
    xd = to_ndhwc(x)
    osp = tuple((d - 1) // s + 1 for d in sp)
    yd = torch.empty((n,) + osp + (cout,), dtype=F16, device=DEV)
    name = ops.conv3d_fwd_kernel_name(xd, yd, 3, s)
    assert "f16" in name.replace("bf16", ""), name
    wq = w if "direct" in name else q(w)       # the direct kernel reads the f32 weights, the MFMA kernels round them
    ref, a = lb.conv_ref(x, wq, stride=s)
    ops.conv3d_fwd(xd, yd, packed, w.to(DEV), 0, None, 3, s)
    torch.cuda.synchronize()
    check_subnormal(from_ndhwc(yd), ref, a, lb.conv_ref(lb.flush_f16_subnormals(x), wq, stride=s)[0], name)


@pytest.mark.parametrize("cin,cout,sp,n", [(16, 16, (6, 8, 20), 2), (32, 32, (33, 60, 120), 1), (16, 8, (5, 5, 5), 1)])
def test_dgrad_keeps_subnormal_output_gradients(cin, cout, sp, n):
    dy = subnormal((n, cout) + sp, 11)
    w = rnd((cout, cin, 3, 3, 3), 12, 2.0 / math.sqrt(cout * 27))
    packed = ops.wpack(F16, 1, w.to(DEV), cout, cin, 3) if ops.mfma_ok(cin, cout) else None
    wq = q(w) if packed is not None else w
    ref, a = lb.convT_ref(dy, wq, stride=1, padding=1, output_padding=0)
    dyd = to_ndhwc(dy)
    dx = torch.empty((n,) + sp + (cin,), dtype=F16, device=DEV)
    ops.conv3d_fwd(dyd, dx, packed, w.to(DEV), 1, None, 3, 1)
    torch.cuda.synchronize()
    flushed = lb.convT_ref(lb.flush_f16_subnormals(dy), wq, stride=1, padding=1, output_padding=0)[0]
    check_subnormal(from_ndhwc(dx), ref, a, flushed, ops.conv3d_fwd_kernel_name(dyd, dx, 3, 1))


@pytest.mark.parametrize("cin,cout,sp,n", [(32, 16, (6, 6, 20), 2), (8, 4, (4, 5, 6), 2)])
def test_convT_fwd_keeps_subnormal_inputs(cin, cout, sp, n):
    x = subnormal((n, cin) + sp, 21)
    w = rnd((cin, cout, 3, 3, 3), 22, 2.0 / math.sqrt(cin * 27 / 8))
    packed = ops.wpack(F16, 2, w.to(DEV), cin, cout, 3) if ops.mfma_ok(cin, cout) else None
    wq = q(w) if packed is not None else w
    ref, a = lb.convT_ref(x, wq)
    xd = to_ndhwc(x)
    yd = torch.empty((n,) + tuple(ref.shape[2:]) + (cout,), dtype=F16, device=DEV)
    ops.convT3d_fwd(xd, yd, packed, w.to(DEV), None)
    torch.cuda.synchronize()
    check_subnormal(from_ndhwc(yd), ref, a, lb.convT_ref(lb.flush_f16_subnormals(x), wq)[0], f"convT {cin}->{cout}")


@pytest.mark.parametrize("case", [(16, 16, 1, (4, 16, 32), 2),      # MFMA weight gradient
                                  (16, 32, 2, (8, 8, 32), 1),
                                  (1, 16, 2, (12, 12, 12), 2),      # small-Cin
                                  (16, 16, 1, (40, 64, 8), 8),      # wave-specialised
                                  (16, 3, 1, (6, 6, 6), 1)],        # direct
                         ids=lambda c: f"{c[0]}to{c[1]}s{c[2]}n{c[4]}")
def test_wgrad_keeps_subnormal_output_gradients(case):
    cin, cout, s, sp, n = case
    x = q(rnd((n, cin) + sp, 31))
    osp = tuple((d - 1) // s + 1 for d in sp)
    dy = subnormal((n, cout) + osp, 32)
    dw_ref, a_dw, db_ref, a_db = lb.wgrad_ref(x, dy, 3, s)
    xd, dyd = to_ndhwc(x), to_ndhwc(dy)
    dw = torch.empty((cout, cin, 3, 3, 3), device=DEV)
    db = torch.empty(cout, device=DEV)
    ws = torch.empty(ops.conv3d_wgrad_workspace(xd, dyd, 3, s), dtype=torch.uint8, device=DEV)
    ops.conv3d_wgrad(xd, dyd, dw, db, 3, s, ws)
    torch.cuda.synchronize()
    dyf = lb.flush_f16_subnormals(dy)
    check_subnormal(dw.cpu(), dw_ref, a_dw, lb.wgrad_ref(x, dyf, 3, s)[0], "dw", rounded=False)
    check_subnormal(db.cpu(), db_ref, a_db, dyf.double().sum((0, 2, 3, 4)), "db", rounded=False)


def _bn_bwd_operands(c, sp, n, seed):
    x = q(rnd((n, c) + sp, seed, 2.0))
    dy = subnormal((n, c) + sp, seed + 1)
    mean, invstd = rnd((c,), seed + 2) * 0.5, rnd((c,), seed + 3).abs() + 0.5
    gamma, beta = rnd((c,), seed + 4) + 1.5, rnd((c,), seed + 5) * 0.3
    coef = torch.stack([rnd((c,), seed + 6, 2.0 ** -17), rnd((c,), seed + 7, 2.0 ** -17)])
    return x, dy, mean, invstd, gamma, beta, coef


def _apply_ref(dy, x, mean, invstd, gamma, coef):
    """dx = gamma invstd (dz - c0 - xhat c1), dz = dy (no PReLU); float64, with its |operand| companion"""
    v = lambda t: t.double().view(1, -1, 1, 1, 1)
    xhat = (x.double() - v(mean)) * v(invstd)
    k = v(gamma) * v(invstd)
    ref = k * (dy.double() - v(coef[0]) - xhat * v(coef[1]))
    a = k.abs() * (dy.double().abs() + v(coef[0]).abs() + (xhat * v(coef[1])).abs())
    return ref, a


@pytest.mark.parametrize("c,sp,n", [(16, (6, 10, 14), 2), (32, (8, 8, 8), 2)])
def test_bn_act_bwd_apply_keeps_subnormal_gradients(c, sp, n):
    x, dy, mean, invstd, gamma, beta, coef = _bn_bwd_operands(c, sp, n, 41)
    xd, dyd = to_ndhwc(x), to_ndhwc(dy)
    dx = torch.empty_like(xd)
    ops.bn_act_bwd_apply(dyd, xd, dx, mean.to(DEV), invstd.to(DEV), gamma.to(DEV), beta.to(DEV), None,
                         coef.to(DEV).contiguous())
    torch.cuda.synchronize()
    ref, a = _apply_ref(dy, x, mean, invstd, gamma, coef)
    flushed = _apply_ref(lb.flush_f16_subnormals(dy), x, mean, invstd, gamma, coef)[0]
    check_subnormal(from_ndhwc(dx), ref, a, flushed, "bn_act_bwd_apply")


def test_bn_backward_one_launch_keeps_subnormal_gradients():
    """segmi_bn_act_bwd_fused: the f32 sums over subnormal dy and the applied dx"""
    c, sp, n = 32, (8, 8, 8), 2
    x, dy, mean, invstd, gamma, beta, _ = _bn_bwd_operands(c, sp, n, 51)
    xd, dyd = to_ndhwc(x), to_ndhwc(dy)
    md, isd, gd, bd = (t.to(DEV) for t in (mean, invstd, gamma, beta))
    dg, db, coef = torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.empty((2, c), device=DEV)
    part = torch.zeros((ops.bn_act_bwd_fused_rows(xd), 3, c), device=DEV)
    dx = torch.full_like(xd, float("nan"))
    assert ops.bn_act_bwd_fused_ok(dyd, xd, dx)
    ops.bn_act_bwd_fused(dyd, xd, dx, md, isd, gd, bd, None, part, (n * sp[0] * sp[1] * sp[2], dg, db, None, coef))
    torch.cuda.synchronize()
    v = lambda t: t.double().view(1, -1, 1, 1, 1)
    xhat = (x.double() - v(mean)) * v(invstd)
    dyf = lb.flush_f16_subnormals(dy).double()
    # dbeta = sum dy, dgamma = sum dy xhat (f32 outputs)
    check_subnormal(db.cpu(), dy.double().sum((0, 2, 3, 4)), dy.double().abs().sum((0, 2, 3, 4)),
                    dyf.sum((0, 2, 3, 4)), "dbeta", rounded=False)
    check_subnormal(dg.cpu(), (dy.double() * xhat).sum((0, 2, 3, 4)), (dy.double() * xhat).abs().sum((0, 2, 3, 4)),
                    (dyf * xhat).sum((0, 2, 3, 4)), "dgamma", rounded=False)
    # dx with the coefficients the launch derived (read back; their own accuracy is the sums' above)
    ref, a = _apply_ref(dy, x, mean, invstd, gamma, coef.cpu())
    check_subnormal(from_ndhwc(dx), ref, a, _apply_ref(dyf.float(), x, mean, invstd, gamma, coef.cpu())[0], "dx")


def test_bn_backward_apply_inside_the_stride2_convolution_keeps_subnormal_gradients():
    """conv_s2_bnbwd: dx (stored by the kernel) and the stride-2 convolution of it"""
    c, cout, sp, n = 16, 32, (16, 24, 40), 2
    x, dy, mean, invstd, gamma, beta, coef = _bn_bwd_operands(c, sp, n, 61)
    xd, dyd = to_ndhwc(x), to_ndhwc(dy)
    w = rnd((cout, c, 3, 3, 3), 67, 2.0 / math.sqrt(c * 27))
    pack = ops.wpack(F16, 0, w.to(DEV), c, cout, 3)
    osp = tuple((v - 1) // 2 + 1 for v in sp)
    out = torch.full((n,) + osp + (cout,), float("nan"), dtype=F16, device=DEV)
    dx = torch.full_like(xd, float("nan"))
    assert ops.bn_act_bwd_apply_conv_ok(dyd, xd, dx, out)
    ops.bn_act_bwd_apply_conv(dyd, xd, dx, mean.to(DEV), invstd.to(DEV), gamma.to(DEV), beta.to(DEV), None,
                              coef.to(DEV).contiguous(), out, pack)
    torch.cuda.synchronize()
    ref, a = _apply_ref(dy, x, mean, invstd, gamma, coef)
    flushed = _apply_ref(lb.flush_f16_subnormals(dy), x, mean, invstd, gamma, coef)[0]
    dxg = from_ndhwc(dx)
    check_subnormal(dxg, ref, a, flushed, "conv_s2_bnbwd dx")
    # the convolution reads the dx it stored (fp16): its reference is the conv of those values
    cref, ca = lb.conv_ref(dxg, q(w), stride=2)
    lb.assert_within(from_ndhwc(out), cref, ca, what="conv_s2_bnbwd out")


def _dice_grads(lg, lab, scale_of):
    """dlogits of the f32 kernel (scale 1) and of the fp16 loss-scaled kernel at scale_of(f32 gradient)"""
    n, k = lg.shape[:2]
    labd = lab.to(DEV).reshape(-1).contiguous()
    outs, scale = {}, None
    for dt in (torch.float32, F16):
        ld = to_ndhwc(lg, dt)
        part = torch.empty((n, ops.dice_chunks(ld), 3, k), device=DEV)
        coef = torch.empty((n, 2, k), device=DEV)
        ops.softmax_dice_fwd(ld, labd, part, coef, torch.empty(1, device=DEV))
        dl = torch.empty_like(ld)
        if dt == F16:
            ops.softmax_dice_bwd_amp(ld, labd, coef, torch.tensor([scale, 0.0, 0.0], device=DEV), dl)
        else:
            ops.softmax_dice_bwd(ld, labd, coef, 1.0, dl)
        torch.cuda.synchronize()
        outs[dt] = from_ndhwc(dl).double()
        if dt == torch.float32:
            scale = scale_of(outs[dt])
    return outs[torch.float32] * scale, outs[F16], scale


@pytest.mark.parametrize("where", ["default", "subnormal"])
@pytest.mark.parametrize("k", [3, 16])
def test_softmax_dice_backward_amp_stores_each_dlogit(k, where):
    """dlogits of the loss-scaled backward, element by element, against the f32 kernel's gradient on the same fp16
    logits times the scale: at the default scale 2^16, and at a power-of-two scale that puts the median dlogit at
    2^-19, so that most of the stored values are fp16 subnormals"""
    n, sp = 2, (16, 32, 32)
    lg = q(rnd((n, k) + sp, 71, 3.0))
    lab = torch.randint(0, k, (n, 1) + sp, generator=torch.Generator().manual_seed(72)).float()
    if where == "default":
        scale_of = lambda g: 2.0 ** 16
    else:
        scale_of = lambda g: 2.0 ** round(-19 - math.log2(float(g.abs().median())))
    ref, got, scale = _dice_grads(lg, lab, scale_of)
    if where == "subnormal":
        assert float((ref.abs() < SUB_HI).double().mean()) > 0.5, scale
    # the f32 kernel's own error is ~2^-22 of the value: inside the accumulation term with A = |ref|
    r = lb.ratio(got, ref, ref.abs())
    assert float(r.max()) <= 1.0, (scale, float(r.max()), float(lb.ratio(got, lb.flush_f16_subnormals(ref), ref.abs()).max()))


# ---------------------------------------------------------------------------------------------- overflow to Inf
def _overflow_bias(cout):
    """per-channel bias: channels 0, 1 -> +/-70000 (must overflow), 2, 3 -> +/-60000 and the rest 1000 (finite)"""
    b = torch.full((cout,), 1000.0)
    b[0], b[1], b[2] = 70000.0, -70000.0, 60000.0
    if cout > 3:
        b[3] = -60000.0
    return b


OVF_CONV_CASES = [
    (16, 16, 1, (16, 64, 128), 1),     # ring3: H16::pack2
    (32, 32, 1, (33, 60, 120), 1),     # ring2: H16::pack2
    (32, 64, 2, (8, 8, 16), 1),        # MFMA conv: store4
    (128, 48, 1, (5, 6, 7), 2),        # K-split: store4
    (1, 16, 2, (12, 12, 12), 2),       # small-Cin
    (16, 3, 1, (6, 7, 9), 1),          # direct: Elem::st
]


@pytest.mark.parametrize("case", OVF_CONV_CASES, ids=lambda c: f"{c[0]}to{c[1]}s{c[2]}")
def test_conv_fwd_store_overflows_to_inf(case):
    cin, cout, s, sp, n = case
    x = q(rnd((n, cin) + sp, 81))
    w = rnd((cout, cin, 3, 3, 3), 82, 0.01)
    b = _overflow_bias(cout)
    packed = ops.wpack(F16, 0, w.to(DEV), cin, cout, 3) if ops.mfma_ok(cin, cout) else None
    ref, _ = lb.conv_ref(x, q(w) if packed is not None else w, b, stride=s)
    xd = to_ndhwc(x)
    yd = torch.empty((n,) + tuple(ref.shape[2:]) + (cout,), dtype=F16, device=DEV)
    ops.conv3d_fwd(xd, yd, packed, w.to(DEV), 0, b.to(DEV), 3, s)
    torch.cuda.synchronize()
    assert_overflow(from_ndhwc(yd), ref, ops.conv3d_fwd_kernel_name(xd, yd, 3, s))


@pytest.mark.parametrize("cin,cout,sp,n", [(32, 16, (6, 6, 20), 2), (64, 16, (5, 3, 33), 1), (8, 4, (4, 5, 6), 2)])
def test_convT_fwd_store_overflows_to_inf(cin, cout, sp, n):
    """Vec8::store of the pixel-shuffle kernels (and Elem::st of the direct one)"""
    x = q(rnd((n, cin) + sp, 91))
    w = rnd((cin, cout, 3, 3, 3), 92, 0.01)
    b = _overflow_bias(cout)
    packed = ops.wpack(F16, 2, w.to(DEV), cin, cout, 3) if ops.mfma_ok(cin, cout) else None
    ref, _ = lb.convT_ref(x, q(w) if packed is not None else w, b)
    xd = to_ndhwc(x)
    yd = torch.empty((n,) + tuple(ref.shape[2:]) + (cout,), dtype=F16, device=DEV)
    ops.convT3d_fwd(xd, yd, packed, w.to(DEV), b.to(DEV))
    torch.cuda.synchronize()
    assert_overflow(from_ndhwc(yd), ref, f"convT {cin}->{cout}")


def test_dectop_store_overflows_to_inf():
    """the fused decoder top (H16::pack2): the conv bias pushes two channels past fp16"""
    n, d, h, w = 1, 8, 16, 16
    x = to_ndhwc(rnd((n, 32, d, h, w), 501))
    wt, wc = rnd((32, 16, 3, 3, 3), 502, 0.06).to(DEV), rnd((16, 16, 3, 3, 3), 503, 0.01).to(DEV)
    scale, ub = (rnd((16,), 504).abs() + 0.5).to(DEV), (rnd((16,), 505) * 0.2).to(DEV)
    cb = _overflow_bias(16).to(DEV)
    alpha = torch.full((1,), 0.25, device=DEV)
    fine = (n, 2 * d, 2 * h, 2 * w, 16)
    out = torch.full(fine, float("nan"), dtype=F16, device=DEV)
    assert ops.dectop_ok(x, out)
    ops.dectop_fwd(x, out, ops.dectop_up_frag(wt, scale, dtype=F16), ub, alpha, ops.wpack(F16, 0, wc, 16, 16, 3), cb,
                   alpha_in_unit_range=True)
    torch.cuda.synchronize()
    # |conv(h) + h| stays below 100 here, so the bias decides the class of every element
    ref = cb.cpu().double().view(1, -1, 1, 1, 1).expand(n, 16, 2 * d, 2 * h, 2 * w)
    assert_overflow(from_ndhwc(out), ref, "dectop")


def test_bn_act_fwd_and_bwd_apply_store_overflow_to_inf():
    """Elem::st of the BatchNorm-apply kernels"""
    c, sp, n = 16, (4, 6, 8), 2
    x = q(rnd((n, c) + sp, 111))
    shift = _overflow_bias(c)
    scale = torch.full((c,), 2.0)
    xd = to_ndhwc(x)
    y = torch.empty_like(xd)
    ops.bn_act_fwd(xd, y, scale.to(DEV), shift.to(DEV))
    torch.cuda.synchronize()
    assert_overflow(from_ndhwc(y), x.double() * 2.0 + shift.double().view(1, -1, 1, 1, 1), "bn_act_fwd")
    # backward apply: dx = gamma invstd dy with dy up to 40000 and gamma invstd = 2 on channels 0, 1
    dy = q(rnd((n, c) + sp, 112, 100.0))
    dy[:, 0] = 40000.0
    dy[:, 1] = -40000.0
    dy[:, 2] = 30000.0
    gamma = torch.ones(c)
    gamma[:2] = 2.0
    dx = torch.empty_like(xd)
    ops.bn_act_bwd_apply(to_ndhwc(dy), xd, dx, torch.zeros(c, device=DEV), torch.ones(c, device=DEV),
                         gamma.to(DEV), torch.zeros(c, device=DEV), None, torch.zeros((2, c), device=DEV))
    torch.cuda.synchronize()
    assert_overflow(from_ndhwc(dx), dy.double() * gamma.double().view(1, -1, 1, 1, 1), "bn_act_bwd_apply")


def test_dice_backward_store_overflows_to_inf():
    """dlogits at a power-of-two loss scale that puts the median |dlogit| near 65536, so that a known set of
    voxels leaves fp16"""
    k, n, sp = 3, 1, (4, 4, 8)
    lg = q(rnd((n, k) + sp, 121, 3.0))
    lab = torch.randint(0, k, (n, 1) + sp, generator=torch.Generator().manual_seed(122)).float()
    ref, got, scale = _dice_grads(lg, lab, lambda g: 2.0 ** round(16 - math.log2(float(g.abs().median()))))
    assert_overflow(got, ref, f"softmax_dice_bwd_amp at scale {scale}")


def test_format_kernels_store_overflow_to_inf():
    """crop_patches and nchw_to_ndhwc: f32 sources beyond fp16's range become ±Inf"""
    g = torch.Generator().manual_seed(131)
    img = torch.randn((1, 10, 12, 14, 1), generator=g) * 1000.0
    img.view(-1)[::7] = 70000.0
    img.view(-1)[3::7] = -1.0e6
    img.view(-1)[5::7] = 65000.0
    lab = torch.zeros((10, 12, 14))
    out = torch.empty((1, 6, 8, 10, 1), dtype=F16, device=DEV)
    ops.crop_patches(img.to(DEV), lab.to(DEV), [[0, 2, 3, 4]], None, out, torch.empty((1, 6, 8, 10), device=DEV))
    torch.cuda.synchronize()
    assert_overflow(out.float().cpu(), img[:, 2:8, 3:11, 4:14], "crop_patches")
    src = torch.randn((2, 3, 4, 5, 6), generator=g) * 1000.0
    src.view(-1)[::5] = 1.0e5
    src.view(-1)[2::5] = -70000.0
    dst = torch.empty((2, 4, 5, 6, 3), dtype=F16, device=DEV)
    ops.nchw_to_ndhwc(src.to(DEV), dst)
    torch.cuda.synchronize()
    assert_overflow(dst.float().cpu(), src.permute(0, 2, 3, 4, 1), "nchw_to_ndhwc")


# ---------------------------------------------------------------------------------------------- Inf / NaN propagation
BAD = [pytest.param(float("inf"), id="inf"), pytest.param(float("-inf"), id="-inf"), pytest.param(float("nan"), id="nan")]


def _found_inf(*grads):
    amp = torch.tensor([2.0 ** 16, 0.0, 0.0], device=DEV)
    ops.amp_check_finite(torch.cat([g.reshape(-1).float().to(DEV) for g in grads]), amp)
    torch.cuda.synchronize()
    return float(amp[1].cpu()) != 0.0


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("case", [(16, 16, 1, (4, 16, 32), 2), (16, 16, 1, (40, 64, 8), 8), (1, 16, 2, (12, 12, 12), 2),
                                  (16, 3, 1, (6, 6, 6), 1)], ids=lambda c: f"{c[0]}to{c[1]}n{c[4]}")
def test_wgrad_carries_a_non_finite_output_gradient(case, bad):
    cin, cout, s, sp, n = case
    x = q(rnd((n, cin) + sp, 141)) + 2.0                   # no zero in x: every tap that reads the voxel sees it
    osp = tuple((d - 1) // s + 1 for d in sp)
    dy = q(rnd((n, cout) + osp, 142))
    co = cout - 1
    dy[n - 1, co, osp[0] // 2, osp[1] // 2, osp[2] // 2] = bad
    xd, dyd = to_ndhwc(x), to_ndhwc(dy)
    dw, db = torch.empty((cout, cin, 3, 3, 3), device=DEV), torch.empty(cout, device=DEV)
    ws = torch.empty(ops.conv3d_wgrad_workspace(xd, dyd, 3, s), dtype=torch.uint8, device=DEV)
    ops.conv3d_wgrad(xd, dyd, dw, db, 3, s, ws)
    torch.cuda.synchronize()
    dw, db = dw.cpu(), db.cpu()
    assert not bool(torch.isfinite(dw[co]).any()), "every dw[co] depends on the non-finite element"
    assert not math.isfinite(float(db[co]))
    assert bool(torch.isfinite(dw[:co]).all()) and bool(torch.isfinite(db[:co]).all())
    assert _found_inf(dw, db)


@pytest.mark.parametrize("bad", BAD)
def test_bn_backward_sums_carry_a_non_finite_gradient(bad):
    """dgamma / dbeta of channel 5 non-finite in the reduce launch, the one-launch form and the sums fused into the
    ring input-gradient kernels (ring3 for 16 channels, ring2 for 32); the other channels stay finite"""
    count_of = lambda t: t.shape[0] * t.shape[1] * t.shape[2] * t.shape[3]
    for c, sp, n in ((16, (32, 64, 128), 2), (32, (33, 60, 120), 2)):
        x = to_ndhwc(q(rnd((n, c) + sp, 151, 2.0)) + 0.3)
        dy_cpu = q(rnd((n, c) + sp, 152))
        dy_cpu[0, 5, 3, 4, 5] = bad
        dy = to_ndhwc(dy_cpu)
        mean, invstd = (rnd((c,), 153) * 0.5).to(DEV), (rnd((c,), 154).abs() + 0.5).to(DEV)
        gamma, beta = (rnd((c,), 155) + 1.5).to(DEV), (rnd((c,), 156) * 0.3).to(DEV)
        alpha = torch.full((1,), 0.25, device=DEV)
        results = {}
        # the separate reduce + finalize, with the finalize fused into the reduce launch
        rows = ops.bn_act_bwd_rows(x)
        dg, db, da, coef = torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.empty(1, device=DEV), \
            torch.empty((2, c), device=DEV)
        ops.bn_act_bwd_reduce(dy, x, mean, invstd, gamma, beta, alpha, torch.zeros((rows, 3, c), device=DEV),
                              fin=(count_of(x), dg, db, da, coef))
        results["reduce"] = (dg.clone(), db.clone())
        if ops.bn_act_bwd_fused_ok(dy, x, x):
            dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
            dx = torch.empty_like(x)
            ops.bn_act_bwd_fused(dy, x, dx, mean, invstd, gamma, beta, alpha,
                                 torch.zeros((ops.bn_act_bwd_fused_rows(x), 3, c), device=DEV),
                                 (count_of(x), dg, db, torch.empty(1, device=DEV), torch.empty((2, c), device=DEV)))
            results["one launch"] = (dg.clone(), db.clone())
        # MODE 4: the sums over the stored input gradient of a conv whose output gradient carries the value
        pk = ops.wpack(F16, 1, rnd((c, c, 3, 3, 3), 157, 0.08).to(DEV), c, c, 3)
        assert ops.conv3d_bn_bwd_sums_ok(dy, dy, 3, 1)
        g = torch.empty_like(dy)
        rows = ops.conv3d_stats_rows(dy, g, 3, 1)
        dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        ops.conv3d_fwd(dy, g, pk, None, 1, None, 3, 1, residual=dy,
                       bn_bwd=(x, mean, invstd, gamma, beta, alpha, torch.zeros((rows, 3, c), device=DEV)),
                       bn_bwd_fin=(count_of(x), dg, db, torch.empty(1, device=DEV), torch.empty((2, c), device=DEV)))
        results[ops.conv3d_fwd_kernel_name(dy, g, 3, 1)] = (dg.clone(), db.clone())
        torch.cuda.synchronize()
        for where, (dg, db) in results.items():
            dg, db = dg.cpu(), db.cpu()
            assert not math.isfinite(float(dg[5])) and not math.isfinite(float(db[5])), (c, where)
            keep = torch.arange(c) != 5
            if where == "reduce" or where == "one launch":
                assert bool(torch.isfinite(dg[keep]).all()) and bool(torch.isfinite(db[keep]).all()), (c, where)
            assert _found_inf(dg, db), (c, where)


# ---------------------------------------------------------------------------------------------- amp_check_finite
@pytest.mark.parametrize("length", [1, 3, 4, 5, 257, 2048 * 256 * 4 + 3])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_amp_check_finite_flags_inf_and_nan_anywhere(length, offset):
    buf = torch.zeros(length + 1, device=DEV)
    g = buf[offset:offset + length]
    g.copy_(rnd((length,), 161).to(DEV))
    where = sorted({0, length - 1, max(0, length - 2), length // 2})
    for bad in (float("inf"), float("-inf"), float("nan")):
        for i in where:
            amp = torch.tensor([2.0 ** 16, 0.0, 0.0], device=DEV)
            g[i] = bad
            ops.amp_check_finite(g, amp)
            torch.cuda.synchronize()
            assert float(amp[1].cpu()) != 0.0, (length, offset, bad, i)
            assert float(amp[0].cpu()) == 2.0 ** 16                  # the check never touches the scale
            g[i] = 0.5
    # large finite values, f32 subnormals and -0 are not flagged; nor is a non-finite value just outside the range
    g[:] = torch.tensor([3.4028234663852886e38, -3.4028234663852886e38, 1e-45, -1e-45, -0.0, 1.0e-39],
                        device=DEV).repeat(length // 6 + 1)[:length]
    buf[length if offset == 0 else 0] = float("nan")
    amp = torch.tensor([2.0 ** 16, 0.0, 0.0], device=DEV)
    ops.amp_check_finite(g, amp)
    torch.cuda.synchronize()
    assert float(amp[1].cpu()) == 0.0


# ---------------------------------------------------------------------------------------------- format-only kernels
def test_format_kernels_are_bit_exact_in_fp16():
    """crop_patches, warp_crop_patches, nchw_to_ndhwc, sw_gather and ndhwc_to_nchw move or convert data only: the
    fp16 output equals the f32 kernel's output converted by torch, bit for bit (ndhwc_to_nchw: torch's fp16 -> f32)"""
    from segmantic_amd.seg.augment import _rot, to_index_map_xyz
    g = torch.Generator().manual_seed(171)
    D, H, W = 20, 24, 28
    img = torch.randn((1, D, H, W, 1), generator=g) * torch.exp2(torch.randint(-20, 10, (1, D, H, W, 1), generator=g))
    lab = torch.randint(0, 4, (D, H, W), generator=g).float()
    imd, lad = img.to(DEV), lab.to(DEV)
    roi = (8, 12, 16)
    starts, flips = [[0, 3, 5, 7], [0, -2, 15, 20]], [0, 5]
    o32 = torch.empty((2,) + roi + (1,), device=DEV)
    o16 = torch.empty((2,) + roi + (1,), dtype=F16, device=DEV)
    l32, l16 = torch.empty((2,) + roi, device=DEV), torch.empty((2,) + roi, device=DEV)
    ops.crop_patches(imd, lad, starts, flips, o32, l32)
    ops.crop_patches(imd, lad, starts, flips, o16, l16)
    torch.cuda.synchronize()
    assert torch.equal(o16.cpu().view(torch.int16), o32.cpu().half().view(torch.int16))
    assert torch.equal(l16, l32)
    ctr = (np.array([D, H, W]) - 1) / 2.0
    to_c, from_c = np.eye(4), np.eye(4)
    to_c[:3, 3], from_c[:3, 3] = -ctr, ctr
    m = from_c @ _rot(0, -0.3) @ np.diag([1 / 1.2, 1 / 1.2, 1 / 1.2, 1.0]) @ to_c
    ops.warp_crop_patches(imd, lad, starts, flips, to_index_map_xyz(m), o32, l32)
    ops.warp_crop_patches(imd, lad, starts, flips, to_index_map_xyz(m), o16, l16)
    torch.cuda.synchronize()
    assert torch.equal(o16.cpu().view(torch.int16), o32.cpu().half().view(torch.int16))
    assert torch.equal(l16, l32)
    src = img.permute(0, 4, 1, 2, 3).contiguous()
    s32 = torch.empty((1, D, H, W, 1), device=DEV)
    s16 = torch.empty((1, D, H, W, 1), dtype=F16, device=DEV)
    ops.nchw_to_ndhwc(src.to(DEV), s32)
    ops.nchw_to_ndhwc(src.to(DEV), s16)
    torch.cuda.synchronize()
    assert torch.equal(s32.cpu(), img)
    assert torch.equal(s16.cpu().view(torch.int16), img.half().view(torch.int16))
    back = torch.empty((1, 1, D, H, W), device=DEV)
    ops.ndhwc_to_nchw(s16, back)
    torch.cuda.synchronize()
    assert torch.equal(back.cpu(), src.half().float())
    wins = [(0, 0, 0), (4, 8, 12), (12, 16, 20)]
    w16 = torch.empty((3, 8, 8, 8, 1), dtype=F16, device=DEV)
    ops.sw_gather(s16, 0, wins, w16)
    torch.cuda.synchronize()
    for i, (z, y, x) in enumerate(wins):
        assert torch.equal(w16[i, ..., 0].cpu().view(torch.int16), img[0, z:z + 8, y:y + 8, x:x + 8, 0].half().view(torch.int16))


@pytest.mark.parametrize("K", [7, 4, 16])
def test_sw_blend_of_an_fp16_cache_matches_the_oracle(K):
    """the sliding-window scatter / finalize path on fp16 window predictions: bit-exact sums and labels, as in f32"""
    from oracle.sliding_ref import ref_sliding_window_inference
    from segmantic_amd.seg.inferers import dense_starts
    img = rnd((1, 1, 20, 27, 33), 181)
    roi = (16, 16, 16)
    wts = rnd((K, 1, 3, 3, 3), 182)

    def predictor(x):
        return q(F.conv3d(x, wts, padding=1))

    ref, cnt_ref, wins = ref_sliding_window_inference(img, roi, 4, predictor, 0.5)
    per_dim = dense_starts((20, 27, 33), roi, 0.5)
    cache = torch.empty((len(wins),) + roi + (K,), dtype=F16, device=DEV)
    for g0 in range(0, len(wins), 4):
        grp = wins[g0:g0 + 4]
        pred = predictor(torch.cat([img[:, :, z:z + 16, y:y + 16, x:x + 16] for z, y, x in grp]))
        cache[g0:g0 + len(grp)] = pred.permute(0, 2, 3, 4, 1).to(DEV).to(F16)
    out = torch.empty((1, 20, 27, 33, K), device=DEV)
    cnt = torch.empty((20, 27, 33), device=DEV)
    lab = torch.empty((20, 27, 33), dtype=torch.uint8, device=DEV)
    ops.sw_blend(cache, per_dim, 0, len(wins), roi, 20, 27, 33, out_logits=out, out_count=cnt, labels=lab)
    torch.cuda.synchronize()
    assert torch.equal(cnt.cpu(), cnt_ref[0, 0])
    assert torch.equal(out.cpu().permute(0, 4, 1, 2, 3), ref)
    assert torch.equal(lab.cpu().long(), torch.argmax(ref, 1)[0])
