"""Where the network-path kernels read and write: every activation of every launch inside a poisoned arena.

Each launch runs with its input activations (x, residual, dy, the BatchNorm-backward x, logits) and its output
activations cut out of arenas of tests/helpers/view_arena.py: guard rows in front and behind, sibling channels beside the
view, all of it a quiet NaN of a payload no kernel produces.  After the launch

  (a) every arena holds the poison bits everywhere outside its view (inputs too, and the inputs hold their data),
  (b) every element of an output view was written,
  (c) every output, statistics row, partial row, dw / db, loss and coefficient is finite -- a read outside an input view
      that is not discarded by a select brings the NaN in,
  (d) the result lies inside the bound the suite already holds that launch to (lowp_bounds, wgrad_bound, bn_bwd_bound,
      or the bit-identical comparison with the separate launches on dense tensors).

View forms (ld, c0) of a c-channel view: dense (c, 0), left (2c, 0), right (2c, c), odd (max(2c, 8), 4).  Where a
launcher refuses a form the refusal and the untouched arenas are asserted; where a form moves the layer to another
kernel family, the family the query reports is asserted and the case kept.  With 16-bit storage the MFMA launchers
refuse the odd form on an INPUT (rows 8 bytes in); the case then goes on with the inputs as right slices and the
outputs odd, which is the form that moves a ring3 layer to ring2.

What the launchers do with the forms (asserted case by case below):
  * dense, left and right are taken by every launch, inputs and outputs;
  * odd inputs are refused by the 16-bit MFMA launchers (ring, k-split, tile, split_act, transposed persistent and tile,
    bn_act_bwd_apply_conv -- its dx too --, dectop); odd outputs are taken, and move a ring3 layer to ring2 CK=16;
  * f32 k-split, small-Cin, direct, the first-layer pair, the element-wise passes and the losses take all four;
  * a 16-bit odd x / dy moves a wave-specialised, MFMA or small-Cin weight gradient to the direct kernel, which refuses
    an input transform; bn_act_bwd_fused refuses channel counts that are no multiple of 4.

Shapes: the smallest extents at which the query confirms the family, ragged on every axis the family tiles, batch 2.
Statistics tables and workspaces carry the sentinel guard of tests/test_conv_plan_gpu.py.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from tests.helpers import lowp_bounds as lb  # noqa: E402
from tests.helpers import view_arena as va  # noqa: E402
from tests.helpers.imbalance_loss_ref import ref_dice_focal_loss, ref_tversky_loss  # noqa: E402
from tests.helpers.loss_ref import ref_dice_ce_loss  # noqa: E402
from tests.helpers.reduce_cases import drop_mask  # noqa: E402
from tests.test_conv_plan_gpu import GUARD_BYTES, SENTINEL, guard_intact, reserve_rows, sentinel_table  # noqa: E402
from tests.test_ops_gpu import DEV, bn_bwd_bound, bn_fwd_ref64, elem_bound, epilogue64, q, rnd  # noqa: E402

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT_NAME = {BF16: "bf16", F16: "f16", F32: "f32"}
FORMS = ("dense", "left", "right", "odd")
REFUSED = (ValueError, RuntimeError)        # a launcher's refusal: bad argument status raised by the binding


def form_of(c, name):
    """(ld, c0); the odd form of a view of fewer than 4 channels sits in a row of 8"""
    return (max(2 * c, 8), 4) if name == "odd" else va.forms(c)[name]


def all_forms(dtypes, extra=()):
    """bf16 (the first type) in all four forms, a type that only changes the template argument as a right slice"""
    out = [(dt, f) for dt in dtypes for f in FORMS] + [(dt, "right") for dt in extra]
    return [pytest.param(dt, f, id=f"{DT_NAME[dt]}-{f}") for dt, f in out]


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(view):
    return view.float().cpu().permute(0, 4, 1, 2, 3).contiguous()


class Arenas:
    """the activation views of one launch"""

    def __init__(self):
        self.ins, self.outs = [], []

    def inp(self, x_ncdhw, dtype, form):
        t = ndhwc(x_ncdhw).to(DEV, dtype)
        rows, view = va.arena(tuple(t.shape), dtype, *form_of(t.shape[-1], form), device=DEV)
        va.fill_view(view, t)
        self.ins.append((rows, view, t))
        return view

    def out(self, shape_ndhwc, dtype, form):
        rows, view = va.arena(tuple(shape_ndhwc), dtype, *form_of(shape_ndhwc[-1], form), device=DEV)
        self.outs.append((rows, view))
        return view

    def check(self):
        """(a), (b) and the outputs' part of (c)"""
        torch.cuda.synchronize()
        for i, (rows, view, data) in enumerate(self.ins):
            assert va.outside_intact(rows, view), f"input {i}: stored outside the view"
            assert torch.equal(va.bits(view), va.bits(data)), f"input {i}: overwritten"
        for i, (rows, view) in enumerate(self.outs):
            assert va.outside_intact(rows, view), f"output {i}: stored outside the view"
            assert va.inside_written(view), f"output {i}: elements of the view left unwritten"
            assert bool(torch.isfinite(view.float()).all()), f"output {i}: not finite (a read outside an input view?)"

    def check_untouched(self):
        """after a refusal"""
        torch.cuda.synchronize()
        for rows, view, data in self.ins:
            assert va.outside_intact(rows, view) and torch.equal(va.bits(view), va.bits(data))
        for rows, _ in self.outs:
            assert va.untouched(rows)


def finite(*tensors):
    for t in tensors:
        if t is not None:
            assert bool(torch.isfinite(t.float()).all())


def relerr64(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def h16(dtype):
    return dtype in (BF16, F16)


def refuses(launch, arenas):
    with pytest.raises(REFUSED):
        launch()
    arenas.check_untouched()


# ---------------------------------------------------------------------------------------------- forward convolution
# family key -> (substring of the kernel name, storage types in four forms, types as a right slice only,
#                input (n, d, h, w), cin, cout, k, s, variants)
RING = (2, 13, 61, 250)          # 256 columns of 8 x 16, 4 z-steps: the smallest layer the ring kernels take
FWD = {
    "ring3": ("conv_ring3", [BF16], [F16], RING, 16, 16, 3, 1, ("plain", "epilogue", "in_tf", "identity")),
    "ring2-32-nt2": ("conv_ring2_kernel<{dt}, CK=32, NT=2>", [BF16], [F16], RING, 32, 32, 3, 1,
                     ("plain", "epilogue", "in_tf", "identity")),
    "ring2-32-nt1": ("conv_ring2_kernel<{dt}, CK=32, NT=1>", [BF16], [], RING, 32, 48, 3, 1, ("plain", "epilogue", "in_tf")),
    "ksplit-16bit": ("conv_fwd_ks", [BF16, F16], [], (2, 5, 6, 19), 64, 64, 3, 1, ("plain", "epilogue")),
    "ksplit-narrow": ("conv_fwd_ks", [BF16], [], (2, 5, 6, 7), 64, 48, 3, 1, ("plain", "epilogue")),
    "ksplit-f32": ("conv_fwd_ks", [F32], [], (2, 5, 6, 19), 32, 32, 3, 1, ("plain", "epilogue")),
    "tile-k3s1": ("conv_fwd_mfma_kernel<{dt}, CK=16, k3 s1>", [BF16], [F16], (2, 5, 9, 19), 16, 16, 3, 1, ("plain", "epilogue")),
    "tile-k3s2": ("conv_fwd_mfma_kernel<{dt}, CK=32, k3 s2>", [BF16], [F16], (2, 9, 10, 35), 32, 64, 3, 2, ("plain", "epilogue")),
    "tile-k1s1": ("conv_fwd_mfma_kernel<{dt}, CK=16, k1 s1>", [BF16], [F16], (2, 5, 9, 19), 16, 16, 1, 1, ("plain", "epilogue")),
    "small-cin": ("conv_small_fwd", [BF16, F32], [F16], (2, 9, 17, 35), 1, 16, 3, 2, ("plain", "epilogue")),
    "small-cin-s1": ("conv_small_fwd", [BF16], [], (2, 5, 9, 19), 3, 32, 3, 1, ("plain", "epilogue")),
    "direct": ("conv_direct", [BF16, F32], [F16], (2, 5, 6, 7), 5, 7, 3, 1, ("plain", "epilogue")),
}
FWD_PARAMS = [pytest.param(key, variant, dt, form, id=f"{key}-{variant}-{DT_NAME[dt]}-{form}")
              for key, c in FWD.items() for variant in c[8]
              for dt, form in [(dt, f) for dt in c[1] for f in FORMS] + [(dt, "right") for dt in c[2]]]


def out_sp(sp, k, s):
    return tuple((e + 2 * ((k - 1) // 2) - k) // s + 1 for e in sp)


@functools.lru_cache(maxsize=4)
def fwd_operands(key):
    _, _, _, (n, d, h, w), cin, cout, k, s, _ = FWD[key]
    seed = 1000 + 10 * sorted(FWD).index(key)
    x = rnd((n, cin, d, h, w), seed)
    wt = rnd((cout, cin, k, k, k), seed + 1, 1.0 / math.sqrt(cin * k ** 3))
    b = rnd((cout,), seed + 2, 0.1)
    r = rnd((n, cout) + out_sp((d, h, w), k, s), seed + 3)
    return x, wt, b, r


@functools.lru_cache(maxsize=6)
def fwd_reference(key, dtype, transformed, f32_weights):
    """float64 convolution of the operands the kernel reads, and its |operand| companion: once per family and type.
    The direct kernel reads the f32 weights as they are, the MFMA kernels (small-Cin included) round them."""
    x, wt, b, _ = fwd_operands(key)
    _, _, _, _, _, _, k, s, _ = FWD[key]
    xin = tf_input(key, dtype) if transformed else q(x, dtype)
    return lb.conv_ref(xin, wt if f32_weights else q(wt, dtype), b, stride=s, padding=(k - 1) // 2)


def tf_params(cin):
    return (1 + 0.3 * rnd((cin,), 77)), 0.2 * rnd((cin,), 78), torch.tensor([0.2])


@functools.lru_cache(maxsize=4)
def tf_input(key, dtype):
    """the input after the producer's BatchNorm-apply + PReLU as bn_act_fwd stores it: the fused transform equals it
    bit for bit (test_conv3d_input_transform_equals_separate_bn_pass)"""
    x = fwd_operands(key)[0]
    scale, shift, alpha = tf_params(x.shape[1])
    u = ndhwc(x).to(DEV, dtype)
    au = torch.empty_like(u)
    ops.bn_act_fwd(u, au, scale.to(DEV), shift.to(DEV), alpha.to(DEV))
    torch.cuda.synchronize()
    return ncdhw(au)


def check_stats(stats, rows, ref_raw, dtype, cout):
    """the workgroups' rows against the tolerances of test_conv3d_fwd; nothing behind the table"""
    assert guard_intact(stats, rows)
    real = stats[:rows - reserve_rows()]
    finite(real)
    cnt = ref_raw.numel() / cout
    ssum, ssq = real[:, 0].double().sum(0).cpu(), real[:, 1].double().sum(0).cpu()
    rs, rq = ref_raw.sum((0, 2, 3, 4)), (ref_raw ** 2).sum((0, 2, 3, 4))
    assert float((ssum - rs).abs().max()) / cnt < (1e-5 if dtype == F32 else 2e-2) * float(ref_raw.abs().max())
    assert float(((ssq - rq).abs() / rq).max()) < (1e-4 if dtype == F32 else 3e-2)


@pytest.mark.parametrize("key,variant,dtype,form", FWD_PARAMS)
def test_forward_convolution_stays_inside_its_views(key, variant, dtype, form):
    family, _, _, (n, d, h, w), cin, cout, k, s, _ = FWD[key]
    family = family.format(dt=DT_NAME[dtype])
    x, wt, b, r = fwd_operands(key)
    osp = out_sp((d, h, w), k, s)
    mfma = ops.mfma_ok(cin, cout)
    wd, bd = wt.to(DEV), b.to(DEV)
    packed = ops.wpack(dtype, 0, wd, cin, cout, k) if mfma else None
    alpha = torch.tensor([0.3], device=DEV) if variant == "epilogue" else None
    tf = tuple(t.to(DEV) for t in tf_params(cin)) if variant == "in_tf" else None
    with_stats = variant != "identity" and (mfma or variant == "plain")      # small-Cin / direct: before PReLU only

    def build(in_form, out_form):
        a = Arenas()
        xv = a.inp(x, dtype, in_form)
        rv = a.inp(r, dtype, in_form) if variant == "epilogue" else (xv if variant == "identity" else None)
        yv = a.out((n,) + osp + (cout,), dtype, out_form)
        return a, xv, rv, yv

    def launch(xv, rv, yv, stats):
        ops.conv3d_fwd(xv, yv, packed, wd, 0, bd, k, s, prelu_alpha=alpha, residual=rv, stats=stats, in_tf=tf)

    in_form = form
    if form == "odd" and mfma and h16(dtype):
        # 16-bit MFMA launchers need 16-byte aligned input rows: the odd input is refused, nothing is touched
        a, xv, rv, yv = build("odd", "odd")
        refuses(lambda: launch(xv, rv, yv, None), a)
        in_form = "right"
    a, xv, rv, yv = build(in_form, form)
    name = ops.conv3d_fwd_kernel_name(xv, yv, k, s)
    if key == "ring3" and form == "odd":
        family = f"conv_ring2_kernel<{DT_NAME[dtype]}, CK=16, NT=1>"       # output rows 8 bytes in: ring3 -> ring2
    assert family in name, name
    if variant == "in_tf":
        assert ops.conv3d_in_affine_ok(xv, yv, k, s)
    rows = ops.conv3d_stats_rows(xv, yv, k, s)
    stats = sentinel_table(rows, 2, cout) if with_stats else None
    launch(xv, rv, yv, stats)
    a.check()
    ref, absref = fwd_reference(key, dtype, variant == "in_tf", "conv_direct" in name)
    res = {"epilogue": q(r, dtype), "identity": q(x, dtype)}.get(variant)
    elem_bound(dtype, ncdhw(yv), *epilogue64(ref, absref, 0.3 if variant == "epilogue" else None, res))
    if with_stats:
        check_stats(stats, rows, ref, dtype, cout)


# ------------------------------------------------------------------------------------------ stride-1 input gradient
# key -> (substring of the kernel name, dy (n, d, h, w), channels of dy, channels of dx)
DGRAD = {
    "ring": ("conv_ring3", RING, 16, 16),
    "ring-32": ("conv_ring2_kernel<bf16, CK=32, NT=2>", RING, 32, 32),
    "ksplit": ("conv_fwd_ks", (2, 5, 6, 19), 64, 64),
    "tile": ("conv_fwd_mfma_kernel<bf16, CK=16, k3 s1>", (2, 5, 9, 19), 16, 16),
}


@functools.lru_cache(maxsize=2)
def dgrad_operands(key):
    _, (n, d, h, w), cdy, cdx = DGRAD[key]
    seed = 2000 + 10 * sorted(DGRAD).index(key)
    dy = rnd((n, cdy, d, h, w), seed, 0.5)
    wt = rnd((cdy, cdx, 3, 3, 3), seed + 1, 1.0 / math.sqrt(cdy * 27))
    xr = rnd((n, cdx, d, h, w), seed + 2, 2.0) + 0.3             # the input of the BatchNorm the gradient flows into
    return dy, wt, xr


@functools.lru_cache(maxsize=2)
def dgrad_reference(key, dtype):
    dy, wt, _ = dgrad_operands(key)
    return lb.convT_ref(q(dy, dtype), q(wt, dtype), stride=1, padding=1, output_padding=0)


DGRAD_PARAMS = [pytest.param(key, sums, form, id=f"{key}-{'bn-sums' if sums else 'plain'}-{form}")
                for key in DGRAD for sums in ((False, True) if key.startswith("ring") else (False,)) for form in FORMS]


@pytest.mark.parametrize("key,sums,form", DGRAD_PARAMS)
def test_stride1_input_gradient_stays_inside_its_views(key, sums, form, dtype=BF16):
    """pack kind 1 on the ring, k-split and tile families; on the ring also with the BatchNorm-backward sums of the
    layer the gradient flows into (MODE 4), finalised in the launch, whose second input x is a poisoned slice too"""
    family, (n, d, h, w), cdy, cdx = DGRAD[key]
    dy, wt, xr = dgrad_operands(key)
    wd = wt.to(DEV)
    packed = ops.wpack(dtype, 1, wd, cdy, cdx, 3)
    c = cdx
    mean, invstd = (rnd((c,), 527) * 0.3).to(DEV), (rnd((c,), 528).abs() + 0.5).to(DEV)
    gamma, beta = (rnd((c,), 529) + 1.5).to(DEV), (rnd((c,), 530) * 0.3).to(DEV)
    count = n * d * h * w

    def build(in_form, out_form):
        a = Arenas()
        dyv = a.inp(dy, dtype, in_form)
        xv = a.inp(xr, dtype, in_form) if sums else None
        dxv = a.out((n, d, h, w, cdx), dtype, out_form)
        return a, dyv, xv, dxv

    def launch(dyv, xv, dxv, part, fin):
        ops.conv3d_fwd(dyv, dxv, packed, None, 1, None, 3, 1,
                       bn_bwd=(xv, mean, invstd, gamma, beta, None, part) if sums else None,
                       bn_bwd_fin=fin if sums else None)

    def outs():
        return [torch.full((c,), float("nan"), device=DEV), torch.full((c,), float("nan"), device=DEV),
                torch.full((2, c), float("nan"), device=DEV)]

    if form == "odd":
        a, dyv, xv, dxv = build("odd", "odd")
        dg, db, coef = outs()
        part = sentinel_table(ops.conv3d_stats_rows(dyv, dxv, 3, 1), 3, c) if sums else None
        refuses(lambda: launch(dyv, xv, dxv, part, (count, dg, db, None, coef)), a)
        if sums:
            assert guard_intact(part, 0)           # not a row of the table was written
    a, dyv, xv, dxv = build("right" if form == "odd" else form, form)
    name = ops.conv3d_fwd_kernel_name(dyv, dxv, 3, 1)
    if key == "ring" and form == "odd":
        family = "conv_ring2_kernel<bf16, CK=16, NT=1>"
    assert family in name, name
    rows = ops.conv3d_stats_rows(dyv, dxv, 3, 1)
    part = sentinel_table(rows, 3, c) if sums else None
    dg, db, coef = outs()
    if sums:
        assert ops.conv3d_bn_bwd_sums_ok(dyv, dxv, 3, 1)
    launch(dyv, xv, dxv, part, (count, dg, db, None, coef))
    a.check()
    got = ncdhw(dxv)
    elem_bound(dtype, got, *dgrad_reference(key, dtype))
    if sums:
        assert guard_intact(part, rows)
        finite(part[:rows - reserve_rows()], dg, db, coef)
        # the sums of the stored gradient, within the bound of test_conv_ring3_dma_ring_ragged_and_segmented_shapes
        gq = got.double()
        xhat = (q(xr, dtype).double() - mean.cpu().double().view(1, -1, 1, 1, 1)) * invstd.cpu().double().view(1, -1, 1, 1, 1)
        for have, want, what in ((dg, (gq * xhat).sum((0, 2, 3, 4)), "dgamma"), (db, gq.sum((0, 2, 3, 4)), "dbeta")):
            assert float((have.cpu().double() - want).abs().max()) < \
                2e-4 * float(want.abs().max()) + 1e-3 * float(want.abs().mean()), what


# ------------------------------------------------------------------- the engine's concat layout: pair and split_act
def concat_out(a, shape_ndhw, c, dtype, form):
    """both outputs as the halves of one 2c-channel view of one arena"""
    both = a.out(tuple(shape_ndhw) + (2 * c,), dtype, form)
    return both, both[..., :c], both[..., c:]


PAIR_CASES = [(1, 16, 2, (9, 17, 35)), (2, 32, 1, (5, 9, 19))]


@pytest.mark.parametrize("dtype,form", all_forms([BF16, F32], [F16]))
@pytest.mark.parametrize("cin,cout,stride,sp", PAIR_CASES, ids=["1to16-s2", "2to32-s1"])
def test_first_layer_pair_stays_inside_the_concat_arena(cin, cout, stride, sp, dtype, form):
    """conv3d_fwd_pair: the subunit-0 and the residual convolution of the first ResidualUnit write the two halves of one
    concat row; against float64 and, bit for bit, against two conv3d_fwd launches on tensors of their own"""
    n = 2
    x = rnd((n, cin) + sp, 301)
    wa, wb = rnd((cout, cin, 3, 3, 3), 302, 0.3), rnd((cout, cin, 3, 3, 3), 303, 0.3)
    ba, bb = rnd((cout,), 304, 0.1), rnd((cout,), 305, 0.1)
    osp = out_sp(sp, 3, stride)
    wad, wbd, bad, bbd = wa.to(DEV), wb.to(DEV), ba.to(DEV), bb.to(DEV)
    a = Arenas()
    xv = a.inp(x, dtype, form)
    both, ya, yb = concat_out(a, (n,) + osp, cout, dtype, form)
    assert ops.conv3d_pair_ok(xv, ya, yb)
    name = ops.conv3d_fwd_kernel_name(xv, ya, 3, stride)
    assert "conv_small_fwd" in name
    rows = ops.conv3d_stats_rows(xv, ya, 3, stride)
    stats = sentinel_table(rows, 2, cout)
    ops.conv3d_fwd_pair(xv, ya, wad, bad, yb, wbd, bbd, stride, stats_a=stats)
    a.check()
    ref_a = lb.conv_ref(q(x, dtype), q(wa, dtype), ba, stride=stride, padding=1)
    elem_bound(dtype, ncdhw(ya), *ref_a, what="a")
    elem_bound(dtype, ncdhw(yb), *lb.conv_ref(q(x, dtype), q(wb, dtype), bb, stride=stride, padding=1), what="b")
    check_stats(stats, rows, ref_a[0], dtype, cout)
    xd = xv.contiguous()
    da, db_ = (torch.empty((n,) + osp + (cout,), dtype=dtype, device=DEV) for _ in range(2))
    ops.conv3d_fwd(xd, da, None, wad, 0, bad, 3, stride)
    ops.conv3d_fwd(xd, db_, None, wbd, 0, bbd, 3, stride)
    torch.cuda.synchronize()
    assert torch.equal(ya, da) and torch.equal(yb, db_)


@pytest.mark.parametrize("mode", ["training", "inference"])
@pytest.mark.parametrize("dtype,form", all_forms([BF16], [F16]))
def test_split_act_pair_stays_inside_the_concat_arena(dtype, form, mode):
    """conv3d_fwd_split_act (tile kernel, k3 s2): one launch over the concatenated pack writes [first subunit | residual
    convolution]; training takes the statistics of the first half, inference applies PReLU to it"""
    n, cin, c, sp = 2, 16, 32, (9, 10, 35)
    x = rnd((n, cin) + sp, 41)
    wa, wb = (rnd((c, cin, 3, 3, 3), s_, 1.0 / math.sqrt(cin * 27)) for s_ in (42, 43))
    ba, bb = rnd((c,), 44, 0.1), rnd((c,), 45, 0.1)
    osp = out_sp(sp, 3, 2)
    wcat, bcat = torch.cat([wa, wb], 0).contiguous(), torch.cat([ba, bb]).contiguous()
    pack = ops.wpack(dtype, 0, wcat.to(DEV), cin, 2 * c, 3)
    alpha = torch.tensor([0.3], device=DEV) if mode == "inference" else None

    def build(in_form):
        a = Arenas()
        xv = a.inp(x, dtype, in_form)
        return (a, xv) + concat_out(a, (n,) + osp, c, dtype, form)

    def launch(xv, both, stats):
        if mode == "training":
            ops.conv3d_fwd_split_act(xv, both, pack, ba.to(DEV), None, c, 3, 2, bias_b=bb.to(DEV), stats=stats)
        else:
            ops.conv3d_fwd_split_act(xv, both, pack, bcat.to(DEV), alpha, c, 3, 2)

    if form == "odd":
        a, xv, both, _, _ = build("odd")
        refuses(lambda: launch(xv, both, None), a)
    a, xv, both, ya, yb = build("right" if form == "odd" else form)
    assert ops.conv3d_split_act_ok(xv, both, 3, 2)
    name = ops.conv3d_fwd_kernel_name(xv, both, 3, 2)
    assert f"conv_fwd_mfma_kernel<{DT_NAME[dtype]}, CK=16, k3 s2>" in name
    rows = ops.conv3d_stats_rows(xv, both, 3, 2)
    stats = sentinel_table(rows, 2, c) if mode == "training" else None
    launch(xv, both, stats)
    a.check()
    ref, absref = lb.conv_ref(q(x, dtype), q(wcat, dtype), bcat, stride=2, padding=1)
    elem_bound(dtype, ncdhw(ya), *epilogue64(ref[:, :c], absref[:, :c], 0.3 if mode == "inference" else None), what="a")
    elem_bound(dtype, ncdhw(yb), ref[:, c:], absref[:, c:], what="b")
    if stats is not None:
        check_stats(stats, rows, ref[:, :c], dtype, c)


# ------------------------------------------------------------------------------------------ transposed convolution
def convt_family(dtype, cin, cout, w_in):
    """the choice conv_plan.h's convt_plan makes (there is no name query for the transposed layer)"""
    if not ops.mfma_ok(cin, cout):
        return "direct"
    psck = 16 if dtype == F32 else 32
    nch, ntiles = cin // psck, cout // 16
    ps = cin % psck == 0 and w_in >= 16 and ((ntiles == 1 and nch <= 2) or (ntiles == 2 and nch == 1 and h16(dtype)))
    return "persistent" if ps else "tile"


def convt_rows(family, n, sp):
    """statistics rows of an MFMA family's grid for a layer of fewer than 1024 tiles"""
    d, h, w = sp
    td, th, tw = (2, 2, 16) if family == "persistent" or w > 8 else (2, 4, 8)
    return n * -(-d // td) * -(-h // th) * -(-w // tw) + reserve_rows()


# key -> (family, types in four forms, types as a right slice, input (d, h, w), cin, cout)
CONVT = {
    "persistent": ("persistent", [BF16], [F16], (3, 5, 17), 32, 16),
    "persistent-2-tiles": ("persistent", [BF16], [], (3, 5, 17), 32, 32),
    "tile": ("tile", [BF16], [F16], (3, 5, 7), 32, 16),
    "direct": ("direct", [BF16, F32], [F16], (3, 5, 6), 8, 4),
}
CONVT_PARAMS = [pytest.param(key, odd, dt, form, id=f"{key}-{'odd' if odd else 'even'}-extent-{DT_NAME[dt]}-{form}")
                for key, c in CONVT.items() for odd in (0, 1)
                for dt, form in [(dt, f) for dt in c[1] for f in FORMS] + [(dt, "right") for dt in c[2]]]


@pytest.mark.parametrize("key,odd,dtype,form", CONVT_PARAMS)
def test_transposed_convolution_stays_inside_its_views(key, odd, dtype, form):
    """even (2 * in) and odd (2 * in - 1) output extents; plain with fused statistics, then PReLU + residual"""
    family, _, _, sp, cin, cout = CONVT[key]
    n = 2
    assert convt_family(dtype, cin, cout, sp[2]) == family
    seed = 3000 + 10 * sorted(CONVT).index(key)
    x = rnd((n, cin) + sp, seed)
    wt = rnd((cin, cout, 3, 3, 3), seed + 1, 1.0 / math.sqrt(cin * 27 / 8))
    b = rnd((cout,), seed + 2, 0.1)
    osp = tuple(2 * e - odd for e in sp)
    r = rnd((n, cout) + osp, seed + 3)
    mfma = ops.mfma_ok(cin, cout)
    wd, bd = wt.to(DEV), b.to(DEV)
    packed = ops.wpack(dtype, 2, wd, cin, cout, 3) if mfma else None
    alpha = torch.tensor([0.2], device=DEV)
    ref, absref = lb.convT_ref(q(x, dtype), q(wt, dtype) if mfma else wt, b, output_padding=0 if odd else 1)

    def build(in_form, with_res):
        a = Arenas()
        xv = a.inp(x, dtype, in_form)
        rv = a.inp(r, dtype, in_form) if with_res else None
        return a, xv, rv, a.out((n,) + osp + (cout,), dtype, form)

    in_form = form
    if form == "odd" and mfma and h16(dtype):
        a, xv, rv, yv = build("odd", True)
        refuses(lambda: ops.convT3d_fwd(xv, yv, packed, wd, bd, prelu_alpha=alpha, residual=rv), a)
        in_form = "right"
    # plain, with the fused statistics
    a, xv, _, yv = build(in_form, False)
    rows = ops.convT3d_stats_rows(xv, yv)
    if family != "direct":
        assert rows == convt_rows(family, n, sp)
    stats = sentinel_table(rows, 2, cout)
    ops.convT3d_fwd(xv, yv, packed, wd, bd, stats=stats)
    a.check()
    elem_bound(dtype, ncdhw(yv), ref, absref)
    assert guard_intact(stats, rows)
    real = stats[:rows - reserve_rows()]
    finite(real)
    ssum = real[:, 0].double().sum(0).cpu()
    assert float((ssum - ref.sum((0, 2, 3, 4))).abs().max()) / (ref.numel() / cout) < \
        (1e-5 if dtype == F32 else 2e-2) * float(ref.abs().max())               # the tolerance of test_convT3d_fwd
    # PReLU + residual: the form the input gradient of a stride-2 convolution uses
    a, xv, rv, yv = build(in_form, True)
    ops.convT3d_fwd(xv, yv, packed, wd, bd, prelu_alpha=alpha, residual=rv)
    a.check()
    elem_bound(dtype, ncdhw(yv), *epilogue64(ref, absref, 0.2, q(r, dtype)), what="epilogue")


# ------------------------------------------------------------- BatchNorm-backward apply inside the stride-2 convolution
@pytest.mark.parametrize("dtype,form", all_forms([BF16], [F16]))
def test_bn_backward_stride2_convolution_stays_inside_its_views(dtype, form):
    """bn_act_bwd_apply_conv reads dy and x, writes dx and the stride-2 convolution of dx: all four are slices.  The
    same bits as bn_act_bwd_apply followed by conv3d_fwd on tensors of their own (the comparison of
    test_bn_backward_apply_inside_the_stride2_convolution_equals_the_two_calls)."""
    n, c, cout, sp = 2, 16, 32, (5, 9, 35)
    x, dy = rnd((n, c) + sp, 71, 2.0), rnd((n, c) + sp, 72)
    mean, invstd = (rnd((c,), 73) * 0.5).to(DEV), (rnd((c,), 74).abs() + 0.5).to(DEV)
    gamma, beta = (rnd((c,), 75) + 1.5).to(DEV), (rnd((c,), 76) * 0.3).to(DEV)
    alpha = torch.full((1,), 0.25, device=DEV)
    coef = (rnd((2, c), 77) * 0.1).to(DEV).contiguous()
    w = (rnd((cout, c, 3, 3, 3), 78) * 0.1).to(DEV)
    pack = ops.wpack(dtype, 0, w, c, cout, 3)
    osp = out_sp(sp, 3, 2)

    def build(in_form, dx_form, out_form):
        a = Arenas()
        return (a, a.inp(dy, dtype, in_form), a.inp(x, dtype, in_form), a.out((n,) + sp + (c,), dtype, dx_form),
                a.out((n,) + osp + (cout,), dtype, out_form))

    def launch(dyv, xv, dxv, ov):
        ops.bn_act_bwd_apply_conv(dyv, xv, dxv, mean, invstd, gamma, beta, alpha, coef, ov, pack)

    dx_form = form
    if form == "odd":
        # dy, x and dx are staged and stored in 16-byte pieces: rows 8 bytes in are refused; the convolution's output
        # needs 8-byte aligned rows only
        for forms in (("odd", "odd", "odd"), ("right", "odd", "odd"), ("odd", "right", "odd")):
            a, dyv, xv, dxv, ov = build(*forms)
            assert not ops.bn_act_bwd_apply_conv_ok(dyv, xv, dxv, ov)
            refuses(lambda: launch(dyv, xv, dxv, ov), a)
        dx_form = "right"
    a, dyv, xv, dxv, ov = build("right" if form == "odd" else form, dx_form, form)
    assert ops.bn_act_bwd_apply_conv_ok(dyv, xv, dxv, ov)
    launch(dyv, xv, dxv, ov)
    a.check()
    dyd, xd = dyv.contiguous(), xv.contiguous()
    dx0 = torch.empty_like(xd)
    out0 = torch.empty((n,) + osp + (cout,), dtype=dtype, device=DEV)
    ops.bn_act_bwd_apply(dyd, xd, dx0, mean, invstd, gamma, beta, alpha, coef)
    ops.conv3d_fwd(dx0, out0, pack, w, 0, None, 3, 2)
    torch.cuda.synchronize()
    assert torch.equal(va.bits(dxv), va.bits(dx0)) and torch.equal(va.bits(ov), va.bits(out0))
    bn_bwd_bound(dtype, ncdhw(dxv), q(dy, dtype), q(x, dtype), mean.cpu(), invstd.cpu(), gamma.cpu(), beta.cpu(), 0.25,
                 coef.cpu())
    elem_bound(dtype, ncdhw(ov), *lb.conv_ref(ncdhw(dxv), q(w.cpu(), dtype), stride=2, padding=1), what="conv")


# --------------------------------------------------------------------------------- the fused full-resolution decoder
@pytest.mark.parametrize("dtype,form", all_forms([BF16], [F16]))
def test_fused_decoder_top_stays_inside_its_views(dtype, form):
    """dectop_fwd: ConvTranspose3d(32 -> 16) + folded BatchNorm + PReLU, then conv(16 -> 16) + identity residual in one
    launch; the same bits as the two launches on tensors of their own.  The launcher takes whole 4 x 16 x 16 output
    tiles only, so the extents are several tiles, not ragged."""
    n, d, h, w = 2, 6, 8, 24
    x = rnd((n, 32, d, h, w), 501)
    wt, wc = rnd((32, 16, 3, 3, 3), 502, 0.06).to(DEV), rnd((16, 16, 3, 3, 3), 503, 0.08).to(DEV)
    scale, ub, cb = (rnd((16,), 504).abs() + 0.5).to(DEV), (rnd((16,), 505) * 0.2).to(DEV), (rnd((16,), 506) * 0.2).to(DEV)
    alpha = torch.full((1,), 0.25, device=DEV)
    fine = (n, 2 * d, 2 * h, 2 * w, 16)
    frag, cv_pack = ops.dectop_up_frag(wt, scale, dtype=dtype), ops.wpack(dtype, 0, wc, 16, 16, 3)

    def build(in_form):
        a = Arenas()
        return a, a.inp(x, dtype, in_form), a.out(fine, dtype, form)

    if form == "odd":
        a, xv, ov = build("odd")
        assert not ops.dectop_ok(xv, ov)
        refuses(lambda: ops.dectop_fwd(xv, ov, frag, ub, alpha, cv_pack, cb, alpha_in_unit_range=True), a)
    a, xv, ov = build("right" if form == "odd" else form)
    assert ops.dectop_ok(xv, ov)
    ops.dectop_fwd(xv, ov, frag, ub, alpha, cv_pack, cb, alpha_in_unit_range=True)
    a.check()
    hmid = torch.empty(fine, dtype=dtype, device=DEV)
    ops.convT3d_fwd(xv.contiguous(), hmid, ops.wpack(dtype, 2, wt, 32, 16, 3, scale=scale), None, ub, prelu_alpha=alpha)
    want = torch.empty_like(hmid)
    ops.conv3d_fwd(hmid, want, cv_pack, None, 0, cb, 3, 1, residual=hmid)
    torch.cuda.synchronize()
    assert torch.equal(va.bits(ov), va.bits(want))
    hq = ncdhw(hmid)
    elem_bound(dtype, ncdhw(ov), *epilogue64(*lb.conv_ref(hq, q(wc.cpu(), dtype), cb.cpu()), None, hq))


# ------------------------------------------------------------------------------------------------ weight gradient
def cdiv(a, b):
    return -(-a // b)


def wgrad_plan(dtype, x, dy, k, s, cus):
    """(path, slabs) as conv_plan.h's wgrad_plan decides them, from the views' fields: the workspace query reports
    the slabs, and the cases below hold it to this"""
    es = x.element_size()
    cin, cout = x.shape[4], dy.shape[4]
    n, d, h, w = dy.shape[:4]
    wide = w > 8

    def aligned(t):
        return t.stride(3) % (16 // es) == 0 and t.data_ptr() % 16 == 0

    def tiles(t):
        return n * cdiv(d, t[0]) * cdiv(h, t[1]) * cdiv(w, t[2])

    cu = ops.wgrad_cus(cus)
    if cin % 16 == 0 and cout % 16 == 0 and aligned(x) and aligned(dy):
        two = h16(dtype) and cout % 32 == 0              # 2 x 1 channel blocking
        chunks = (cin // 16) * (cout // (32 if two else 16))
        if s == 2:
            t3 = (2, 4, 16) if wide else (2, 8, 8)
        else:
            t3 = ((2 if two else 4), 8, 16) if wide else (4, 8, 8)
        if h16(dtype) and k == 3:
            gx = cu // chunks // 8 * 8
            if gx >= 8 and tiles(t3) >= 4 * gx:
                return "wave-specialised", gx
        want = (cu if two else 2 * cu) // chunks
        return "mfma", max(1, min(want, tiles(t3)))
    if k == 3 and 1 <= cin <= 4 and cout in (16, 32) and aligned(dy):
        return "small-cin", min(tiles((2, 8, 16)), 1024)
    return "direct", min(cdiv(n * d * h * w, 512), 1024)


# key -> (path, types in four forms, types as a right slice, cin, cout, s, x (n, d, h, w), with the input transform too)
WGRAD = {
    "wave-specialised-s1": ("wave-specialised", [BF16], [F16], 32, 16, 1, (2, 13, 61, 125), True),
    "wave-specialised-s2": ("wave-specialised", [BF16], [F16], 32, 16, 2, (2, 25, 61, 157), True),
    "mfma-16bit": ("mfma", [BF16], [F16], 16, 16, 1, (2, 5, 9, 19), True),
    "mfma-f32": ("mfma", [F32], [], 32, 32, 1, (2, 5, 9, 19), False),
    "small-cin": ("small-cin", [BF16, F32], [F16], 1, 16, 2, (2, 9, 17, 35), False),
    "direct": ("direct", [BF16, F32], [F16], 5, 7, 1, (2, 5, 6, 7), False),
}
WGRAD_PARAMS = [pytest.param(key, dt, form, id=f"{key}-{DT_NAME[dt]}-{form}") for key, c in WGRAD.items()
                for dt, form in [(dt, f) for dt in c[1] for f in FORMS] + [(dt, "right") for dt in c[2]]]


@functools.lru_cache(maxsize=2)
def wgrad_operands(key):
    _, _, _, cin, cout, s, (n, d, h, w), _ = WGRAD[key]
    seed = 4000 + 10 * sorted(WGRAD).index(key)
    return rnd((n, cin, d, h, w), seed), rnd((n, cout) + out_sp((d, h, w), 3, s), seed + 1)


_WGRAD_REF = {}


def wgrad_reference(key, dtype, transformed, x):
    """what wgrad_bound compares with (lb.wgrad_ref on the operands the kernel reads), once per case and type"""
    if (key, dtype, transformed) not in _WGRAD_REF:
        if len(_WGRAD_REF) >= 4:
            _WGRAD_REF.clear()
        _WGRAD_REF[key, dtype, transformed] = lb.wgrad_ref(q(x, dtype), q(wgrad_operands(key)[1], dtype), 3, WGRAD[key][5])
    return _WGRAD_REF[key, dtype, transformed]


def sentinel_f32(numel):
    """an f32 buffer of `numel` elements with a sentinel tail, all of it sentinel before the launch"""
    t = torch.empty(numel + 64, device=DEV)
    t.view(torch.int32).fill_(SENTINEL)
    return t


@pytest.mark.parametrize("key,dtype,form", WGRAD_PARAMS)
def test_weight_gradient_stays_inside_its_views(key, dtype, form):
    """x and dy are poisoned slices of the same form; dw / db f32 buffers with a sentinel tail; the slab workspace with
    the guard of test_conv_plan_gpu; at cus 0 and 64, without and (where the path takes it) with the input transform.
    A 16-bit odd slice (rows 8 bytes in) moves an MFMA layer to the direct kernel, which takes no transform."""
    path, _, _, cin, cout, s, (n, d, h, w), with_tf = WGRAD[key]
    x, dy = wgrad_operands(key)
    a = Arenas()
    xv, dyv = a.inp(x, dtype, form), a.inp(dy, dtype, form)
    moved = form == "odd" and h16(dtype) and path != "direct"
    nout = cin * cout * 27
    tf = ((rnd((cin,), 333).abs() + 0.5).to(DEV), (rnd((cin,), 334) * 0.3).to(DEV), torch.full((1,), 0.25, device=DEV))
    x_tf = None
    for cus in (0, 64):
        want_path, slabs = wgrad_plan(dtype, xv, dyv, 3, s, cus)
        assert want_path == ("direct" if moved else path)
        nbytes = ops.conv3d_wgrad_workspace(xv, dyv, 3, s, cus)
        # the slabs are the first block of the workspace; what follows does not depend on the budget
        other = wgrad_plan(dtype, xv, dyv, 3, s, 8)[1]
        a256 = lambda v: (v + 255) // 256 * 256
        assert nbytes - ops.conv3d_wgrad_workspace(xv, dyv, 3, s, 8) == a256(slabs * nout * 4) - a256(other * nout * 4)
        for in_tf in ((None, tf) if with_tf else (None,)):
            ws = torch.empty(nbytes + GUARD_BYTES, dtype=torch.uint8, device=DEV)
            ws[nbytes:].view(torch.int32).fill_(SENTINEL)
            dw, db = sentinel_f32(nout), sentinel_f32(cout)

            def launch():
                ops.conv3d_wgrad(xv, dyv, dw[:nout].view(cout, cin, 3, 3, 3), db[:cout], 3, s, ws, in_tf=in_tf, cus=cus)

            if in_tf is not None and moved:
                refuses(launch, a)
                assert guard_intact(dw, 0) and guard_intact(db, 0)
                continue
            launch()
            a.check()
            assert bool((ws[nbytes:].view(torch.int32) == SENTINEL).all())
            assert guard_intact(dw, nout) and guard_intact(db, cout)
            finite(dw[:nout], db[:cout])
            xin = x
            if in_tf is not None:
                if x_tf is None:                 # the producer's BatchNorm-apply + PReLU as bn_act_fwd stores it
                    xd = xv.contiguous()
                    xn = torch.empty_like(xd)
                    ops.bn_act_fwd(xd, xn, *tf)
                    torch.cuda.synchronize()
                    x_tf = ncdhw(xn)
                xin = x_tf
            dw_ref, a_dw, db_ref, a_db = wgrad_reference(key, dtype, in_tf is not None, xin)
            elem_bound(dtype, dw[:nout].view(cout, cin, 3, 3, 3).cpu(), dw_ref, a_dw, what=f"dw cus={cus}", rounded=False)
            elem_bound(dtype, db[:cout].cpu(), db_ref, a_db, what=f"db cus={cus}", rounded=False)


# ------------------------------------------------------------------- element-wise and reduction passes over views
EW_SHAPE = (2, 3, 5, 7)          # 210 voxels: 12 channels = 2520 elements on the 4-element path, 3 channels = 630 scalar
EW_PARAMS = [pytest.param(c, dt, form, id=f"c{c}-{DT_NAME[dt]}-{form}") for c in (12, 3) for dt in (BF16, F16, F32)
             for form in FORMS]


def ew_operands(c, dtype, form):
    n, d, h, w = EW_SHAPE
    x, res, dy = rnd((n, c, d, h, w), 51, 2.0), rnd((n, c, d, h, w), 54), rnd((n, c, d, h, w), 55)
    a = Arenas()
    return a, x, res, dy, a.inp(x, dtype, form), a.inp(res, dtype, form), a.inp(dy, dtype, form)


@pytest.mark.parametrize("c,dtype,form", EW_PARAMS)
def test_batchnorm_forward_passes_stay_inside_their_views(c, dtype, form):
    """bn_stats and bn_act_fwd (residual; dropout) read and write slices; the element counts are no multiple of 256"""
    n, d, h, w = EW_SHAPE
    a, x, res, _, xv, rv, _ = ew_operands(c, dtype, form)
    count = n * d * h * w
    rows = ops.bn_stats_rows(xv)
    part = sentinel_table(rows, 2, c)
    ops.bn_stats(xv, part)
    gamma, beta, alpha = (1 + 0.2 * rnd((c,), 52)).to(DEV), (0.1 * rnd((c,), 53)).to(DEV), torch.tensor([0.25], device=DEV)
    mean, invstd, scale, shift = (torch.full((c,), float("nan"), device=DEV) for _ in range(4))
    run_m, run_v = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    ops.bn_finalize(part, rows, c, count, gamma, beta, run_m, run_v, 0.1, 1e-5, mean, invstd, scale, shift)
    a.check()
    assert guard_intact(part, rows)
    finite(mean, invstd, scale, shift, run_m, run_v)
    xq = q(x, dtype).double()
    want_rm, want_rv = 0.1 * xq.mean((0, 2, 3, 4)), 0.9 + 0.1 * xq.var((0, 2, 3, 4), unbiased=True)
    # the running statistics within the 1e-5 of test_bn_prelu_fwd_bwd
    assert relerr64(run_m.cpu().double(), want_rm) < 1e-5 and relerr64(run_v.cpu().double(), want_rv) < 1e-5
    for with_res, drop in ((True, (0.0, 0)), (False, (0.3, 0xC0FFEE))):
        yv = a.out((n, d, h, w, c), dtype, form)
        ops.bn_act_fwd(xv, yv, scale, shift, alpha, rv if with_res else None, dropout=drop)
        a.check()
        mask = None
        if drop[0]:
            mask = torch.from_numpy(drop_mask(count * c, *drop)).reshape(n, d, h, w, c).permute(0, 4, 1, 2, 3)
        elem_bound(dtype, ncdhw(yv), *bn_fwd_ref64(q(x, dtype), scale.cpu(), shift.cpu(), 0.25,
                                                   q(res, dtype) if with_res else None, mask), what="y")


@pytest.mark.parametrize("c,dtype,form", EW_PARAMS)
def test_batchnorm_backward_passes_stay_inside_their_views(c, dtype, form):
    """bn_act_bwd_reduce, bn_act_bwd_apply and the one-launch bn_act_bwd_fused"""
    n, d, h, w = EW_SHAPE
    a, x, _, dy, xv, _, dyv = ew_operands(c, dtype, form)
    count = n * d * h * w
    mean, invstd = (rnd((c,), 63) * 0.5).to(DEV), (rnd((c,), 64).abs() + 0.5).to(DEV)
    gamma, beta = (rnd((c,), 65) + 1.5).to(DEV), (rnd((c,), 66) * 0.3).to(DEV)
    alpha = torch.full((1,), 0.25, device=DEV)

    def outs():
        return [torch.full(s_, float("nan"), device=DEV) for s_ in ((c,), (c,), (1,), (2, c))]

    rows = ops.bn_act_bwd_rows(xv)
    part = sentinel_table(rows, 3, c)
    dg, db, da, coef = outs()
    ops.bn_act_bwd_reduce(dyv, xv, mean, invstd, gamma, beta, alpha, part)
    ops.bn_act_bwd_finalize(part, rows, c, count, gamma, invstd, dg, db, da, coef)
    dxv = a.out((n, d, h, w, c), dtype, form)
    ops.bn_act_bwd_apply(dyv, xv, dxv, mean, invstd, gamma, beta, alpha, coef)
    a.check()
    assert guard_intact(part, rows)
    finite(dg, db, da, coef)
    args = (q(dy, dtype), q(x, dtype), mean.cpu(), invstd.cpu(), gamma.cpu(), beta.cpu(), 0.25)
    bn_bwd_bound(dtype, ncdhw(dxv), *args, coef.cpu())
    # the sums against float64 on the operands, as test_bn_prelu_fwd_bwd holds them (1e-4 of the largest)
    v = lambda t: t.cpu().double().view(1, -1, 1, 1, 1)
    xh = (q(x, dtype).double() - v(mean)) * v(invstd)
    z = xh * v(gamma) + v(beta)
    dz = torch.where(z > 0, q(dy, dtype).double(), 0.25 * q(dy, dtype).double())
    for have, want in ((dg, (dz * xh).sum((0, 2, 3, 4))), (db, dz.sum((0, 2, 3, 4)))):
        assert float((have.cpu().double() - want).abs().max()) < 1e-4 * float(want.abs().max())
    # one launch (4-channel rows only)
    dx2 = a.out((n, d, h, w, c), dtype, form)
    if not ops.bn_act_bwd_fused_ok(dyv, xv, dx2):
        assert c % 4 != 0                          # the one-launch form takes 4-element aligned rows only
        part2 = sentinel_table(4, 3, c)
        f = outs()
        with pytest.raises(REFUSED):
            ops.bn_act_bwd_fused(dyv, xv, dx2, mean, invstd, gamma, beta, alpha, part2, (count, f[0], f[1], f[2], f[3]))
        torch.cuda.synchronize()
        assert va.untouched(a.outs[-1][0]) and guard_intact(part2, 0)
        a.outs.pop()
        a.check()
        return
    rows2 = ops.bn_act_bwd_fused_rows(xv)
    part2 = sentinel_table(rows2, 3, c)
    f = outs()
    ops.bn_act_bwd_fused(dyv, xv, dx2, mean, invstd, gamma, beta, alpha, part2, (count, f[0], f[1], f[2], f[3]))
    a.check()
    assert ops.fused_timeouts() == 0
    assert guard_intact(part2, rows2)
    finite(*f)
    bn_bwd_bound(dtype, ncdhw(dx2), *args, f[3].cpu(), what="dx (one launch)")
    for one, three in zip(f, (dg, db, da, coef)):          # the bound of test_bn_backward_as_one_launch_matches_the_three_calls
        assert float((one - three).abs().max()) <= 2e-6 * float(three.abs().max()) + 1e-7


@pytest.mark.parametrize("c,dtype,form", EW_PARAMS)
def test_add_and_cast_copy_stay_inside_their_views(c, dtype, form):
    n, d, h, w = EW_SHAPE
    a, x, res, _, xv, rv, _ = ew_operands(c, dtype, form)
    sv = a.out((n, d, h, w, c), dtype, form)
    ops.add(xv, rv, sv)
    a.check()
    want = q(x, dtype).double() + q(res, dtype).double()
    elem_bound(dtype, ncdhw(sv), want, q(x, dtype).double().abs() + q(res, dtype).double().abs(), what="add")
    for other in (dtype, F32) if dtype != F32 else (BF16, F16, F32):          # a pair is the same type or has f32 in it
        cv = a.out((n, d, h, w, c), other, form)
        ops.cast_copy(xv, cv)
        a.check()
        assert torch.equal(cv, xv.to(other)), f"cast_copy {DT_NAME[dtype]} -> {DT_NAME[other]}"      # one rounding: exact


# ------------------------------------------------------------------------------------------------ loss and labels
LOSS_N, LOSS_SP, KPAD = 2, (17, 24, 33), 16          # one full 8192-voxel chunk and a ragged one per sample
LOSSES = ("dice", "dice_ce", "tversky", "dice_focal")
TV_ALPHA, TV_BETA = float(torch.tensor(0.3)), float(torch.tensor(0.7))          # the f32 values the kernel reads
GRAD_SCALE = {F32: 1.0, BF16: 1.0, F16: 2.0 ** 10}   # fp16 gradients of a mean are subnormal unscaled (test_imbalance_loss_gpu)


@functools.lru_cache(maxsize=None)
def loss_inputs(k):
    lg = rnd((LOSS_N, k) + LOSS_SP, 61 + k, 3.0)
    lab = torch.randint(0, k, (LOSS_N, 1) + LOSS_SP, generator=torch.Generator().manual_seed(62 + k)).float()
    return lg, lab


@functools.lru_cache(maxsize=None)
def loss_truth(loss, k, dtype):
    from oracle.unet_ref import ref_dice_loss
    lg, lab = loss_inputs(k)
    lq = lg.to(dtype).double().requires_grad_(True)
    fn = {"dice": ref_dice_loss, "dice_ce": ref_dice_ce_loss, "dice_focal": ref_dice_focal_loss,
          "tversky": functools.partial(ref_tversky_loss, alpha=TV_ALPHA, beta=TV_BETA)}[loss]
    v = fn(lq, lab)
    v.backward()
    return float(v.detach()), lq.grad.detach()


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("loss", LOSSES)
def test_loss_reads_and_writes_the_real_classes_of_a_padded_row(loss, k, dtype):
    """logits[..., :k] of a kpad = 16 row whose padding classes are poisoned, dlogits written through the same kind of
    slice.  The engine zeroes the padded gradient tensor once and relies on the loss kernels never writing the
    padding (UNetEngine.dlogits_buffer): the padding classes of dlogits must keep the poison bits.  Default parameters;
    the gates of tests/test_loss_gpu.py and tests/test_imbalance_loss_gpu.py."""
    lg, lab = loss_inputs(k)
    want, grad = loss_truth(loss, k, dtype)
    gs = GRAD_SCALE[dtype]
    grad = grad * gs
    a = Arenas()
    t = ndhwc(lg).to(DEV, dtype)
    rows, lv = va.arena(tuple(t.shape), dtype, KPAD, 0, device=DEV)
    va.fill_view(lv, t)
    a.ins.append((rows, lv, t))
    drows, dv = va.arena(tuple(t.shape), dtype, KPAD, 0, device=DEV)
    a.outs.append((drows, dv))
    labd = lab.to(DEV).reshape(-1).contiguous()
    n = LOSS_N
    width = 3 if loss in ("dice", "tversky") else 4
    chunks = ops.dice_chunks(lv) if loss == "dice" else ops.dice_ce_chunks(lv)
    shape = (n, chunks, 3, k) if loss == "dice" else (chunks, n, width, k)
    part = torch.empty((shape[0] * shape[1] * shape[2] + GUARD_BYTES // 4, k), device=DEV)
    part.view(torch.int32).fill_(SENTINEL)
    used = shape[0] * shape[1] * shape[2]
    coef = torch.full((n, width - 1 if loss != "dice" else 2, k), float("nan"), device=DEV)
    out = torch.full((1,), float("nan"), device=DEV)
    db = torch.full((k,), float("nan"), device=DEV)
    if loss == "dice":
        ops.softmax_dice_fwd(lv, labd, part, coef, out)
        ops.softmax_dice_bwd(lv, labd, coef, gs, dv, scratch=part, bias_grad=db)
    elif loss == "dice_ce":
        ops.softmax_dice_ce_fwd(lv, labd, part, coef, out)
        ops.softmax_dice_ce_bwd(lv, labd, coef, gs, dv, scratch=part, bias_grad=db)
    elif loss == "tversky":
        ops.softmax_tversky_fwd(lv, labd, part, coef, out, alpha=TV_ALPHA, beta=TV_BETA)
        ops.softmax_tversky_bwd(lv, labd, coef, gs, dv, scratch=part, bias_grad=db)
    else:
        ops.softmax_dice_focal_fwd(lv, labd, part, coef, out)
        ops.softmax_dice_focal_bwd(lv, labd, coef, 2.0, gs, dv, scratch=part, bias_grad=db)
    a.check()
    assert bool((part[used:].view(torch.int32) == SENTINEL).all())
    finite(out, coef, db)
    rtol = 1e-4 if dtype == F32 else 1e-2
    got = float(out.cpu())
    # test_softmax_dice holds the Dice loss of every type to 1e-6; the others: 1e-6 in f32, 1e-4 of the loss in 16 bits
    assert abs(got - want) < (1e-6 * max(1.0, abs(want)) if dtype == F32 or loss == "dice" else 1e-4 * abs(want))
    assert relerr64(grad.to(dtype).double(), grad) < rtol / 2          # the storage rounding alone leaves room
    assert relerr64(ncdhw(dv).double(), grad) < rtol
    assert float((db.cpu().double() - grad.sum((0, 2, 3, 4))).abs().max()) < 1e-5 + rtol * float(grad.abs().sum() / k)


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("k", [3, 5])
def test_argmax_reads_the_real_classes_of_a_padded_row(k, dtype):
    """NaN counts as maximal in argmax: one padding class read and the label is wrong"""
    lg, _ = loss_inputs(k)
    a = Arenas()
    t = ndhwc(lg).to(DEV, dtype)
    rows, lv = va.arena(tuple(t.shape), dtype, KPAD, 0, device=DEV)
    va.fill_view(lv, t)
    a.ins.append((rows, lv, t))
    nvox = t.numel() // k
    lab = torch.full((nvox + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    ops.argmax(lv, lab[:nvox].view(t.shape[:4]))
    a.check()
    assert bool((lab[nvox:] == 0xA5).all())
    assert torch.equal(lab[:nvox].view(t.shape[:4]).cpu().long(), torch.argmax(t.float().cpu(), dim=4))


# ---------------------------------------------------------------------------------- no family drops out silently
FWD_FAMILIES = {
    "conv_ring3_kernel<{t}, CK=16> (LDS-DMA ring)": ("bf16", "f16"),
    "conv_ring2_kernel<{t}, CK=16, NT=1>": ("bf16",),
    "conv_ring2_kernel<{t}, CK=32, NT=1>": ("bf16",),
    "conv_ring2_kernel<{t}, CK=32, NT=2>": ("bf16", "f16"),
    "conv_fwd_ks_kernel<{t}, k3 s1>": ("bf16", "f16", "f32"),
    "conv_fwd_mfma_kernel<{t}, CK=16, k3 s1>": ("bf16", "f16"),
    "conv_fwd_mfma_kernel<{t}, CK=32, k3 s2>": ("bf16", "f16"),
    "conv_fwd_mfma_kernel<{t}, CK=16, k1 s1>": ("bf16", "f16"),
    "conv_small_fwd_kernel<{t}>": ("bf16", "f16", "f32"),
    "conv_direct_kernel<{t}>": ("bf16", "f16", "f32"),
}


def fabricated(base, n, sp, c, form, dtype):
    """a view of made-up, 4 KiB aligned address: the queries read the fields only (tests/helpers/conv_plan_queries.py)"""
    from segmantic_amd import _lib
    ld, c0 = form_of(c, form)
    es = torch.empty((), dtype=dtype).element_size()
    return _lib.Act(base + c0 * es, n, sp[0], sp[1], sp[2], c, ld)


def test_the_cases_reach_every_family_of_the_issue():
    """the kernel names the forward and input-gradient cases are launched under, asked of the query with the views'
    fields, equal the family list; the weight-gradient cases reach the four paths, the wave-specialised one with
    stride 1 and 2; the transposed cases the three transposed kernels"""
    import ctypes as C
    from segmantic_amd import _lib
    code = {F32: _lib.SEGMI_F32, BF16: _lib.SEGMI_BF16, F16: _lib.SEGMI_F16}
    reached = set()
    for key, (_, four, right, (n, d, h, w), cin, cout, k, s, _) in FWD.items():
        for dt, form in [(dt, f) for dt in four for f in FORMS] + [(dt, "right") for dt in right]:
            in_form = "right" if form == "odd" and ops.mfma_ok(cin, cout) and h16(dt) else form
            a_in = fabricated(0x10_0000_0000, n, (d, h, w), cin, in_form, dt)
            a_out = fabricated(0x20_0000_0000, n, out_sp((d, h, w), k, s), cout, form, dt)
            reached.add(_lib.lib.segmi_conv3d_fwd_kernel_name(code[dt], C.byref(a_in), C.byref(a_out), k, s).decode())
    want = {name.format(t=t) for name, types in FWD_FAMILIES.items() for t in types}
    assert reached == want, (sorted(want - reached), sorted(reached - want))
    dgrad = set()
    for key, (_, (n, d, h, w), cdy, cdx) in DGRAD.items():
        for form in FORMS:
            a_in = fabricated(0x10_0000_0000, n, (d, h, w), cdy, "right" if form == "odd" else form, BF16)
            a_out = fabricated(0x20_0000_0000, n, (d, h, w), cdx, form, BF16)
            dgrad.add(_lib.lib.segmi_conv3d_fwd_kernel_name(code[BF16], C.byref(a_in), C.byref(a_out), 3, 1).decode())
    assert dgrad == {"conv_ring3_kernel<bf16, CK=16> (LDS-DMA ring)", "conv_ring2_kernel<bf16, CK=16, NT=1>",
                     "conv_ring2_kernel<bf16, CK=32, NT=2>", "conv_fwd_ks_kernel<bf16, k3 s1>",
                     "conv_fwd_mfma_kernel<bf16, CK=16, k3 s1>"}, sorted(dgrad)
    assert {(c[0], c[5]) for c in WGRAD.values()} == {("wave-specialised", 1), ("wave-specialised", 2), ("mfma", 1),
                                                      ("small-cin", 2), ("direct", 1)}
    assert {convt_family(dt, c[4], c[5], c[3][2]) for c in CONVT.values() for dt in c[1]} == {"persistent", "tile", "direct"}
