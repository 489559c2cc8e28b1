"""The bf16 and f32 bounds of tests/helpers/lowp_bounds.py, host side (no GPU).

tests/helpers/lowp_bounds.py is the gate every bf16 / f32 op test applies.  These cases prove on the CPU, with the
reference alone, that it accepts a correctly rounded result and rejects each failure mode the GPU tests look for: a
bf16 store that truncates, a convolution that misses a tap, f32 operands that went through bf16, and non-finite
values.  The shares asserted here are conditions on the gate, not tolerances of a kernel.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import lowp_bounds as lb

BOUND_CONVS = [(16, 16, (6, 8, 10)), (128, 16, (4, 6, 6)), (1, 16, (6, 8, 10))]
BF16, F32 = torch.bfloat16, torch.float32


def _u(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def _conv_operands(cin, cout, sp, seed, dtype=BF16):
    """U(-1, 1) activations and weights scaled by (27 Cin)^-1/2, rounded to ``dtype``, as float64"""
    x = _u((1, cin) + sp, seed).to(dtype).double()
    w = _u((cout, cin, 3, 3, 3), seed + 1, 1.0 / math.sqrt(27 * cin)).to(dtype).double()
    return x, w


def _conv32(x, w):
    return F.conv3d(x.float(), w.float(), padding=1)


def _truncate_to_bf16(v):
    """the f32 value with its low 16 bits cleared: a bf16 store that does not round"""
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def test_storage_names_and_dtypes_select_the_same_bound():
    ref, a = torch.tensor([1.0, -3.0, 0.0]), torch.tensor([2.0, 3.0, 0.0])
    for name, dt in (("f16", torch.float16), ("bf16", BF16), ("f32", F32)):
        assert torch.equal(lb.bound(ref, a, storage=name), lb.bound(ref, a, storage=dt))
        assert lb.storage_of(dt) == name
    assert torch.equal(lb.bound(ref, a), lb.bound(ref, a, storage="f16"))                 # the default is fp16
    assert torch.equal(lb.bound(ref, a, storage="bf16"), lb.REL_BF16 * ref.double().abs() + lb.REL_ACC * a.double())
    assert torch.equal(lb.bound(ref, a, storage="f32"), lb.REL_F32 * ref.double().abs() + lb.REL_ACC * a.double())
    for st in ("bf16", "f32"):                                                             # the accumulator output
        assert torch.equal(lb.bound(ref, a, rounded=False, storage=st), lb.REL_ACC * a.double())
    assert lb.REL_BF16 == 1.05 * 2.0 ** -8 and lb.REL_F32 == 1.05 * 2.0 ** -24
    with pytest.raises(ValueError):
        lb.bound(ref, a, storage="fp8")


@pytest.mark.parametrize("cin,cout,sp", BOUND_CONVS)
def test_bounds_accept_the_correctly_rounded_result(cin, cout, sp, record_property):
    x, w = _conv_operands(cin, cout, sp, 10)
    ref, a = lb.conv_ref(x, w)
    y32 = _conv32(x, w)
    worst = {"bf16": lb.assert_within(y32.bfloat16(), ref, a, storage="bf16", what="bf16"),
             "f32": lb.assert_within(y32, ref, a, storage="f32", what="f32")}
    # the weight gradient: an f32 accumulator output, no storage rounding
    dy = _u((1, cout) + sp, 12).bfloat16().double()
    dw, adw, db, adb = lb.wgrad_ref(x, dy)
    w0 = torch.zeros((cout, cin, 3, 3, 3), requires_grad=True)
    b0 = torch.zeros((cout,), requires_grad=True)
    F.conv3d(x.float(), w0, b0, padding=1).backward(dy.float())
    for st in ("bf16", "f32"):
        worst[f"dw {st}"] = lb.assert_within(w0.grad, dw, adw, rounded=False, storage=st, what="dw")
        worst[f"db {st}"] = lb.assert_within(b0.grad, db, adb, rounded=False, storage=st, what="db")
    for k, v in worst.items():
        record_property(f"worst ratio {k}", round(v, 4))
        assert v <= 1.0


@pytest.mark.parametrize("cin,cout,sp", BOUND_CONVS)
def test_bf16_bound_rejects_a_truncating_store(cin, cout, sp, record_property):
    x, w = _conv_operands(cin, cout, sp, 20)
    ref, a = lb.conv_ref(x, w)
    y32 = _conv32(x, w)
    r = lb.ratio(_truncate_to_bf16(y32), ref, a, storage="bf16")
    share = float((r > 1).double().mean())
    record_property("share outside", round(share, 4))
    assert share > 0.10
    # while the max-norm gate of 1.5 % lets it through
    assert float((_truncate_to_bf16(y32).double() - ref).abs().max() / ref.abs().max()) < 1.5e-2
    with pytest.raises(AssertionError, match="bf16 bound"):
        lb.assert_within(_truncate_to_bf16(y32), ref, a, storage="bf16")


@pytest.mark.parametrize("cin,cout,sp", BOUND_CONVS)
def test_bf16_bound_rejects_a_missing_tap(cin, cout, sp, record_property):
    x, w = _conv_operands(cin, cout, sp, 30)
    ref, a = lb.conv_ref(x, w)
    wm = w.clone()
    wm[:, :, 0, 0, 0] = 0
    r = lb.ratio(_conv32(x, wm).bfloat16(), ref, a, storage="bf16")
    share = float((r > 1).double().mean())
    record_property("share outside", round(share, 4))
    assert share > 0.40


@pytest.mark.parametrize("cin,cout,sp", BOUND_CONVS)
def test_f32_bound_rejects_one_channel_of_bf16_rounded_operands(cin, cout, sp):
    """f32 operands here (bf16-rounded ones would not change): one input channel through bf16 leaves the bound"""
    x, w = _conv_operands(cin, cout, sp, 40, dtype=F32)
    ref, a = lb.conv_ref(x, w)
    assert lb.assert_within(_conv32(x, w), ref, a, storage="f32") <= 1.0
    ch = min(3, cin - 1)
    wb = w.clone()
    wb[:, ch] = wb[:, ch].float().bfloat16().double()
    assert float(lb.ratio(_conv32(x, wb), ref, a, storage="f32").max()) > 1.0
    xb = x.clone()
    xb[:, ch] = xb[:, ch].float().bfloat16().double()
    assert float(lb.ratio(_conv32(xb, w), ref, a, storage="f32").max()) > 1.0
    # ... and the f32 accumulator bound of a weight gradient
    dy = _u((1, cout) + sp, 42).float().double()
    dw, adw, _, _ = lb.wgrad_ref(x, dy)
    dwb, _, _, _ = lb.wgrad_ref(xb, dy)
    assert float(lb.ratio(dwb, dw, adw, rounded=False, storage="f32").max()) > 1.0


@pytest.mark.parametrize("storage", ["bf16", "f32"])
@pytest.mark.parametrize("rounded", [True, False])
def test_bounds_reject_non_finite_values_the_reference_does_not_have(storage, rounded):
    inf, nan = float("inf"), float("nan")
    ref = torch.tensor([1.0, -2.0, inf, -inf, nan, 3.0, 0.0, 0.0], dtype=torch.float64)
    a = torch.tensor([1.0, 2.0, inf, inf, nan, 3.0, 0.0, 0.0], dtype=torch.float64)
    right = ref.clone()
    assert lb.assert_within(right, ref, a, rounded=rounded, storage=storage) == 0.0
    for i, v in ((0, inf), (1, -inf), (0, nan), (5, nan),       # Inf / NaN against a finite reference
                 (2, 1.0e38), (3, -1.0e38),                     # a finite value against an Inf reference
                 (2, -inf), (3, inf), (2, nan),                 # the wrong Inf, NaN for Inf
                 (4, 1.0), (4, inf),                            # anything but NaN for a NaN reference
                 (6, 1e-30), (7, -1e-45)):                      # a zero bound accepts the exact result only
        bad = right.clone()
        bad[i] = v
        r = lb.ratio(bad, ref, a, rounded=rounded, storage=storage)
        assert float(r[i]) == inf, (i, v)
        keep = torch.arange(ref.numel()) != i
        assert bool((r[keep] == 0).all()), (i, v)
        with pytest.raises(AssertionError):
            lb.assert_within(bad, ref, a, rounded=rounded, storage=storage)
    # -0 for +0 is the exact result
    assert float(lb.ratio(torch.tensor([-0.0]), torch.tensor([0.0]), torch.tensor([0.0]), storage=storage).max()) == 0.0
