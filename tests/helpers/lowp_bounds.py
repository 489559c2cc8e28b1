"""Elementwise error bound for 16-bit-storage kernels that accumulate in f32.

An op of this kind reads fp16 (or bf16) operands, accumulates their products in f32 and rounds the
result once to its storage type.  ``ref`` is the same op in float64 on the very operands the kernel
reads (already rounded to the storage type), with every intermediate rounding the kernel performs by
contract emulated; ``absref`` (``A``) is the op applied to |operands| in float64 -- ``conv(|x|, |w|)``
for a convolution, ``wgrad(|x|, |dy|)`` for a weight gradient.  Per element:

    |got - ref| <= 1.05 * 2^-11 * |ref| + 2^-18 * A + 2^-25          (fp16 output)
    |got - ref| <=                        2^-18 * A + 2^-25          (f32 output: ``rounded=False``)

* ``2^-11 |ref|`` is half an fp16 ulp relative to the value: the single rounding of the output to
  nearest even.  The factor 1.05 leaves room for the f32 sum landing on the other side of a rounding
  boundary than the float64 sum.  A bf16-rounded output errs by up to 2^-8 |ref|, 7.6x this term, and a
  calibration on U(-1, 1) convolutions fails it on 64-73 % of the elements; ``HALF_OUT_MIN_RATIO``
  below is the margin the host self-test holds it to.
* ``2^-18 A`` is the f32 accumulation: every f32 add errs by at most 2^-24 of a partial sum, and the
  partial sums are bounded by ``A``, so 2^-18 leaves a factor of 64 for the length and order of the
  chain.  It is measured against ``A``, not ``|ref|``, because cancellation makes ``|ref|`` arbitrarily
  small while the rounding noise stays proportional to ``A``.
* ``2^-25`` is half the spacing of fp16 subnormals (2^-24): the rounding of an output in the subnormal
  range.  It is far below any fp16 operand, so an operand flushed to zero (>= 2^-24 lost per product,
  times a normal weight) or rounded through bf16 (2^-9 of it) exceeds the bound.  An f32 output keeps
  the same absolute floor: it costs nothing at the magnitudes these tests use.

Overflow.  The fp16 store rounds ``|v| >= 65520`` to Inf (nearest even; 65504 is the largest finite
value).  Where ``|ref|`` clears 65520 by more than the accumulation term the output must be exactly
``±Inf`` with the sign of ``ref``; where it is below 65520 by that margin it must be finite and inside
the bound; in the band between either is accepted.  A store that saturates to 65504 fails.  NaN in
the output is never accepted unless ``ref`` is NaN.

Other storage types.  ``bound``, ``ratio`` and ``assert_within`` take the storage type of the output
(``"f16"``, the default, ``"bf16"`` or ``"f32"``, or the torch dtype).  Per element:

    |got - ref| <= 1.05 * 2^-8  * |ref| + 2^-18 * A                  (bf16 output)
    |got - ref| <= 1.05 * 2^-24 * |ref| + 2^-18 * A                  (f32 output, ``rounded=True``)
    |got - ref| <=                        2^-18 * A                  (f32 accumulator: ``rounded=False``)

* bf16 keeps 8 significand bits (7 stored and the implicit one): a value in [2^e, 2^(e+1)) lies on a grid of
  spacing 2^(e-7), so rounding to nearest moves it by at most 2^(e-8) <= 2^-8 |v|.  A store that truncates
  errs by up to a whole spacing, 2^-7 |v|, one-sidedly: on U(-1, 1) convolutions 18-24 % of its elements
  leave this bound while its max-norm error (0.4-0.7 %) stays inside a 1.5 % gate.
* f32 keeps 24 significand bits, so each rounding of a value to f32 moves it by at most 2^-24 |v|.  An f32
  kernel rounds its operands nowhere; the term stands for the last f32 operation of the epilogue (bias,
  PReLU or residual add) on the result, the earlier ones being part of the chain the ``A`` term covers.
  Operands rounded through bf16 err by 2^-9 of a product each, 2^9 times the ``A`` term's unit.
* The factor 1.05 is the same allowance as for fp16: the f32 sum may lie across a rounding boundary from
  the float64 sum.  ``2^-18 A`` is the same f32 accumulation term: the accumulator is f32 for every type.
* No absolute floor: the subnormal range of bf16 and f32 starts at 2^-126, far below these magnitudes.
  Where the bound is 0 (``A == 0``: every product is zero) only the exact result is accepted.
* No overflow band.  A non-finite output is accepted only where ``ref`` is non-finite: ``±Inf`` of the same
  sign for an infinite ``ref``, NaN for a NaN ``ref``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

REL_HALF = 1.05 * 2.0 ** -11       # one fp16 output rounding, with a 5 % margin
REL_ACC = 2.0 ** -18               # f32 accumulation, relative to A = op(|operands|)
ABS_FLOOR = 2.0 ** -25             # half the fp16 subnormal spacing
F16_OVERFLOW = 65520.0             # round-to-nearest-even threshold of fp16 overflow
HALF_OUT_MIN_RATIO = 4.0           # a bf16-rounded output must exceed the bound by this factor
REL_BF16 = 1.05 * 2.0 ** -8        # one bf16 output rounding (8 significand bits), with the same 5 % margin
REL_F32 = 1.05 * 2.0 ** -24        # one f32 rounding of the result (24 significand bits), same margin

__all__ = ["REL_HALF", "REL_ACC", "ABS_FLOOR", "F16_OVERFLOW", "HALF_OUT_MIN_RATIO", "REL_BF16", "REL_F32",
           "storage_of", "bound", "ratio", "assert_within", "conv_ref", "convT_ref", "wgrad_ref", "flush_f16_subnormals"]


_STORAGE = {"f16": "f16", "fp16": "f16", torch.float16: "f16", "bf16": "bf16", torch.bfloat16: "bf16",
            "f32": "f32", "fp32": "f32", torch.float32: "f32"}
_REL = {"bf16": REL_BF16, "f32": REL_F32}


def storage_of(storage) -> str:
    """'f16' / 'bf16' / 'f32' for a storage-type name or torch dtype"""
    try:
        return _STORAGE[storage]
    except KeyError:
        raise ValueError(f"unknown storage type {storage!r}: expected f16, bf16, f32 or their torch dtypes") from None


def bound(ref: torch.Tensor, absref: torch.Tensor, rounded: bool = True, storage="f16") -> torch.Tensor:
    ref, absref = ref.double(), absref.double()
    storage = storage_of(storage)
    if storage != "f16":
        b = REL_ACC * absref
        return b + _REL[storage] * ref.abs() if rounded else b
    b = REL_ACC * absref + ABS_FLOOR
    if rounded:
        b = b + REL_HALF * ref.abs()
    return b


def _classify(ref, absref, rounded):
    """(must_be_inf, must_be_finite): masks of elements whose fp16 store must / must not overflow."""
    ref, absref = ref.double(), absref.double()
    if not rounded:
        fin = torch.isfinite(ref)
        return torch.zeros_like(fin), fin
    slack = REL_ACC * absref + ABS_FLOOR
    return ref.abs() - slack >= F16_OVERFLOW, ref.abs() + slack < F16_OVERFLOW


def _ratio_wide(got, ref, absref, rounded, storage):
    """bf16 / f32 storage: no overflow band, no floor (a zero bound accepts the exact result only)"""
    b = bound(ref, absref, rounded, storage)
    zero, inf = torch.zeros_like(ref), torch.full_like(ref, float("inf"))
    fin = torch.isfinite(ref) & torch.isfinite(got)
    err = torch.where(fin, got - ref, zero).abs()
    r = torch.where(b > 0, err / torch.where(b > 0, b, torch.ones_like(b)), torch.where(err == 0, zero, inf))
    r = torch.where(torch.isnan(r), inf, r)                    # a NaN bound (NaN in A) accepts nothing
    r = torch.where(torch.isfinite(got), r, inf)               # finite reference: the output must be finite
    right_inf = torch.isinf(got) & (torch.sign(got) == torch.sign(ref))
    r = torch.where(torch.isinf(ref), torch.where(right_inf, zero, inf), r)
    return torch.where(torch.isnan(ref), torch.where(torch.isnan(got), zero, inf), r)


def ratio(got: torch.Tensor, ref: torch.Tensor, absref: torch.Tensor, rounded: bool = True,
          storage="f16") -> torch.Tensor:
    """Per-element |got - ref| / bound on the elements that must be finite; +inf where an element that
    must overflow is not ±Inf of the right sign, or where a finite element is not finite.  Elements in
    the overflow band are 0 when they are ±Inf of the right sign or finite within the bound at 65504.
    bf16 and f32 storage have no overflow band: +inf wherever the output is non-finite and the reference
    is not non-finite in the same way, and wherever a zero bound is missed."""
    got, ref, absref = got.double().cpu(), ref.double().cpu(), absref.double().cpu()
    storage = storage_of(storage)
    if storage != "f16":
        return _ratio_wide(got, ref, absref, rounded, storage)
    must_inf, must_fin = _classify(ref, absref, rounded)
    r = torch.zeros_like(ref)
    b = bound(ref, absref, rounded)
    with torch.no_grad():
        err = (got - ref).abs() / b
    right_inf = torch.isinf(got) & (torch.sign(got) == torch.sign(ref))
    band = ~must_inf & ~must_fin & torch.isfinite(ref)
    r = torch.where(must_fin, torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf"))), r)
    r = torch.where(must_inf, torch.where(right_inf, torch.zeros_like(err), torch.full_like(err, float("inf"))), r)
    band_err = torch.where(torch.isfinite(got), (got - ref.clamp(-65504.0, 65504.0)).abs() / b,
                           torch.full_like(err, float("inf")))
    r = torch.where(band, torch.where(right_inf, torch.zeros_like(err), band_err), r)
    nan_ref = torch.isnan(ref)
    r = torch.where(nan_ref, torch.where(torch.isnan(got), torch.zeros_like(err), torch.full_like(err, float("inf"))), r)
    return r


def assert_within(got, ref, absref, rounded: bool = True, what: str = "", storage="f16") -> float:
    """Assert the bound on every element; returns the worst ratio (for reports)."""
    r = ratio(got, ref, absref, rounded, storage)
    name = {"f16": "fp16", "bf16": "bf16", "f32": "f32"}[storage_of(storage)]
    worst = float(r.max()) if r.numel() else 0.0
    if not worst <= 1.0:
        bad = r > 1.0
        i = int(torch.argmax(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)))
        g, f, a = got.double().cpu().flatten()[i], ref.double().cpu().flatten()[i], absref.double().cpu().flatten()[i]
        raise AssertionError(f"{what}: {int(bad.sum())}/{r.numel()} elements outside the {name} bound, worst "
                             f"ratio {worst:.3g} at flat index {i}: got {float(g)!r}, ref {float(f)!r}, A {float(a)!r}")
    return worst


# ------------------------------------------------------------------------------------ float64 references
def conv_ref(x, w, bias=None, stride=1, padding=1):
    """conv3d in float64 (NCDHW) and its |operand| companion A."""
    x, w = x.double(), w.double()
    ref = F.conv3d(x, w, None if bias is None else bias.double(), stride=stride, padding=padding)
    a = F.conv3d(x.abs(), w.abs(), None if bias is None else bias.double().abs(), stride=stride, padding=padding)
    return ref, a


def convT_ref(x, w, bias=None, stride=2, padding=1, output_padding=1):
    x, w = x.double(), w.double()
    kw = dict(stride=stride, padding=padding, output_padding=output_padding)
    ref = F.conv_transpose3d(x, w, None if bias is None else bias.double(), **kw)
    a = F.conv_transpose3d(x.abs(), w.abs(), None if bias is None else bias.double().abs(), **kw)
    return ref, a


def wgrad_ref(x, dy, ksize=3, stride=1):
    """(dw, A_dw, db, A_db) of conv3d(x, w) for output gradient dy, all float64 (NCDHW)."""
    pad = (ksize - 1) // 2
    cout, cin = dy.shape[1], x.shape[1]

    def dw_of(xx, gg):
        w0 = torch.zeros((cout, cin, ksize, ksize, ksize), dtype=torch.float64, requires_grad=True)
        F.conv3d(xx, w0, None, stride=stride, padding=pad).backward(gg)
        return w0.grad

    x, dy = x.double(), dy.double()
    return dw_of(x, dy), dw_of(x.abs(), dy.abs()), dy.sum((0, 2, 3, 4)), dy.abs().sum((0, 2, 3, 4))


def flush_f16_subnormals(t: torch.Tensor) -> torch.Tensor:
    """What a denormal-flushing unit would read: fp16 subnormals (|v| < 2^-14) replaced by signed zero."""
    return torch.where(t.abs() < 2.0 ** -14, t * 0, t)
