"""The Tversky and Dice + focal loss kernels and the configured training objective on the GPU.

Op level: ``segmi_softmax_tversky_*`` and ``segmi_softmax_dice_focal_*`` against the float64 reference of
tests/helpers/imbalance_loss_ref.py on the logits rounded to the storage type, with the shapes, cases and gates of
tests/test_loss_gpu.py: n = 3, 17 x 24 x 33 = one full 8192-voxel chunk + a ragged one, a batch-global normaliser;
K in {2, 3, 4, 5, 16, 32, 64}; loss 1e-6 * max(1, |loss|) in f32 and 1e-4 * |loss| in 16 bits, dlogits max-relative
1e-4 / 1e-2, bias sums 1e-5 + rtol * sum|g| / k.

Whole step: ``Net.training_step`` with a configured loss against ``unet_sweep.oracle_step`` with the same loss.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from tests.helpers import lowp_bounds as lb  # noqa: E402
from tests.helpers import unet_sweep as us  # noqa: E402
from tests.helpers.imbalance_loss_ref import ref_dice_focal_loss, ref_tversky_loss, tversky_grad_abs  # noqa: E402

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = {"f32": F32, "bf16": BF16, "fp16": F16}
N, SP = 3, (17, 24, 33)
KS = [2, 3, 4, 5, 16, 32, 64]
# grad_scale of the parity runs.  The gradient of a mean over 3 x 13 464 voxels is small: its largest element is 2.4e-6
# to 2.5e-5 on these inputs, inside fp16's subnormal range (below 6.1e-5, spacing 6.0e-8), where the nearest fp16 value
# of the exact gradient is already off by up to 3.0e-8 -- 0.0126 of the largest element for Tversky at K = 64, above the
# 1e-2 gate before any kernel has run.  No fp16 gradient is stored unscaled in training (the loss scale exists for
# this), so the fp16 cases run at 2^10, which puts the largest elements into the normal range; a power of two scales
# the float64 reference exactly.  ``check_parity`` asserts that the storage rounding of the exact gradient alone is below
# half the gate (bf16's is 2^-8 = 0.0039 of the largest element at any scale, fp16's 2^-11 in the normal range), so that
# the gate measures the kernel.
GRAD_SCALE = {"f32": 1.0, "bf16": 1.0, "fp16": 2.0 ** 10}


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def relerr(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def from_ndhwc(t):
    return t.float().cpu().permute(0, 4, 1, 2, 3).contiguous()


def to_ndhwc(x_ncdhw, dtype, ld=None):
    """NDHWC device tensor of the K real classes; ``ld`` > K: a view into rows padded to ``ld`` channels"""
    t = x_ncdhw.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)
    if ld is None:
        return t
    full = torch.zeros(tuple(t.shape[:4]) + (ld,), dtype=dtype, device=DEV)
    full[..., :t.shape[4]] = t
    return full[..., :t.shape[4]]


def empty_like_rows(t, ld=None):
    if ld is None:
        return torch.empty_like(t)
    return torch.zeros(tuple(t.shape[:4]) + (ld,), dtype=t.dtype, device=DEV)[..., :t.shape[4]]


def weights_for(k, seed, zero_at=None):
    w = (torch.rand(k, generator=torch.Generator().manual_seed(seed)) * 1.9 + 0.1).tolist()
    if zero_at is not None:
        w[zero_at] = 0.0
    return [float(torch.tensor(v, dtype=F32)) for v in w]       # the f32 values the kernel reads


def f32v(v):
    return float(torch.tensor(v, dtype=F32))


# --------------------------------------------------------------------------------------------- cases
T_PSETS = ["defaults", "nobg", "fp-heavy-focal", "absent-class"]
F_PSETS = ["gamma1", "gamma2", "gamma5", "weights", "zero-weight", "focal-only"]


def param_set(loss, name, k):
    """keyword arguments of the loss (reference and kernel alike; the values are exact in f32 or rounded to it)"""
    if loss == "tversky":
        base = dict(include_background=True, alpha=f32v(0.3), beta=f32v(0.7), exponent=1.0)
        if name == "nobg":
            base.update(include_background=False)
        elif name == "fp-heavy-focal":
            base.update(alpha=f32v(0.7), beta=f32v(0.3), exponent=0.75)
        else:
            assert name in ("defaults", "absent-class", "dice")
            if name == "dice":
                base.update(alpha=0.5, beta=0.5)
        return base
    base = dict(include_background=True, lambda_dice=1.0, lambda_focal=1.0, gamma=2.0, weight=None)
    if name == "gamma1":
        base.update(gamma=1.0)
    elif name == "gamma5":
        base.update(gamma=5.0, include_background=False)
    elif name == "weights":
        base.update(weight=weights_for(k, 100 + k), lambda_dice=0.5, lambda_focal=2.0, gamma=1.5)
    elif name == "zero-weight":
        base.update(weight=weights_for(k, 200 + k, zero_at=k // 2))
    elif name == "focal-only":
        base.update(lambda_dice=0.0)
    else:
        assert name == "gamma2"
    return base


@functools.lru_cache(maxsize=None)
def inputs(k, absent=False):
    lg = rnd((N, k) + SP, 61 + k, 3.0)
    lab = torch.randint(0, k, (N, 1) + SP, generator=torch.Generator().manual_seed(62 + k)).float()
    if absent:                             # class k-1 does not occur in sample 1
        lab[1] = torch.where(lab[1] == k - 1, torch.zeros_like(lab[1]), lab[1])
        assert not bool((lab[1] == k - 1).any()) and bool((lab[0] == k - 1).any())
    return lg, lab


def ref_loss(loss, lq, lab, params):
    return ref_tversky_loss(lq, lab, **params) if loss == "tversky" else ref_dice_focal_loss(lq, lab, **params)


@functools.lru_cache(maxsize=None)
def truth(loss, k, dt, pset):
    """float64 reference on the logits rounded to the storage type: (loss, dlogits, bias sums), computed once"""
    lg, lab = inputs(k, pset == "absent-class")
    lq = lg.to(DTYPES[dt]).double().requires_grad_(True)
    v = ref_loss(loss, lq, lab, param_set(loss, pset, k))
    v.backward()
    return float(v.detach()), lq.grad.detach(), lq.grad.detach().sum((0, 2, 3, 4))


def run_tversky(ld_, labd, params, grad_scale=1.0, bias=True, amp=None, ld=None, smooth=1e-5):
    n, k = ld_.shape[0], ld_.shape[4]
    part = torch.empty((ops.dice_ce_chunks(ld_), n, 3, k), device=DEV)
    coef = torch.empty((n, 2, k), device=DEV)
    out = torch.empty(1, device=DEV)
    ops.softmax_tversky_fwd(ld_, labd, part, coef, out, smooth, smooth, params["alpha"], params["beta"],
                            params["exponent"], params["include_background"])
    dl = empty_like_rows(ld_, ld)
    db = torch.empty(k, device=DEV) if bias else None
    kw = dict(scratch=part if bias else None, bias_grad=db)
    if amp is not None:
        ops.softmax_tversky_bwd_amp(ld_, labd, coef, amp, dl, **kw)
    else:
        ops.softmax_tversky_bwd(ld_, labd, coef, grad_scale, dl, **kw)
    torch.cuda.synchronize()
    return out, dl, db


def run_focal(ld_, labd, params, grad_scale=1.0, bias=True, amp=None, ld=None):
    n, k = ld_.shape[0], ld_.shape[4]
    part = torch.empty((ops.dice_ce_chunks(ld_), n, 4, k), device=DEV)
    coef = torch.empty((n, 3, k), device=DEV)
    out = torch.empty(1, device=DEV)
    w = params["weight"]
    wd = None if w is None else torch.tensor(w, dtype=F32, device=DEV)
    ops.softmax_dice_focal_fwd(ld_, labd, part, coef, out, lambda_dice=params["lambda_dice"],
                               lambda_focal=params["lambda_focal"], gamma=params["gamma"],
                               include_background=params["include_background"], class_weight=wd)
    dl = empty_like_rows(ld_, ld)
    db = torch.empty(k, device=DEV) if bias else None
    kw = dict(scratch=part if bias else None, bias_grad=db)
    if amp is not None:
        ops.softmax_dice_focal_bwd_amp(ld_, labd, coef, params["gamma"], amp, dl, **kw)
    else:
        ops.softmax_dice_focal_bwd(ld_, labd, coef, params["gamma"], grad_scale, dl, **kw)
    torch.cuda.synchronize()
    return out, dl, db


def run_dice_ce(ld_, labd, lambda_dice, lambda_ce, include_background=True, weight=None, bias=True):
    n, k = ld_.shape[0], ld_.shape[4]
    part = torch.empty((ops.dice_ce_chunks(ld_), n, 4, k), device=DEV)
    coef = torch.empty((n, 3, k), device=DEV)
    out = torch.empty(1, device=DEV)
    wd = None if weight is None else torch.tensor(weight, dtype=F32, device=DEV)
    ops.softmax_dice_ce_fwd(ld_, labd, part, coef, out, lambda_dice=lambda_dice, lambda_ce=lambda_ce,
                            include_background=include_background, class_weight=wd)
    dl = torch.empty_like(ld_)
    db = torch.empty(k, device=DEV) if bias else None
    ops.softmax_dice_ce_bwd(ld_, labd, coef, 1.0, dl, scratch=part if bias else None, bias_grad=db)
    torch.cuda.synchronize()
    return out, dl, db


RUN = {"tversky": run_tversky, "focal": run_focal}


def check_parity(loss, k, dt, pset, ld=None):
    dtype = DTYPES[dt]
    lg, lab = inputs(k, pset == "absent-class")
    loss_ref, grad_ref, db_ref = truth(loss, k, dt, pset)
    gs = GRAD_SCALE[dt]
    grad_ref, db_ref = grad_ref * gs, db_ref * gs
    rtol = 1e-4 if dtype == F32 else 1e-2
    storage = relerr(grad_ref.to(dtype).double(), grad_ref)     # the exact gradient rounded to the storage type
    assert storage < rtol / 2, storage
    ld_ = to_ndhwc(lg, dtype, ld)
    labd = lab.to(DEV).reshape(-1).contiguous()
    out, dl, db = RUN[loss](ld_, labd, param_set(loss, pset, k), grad_scale=gs, ld=ld)
    got = float(out.cpu())
    gerr = relerr(from_ndhwc(dl).double(), grad_ref)
    berr = float((db.cpu().double() - db_ref).abs().max())
    blim = 1e-5 + rtol * float(grad_ref.abs().sum() / k)
    llim = 1e-6 * max(1.0, abs(loss_ref)) if dtype == F32 else 1e-4 * abs(loss_ref)
    print(f"MEASURED {loss} K={k} {dt} {pset} ld={ld}: loss {got!r} ref {loss_ref!r} |d| {abs(got - loss_ref):.3g} "
          f"(limit {llim:.3g}, ratio {abs(got - loss_ref) / llim:.3g}); dlogits rel {gerr:.3g} (limit {rtol:g}, "
          f"ratio {gerr / rtol:.3g}, storage rounding alone {storage:.3g}); bias {berr:.3g} (limit {blim:.3g}, ratio {berr / blim:.3g})")
    assert abs(got - loss_ref) < llim
    assert gerr < rtol
    assert berr < blim
    return dl


# ------------------------------------------------------------------------------------------------ op-level parity
@pytest.mark.parametrize("pset", T_PSETS)
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("k", KS)
def test_tversky_matches_the_float64_reference(k, dt, pset):
    check_parity("tversky", k, dt, pset)


@pytest.mark.parametrize("pset", F_PSETS)
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("k", KS)
def test_dice_focal_matches_the_float64_reference(k, dt, pset):
    check_parity("focal", k, dt, pset)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("loss,pset", [("tversky", "fp-heavy-focal"), ("focal", "weights")])
def test_padded_class_row(loss, pset, dt):
    """K = 5 real classes in rows of 16 (the engine's kpad layout): logits and dlogits are views with row stride 16;
    the padding of dlogits stays untouched"""
    dl = check_parity(loss, 5, dt, pset, ld=16)
    full = dl._base if dl._base is not None else dl
    assert tuple(full.shape[-1:]) == (16,) and not bool(full[..., 5:].any())


# ------------------------------------------------------------------------------------------------ Tversky = Dice
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("k", [3, 16])
def test_tversky_with_half_weights_is_the_dice_kernels(k, dt):
    """alpha = beta = 0.5, exponent = 1, smooths s / 2 against segmi_softmax_dice_ce_fwd / _bwd with lambda_ce = 0: the
    loss at 1e-6, dlogits within the f32 gate (both kernels read the same stored logits, so the gate is f32's for every
    storage type up to the rounding of the stored gradient)"""
    lg, lab = inputs(k)
    ld_ = to_ndhwc(lg, DTYPES[dt])
    labd = lab.to(DEV).reshape(-1).contiguous()
    out, dl, db = run_tversky(ld_, labd, param_set("tversky", "dice", k), smooth=5e-6)
    for nobg in (False, True):
        if nobg:
            out, dl, db = run_tversky(ld_, labd, dict(param_set("tversky", "dice", k), include_background=False),
                                      smooth=5e-6)
        out0, dl0, db0 = run_dice_ce(ld_, labd, 1.0, 0.0, include_background=not nobg)
        a, b = float(out.cpu()), float(out0.cpu())
        gerr = relerr(from_ndhwc(dl).double(), from_ndhwc(dl0).double())
        print(f"MEASURED tversky=dice K={k} {dt} nobg={nobg}: {a!r} vs {b!r}; dlogits rel {gerr:.3g}")
        assert abs(a - b) < 1e-6
        # a 16-bit store may round the two nearly equal gradients to neighbouring values: one ulp, 2^-7 (bf16) / 2^-10 (fp16)
        assert gerr < (1e-4 if dt == "f32" else 1e-4 + (2.0 ** -7 if dt == "bf16" else 2.0 ** -10))


# ------------------------------------------------------------------------------------------------ gamma = 0
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("k", [3, 16])
def test_gamma_zero_is_the_dice_ce_kernels_bit_for_bit(k, dt):
    lg, lab = inputs(k)
    ld_ = to_ndhwc(lg, DTYPES[dt])
    labd = lab.to(DEV).reshape(-1).contiguous()
    w = weights_for(k, 100 + k)
    params = dict(include_background=False, lambda_dice=0.5, lambda_focal=2.0, gamma=0.0, weight=w)
    a = run_focal(ld_, labd, params)
    b = run_dice_ce(ld_, labd, 0.5, 2.0, include_background=False, weight=w)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    amp = torch.tensor([1.0, 0.0, 0.0], device=DEV)
    c = run_focal(ld_, labd, params, amp=amp)
    assert torch.equal(c[1], b[1])


# ------------------------------------------------------------------------------------------------ edge cases
def test_true_class_200_below_the_maximum_contributes_200():
    """f32, K = 3: class 0 at 200, the others (among them every voxel's true class) at 0: q = 1, so the focal term is
    the cross-entropy's 200, and every dlogit is finite"""
    lg = torch.zeros((N, 3) + SP)
    lg[:, 0] = 200.0
    lab = torch.randint(1, 3, (N, 1) + SP, generator=torch.Generator().manual_seed(7)).float()
    ld_, labd = to_ndhwc(lg, F32), lab.to(DEV).reshape(-1).contiguous()
    for params in (dict(include_background=True, lambda_dice=0.0, lambda_focal=1.0, gamma=2.0, weight=None),
                   param_set("focal", "gamma2", 3)):
        ref = float(ref_dice_focal_loss(lg.double(), lab, **params))
        out, dl, db = run_focal(ld_, labd, params)
        got = float(out.cpu())
        print(f"far true class: loss {got!r} ref {ref!r}")
        assert abs(got - ref) < 1e-6 * max(1.0, abs(ref))
        if params["lambda_dice"] == 0.0:
            assert abs(got - 200.0) < 1e-6 * 200.0
        assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(db).all())
    lq = lg.double().requires_grad_(True)
    ref_dice_focal_loss(lq, lab, **param_set("focal", "gamma2", 3)).backward()
    assert relerr(from_ndhwc(dl).double(), lq.grad) < 1e-4


@pytest.mark.parametrize("gamma", [1.0, 2.0])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_perfectly_classified_voxels_contribute_nothing(dt, gamma):
    """the true class 200 above the others: q = 0 exactly, the focal loss is 0 and so is its gradient (no NaN from
    0^(gamma - 1) or log2(0))"""
    lg = torch.zeros((N, 3) + SP)
    lab = torch.randint(0, 3, (N, 1) + SP, generator=torch.Generator().manual_seed(8)).float()
    lg.scatter_(1, lab.long(), 200.0)
    out, dl, db = run_focal(to_ndhwc(lg, DTYPES[dt]), lab.to(DEV).reshape(-1).contiguous(),
                            dict(include_background=True, lambda_dice=0.0, lambda_focal=1.0, gamma=gamma, weight=None))
    assert float(out.cpu()) == 0.0
    assert not bool(dl.any()) and not bool(db.any())


def test_all_zero_weights_give_nan():
    lg, lab = inputs(3)
    params = dict(include_background=True, lambda_dice=1.0, lambda_focal=1.0, gamma=2.0, weight=[0.0, 0.0, 0.0])
    assert math.isnan(float(ref_dice_focal_loss(lg.double(), lab, **params)))
    out, _, _ = run_focal(to_ndhwc(lg, F32), lab.to(DEV).reshape(-1).contiguous(), params)
    assert math.isnan(float(out.cpu()))
    # lambda_focal = 0 switches the term off: no NaN then
    params["lambda_focal"] = 0.0
    out, dl, _ = run_focal(to_ndhwc(lg, F32), lab.to(DEV).reshape(-1).contiguous(), params)
    want = float(ref_dice_focal_loss(lg.double(), lab, **params))
    assert abs(float(out.cpu()) - want) < 1e-6 and bool(torch.isfinite(dl).all())


@pytest.mark.parametrize("loss", ["tversky", "focal"])
def test_out_of_range_labels_count_for_nothing(loss):
    """labels outside [0, K) are in no class row: no target sum, no focal term, no normaliser"""
    k = 4
    lg, lab = inputs(k)
    lab = lab.clone()
    bad = torch.rand(lab.shape, generator=torch.Generator().manual_seed(3)) < 0.1
    lab[bad] = torch.where(torch.rand(int(bad.sum()), generator=torch.Generator().manual_seed(4)) < 0.5, -1.0, float(k))
    params = param_set(loss, "defaults", k) if loss == "tversky" else \
        dict(include_background=True, lambda_dice=0.0, lambda_focal=1.0, gamma=2.0, weight=weights_for(k, 9))
    lq = lg.double().requires_grad_(True)
    ref = ref_loss(loss, lq, lab, params)
    ref.backward()
    out, dl, _ = RUN[loss](to_ndhwc(lg, F32), lab.to(DEV).reshape(-1).contiguous(), params)
    assert abs(float(out.cpu()) - float(ref.detach())) < 1e-6 * max(1.0, abs(float(ref.detach())))
    g = from_ndhwc(dl)
    assert relerr(g.double(), lq.grad) < 1e-4
    if loss == "focal":
        assert not bool(g.permute(0, 2, 3, 4, 1)[bad[:, 0]].any())      # no focal gradient at those voxels


def test_tversky_zero_term_has_zero_coefficients():
    """smooth_nr > smooth_dr with every voxel right by 60: 1 - TI <= 0 for every class, so the loss and every dlogit
    are 0 (the rule of segmi.h)"""
    lg = torch.zeros((N, 3) + SP)
    lab = torch.randint(0, 3, (N, 1) + SP, generator=torch.Generator().manual_seed(8)).float()
    lg.scatter_(1, lab.long(), 60.0)
    ld_, labd = to_ndhwc(lg, F32), lab.to(DEV).reshape(-1).contiguous()
    n, k = N, 3
    part = torch.empty((ops.dice_ce_chunks(ld_), n, 3, k), device=DEV)
    coef = torch.empty((n, 2, k), device=DEV)
    out = torch.empty(1, device=DEV)
    ops.softmax_tversky_fwd(ld_, labd, part, coef, out, 1.0, 1e-5, 0.3, 0.7, 0.75, True)
    torch.cuda.synchronize()
    assert float(out.cpu()) == 0.0 and not bool(coef.any())


# ------------------------------------------------------------------------------------------------ determinism, fusion
@pytest.mark.parametrize("loss,pset", [("tversky", "fp-heavy-focal"), ("focal", "weights")])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("k", [5, 16])
def test_two_calls_are_bit_identical_and_bias_fusion_changes_nothing(k, dt, loss, pset):
    lg, lab = inputs(k)
    ld_ = to_ndhwc(lg, DTYPES[dt])
    labd = lab.to(DEV).reshape(-1).contiguous()
    params = param_set(loss, pset, k)
    a = RUN[loss](ld_, labd, params)
    b = RUN[loss](ld_, labd, params)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = RUN[loss](ld_, labd, params, bias=False)
    assert c[2] is None and torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


# ------------------------------------------------------------------------------------------------ loss-scaled backward
@pytest.mark.parametrize("loss,pset", [("tversky", "fp-heavy-focal"), ("focal", "weights")])
@pytest.mark.parametrize("k", [3, 16])
def test_loss_scaled_backward_stores_each_dlogit(k, loss, pset):
    """fp16 at scale 2^16, element by element against the f32 kernel's gradient on the same fp16 logits times the
    scale: the bound and method of ``test_loss_gpu.py::test_loss_scaled_backward_stores_each_dlogit``.  That test hands
    ``lowp_bounds`` ``|ref|`` as the accumulation companion ``A``, which holds where the gradient's terms do not cancel
    (the cross-entropy and focal terms dominate there).  In the Tversky gradient ``p_j (D_j - sum_i p_i D_i)`` they do,
    by factors up to 10^6 on these inputs, so for Tversky ``A`` is what ``lowp_bounds`` defines it to be, the expression
    on the absolute values of its operands (``tversky_grad_abs``); with ``|ref|`` the worst ratio was 1.0065 at K = 16.
    The bound grows by 1 to 2 % on the median element."""
    lg, lab = inputs(k)
    lg = lg.half().float()
    labd = lab.to(DEV).reshape(-1).contiguous()
    params = param_set(loss, pset, k)
    scale = 2.0 ** 16
    _, ref, ref_b = RUN[loss](to_ndhwc(lg, F32), labd, params)
    amp = torch.tensor([scale, 0.0, 0.0], device=DEV)
    _, got, got_b = RUN[loss](to_ndhwc(lg, F16), labd, params, amp=amp)
    ref = from_ndhwc(ref).double() * scale
    absref = ref.abs()
    if loss == "tversky":
        absref = tversky_grad_abs(lg.double(), lab, **params) * scale
        assert bool((absref >= ref.abs() * (1.0 - 1e-5)).all())       # A bounds |g| (f32 kernel against float64)
    r = lb.ratio(from_ndhwc(got).double(), ref, absref)
    print(f"MEASURED {loss} amp K={k}: worst ratio {float(r.max()):.3g} "
          f"(with |ref| for A: {float(lb.ratio(from_ndhwc(got).double(), ref, ref.abs()).max()):.3g})")
    assert float(r.max()) <= 1.0
    berr = float((got_b.cpu().double() - ref_b.cpu().double() * scale).abs().max())
    assert berr < 1e-5 + 1e-2 * float(ref.abs().sum() / k)


# ------------------------------------------------------------------------------------------------ whole step
STEP_CFGS = ["l16-32-64-K3-b1-12x24x40", "l16-16-32-64-K20-leaky-b3-24x40x64"]
CFG = {c.name: c for c in us.SWEEP}


def loss_cfg(name, k):
    if name == "Tversky":
        return {"name": "Tversky", "include_background": False, "alpha": 0.3, "beta": 0.7, "exponent": 0.75}
    return {"name": "DiceFocal", "include_background": False, "lambda_dice": 1.0, "lambda_focal": 1.0, "gamma": 2.0,
            "class_weights": weights_for(k, 300 + k)}


def ref_fn(name, k):
    lc = loss_cfg(name, k)
    if name == "Tversky":
        return functools.partial(ref_tversky_loss, include_background=False, alpha=f32v(0.3), beta=f32v(0.7),
                                 exponent=0.75)
    return functools.partial(ref_dice_focal_loss, include_background=False, lambda_dice=1.0, lambda_focal=1.0,
                             gamma=2.0, weight=lc["class_weights"])


def configured_net(cfg, precision, loss=None):
    from segmantic_amd.seg.monai_unet import Net
    net = us.make_net(cfg, us.initial_state(cfg), precision)
    net.optimizer = dict(Net.optimizer, **({"loss": loss} if loss is not None else {}))
    return net.to(DEV).train()


def step_result(net, cfg, img, lab):
    """what ``unet_sweep.engine_step`` reads after one ``training_step`` (f32)"""
    res = net.training_step({"image": img.to(DEV), "label": lab.to(DEV)})
    torch.cuda.synchronize()
    logits = net._engine._bufs["logits.t"][..., :cfg.K].float().cpu().permute(0, 4, 1, 2, 3).contiguous()
    return {"logits": logits, "loss": float(res["loss"].cpu()), "loss_bits": res["loss"].detach().cpu().clone(),
            "grads": {n: p.grad.detach().cpu().clone() for n, p in net._model.named_parameters()},
            "state": {k: v.detach().cpu().clone() for k, v in net._model.state_dict().items()},
            "params": {n: p.detach().cpu().clone() for n, p in net._model.named_parameters()}}


@pytest.mark.parametrize("loss", ["Tversky", "DiceFocal"])
@pytest.mark.parametrize("name", STEP_CFGS)
def test_training_step_matches_the_oracle_f32(name, loss):
    from segmantic_amd.seg import losses
    cfg = CFG[name]
    img, lab = us.make_batch(cfg)
    ref = us.oracle_step(cfg, img, lab, loss_fn=ref_fn(loss, cfg.K))
    net = configured_net(cfg, False, loss_cfg(loss, cfg.K))
    got = step_result(net, cfg, img, lab)
    assert type(net.loss_function) is getattr(losses, loss + "Loss")
    bad = us.f32_step_violations(got, ref)
    print(f"{name} {loss}: loss {got['loss']!r} oracle {ref['loss']!r}")
    assert not bad, bad


@pytest.mark.parametrize("loss", ["Tversky", "DiceFocal"])
@pytest.mark.parametrize("precision", [True, "fp16"], ids=["bf16", "fp16"])
def test_three_lowp_steps(precision, loss):
    cfg = CFG[STEP_CFGS[0]]
    img, lab = us.make_batch(cfg)
    net = configured_net(cfg, precision, loss_cfg(loss, cfg.K))
    batch = {"image": img.to(DEV), "label": lab.to(DEV)}
    losses = [float(net.training_step(batch)["loss"].cpu()) for _ in range(3)]
    torch.cuda.synchronize()
    print(f"{loss} {precision}: losses {losses}")
    assert all(math.isfinite(v) for v in losses)
    if precision == "fp16":
        assert net.grad_scaler().skipped_steps() == 0
    assert losses[2] < losses[0]


@pytest.mark.parametrize("loss", ["Tversky", "DiceFocal"])
def test_reconfigured_default_reproduces_the_dice_step_bit_for_bit(loss):
    """a net that trained with one of the new losses and is configured back to the default (weights reloaded) takes the
    very step a fresh default net takes"""
    from segmantic_amd.seg.losses import DiceLoss
    from segmantic_amd.seg.monai_unet import Net
    cfg = CFG[STEP_CFGS[0]]
    img, lab = us.make_batch(cfg)
    fresh = step_result(configured_net(cfg, False), cfg, img, lab)
    net = configured_net(cfg, False, loss_cfg(loss, cfg.K))
    net.training_step({"image": img.to(DEV), "label": lab.to(DEV)})
    torch.cuda.synchronize()
    net.load_state_dict({"_model." + k: v.clone() for k, v in us.initial_state(cfg).items()})
    net.optimizer = dict(Net.optimizer)
    net.configure_optimizers()
    assert type(net.loss_function) is DiceLoss
    again = step_result(net, cfg, img, lab)
    assert torch.equal(again["loss_bits"], fresh["loss_bits"])
    assert torch.equal(again["logits"], fresh["logits"])
    for n in fresh["grads"]:
        assert torch.equal(again["grads"][n], fresh["grads"][n]), n
        assert torch.equal(again["params"][n], fresh["params"][n]), n


def test_validation_value_and_autograd_bridge():
    """the loss objects called as modules: under ``no_grad`` (the value ``validation_step`` logs) and through autograd"""
    from segmantic_amd.seg.losses import DiceFocalLoss, TverskyLoss
    k = 5
    lg, lab = inputs(k)
    for loss, pset, mod in (
            ("tversky", "fp-heavy-focal", TverskyLoss(alpha=f32v(0.7), beta=f32v(0.3), exponent=0.75)),
            ("focal", "weights", None)):
        params = param_set(loss, pset, k)
        if mod is None:
            mod = DiceFocalLoss(lambda_dice=params["lambda_dice"], lambda_focal=params["lambda_focal"],
                                gamma=params["gamma"], weight=params["weight"])
        lq = lg.double().requires_grad_(True)
        ref = ref_loss(loss, lq, lab, params)
        ref.backward()
        want = float(ref.detach())
        x = lg.to(DEV).requires_grad_(True)
        with torch.no_grad():
            v = mod(x, lab.to(DEV))
        assert not v.requires_grad and abs(float(v) - want) < 1e-6 * max(1.0, abs(want))
        out = mod(x, lab.to(DEV))
        (out * 2.0).backward()
        assert abs(float(out.detach()) - want) < 1e-6 * max(1.0, abs(want))
        assert relerr(x.grad.cpu().double(), 2.0 * lq.grad) < 1e-4
    with pytest.raises(ValueError, match="class_weights"):
        DiceFocalLoss(weight=[1.0, 2.0])(lg.to(DEV), lab.to(DEV))
