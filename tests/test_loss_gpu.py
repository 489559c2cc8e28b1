"""The Dice + cross-entropy loss kernels and the configurable training objective on the GPU.

Op level: ``segmi_softmax_dice_ce_fwd / _bwd / _bwd_amp`` against the float64 reference of tests/helpers/loss_ref.py on
the quantised logits (the method and the gradient / bias gates of ``tests/test_ops_gpu.py::test_softmax_dice``; the loss
gate is that test's 1e-6 * max(1, |loss|) in f32 and the 1e-4 * |loss| of ``unet_sweep.f32_step_violations`` for the
16-bit paths, which may use the hardware log).  Shape: n = 3, 17 x 24 x 33 = 13 464 voxels per sample = one full
8192-voxel chunk + one ragged chunk whose length is no multiple of the unrolled trip; the batch of 3 shows that the
cross-entropy normaliser W is batch-global.  K in {2, 3, 4, 5, 16, 32, 64} reaches every KMAX, full and ragged, with
vector and scalar loads.

Whole step: ``Net.training_step`` with a configured DiceCE loss against ``unet_sweep.oracle_step`` with the same loss.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from tests.helpers import lowp_bounds as lb  # noqa: E402
from tests.helpers import unet_sweep as us  # noqa: E402
from tests.helpers.loss_ref import ref_dice_ce_loss  # noqa: E402

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = {"f32": F32, "bf16": BF16, "fp16": F16}
N, SP = 3, (17, 24, 33)
KS = [2, 3, 4, 5, 16, 32, 64]


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


def param_set(name, k):
    """keyword arguments of the loss (reference and kernel alike)"""
    base = dict(include_background=True, lambda_dice=1.0, lambda_ce=1.0, weight=None)
    if name == "nobg":
        base.update(include_background=False)
    elif name == "weights":
        base.update(weight=weights_for(k, 100 + k), lambda_dice=0.5, lambda_ce=2.0)
    elif name == "zero-weight":
        base.update(weight=weights_for(k, 200 + k, zero_at=k // 2))
    elif name == "ce-only":
        base.update(lambda_dice=0.0)
    else:
        assert name in ("defaults", "absent-class")
    return base


PSETS = ["defaults", "nobg", "weights", "zero-weight", "ce-only", "absent-class"]


@functools.lru_cache(maxsize=None)
def inputs(k, pset):
    lg = rnd((N, k) + SP, 61 + k, 3.0)
    lab = torch.randint(0, k, (N, 1) + SP, generator=torch.Generator().manual_seed(62 + k)).float()
    if pset == "absent-class":             # class k-1 does not occur in sample 1
        lab[1] = torch.where(lab[1] == k - 1, torch.zeros_like(lab[1]), lab[1])
        assert not bool((lab[1] == k - 1).any()) and bool((lab[0] == k - 1).any())
    return lg, lab


@functools.lru_cache(maxsize=None)
def truth(k, dt, pset):
    """float64 reference on the logits rounded to the storage type: (loss, dlogits, bias sums), computed once"""
    lg, lab = inputs(k, pset)
    lq = lg.to(DTYPES[dt]).double().requires_grad_(True)
    loss = ref_dice_ce_loss(lq, lab, **param_set(pset, k))
    loss.backward()
    return float(loss.detach()), lq.grad.detach(), lq.grad.detach().sum((0, 2, 3, 4))


def run_kernels(ld_, labd, params, grad_scale=1.0, bias=True, amp=None, ld=None):
    """forward + backward of the new entry points -> (loss f32[1], dlogits, bias_grad or None), on the device"""
    n, k = ld_.shape[0], ld_.shape[4]
    part = torch.empty((ops.dice_ce_chunks(ld_), n, 4, k), device=DEV)
    coef = torch.empty((n, 3, k), device=DEV)
    out = torch.empty(1, device=DEV)
    w = params["weight"]
    wd = None if w is None else torch.tensor(w, dtype=F32, device=DEV)
    ops.softmax_dice_ce_fwd(ld_, labd, part, coef, out, lambda_dice=params["lambda_dice"],
                            lambda_ce=params["lambda_ce"], include_background=params["include_background"],
                            class_weight=wd)
    dl = empty_like_rows(ld_, ld)
    db = torch.empty(k, device=DEV) if bias else None
    kw = dict(scratch=part if bias else None, bias_grad=db)
    if amp is not None:
        ops.softmax_dice_ce_bwd_amp(ld_, labd, coef, amp, dl, **kw)
    else:
        ops.softmax_dice_ce_bwd(ld_, labd, coef, grad_scale, dl, **kw)
    torch.cuda.synchronize()
    return out, dl, db


def check_parity(k, dt, pset, ld=None):
    dtype = DTYPES[dt]
    lg, lab = inputs(k, pset)
    loss_ref, grad_ref, db_ref = truth(k, dt, pset)
    ld_ = to_ndhwc(lg, dtype, ld)
    labd = lab.to(DEV).reshape(-1).contiguous()
    out, dl, db = run_kernels(ld_, labd, param_set(pset, k), ld=ld)
    got = float(out.cpu())
    gerr = relerr(from_ndhwc(dl).double(), grad_ref)
    berr = float((db.cpu().double() - db_ref).abs().max())
    rtol = 1e-4 if dtype == F32 else 1e-2
    blim = 1e-5 + rtol * float(grad_ref.abs().sum() / k)
    llim = 1e-6 * max(1.0, abs(loss_ref)) if dtype == F32 else 1e-4 * abs(loss_ref)
    print(f"K={k} {dt} {pset} ld={ld}: loss {got!r} ref {loss_ref!r} |d| {abs(got - loss_ref):.3g} (limit {llim:.3g}); "
          f"dlogits rel {gerr:.3g} (limit {rtol:g}); bias {berr:.3g} (limit {blim:.3g})")
    assert abs(got - loss_ref) < llim
    assert gerr < rtol
    assert berr < blim


# ------------------------------------------------------------------------------------------------ op-level parity
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("k", KS)
def test_dice_ce_matches_the_float64_reference(k, dt, pset):
    check_parity(k, dt, pset)


@pytest.mark.parametrize("pset", ["defaults", "weights", "nobg"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_dice_ce_on_a_padded_class_row(dt, pset):
    """K = 5 real classes in rows of 16 (the engine's kpad layout): logits and dlogits are views with row stride 16"""
    check_parity(5, dt, pset, ld=16)


def test_padded_dlogits_leave_the_padding_untouched():
    lg, lab = inputs(5, "defaults")
    ld_ = to_ndhwc(lg, BF16, 16)
    _, dl, _ = run_kernels(ld_, lab.to(DEV).reshape(-1).contiguous(), param_set("defaults", 5), ld=16)
    full = dl._base if dl._base is not None else dl
    assert tuple(full.shape[-1:]) == (16,) and not bool(full[..., 5:].any())


# ------------------------------------------------------------------------------------------------ edge cases
def test_true_class_200_below_the_maximum_contributes_200():
    """f32, K = 3: class 0 at 200, the others (among them every voxel's true class) at 0: exp(-200) is 0 in f32, so a
    log of the stored probability would give Inf; CE must be 200 and every dlogit finite"""
    lg = torch.zeros((N, 3) + SP)
    lg[:, 0] = 200.0
    lab = torch.randint(1, 3, (N, 1) + SP, generator=torch.Generator().manual_seed(7)).float()
    ld_, labd = to_ndhwc(lg, F32), lab.to(DEV).reshape(-1).contiguous()
    for params in (dict(include_background=True, lambda_dice=0.0, lambda_ce=1.0, weight=None),
                   param_set("defaults", 3)):
        ref = float(ref_dice_ce_loss(lg.double(), lab, **params))
        out, dl, db = run_kernels(ld_, labd, params)
        got = float(out.cpu())
        print(f"far true class: loss {got!r} ref {ref!r}")
        assert abs(got - ref) < 1e-6 * max(1.0, abs(ref))
        if params["lambda_dice"] == 0.0:
            assert abs(got - 200.0) < 1e-6 * 200.0
        assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(db).all())
    lq = lg.double().requires_grad_(True)
    ref_dice_ce_loss(lq, lab, **param_set("defaults", 3)).backward()
    assert relerr(from_ndhwc(dl).double(), lq.grad) < 1e-4


def test_all_zero_weights_give_nan_as_torch_does():
    lg, lab = inputs(3, "defaults")
    params = dict(include_background=True, lambda_dice=1.0, lambda_ce=1.0, weight=[0.0, 0.0, 0.0])
    assert math.isnan(float(ref_dice_ce_loss(lg.double(), lab, **params)))
    out, _, _ = run_kernels(to_ndhwc(lg, F32), lab.to(DEV).reshape(-1).contiguous(), params)
    assert math.isnan(float(out.cpu()))


def test_out_of_range_labels_count_for_nothing():
    """labels outside [0, K) are in neither CE nor W (nor the Dice target sums): the loss equals the reference's on
    logits and labels with those voxels' cross-entropy left out"""
    k = 4
    lg, lab = inputs(k, "defaults")
    lab = lab.clone()
    bad = torch.rand(lab.shape, generator=torch.Generator().manual_seed(3)) < 0.1
    lab[bad] = torch.where(torch.rand(int(bad.sum()), generator=torch.Generator().manual_seed(4)) < 0.5, -1.0, float(k))
    w = weights_for(k, 9)
    lq = lg.double()
    keep = ~bad[:, 0]
    logp = torch.log_softmax(lq, 1)
    y = lab[:, 0].long().clamp(0, k - 1)
    wt = torch.tensor(w, dtype=torch.float64)
    nll = -logp.gather(1, y[:, None])[:, 0]
    ce = float((wt[y] * nll)[keep].sum() / wt[y][keep].sum())
    out, dl, _ = run_kernels(to_ndhwc(lg, F32), lab.to(DEV).reshape(-1).contiguous(),
                             dict(include_background=True, lambda_dice=0.0, lambda_ce=1.0, weight=w))
    assert abs(float(out.cpu()) - ce) < 1e-6 * max(1.0, abs(ce))
    g = from_ndhwc(dl)
    assert not bool(g.permute(0, 2, 3, 4, 1)[bad[:, 0]].any())          # no cross-entropy gradient at those voxels


# ------------------------------------------------------------------------------------------------ no regression
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("k", [3, 16])
def test_lambda_ce_zero_reproduces_the_dice_kernels_bit_for_bit(k, dt):
    lg, lab = inputs(k, "defaults")
    ld_ = to_ndhwc(lg, DTYPES[dt])
    labd = lab.to(DEV).reshape(-1).contiguous()
    part = torch.empty((N, ops.dice_chunks(ld_), 3, k), device=DEV)
    coef = torch.empty((N, 2, k), device=DEV)
    loss0 = torch.empty(1, device=DEV)
    ops.softmax_dice_fwd(ld_, labd, part, coef, loss0)
    dl0, db0 = torch.empty_like(ld_), torch.empty(k, device=DEV)
    ops.softmax_dice_bwd(ld_, labd, coef, 1.0, dl0, scratch=part, bias_grad=db0)
    torch.cuda.synchronize()
    loss1, dl1, db1 = run_kernels(ld_, labd, dict(include_background=True, lambda_dice=1.0, lambda_ce=0.0, weight=None))
    assert torch.equal(loss1, loss0)
    assert torch.equal(dl1, dl0)
    # the bias sums add the same stored values; the compiler may fuse the last multiply of an addend into the running
    # sum in one instantiation and not in the other, so each addend differs by at most one f32 rounding (2^-24 of it)
    lim = 2.0 ** -22 * float(dl0.float().abs().sum((0, 1, 2, 3)).max())
    assert float((db1 - db0).abs().max()) <= lim


# ------------------------------------------------------------------------------------------------ determinism, fusion
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("k", [5, 16])
def test_two_calls_are_bit_identical_and_bias_fusion_changes_nothing(k, dt):
    lg, lab = inputs(k, "weights")
    ld_ = to_ndhwc(lg, DTYPES[dt])
    labd = lab.to(DEV).reshape(-1).contiguous()
    params = param_set("weights", k)
    a = run_kernels(ld_, labd, params)
    b = run_kernels(ld_, labd, params)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = run_kernels(ld_, labd, params, bias=False)
    assert c[2] is None and torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


# ------------------------------------------------------------------------------------------------ loss-scaled backward
@pytest.mark.parametrize("k", [3, 16])
def test_loss_scaled_backward_stores_each_dlogit(k):
    """fp16 at scale 2^16, element by element against the f32 kernel's gradient on the same fp16 logits times the
    scale: the bound and method of ``test_softmax_dice_backward_amp_stores_each_dlogit``"""
    lg, lab = inputs(k, "weights")
    lg = lg.half().float()
    labd = lab.to(DEV).reshape(-1).contiguous()
    params = param_set("weights", k)
    scale = 2.0 ** 16
    _, ref, ref_b = run_kernels(to_ndhwc(lg, F32), labd, params)
    amp = torch.tensor([scale, 0.0, 0.0], device=DEV)
    _, got, got_b = run_kernels(to_ndhwc(lg, F16), labd, params, amp=amp)
    ref = from_ndhwc(ref).double() * scale
    r = lb.ratio(from_ndhwc(got).double(), ref, ref.abs())
    print(f"K={k}: worst ratio {float(r.max()):.3g}")
    assert float(r.max()) <= 1.0
    # the fused bias sums follow the stored gradient: the bias-sum bound of test_softmax_dice (16-bit), at this scale
    berr = float((got_b.cpu().double() - ref_b.cpu().double() * scale).abs().max())
    assert berr < 1e-5 + 1e-2 * float(ref.abs().sum() / k)


# ------------------------------------------------------------------------------------------------ whole step
STEP_CFGS = ["l16-32-64-K3-b1-12x24x40", "l16-16-32-64-K20-leaky-b3-24x40x64"]
CFG = {c.name: c for c in us.SWEEP}


def loss_cfg(k):
    return {"name": "DiceCE", "include_background": False, "lambda_dice": 1.0, "lambda_ce": 1.0,
            "class_weights": weights_for(k, 300 + k)}


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


@pytest.mark.parametrize("name", STEP_CFGS)
def test_training_step_with_dice_ce_matches_the_oracle_f32(name):
    from segmantic_amd.seg.losses import DiceCELoss
    cfg = CFG[name]
    img, lab = us.make_batch(cfg)
    lc = loss_cfg(cfg.K)
    ref = us.oracle_step(cfg, img, lab, loss_fn=functools.partial(
        ref_dice_ce_loss, include_background=False, lambda_dice=1.0, lambda_ce=1.0, weight=lc["class_weights"]))
    net = configured_net(cfg, False, lc)
    got = step_result(net, cfg, img, lab)
    assert type(net.loss_function) is DiceCELoss and net.loss_function.weight == lc["class_weights"]
    bad = us.f32_step_violations(got, ref)
    print(f"{name}: loss {got['loss']!r} oracle {ref['loss']!r}")
    assert not bad, bad


@pytest.mark.parametrize("precision", [True, "fp16"], ids=["bf16", "fp16"])
def test_three_lowp_steps_with_dice_ce(precision):
    cfg = CFG[STEP_CFGS[0]]
    img, lab = us.make_batch(cfg)
    net = configured_net(cfg, precision, loss_cfg(cfg.K))
    batch = {"image": img.to(DEV), "label": lab.to(DEV)}
    losses = [float(net.training_step(batch)["loss"].cpu()) for _ in range(3)]
    torch.cuda.synchronize()
    print(f"{precision}: losses {losses}")
    assert all(math.isfinite(v) for v in losses)
    if precision == "fp16":
        assert net.grad_scaler().skipped_steps() == 0
    assert losses[2] < losses[0]


def test_reconfigured_default_reproduces_the_dice_step_bit_for_bit():
    """a net that trained with DiceCE and is configured back to the default (weights reloaded) takes the very step a
    fresh default net takes: configuring a loss leaves no state behind"""
    from segmantic_amd.seg.losses import DiceLoss
    from segmantic_amd.seg.monai_unet import Net
    cfg = CFG[STEP_CFGS[0]]
    img, lab = us.make_batch(cfg)
    fresh = step_result(configured_net(cfg, False), cfg, img, lab)
    net = configured_net(cfg, False, loss_cfg(cfg.K))
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


def test_validation_loss_and_autograd_bridge_follow_the_configured_loss():
    """``DiceCELoss`` / ``DiceLoss(include_background=False)`` called as modules: under ``no_grad`` (the value
    ``validation_step`` logs) and through autograd (external loops), against the reference"""
    from segmantic_amd.seg.losses import DiceCELoss, DiceLoss
    k = 5
    lg, lab = inputs(k, "weights")
    params = param_set("weights", k)
    lq = lg.double().requires_grad_(True)
    ref = ref_dice_ce_loss(lq, lab, **params)
    ref.backward()
    mod = DiceCELoss(include_background=True, lambda_dice=params["lambda_dice"], lambda_ce=params["lambda_ce"],
                     weight=params["weight"])
    x = lg.to(DEV).requires_grad_(True)
    with torch.no_grad():
        v = mod(x, lab.to(DEV))
    assert not v.requires_grad and abs(float(v) - float(ref)) < 1e-6 * max(1.0, abs(float(ref)))
    out = mod(x, lab.to(DEV))
    (out * 2.0).backward()
    assert abs(float(out) - float(ref)) < 1e-6 * max(1.0, abs(float(ref)))
    assert relerr(x.grad.cpu().double(), 2.0 * lq.grad) < 1e-4
    # the public ``weight`` attribute may be edited between calls: the kernels follow it, and it is validated again
    w2 = weights_for(k, 77)
    mod.weight = w2
    with torch.no_grad():
        v = mod(x, lab.to(DEV))
    want = float(ref_dice_ce_loss(lg.double(), lab, **dict(params, weight=w2)))
    assert abs(float(v) - want) < 1e-6 * max(1.0, abs(want)) and abs(want - float(ref)) > 1e-3
    mod.weight = [-1.0] + w2[1:]
    with pytest.raises(ValueError, match="class_weights"):
        mod(x, lab.to(DEV))
    d = DiceLoss(include_background=False)
    with torch.no_grad():
        v = d(lg.to(DEV), lab.to(DEV))
    want = float(ref_dice_ce_loss(lg.double(), lab, include_background=False, lambda_ce=0.0))
    assert abs(float(v) - want) < 1e-6 * max(1.0, abs(want))
    with pytest.raises(ValueError, match="class_weights"):
        DiceCELoss(weight=[1.0, 2.0])(lg.to(DEV), lab.to(DEV))
