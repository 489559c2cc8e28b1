"""fp16 storage with dynamic loss scaling on the GPU: the conversion, the fp16 instances of the kernel families
(same family as bf16 for every layer shape), the network against the CPU oracle (fp16 must be markedly closer
than bf16), the loss-scaled training step, the scaler's torch.amp.GradScaler semantics, schedule invariance and
the train-config / predict surface.

fp16 tolerances: output rounding 2^-11 relative plus f32 accumulation-order noise (2e-3 of max |ref|), against
torch-CPU f32 evaluated on fp16-rounded inputs.
"""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle.unet_ref import RefUNet, deterministic_fill_, ref_dice_loss, synthetic_batch  # noqa: E402
from segmantic_amd import ops  # noqa: E402
from segmantic_amd.seg.amp import GradScaler  # noqa: E402
from segmantic_amd.seg.monai_unet import Net  # noqa: E402

DEV = "cuda:0"
F16 = torch.float16
F16_RTOL = 2e-3
CHANNELS, STRIDES = (16, 32, 64, 128, 256), (2, 2, 2, 2)


def to_ndhwc(x_ncdhw, dtype):
    return x_ncdhw.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)


def from_ndhwc(t):
    return t.float().cpu().permute(0, 4, 1, 2, 3).contiguous()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def q(x, dtype):
    return x.to(dtype).float()


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-20))


def build_pair(k, channels=CHANNELS, strides=STRIDES, seed=0):
    ref = RefUNet(3, 1, k, channels, strides)
    deterministic_fill_(ref, seed)
    net = Net(num_classes=k, channels=channels, strides=strides)
    net.load_state_dict({"_model." + kk: v.clone() for kk, v in ref.state_dict().items()})
    return ref, net


# ---------------------------------------------------------------------------------------------- conversion
def test_f32_to_f16_cast_is_bit_identical_to_torch_half():
    """round to nearest even, subnormals kept, > 65504 -> Inf, Inf / NaN kept (never v_cvt_pkrtz, never a saturation)"""
    vals = [0.0, -0.0, 1.0, -2.5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -12, 3.14159265,
            2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 6.0e-8, 5.9e-5, 6.1e-5, 2.0 ** -14 * 0.75, 65504.0, 65519.0,
            65520.0, 65536.0, 1.0e6, -1.0e6, 1.0e-30, float("inf"), float("-inf"), float("nan")]
    g = torch.Generator().manual_seed(7)
    rand = torch.randn(4096 - len(vals), generator=g) * torch.exp2(torch.randint(-30, 20, (4096 - len(vals),),
                                                                                  generator=g).float())
    x = torch.cat([torch.tensor(vals), rand]).reshape(1, 4, 16, 16, 4)       # NDHWC, 4 channels
    src = x.to(DEV)
    dst = torch.empty(src.shape, dtype=F16, device=DEV)
    ops.cast_copy(src, dst)
    back = torch.empty_like(src)
    ops.cast_copy(dst, back)
    torch.cuda.synchronize()
    want = x.half()
    assert torch.equal(dst.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(back.cpu().view(torch.int32), want.float().view(torch.int32))


# ---------------------------------------------------------------------------------------------- kernel families
CONV_CASES = [
    # cin, cout, k, s, spatial (d,h,w), batch
    (16, 16, 3, 1, (8, 12, 20), 2),
    (16, 32, 3, 2, (10, 12, 36), 1),
    (32, 64, 3, 2, (8, 8, 16), 1),
    (128, 256, 1, 1, (4, 4, 4), 2),
    (16, 16, 3, 1, (16, 64, 128), 4),    # z-marching ring (ring3: LDS-DMA ring)
    (16, 16, 3, 1, (33, 60, 120), 2),    # ring, 2 z-segments, ragged extents
    (32, 32, 3, 1, (33, 60, 120), 2),    # ring2, CK=32, two output tiles
    (128, 48, 3, 1, (5, 6, 7), 2),       # K-split
    (64, 64, 3, 1, (9, 10, 40), 2),      # K-split, wide tiles
    (1, 16, 3, 2, (12, 12, 12), 2),      # small-Cin MFMA kernel
    (2, 32, 3, 1, (5, 9, 19), 2),        # small-Cin, stride 1
    (16, 3, 3, 1, (6, 7, 9), 1),         # direct kernel
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv3d_fwd_fp16_matches_torch_and_picks_the_bf16_family(case):
    cin, cout, k, s, sp, n = case
    x = rnd((n, cin) + sp, 1)
    w = rnd((cout, cin, k, k, k), 2, 1.0 / math.sqrt(cin * k ** 3))
    b = rnd((cout,), 3, 0.1)
    ref = F.conv3d(q(x, F16), q(w, F16), b, stride=s, padding=(k - 1) // 2)
    xd = to_ndhwc(x, F16)
    yd = torch.empty((n,) + tuple(ref.shape[2:]) + (cout,), dtype=F16, device=DEV)
    wd, bd = w.to(DEV), b.to(DEV)
    packed = ops.wpack(F16, 0, wd, cin, cout, k) if ops.mfma_ok(cin, cout) else None
    rows = ops.conv3d_stats_rows(xd, yd, k, s)
    stats = torch.zeros((rows, 2, cout), device=DEV)
    ops.conv3d_fwd(xd, yd, packed, wd, 0, bd, k, s, stats=stats)
    torch.cuda.synchronize()
    assert relerr(from_ndhwc(yd), ref) < F16_RTOL
    ssum = stats[:, 0].double().sum(0).cpu()
    rs = ref.double().sum((0, 2, 3, 4))
    assert float((ssum - rs).abs().max()) / (ref.numel() / cout) < 1e-3 * float(ref.abs().max())
    # the same kernel family as bf16 for this layer
    xb, yb = xd.to(torch.bfloat16), yd.to(torch.bfloat16)
    name16, nameb = ops.conv3d_fwd_kernel_name(xd, yd, k, s), ops.conv3d_fwd_kernel_name(xb, yb, k, s)
    assert name16 == nameb.replace("bf16", "f16"), (name16, nameb)
    assert "f16" in name16


@pytest.mark.parametrize("case", [(16, 16, 1, (8, 12, 20), 2), (32, 32, 1, (33, 60, 120), 2),
                                  (64, 64, 1, (9, 10, 40), 2)])
def test_conv3d_dgrad_s1_fp16(case):
    cin, cout, _, sp, n = case
    dy = rnd((n, cout) + sp, 11)
    w = rnd((cout, cin, 3, 3, 3), 12, 1.0 / math.sqrt(cout * 27))
    ref = F.conv_transpose3d(q(dy, F16), q(w, F16), stride=1, padding=1)
    dyd = to_ndhwc(dy, F16)
    dx = torch.empty((n,) + sp + (cin,), dtype=F16, device=DEV)
    wd = w.to(DEV)
    ops.conv3d_fwd(dyd, dx, ops.wpack(F16, 1, wd, cout, cin, 3), wd, 1, None, 3, 1)
    torch.cuda.synchronize()
    assert relerr(from_ndhwc(dx), ref) < F16_RTOL


@pytest.mark.parametrize("case", [(16, 16, 3, 1, (32, 64, 64), 2), (16, 32, 3, 2, (64, 64, 128), 1),
                                  (32, 32, 3, 1, (16, 32, 64), 2), (1, 16, 3, 2, (16, 16, 16), 2)])
def test_conv3d_wgrad_fp16_matches_torch(case):
    """the wave-specialised kernel (k3, 16 input channels per workgroup), the MFMA kernel and the small-Cin one"""
    cin, cout, k, s, sp, n = case
    x = rnd((n, cin) + sp, 331)
    osp = tuple((d + 2 - k) // s + 1 for d in sp)
    dy = rnd((n, cout) + osp, 332)
    w0 = torch.zeros((cout, cin, k, k, k), requires_grad=True)
    b0 = torch.zeros((cout,), requires_grad=True)
    F.conv3d(q(x, F16), w0, b0, stride=s, padding=1).backward(q(dy, F16))
    xd, dyd = to_ndhwc(x, F16), to_ndhwc(dy, F16)
    dw = torch.empty_like(w0, device=DEV)
    db = torch.empty_like(b0, device=DEV)
    ws = torch.empty(ops.conv3d_wgrad_workspace(xd, dyd, k, s), dtype=torch.uint8, device=DEV)
    ops.conv3d_wgrad(xd, dyd, dw, db, k, s, ws)
    torch.cuda.synchronize()
    assert relerr(dw.cpu(), w0.grad) < 5e-5
    assert relerr(db.cpu(), b0.grad) < 5e-5


@pytest.mark.parametrize("k", [3, 16])
def test_softmax_dice_fp16_and_device_loss_scale(k):
    n, sp = 2, (8, 12, 16)
    logits = rnd((n, k) + sp, 21, 3.0)
    lab = torch.randint(0, k, (n, 1) + sp, generator=torch.Generator().manual_seed(22)).float()
    lq = q(logits, F16).requires_grad_(True)
    loss_ref = ref_dice_loss(lq, lab)
    loss_ref.backward()
    from segmantic_amd.seg.losses import DiceLoss, dice_backward, dice_forward
    mod = DiceLoss(to_onehot_y=True, softmax=True)
    lg = to_ndhwc(logits, F16)
    loss = dice_forward(mod._state, lg, lab.to(DEV), mod.smooth_nr, mod.smooth_dr)
    amp = torch.tensor([2.0 ** 16, 0.0, 0.0], device=DEV)
    g = dice_backward(mod._state, lg, 1.0, amp=amp)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * abs(float(loss_ref))
    assert relerr(from_ndhwc(g) / 2.0 ** 16, lq.grad) < F16_RTOL


# ---------------------------------------------------------------------------------------------- network accuracy
@pytest.mark.parametrize("size", [64, 128])
def test_fp16_network_is_closer_to_the_oracle_than_bf16(size, record_property):
    """the inputs of test_bf16_training_forward_vs_oracle_at_benchmark_scale: one patch, 16 labels,
    training-mode BatchNorm.  fp16 carries 3 more mantissa bits: its error must be below a quarter of bf16's
    (emulation: an eighth), its argmax agreement at least bf16's.  Whether fp16 meets north_star's 1e-3 is
    recorded."""
    k = 16
    ref, net = build_pair(k)
    img, lab = synthetic_batch(1, size, k, seed=11)
    ref.train()
    with torch.no_grad():
        out_ref = ref(img)
    net.to(DEV).train()
    res = {}
    for mode in (True, "fp16"):
        net.mixed_precision = mode
        with torch.no_grad():
            out = net(img.to(DEV)).float().cpu()
        torch.cuda.synchronize()
        res[mode] = (relerr(out, out_ref), float((torch.argmax(out, 1) == torch.argmax(out_ref, 1)).float().mean()))
    (eb, ab), (eh, ah) = res[True], res["fp16"]
    print(f"\n@ {size}^3 vs oracle: bf16 rel. logit error {eb:.3e}, argmax {ab:.5f}; fp16 {eh:.3e}, argmax {ah:.5f}; "
          f"fp16 meets 1e-3: {eh < 1e-3}")
    for name, v in (("bf16_rel_err", eb), ("bf16_argmax_agreement", ab), ("fp16_rel_err", eh),
                    ("fp16_argmax_agreement", ah)):
        record_property(f"{name}_{size}", v)
    assert eh < 0.25 * eb, (eh, eb)
    assert ah >= ab, (ah, ab)


def test_fp16_eval_forward_uses_the_fused_decoder_top_and_matches_the_oracle():
    k = 16
    ref, net = build_pair(k)
    img, _ = synthetic_batch(1, 64, k, seed=3)
    ref.eval()
    with torch.no_grad():
        out_ref = ref(img)
    net.to(DEV).eval()
    net.mixed_precision = "fp16"
    with torch.no_grad():
        out = net(img.to(DEV)).float().cpu()
    torch.cuda.synchronize()
    assert net._engine.dtype == F16 and net._engine.eval_top_fused
    assert relerr(out, out_ref) < 3e-3


# ---------------------------------------------------------------------------------------------- training step
def test_fp16_training_step_matches_the_oracle_step():
    """64^3: loss, unscaled gradients (flat_grad / scale), BatchNorm running statistics, post-Adam weights"""
    k = 16
    ref, net = build_pair(k)
    img, lab = synthetic_batch(1, 64, k, seed=11)
    ref.train()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    out_ref = ref(img)
    opt.zero_grad()
    loss_ref = ref_dice_loss(out_ref, lab)
    loss_ref.backward()
    grads_ref = {n: p.grad.clone() for n, p in ref.named_parameters()}
    opt.step()
    net.to(DEV).train()
    net.mixed_precision = "fp16"
    eng = net._engine_for()
    res = net.training_step({"image": img.to(DEV), "label": lab.to(DEV)})
    torch.cuda.synchronize()
    scaler = net.grad_scaler()
    assert scaler.skipped_steps() == 0 and scaler.get_scale() == 2.0 ** 16
    loss = float(res["loss"].cpu())                           # unscaled
    assert abs(loss - float(loss_ref.detach())) < 1e-4 * abs(float(loss_ref.detach()))
    # p.grad: views of the (scaled) gradient arena.  The Dice gradient is mostly subnormal in fp16 at the default
    # scale, so the gate is normwise per weight tensor (PReLU slopes and biases are single sums with heavy
    # cancellation: covered by the arena-wide norm) and over the whole arena
    gmax = max(float(g.abs().max()) for g in grads_ref.values())
    bad, num, den = [], 0.0, 0.0
    for n, p in net._model.named_parameters():
        g, gr = p.grad.cpu().double() / scaler.get_scale(), grads_ref[n].double()
        num, den = num + float(((g - gr) ** 2).sum()), den + float((gr ** 2).sum())
        if n.endswith(".A.weight") or n.endswith(".bias"):
            continue
        e = float((g - gr).norm() / gr.norm().clamp(min=1e-30))
        if e > 0.1:
            bad.append((n, e))
    print(f"\nfp16 step: arena gradient rel. error {math.sqrt(num / den):.3e}")
    assert math.sqrt(num / den) < 3e-2
    assert not bad, bad[:8]
    sd_ref = ref.state_dict()
    for kk, v in net._model.state_dict().items():
        if "running" in kk:
            assert relerr(v.cpu(), sd_ref[kk]) < 2e-3, kk
    for n, p in net._model.named_parameters():
        gr = grads_ref[n]
        mask = gr.abs() > 1e-2 * gmax            # Adam's first step is lr * sign(g) where g is well above noise
        if mask.any():
            d = (dict(ref.named_parameters())[n].detach() - p.detach().cpu())[mask].abs().max()
            assert float(d) < 5e-6, (n, float(d))


def test_overflowing_step_is_skipped_bit_for_bit_and_the_scale_backs_off():
    k = 16
    _, net = build_pair(k)
    img, lab = synthetic_batch(1, 64, k, seed=11)
    batch = {"image": img.to(DEV), "label": lab.to(DEV)}
    net.to(DEV).train()
    net.mixed_precision = "fp16"
    net.training_step(batch)                                  # one applied step: moments are non-zero
    opt = net.optimizers()
    before = [t.clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq)]
    steps_before = opt.applied_steps()
    running = {kk: v.clone() for kk, v in net._model.state_dict().items() if "running_mean" in kk}
    net._scaler = GradScaler(DEV, init_scale=2.0 ** 64)
    net.training_step(batch)
    torch.cuda.synchronize()
    for a, b in zip(before, (opt.flat, opt.exp_avg, opt.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert opt.applied_steps() == steps_before
    assert net._scaler.get_scale() == 2.0 ** 63 and net._scaler.get_growth_tracker() == 0
    assert net._scaler.skipped_steps() == 1
    # BatchNorm running statistics still move on a skipped step, as in torch
    assert any(not torch.equal(running[kk], v) for kk, v in net._model.state_dict().items() if kk in running)


def test_scale_tracker_and_skips_follow_torch_grad_scaler():
    """growth interval 3 over a fixed found-inf pattern: scale and growth tracker after every step equal
    torch.amp.GradScaler's; a step with an Inf / NaN gradient leaves params, moments and the step count bit-untouched"""
    from segmantic_amd.seg.optim import FlatAdam
    pattern = [True, False, False, False, True, False, False, False, False, False, False, True, False, False]
    n = 4099
    g = torch.Generator().manual_seed(9)
    flat = torch.randn(n, generator=g).to(DEV)
    grad_u = (torch.randn(n, generator=g) * 1e-3).to(DEV)
    grad = torch.empty_like(grad_u)
    opt = FlatAdam(flat, grad, lr=1e-3)
    scaler = GradScaler(DEV, init_scale=2.0 ** 16, growth_interval=3)
    ours = []
    for i, inf in enumerate(pattern):
        grad.copy_(grad_u * scaler.amp[0])
        if inf:
            grad[(97 * i) % n] = float("nan") if i % 2 else float("inf")
        before = [t.clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq)]
        steps = opt.applied_steps()
        scaler.check(grad)
        opt.step_amp(scaler)
        scaler.update(opt)
        if inf:
            assert all(torch.equal(a, b) for a, b in zip(before, (opt.flat, opt.exp_avg, opt.exp_avg_sq)))
            assert opt.applied_steps() == steps
        else:
            assert opt.applied_steps() == steps + 1 and not torch.equal(before[0], opt.flat)
        ours.append((scaler.get_scale(), scaler.get_growth_tracker()))
    assert scaler.skipped_steps() == sum(pattern)
    p = torch.zeros(4, device=DEV, requires_grad=True)
    sgd = torch.optim.SGD([p], lr=0.0)
    ts = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16, growth_interval=3)
    theirs = []
    for inf in pattern:
        sgd.zero_grad()
        ts.scale(torch.ones((), device=DEV))
        p.grad = torch.full_like(p, float("inf") if inf else 1.0)
        ts.step(sgd)
        ts.update()
        theirs.append((float(ts.get_scale()), int(ts._get_growth_tracker())))
    assert ours == theirs, (ours, theirs)


def test_gated_adam_equals_torch_adam_on_the_unscaled_gradient():
    """finite gradients: the loss-scaled Adam update over three steps equals torch.optim.Adam on grad / scale"""
    from segmantic_amd.seg.optim import FlatAdam
    n = 50000
    g = torch.Generator().manual_seed(13)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 1e-3 for _ in range(3)]
    flat, grad = p0.clone().to(DEV), torch.empty(n, device=DEV)
    opt = FlatAdam(flat, grad, lr=1e-3)
    scaler = GradScaler(DEV)
    pt = p0.clone().requires_grad_(True)
    topt = torch.optim.Adam([pt], lr=1e-3)
    for gr in grads:
        grad.copy_(gr.to(DEV) * 2.0 ** 16)
        scaler.check(grad)
        opt.step_amp(scaler)
        scaler.update(opt)
        pt.grad = gr.clone()
        topt.step()
    torch.cuda.synchronize()
    assert float((flat.cpu() - pt.detach()).abs().max()) < 1e-6


@pytest.mark.parametrize("optimizer", [{"optimizer": "SGD", "lr": 1e-2, "momentum": 0.9},
                                       {"optimizer": "AdaBelief", "lr": 1e-3}])
def test_gated_sgd_and_adabelief_match_their_plain_updates(optimizer):
    """with a finite gradient the loss-scaled updates equal the plain kernels on the unscaled gradient"""
    from segmantic_amd.seg.optim import make_optimizer
    n = 100003
    g = torch.Generator().manual_seed(5)
    flat0 = torch.randn(n, generator=g).to(DEV)
    grad = (torch.randn(n, generator=g) * 1e-3).to(DEV)
    scaler = GradScaler(DEV, init_scale=2.0 ** 10)
    fa, fb = flat0.clone(), flat0.clone()
    ga, gb = grad * 2.0 ** 10, grad.clone()
    oa, ob = make_optimizer(optimizer, fa, ga), make_optimizer(optimizer, fb, gb)
    for _ in range(3):
        scaler.check(ga)
        oa.step_amp(scaler)
        scaler.update(oa)
        ob.step()
    torch.cuda.synchronize()
    assert oa.applied_steps() == 3
    assert torch.equal(fa, fb)


# ---------------------------------------------------------------------------------------------- schedules
def test_fp16_serial_and_overlapped_schedules_agree():
    K = 16
    img, lab = synthetic_batch(2, 64, K, seed=5)
    batch = {"image": img.to(DEV), "label": lab.to(DEV)}

    def run(overlap):
        _, net = build_pair(K)
        net.to(DEV).train()
        net.mixed_precision = "fp16"
        eng = net._engine_for(batch["image"])
        eng.overlap_wgrad = overlap
        net.training_step(batch)
        torch.cuda.synchronize()
        return eng.flat_grad.clone(), eng.flat.clone()

    g0, w0 = run(False)
    g1, w1 = run(True)
    d = float((g0 - g1).norm() / g0.norm())
    print(f"\nfp16 serial vs overlapped: gradient arena rel. difference {d:.3e}, bit-identical {torch.equal(g0, g1)}")
    assert d < 1e-3


# ---------------------------------------------------------------------------------------------- end to end
def test_sliding_window_inference_with_an_fp16_engine():
    from segmantic_amd.seg.inferers import sliding_window_inference
    k = 3
    _, net = build_pair(k, (16, 32, 64), (2, 2))
    img, _ = synthetic_batch(1, 40, k, seed=8)
    net.to(DEV).eval()
    outs = {}
    for mode in (False, "fp16"):
        net.mixed_precision = mode
        with torch.no_grad():
            outs[mode] = sliding_window_inference(img.to(DEV), (32, 32, 32), 2, net, overlap=0.25).float().cpu()
    torch.cuda.synchronize()
    assert relerr(outs["fp16"], outs[False]) < 5e-3


def test_cli_train_config_fp16_then_predict(tmp_path):
    import yaml
    from typer.testing import CliRunner

    from segmantic_amd.commands.monai_unet_cli import app
    from segmantic_amd.data.nifti import read_nifti, write_nifti
    root = tmp_path / "data"
    (root / "image").mkdir(parents=True)
    (root / "label").mkdir()
    A = np.diag([1.0, 1.0, 1.0, 1.0])
    for i in range(4):
        img, lab = synthetic_batch(1, 24, 3, seed=20 + i)
        write_nifti(root / "image" / f"c{i}.nii.gz", (img[0, 0].numpy() * 100 + 300).astype(np.float32).transpose(2, 1, 0), A)
        write_nifti(root / "label" / f"c{i}.nii.gz", lab[0, 0].numpy().astype(np.uint8).transpose(2, 1, 0), A)
    dl = {"labels": {"1": "a", "2": "b"},
          "training": [{"image": f"image/c{i}.nii.gz", "label": f"label/c{i}.nii.gz"} for i in range(3)],
          "validation": [{"image": "image/c3.nii.gz", "label": "label/c3.nii.gz"}],
          "test": ["image/c3.nii.gz"]}
    (root / "dataset.json").write_text(json.dumps(dl))
    dl["test"] = [{"image": "image/c3.nii.gz", "label": "label/c3.nii.gz"}]      # predict's decathlon loader
    (root / "predict.json").write_text(json.dumps(dl))
    out = tmp_path / "results"
    cfg = {"datalist": str(root / "dataset.json"), "output_dir": str(out), "spatial_size": [16, 16, 16],
           "channels": [16, 32, 64], "strides": [2, 2], "max_epochs": 2, "mixed_precision": "fp16",
           "num_samples": 2, "gpu_ids": [0], "optimizer": {"optimizer": "Adam", "lr": 1e-3, "amsgrad": False}}
    (tmp_path / "cfg.yml").write_text(yaml.safe_dump(cfg))
    runner = CliRunner()
    res = runner.invoke(app, ["train-config", "-c", str(tmp_path / "cfg.yml")])
    assert res.exit_code == 0, (res.output, res.exception)
    dice = [float(m) for m in __import__("re").findall(r"current epoch: \d+ mean val dice: ([-0-9.eE+naif]+)", res.output)]
    assert len(dice) >= 1 and all(np.isfinite(dice)), res.output
    ckpts = sorted(out.glob("epoch=*-val_loss=*-val_dice=*.ckpt"))
    assert ckpts
    res = runner.invoke(app, ["predict", "-d", str(root / "predict.json"), "-m", str(ckpts[-1]), "-r",
                              str(tmp_path / "pred"), "--gpu-ids", "0"])
    assert res.exit_code == 0, (res.output, res.exception)
    pred, _ = read_nifti(tmp_path / "pred" / "c3.nii.gz")
    assert pred.shape == (24, 24, 24) and pred.max() <= 2


def test_convergence_trajectory_holds_under_fp16(golden_dir, record_property):
    """the committed 30-step trajectory (tests/golden/convergence_c1.json) at the gate of its bf16 check"""
    g = json.loads((golden_dir / "convergence_c1.json").read_text())
    cfg, runs = g["config"], g["runs"]
    K, S, B = cfg["labels"], cfg["patch"], cfg["batch"]
    ref, net = build_pair(K)
    net.to(DEV)
    net.mixed_precision = "fp16"
    net.optimizer = dict(Net.optimizer, lr=cfg["lr"])
    net.train()
    val = [synthetic_batch(1, S, K, seed=900 + i) for i in range(cfg["val_volumes"])]
    out = {"train_loss": [], "val_dice": []}
    for step in range(cfg["steps"]):
        img, lab = synthetic_batch(B, S, K, seed=100 + step)
        res = net.training_step({"image": img.to(DEV), "label": lab.to(DEV)})
        out["train_loss"].append(float(res["loss"].cpu()))
        if (step + 1) % cfg["validate_every"] == 0:
            for img_v, lab_v in val:
                net.validation_step({"image": img_v.to(DEV), "label": lab_v.to(DEV)})
            out["val_dice"].append(float(net.dice_metric.aggregate().item()))
            net.dice_metric.reset()
            net.validation_step_outputs.clear()
            net.train()
    bd = [min(abs(h - r["val_dice"][i]) for r in runs) for i, h in enumerate(out["val_dice"])]
    bt = max(abs(h - runs[0]["train_loss"][i]) / runs[0]["train_loss"][i] for i, h in enumerate(out["train_loss"]))
    print(f"\nconvergence fp16: |val_dice - oracle| = {bd}, train-loss rel. {bt:.2e}, "
          f"skipped steps {net.grad_scaler().skipped_steps()}")
    record_property("fp16_val_dice_dev", bd)
    assert len(bd) == 3
    assert max(bd) < 5e-2 and bt < 2e-2
