"""Host side of the UNet sweep (tests/helpers/unet_sweep.py): every configuration is legal, well conditioned (plain
torch f32 stays within a quarter of every f32 gate against the float64 oracle), and the gates fail for six deliberately
wrong oracles -- so a pass of tests/test_unet_sweep_gpu.py means something."""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle.unet_ref import RefUNet, ref_dice_loss
from segmantic_amd.seg.monai_unet import Net
from tests.helpers import unet_sweep as us


# ------------------------------------------------------------------------------------------------ legality
def test_sweep_covers_what_it_must():
    cfgs = us.SWEEP
    assert {1, 3, 8} <= {c.batch for c in cfgs}
    assert {1, 2, 4} <= {c.cin for c in cfgs}
    assert {2, 3, 16, 20, 33} <= {c.K for c in cfgs}
    ladders = {tuple(c.channels) for c in cfgs}
    assert {(8, 16, 32), (16, 16, 32, 64), (32, 64, 128), us.DEFAULT5} <= ladders
    assert sum(c.act == "RELU" for c in cfgs) == 1 and sum(c.act == "LEAKYRELU" for c in cfgs) == 1
    assert sum(c.dims == 2 for c in cfgs) == 1
    assert any(len(set(c.spatial)) == 3 for c in cfgs)
    # one total stride in one dimension, several in another
    assert any(min(c.spatial) == us.total_stride(c) and max(c.spatial) >= 2 * us.total_stride(c) for c in cfgs)
    # size limit: 64 x 64 x 96 voxels per sample; ONE case may reach 128 in a dimension
    big = [c for c in cfgs if max(c.spatial) > 96]
    assert len(big) <= 1 and all(max(c.spatial) <= 128 for c in big)
    for c in cfgs:
        if c not in big:
            assert torch.Size(c.spatial).numel() <= 64 * 64 * 96, c.name
    assert len(us.UNREACHABLE) <= 3 and all(len(r.split()) > 8 for r in us.UNREACHABLE.values())


@pytest.mark.parametrize("cfg", us.SWEEP, ids=us.SWEEP_IDS)
def test_sweep_entry_is_legal(cfg):
    assert len(cfg.spatial) == cfg.dims and len(cfg.strides) == len(cfg.channels) - 1
    assert all(s == 2 for s in cfg.strides)          # the only legal kind (see STRIDE1_REFUSED)
    assert all(e % us.total_stride(cfg) == 0 for e in cfg.spatial)
    ref = RefUNet(cfg.dims, cfg.cin, cfg.K, cfg.channels, cfg.strides, dropout=cfg.dropout, act=cfg.act)
    net = Net(num_classes=cfg.K, num_channels=cfg.cin, spatial_dims=cfg.dims, channels=cfg.channels,
              strides=cfg.strides, dropout=cfg.dropout, act=cfg.act)
    a, b = net.state_dict(), ref.state_dict()
    assert list(a) == ["_model." + k for k in b]
    assert all(a["_model." + k].shape == v.shape for k, v in b.items())
    img, lab = us.make_batch(cfg)
    assert img.shape == (cfg.batch, cfg.cin) + tuple(cfg.spatial) and lab.shape == (cfg.batch, 1) + tuple(cfg.spatial)
    assert sorted(torch.unique(lab).tolist()) == list(range(cfg.K))       # every class present


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("cfg", us.SWEEP, ids=us.SWEEP_IDS)
def test_sweep_entry_is_well_conditioned(cfg):
    """The CPU oracle in float32 (the reference of tests/test_unet_gpu.py) against the float64 one: both are
    f32-accurate evaluations of the same graph, so an entry where this uses more than a quarter of a gate would test
    its own conditioning, not the kernels.  Seeds were chosen so that this holds (many do not: some seeds put plain
    torch f32 at 17x the weight-gradient gate, and the float64 oracle itself then jumps by 1-2x the gate when its input
    moves by 2^-24 -- hence the second, perturbation check below).

    One family of tensors is judged differently here: the bias of a convolution in front of a training-mode BatchNorm
    has an identically zero gradient (asserted on the float64 result).  What torch f32 reports for it is the rounding
    noise of ITS per-channel sum over all voxels -- it grows with the voxel count, exceeds the 2e-6 * gmax floor at the
    ring-sized K = 20 entries for every seed tried, and says nothing about conditioning.  The engine writes an exact
    zero there and stays under the unchanged gate in the GPU test."""
    img, lab = us.make_batch(cfg)
    r64 = us.oracle_step(cfg, img, lab)
    r32 = us.oracle_step(cfg, img, lab, torch.float32)
    zero = us.biases_under_batchnorm(r64["grads"])
    gmax = max(float(g.abs().max()) for g in r64["grads"].values())
    assert zero and all(float(r64["grads"][n].abs().max()) < 1e-12 * gmax for n in zero)
    bad = us.f32_step_violations(r32, r64, scale=0.25, skip=zero)
    assert not bad, bad[:8]
    # one f32 evaluation can be lucky: the float64 oracle itself, seeing an input moved by 2^-24 and f32-rounded
    # activations, must stay within the same quarter (three seeded trials)
    for trial in range(3):
        bad = us.f32_step_violations(us.wobbled_oracle_step(cfg, img, lab, trial), r64, scale=0.25, skip=zero)
        assert not bad, (trial, bad[:8])
    e64 = us.oracle_eval(cfg, r32["state"], img)
    e32 = us.oracle_eval(cfg, r32["state"], img, torch.float32)
    bad = us.f32_eval_violations(e32, e64, scale=0.25)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the gates bite
FAULT_CFG = next(c for c in us.SWEEP if c.name == "l16-32-64-K3-b1-12x24x40")


def _border_tap_zeroed(ref):
    """second convolution of the first encoder unit: for output voxels on the x = 0 face the tap kw = 2 is dropped"""
    conv = ref.model[0].conv.unit1.conv

    def hook(m, inp, out):
        w = torch.zeros_like(m.weight)
        w[:, :, :, :, 2] = m.weight[:, :, :, :, 2]
        part = F.conv3d(inp[0], w, None, m.stride, m.padding)
        mask = torch.zeros_like(out)
        mask[..., 0] = 1.0
        return out - part * mask
    conv.register_forward_hook(hook)


def _output_padding_dropped(ref):
    """top transposed convolution: output_padding 0 along x, the missing plane zero-filled"""
    conv = ref.model[2][0].conv

    def hook(m, inp, out):
        y = F.conv_transpose3d(inp[0], m.weight, m.bias, m.stride, m.padding, output_padding=(1, 1, 0))
        return F.pad(y, (0, 1))
    conv.register_forward_hook(hook)


def _biased_running_var(ref):
    bn = ref.model[1].submodule[1].submodule.conv.unit0.adn.N
    keep = {}

    def pre(m, inp):
        keep["rv"] = m.running_var.clone()

    def post(m, inp, out):
        if m.training:
            x = inp[0]
            var = x.var(dim=[0, 2, 3, 4], unbiased=False)
            m._buffers["running_var"] = (1 - m.momentum) * keep["rv"] + m.momentum * var.detach()
    bn.register_forward_pre_hook(pre)
    bn.register_forward_hook(post)


def _prelu_slope_gradient_dropped(ref):
    ref.model[1].submodule[0].conv.unit0.adn.A.weight.register_hook(torch.zeros_like)


def _residual_add_skipped_in_backward(ref):
    """a decoder unit with an identity residual: its input receives the convolution branch's gradient only"""
    unit = ref.model[1].submodule[2][1]
    assert isinstance(unit.residual, torch.nn.Identity)

    def forward(self, x):
        return self.conv(x) + x.detach()
    unit.forward = types.MethodType(forward, unit)


def _dice_over_padded_classes(logits, labels):
    """the loss over kpad = 16 class channels (zero logits in the padding) instead of K = 3"""
    pad = torch.zeros((logits.shape[0], 16 - logits.shape[1]) + tuple(logits.shape[2:]), dtype=logits.dtype)
    return ref_dice_loss(torch.cat([logits, pad], 1), labels)


FAULTS = {
    "border-tap-zeroed-on-one-face": (_border_tap_zeroed, None),
    "output-padding-dropped-on-one-axis": (_output_padding_dropped, None),
    "running-var-from-biased-variance": (_biased_running_var, None),
    "prelu-slope-gradient-dropped": (_prelu_slope_gradient_dropped, None),
    "residual-add-skipped-in-backward": (_residual_add_skipped_in_backward, None),
    "dice-over-padded-classes": (None, _dice_over_padded_classes),
}


@pytest.fixture(scope="module")
def fault_truth():
    img, lab = us.make_batch(FAULT_CFG)
    return img, lab, us.oracle_step(FAULT_CFG, img, lab)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_gates_fail_for_a_wrong_implementation(fault, fault_truth):
    """float64 throughout: the only difference to the oracle is the injected defect"""
    assert FAULT_CFG.K == 3
    img, lab, truth = fault_truth
    edit, loss_fn = FAULTS[fault]
    ref = us.make_ref(FAULT_CFG)
    if edit is not None:
        edit(ref)
    wrong = us.oracle_step(FAULT_CFG, img, lab, ref=ref, loss_fn=loss_fn or ref_dice_loss)
    bad = us.f32_step_violations(wrong, truth)
    print(fault, [(b[0], b[1], f"{b[2]:.2e} > {b[3]:.2e}") for b in bad[:4]])
    assert bad, f"the f32 gates do not notice: {fault}"
    # and an untouched second evaluation passes them (the gates are not simply always red)
    assert not us.f32_step_violations(us.oracle_step(FAULT_CFG, img, lab), truth)
