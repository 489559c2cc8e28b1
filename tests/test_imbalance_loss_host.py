"""CPU tests of the class-imbalance losses (Tversky, Dice + focal): known answers of their float64 reference
(tests/helpers/imbalance_loss_ref.py), the C-ABI entry points, and the ``optimizer["loss"]`` configuration path."""
import inspect
import math
import re
import subprocess
from pathlib import Path

import pytest
import torch

from oracle.unet_ref import ref_dice_loss
from tests.helpers.imbalance_loss_ref import ref_dice_focal_loss, ref_focal_term, ref_tversky_loss
from tests.helpers.loss_ref import ref_dice_ce_loss

ROOT = Path(__file__).resolve().parent.parent

NEW_SYMBOLS = ("segmi_softmax_tversky_fwd", "segmi_softmax_tversky_bwd", "segmi_softmax_tversky_bwd_amp",
               "segmi_softmax_dice_focal_fwd", "segmi_softmax_dice_focal_bwd", "segmi_softmax_dice_focal_bwd_amp")


def _seeded(k, seed=5, shape=(5, 6, 7), n=2):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn((n, k) + shape, generator=g, dtype=torch.float64) * 3
    lab = torch.randint(0, k, (n, 1) + shape, generator=g).double()
    return lg, lab


def _two_voxels():
    """2 voxels, 3 classes: x0 = (0, ln 2, ln 3) with y = 2, x1 = (ln 4, 0, 0) with y = 0; probabilities by hand:
    p0 = (1/6, 2/6, 3/6), p1 = (4/6, 1/6, 1/6)"""
    lg = torch.tensor([[0.0, math.log(2.0), math.log(3.0)], [math.log(4.0), 0.0, 0.0]], dtype=torch.float64)
    lg = lg.t().reshape(1, 3, 1, 1, 2).contiguous()
    lab = torch.tensor([2.0, 0.0], dtype=torch.float64).reshape(1, 1, 1, 1, 2)
    return lg, lab


# ------------------------------------------------------------------ known answers of the reference
def test_zero_logits_focal_is_q_pow_gamma_log_k():
    for k in (2, 5, 16):
        lg = torch.zeros((2, k, 3, 4, 5), dtype=torch.float64)
        lab = torch.randint(0, k, (2, 1, 3, 4, 5), generator=torch.Generator().manual_seed(k)).double()
        for gamma in (1.0, 2.0, 5.0):
            want = (1.0 - 1.0 / k) ** gamma * math.log(k)
            assert abs(float(ref_focal_term(lg, lab, gamma)) - want) < 1e-12
            # the weights cancel when every voxel has the same term
            w = [0.5 + j for j in range(k)]
            got = ref_dice_focal_loss(lg, lab, lambda_dice=0.0, gamma=gamma, weight=w)
            assert abs(float(got) - want) < 1e-12


def test_tversky_with_half_weights_is_dice_exactly():
    """alpha = beta = 0.5, exponent = 1, both smooths s / 2: the Dice loss with smooth s, to 0.0 in float64"""
    for k, seed in ((2, 1), (4, 5), (16, 9)):
        lg, lab = _seeded(k, seed)
        for s in (1e-5, 0.25):
            a = ref_tversky_loss(lg, lab, alpha=0.5, beta=0.5, exponent=1.0, smooth_nr=s / 2, smooth_dr=s / 2)
            b = ref_dice_loss(lg, lab) if s == 1e-5 else ref_dice_ce_loss(lg, lab, lambda_ce=0.0, smooth_nr=s, smooth_dr=s)
            assert a.dtype == torch.float64 and float(a) - float(b) == 0.0
        a = ref_tversky_loss(lg, lab, include_background=False, alpha=0.5, beta=0.5, smooth_nr=5e-6, smooth_dr=5e-6)
        b = ref_dice_ce_loss(lg, lab, include_background=False, lambda_ce=0.0)
        assert float(a) - float(b) == 0.0


def test_hand_computed_tversky():
    lg, lab = _two_voxels()
    s, al, be = 1e-5, 0.3, 0.7
    # (I, P, T): class 0 (4/6, 5/6, 1), class 1 (0, 1/2, 0), class 2 (1/2, 2/3, 1)
    rows = [(4.0 / 6.0, 5.0 / 6.0, 1.0), (0.0, 0.5, 0.0), (0.5, 2.0 / 3.0, 1.0)]
    u = [1.0 - (i + s) / (i + al * (p - i) + be * (t - i) + s) for i, p, t in rows]
    assert abs(float(ref_tversky_loss(lg, lab)) - sum(u) / 3.0) < 1e-12
    assert abs(float(ref_tversky_loss(lg, lab, include_background=False)) - (u[1] + u[2]) / 2.0) < 1e-12
    want = sum(v ** 0.75 for v in u) / 3.0
    assert abs(float(ref_tversky_loss(lg, lab, exponent=0.75)) - want) < 1e-12
    # alpha and beta swap the roles of false positives and false negatives
    u2 = [1.0 - (i + s) / (i + be * (p - i) + al * (t - i) + s) for i, p, t in rows]
    assert abs(float(ref_tversky_loss(lg, lab, alpha=be, beta=al)) - sum(u2) / 3.0) < 1e-12
    with pytest.raises(ValueError):
        ref_tversky_loss(lg[:, :1], lab * 0, include_background=False)


def test_tversky_term_is_zero_where_one_minus_ti_is_not_positive():
    """smooth_nr > smooth_dr on a perfectly predicted class makes TI > 1: term and gradient are 0"""
    lg = torch.zeros((1, 2, 1, 1, 3), dtype=torch.float64)
    lg[:, 0] = 60.0
    lab = torch.zeros((1, 1, 1, 1, 3), dtype=torch.float64)
    lq = lg.clone().requires_grad_(True)
    v = ref_tversky_loss(lq, lab, include_background=True, exponent=0.75, smooth_nr=1.0, smooth_dr=1e-5)
    v.backward()
    # class 0: TI = 4 / (3 + 1e-5) > 1 -> 0; class 1: I = P = T = 0 up to exp(-60): TI = 1 / 1e-5 -> 0
    assert float(v.detach()) == 0.0 and not bool(lq.grad.any()) and bool(torch.isfinite(lq.grad).all())


def test_hand_computed_focal():
    lg, lab = _two_voxels()
    w = [0.25, 1.0, 2.0]
    # voxel 0: q = 1/2, nll = ln 2, w = 2; voxel 1: q = 1/3, nll = ln 1.5, w = 0.25
    want = (2.0 * 0.25 * math.log(2.0) + 0.25 * (1.0 / 9.0) * math.log(1.5)) / 2.25
    got = ref_dice_focal_loss(lg, lab, lambda_dice=0.0, lambda_focal=1.0, gamma=2.0, weight=w)
    assert abs(float(got) - want) < 1e-12
    plain = (0.5 * math.log(2.0) + (1.0 / 3.0) * math.log(1.5)) / 2.0
    assert abs(float(ref_dice_focal_loss(lg, lab, lambda_dice=0.0, gamma=1.0)) - plain) < 1e-12
    # with the Dice term and the lambdas
    dice = float(ref_dice_ce_loss(lg, lab, lambda_ce=0.0))
    got = ref_dice_focal_loss(lg, lab, lambda_dice=0.5, lambda_focal=3.0, gamma=2.0, weight=w)
    assert abs(float(got) - (0.5 * dice + 3.0 * want)) < 1e-12


def test_gamma_zero_is_the_dice_ce_reference():
    lg, lab = _seeded(4)
    w = [0.2, 1.0, 1.5, 2.0]
    for kw in (dict(), dict(weight=w, include_background=False, lambda_dice=0.5)):
        a = ref_dice_focal_loss(lg, lab, gamma=0.0, lambda_focal=2.0, **kw)
        b = ref_dice_ce_loss(lg, lab, lambda_ce=2.0, **kw)
        assert abs(float(a) - float(b)) < 1e-14


def test_focal_gradient_formula():
    """d Focal_v / d x_j = g_v (p_j - [j = y]), g_v = q^gamma + gamma q^(gamma - 1) nll p_y: what the kernel applies"""
    lg, lab = _seeded(5, 11, (3, 4, 5), 1)
    for gamma in (1.0, 2.0, 5.0):
        lq = lg.clone().requires_grad_(True)
        ref_focal_term(lq, lab, gamma).backward()
        p = torch.softmax(lg, 1)
        y = lab[:, 0].long()
        oh = torch.nn.functional.one_hot(y, 5).movedim(-1, 1).double()
        py = (p * oh).sum(1)
        q, nll = 1.0 - py, -torch.log(py)
        g = q ** gamma + gamma * q ** (gamma - 1.0) * nll * py
        want = g[:, None] * (p - oh) / y.numel()
        assert float((lq.grad - want).abs().max()) < 1e-14


def test_far_true_class_and_perfect_voxels_in_the_focal_reference():
    lg = torch.zeros((1, 3, 1, 1, 4), dtype=torch.float64)
    lg[:, 0] = 200.0
    lab = torch.ones((1, 1, 1, 1, 4), dtype=torch.float64)
    assert abs(float(ref_dice_focal_loss(lg, lab, lambda_dice=0.0, gamma=2.0)) - 200.0) < 1e-9
    assert math.isnan(float(ref_dice_focal_loss(lg, lab, lambda_dice=0.0, weight=[0.0, 0.0, 0.0])))
    assert float(ref_dice_focal_loss(lg, lab * 0, lambda_dice=0.0, gamma=2.0)) == 0.0         # q = 0
    # labels outside [0, K) count for nothing
    lab2 = lab.clone()
    lab2[..., 0] = 3.0
    lab2[..., 1] = -1.0
    assert abs(float(ref_dice_focal_loss(lg, lab2, lambda_dice=0.0, gamma=2.0)) - 200.0) < 1e-9


# ------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_entry_points():
    from segmantic_amd import _lib, ops
    hdr = (ROOT / "include" / "segmi.h").read_text()
    declared = set(re.findall(r"^int\s+(segmi_\w+)\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    exported = set(re.findall(r"\sT\s+(segmi_\w+)", nm))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert name in exported, name
        assert hasattr(ops, name[len("segmi_"):]), name
    # the number of arguments in the header is the number in the binding
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        args = re.search(r"^int\s+" + name + r"\((.*?)\);", flat, re.M | re.S).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the existing entry points keep their signatures
    assert len(_lib.SIGNATURES["segmi_softmax_dice_fwd"][1]) == 9
    assert len(_lib.SIGNATURES["segmi_softmax_dice_ce_fwd"][1]) == 13
    assert len(_lib.SIGNATURES["segmi_softmax_dice_ce_bwd"][1]) == 9


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes as C

    from segmantic_amd import _lib
    a = _lib.Act(0x1000, 1, 2, 2, 2, 3, 3)
    p = C.c_void_p(0x1000)
    tv = _lib.lib.segmi_softmax_tversky_fwd
    for al, be, ex, word in ((-0.1, 0.7, 1.0, "alpha"), (0.3, float("nan"), 1.0, "beta"), (0.0, 0.0, 1.0, "alpha"),
                             (0.3, 0.7, 0.0, "exponent"), (0.3, 0.7, 3.5, "exponent")):
        assert tv(0, a, p, p, p, p, 1e-5, 1e-5, al, be, ex, 1, None) != 0
        assert word in _lib.last_error()
    assert tv(0, a, p, None, p, p, 1e-5, 1e-5, 0.3, 0.7, 1.0, 1, None) != 0
    assert tv(7, a, p, p, p, p, 1e-5, 1e-5, 0.3, 0.7, 1.0, 1, None) != 0
    one = _lib.Act(0x1000, 1, 2, 2, 2, 1, 1)
    assert tv(0, one, p, p, p, p, 1e-5, 1e-5, 0.3, 0.7, 1.0, 0, None) != 0
    assert "include_background" in _lib.last_error()
    big = _lib.Act(0x1000, 29, 2, 2, 2, 64, 64)                       # n * k = 1856 > 1792
    assert tv(0, big, p, p, p, p, 1e-5, 1e-5, 0.3, 0.7, 1.0, 1, None) != 0
    assert "1792" in _lib.last_error()
    assert _lib.lib.segmi_softmax_tversky_bwd_amp(0, a, p, p, None, a, None, None, None) != 0
    assert "amp" in _lib.last_error()
    fo = _lib.lib.segmi_softmax_dice_focal_fwd
    for gamma in (0.5, -1.0, 5.5, float("nan")):
        assert fo(0, a, p, p, p, p, 1e-5, 1e-5, 1.0, 1.0, gamma, 1, None, None) != 0
        assert "gamma" in _lib.last_error()
        assert _lib.lib.segmi_softmax_dice_focal_bwd(0, a, p, p, gamma, 1.0, a, None, None, None) != 0
        assert "gamma" in _lib.last_error()
    # the storage type is checked first: an unknown code with a bad gamma is reported as the type
    assert fo(7, a, p, p, p, p, 1e-5, 1e-5, 1.0, 1.0, 0.5, 1, None, None) != 0
    assert "dtype" in _lib.last_error()
    assert _lib.lib.segmi_softmax_dice_focal_bwd(7, a, p, p, 0.5, 1.0, a, None, None, None) != 0
    assert "dtype" in _lib.last_error()
    assert fo(0, a, p, p, p, p, 1e-5, 1e-5, -1.0, 1.0, 2.0, 1, None, None) != 0
    assert "lambda" in _lib.last_error()
    assert fo(0, a, p, p, p, p, 1e-5, 1e-5, -1.0, 1.0, 0.0, 1, None, None) != 0       # gamma = 0: the DiceCE checks
    assert "lambda" in _lib.last_error()
    assert fo(0, big, p, p, p, p, 1e-5, 1e-5, 1.0, 1.0, 2.0, 1, None, None) != 0
    assert "LDS" in _lib.last_error()
    assert fo(0, one, p, p, p, p, 1e-5, 1e-5, 1.0, 1.0, 2.0, 0, None, None) != 0
    assert _lib.lib.segmi_softmax_dice_focal_bwd_amp(0, a, p, p, 2.0, None, a, None, None, None) != 0
    assert "amp" in _lib.last_error()
    assert _lib.lib.segmi_softmax_dice_focal_bwd(0, a, p, p, 2.0, 1.0, a, None, p, None) != 0   # bias_grad, no scratch


# ------------------------------------------------------------------ configuration
YAML = """
datalist: data.json
output_dir: out
num_classes: 4
optimizer:
  optimizer: Adam
  lr: 1.0e-4
  loss: %s
"""
LOSS_YAML = {
    "Tversky": "{name: Tversky, include_background: false, alpha: 0.7, beta: 0.3, exponent: 0.75}",
    "DiceFocal": "{name: DiceFocal, lambda_dice: 0.5, lambda_focal: 2.0, gamma: 3, class_weights: [0.2, 1, 1, 2]}",
}


def _args(tmp_path, text):
    from segmantic_amd.seg.monai_unet import train
    from segmantic_amd.utils import config
    from segmantic_amd.utils.cli import validate_args
    f = tmp_path / "train.yml"
    f.write_text(text)
    return validate_args(config.load(f), inspect.signature(train))


@pytest.mark.parametrize("name", list(LOSS_YAML))
def test_yaml_config_becomes_the_loss_object(name, tmp_path):
    from segmantic_amd.seg import losses
    from segmantic_amd.seg.monai_unet import Net
    args = _args(tmp_path, YAML % LOSS_YAML[name])
    assert args["optimizer"]["loss"]["name"] == name
    net = Net(num_classes=args["num_classes"], channels=(16, 32), strides=(2,))
    net.optimizer = args["optimizer"]
    loss = net.configure_loss()
    assert loss is net.loss_function and net.configure_loss() is loss
    if name == "Tversky":
        assert type(loss) is losses.TverskyLoss and loss.include_background is False
        assert (loss.alpha, loss.beta, loss.exponent) == (0.7, 0.3, 0.75)
        d = losses.loss_from_config({"name": "Tversky"}, 4)
        assert (d.alpha, d.beta, d.exponent, d.include_background) == (0.3, 0.7, 1.0, True)
        assert (d.smooth_nr, d.smooth_dr) == (1e-5, 1e-5)
    else:
        assert type(loss) is losses.DiceFocalLoss and loss.include_background is True
        assert (loss.lambda_dice, loss.lambda_focal, loss.gamma) == (0.5, 2.0, 3.0)
        assert loss.weight == [0.2, 1.0, 1.0, 2.0]
        d = losses.loss_from_config({"name": "DiceFocal"}, 4)
        assert (d.lambda_dice, d.lambda_focal, d.gamma, d.weight) == (1.0, 1.0, 2.0, None)
        assert losses.loss_from_config({"name": "DiceFocal", "gamma": 0, "lambda_dice": 0}, 4).gamma == 0.0
    assert name in losses.LOSS_NAMES
    for meth in ("forward_ndhwc", "backward_ndhwc"):
        assert callable(getattr(loss, meth))
    assert isinstance(loss, losses._FusedLoss)
    # back to the default
    net.optimizer = dict(Net.optimizer)
    assert type(net.configure_loss()) is losses.DiceLoss


BAD = [
    ({"name": "Tversky", "alpha": -0.1}, "alpha"),
    ({"name": "Tversky", "alpha": float("inf")}, "alpha"),
    ({"name": "Tversky", "alpha": 0.0, "beta": 0.0}, "alpha"),
    ({"name": "Tversky", "beta": -1}, "beta"),
    ({"name": "Tversky", "beta": "high"}, "beta"),
    ({"name": "Tversky", "exponent": 0.0}, "exponent"),
    ({"name": "Tversky", "exponent": 3.5}, "exponent"),
    ({"name": "Tversky", "class_weights": [1, 1, 1, 1]}, "class_weights"),
    ({"name": "Tversky", "gamma": 2.0}, "gamma"),
    ({"name": "Tversky", "include_background": 0}, "include_background"),
    ({"name": "DiceFocal", "gamma": 0.5}, "gamma"),
    ({"name": "DiceFocal", "gamma": 6}, "gamma"),
    ({"name": "DiceFocal", "gamma": -1}, "gamma"),
    ({"name": "DiceFocal", "lambda_focal": -1}, "lambda_focal"),
    ({"name": "DiceFocal", "lambda_ce": 1.0}, "lambda_ce"),
    ({"name": "DiceFocal", "alpha": 0.25}, "alpha"),
    ({"name": "DiceFocal", "class_weights": [1, 1, 1]}, "class_weights"),
    ({"name": "DiceFocal", "class_weights": [1, -1, 1, 1]}, "class_weights"),
    ({"name": "DiceCE", "lambda_focal": 1.0}, "lambda_focal"),
    ({"name": "Dice", "alpha": 0.3}, "alpha"),
]


@pytest.mark.parametrize("cfg,key", BAD, ids=[f"{i}-{c['name']}-{k}" for i, (c, k) in enumerate(BAD)])
def test_bad_loss_entries_are_refused_with_the_key_named(cfg, key, tmp_path):
    from segmantic_amd.seg.losses import loss_from_config
    from segmantic_amd.seg.monai_unet import Net, train
    with pytest.raises(ValueError, match=key):
        loss_from_config(cfg, 4)
    net = Net(num_classes=4, channels=(16, 32), strides=(2,))
    net.optimizer = {"optimizer": "Adam", "lr": 1e-4, "loss": cfg}
    with pytest.raises(ValueError, match=key):
        net.configure_optimizers()
    with pytest.raises(ValueError, match=key):
        train(datalist=tmp_path / "missing.json", output_dir=tmp_path / "out", num_classes=4,
              optimizer={"optimizer": "Adam", "lr": 1e-4, "loss": cfg}, gpu_ids=[0, 1])
    assert not (tmp_path / "out").exists()


def test_loss_constructors_validate():
    from segmantic_amd.seg.losses import DiceFocalLoss, TverskyLoss
    for kw, key in ((dict(alpha=-1.0), "alpha"), (dict(beta=float("nan")), "beta"), (dict(alpha=0.0, beta=0.0), "alpha"),
                    (dict(exponent=0.0), "exponent"), (dict(exponent=3.01), "exponent")):
        with pytest.raises(ValueError, match=key):
            TverskyLoss(**kw)
    for kw, key in ((dict(gamma=0.5), "gamma"), (dict(gamma=5.5), "gamma"), (dict(lambda_dice=-1.0), "lambda_dice"),
                    (dict(lambda_focal=float("inf")), "lambda_focal"), (dict(weight=[1.0, -2.0]), "class_weights")):
        with pytest.raises(ValueError, match=key):
            DiceFocalLoss(**kw)
    with pytest.raises(NotImplementedError):
        TverskyLoss(softmax=False)
    with pytest.raises(NotImplementedError):
        DiceFocalLoss(to_onehot_y=False)
    assert TverskyLoss(exponent=3.0, alpha=0.0, beta=1.0).exponent == 3.0
    assert DiceFocalLoss(gamma=0).gamma == 0.0 and DiceFocalLoss(gamma=1).gamma == 1.0
    assert list(inspect.signature(TverskyLoss.__init__).parameters)[1:] == [
        "include_background", "to_onehot_y", "softmax", "alpha", "beta", "exponent", "smooth_nr", "smooth_dr"]
    assert list(inspect.signature(DiceFocalLoss.__init__).parameters)[1:] == [
        "include_background", "to_onehot_y", "softmax", "lambda_dice", "lambda_focal", "gamma", "weight", "smooth_nr",
        "smooth_dr"]
