"""CPU tests of the Dice + cross-entropy loss: known answers of its reference (tests/helpers/loss_ref.py), the C-ABI
entry points, and the ``optimizer["loss"]`` configuration path (YAML -> ``validate_args`` -> loss object)."""
import inspect
import math
import re
import subprocess
from pathlib import Path

import pytest
import torch

from tests.helpers.loss_ref import ref_dice_ce_loss
from oracle.unet_ref import ref_dice_loss

ROOT = Path(__file__).resolve().parent.parent

NEW_SYMBOLS = ("segmi_dice_ce_chunks", "segmi_softmax_dice_ce_fwd", "segmi_softmax_dice_ce_bwd",
               "segmi_softmax_dice_ce_bwd_amp")


# ------------------------------------------------------------------ known answers of the reference
def test_zero_logits_give_log_k():
    for k in (2, 5, 16):
        lg = torch.zeros((2, k, 3, 4, 5), dtype=torch.float64)
        lab = torch.randint(0, k, (2, 1, 3, 4, 5), generator=torch.Generator().manual_seed(k)).double()
        ce = ref_dice_ce_loss(lg, lab, lambda_dice=0.0, lambda_ce=1.0)
        assert abs(float(ce) - math.log(k)) < 1e-12
        # the weights cancel when every voxel has the same -log p
        w = [0.5 + j for j in range(k)]
        assert abs(float(ref_dice_ce_loss(lg, lab, lambda_dice=0.0, weight=w)) - math.log(k)) < 1e-12


def _two_voxels():
    """2 voxels, 3 classes: x0 = (0, ln 2, ln 3) with y = 2, x1 = (ln 4, 0, 0) with y = 0; probabilities by hand:
    p0 = (1/6, 2/6, 3/6), p1 = (4/6, 1/6, 1/6)"""
    lg = torch.tensor([[0.0, math.log(2.0), math.log(3.0)], [math.log(4.0), 0.0, 0.0]], dtype=torch.float64)
    lg = lg.t().reshape(1, 3, 1, 1, 2).contiguous()
    lab = torch.tensor([2.0, 0.0], dtype=torch.float64).reshape(1, 1, 1, 1, 2)
    return lg, lab


def test_hand_computed_weighted_cross_entropy():
    lg, lab = _two_voxels()
    w = [0.25, 1.0, 2.0]
    # CE = (w2 * -ln(1/2) + w0 * -ln(2/3)) / (w2 + w0)
    want = (2.0 * math.log(2.0) + 0.25 * math.log(1.5)) / 2.25
    got = ref_dice_ce_loss(lg, lab, lambda_dice=0.0, lambda_ce=1.0, weight=w)
    assert abs(float(got) - want) < 1e-12
    # lambda_ce scales it; unweighted is the plain mean
    assert abs(float(ref_dice_ce_loss(lg, lab, lambda_dice=0.0, lambda_ce=0.5, weight=w)) - 0.5 * want) < 1e-12
    plain = (math.log(2.0) + math.log(1.5)) / 2.0
    assert abs(float(ref_dice_ce_loss(lg, lab, lambda_dice=0.0)) - plain) < 1e-12


def test_hand_computed_dice_without_background():
    lg, lab = _two_voxels()
    s = 1e-5
    # class 1: I = 0, P = 2/6 + 1/6, T = 0;  class 2: I = 3/6, P = 3/6 + 1/6, T = 1
    f1 = 1.0 - (0.0 + s) / (0.5 + s)
    f2 = 1.0 - (2.0 * 0.5 + s) / (1.0 + 4.0 / 6.0 + s)
    got = ref_dice_ce_loss(lg, lab, include_background=False, lambda_dice=1.0, lambda_ce=0.0)
    assert abs(float(got) - (f1 + f2) / 2.0) < 1e-12
    # with the background: class 0 has I = 4/6, P = 1/6 + 4/6, T = 1
    f0 = 1.0 - (2.0 * 4.0 / 6.0 + s) / (1.0 + 5.0 / 6.0 + s)
    got = ref_dice_ce_loss(lg, lab, include_background=True, lambda_dice=1.0, lambda_ce=0.0)
    assert abs(float(got) - (f0 + f1 + f2) / 3.0) < 1e-12
    with pytest.raises(ValueError):
        ref_dice_ce_loss(lg[:, :1], lab * 0, include_background=False)


def test_lambda_ce_zero_is_the_dice_oracle():
    g = torch.Generator().manual_seed(5)
    lg = torch.randn((2, 4, 5, 6, 7), generator=g, dtype=torch.float64) * 3
    lab = torch.randint(0, 4, (2, 1, 5, 6, 7), generator=g).double()
    a, b = ref_dice_ce_loss(lg, lab, lambda_ce=0.0), ref_dice_loss(lg, lab)
    assert a.dtype == torch.float64 and abs(float(a) - float(b)) < 1e-15
    assert ref_dice_ce_loss(lg.float(), lab).dtype == torch.float32


def test_far_true_class_contributes_its_distance_not_inf():
    lg = torch.zeros((1, 3, 1, 1, 4), dtype=torch.float64)
    lg[:, 0] = 200.0
    lab = torch.ones((1, 1, 1, 1, 4), dtype=torch.float64)
    assert abs(float(ref_dice_ce_loss(lg, lab, lambda_dice=0.0)) - 200.0) < 1e-9
    assert math.isnan(float(ref_dice_ce_loss(lg, lab, lambda_dice=0.0, weight=[0.0, 0.0, 0.0])))


# ------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_entry_points():
    from segmantic_amd import _lib
    hdr = (ROOT / "include" / "segmi.h").read_text()
    declared = set(re.findall(r"^int\s+(segmi_\w+)\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    exported = set(re.findall(r"\sT\s+(segmi_\w+)", nm))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert name in exported, name
    # the Dice-only entry points keep their signatures
    assert len(_lib.SIGNATURES["segmi_softmax_dice_fwd"][1]) == 9
    assert len(_lib.SIGNATURES["segmi_softmax_dice_bwd"][1]) == 9
    assert len(_lib.SIGNATURES["segmi_softmax_dice_bwd_amp"][1]) == 9
    assert _lib.lib.segmi_dice_ce_chunks(None) == 0
    a = _lib.Act(None, 3, 17, 24, 33, 5, 16)
    assert _lib.lib.segmi_dice_ce_chunks(a) == 2                      # 13 464 voxels in chunks of 8192


def test_bad_arguments_are_refused_before_any_launch():
    """SEGMI_CHECK_ARG: negative lambdas, a single class without its background, null buffers (the pointers are never
    dereferenced on the host, so made-up non-null values do)"""
    import ctypes as C

    from segmantic_amd import _lib
    a = _lib.Act(0x1000, 1, 2, 2, 2, 3, 3)
    p = C.c_void_p(0x1000)
    fwd = _lib.lib.segmi_softmax_dice_ce_fwd
    assert fwd(0, a, p, p, p, p, 1e-5, 1e-5, -1.0, 1.0, 1, None, None) != 0
    assert "lambda" in _lib.last_error()
    assert fwd(0, a, p, p, p, p, 1e-5, 1e-5, 1.0, float("nan"), 1, None, None) != 0
    assert fwd(0, a, p, None, p, p, 1e-5, 1e-5, 1.0, 1.0, 1, None, None) != 0
    assert fwd(7, a, p, p, p, p, 1e-5, 1e-5, 1.0, 1.0, 1, None, None) != 0
    one = _lib.Act(0x1000, 1, 2, 2, 2, 1, 1)
    assert fwd(0, one, p, p, p, p, 1e-5, 1e-5, 1.0, 1.0, 0, None, None) != 0
    assert "include_background" in _lib.last_error()
    big = _lib.Act(0x1000, 29, 2, 2, 2, 64, 64)                       # n * k = 1856 > 1792
    assert fwd(0, big, p, p, p, p, 1e-5, 1e-5, 1.0, 1.0, 1, None, None) != 0
    assert "LDS" in _lib.last_error()
    # the Dice-only forward folds 3 rows: it refuses beyond its own bound, n * k <= 2389
    huge = _lib.Act(0x1000, 38, 2, 2, 2, 64, 64)                      # n * k = 2432
    assert _lib.lib.segmi_softmax_dice_fwd(0, huge, p, p, p, p, 1e-5, 1e-5, None) != 0
    assert "LDS" in _lib.last_error() and "2389" in _lib.last_error()
    assert _lib.lib.segmi_softmax_tversky_bwd(0, a, p, p, 1.0, a, None, p, None) != 0
    assert "softmax_tversky_bwd" in _lib.last_error()                 # reported under the entry point called
    assert _lib.lib.segmi_softmax_dice_ce_bwd_amp(0, a, p, p, None, a, None, None, None) != 0
    assert "amp" in _lib.last_error()
    assert _lib.lib.segmi_softmax_dice_ce_bwd(0, a, p, p, 1.0, a, None, p, None) != 0      # bias_grad without scratch


# ------------------------------------------------------------------ configuration
YAML = """
datalist: data.json
output_dir: out
num_classes: 4
optimizer:
  optimizer: Adam
  lr: 1.0e-4
  loss: {name: DiceCE, include_background: false, lambda_dice: 1.0, lambda_ce: 1.0, class_weights: [0.2, 1, 1, 2]}
"""


def _args(tmp_path, text=YAML):
    from segmantic_amd.seg.monai_unet import train
    from segmantic_amd.utils import config
    from segmantic_amd.utils.cli import validate_args
    f = tmp_path / "train.yml"
    f.write_text(text)
    return validate_args(config.load(f), inspect.signature(train))


def test_yaml_config_becomes_the_loss_object(tmp_path):
    from segmantic_amd.seg.losses import DiceCELoss, DiceLoss, loss_from_config
    from segmantic_amd.seg.monai_unet import Net
    from segmantic_amd.seg.optim import make_optimizer
    args = _args(tmp_path)
    assert args["optimizer"]["loss"]["name"] == "DiceCE"
    net = Net(num_classes=args["num_classes"], channels=(16, 32), strides=(2,))
    assert isinstance(net.loss_function, DiceLoss) and net.loss_function.include_background
    net.optimizer = args["optimizer"]
    loss = net.configure_loss()
    assert type(loss) is DiceCELoss and loss is net.loss_function
    assert loss.include_background is False and loss.lambda_dice == 1.0 and loss.lambda_ce == 1.0
    assert loss.weight == [0.2, 1.0, 1.0, 2.0]
    assert net.configure_loss() is loss                                # unchanged entry: the same object
    net.optimizer["loss"]["class_weights"][0] = 0.5                    # an edit inside the nested list is noticed
    edited = net.configure_loss()
    assert edited is not loss and edited.weight == [0.5, 1.0, 1.0, 2.0]
    loss = edited
    # absent -> the default Dice loss again, a fresh object without the other loss's state
    net.optimizer = dict(Net.optimizer)
    assert "loss" not in Net.optimizer
    back = net.configure_loss()
    assert type(back) is DiceLoss and back.include_background
    # ... bound to the Dice-only entry points and their 3-row / 2-row scratch, not to the _ce ones
    from segmantic_amd import ops
    assert (back._fwd, back._bwd, back._bwd_amp) == (ops.softmax_dice_fwd, ops.softmax_dice_bwd,
                                                     ops.softmax_dice_bwd_amp)
    assert (back._state.rows, back._state.coef_rows) == (3, 2) and back._state is not loss._state
    assert type(loss_from_config(None)) is DiceLoss
    # names
    ce = loss_from_config({"name": "CE", "class_weights": [1, 2, 3]}, 3)
    assert type(ce) is DiceCELoss and ce.lambda_dice == 0.0 and ce.lambda_ce == 1.0 and ce.weight == [1.0, 2.0, 3.0]
    d = loss_from_config({"name": "Dice", "include_background": False}, 3)
    assert type(d) is DiceLoss and d.include_background is False
    assert type(loss_from_config({}, 3)) is DiceLoss
    # make_optimizer ignores the key
    flat = torch.zeros(8)
    opt = make_optimizer(args["optimizer"], flat, torch.zeros(8))
    assert type(opt).__name__ == "FlatAdam" and opt.lr == 1e-4


BAD = [
    ({"name": "Focal"}, "name"),
    ({"name": "DiceCE", "gamma": 2.0}, "gamma"),
    ({"name": "Dice", "lambda_ce": 1.0}, "lambda_ce"),
    ({"name": "CE", "lambda_dice": 1.0}, "lambda_dice"),
    ({"name": "DiceCE", "class_weights": [1, 1, 1]}, "class_weights"),
    ({"name": "DiceCE", "class_weights": [1, -1, 1, 1]}, "class_weights"),
    ({"name": "DiceCE", "class_weights": [1, float("nan"), 1, 1]}, "class_weights"),
    ({"name": "DiceCE", "class_weights": "balanced"}, "class_weights"),
    ({"name": "DiceCE", "lambda_dice": -0.5}, "lambda_dice"),
    ({"name": "DiceCE", "lambda_ce": -1}, "lambda_ce"),
    ({"name": "DiceCE", "include_background": "no"}, "include_background"),
]


@pytest.mark.parametrize("cfg,key", BAD, ids=[f"{i}-{k}" for i, (_, k) in enumerate(BAD)])
def test_bad_loss_entries_are_refused_with_the_key_named(cfg, key, tmp_path):
    from segmantic_amd.seg.losses import loss_from_config
    from segmantic_amd.seg.monai_unet import Net, train
    with pytest.raises(ValueError, match=key):
        loss_from_config(cfg, 4)
    # Net.configure_optimizers refuses it before it builds anything on a device (the net is on the CPU)
    net = Net(num_classes=4, channels=(16, 32), strides=(2,))
    net.optimizer = {"optimizer": "Adam", "lr": 1e-4, "loss": cfg}
    with pytest.raises(ValueError, match=key):
        net.configure_optimizers()
    # train() refuses it before any device call, data access or rank launch
    with pytest.raises(ValueError, match=key):
        train(datalist=tmp_path / "missing.json", output_dir=tmp_path / "out", num_classes=4,
              optimizer={"optimizer": "Adam", "lr": 1e-4, "loss": cfg}, gpu_ids=[0, 1])
    assert not (tmp_path / "out").exists()


def test_loss_constructors_validate():
    from segmantic_amd.seg.losses import DiceCELoss, DiceLoss
    with pytest.raises(ValueError, match="lambda_dice"):
        DiceCELoss(lambda_dice=-1.0)
    with pytest.raises(ValueError, match="lambda_ce"):
        DiceCELoss(lambda_ce=float("inf"))
    with pytest.raises(ValueError, match="class_weights"):
        DiceCELoss(weight=[1.0, -2.0])
    with pytest.raises(NotImplementedError):
        DiceCELoss(softmax=False)
    with pytest.raises(NotImplementedError):
        DiceLoss(to_onehot_y=False)
    assert DiceCELoss(weight=torch.tensor([1.0, 0.0, 2.0])).weight == [1.0, 0.0, 2.0]
    sig = inspect.signature(DiceCELoss.__init__)
    assert list(sig.parameters)[1:] == ["include_background", "to_onehot_y", "softmax", "lambda_dice", "lambda_ce",
                                       "weight", "smooth_nr", "smooth_dr"]


def test_training_step_names_no_dice_function():
    """the step drives the configured loss through the loss object's interface only"""
    from segmantic_amd.seg import monai_unet
    src = inspect.getsource(monai_unet)
    assert "dice_forward" not in src and "dice_backward" not in src
    step = inspect.getsource(monai_unet.Net.training_step)
    assert "forward_ndhwc" in step and "backward_ndhwc" in step


def test_train_signature_is_unchanged():
    from segmantic_amd.seg.monai_unet import Net, train
    assert list(inspect.signature(train).parameters) == [
        "datalist", "image_dir", "labels_dir", "output_dir", "checkpoint_file", "num_classes", "num_channels",
        "spatial_dims", "spatial_size", "preprocessing", "augmentation", "augment_intensity", "augment_spatial",
        "channels", "strides", "dropout", "act", "num_samples", "optimizer", "lr_scheduling", "max_epochs",
        "early_stop_patience", "mixed_precision", "cache_rate", "gpu_ids", "tissue_list"]
    assert Net.optimizer == {"optimizer": "Adam", "lr": 1e-4, "momentum": 0.9, "epsilon": 1e-8, "amsgrad": False,
                             "weight_decouple": False}
