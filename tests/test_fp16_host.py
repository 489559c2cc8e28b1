"""fp16 mode, host side (no GPU): the C-ABI declares it and the loss-scaling entry points, the bindings match,
and ``mixed_precision: fp16`` in a train-config selects float16 while ``True`` keeps selecting bfloat16."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
AMP_SYMBOLS = ("segmi_softmax_dice_bwd_amp", "segmi_amp_check_finite", "segmi_amp_update_scale",
               "segmi_adam_step_amp", "segmi_sgd_step_amp", "segmi_adabelief_step_amp")


def test_header_declares_f16_and_the_loss_scaling_entry_points():
    hdr = (ROOT / "include" / "segmi.h").read_text()
    assert "SEGMI_F16 = 2" in hdr and "SEGMI_BF16 = 1" in hdr and "SEGMI_F32 = 0" in hdr
    assert re.search(r"#define SEGMI_VERSION 1\b", hdr)
    declared = set(re.findall(r"^(?:int|int64_t|unsigned|const char\*)\s+(segmi_\w+)\(", hdr, re.M))
    from segmantic_amd import _lib
    assert _lib.SEGMI_F16 == 2
    for name in AMP_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert declared == set(_lib.SIGNATURES)


def test_library_exports_the_loss_scaling_entry_points():
    from segmantic_amd import _lib
    for name in AMP_SYMBOLS:
        assert hasattr(_lib.lib, name), name


def test_ops_maps_float16_to_the_f16_dtype_code():
    from segmantic_amd import _lib, ops
    assert ops._DT[torch.float16] == _lib.SEGMI_F16
    assert ops._DT[torch.bfloat16] == _lib.SEGMI_BF16 and ops._DT[torch.float32] == _lib.SEGMI_F32


@pytest.mark.parametrize("value,dtype", [(True, torch.bfloat16), (False, torch.float32), ("bf16", torch.bfloat16),
                                         ("fp16", torch.float16), ("FP16", torch.float16)])
def test_mixed_precision_selects_the_compute_dtype(value, dtype):
    from segmantic_amd.seg.monai_unet import Net
    net = Net(num_classes=3, channels=(16, 32, 64), strides=(2, 2))
    net.mixed_precision = value
    assert net.compute_dtype == dtype


def test_unknown_mixed_precision_string_is_refused():
    from segmantic_amd.seg.amp import precision_mode
    with pytest.raises(ValueError, match="fp16"):
        precision_mode("fp8")


def test_train_config_yaml_mixed_precision_fp16(tmp_path):
    """the train-config path: YAML -> validate_args against train()'s signature -> the Net's compute dtype.
    No new config key: the default stays True (bf16)."""
    import inspect

    import yaml

    from segmantic_amd.seg import monai_unet
    from segmantic_amd.utils import config
    from segmantic_amd.utils.cli import get_default_args, validate_args
    sig = inspect.signature(monai_unet.train)
    assert get_default_args(sig)["mixed_precision"] is True
    for text, want in (("fp16", torch.float16), ("true", torch.bfloat16), ("bf16", torch.bfloat16),
                       ("false", torch.float32)):
        f = tmp_path / f"cfg_{text}.yml"
        f.write_text(f"datalist: d.json\nmixed_precision: {text}\n")
        args = validate_args(config.load(f), signature=sig)
        net = monai_unet.Net(num_classes=3, channels=(16, 32, 64), strides=(2, 2))
        net.mixed_precision = args["mixed_precision"]
        assert net.compute_dtype == want, text
    assert yaml.safe_load("mixed_precision: fp16")["mixed_precision"] == "fp16"


def test_engine_refuses_unknown_dtypes_but_names_float16():
    from segmantic_amd.seg.unet import UNetEngine, UNetParams
    p = UNetParams(spatial_dims=3, in_channels=1, out_channels=3, channels=(16, 32, 64), strides=(2, 2),
                   num_res_units=2)
    with pytest.raises(TypeError, match="float16"):
        UNetEngine(p, torch.device("cpu"), torch.float64)


# ---------------------------------------------------------------------------------------------- the fp16 bound
# tests/helpers/lowp_bounds.py is the gate every fp16 op test applies.  These cases prove on CPU that it accepts
# a correctly rounded fp16 result and rejects each failure mode the GPU tests look for.
from tests.helpers import lowp_bounds as lb  # noqa: E402

BOUND_CONVS = [(16, 16, (6, 8, 10)), (128, 16, (4, 6, 6))]


def _u(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def _conv_operands(cin, cout, sp, seed):
    x = _u((1, cin) + sp, seed).half().double()
    w = _u((cout, cin, 3, 3, 3), seed + 1).half().double()
    return x, w


def _f16_result(v):
    """what a correct kernel stores: the f32 sum (the float64 one is close enough here) rounded to fp16"""
    return v.float().half().double()


@pytest.mark.parametrize("cin,cout,sp", BOUND_CONVS)
def test_fp16_bound_accepts_the_fp16_rounded_result(cin, cout, sp):
    x, w = _conv_operands(cin, cout, sp, 10)
    ref, a = lb.conv_ref(x, w)
    assert lb.assert_within(_f16_result(F.conv3d(x.float(), w.float(), padding=1)), ref, a) <= 1.0
    # an f32 output (no storage rounding) passes the bound without the 2^-11 term
    assert lb.assert_within(F.conv3d(x.float(), w.float(), padding=1), ref, a, rounded=False) <= 1.0


@pytest.mark.parametrize("cin,cout,sp", BOUND_CONVS)
def test_fp16_bound_rejects_a_bf16_rounded_output(cin, cout, sp):
    x, w = _conv_operands(cin, cout, sp, 20)
    ref, a = lb.conv_ref(x, w)
    r = lb.ratio(ref.float().bfloat16().double(), ref, a)
    assert float(r.max()) > lb.HALF_OUT_MIN_RATIO
    assert float((r > 1).double().mean()) > 0.3


@pytest.mark.parametrize("cin,cout,sp", BOUND_CONVS)
def test_fp16_bound_rejects_one_channel_of_bf16_rounded_operands(cin, cout, sp):
    x, w = _conv_operands(cin, cout, sp, 30)
    ref, a = lb.conv_ref(x, w)
    wb = w.clone()
    wb[:, 3] = wb[:, 3].float().bfloat16().double()            # one input channel's weights through bf16
    bad = _f16_result(F.conv3d(x, wb, padding=1))
    assert float(lb.ratio(bad, ref, a).max()) > 1.0
    xb = x.clone()
    xb[:, 5] = xb[:, 5].float().bfloat16().double()            # one activation channel through bf16
    assert float(lb.ratio(_f16_result(F.conv3d(xb, w, padding=1)), ref, a).max()) > 1.0


@pytest.mark.parametrize("rounded", [True, False])
def test_fp16_bound_rejects_flushed_subnormal_operands(rounded):
    """activations in [2^-24, 2^-14) (mostly fp16 subnormals) against normal weights: the reference lies partly in
    fp16's subnormal range and partly above it; a unit that flushes the subnormal inputs fails the bound."""
    cin, cout, sp = 16, 16, (6, 8, 10)
    g = torch.Generator().manual_seed(40)
    mag = torch.exp2(-24 + 10 * torch.rand((1, cin) + sp, generator=g, dtype=torch.float64))
    sign = torch.where(torch.rand((1, cin) + sp, generator=g) < 0.5, -1.0, 1.0).double()
    x = (mag * sign).half().double()
    assert float((x.abs() < 2.0 ** -14).double().mean()) > 0.5
    w = _u((cout, cin, 3, 3, 3), 41, 0.5).half().double()
    ref, a = lb.conv_ref(x, w)
    assert float((ref.abs() > 2.0 ** -24).double().mean()) > 0.5 and float((ref.abs() < 2.0 ** -14).double().mean()) > 0.1
    good = F.conv3d(x.float(), w.float(), padding=1)
    good = _f16_result(good) if rounded else good.double()
    assert lb.assert_within(good, ref, a, rounded=rounded) <= 1.0
    flushed = F.conv3d(lb.flush_f16_subnormals(x), w, padding=1)
    flushed = _f16_result(flushed) if rounded else flushed
    assert float(lb.ratio(flushed, ref, a, rounded=rounded).max()) > 1.0
    # and a weight gradient (f32 output) with a subnormal output gradient
    dy = (mag[:, :, :, :, :] * sign)[:, :cout].half().double()
    xn = _u((1, cin) + sp, 42).half().double()
    dw, adw, db, adb = lb.wgrad_ref(xn, dy)
    w0 = torch.zeros((cout, cin, 3, 3, 3), requires_grad=True)
    F.conv3d(xn.float(), w0, None, padding=1).backward(dy.float())
    assert lb.assert_within(w0.grad, dw, adw, rounded=False) <= 1.0
    dwf, _, _, _ = lb.wgrad_ref(xn, lb.flush_f16_subnormals(dy))
    assert float(lb.ratio(dwf, dw, adw, rounded=False).max()) > 1.0


def test_fp16_bound_rejects_saturation_and_accepts_inf():
    ref = torch.tensor([70000.0, -1.0e6, 65600.0, 1000.0, -65000.0, 65510.0], dtype=torch.float64)
    a = ref.abs()
    right = torch.tensor([float("inf"), float("-inf"), float("inf"), 1000.0, -64992.0, 65504.0], dtype=torch.float64)
    assert lb.assert_within(right, ref, a) <= 1.0
    saturated = right.clone()
    saturated[:3] = torch.tensor([65504.0, -65504.0, 65504.0])
    r = lb.ratio(saturated, ref, a)
    assert bool((r[:3] > 1.0).all()) and bool((r[3:] <= 1.0).all())
    wrong_sign = right.clone()
    wrong_sign[1] = float("inf")
    assert float(lb.ratio(wrong_sign, ref, a)[1]) > 1.0
    # an Inf where the reference is finite, or a NaN anywhere, is rejected
    spurious = right.clone()
    spurious[3], spurious[4] = float("inf"), float("nan")
    r = lb.ratio(spurious, ref, a)
    assert float(r[3]) > 1.0 and float(r[4]) > 1.0
