"""fp16 mode, host side (no GPU): the C-ABI declares it and the loss-scaling entry points, the bindings match,
and ``mixed_precision: fp16`` in a train-config selects float16 while ``True`` keeps selecting bfloat16."""
import re
from pathlib import Path

import pytest
import torch

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
