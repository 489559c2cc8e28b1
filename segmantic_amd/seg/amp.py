"""Dynamic loss scaling for fp16 training: ``torch.amp.GradScaler`` semantics with every piece of state
on the device.

The reference trains with Lightning ``precision=16`` (fp16 autocast, f32 master weights and a
``GradScaler``, reference ``src/segmantic/seg/monai_unet.py:424,533``).  Here the fp16 engine keeps f32
master weights in the parameter arena and this object scales the Dice gradient, checks the whole f32
gradient arena for Inf / NaN in one launch, gates the optimiser update on that and updates the scale
(``segmi_amp_*``, ``include/segmi.h``).  Nothing in a step reads device memory on the host.
"""
from __future__ import annotations

import torch

from .. import ops

MIXED_PRECISION_MODES = ("bf16", "fp16")


def precision_mode(mixed_precision) -> str:
    """``Net.mixed_precision`` / ``train(mixed_precision=...)`` -> "fp32", "bf16" or "fp16".
    ``True`` keeps meaning bf16 storage, ``False`` the exact-f32 path."""
    if isinstance(mixed_precision, str):
        mode = mixed_precision.strip().lower()
        if mode not in MIXED_PRECISION_MODES:
            raise ValueError(f"mixed_precision must be true, false, 'bf16' or 'fp16' (got '{mixed_precision}')")
        return mode
    return "bf16" if bool(mixed_precision) else "fp32"


def precision_dtype(mixed_precision) -> torch.dtype:
    return {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[precision_mode(mixed_precision)]


class GradScaler:
    """torch.amp.GradScaler defaults: initial scale 2**16, growth 2.0, backoff 0.5, growth interval 2000.

    ``amp`` is the f32[3] device tensor {scale, found_inf, skipped steps} the kernels read and write;
    ``tracker`` the int32 growth tracker.  Per step: ``check(flat_grad)`` after backward (and after the gradient all-reduce, so that
    every rank takes the same decision), the optimiser's ``step_amp``, then ``update(opt)``."""

    def __init__(self, device, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000):
        self.device = torch.device(device)
        self.amp = torch.tensor([float(init_scale), 0.0, 0.0], dtype=torch.float32, device=self.device)
        self.tracker = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.growth_factor = float(growth_factor)
        self.backoff_factor = float(backoff_factor)
        self.growth_interval = int(growth_interval)

    def check(self, flat_grad: torch.Tensor) -> None:
        ops.amp_check_finite(flat_grad, self.amp)

    def update(self, opt) -> None:
        """_amp_update_scale_ + the optimiser's applied-step count (advanced when the step was applied)."""
        ops.amp_update_scale(self.amp, self.tracker, opt.device_steps(), self.growth_factor,
                             self.backoff_factor, self.growth_interval)

    # ------------------------------------------------------------------ state (reads the device)
    def get_scale(self) -> float:
        return float(self.amp[0].item())

    def get_growth_tracker(self) -> int:
        return int(self.tracker.item())

    def skipped_steps(self) -> int:
        """steps whose gradients held Inf / NaN (the optimiser left the parameters untouched)"""
        return int(self.amp[2].item())

    def state_dict(self) -> dict:
        return {"scale": self.get_scale(), "growth_tracker": self.get_growth_tracker(),
                "skipped_steps": self.skipped_steps(), "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval}
