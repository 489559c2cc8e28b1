"""Array plumbing shared by the label-volume modules above ``ops.py`` (``seg/transforms.py``,
``seg/morphology.py``, ``seg/evaluation.py``, ``image/surfaces.py``): what an input may be, how it reaches the
device in a type the kernels read in place, and how a result goes back in the form of the input."""
from __future__ import annotations

import math
from typing import Union

import numpy as np
import torch

from .image.processing import Image

ArrayLike = Union[Image, np.ndarray, torch.Tensor]

MAX_LABEL = 65535
_IN_PLACE = (torch.uint8, torch.int16, torch.int32)


def _require_gpu(what: str, near=None) -> torch.device:
    """the device to compute on: that of ``near`` when it is a tensor on a GPU, else the current one.  ``what``
    opens the error raised without a GPU, e.g. "segmantic_amd.seg.transforms needs an MI355X"."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what}; no GPU is visible and there is no CPU path")
    if isinstance(near, torch.Tensor) and near.is_cuda:
        return near.device
    return torch.device("cuda", torch.cuda.current_device())


def _raw(x: ArrayLike):
    if isinstance(x, Image):
        return x.data
    if isinstance(x, (np.ndarray, torch.Tensor)):
        return x
    raise TypeError(f"expected an Image, a numpy array or a torch tensor, not {type(x).__name__}")


def _is_integer(a) -> bool:
    if isinstance(a, torch.Tensor):
        return not (a.is_floating_point() or a.is_complex())
    return a.dtype.kind in "biu"


def _tensor(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a


def _to_device(a, dev: torch.device, check_range: bool = False) -> torch.Tensor:
    """contiguous device tensor of a type the kernels read in place.  ``check_range``: the class tables of the
    clean-up transforms cover 0 .. MAX_LABEL; checking that is their one host synchronisation (uint8 needs none)"""
    t = _tensor(a)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    t = t.to(dev)
    if check_range and t.dtype != torch.uint8:
        lo, hi = torch.stack(torch.aminmax(t)).tolist()
        if lo < 0 or hi > MAX_LABEL:
            raise ValueError(f"label values must lie in 0 .. {MAX_LABEL}, the volume holds {lo} .. {hi}")
    if t.dtype not in _IN_PLACE:
        t = t.to(torch.int32)
    return t.contiguous()


def _wrap(x: ArrayLike, out: torch.Tensor):
    """result in the form of the input: Image (geometry copied), numpy array, or tensor on the input's device"""
    if isinstance(x, Image):
        return Image(out.to(x.data.device), x.spacing, x.origin, x.direction)
    if isinstance(x, np.ndarray):
        return out.cpu().numpy()
    return out.to(x.device)


def _back(x: ArrayLike, out: torch.Tensor):
    """like _wrap, in the input's dtype"""
    a = _raw(x)
    dt = torch.from_numpy(np.empty(0, a.dtype)).dtype if isinstance(a, np.ndarray) else a.dtype
    return _wrap(x, out if out.dtype == dt else out.to(dt))


def _check_spacing(spacing, ndim: int) -> tuple:
    if spacing is None:
        return (1.0,) * ndim
    if isinstance(spacing, (int, float, np.integer, np.floating)):
        spacing = (spacing,) * ndim
    sp = tuple(float(s) for s in spacing)
    if len(sp) != ndim:
        raise ValueError(f"spacing needs one entry per array axis ({ndim}), got {sp}")
    if any(not (s > 0.0 and math.isfinite(s)) for s in sp):
        raise ValueError(f"spacing must be positive and finite, got {sp}")
    return sp


def _zyx(sp: tuple) -> tuple:
    """the three spacings the kernels take; a 2-D input repeats its y spacing for the absent axis"""
    return sp if len(sp) == 3 else (sp[0],) + sp
