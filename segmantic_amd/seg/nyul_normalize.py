"""Nyul-Udupa histogram intensity standardisation on the MI355X (``csrc/nyul.hip``).

Port of the reference's ``segmantic.seg.nyul_normalize.NyulNormalize`` with the semantics of its torch
path: per segment (a channel when ``channel_wise``, else the whole tensor) the landmarks are
``torch.quantile`` of the masked values (``x != 0`` when ``nonzero``) at ``quantiles``, and the masked
values are mapped piecewise-linearly so that the landmarks land on ``standard_scale``.  Unlike the
reference, volumes of more than 2^24 masked values work: there the landmarks follow ``numpy.quantile``.
"""
from __future__ import annotations

from typing import Iterable, Tuple, Union

import numpy as np
import torch

from .. import ops

Array = Union[np.ndarray, torch.Tensor]


def _host_f64(v, what: str) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"NyulNormalize: {what} must be finite")
    return a


class NyulNormalize:
    """``NyulNormalize(quantiles, standard_scale, nonzero=False, channel_wise=False)``; ``__call__(img)``
    standardises ``img`` of shape [C, ...] in place and returns it.

    - The quantiles are sorted (stable) and ``standard_scale`` is permuted with them; 2 <= L <= 64
      landmarks, each quantile in [0, 1].
    - Landmarks are torch.quantile's (linear interpolation of exact order statistics, its f32 rank and
      lerp arithmetic) for up to 2^24 masked values of a segment, numpy.quantile's (f64) above, where the
      reference's torch path raises.  A segment with a masked NaN gets NaN landmarks (so NaN output); a
      segment whose mask is empty is left untouched.
    - The map is the reference's torch ``interp1d`` in f32 (each operation rounded, no FMA).  Duplicate
      landmarks (say a CT whose lowest landmarks are all -1024) give an infinite slope and the Inf / NaN
      outputs the reference produces: they are reproduced, not repaired.
    - f32 CUDA tensors are the exact path and are processed without a host synchronisation.  Other inputs
      are processed through an f32 copy on the current GPU and written back in place: non-contiguous
      tensors, CPU tensors and numpy arrays (type and device kept), and f64 / f16 / bf16 values, which are
      computed in f32 and cast back, so they are not bit-equal to the reference.
    """

    def __init__(self, quantiles, standard_scale, nonzero: bool = False, channel_wise: bool = False) -> None:
        q = _host_f64(quantiles, "quantiles")
        s = _host_f64(standard_scale, "standard_scale")
        if not 2 <= q.size <= ops.NYUL_MAX_LANDMARKS:
            raise ValueError(f"NyulNormalize: 2 .. {ops.NYUL_MAX_LANDMARKS} quantiles, got {q.size}")
        if s.size != q.size:
            raise ValueError(f"NyulNormalize: {s.size} standard_scale values for {q.size} quantiles")
        if np.any(q < 0) or np.any(q > 1):
            raise ValueError("NyulNormalize: quantiles must lie in [0, 1]")
        order = np.argsort(q, kind="stable")
        self.quantiles = q[order]
        self.standard_scale = s[order]
        self.nonzero = bool(nonzero)
        self.channel_wise = bool(channel_wise)

    # ------------------------------------------------------------------ device plumbing
    def _segments(self, t: torch.Tensor) -> int:
        if t.dim() == 0:
            raise ValueError("NyulNormalize: expected an image of shape [C, ...]")
        return int(t.shape[0]) if self.channel_wise else 1

    @staticmethod
    def _work_copy(img: Array) -> Tuple[torch.Tensor, bool]:
        """(contiguous f32 CUDA tensor, whether it is ``img`` itself)"""
        if isinstance(img, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(torch.cuda.current_device()), False
        if not isinstance(img, torch.Tensor):
            raise TypeError(f"NyulNormalize: expected a numpy array or a torch tensor, got {type(img).__name__}")
        if img.is_cuda and img.dtype == torch.float32 and img.is_contiguous():
            return img, True
        dev = img.device if img.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return img.detach().to(device=dev, dtype=torch.float32, memory_format=torch.contiguous_format).contiguous(), False

    def landmarks(self, img: Array) -> torch.Tensor:
        """f32 device tensor [S, L]: the landmarks of each segment (NaN for an empty or NaN segment)."""
        t, _ = self._work_copy(img)
        if t.numel() == 0:
            raise ValueError("NyulNormalize: empty image")
        lm, _ = ops.nyul_landmarks(t, self._segments(t), self.nonzero, self.quantiles)
        return lm

    @staticmethod
    def interp1d(x: torch.Tensor, xp: torch.Tensor, fp: torch.Tensor) -> torch.Tensor:
        """The reference's torch ``interp1d`` (piecewise-linear, extrapolating) of device tensors, by the
        HIP map: a new f32 tensor shaped like ``x``.  ``fp`` is read on the host."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise TypeError("NyulNormalize.interp1d: x must be a CUDA tensor")
        y = x.detach().to(torch.float32).contiguous().clone()
        xp = xp.detach().to(device=x.device, dtype=torch.float32).reshape(1, -1).contiguous()
        if y.numel():
            ops.nyul_apply_(y.view(-1), 1, False, xp, None, _host_f64(fp, "fp"))
        return y

    def __call__(self, img: Array) -> Array:
        t, same = self._work_copy(img)
        if t.numel() == 0:
            return img
        seg = self._segments(t)
        lm, counts = ops.nyul_landmarks(t, seg, self.nonzero, self.quantiles)
        ops.nyul_apply_(t, seg, self.nonzero, lm, counts, self.standard_scale)
        if same:
            return img
        if isinstance(img, np.ndarray):
            img[...] = t.cpu().numpy().astype(img.dtype, copy=False)
        else:
            with torch.no_grad():
                img.copy_(t)
        return img


def fit_standard_scale(images: Iterable[Array], quantiles, nonzero: bool = False, channel_wise: bool = False,
                       s_min: float = 0.0, s_max: float = 100.0) -> Tuple[np.ndarray, int]:
    """Nyul-Udupa training: map each segment's landmarks linearly so that the first lands on ``s_min`` and
    the last on ``s_max``, and average them (f64, in image then segment order).  Returns
    ``(standard_scale f64 [L] in sorted-quantile order, segments skipped)``: a segment is skipped when it is
    empty, has a non-finite landmark (a NaN in its mask) or has its first landmark equal to its last.
    Landmarks stay on the device until one copy at the end.  Raises ValueError when no segment remains."""
    q = _host_f64(quantiles, "quantiles")
    nn = NyulNormalize(q, np.linspace(0.0, 1.0, q.size), nonzero=nonzero, channel_wise=channel_wise)
    rows = [nn.landmarks(img) for img in images]
    if not rows:
        raise ValueError("fit_standard_scale: no images")
    lm = torch.cat([r.to(rows[0].device) for r in rows]).cpu().numpy().astype(np.float64)
    keep = np.all(np.isfinite(lm), axis=1) & (lm[:, 0] != lm[:, -1])
    if not np.any(keep):
        raise ValueError("fit_standard_scale: every segment is empty, holds NaN or has a constant range")
    lk = lm[keep]
    mapped = s_min + (lk - lk[:, :1]) * ((s_max - s_min) / (lk[:, -1:] - lk[:, :1]))
    return mapped.mean(axis=0), int(np.count_nonzero(~keep))
