"""Mirror test-time augmentation and per-voxel uncertainty.

The network is run on every mirrored copy of the volume (the unchanged sliding-window driver), each pass's
softmax is added at the un-mirrored voxel (``segmi_tta_accumulate``) and the sum is turned into labels,
confidence, normalised entropy and probabilities in one pass (``segmi_tta_finalize``).  The reference has
neither; nnU-Net mirrors by default.  ``torch.flip`` of the (one-channel) input is the only torch operation
on the data path.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Union

import numpy as np
import torch

from .. import ops
from .inferers import sliding_window_inference
from .losses import as_ndhwc


class TTAResult(NamedTuple):
    probs: torch.Tensor          # [B, K, *spatial] f32 view of the NDHWC accumulator, sums to 1 over K
    labels: torch.Tensor         # [B, 1, *spatial] uint8 (K <= 256) or int32
    confidence: torch.Tensor     # [B, 1, *spatial] f32, the probability of the label
    entropy: torch.Tensor        # [B, 1, *spatial] f32 in [0, 1]
    passes: int


def flip_sets(spatial_dims: int, flips: Union[str, Sequence[Sequence[int]]] = "all") -> List[int]:
    """Axis masks of the passes (bit a = spatial axis a is mirrored).  ``"all"``: every subset of the axes in
    ascending mask order, identity first (8 in 3-D, 4 in 2-D).  Otherwise a list of axis tuples, e.g.
    ``[(), (0,), (1, 2)]``, kept in the given order; the identity need not be among them."""
    if spatial_dims not in (2, 3):
        raise ValueError(f"flip_sets: spatial_dims must be 2 or 3, got {spatial_dims}")
    if isinstance(flips, str):
        if flips != "all":
            raise ValueError(f"flip_sets: unknown flip set {flips!r} ('all' or a list of axis tuples)")
        return list(range(1 << spatial_dims))
    masks = []
    for axes in flips:
        if isinstance(axes, (str, bytes)) or not hasattr(axes, "__iter__"):
            raise ValueError(f"flip_sets: {axes!r} is not a tuple of axes")
        m = 0
        for a in axes:
            if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 0 <= int(a) < spatial_dims:
                raise ValueError(f"flip_sets: axis {a!r} outside 0 .. {spatial_dims - 1}")
            if m & (1 << int(a)):
                raise ValueError(f"flip_sets: axis {a} twice in {tuple(axes)}")
            m |= 1 << int(a)
        if m in masks:
            raise ValueError(f"flip_sets: the flip {tuple(axes)} is listed twice")
        masks.append(m)
    if not masks:
        raise ValueError("flip_sets: no pass")
    return masks


def parse_flips(text: str):
    """``--tta-flips`` syntax: ``all`` or passes separated by ``,`` with the axes of a pass joined by ``+``
    and ``none`` for the identity, e.g. ``none,0,1+2``."""
    text = text.strip()
    if text == "all":
        return "all"
    out = []
    for part in text.split(","):
        part = part.strip()
        out.append(() if part in ("none", "") else tuple(int(a) for a in part.split("+")))
    return out


def mirror_tta_inference(inputs: torch.Tensor, roi_size, sw_batch_size: int, predictor, flips="all",
                         **sliding_kwargs) -> TTAResult:
    """inputs [B, C, D, H, W] (or [B, C, H, W]) float32 on the GPU; the other arguments as
    ``sliding_window_inference``.  One sliding-window pass per mask of ``flip_sets(spatial_dims, flips)``."""
    if inputs.dim() not in (4, 5):
        raise ValueError("mirror_tta_inference expects [B,C,D,H,W] (or [B,C,H,W])")
    if not inputs.is_cuda:
        raise RuntimeError("segmantic_amd test-time augmentation runs on the GPU only")
    for k in ("return_labels", "return_logits", "window_range", "z_slab"):
        if k in sliding_kwargs:
            raise ValueError(f"mirror_tta_inference: {k} is not supported (whole-volume logits are needed)")
    sd = inputs.dim() - 2
    masks = flip_sets(sd, flips)
    shift = 3 - sd                       # 2-D runs as depth 1: spatial axis a is kernel axis a + 1
    B = inputs.shape[0]
    acc = None
    for i, m in enumerate(masks):
        dims = [2 + a for a in range(sd) if m & (1 << a)]
        x = torch.flip(inputs, dims) if dims else inputs
        logits = sliding_window_inference(x, roi_size, sw_batch_size, predictor, return_logits=True,
                                          **sliding_kwargs)
        if sd == 2:
            logits = logits.unsqueeze(2)
        nd = as_ndhwc(logits.float())
        if acc is None:
            acc = torch.empty(tuple(nd.shape), dtype=torch.float32, device=nd.device)
        for b in range(B):
            ops.tta_accumulate(nd[b:b + 1], m << shift, acc[b], first=(i == 0))
    K = acc.shape[4]
    vox = tuple(acc.shape[:4])
    labels = torch.empty(vox, dtype=torch.uint8 if K <= 256 else torch.int32, device=acc.device)
    conf = torch.empty(vox, dtype=torch.float32, device=acc.device)
    ent = torch.empty(vox, dtype=torch.float32, device=acc.device)
    ops.tta_finalize(acc, labels, conf, ent, probs_out=acc)
    probs = acc.permute(0, 4, 1, 2, 3)
    labels, conf, ent = labels.unsqueeze(1), conf.unsqueeze(1), ent.unsqueeze(1)
    if sd == 2:
        probs, labels, conf, ent = probs.squeeze(2), labels.squeeze(2), conf.squeeze(2), ent.squeeze(2)
    return TTAResult(probs, labels, conf, ent, len(masks))


def uncertainty_summary(labels: torch.Tensor, entropy: torch.Tensor, confidence: torch.Tensor,
                        num_classes: int) -> dict:
    """Per label 0 .. num_classes - 1: ``voxels`` (int64), ``mean_entropy`` and ``mean_confidence`` (float64,
    NaN for a label without voxels), as numpy arrays.  Two ``segmi_label_means`` launches."""
    lab = labels.contiguous()
    if lab.dtype not in (torch.uint8, torch.int32):
        lab = lab.to(torch.int32)
    es, cnt = ops.label_means(lab, entropy.contiguous(), num_classes)
    cs, _ = ops.label_means(lab, confidence.contiguous(), num_classes)
    n = cnt.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        me = np.where(n > 0, es.cpu().numpy() / n, np.nan)
        mc = np.where(n > 0, cs.cpu().numpy() / n, np.nan)
    return {"voxels": n, "mean_entropy": me, "mean_confidence": mc}
