"""Patch-based label fusion for multi-atlas segmentation on the MI355X (``csrc/patch_fusion.hip``, DESIGN.md
section 25): every atlas votes at every voxel with a weight given by how well its image patch fits the target's,
and, with a search radius, also from the neighbouring positions whose patches fit better (locally weighted voting
and the non-local fusion of Coupe et al. 2011, on intensities quantised to 8 bits).  Unlike STAPLE
(``seg/staple.py``) it compares intensities, judges every place on its own and repairs a residual shift that the
atlases share.  The atlas images and label maps must already lie on the target's grid."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .._arrays import ArrayLike, _is_integer, _raw, _require_gpu, _tensor, _to_device, _wrap

MAX_ATLASES = 16
MAX_CLASSES = 64
MAX_RADIUS = 3


@dataclass
class PatchFusionResult:
    labels: object                      # in the form of the target, in the dtype of the first label map
    confidence: object                  # float32 in the form of the target: the winner's share of the votes
    scores: Optional[object] = None     # int32 [K, *shape] when asked for (numpy for host inputs)


def _is_real(a) -> bool:
    return not a.is_complex() if isinstance(a, torch.Tensor) else a.dtype.kind in "fiub"


def _rank_range(name: str, a) -> tuple:
    """default range of an image: its order statistics at ranks floor(0.005 (N - 1)) and ceil(0.995 (N - 1))"""
    n = int(np.prod(tuple(a.shape)))
    klo, khi = int(math.floor(0.005 * (n - 1))), int(math.ceil(0.995 * (n - 1)))
    if isinstance(a, torch.Tensor) and a.is_cuda:
        s = torch.sort(a.reshape(-1).to(torch.float32)).values
        lo, hi = float(s[klo]), float(s[khi])
    else:
        v = (a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).reshape(-1).astype(np.float32)
        p = np.partition(v, (klo, khi))
        lo, hi = float(p[klo]), float(p[khi])
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{name}: its default intensity range ({lo}, {hi}) is not finite; pass intensity_ranges")
    if not hi > lo:
        raise ValueError(f"{name} is constant over its default intensity range (both ends are {lo}): there is nothing "
                         f"to compare")
    return lo, hi


def _bandwidth(bandwidth, min_h2) -> tuple:
    """(h2, min_h2) for ops.patch_fusion: h2 None = adaptive"""
    from .. import ops
    if isinstance(bandwidth, str):
        if bandwidth != "adaptive":
            raise ValueError(f"bandwidth must be \"adaptive\" or a number, got {bandwidth!r}")
        return None, min_h2
    if isinstance(bandwidth, bool) or not isinstance(bandwidth, (int, float, np.integer, np.floating)) or \
            not math.isfinite(float(bandwidth)) or float(bandwidth) != int(bandwidth) or \
            not 1 <= int(bandwidth) <= ops.PF_MAX_H2:
        raise ValueError(f"bandwidth must be \"adaptive\" or a whole number of squared 8-bit quanta per patch voxel in "
                         f"1 .. {ops.PF_MAX_H2}, got {bandwidth!r}")
    return int(bandwidth), min_h2


def _check_wide_labels(a_idx: int, a, num_classes: int) -> None:
    """a label type that the kernels do not read in place is narrowed to int32: its range is checked before"""
    if isinstance(a, torch.Tensor):
        if a.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32):
            return
        lo, hi = (int(v) for v in torch.aminmax(a))
    else:
        if a.dtype.kind == "b" or (a.dtype.kind == "i" and a.dtype.itemsize <= 4) or a.dtype.itemsize <= 1:
            return
        lo, hi = int(a.min()), int(a.max())
    if lo < 0 or hi >= num_classes:
        raise ValueError(f"patch_fusion: atlas {a_idx} holds the label {lo if lo < 0 else hi}, outside 0 .. "
                         f"{num_classes - 1}")


def patch_fusion(target: ArrayLike, atlas_images: Sequence[ArrayLike], atlas_labels: Sequence[ArrayLike],
                 num_classes: Optional[int] = None, *, patch_radius=1, search_radius=2, beta: float = 1.0,
                 bandwidth="adaptive", min_h2: int = 4, intensity_ranges=None, return_scores: bool = False,
                 device=None) -> PatchFusionResult:
    """Fuse the label maps of 1 .. 16 atlases onto ``target``.  Inputs are numpy arrays, tensors or ``Image``s of one
    shape, 2-D or 3-D; images are real-valued, label maps hold integers in 0 .. num_classes - 1 (``num_classes``
    defaults to the largest label + 1, at least 2).  A radius is one integer or one per axis (z, y, x), each 0 .. 3;
    ``search_radius=0`` is locally weighted voting.  ``bandwidth``: "adaptive" (the smallest patch distance among a
    voxel's candidates, at least ``min_h2`` per patch voxel) or a fixed number of squared 8-bit quanta per patch
    voxel.  ``intensity_ranges``: (lo, hi) for the target and then every atlas image (None: its 0.5 % and 99.5 %
    order statistics), mapped to 0 .. 255.  Every argument error is raised before the device is touched."""
    from .. import ops

    for name, seq in (("atlas_images", atlas_images), ("atlas_labels", atlas_labels)):
        if isinstance(seq, (np.ndarray, torch.Tensor)) or not hasattr(seq, "__len__"):
            raise TypeError(f"{name} must be a sequence, one entry per atlas")
    atlas_images, atlas_labels = list(atlas_images), list(atlas_labels)
    if len(atlas_images) != len(atlas_labels):
        raise ValueError(f"{len(atlas_images)} atlas images for {len(atlas_labels)} label maps")
    A = len(atlas_images)
    if not 1 <= A <= MAX_ATLASES:
        raise ValueError(f"1 .. {MAX_ATLASES} atlases, got {A}")
    t_raw = _raw(target)
    shape = tuple(t_raw.shape)
    if len(shape) not in (2, 3) or 0 in shape:
        raise ValueError(f"target must be a non-empty 2-D or 3-D image, got shape {shape}")
    i_raw, l_raw = [_raw(x) for x in atlas_images], [_raw(x) for x in atlas_labels]
    for a in range(A):
        if not _is_real(i_raw[a]):
            raise TypeError(f"atlas_images[{a}] has the dtype {i_raw[a].dtype}; images are real-valued")
        if not _is_integer(l_raw[a]):
            raise TypeError(f"atlas_labels[{a}] has the float dtype {l_raw[a].dtype}; label maps are integer")
        for what, x in ((f"atlas_images[{a}]", i_raw[a]), (f"atlas_labels[{a}]", l_raw[a])):
            if tuple(x.shape) != shape:
                raise ValueError(f"{what} has shape {tuple(x.shape)}, the target has {shape}")
    if not _is_real(t_raw):
        raise TypeError(f"target has the dtype {t_raw.dtype}; images are real-valued")
    h2, min_h2 = _bandwidth(bandwidth, min_h2)
    table = ops.patch_fusion_table(beta)
    ops.pf_check_args(A, 2 if num_classes is None else num_classes, patch_radius, search_radius, h2, min_h2)
    if intensity_ranges is None:
        intensity_ranges = [None] * (A + 1)
    intensity_ranges = list(intensity_ranges)
    if len(intensity_ranges) != A + 1:
        raise ValueError(f"intensity_ranges: one (lo, hi) for the target and one per atlas image ({A + 1}), got "
                         f"{len(intensity_ranges)}")
    names = ["target"] + [f"atlas_images[{a}]" for a in range(A)]
    images = [t_raw] + i_raw
    ranges = []
    for name, im, r in zip(names, images, intensity_ranges):
        if r is not None:
            if not hasattr(r, "__len__") or len(r) != 2:
                raise ValueError(f"intensity_ranges: (lo, hi) expected for {name}, got {r!r}")
            ranges.append(ops.quantise_range_check(r[0], r[1]))
        elif isinstance(im, torch.Tensor) and im.is_cuda:
            ranges.append(None)                            # a device image: its range is read on the device below
        else:
            ranges.append(ops.quantise_range_check(*_rank_range(name, im)))
    if num_classes is None:
        num_classes = max(max(int(a.max()) for a in l_raw) + 1, 2)
        ops.pf_check_args(A, num_classes, patch_radius, search_radius, h2, min_h2)
    for a in range(A):
        _check_wide_labels(a, l_raw[a], int(num_classes))
    dev = _require_gpu("segmantic_amd.seg.patch_fusion needs an MI355X", t_raw)
    if device is not None:
        dev = torch.device(device)
    quantised = []
    for name, im, r in zip(names, images, ranges):
        t = _tensor(im).to(dev).to(torch.float32).contiguous()
        if r is None:
            r = ops.quantise_range_check(*_rank_range(name, t))
        quantised.append(ops.quantise_u8(t, r[0], r[1]))
    labs = [_to_device(a, dev) for a in l_raw]
    if len({t.dtype for t in labs}) > 1:
        labs = [t.to(torch.int32) for t in labs]
    res = ops.patch_fusion(quantised[0], quantised[1:], labs, int(num_classes), patch_radius=patch_radius,
                           search_radius=search_radius, table=table, h2=h2, min_h2=min_h2, return_scores=return_scores,
                           return_confidence=True)
    out, best, total = res[:3]
    first = l_raw[0]
    dt = torch.from_numpy(np.empty(0, first.dtype)).dtype if isinstance(first, np.ndarray) else first.dtype
    if dt == torch.bool:
        dt = torch.uint8
    confidence = best.to(torch.float32) / total.to(torch.float32)
    scores = None
    if return_scores:
        scores = res[3].cpu().numpy() if isinstance(t_raw, np.ndarray) else res[3].to(t_raw.device)
    return PatchFusionResult(_wrap(target, out if out.dtype == dt else out.to(dt)), _wrap(target, confidence), scores)
