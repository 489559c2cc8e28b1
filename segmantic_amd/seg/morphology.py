"""Euclidean distance / feature transform and label morphology by a physical radius on the MI355X, computed by
the HIP kernels of ``csrc/morphology.hip``.  The names follow the libraries users come from:
``scipy.ndimage.distance_transform_edt`` / MONAI ``DistanceTransformEDT`` and scikit-image ``expand_labels``.
There is no CPU fallback: with no GPU every entry raises ``RuntimeError``.

Contract
--------
The definitions below are the specification; the tests check them against a numpy restatement
(``tests/helpers/morphology_ref.py``), bit for bit when all spacings are equal.

* Arrays are ``[z, y, x]`` (3-D) or ``[y, x]`` (2-D) with fewer than ``2^31`` voxels; label maps hold integers
  (``uint8``, ``int16`` and ``int32`` are read in place).  ``spacing`` / ``sampling`` is one positive number
  per array axis (a single number stands for all axes, ``None`` for 1).
* **Squared distance** between two voxels, in f64: with one spacing ``s`` for all axes
  ``float(dz^2 + dy^2 + dx^2) * (s * s)``, the sum in integers (exact); otherwise
  ``((sz dz)^2 + (sy dy)^2) + (sx dx)^2`` in exactly this order, so that voxels at mirrored offsets are
  exactly as far.  A radius ``r`` reaches a voxel when that value is ``<= float(r) * float(r)``.
* **Nearest feature** of a voxel: the feature voxel at the smallest squared distance; among equally near
  ones the smallest raster index wins (z, then y, then x).  The rule is part of the contract: results are
  canonical.  With unequal spacings candidates whose distances differ only by rounding (relative ``1e-9``)
  may be told apart differently than real arithmetic would.
* numpy arrays in -> numpy out, tensors in -> tensors on the input's device out,
  :class:`~segmantic_amd.image.processing.Image` in -> ``Image`` out (label operations and distances).  Label
  results keep the input's dtype.  The input is never modified.
* ``radius`` / ``distance`` are finite and ``>= 0`` (``ValueError`` otherwise); 0 is the identity.
* ``applied_labels`` lie in ``0 .. 65535`` and so do the values of a volume they are applied to.

Deviations from scipy / scikit-image: the tie rule (scipy leaves ties unspecified); a volume without any zero
voxel gives distances ``+inf`` and indices ``-1`` (scipy returns garbage there); distances are ``float32`` of
the f64 value, indices ``int32``; one-hot inputs are refused.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from .._arrays import ArrayLike, _back, _check_spacing, _raw, _require_gpu, _to_device, _wrap, _zyx
from .transforms import _channel_first, _check_applied, _check_labels, _Dict, _ops, _restore

_NEEDS_GPU = "segmantic_amd.seg.morphology needs an MI355X"
BOX_MAX_LABELS = 1024          # label boxes come from one pass for labels below this; larger ones use the volume


# ------------------------------------------------------------------ validation
def _check_radius(radius, what: str = "radius") -> float:
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} must be a number, got {radius!r}")
    r = float(radius)
    if not (math.isfinite(r) and r >= 0.0):
        raise ValueError(f"{what} must be finite and >= 0, got {radius!r}")
    return r


def _applied_nonzero(applied_labels) -> Optional[list]:
    applied = _check_applied(applied_labels)
    return None if applied is None else [v for v in applied if v != 0]


# ------------------------------------------------------------------ device-tensor implementations
def _dilate(t: torch.Tensor, r: float, zyx: tuple, applied: Optional[list]) -> torch.Tensor:
    ops = _ops()
    if applied is None:
        index, _ = ops.feature_transform(t, ops.FT_NONZERO, zyx)
    else:
        table = torch.zeros(ops.FT_TABLE_SIZE, dtype=torch.uint8, device=t.device)
        table[torch.tensor(applied, dtype=torch.int64, device=t.device)] = 1
        index, _ = ops.feature_transform(t, ops.FT_TABLE, zyx, table=table)
    return ops.morph_gather(t, index, zyx, r)


def _label_boxes(t: torch.Tensor, applied: Optional[list]):
    """-> [(label, half-open box z0 z1 y0 y1 x0 x1)] of the applied labels that occur; the one host
    synchronisation of an erosion"""
    ops = _ops()
    d, h, w = (1,) + tuple(t.shape) if t.dim() == 2 else tuple(t.shape)
    if applied is None:
        applied = [int(v) for v in torch.unique(t).tolist() if v != 0]
    out = []
    small = [v for v in applied if v < BOX_MAX_LABELS]
    if small:
        k = max(small) + 1
        boxes = torch.empty((k, 6), dtype=torch.int32, device=t.device)
        counts = torch.empty((k, 2), dtype=torch.int64, device=t.device)
        ops.label_boxes(t, t, k, boxes, counts)
        host = boxes.cpu().numpy()
        out += [(v, [int(b) for b in host[v]]) for v in small if host[v][1] > host[v][0]]
    large = [v for v in applied if v >= BOX_MAX_LABELS]
    if large:
        present = torch.isin(torch.tensor(large, dtype=t.dtype, device=t.device), t).tolist()
        out += [(v, [0, d, 0, h, 0, w]) for v, there in zip(large, present) if there]
    return out, (d, h, w)


def _erode(t: torch.Tensor, r: float, zyx: tuple, applied: Optional[list],
           keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    ops = _ops()
    out = t.clone()
    boxes, dims = _label_boxes(t, applied)
    for label, box in boxes:
        grown = []
        for a in range(3):
            # every voxel within r of the label lies at most ceil(r / spacing) voxels outside its box
            g = min(int(math.ceil(r / zyx[a])), dims[a]) + 1
            grown += [max(box[2 * a] - g, 0), min(box[2 * a + 1] + g, dims[a])]
        index, _ = ops.feature_transform(t, ops.FT_NOT_EQUAL, zyx, label=label, box=grown)
        ops.morph_erode_select(t, label, grown, index, zyx, r, out, keep=keep)
    return out


def _prepare(labels: ArrayLike, spacing):
    a = _check_labels(labels)
    sp = _check_spacing(spacing, len(a.shape))
    return a, _zyx(sp)


# ------------------------------------------------------------------ functions
def distance_transform_edt(img: ArrayLike, sampling=None, return_distances: bool = True,
                           return_indices: bool = False, squared: bool = False):
    """``scipy.ndimage.distance_transform_edt``: for every non-zero voxel the distance to the nearest zero
    voxel (zero voxels get 0), as ``float32`` of the square root of the f64 squared distance
    (``squared=True``: of the squared distance itself, an exact integer for unit spacing), and / or the
    ``int32 [ndim, ...]`` coordinates of that zero voxel.  Returns the distances, the indices, or the tuple
    of both.  Deviations from scipy: ties go to the smallest raster index (scipy leaves them unspecified),
    and an input without any zero voxel gives distances ``+inf`` and indices ``-1`` (scipy returns garbage)."""
    if not (return_distances or return_indices):
        raise ValueError("at least one of return_distances / return_indices must be True")
    a = _raw(img)
    shape = tuple(int(s) for s in a.shape)
    if len(shape) not in (2, 3) or 0 in shape or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
        raise ValueError(f"distance_transform_edt: inputs are 2-D or 3-D with 1 .. 2^31 - 1 voxels, got shape {shape}")
    zyx = _zyx(_check_spacing(sampling, len(shape)))
    dev = _require_gpu(_NEEDS_GPU)
    ops = _ops()
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = t.to(dev)
    if t.dtype not in (torch.uint8, torch.int16, torch.int32):
        t = (t != 0).to(torch.uint8)
    t = t.contiguous()
    index, dist = ops.feature_transform(t, ops.FT_ZERO, zyx, with_dist=return_distances, dist_sqrt=not squared)
    res = []
    if return_distances:
        res.append(_wrap(img, dist))
    if return_indices:
        planes = ops.morph_index_planes(index)
        res.append(planes.cpu().numpy() if isinstance(a, np.ndarray) else planes.to(a.device))
    return res[0] if len(res) == 1 else tuple(res)


def nearest_label(labels: ArrayLike, spacing=None):
    """Every voxel takes the value of its nearest non-zero voxel (its own when it is non-zero); ties go to
    the smallest raster index.  A volume of zeros stays as it is."""
    a, zyx = _prepare(labels, spacing)
    dev = _require_gpu(_NEEDS_GPU)
    return _back(labels, _dilate(_to_device(a, dev), math.inf, zyx, None))


def expand_labels(labels: ArrayLike, distance=1, spacing=None):
    """scikit-image's ``expand_labels``: a background (0) voxel whose nearest labelled voxel lies within
    ``distance`` (``<=``) takes that voxel's label; labelled voxels never change.  Where two labels are equally
    near, the voxel with the smallest raster index gives its label."""
    a, zyx = _prepare(labels, spacing)
    r = _check_radius(distance, "distance")
    dev = _require_gpu(_NEEDS_GPU)
    t = _to_device(a, dev)
    return _back(labels, t.clone() if r == 0.0 else _dilate(t, r, zyx, None))


def dilate_labels(labels: ArrayLike, radius, spacing=None, applied_labels: Optional[Sequence[int]] = None):
    """``expand_labels`` in which only the voxels of ``applied_labels`` are features (default: every label):
    a background voxel within ``radius`` of one takes the label of the nearest."""
    a, zyx = _prepare(labels, spacing)
    r = _check_radius(radius)
    applied = _applied_nonzero(applied_labels)
    dev = _require_gpu(_NEEDS_GPU)
    t = _to_device(a, dev, check_range=applied is not None)
    if r == 0.0 or applied == []:
        return _back(labels, t.clone())
    return _back(labels, _dilate(t, r, zyx, applied))


def erode_labels(labels: ArrayLike, radius, spacing=None, applied_labels: Optional[Sequence[int]] = None):
    """A voxel of an applied label ``L`` (default: every non-zero label) becomes 0 when some voxel of the
    volume with a value ``!= L`` lies within ``radius`` (``<=``).  Outside the volume there are no voxels, so
    the array border does not erode; this matches ``distance_transform_edt``."""
    a, zyx = _prepare(labels, spacing)
    r = _check_radius(radius)
    applied = _applied_nonzero(applied_labels)
    dev = _require_gpu(_NEEDS_GPU)
    t = _to_device(a, dev, check_range=True)
    if r == 0.0 or applied == []:
        return _back(labels, t.clone())
    return _back(labels, _erode(t, r, zyx, applied))


def open_labels(labels: ArrayLike, radius, spacing=None, applied_labels: Optional[Sequence[int]] = None):
    """``open_labels(labels, radius, ...)`` is ``dilate_labels(erode_labels(labels, ...), ...)``."""
    a, zyx = _prepare(labels, spacing)
    r = _check_radius(radius)
    applied = _applied_nonzero(applied_labels)
    dev = _require_gpu(_NEEDS_GPU)
    t = _to_device(a, dev, check_range=True)
    if r == 0.0 or applied == []:
        return _back(labels, t.clone())
    return _back(labels, _dilate(_erode(t, r, zyx, applied), r, zyx, applied))


def close_labels(labels: ArrayLike, radius, spacing=None, applied_labels: Optional[Sequence[int]] = None):
    """``close_labels(labels, radius, ...)`` is
    ``where(labels != 0, labels, erode_labels(dilate_labels(labels, ...), ...))``."""
    a, zyx = _prepare(labels, spacing)
    r = _check_radius(radius)
    applied = _applied_nonzero(applied_labels)
    dev = _require_gpu(_NEEDS_GPU)
    t = _to_device(a, dev, check_range=True)
    if r == 0.0 or applied == []:
        return _back(labels, t.clone())
    # a labelled voxel keeps its label through the dilation, so "where(labels != 0, labels, ...)" is the
    # erosion that leaves those voxels alone
    return _back(labels, _erode(_dilate(t, r, zyx, applied), r, zyx, applied, keep=t))


# ------------------------------------------------------------------ MONAI-style callables
class DistanceTransformEDT:
    """MONAI's ``DistanceTransformEDT``: channel-first ``[1, ...]`` inputs and plain arrays; the distances."""

    def __init__(self, sampling=None) -> None:
        self.sampling = sampling

    def __call__(self, img: ArrayLike):
        x, shape = _channel_first(img, None)
        return _restore(distance_transform_edt(x, self.sampling), shape)


class _Morph:
    _fn = None

    def __init__(self, radius, spacing=None, applied_labels: Optional[Sequence[int]] = None,
                 is_onehot: Optional[bool] = None) -> None:
        if is_onehot:
            raise ValueError("is_onehot=True: one-hot inputs are not supported, pass the label map (argmax)")
        self.radius = _check_radius(radius)
        self.spacing = spacing
        self.applied_labels = _check_applied(applied_labels)

    def __call__(self, img: ArrayLike):
        x, shape = _channel_first(img, None)
        return _restore(type(self)._fn(x, self.radius, self.spacing, self.applied_labels), shape)


class DilateLabels(_Morph):
    """:func:`dilate_labels` as a transform."""
    _fn = staticmethod(dilate_labels)


class ErodeLabels(_Morph):
    """:func:`erode_labels` as a transform."""
    _fn = staticmethod(erode_labels)


class OpenLabels(_Morph):
    """:func:`open_labels` as a transform."""
    _fn = staticmethod(open_labels)


class CloseLabels(_Morph):
    """:func:`close_labels` as a transform."""
    _fn = staticmethod(close_labels)


class DistanceTransformEDTd(_Dict):
    def __init__(self, keys, sampling=None, allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = DistanceTransformEDT(sampling)


class DilateLabelsd(_Dict):
    def __init__(self, keys, radius, spacing=None, applied_labels=None, allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = DilateLabels(radius, spacing, applied_labels)


class ErodeLabelsd(_Dict):
    def __init__(self, keys, radius, spacing=None, applied_labels=None, allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = ErodeLabels(radius, spacing, applied_labels)


class OpenLabelsd(_Dict):
    def __init__(self, keys, radius, spacing=None, applied_labels=None, allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = OpenLabels(radius, spacing, applied_labels)


class CloseLabelsd(_Dict):
    def __init__(self, keys, radius, spacing=None, applied_labels=None, allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = CloseLabels(radius, spacing, applied_labels)
