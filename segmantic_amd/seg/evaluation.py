"""Drop-in for ``segmantic.seg.evaluation`` (reference ``src/segmantic/seg/evaluation.py``) on the MI355X:
exact Euclidean distance transforms, Hausdorff and surface-distance metrics and confusion matrices,
computed by the HIP kernels of ``csrc/distance.hip``.  There is no CPU fallback: with no GPU every entry
raises ``RuntimeError``.

Contract
--------
* Arrays are indexed ``[z, y, x]`` (2-D: ``[y, x]``) and ``spacing`` is given per array axis.  An
  :class:`~segmantic_amd.image.processing.Image` carries ``(x, y, z)`` spacing, which is reversed.
* **Foreground** of a mask: voxels ``!= 0`` (for a label map and label ``c``: voxels ``== c``).
* **Contour** of a mask: foreground voxels with at least one face neighbour (6 in 3-D, 4 in 2-D; a 2-D
  input never looks along z) that is background; a neighbour outside the image is background.  This is
  MONAI's ``get_mask_edges`` and is taken to be ITK's ``BinaryContour(fullyConnected=False)``.
* ``d(p, F)``: physical Euclidean distance from voxel centre ``p`` to the nearest voxel of ``F``.  For a
  query point outside a mask, the distance to the mask equals the distance to its contour: a nearest
  foreground voxel always has a background face neighbour that lies closer to ``p``.  One signed contour
  transform per volume therefore serves both query kinds below.
* **Directed statistics** per label and direction: count, sum, sum of squares and max of
  ``d(q, target)`` over the query set, plus exact order statistics where needed.
  *surface*: query = contour(A), target = contour(B);  *pointwise*: query = foreground(A),
  target = foreground(B) (points inside B have distance 0, the reference's clamp of ``<= 0`` to 0).
* Derived on the host, in f64: the reference's ``hausdorff_surface_distance`` /
  ``hausdorff_pointwise_distance`` (mean, median as ``np.median``, std with ``ddof=0``, max over both
  directions concatenated); ITK ``HausdorffDistanceImageFilter`` (``hausdorff`` = pointwise max,
  ``average_hausdorff`` = mean of the two directed pointwise means); MONAI
  ``HausdorffDistanceMetric(percentile=p)`` (the larger directed surface percentile, ``np.percentile``
  linear interpolation; ``p=None`` gives the surface max).
* A label absent from one or both volumes gets NaN for every distance value; its voxel counts are still
  reported.  The two reference functions raise ``ValueError`` on an empty mask.

``confusion_matrix`` returns ``cm[true, pred]`` as its docstring and sklearn define it.  The reference's
numba branch loops over ``range(num_classes)`` instead of the voxels and its fallback swaps the indices;
neither bug is reproduced here.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .._arrays import ArrayLike, Image, _is_integer, _raw, _require_gpu, _tensor, _to_device

SURFACE_KEYS = ("mean", "median", "std", "max")
_NEEDS_GPU = "segmantic_amd.seg.evaluation runs on an MI355X only"


def _axis_spacing(x: ArrayLike, spacing: Optional[Sequence[float]]):
    """spacing per array axis: the argument, else an Image's own (x, y, z) reversed, else None"""
    return tuple(reversed(x.spacing)) if spacing is None and isinstance(x, Image) else spacing


def _prepare_pair(y_pred: ArrayLike, y_ref: ArrayLike, spacing: Optional[Sequence[float]]):
    """Validate a volume pair (host only) -> (pred, ref, spacing_zyx (3 floats), spatial dims)."""
    p, sp_p = _raw(y_pred), _axis_spacing(y_pred, spacing)
    r, sp_r = _raw(y_ref), _axis_spacing(y_ref, spacing)
    ndim = len(p.shape)
    if ndim not in (2, 3):
        raise ValueError(f"label volumes are 2-D or 3-D, got {ndim} dimensions")
    if tuple(p.shape) != tuple(r.shape):
        raise ValueError(f"shape mismatch: prediction {tuple(p.shape)} vs reference {tuple(r.shape)}")
    sp = sp_p if sp_p is not None else sp_r
    sp = [1.0] * ndim if sp is None else [float(s) for s in sp]
    if len(sp) != ndim:
        raise ValueError(f"spacing has {len(sp)} entries for a {ndim}-D volume")
    if not all(s > 0 and math.isfinite(s) for s in sp):
        raise ValueError(f"spacing must be positive and finite, got {sp}")
    if not (_is_integer(p) and _is_integer(r)):
        raise ValueError("label volumes must hold integers")
    sp3 = ([1.0] + sp) if ndim == 2 else sp
    return p, r, tuple(sp3), ndim


def _lerp(a: float, b: float, t: float) -> float:
    """np.percentile's linear interpolation (numpy's _lerp, including its t >= 0.5 form)"""
    diff = b - a
    return b - diff * (1.0 - t) if t >= 0.5 else a + diff * t


def _percentile_ranks(n: torch.Tensor, q: float) -> torch.Tensor:
    """ranks floor(q (n-1)) and the next one, on the device (n: i64 tensor)"""
    pos = (n.to(torch.float64) - 1.0).clamp_min(0.0) * q
    lo = torch.floor(pos).to(torch.int64)
    return torch.stack([lo, lo + 1], -1)


def _median_ranks(n: torch.Tensor) -> torch.Tensor:
    return torch.stack([(n - 1).clamp_min(0) // 2, n // 2], -1)


def _pct_host(n: int, q: float, v: np.ndarray) -> float:
    """np.percentile(values, 100 q) from the selected squared distances v = (rank lo, rank lo+1)"""
    if n == 0:
        return math.nan
    pos = q * (n - 1)
    lo = math.floor(pos)
    a = math.sqrt(float(v[0]))
    b = math.sqrt(float(v[1])) if lo + 1 < n else a
    return _lerp(a, b, pos - lo)


def _median_host(n: int, v: np.ndarray) -> float:
    if n == 0:
        return math.nan
    a, b = math.sqrt(float(v[0])), math.sqrt(float(v[1]))
    return a if n % 2 else (a + b) / 2.0


def _moments(stats: np.ndarray):
    """stats [m, 4] of directed samplings -> (mean, std ddof=0, max) over their concatenation"""
    n = stats[:, 0].sum()
    if n == 0:
        return math.nan, math.nan, math.nan
    mean = stats[:, 1].sum() / n
    var = max(stats[:, 2].sum() / n - mean * mean, 0.0)
    return float(mean), math.sqrt(var), float(stats[:, 3].max())


def _run(pred: torch.Tensor, ref: torch.Tensor, spacing_zyx, labels, k: int, percentile: Optional[float],
         medians: bool = True):
    """The evaluation of a volume pair on the device for the labels of ``labels`` (None: all present).

    Two host synchronisations: the box read-back (it sets the grid sizes) and the final statistics.
    Per present label: two signed contour EDTs over the label's box and four samplings (surface and
    point-wise, both directions).  Returns per-label host dicts."""
    from .. import ops

    dev = pred.device
    boxes = torch.empty((k, 6), dtype=torch.int32, device=dev)
    counts = torch.empty((k, 2), dtype=torch.int64, device=dev)
    ops.label_boxes(pred, ref, k, boxes, counts)
    bc = torch.cat([boxes.to(torch.int64).reshape(-1), counts.reshape(-1)]).cpu().numpy()  # synchronisation 1
    boxes_h, counts_h = bc[:6 * k].reshape(k, 6), bc[6 * k:].reshape(k, 2)
    todo = [c for c in (range(k) if labels is None else labels)
            if counts_h[c, 0] > 0 and counts_h[c, 1] > 0]
    out = {c: {"n_pred": int(counts_h[c, 0]), "n_ref": int(counts_h[c, 1])} for c in range(k)}
    if not todo:
        return out, boxes_h, counts_h
    vol = lambda c: int(np.prod(boxes_h[c, 1::2] - boxes_h[c, 0::2]))  # noqa: E731
    big = max(todo, key=vol)
    nvox = vol(big)
    dist = torch.empty(nvox, dtype=torch.float32, device=dev)
    ws = torch.empty(ops.edt_workspace_bytes(boxes_h[big]), dtype=torch.uint8, device=dev)
    sel_ws = torch.empty(ops.select_workspace_bytes(2), dtype=torch.uint8, device=dev)
    nt = len(todo)
    # per label: stats of the 4 samplings (0 pred->ref surface, 1 ref->pred surface, 2 / 3 point-wise)
    stats = torch.zeros((nt, 4, 4), dtype=torch.float64, device=dev)
    nvals = torch.zeros((nt, 4), dtype=torch.int64, device=dev)
    sel = torch.full((nt, 4, 2), math.nan, dtype=torch.float32, device=dev)
    q = None if percentile is None else float(percentile) / 100.0
    for i, c in enumerate(todo):
        box = boxes_h[c]
        npd, nrf = int(counts_h[c, 0]), int(counts_h[c, 1])
        # surface values: pred queries at [0, npd), ref queries at [npd, npd + nrf); the unused tail of
        # the first segment stays +inf, which sorts last, so [0, npd + n_ref_queries) holds the
        # concatenation for the median.  Point-wise queries fill their segments exactly.
        want_vals = medians or q is not None
        sv = torch.full((npd + nrf,), math.inf, dtype=torch.float32, device=dev) if want_vals else None
        pv = torch.empty((npd + nrf,), dtype=torch.float32, device=dev) if medians else None
        for j, (tgt, qry, off) in enumerate(((ref, pred, 0), (pred, ref, npd))):
            ops.edt_sq(tgt, c, 1, box, spacing_zyx, dist, ws)
            ops.edt_sample(dist, qry, c, 1, box, stats[i, j], ws,
                           sv[off:] if sv is not None else None, nvals[i, j] if sv is not None else None)
            ops.edt_sample(dist, qry, c, 0, box, stats[i, 2 + j], ws,
                           pv[off:] if pv is not None else None, nvals[i, 2 + j] if pv is not None else None)
        if q is not None:
            ranks = _percentile_ranks(nvals[i, :2], q).contiguous()
            ops.select_f32(sv, nvals[i, 0:1], ranks[0], sel[i, 0], sel_ws)
            ops.select_f32(sv[npd:], nvals[i, 1:2], ranks[1], sel[i, 1], sel_ws)
        if medians:
            ns = torch.stack([nvals[i, 0] + nvals[i, 1], nvals[i, 2] + nvals[i, 3]])
            mr = _median_ranks(ns).contiguous()
            n_cat = (nvals[i, 1:2] + npd).contiguous()
            ops.select_f32(sv, n_cat, mr[0], sel[i, 2], sel_ws)
            ops.select_f32(pv, ns[1:2].contiguous(), mr[1], sel[i, 3], sel_ws)
    packed = torch.cat([stats.reshape(-1), nvals.to(torch.float64).reshape(-1), sel.to(torch.float64).reshape(-1)])
    host = packed.cpu().numpy()                         # synchronisation 2
    st_h = host[:nt * 16].reshape(nt, 4, 4)
    nv_h = host[nt * 16:nt * 20].reshape(nt, 4).astype(np.int64)
    sel_h = host[nt * 20:].reshape(nt, 4, 2)
    for i, c in enumerate(todo):
        s = st_h[i]
        r = out[c]
        r["surface_mean"], r["surface_std"], r["surface_max"] = _moments(s[0:2])
        r["pointwise_mean"], r["pointwise_std"], r["pointwise_max"] = _moments(s[2:4])
        if medians:
            r["surface_median"] = _median_host(int(nv_h[i, 0] + nv_h[i, 1]), sel_h[i, 2])
            r["pointwise_median"] = _median_host(int(nv_h[i, 2] + nv_h[i, 3]), sel_h[i, 3])
        r["hausdorff"] = r["pointwise_max"]
        r["average_hausdorff"] = 0.5 * (s[2, 1] / s[2, 0] + s[3, 1] / s[3, 0])
        r["surface_mean_directed"] = (s[0, 1] / s[0, 0], s[1, 1] / s[1, 0])
        if q is None:
            r["percentile_hausdorff"] = r["surface_max"]
        else:
            r["percentile_hausdorff"] = max(_pct_host(int(nv_h[i, 0]), q, sel_h[i, 0]),
                                            _pct_host(int(nv_h[i, 1]), q, sel_h[i, 1]))
    return out, boxes_h, counts_h


def _binary(y_pred: ArrayLike, y_ref: ArrayLike, spacing, kind: str) -> Dict[str, float]:
    p, r, sp, _ = _prepare_pair(y_pred, y_ref, spacing)
    dev = _require_gpu(_NEEDS_GPU)
    p = (_tensor(p).to(dev) != 0).to(torch.uint8).contiguous()
    r = (_tensor(r).to(dev) != 0).to(torch.uint8).contiguous()
    res, _, _ = _run(p, r, sp, [1], 2, None)
    one = res[1]
    if one["n_pred"] == 0 or one["n_ref"] == 0:
        raise ValueError("empty mask: %s has no foreground voxels" % ("y_pred" if one["n_pred"] == 0 else "y_ref"))
    return {key: float(one[f"{kind}_{key}"]) for key in SURFACE_KEYS}


def hausdorff_surface_distance(y_pred: ArrayLike, y_ref: ArrayLike,
                               spacing: Optional[Sequence[float]] = None) -> Dict[str, float]:
    """Symmetric surface distances between two binary masks (reference ``evaluation.py:5-49``).

    ``Image`` inputs use their spacing (``useImageSpacing=True``); arrays / tensors take ``spacing`` per
    array axis (default 1).  Returns ``{"mean", "median", "std", "max"}`` over the distances of both
    contours to the other contour."""
    return _binary(y_pred, y_ref, spacing, "surface")


def hausdorff_pointwise_distance(y_pred: ArrayLike, y_ref: ArrayLike,
                                 spacing: Optional[Sequence[float]] = None) -> Dict[str, float]:
    """Symmetric point-wise distances between two binary masks (reference ``evaluation.py:52-93``):
    every foreground voxel of each mask to the other mask (0 inside it)."""
    return _binary(y_pred, y_ref, spacing, "pointwise")


RESULT_KEYS = ("surface_mean", "surface_median", "surface_std", "surface_max", "pointwise_mean",
               "pointwise_median", "pointwise_std", "pointwise_max", "hausdorff", "average_hausdorff",
               "percentile_hausdorff", "n_pred", "n_ref")


def surface_distances(pred_labels: ArrayLike, ref_labels: ArrayLike, num_classes: Optional[int] = None,
                      spacing: Optional[Sequence[float]] = None, percentile: Optional[float] = 95.0,
                      include_background: bool = False) -> Dict[str, np.ndarray]:
    """Distance metrics of every label of a predicted / reference label map pair.

    Returns float64 arrays indexed by label (``num_classes`` entries): the reference's surface and
    point-wise mean / median / std / max (``surface_*``, ``pointwise_*``), ITK's ``hausdorff`` and
    ``average_hausdorff``, MONAI's ``percentile_hausdorff`` (``percentile=None``: the surface max) and the
    voxel counts ``n_pred`` / ``n_ref``.  Distance values are NaN for a label absent from either volume and
    for label 0 unless ``include_background``.  ``num_classes=None`` reads the largest label back first
    (one more synchronisation)."""
    p, r, sp, _ = _prepare_pair(pred_labels, ref_labels, spacing)
    if percentile is not None and not 0.0 <= float(percentile) <= 100.0:
        raise ValueError(f"percentile must lie in [0, 100], got {percentile}")
    dev = _require_gpu(_NEEDS_GPU)
    p = _to_device(p, dev)
    r = _to_device(r, dev)
    if p.dtype != r.dtype:
        p, r = p.to(torch.int32), r.to(torch.int32)
    if num_classes is None:
        num_classes = int(torch.maximum(p.max(), r.max())) + 1
    k = int(num_classes)
    if k < 1:
        raise ValueError("num_classes must be positive")
    labels = list(range(0 if include_background else 1, k))
    res, _, _ = _run(p, r, sp, labels, k, percentile)
    out = {key: np.full(k, math.nan) for key in RESULT_KEYS}
    for c in range(k):
        for key, v in res[c].items():
            if key in out:
                out[key][c] = v
    return out


def confusion_matrix(num_classes: int, y_pred: ArrayLike, y: ArrayLike) -> np.ndarray:
    """float64 ``[num_classes, num_classes]`` with ``cm[true, pred]`` (sklearn's convention; reference
    ``evaluation.py:96-125``).  Labels outside ``[0, num_classes)`` raise ``ValueError``."""
    p, t = _raw(y_pred), _raw(y)
    if tuple(p.shape) != tuple(t.shape):
        raise ValueError(f"shape mismatch: {tuple(p.shape)} vs {tuple(t.shape)}")
    k = int(num_classes)
    if k < 1:
        raise ValueError("num_classes must be positive")
    dev = _require_gpu(_NEEDS_GPU)
    from .. import ops

    p = _to_device(p.reshape(-1), dev)
    t = _to_device(t.reshape(-1), dev)
    if p.dtype != t.dtype:
        p, t = p.to(torch.int32), t.to(torch.int32)
    cm = torch.empty((k, k), dtype=torch.int64, device=dev)
    if p.numel() == 0:
        return np.zeros((k, k))
    ops.confusion_counts(p, t, k, cm)
    out = cm.cpu().numpy().astype(np.float64)
    if int(out.sum()) != p.numel():
        raise ValueError(f"labels outside [0, {k}) in y_pred or y")
    return out
