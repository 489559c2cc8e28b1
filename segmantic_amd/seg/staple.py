"""Multi-label STAPLE label fusion (Warfield et al. 2004, in the multi-label form of ITK's
``MultiLabelSTAPLEImageFilter``) on the MI355X: an EM estimate of every rater's confusion matrix from the label
maps alone, and the fusion weighted by it (``csrc/staple.hip``).  The raters are the models
of an ensemble or human raters.  The by-products feed ``select_best``: ``performance_table`` lists sensitivity and
positive predictive value per rater and tissue, ``best_candidates`` picks the most sensitive rater per tissue.
Pooling over several volumes means adding their ``sums``."""
from __future__ import annotations

import csv
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .._arrays import ArrayLike, _is_integer, _raw, _require_gpu, _to_device, _back

Q = 1 << 24
MAX_RATERS = 16
MAX_CLASSES = 64


@dataclass
class StapleResult:
    labels: object                      # in the form and dtype of the first input
    confusion: np.ndarray               # theta, float64 [R, L, L]: P(rater r says l | truth s)
    sums: np.ndarray                    # int64 [R, L, L], S of the last M-step (Q = 2^24 per voxel)
    prior: np.ndarray                   # float64 [L]
    iterations: int
    converged: bool
    posterior: Optional[object] = None  # float32 [L, *shape] when asked for


def _totals(sums: np.ndarray) -> np.ndarray:
    """T[s] = sum over l of S[0][l][s] (every rater's column sums are equal)"""
    return sums[0].sum(axis=0)


def confusion_of(sums) -> np.ndarray:
    """theta[r][l][s] = S[r][l][s] / T[s] in float64, 0 where T[s] = 0"""
    sums = _check_sums(sums)
    T = np.broadcast_to(_totals(sums).astype(np.float64)[None, None, :], sums.shape)
    out = np.zeros(sums.shape, dtype=np.float64)
    np.divide(sums.astype(np.float64), T, out=out, where=T != 0)
    return out


def _check_sums(sums) -> np.ndarray:
    s = np.asarray(sums)
    if s.ndim != 3 or s.shape[1] != s.shape[2] or s.shape[0] < 1 or s.dtype.kind not in "iu":
        raise ValueError(f"sums must be an integer array [raters, L, L], got {s.dtype} {s.shape}")
    return s.astype(np.int64)


def _check_wide_labels(r: int, a, num_classes: int) -> None:
    """The kernels read 1, 2 or 4 signed bytes (uint8 apart).  A wider or unsigned type is narrowed to int32, which
    would wrap a label such as 2^32 + 1 into the range, so its range is checked while it still has its own type."""
    if isinstance(a, torch.Tensor):
        if a.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32):
            return
        lo, hi = (int(v) for v in torch.aminmax(a))
    else:
        if a.dtype.kind == "b" or (a.dtype.kind == "i" and a.dtype.itemsize <= 4) or a.dtype.itemsize <= 1:
            return
        lo, hi = int(a.min()), int(a.max())
    if lo < 0 or hi >= num_classes:
        raise ValueError(f"staple: rater {r} holds the label {lo if lo < 0 else hi}, outside 0 .. {num_classes - 1}")


def staple(labels: Sequence[ArrayLike], num_classes: Optional[int] = None, *, prior=None, max_iterations: int = 100,
           tolerance: float = 1e-5, return_posterior: bool = False) -> StapleResult:
    """Fuse 1 .. 16 label maps (numpy arrays, tensors or ``Image``s of one shape, 2-D or 3-D, integer labels in
    0 .. num_classes - 1; ``num_classes`` defaults to the largest label + 1, at least 2).  Every argument error is
    raised before the device is touched; a label type wider than int32 is range-checked before it is narrowed."""
    from .. import ops

    if isinstance(labels, (np.ndarray, torch.Tensor)) or not hasattr(labels, "__len__"):
        raise TypeError("labels must be a sequence of label maps, one per rater")
    labels = list(labels)
    if not 1 <= len(labels) <= MAX_RATERS:
        raise ValueError(f"labels: 1 .. {MAX_RATERS} raters, got {len(labels)}")
    raws = [_raw(x) for x in labels]
    for r, a in enumerate(raws):
        if not _is_integer(a):
            raise TypeError(f"labels[{r}] has the float dtype {a.dtype}; label maps are integer")
        if tuple(a.shape) != tuple(raws[0].shape):
            raise ValueError(f"labels[{r}] has shape {tuple(a.shape)}, labels[0] has {tuple(raws[0].shape)}")
    if len(raws[0].shape) not in (2, 3) or 0 in tuple(raws[0].shape):
        raise ValueError(f"labels must be non-empty 2-D or 3-D volumes, got shape {tuple(raws[0].shape)}")
    if num_classes is None:
        # what needs no label value is checked first: the largest label of a device tensor is a read-back
        ops.staple_check_args(len(raws), 2, None, max_iterations, tolerance)
        if prior is not None:
            if not 2 <= np.size(prior) <= MAX_CLASSES:
                raise ValueError(f"prior must hold num_classes (2 .. {MAX_CLASSES}) finite values, got {np.size(prior)}")
            ops.staple_check_args(len(raws), np.size(prior), np.ravel(prior), max_iterations, tolerance)
        top = max(int(a.max()) for a in raws)
        num_classes = max(top + 1, 2)
    if isinstance(num_classes, bool) or int(num_classes) != num_classes or not 2 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"num_classes must be an integer in 2 .. {MAX_CLASSES}, got {num_classes}")
    ops.staple_check_args(len(raws), num_classes, prior, max_iterations, tolerance)
    for r, a in enumerate(raws):
        _check_wide_labels(r, a, int(num_classes))
    dev = _require_gpu("segmantic_amd.seg.staple needs an MI355X", raws[0])
    ts = [_to_device(a, dev) for a in raws]
    if len({t.dtype for t in ts}) > 1:
        ts = [t.to(torch.int32) for t in ts]
    res = ops.staple(ts, int(num_classes), prior=prior, max_iterations=int(max_iterations), tolerance=float(tolerance),
                     return_posterior=return_posterior)
    out, sums, prior_out, it, converged = res[:5]
    sums_h = sums.cpu().numpy()
    first = labels[0]
    post = None
    if return_posterior:
        post = res[5].cpu().numpy() if isinstance(raws[0], np.ndarray) else res[5].to(raws[0].device)
    return StapleResult(_back(first, out), confusion_of(sums_h), sums_h, prior_out.cpu().numpy(), it, converged, post)


def _tissue_names(n_labels: int, tissues: Optional[Dict[str, int]]) -> List[str]:
    names = [str(s) for s in range(n_labels)]
    for name, idx in (tissues or {}).items():
        if 0 <= int(idx) < n_labels:
            names[int(idx)] = str(name)
    return names


def performance_table(sums, names: Optional[Sequence[str]] = None, tissues: Optional[Dict[str, int]] = None) -> List[dict]:
    """One row per (rater, label): ``rater`` (its name, default its index), ``label``, ``tissue``, ``sensitivity`` =
    theta_r[s][s], ``ppv`` = S[r][s][s] / sum_t S[r][s][t] and ``voxels`` = T[s] / Q (nan where undefined)."""
    sums = _check_sums(sums)
    R, L, _ = sums.shape
    if names is not None and len(names) != R:
        raise ValueError(f"names: {R} raters, got {len(names)} names")
    T = _totals(sums)
    tn = _tissue_names(L, tissues)
    rows = []
    for r in range(R):
        for s in range(L):
            said = int(sums[r, s].sum())
            rows.append({"rater": str(names[r]) if names is not None else r, "label": s, "tissue": tn[s],
                         "sensitivity": float(sums[r, s, s]) / float(T[s]) if T[s] else float("nan"),
                         "ppv": float(sums[r, s, s]) / float(said) if said else float("nan"),
                         "voxels": float(T[s]) / float(Q)})
    return rows


def best_candidates(sums, tissue_dict: Dict[str, int]) -> Dict[str, int]:
    """{tissue name: rater index} by the largest sensitivity, ties to the lowest index, tissues with T = 0 (or
    outside the table) left out: the file ``select_best`` loads from ``candidate_per_tissue_path``."""
    sums = _check_sums(sums)
    T = _totals(sums)
    out = {}
    for name, idx in tissue_dict.items():
        s = int(idx)
        if not 0 <= s < sums.shape[1] or T[s] == 0:
            continue
        out[str(name)] = int(np.argmax(sums[:, s, s]))     # one T[s] for every rater: largest S = largest theta
    return out


def write_performance_csv(rows: List[dict], path) -> None:
    with open(Path(path), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["rater", "label", "tissue", "sensitivity", "ppv", "voxels"])
        w.writeheader()
        for row in rows:
            w.writerow({k: (repr(v) if isinstance(v, float) else v) for k, v in row.items()})


def write_candidates(candidates: Dict[str, int], path) -> None:
    from ..utils import config
    config.dump(dict(candidates), config_file=Path(path))
