"""Rigid / affine registration of two ``processing.Image`` s by mutual information, on the MI355X.

``register(fixed, moving)`` returns the homogeneous matrix that maps fixed physical points to moving physical
points: exactly what ``processing.apply_transform(moving, fixed, transform, ...)`` takes.  DESIGN.md section 23
is the definition: a block-mean pyramid, a joint intensity histogram with integer (fixed-point) weights built by
``segmi_joint_histogram`` for a batch of candidate transforms per launch, the metric in float64 on the host from
the integer table, and a deterministic pattern search over parameters measured in millimetres.  Every quantity
is defined operation by operation, so a registration is bit-equal to its numpy restatement
(``tests/helpers/registration_ref.py``) and the same from run to run.
"""
from __future__ import annotations

import json
import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import processing
from .processing import Image

TRANSFORMS = ("translation", "rigid", "affine")
METRICS = ("nmi", "mi")
BINS = (16, 32, 64)
LEVELS = (1, 2, 4, 8)
UNIT = 1 << 16                       # fixed-point weight of one sample in a joint histogram
IGNORE = 255                         # fixed bin of a sample that never counts
N_PARAMETERS = {2: {"translation": 2, "rigid": 3, "affine": 6}, 3: {"translation": 3, "rigid": 6, "affine": 12}}


@dataclass
class RegistrationResult:
    """``transform``: (d+1) x (d+1) float64, fixed -> moving physical points.  ``parameters``: the search's
    parameter vector (mm; see ``parameters_to_matrix``).  ``value``: the metric at the end of the last level.
    Per level, in the order run: ``levels`` (the shrink factor), ``iterations``, ``evaluations`` (candidates
    scored), ``final_step`` (mm) and ``level_values``.  ``converged``: every level ended on its smallest step."""
    transform: np.ndarray
    parameters: np.ndarray
    kind: str
    metric: str
    value: float
    levels: List[int] = field(default_factory=list)
    iterations: List[int] = field(default_factory=list)
    evaluations: List[int] = field(default_factory=list)
    final_step: List[float] = field(default_factory=list)
    level_values: List[float] = field(default_factory=list)
    converged: bool = False
    initial: Optional[np.ndarray] = None
    readback_seconds: float = 0.0


# ---------------------------------------------------------------------------- geometry
class _Geometry:
    """size (x, y[, z]), spacing, origin and direction of a grid: what ``processing._index_map`` reads of an image"""

    def __init__(self, size, spacing, origin, direction):
        self.size = tuple(int(v) for v in size)
        self.spacing = tuple(float(v) for v in spacing)
        self.origin = tuple(float(v) for v in origin)
        self.direction = tuple(float(v) for v in direction)

    @classmethod
    def of(cls, image: Image) -> "_Geometry":
        return cls(image.GetSize(), image.spacing, image.origin, image.direction)

    def GetDimension(self) -> int:
        return len(self.size)


def grid_centre(g) -> np.ndarray:
    """physical position of the middle of the grid: origin + D (0.5 (n - 1) spacing)"""
    nd = len(g.size)
    d = np.asarray(g.direction, np.float64).reshape(nd, nd)
    return np.asarray(g.origin, np.float64) + d @ (0.5 * (np.asarray(g.size, np.float64) - 1.0)
                                                  * np.asarray(g.spacing, np.float64))


def grid_radius(g) -> float:
    """half the physical diagonal between the first and the last voxel centre"""
    return 0.5 * float(np.sqrt((((np.asarray(g.size, np.float64) - 1.0) * np.asarray(g.spacing, np.float64)) ** 2).sum()))


def level_geometry(g: _Geometry, factors_xyz) -> _Geometry:
    """grid of the block means: spacing * factor, origin moved to the middle of the first block"""
    nd = len(g.size)
    f = np.asarray(factors_xyz, np.float64)
    sp = np.asarray(g.spacing, np.float64)
    d = np.asarray(g.direction, np.float64).reshape(nd, nd)
    origin = np.asarray(g.origin, np.float64) + d @ (0.5 * (f - 1.0) * sp)
    return _Geometry([n // int(k) for n, k in zip(g.size, factors_xyz)], sp * f, origin, g.direction)


# ---------------------------------------------------------------------------- parameters
def _rot(axis: int, a: float) -> np.ndarray:
    c, s = np.cos(a), np.sin(a)
    m = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    m[i, i], m[j, j] = c, c
    if axis == 1:
        m[i, j], m[j, i] = s, -s
    else:
        m[i, j], m[j, i] = -s, s
    return m


def parameters_to_matrix(kind: str, nd: int, q, centre, radius: float) -> np.ndarray:
    """(nd+1) x (nd+1) matrix of T(p) = A (p - c) + c + t.  One parameter unit is 1 mm, for an angle, a log-scale
    or a shear 1 mm of displacement at distance ``radius`` from ``centre``.
    3-D: translation q = t; rigid q = (rx, ry, rz, t), A = Rz(rz/r) Ry(ry/r) Rx(rx/r); affine q = (rx, ry, rz, s, k, t),
    A = R diag(exp(s/r)) U with U unit upper-triangular, k/r at (0,1), (0,2), (1,2).
    2-D: the in-plane subset: t; (rz, t); (rz, sx, sy, kxy, t)."""
    q = np.asarray(q, np.float64)
    if q.shape != (N_PARAMETERS[nd][kind],):
        raise ValueError(f"a {nd}-D {kind} transform has {N_PARAMETERS[nd][kind]} parameters, got {q.shape}")
    c = np.asarray(centre, np.float64)
    r = float(radius)
    a = np.eye(nd)
    if kind != "translation":
        if nd == 3:
            a = _rot(2, q[2] / r) @ _rot(1, q[1] / r) @ _rot(0, q[0] / r)
            rest = q[3:]
        else:
            a = _rot(2, q[0] / r)[:2, :2]
            rest = q[1:]
        if kind == "affine":
            u = np.eye(nd)
            if nd == 3:
                u[0, 1], u[0, 2], u[1, 2] = rest[3] / r, rest[4] / r, rest[5] / r
            else:
                u[0, 1] = rest[2] / r
            a = a @ np.diag(np.exp(rest[:nd] / r)) @ u
    t = q[-nd:]
    m = np.eye(nd + 1)
    m[:nd, :nd] = a
    m[:nd, nd] = (c + t) - a @ c
    return m


# ---------------------------------------------------------------------------- metric
def _entropy(v: np.ndarray) -> float:
    v = v[v > 0]
    if v.size == 0:
        return 0.0
    return -float(np.cumsum(v * np.log(v))[-1])          # cumsum: one add per term, in ascending bin order


def metric_values(hist: np.ndarray, metric: str, min_samples: float) -> np.ndarray:
    """float64 [T] of an int64 [T, B, B] table.  p = h / sum(h); the marginals come from the integer row and column
    sums; H(v) = -sum_{v > 0} v log v in ascending bin order; nmi = (H_f + H_m) / H_fm, mi = H_f + H_m - H_fm.
    -inf when fewer than ``min_samples`` samples counted, and for nmi when all of them share one cell."""
    out = np.full(hist.shape[0], -np.inf)
    for t, h in enumerate(hist):
        total = int(h.sum())
        if total == 0 or total / UNIT < min_samples:
            continue
        ft = float(total)
        h_fm = _entropy(h.reshape(-1).astype(np.float64) / ft)
        h_f = _entropy(h.sum(axis=1).astype(np.float64) / ft)
        h_m = _entropy(h.sum(axis=0).astype(np.float64) / ft)
        if metric == "mi":
            out[t] = h_f + h_m - h_fm
        elif h_fm > 0.0:
            out[t] = (h_f + h_m) / h_fm
    return out


# ---------------------------------------------------------------------------- search
def pattern_search(evaluate, q0: np.ndarray, step: float, min_step: float, max_iterations: int):
    """Deterministic batched pattern search that maximises ``evaluate(list of q) -> values``.  The start is scored
    once; an iteration scores q + step e_k, q - step e_k for ascending k in one call, moves to the first best
    candidate when it is strictly better, and halves the step otherwise.  Stops at step < min_step or after
    ``max_iterations``.  Returns (q, value, iterations, evaluations, step)."""
    q = np.array(q0, np.float64)
    value = float(evaluate([q])[0])
    evaluations, iterations = 1, 0
    n = q.size
    while step >= min_step and iterations < max_iterations:
        cands = []
        for k in range(n):
            for sign in (1.0, -1.0):
                c = q.copy()
                c[k] = c[k] + sign * step
                cands.append(c)
        vals = np.asarray(evaluate(cands), np.float64)
        evaluations += len(cands)
        iterations += 1
        best = int(np.argmax(vals))                      # the first of equal maxima
        if vals[best] > value:
            q, value = cands[best], float(vals[best])
        else:
            step = step / 2.0
    return q, value, iterations, evaluations, step


# ---------------------------------------------------------------------------- checks
def _check(fixed, moving, transform, metric, bins, levels, fixed_mask, initial, min_overlap, max_iterations):
    for name, im in (("fixed", fixed), ("moving", moving)):
        if not isinstance(im, Image):
            raise TypeError(f"{name} must be a processing.Image, not {type(im).__name__}")
        if im.GetDimension() not in (2, 3):
            raise ValueError(f"{name} must be 2-D or 3-D, got {im.GetDimension()}-D")
        if im.data.dtype not in processing._NAME:
            raise TypeError(f"{name}: unsupported pixel type {im.data.dtype}")
        if im.data.numel() == 0:
            raise ValueError(f"{name} is empty")
    nd = fixed.GetDimension()
    if moving.GetDimension() != nd:
        raise ValueError(f"dimension mismatch: fixed is {nd}-D, moving is {moving.GetDimension()}-D")
    if transform not in TRANSFORMS:
        raise ValueError(f"unknown transform {transform!r}: one of {', '.join(TRANSFORMS)}")
    if metric not in METRICS:
        raise ValueError(f"unknown metric {metric!r}: one of {', '.join(METRICS)}")
    if bins not in BINS:
        raise ValueError(f"bins must be one of {BINS}, got {bins!r}")
    try:
        levels = tuple(levels)
    except TypeError:
        raise ValueError(f"levels must be a sequence of pyramid factors among {LEVELS}, got {levels!r}")
    if not levels or any(lv not in LEVELS for lv in levels):
        raise ValueError(f"levels must be a non-empty sequence of pyramid factors among {LEVELS}, got {levels!r}")
    if not 0.0 <= float(min_overlap) <= 1.0:
        raise ValueError(f"min_overlap must lie in 0 .. 1, got {min_overlap!r}")
    if int(max_iterations) != max_iterations or int(max_iterations) < 1:
        raise ValueError(f"max_iterations must be an integer >= 1, got {max_iterations!r}")
    if grid_radius(_Geometry.of(fixed)) <= 0.0:
        raise ValueError("fixed holds a single voxel: nothing to register")
    if fixed_mask is not None:
        if not isinstance(fixed_mask, Image):
            raise TypeError(f"fixed_mask must be a processing.Image, not {type(fixed_mask).__name__}")
        if fixed_mask.GetSize() != fixed.GetSize():
            raise ValueError(f"fixed_mask has size {fixed_mask.GetSize()}, fixed has {fixed.GetSize()}")
        if fixed_mask.data.dtype not in processing._NAME:
            raise TypeError(f"fixed_mask: unsupported pixel type {fixed_mask.data.dtype}")
    if initial is None:
        m0 = np.eye(nd + 1)
    elif isinstance(initial, str):
        if initial != "geometry":
            raise ValueError(f"initial must be None, 'geometry' or a {nd + 1} x {nd + 1} matrix, got {initial!r}")
        m0 = np.eye(nd + 1)
        m0[:nd, nd] = grid_centre(_Geometry.of(moving)) - grid_centre(_Geometry.of(fixed))
    else:
        m0 = np.array(initial, np.float64)
        if m0.shape != (nd + 1, nd + 1) or not np.isfinite(m0).all():
            raise ValueError(f"initial must be None, 'geometry' or a finite {nd + 1} x {nd + 1} matrix")
    return nd, levels, m0


def _volume(image: Image, dev) -> torch.Tensor:
    t = image.data.to(dev).contiguous()
    return t.unsqueeze(0) if t.dim() == 2 else t


# ---------------------------------------------------------------------------- the registration
def register(fixed: Image, moving: Image, *, transform: str = "rigid", metric: str = "nmi", bins: int = 32,
             levels: Sequence[int] = (4, 2, 1), fixed_mask: Optional[Image] = None, initial=None,
             min_overlap: float = 0.25, max_iterations: int = 200, device=None) -> RegistrationResult:
    """Register ``moving`` to ``fixed``.  ``transform``: translation | rigid | affine.  ``metric``: nmi (Studholme's
    (H_f + H_m) / H_fm) | mi.  ``levels``: pyramid factors, run in the order given.  ``fixed_mask``: an image on
    the fixed grid; samples whose block mean of it is below 0.5 never count.  ``initial``: None (identity),
    "geometry" (the grid centres aligned) or a matrix; the search composes its transform after it.  A candidate
    scores -inf when fewer than ``min_overlap`` of the usable fixed samples land inside ``moving``."""
    nd, levels, m0 = _check(fixed, moving, transform, metric, bins, levels, fixed_mask, initial, min_overlap,
                            max_iterations)
    from .. import ops
    if not torch.cuda.is_available():
        raise RuntimeError("segmantic_amd registration runs on an MI355X (no CPU path)")
    dev = device or (fixed.data.device if fixed.data.is_cuda else torch.device("cuda:0"))
    fvol, mvol = _volume(fixed, dev), _volume(moving, dev)
    mask = _volume(fixed_mask, dev) if fixed_mask is not None else None
    gf, gm = _Geometry.of(fixed), _Geometry.of(moving)
    centre, radius = grid_centre(gf), grid_radius(gf)
    q = np.zeros(N_PARAMETERS[nd][transform])
    res = RegistrationResult(np.eye(nd + 1), q, transform, metric, float("-inf"), initial=m0)
    converged = True
    for lv in levels:
        ff = ops.shrink_factors(fvol.shape, lv)          # (z, y, x)
        mf = ops.shrink_factors(mvol.shape, lv)
        fimg = ops.bin_shrink(fvol, ff)
        mimg = mvol if lv == 1 else ops.bin_shrink(mvol, mf)   # the finest level reads the native pixel type
        flo, fhi = float(fimg.min()), float(fimg.max())
        mwide = mimg.to(torch.int32) if mimg.dtype == torch.uint16 else mimg
        mlo, mhi = float(mwide.min()), float(mwide.max())
        if not fhi > flo:
            raise ValueError(f"fixed is constant at pyramid level {lv}: no intensity to register")
        if not mhi > mlo:
            raise ValueError(f"moving is constant at pyramid level {lv}: no intensity to register")
        mmean = ops.bin_shrink(mask, ff) if mask is not None else None
        fbin = ops.fixed_bins(fimg, flo, fhi, bins, mmean)
        usable = int((fbin != IGNORE).sum())
        if usable == 0:
            raise ValueError(f"fixed_mask leaves no sample at pyramid level {lv}")
        mscale = (bins - 1) / (mhi - mlo)
        lgf = level_geometry(gf, tuple(reversed(ff))[:nd])
        lgm = level_geometry(gm, tuple(reversed(mf))[:nd])

        def evaluate(cands):
            maps = np.stack([processing._index_map(lgm, lgf.spacing, lgf.origin, lgf.direction,
                                                   m0 @ parameters_to_matrix(transform, nd, c, centre, radius))
                             for c in cands])
            vals = []
            for a in range(0, len(maps), ops.JOINT_HIST_MAX_CANDIDATES):
                h = ops.joint_histogram(fbin, mimg, maps[a:a + ops.JOINT_HIST_MAX_CANDIDATES], bins, mlo, mscale)
                torch.cuda.current_stream().synchronize()    # the copy below would wait for the launch anyway
                t0 = time.perf_counter()
                h = h.cpu().numpy()                      # the one read-back of the batch
                res.readback_seconds += time.perf_counter() - t0
                vals.append(metric_values(h, metric, min_overlap * usable))
            return np.concatenate(vals)

        step = 2.0 * min(lgf.spacing)
        q, value, its, evs, last = pattern_search(evaluate, q, step, step / 32.0, int(max_iterations))
        res.levels.append(int(lv))
        res.iterations.append(its)
        res.evaluations.append(evs)
        res.final_step.append(last)
        res.level_values.append(value)
        converged = converged and last < step / 32.0
    res.parameters = q
    res.value = res.level_values[-1]
    res.transform = m0 @ parameters_to_matrix(transform, nd, q, centre, radius)
    res.converged = converged
    return res


# ---------------------------------------------------------------------------- files
def save_transform(path, result: RegistrationResult, fixed: Image) -> None:
    """JSON: kind, matrix, parameters, initial matrix, the fixed grid, metric and value."""
    doc = {"kind": result.kind, "dimension": fixed.GetDimension(),
           "matrix": np.asarray(result.transform, np.float64).tolist(),
           "parameters": np.asarray(result.parameters, np.float64).tolist(),
           "initial": None if result.initial is None else np.asarray(result.initial, np.float64).tolist(),
           "fixed": {"size": list(fixed.GetSize()), "spacing": list(fixed.spacing), "origin": list(fixed.origin),
                     "direction": list(fixed.direction)},
           "metric": result.metric, "value": result.value, "levels": result.levels, "iterations": result.iterations,
           "evaluations": result.evaluations, "final_step": result.final_step, "converged": result.converged}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def load_transform(path) -> dict:
    """The document ``save_transform`` wrote, ``matrix`` (and ``parameters`` / ``initial``) as float64 arrays; Python's
    JSON writes a float64 with the digits that read back to the same bits."""
    with open(path) as f:
        doc = json.load(f)
    for key in ("kind", "matrix", "parameters", "fixed", "metric", "value"):
        if key not in doc:
            raise ValueError(f"{path}: not a transform file (no {key!r})")
    if doc["kind"] not in TRANSFORMS:
        raise ValueError(f"{path}: unknown transform kind {doc['kind']!r}")
    doc["matrix"] = np.asarray(doc["matrix"], np.float64)
    nd = len(doc["fixed"]["size"])
    if doc["matrix"].shape != (nd + 1, nd + 1):
        raise ValueError(f"{path}: a {nd}-D transform needs a {nd + 1} x {nd + 1} matrix, got {doc['matrix'].shape}")
    doc["parameters"] = np.asarray(doc["parameters"], np.float64)
    if doc.get("initial") is not None:
        doc["initial"] = np.asarray(doc["initial"], np.float64)
    return doc
