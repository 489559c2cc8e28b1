"""Rigid / affine registration of two ``processing.Image`` s by mutual information, on the MI355X.

``register(fixed, moving)`` returns the homogeneous matrix that maps fixed physical points to moving physical
points: exactly what ``processing.apply_transform(moving, fixed, transform, ...)`` takes.  DESIGN.md section 23
is the definition: a block-mean pyramid, a joint intensity histogram with integer (fixed-point) weights built by
``segmi_joint_histogram`` for a batch of candidate transforms per launch, the metric in float64 on the host from
the integer table, and a deterministic pattern search over parameters measured in millimetres.  Every quantity
is defined operation by operation, so a registration is bit-equal to its numpy restatement
(``tests/helpers/registration_ref.py``) and the same from run to run.

``register_deformable(fixed, moving, initial=matrix)`` fits a cubic B-spline free-form deformation on top of such a
matrix: gradient ascent on the same metric minus a membrane penalty, the gradient an integer
sum built by ``segmi_ffd_gradient``, every step scored by exact histograms (``segmi_ffd_joint_histogram``) and
checked for folds (``segmi_ffd_jacobian``).  ``warp``, ``displacement_field`` and ``jacobian_determinant`` apply
and inspect the ``DeformableResult``; its restatement is ``tests/helpers/deformable_ref.py``.
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
BSPLINE = "bspline"                  # the kind of a ``DeformableResult`` in a transform file
MAX_CONTROL_POINTS = 32768           # SEGMI_FFD_MAX_CONTROL_POINTS
STEP_FACTORS = (2.0, 1.0, 0.5, 0.25)  # the four candidates of a deformable iteration, in units of the step
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


def _device(device):
    if not torch.cuda.is_available():
        raise RuntimeError("segmantic_amd registration runs on an MI355X (no CPU path)")
    return device or torch.device("cuda:0")


def _prepare_level(fvol, mvol, mask, gf: _Geometry, gm: _Geometry, lv: int, bins: int):
    """One pyramid level of a pair, as (ff, mf, fbin, mimg, mlo, mhi, mscale, usable, lgf, lgm): the shrink factors
    (z, y, x) of fixed and moving, the fixed bin volume, the moving level image (the finest level reads the native
    pixel type), its range and bin scale, the number of fixed samples that count, and the two level grids."""
    from .. import ops
    nd = len(gf.size)
    ff = ops.shrink_factors(fvol.shape, lv)
    mf = ops.shrink_factors(mvol.shape, lv)
    fimg = ops.bin_shrink(fvol, ff)
    mimg = mvol if lv == 1 else ops.bin_shrink(mvol, mf)
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
    return (ff, mf, fbin, mimg, mlo, mhi, (bins - 1) / (mhi - mlo), usable,
            level_geometry(gf, tuple(reversed(ff))[:nd]), level_geometry(gm, tuple(reversed(mf))[:nd]))


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
    dev = _device(device or (fixed.data.device if fixed.data.is_cuda else None))
    fvol, mvol = _volume(fixed, dev), _volume(moving, dev)
    mask = _volume(fixed_mask, dev) if fixed_mask is not None else None
    gf, gm = _Geometry.of(fixed), _Geometry.of(moving)
    centre, radius = grid_centre(gf), grid_radius(gf)
    q = np.zeros(N_PARAMETERS[nd][transform])
    res = RegistrationResult(np.eye(nd + 1), q, transform, metric, float("-inf"), initial=m0)
    converged = True
    for lv in levels:
        ff, _, fbin, mimg, mlo, mhi, mscale, usable, lgf, lgm = _prepare_level(fvol, mvol, mask, gf, gm, lv, bins)

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


# ---------------------------------------------------------------------------- deformable registration
@dataclass
class DeformableResult:
    """``control``: float64 [3, nz, ny, nx], the displacement in mm along the fixed image's array axes (components
    x, y, z) at the control points of a uniform cubic B-spline grid over the fixed image.  ``affine``: the
    (d+1) x (d+1) matrix A of T(p) = A (p + D_f u(p)), fixed -> moving physical points.  ``fixed``: the geometry of
    the fixed grid the control grid belongs to.  Per level, in the order run: ``levels`` (shrink factor), ``spans``
    (x, y, z), ``iterations``, ``evaluations``, ``final_step`` (mm) and ``level_values`` (the objective J).
    ``converged``: every level ended on its smallest step.  ``folded`` / ``min_jacobian``: voxels of the full fixed
    grid with det(I + du/ds) <= 0 and the smallest determinant."""
    control: np.ndarray
    affine: np.ndarray
    fixed: _Geometry
    metric: str
    value: float
    regularisation: float = 0.0
    levels: List[int] = field(default_factory=list)
    spans: List[tuple] = field(default_factory=list)
    iterations: List[int] = field(default_factory=list)
    evaluations: List[int] = field(default_factory=list)
    final_step: List[float] = field(default_factory=list)
    level_values: List[float] = field(default_factory=list)
    converged: bool = False
    folded: int = 0
    min_jacobian: float = 1.0
    kind: str = BSPLINE
    accepted: List[List[float]] = field(default_factory=list)   # per level: J at its start and after every move
    skipped_folds: int = 0


def control_spans(size, spacing, grid_spacing, n_levels: int):
    """Spans of the control grid per level, coarse to fine, each (x, y, z).  The coarsest level has
    ``max(1, floor(extent / (grid_spacing 2^(L-1)) + 0.5))`` spans per axis, ``extent = (size - 1) * spacing`` in mm;
    the spans double per level; an axis of extent 1 (and the z axis of a 2-D image) keeps one span.  More than
    32 768 control points on the finest level are refused."""
    nd = len(size)
    try:
        gs = np.asarray(grid_spacing, np.float64)
    except (TypeError, ValueError):
        gs = np.full((nd + 1,), np.nan)
    if gs.shape not in ((), (nd,)) or not (np.isfinite(gs).all() and (gs > 0).all()):
        raise ValueError(f"grid_spacing must be a positive number of mm or one per axis (x, y[, z]), got {grid_spacing!r}")
    gs = np.broadcast_to(gs, (nd,))
    first = []
    for n, sp, g in zip(size, spacing, gs):
        if int(n) == 1:
            first.append(1)
        else:
            first.append(max(1, int(np.floor((int(n) - 1) * float(sp) / (float(g) * 2.0 ** (n_levels - 1)) + 0.5))))
    first = first + [1] * (3 - nd)
    flat = [int(n) == 1 for n in size] + [True] * (3 - nd)
    out = [tuple(s if fl else s * 2 ** lv for s, fl in zip(first, flat)) for lv in range(n_levels)]
    points = int(np.prod([s + 3 for s in out[-1]]))
    if points > MAX_CONTROL_POINTS:
        raise ValueError(f"grid_spacing {grid_spacing!r} gives {points} control points on the finest level, at most "
                         f"{MAX_CONTROL_POINTS}: use a larger grid_spacing")
    return out


def _refine_axis(c: np.ndarray, axis: int) -> np.ndarray:
    c = np.moveaxis(c, axis, -1)
    n = c.shape[-1]
    out = np.empty(c.shape[:-1] + (2 * n - 3,), np.float64)
    out[..., 0::2] = (c[..., :-1] + c[..., 1:]) / 2.0
    out[..., 1::2] = ((c[..., :-2] + 6.0 * c[..., 1:-1]) + c[..., 2:]) / 8.0
    return np.moveaxis(out, -1, axis)


def refine_grid(control, flat=(False, False, False)) -> np.ndarray:
    """Exact uniform cubic B-spline subdivision of a control grid [3, nz, ny, nx]: the spans double along x, then y,
    then z (not along an axis marked in ``flat`` = (x, y, z)); new even points are ``(c_i + c_{i+1}) / 2``, new odd
    points ``((c_i + 6 c_{i+1}) + c_{i+2}) / 8``.  The refined field equals the coarse one."""
    phi = np.asarray(control, np.float64)
    if phi.ndim != 4 or phi.shape[0] != 3 or min(phi.shape[1:]) < 4:
        raise ValueError(f"a control grid is [3, nz, ny, nx] with at least 4 points per axis, got {phi.shape}")
    for axis, fl in zip((3, 2, 1), flat):
        if not fl:
            phi = _refine_axis(phi, axis)
    return np.ascontiguousarray(phi)


def _control_spacing(size3, spacing3, n_xyz):
    """control spacing h in mm per axis (x, y, z); 0 on an axis of extent 1"""
    return [0.0 if d == 1 else (d - 1) * float(sp) / float(n - 3) for d, sp, n in zip(size3, spacing3, n_xyz)]


def _regulariser(phi: np.ndarray, h) -> float:
    total = 0.0
    for axis, hb in zip((3, 2, 1), h):
        if hb == 0.0:
            continue
        d = np.diff(phi, axis=axis)
        total = total + float((d * d).sum()) / float(d[0].size) / (hb * hb)
    return total


def _regulariser_gradient(phi: np.ndarray, h) -> np.ndarray:
    g = np.zeros(phi.shape, np.float64)
    for axis, hb in zip((3, 2, 1), h):
        if hb == 0.0:
            continue
        d = np.diff(phi, axis=axis)
        c = 2.0 / float(d[0].size) / (hb * hb)
        lo, hi = [slice(None)] * 4, [slice(None)] * 4
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        g[tuple(hi)] += c * d
        g[tuple(lo)] -= c * d
    return g


def derivative_table(h: np.ndarray, metric: str):
    """(max|D|, Qd) of one int64 [B, B] table: ``Lt`` = the derivative of the metric by a cell's probability up to
    the constants that cancel (0 in empty cells), ``D[f][i] = Lt[f][i+1] - Lt[f][i]``, ``Qd = rint(D / max|D| * 2^15)``
    as int32 (all zero when ``max|D|`` is 0)."""
    total = float(int(h.sum()))
    p = h.astype(np.float64) / total
    pf = h.sum(axis=1).astype(np.float64) / total
    pm = h.sum(axis=0).astype(np.float64) / total
    some = h > 0
    lp = np.where(some, np.log(np.where(some, p, 1.0)), 0.0)
    lf = np.where(pf > 0, np.log(np.where(pf > 0, pf, 1.0)), 0.0)
    lm = np.where(pm > 0, np.log(np.where(pm > 0, pm, 1.0)), 0.0)
    if metric == "mi":
        lt = (lp - lf[:, None]) - lm[None, :]
    else:
        h_fm = _entropy(p.reshape(-1))
        s = (_entropy(pf) + _entropy(pm)) / h_fm
        lt = (((-lf[:, None]) - lm[None, :]) + s * lp) / h_fm
    lt = np.where(some, lt, 0.0)
    d = lt[:, 1:] - lt[:, :-1]
    dmax = float(np.abs(d).max())
    if dmax == 0.0 or not np.isfinite(dmax):
        return 0.0, np.zeros(d.shape, np.int32)
    return dmax, np.rint(d / dmax * 32768.0).astype(np.int32)


def _geometry3(g):
    """(size, spacing, direction 3 x 3) of a 2-D or 3-D geometry as a depth-1 volume"""
    nd = len(g.size)
    d = np.eye(3)
    d[:nd, :nd] = np.asarray(g.direction, np.float64).reshape(nd, nd)
    return tuple(g.size) + (1,) * (3 - nd), tuple(g.spacing) + (1.0,) * (3 - nd), d


def _r_matrix(moving_geometry, fixed_geometry, affine) -> np.ndarray:
    """3 x 3: a millimetre of u along the fixed array axes -> index units of the moving grid"""
    nd = len(fixed_geometry.size)
    a = np.asarray(affine, np.float64)[:nd, :nd]
    dm = np.asarray(moving_geometry.direction, np.float64).reshape(nd, nd)
    df = np.asarray(fixed_geometry.direction, np.float64).reshape(nd, nd)
    small = np.diag(1.0 / np.asarray(moving_geometry.spacing, np.float64)) @ np.linalg.inv(dm) @ a @ df
    r = np.zeros((3, 3))
    r[:nd, :nd] = small
    return r


def _check_deformable(fixed, moving, initial, grid_spacing, levels, metric, bins, regularisation, fixed_mask,
                      min_overlap, max_iterations):
    nd, levels, a0 = _check(fixed, moving, "affine", metric, bins, levels, fixed_mask, initial, min_overlap,
                            max_iterations)
    try:
        lam = float(regularisation)
    except (TypeError, ValueError):
        lam = float("nan")
    if not (np.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"regularisation must be a finite number >= 0, got {regularisation!r}")
    spans = control_spans(fixed.GetSize(), fixed.spacing, grid_spacing, len(levels))
    return nd, levels, a0, lam, spans


def register_deformable(fixed: Image, moving: Image, *, initial=None, grid_spacing=16.0,
                        levels: Sequence[int] = (4, 2, 1), metric: str = "nmi", bins: int = 32,
                        regularisation: float = 0.01, fixed_mask: Optional[Image] = None, min_overlap: float = 0.25,
                        max_iterations: int = 60, device=None) -> DeformableResult:
    """Register ``moving`` to ``fixed`` with a cubic B-spline free-form deformation on top of the affine matrix
    ``initial`` (fixed -> moving; typically ``register(..., transform="affine").transform``; None = identity),
    maximising ``metric - regularisation * membrane energy`` by gradient ascent.
    ``grid_spacing``: the control spacing of the finest level in mm, a number or one per axis."""
    nd, levels, a0, lam, spans = _check_deformable(fixed, moving, initial, grid_spacing, levels, metric, bins,
                                                   regularisation, fixed_mask, min_overlap, max_iterations)
    from .. import ops
    dev = _device(device or (fixed.data.device if fixed.data.is_cuda else None))
    fvol, mvol = _volume(fixed, dev), _volume(moving, dev)
    mask = _volume(fixed_mask, dev) if fixed_mask is not None else None
    gf, gm = _Geometry.of(fixed), _Geometry.of(moving)
    size3, spacing3, _ = _geometry3(gf)
    flat = [d == 1 for d in size3]
    full = tuple(fvol.shape)
    res = DeformableResult(None, a0, gf, metric, float("-inf"), lam)
    phi = None
    converged = True
    for lv, sp in zip(levels, spans):
        n_xyz = tuple(s + 3 for s in sp)
        phi = np.zeros((3,) + tuple(reversed(n_xyz))) if phi is None else refine_grid(phi, flat)
        ff, _, fbin, mimg, mlo, mhi, mscale, usable, lgf, lgm = _prepare_level(fvol, mvol, mask, gf, gm, lv, bins)
        m = processing._index_map(lgm, lgf.spacing, lgf.origin, lgf.direction, a0)
        r = _r_matrix(lgm, gf, a0)
        gscale = 1.0 / ((mhi - mlo) * float(np.abs(r).sum(axis=1).max()))
        h = _control_spacing(size3, spacing3, n_xyz)
        inv_h = [0.0 if v == 0.0 else 1.0 / v for v in h]

        def score(grids: np.ndarray):
            dgrids = torch.from_numpy(np.ascontiguousarray(grids)).to(dev)
            hist = ops.ffd_joint_histogram(fbin, mimg, dgrids, full, ff, m, r, bins, mlo, mscale).cpu().numpy()
            s = metric_values(hist, metric, min_overlap * usable)
            return dgrids, hist, [float(v) - lam * _regulariser(g, h) for v, g in zip(s, grids)]

        _, hist, vals = score(phi[None])
        cur_h, cur = hist[0], vals[0]
        if not np.isfinite(cur):
            raise ValueError(f"initial leaves too little overlap at pyramid level {lv} (min_overlap {min_overlap})")
        step = float(lv) * float(min(gf.spacing))
        min_step = step / 32.0
        its, evs = 0, 1
        res.accepted.append([cur])
        while step >= min_step and its < int(max_iterations):
            dmax, qd = derivative_table(cur_h, metric)
            if dmax == 0.0:
                break
            gi = ops.ffd_gradient(fbin, mimg, torch.from_numpy(phi).to(dev), full, ff, m, r, bins, mlo, mscale, gscale,
                                  torch.from_numpy(qd).to(dev)).cpu().numpy()
            counted = int(cur_h.sum()) // UNIT
            scale = (((dmax * mscale) / gscale) / float(1 << 42)) / float(counted)
            g = gi.astype(np.float64) * scale - lam * _regulariser_gradient(phi, h)
            gmax = float(np.abs(g).max())
            if gmax == 0.0:
                break
            d = g / gmax
            cands = np.stack([phi + (step * c) * d for c in STEP_FACTORS])
            dgrids, hist, vals = score(cands)
            evs += len(cands)
            its += 1
            take = None
            for i in sorted(range(len(vals)), key=lambda k: (-vals[k], k)):   # descending J, the earlier one on ties
                if not vals[i] > cur:
                    break
                folded, _, _ = ops.ffd_jacobian(dgrids[i], fbin.shape, full, ff, inv_h)
                if int(folded.item()) == 0:
                    take = i
                    break
                res.skipped_folds += 1
            if take is None:
                step = step / 8.0
            else:
                phi, cur, cur_h = cands[take], vals[take], hist[take]
                res.accepted[-1].append(cur)
                step = step / 2.0 if STEP_FACTORS[take] == 0.25 else step * STEP_FACTORS[take]
        res.levels.append(int(lv))
        res.spans.append(tuple(sp))
        res.iterations.append(its)
        res.evaluations.append(evs)
        res.final_step.append(step)
        res.level_values.append(cur)
        converged = converged and step < min_step
    res.control = phi
    res.value = res.level_values[-1]
    res.converged = converged
    folded, lowest, _ = _jacobian(res, dev, False)
    res.folded, res.min_jacobian = int(folded.item()), float(lowest.item())
    return res


def _check_result(result, what: str) -> None:
    if not isinstance(result, DeformableResult):
        raise TypeError(f"{what} takes a DeformableResult, not {type(result).__name__}")
    c = np.asarray(result.control)
    if c.ndim != 4 or c.shape[0] != 3 or min(c.shape[1:]) < 4:
        raise ValueError(f"{what}: the control grid is [3, nz, ny, nx] with at least 4 points per axis, got {c.shape}")


def _jacobian(result: DeformableResult, dev, want_map: bool):
    from .. import ops
    size3, spacing3, _ = _geometry3(result.fixed)
    full = tuple(reversed(size3))
    h = _control_spacing(size3, spacing3, tuple(reversed(result.control.shape[1:])))
    control = torch.from_numpy(np.ascontiguousarray(result.control, dtype=np.float64)).to(dev)
    return ops.ffd_jacobian(control, full, full, (1, 1, 1), [0.0 if v == 0.0 else 1.0 / v for v in h], want_map)


def _same_grid(fixed: Image, g: _Geometry) -> bool:
    return (tuple(fixed.GetSize()) == tuple(g.size) and np.array_equal(np.asarray(fixed.spacing), np.asarray(g.spacing))
            and np.array_equal(np.asarray(fixed.origin), np.asarray(g.origin))
            and np.array_equal(np.asarray(fixed.direction), np.asarray(g.direction)))


def warp(moving: Image, fixed: Image, result: DeformableResult, nearest: bool = False, *, device=None) -> Image:
    """``moving`` resampled onto the grid of ``fixed`` through ``result`` (linear, or nearest for label maps), with the
    resampler's default value 0 and output cast.  ``fixed`` must have the geometry the transform was fitted on."""
    _check_result(result, "warp")
    for name, im in (("moving", moving), ("fixed", fixed)):
        if not isinstance(im, Image):
            raise TypeError(f"{name} must be a processing.Image, not {type(im).__name__}")
    if moving.GetDimension() != len(result.fixed.size):
        raise ValueError(f"dimension mismatch: the transform is {len(result.fixed.size)}-D, moving is "
                         f"{moving.GetDimension()}-D")
    if moving.data.dtype not in processing._NAME:
        raise TypeError(f"moving: unsupported pixel type {moving.data.dtype}")
    if not _same_grid(fixed, result.fixed):
        raise ValueError("fixed does not have the geometry the bspline transform was fitted on (size, spacing, origin "
                         "and direction must match)")
    from .. import ops
    dev = _device(device or (moving.data.device if moving.data.is_cuda else None))
    gm = _Geometry.of(moving)
    size3, _, _ = _geometry3(result.fixed)
    m = processing._index_map(gm, result.fixed.spacing, result.fixed.origin, result.fixed.direction, result.affine)
    r = _r_matrix(gm, result.fixed, result.affine)
    control = torch.from_numpy(np.ascontiguousarray(result.control, dtype=np.float64)).to(dev)
    out, _ = ops.ffd_warp(_volume(moving, dev), control, tuple(reversed(size3)), m, r, nearest=nearest)
    if moving.GetDimension() == 2:
        out = out[0]
    if not moving.data.is_cuda and device is None:
        out = out.cpu()
    return Image(out, result.fixed.spacing, result.fixed.origin, result.fixed.direction)


def displacement_field(result: DeformableResult, *, device=None) -> torch.Tensor:
    """float32 [3, z, y, x] (2-D: [2, y, x]) on the fixed grid: D_f u in mm along the physical axes (x, y[, z]),
    the non-rigid part of T(p) = A (p + D_f u); on the device."""
    _check_result(result, "displacement_field")
    from .. import ops
    dev = _device(device)
    size3, _, d3 = _geometry3(result.fixed)
    control = torch.from_numpy(np.ascontiguousarray(result.control, dtype=np.float64)).to(dev)
    _, disp = ops.ffd_warp(None, control, tuple(reversed(size3)), np.zeros((3, 4)), np.zeros((3, 3)), direction=d3,
                           want_displacement=True)
    return disp[:2, 0] if len(result.fixed.size) == 2 else disp


def jacobian_determinant(result: DeformableResult, *, device=None) -> torch.Tensor:
    """float32 [z, y, x] (2-D: [y, x]) on the fixed grid: det(I + du/ds); <= 0 where the transform folds"""
    _check_result(result, "jacobian_determinant")
    _, _, dmap = _jacobian(result, _device(device), True)
    return dmap[0] if len(result.fixed.size) == 2 else dmap

# ---------------------------------------------------------------------------- files
def _geometry_doc(g) -> dict:
    return {"size": list(g.size), "spacing": list(g.spacing), "origin": list(g.origin), "direction": list(g.direction)}


def save_transform(path, result, fixed: Optional[Image] = None) -> None:
    """JSON.  A ``RegistrationResult``: kind, matrix, parameters, initial matrix, the fixed grid, metric and value.
    A ``DeformableResult`` (kind ``"bspline"``): grid shape (nz, ny, nx), control values, affine part, its own fixed
    geometry (``fixed`` is not needed), metric, value and the per-level record."""
    if isinstance(result, DeformableResult):
        doc = {"kind": BSPLINE, "dimension": len(result.fixed.size), "grid": list(result.control.shape[1:]),
               "control": np.asarray(result.control, np.float64).reshape(-1).tolist(),
               "affine": np.asarray(result.affine, np.float64).tolist(), "fixed": _geometry_doc(result.fixed),
               "metric": result.metric, "value": result.value, "regularisation": result.regularisation,
               "levels": result.levels, "spans": [list(v) for v in result.spans], "iterations": result.iterations,
               "evaluations": result.evaluations, "final_step": result.final_step, "level_values": result.level_values,
               "converged": result.converged, "folded": result.folded, "min_jacobian": result.min_jacobian}
    else:
        if fixed is None:
            raise ValueError("save_transform: a matrix transform is saved with its fixed image")
        doc = {"kind": result.kind, "dimension": fixed.GetDimension(),
               "matrix": np.asarray(result.transform, np.float64).tolist(),
               "parameters": np.asarray(result.parameters, np.float64).tolist(),
               "initial": None if result.initial is None else np.asarray(result.initial, np.float64).tolist(),
               "fixed": _geometry_doc(_Geometry.of(fixed)),
               "metric": result.metric, "value": result.value, "levels": result.levels, "iterations": result.iterations,
               "evaluations": result.evaluations, "final_step": result.final_step, "converged": result.converged}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def _load_bspline(path, doc: dict) -> dict:
    for key in ("grid", "control", "affine", "fixed", "metric", "value"):
        if key not in doc:
            raise ValueError(f"{path}: not a bspline transform file (no {key!r})")
    nd = len(doc["fixed"]["size"])
    grid = tuple(int(v) for v in doc["grid"])
    control = np.asarray(doc["control"], np.float64)
    if len(grid) != 3 or min(grid) < 4 or control.size != 3 * grid[0] * grid[1] * grid[2]:
        raise ValueError(f"{path}: a bspline transform holds 3 x nz x ny x nx control values with at least 4 points "
                         f"per axis, got grid {grid} and {control.size} values")
    doc["control"] = control.reshape((3,) + grid)
    doc["affine"] = np.asarray(doc["affine"], np.float64)
    if doc["affine"].shape != (nd + 1, nd + 1):
        raise ValueError(f"{path}: a {nd}-D transform needs a {nd + 1} x {nd + 1} affine part, got {doc['affine'].shape}")
    f = doc["fixed"]
    doc["result"] = DeformableResult(
        doc["control"], doc["affine"], _Geometry(f["size"], f["spacing"], f["origin"], f["direction"]), doc["metric"],
        float(doc["value"]), float(doc.get("regularisation", 0.0)), list(doc.get("levels", [])),
        [tuple(v) for v in doc.get("spans", [])], list(doc.get("iterations", [])), list(doc.get("evaluations", [])),
        list(doc.get("final_step", [])), list(doc.get("level_values", [])), bool(doc.get("converged", False)),
        int(doc.get("folded", 0)), float(doc.get("min_jacobian", 1.0)))
    return doc


def load_transform(path) -> dict:
    """The document ``save_transform`` wrote, ``matrix`` (and ``parameters`` / ``initial``) as float64 arrays; Python's
    JSON writes a float64 with the digits that read back to the same bits.  For the kind ``"bspline"`` the document
    has ``control`` [3, nz, ny, nx] and ``affine`` as float64 arrays and ``result``, the ``DeformableResult``."""
    with open(path) as f:
        doc = json.load(f)
    if doc.get("kind") == BSPLINE:
        return _load_bspline(path, doc)
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
