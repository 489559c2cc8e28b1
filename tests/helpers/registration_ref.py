"""numpy restatement of DESIGN.md section 23 (registration by mutual information): pyramid level, fixed bins, joint
histogram (``np.add.at``), metric, parameter matrices, pattern search and the whole registration, plus the analytic
phantom the tests register.  Written from the definitions, not from the package's code; the GPU tests compare
the two bit for bit.  ``fault=`` seeds one deliberate deviation, for the tests that show a gate can fail."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

UNIT = 1 << 16
IGNORE = 255
N_PARAMETERS = {2: {"translation": 2, "rigid": 3, "affine": 6}, 3: {"translation": 3, "rigid": 6, "affine": 12}}
FAULTS = ("truncate_q", "swap_axes", "border_clamp", "minus_first", "no_halving", "no_origin_shift")


class Grid:
    """data [z][y][x] (2-D: [y][x]) with spacing / origin (x, y[, z]) and a row-major direction matrix"""

    def __init__(self, data, spacing=None, origin=None, direction=None):
        self.data = np.ascontiguousarray(data)
        nd = self.data.ndim
        self.nd = nd
        self.size = tuple(reversed(self.data.shape))
        self.spacing = np.asarray(spacing if spacing is not None else [1.0] * nd, np.float64)
        self.origin = np.asarray(origin if origin is not None else [0.0] * nd, np.float64)
        self.direction = np.asarray(direction if direction is not None else np.eye(nd), np.float64).reshape(nd, nd)

    def volume(self):
        return self.data[None] if self.nd == 2 else self.data

    def centre(self):
        return self.origin + self.direction @ (0.5 * (np.asarray(self.size, np.float64) - 1.0) * self.spacing)

    def radius(self):
        return 0.5 * float(np.sqrt((((np.asarray(self.size, np.float64) - 1.0) * self.spacing) ** 2).sum()))

    def corners(self):
        """physical positions of the 2^nd corner voxels"""
        n = np.asarray(self.size, np.float64) - 1.0
        out = []
        for k in range(1 << self.nd):
            idx = np.array([n[d] if (k >> d) & 1 else 0.0 for d in range(self.nd)])
            out.append(self.origin + self.direction @ (idx * self.spacing))
        return np.array(out)


# ---------------------------------------------------------------------------- pyramid level
def shrink_factors(shape_zyx, factor):
    out = []
    for n in shape_zyx:
        f = factor
        while f > 1 and (n == 1 or n // f < 8):
            f //= 2
        out.append(f)
    return tuple(out)


def bin_shrink(vol, factors_zyx):
    """block means of vol [z][y][x]: float64 sum with x innermost and z outermost, / count, as float32"""
    fz, fy, fx = factors_zyx
    oz, oy, ox = vol.shape[0] // fz, vol.shape[1] // fy, vol.shape[2] // fx
    acc = np.zeros((oz, oy, ox), np.float64)
    for z in range(fz):
        for y in range(fy):
            for x in range(fx):
                acc = acc + vol[z:oz * fz:fz, y:oy * fy:fy, x:ox * fx:fx].astype(np.float64)
    return (acc / float(fz * fy * fx)).astype(np.float32)


def level_grid(g: Grid, data, factors_xyz, fault=None) -> Grid:
    f = np.asarray(factors_xyz, np.float64)
    origin = g.origin if fault == "no_origin_shift" else g.origin + g.direction @ (0.5 * (f - 1.0) * g.spacing)
    return Grid(data, g.spacing * f, origin, g.direction)


def fixed_bins(img, lo, hi, bins, mask_mean=None):
    scale = (bins - 1) / (float(hi) - float(lo))
    b = np.floor((img.astype(np.float64) - float(lo)) * scale + 0.5)
    out = np.clip(b, 0, bins - 1).astype(np.uint8)
    if mask_mean is not None:
        out[mask_mean < np.float32(0.5)] = IGNORE
    return out


# ---------------------------------------------------------------------------- index map, histogram
def index_map(moving: Grid, fixed: Grid, transform) -> np.ndarray:
    """3 x 4: fixed index (x, y, z, 1) -> continuous moving index; transform maps fixed to moving physical points"""
    nd = moving.nd
    a = fixed.direction @ np.diag(fixed.spacing)
    t = fixed.origin.copy()
    if transform is not None:
        tm = np.asarray(transform, np.float64)
        a = tm[:nd, :nd] @ a
        t = tm[:nd, :nd] @ t + tm[:nd, nd]
    inv = np.diag(1.0 / moving.spacing) @ np.linalg.inv(moving.direction)
    m = np.zeros((3, 4))
    m[:nd, :nd] = inv @ a
    m[:nd, 3] = inv @ (t - moving.origin)
    if nd == 2:
        m[2, 2] = 1.0
    return m


def joint_histogram(fbin, mov, maps, bins, mlo, mscale, fault=None):
    """int64 [T][bins][bins] and the number of samples that counted per candidate"""
    maps = np.asarray(maps, np.float64).reshape(-1, 3, 4)
    nz, ny, nx = mov.shape
    zi, yi, xi = np.nonzero(fbin != IGNORE)
    fb = fbin[zi, yi, xi].astype(np.int64)
    x, y, z = xi.astype(np.float64), yi.astype(np.float64), zi.astype(np.float64)
    movf = mov.astype(np.float64)
    out = np.zeros((len(maps), bins, bins), np.int64)
    counted = np.zeros(len(maps), np.int64)
    for t, m in enumerate(maps):
        c = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]
        n = (nx, ny, nz)
        if fault == "border_clamp":
            c = [np.clip(c[r], 0.0, n[r] - 1.0) for r in range(3)]
        ok = np.ones(x.shape, bool)
        for r in range(3):
            ok &= (c[r] >= 0.0) & (c[r] <= n[r] - 1.0)
        cx, cy, cz = (v[ok] for v in c)
        f = fb[ok]
        counted[t] = f.size
        fl = [np.floor(v) for v in (cx, cy, cz)]
        fr = [v - w for v, w in zip((cx, cy, cz), fl)]
        i0 = [w.astype(np.int64) for w in fl]
        i1 = [np.minimum(i0[r] + 1, n[r] - 1) for r in range(3)]
        val = np.zeros(cx.shape, np.float64)
        for corner in range(8):
            px = i1[0] if corner & 1 else i0[0]
            py = i1[1] if corner & 2 else i0[1]
            pz = i1[2] if corner & 4 else i0[2]
            w = fr[0] if corner & 1 else 1.0 - fr[0]
            w = w * (fr[1] if corner & 2 else 1.0 - fr[1])
            w = w * (fr[2] if corner & 4 else 1.0 - fr[2])
            val = val + w * movf[pz, py, px]
        b = np.clip((val - mlo) * mscale, 0.0, bins - 1.0)
        i = np.minimum(np.floor(b), bins - 2.0)
        tt = b - i
        q = np.floor(tt * 65536.0) if fault == "truncate_q" else np.floor(tt * 65536.0 + 0.5)
        q = q.astype(np.int64)
        i = i.astype(np.int64)
        if fault == "swap_axes":
            np.add.at(out[t], (i, f), UNIT - q)
            np.add.at(out[t], (i + 1, f), q)
        else:
            np.add.at(out[t], (f, i), UNIT - q)
            np.add.at(out[t], (f, i + 1), q)
    return out, counted


# ---------------------------------------------------------------------------- metric
def entropy(v):
    v = np.asarray(v, np.float64).reshape(-1)
    v = v[v > 0]
    h = 0.0
    for term in v * np.log(v):                           # one add per term, in ascending bin order
        h = h + term
    return -h


def metric_value(h, metric, min_samples):
    total = int(h.sum())
    if total == 0 or total / UNIT < min_samples:
        return -np.inf
    p = h.astype(np.float64) / float(total)
    pf = h.sum(axis=1).astype(np.float64) / float(total)
    pm = h.sum(axis=0).astype(np.float64) / float(total)
    h_fm, h_f, h_m = entropy(p), entropy(pf), entropy(pm)
    if metric == "mi":
        return h_f + h_m - h_fm
    return (h_f + h_m) / h_fm if h_fm > 0.0 else -np.inf


# ---------------------------------------------------------------------------- parameters
def rot_x(a):
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], np.float64)


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float64)


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float64)


def parameters_to_matrix(kind, nd, q, c, r):
    q = np.asarray(q, np.float64)
    assert q.shape == (N_PARAMETERS[nd][kind],)
    a = np.eye(nd)
    if kind != "translation":
        if nd == 3:
            a = rot_z(q[2] / r) @ rot_y(q[1] / r) @ rot_x(q[0] / r)
            rest = q[3:]
        else:
            a = rot_z(q[0] / r)[:2, :2]
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


# ---------------------------------------------------------------------------- search
def pattern_search(evaluate, q0, step, min_step, max_iterations, fault=None):
    q = np.array(q0, np.float64)
    value = float(evaluate([q])[0])
    evaluations, iterations = 1, 0
    signs = (-1.0, 1.0) if fault == "minus_first" else (1.0, -1.0)
    while step >= min_step and iterations < max_iterations:
        cands = []
        for k in range(q.size):
            for s in signs:
                c = q.copy()
                c[k] = c[k] + s * step
                cands.append(c)
        vals = np.asarray(evaluate(cands), np.float64)
        evaluations += len(cands)
        iterations += 1
        best = 0
        for j in range(1, len(vals)):
            if vals[j] > vals[best]:
                best = j
        if vals[best] > value:
            q, value = cands[best], float(vals[best])
        elif fault == "no_halving":
            step = step - 0.0
        else:
            step = step / 2.0
    return q, value, iterations, evaluations, step


# ---------------------------------------------------------------------------- the registration
@dataclass
class RefResult:
    transform: np.ndarray
    parameters: np.ndarray
    value: float
    iterations: List[int] = field(default_factory=list)
    evaluations: List[int] = field(default_factory=list)
    final_step: List[float] = field(default_factory=list)
    level_values: List[float] = field(default_factory=list)
    converged: bool = False


def initial_matrix(fixed: Grid, moving: Grid, initial):
    nd = fixed.nd
    if initial is None:
        return np.eye(nd + 1)
    if isinstance(initial, str):
        assert initial == "geometry"
        m = np.eye(nd + 1)
        m[:nd, nd] = moving.centre() - fixed.centre()
        return m
    return np.array(initial, np.float64)


def register_ref(fixed: Grid, moving: Grid, transform="rigid", metric="nmi", bins=32, levels=(4, 2, 1),
                 fixed_mask: Optional[Grid] = None, initial=None, min_overlap=0.25, max_iterations=200,
                 fault=None) -> RefResult:
    nd = fixed.nd
    m0 = initial_matrix(fixed, moving, initial)
    fvol, mvol = fixed.volume(), moving.volume()
    centre, radius = fixed.centre(), fixed.radius()
    q = np.zeros(N_PARAMETERS[nd][transform])
    res = RefResult(np.eye(nd + 1), q, -np.inf)
    converged = True
    for lv in levels:
        ff, mf = shrink_factors(fvol.shape, lv), shrink_factors(mvol.shape, lv)
        fimg = bin_shrink(fvol, ff)
        mimg = mvol if lv == 1 else bin_shrink(mvol, mf)
        flo, fhi = float(fimg.min()), float(fimg.max())
        mlo, mhi = float(mimg.min()), float(mimg.max())
        assert fhi > flo and mhi > mlo
        mmean = bin_shrink(fixed_mask.volume(), ff) if fixed_mask is not None else None
        fbin = fixed_bins(fimg, flo, fhi, bins, mmean)
        usable = int((fbin != IGNORE).sum())
        mscale = (bins - 1) / (mhi - mlo)
        lf = level_grid(fixed, fimg[0] if nd == 2 else fimg, tuple(reversed(ff))[:nd], fault)
        lm = level_grid(moving, mimg[0] if nd == 2 else mimg, tuple(reversed(mf))[:nd], fault)

        def evaluate(cands):
            maps = [index_map(lm, lf, m0 @ parameters_to_matrix(transform, nd, c, centre, radius)) for c in cands]
            h, _ = joint_histogram(fbin, mimg, maps, bins, mlo, mscale, fault)
            return [metric_value(t, metric, min_overlap * usable) for t in h]

        step = 2.0 * float(lf.spacing.min())
        q, value, its, evs, last = pattern_search(evaluate, q, step, step / 32.0, max_iterations, fault)
        res.iterations.append(its)
        res.evaluations.append(evs)
        res.final_step.append(last)
        res.level_values.append(value)
        converged = converged and last < step / 32.0
    res.parameters, res.value, res.converged = q, res.level_values[-1], converged
    res.transform = m0 @ parameters_to_matrix(transform, nd, q, centre, radius)
    return res


def tre(fixed: Grid, ta, tb) -> float:
    """target registration error: the largest distance between the two transforms' images of the fixed box's corners"""
    nd = fixed.nd
    worst = 0.0
    for p in fixed.corners():
        a = np.asarray(ta)[:nd, :nd] @ p + np.asarray(ta)[:nd, nd]
        b = np.asarray(tb)[:nd, :nd] @ p + np.asarray(tb)[:nd, nd]
        worst = max(worst, float(np.sqrt(((a - b) ** 2).sum())))
    return worst


# ---------------------------------------------------------------------------- phantom
_BLOBS = (  # centre (x, y, z) mm, sigma mm, amplitude
    ((-9.0, -6.0, -5.0), 5.0, 0.55), ((8.0, 7.0, 3.0), 4.0, 0.45), ((3.0, -9.0, 8.0), 3.5, 0.40),
    ((-6.0, 9.0, -8.0), 4.5, 0.35), ((10.0, -3.0, -9.0), 3.0, 0.30))
_ELLIPSOID = ((1.0, -1.0, 0.5), (17.0, 14.0, 12.0), 0.30)   # centre, semi-axes (mm), amplitude


def phantom(p):
    """intensity in 0 .. 1 at physical points p [..., 2 or 3] (2-D: the plane z = 0): Gaussian blobs + an ellipsoid"""
    p = np.asarray(p, np.float64)
    if p.shape[-1] == 2:
        p = np.concatenate([p, np.zeros(p.shape[:-1] + (1,))], axis=-1)
    v = np.zeros(p.shape[:-1])
    for c, s, a in _BLOBS:
        v = v + a * np.exp(-((p - np.asarray(c)) ** 2).sum(-1) / (2.0 * s * s))
    c, ax, a = _ELLIPSOID
    d = np.sqrt((((p - np.asarray(c)) / np.asarray(ax)) ** 2).sum(-1))
    v = v + a * np.clip((1.0 - d) * 6.0, 0.0, 1.0)
    return np.clip(v, 0.0, 1.0)


def _points(size_xyz, spacing, origin):
    nd = len(size_xyz)
    axes = [origin[d] + spacing[d] * np.arange(size_xyz[d], dtype=np.float64) for d in range(nd)]
    mesh = np.meshgrid(*reversed(axes), indexing="ij")            # [z][y][x] order
    return np.stack(list(reversed(mesh)), axis=-1)                # last axis (x, y[, z])


def centred_origin(size_xyz, spacing):
    return -0.5 * (np.asarray(size_xyz, np.float64) - 1.0) * np.asarray(spacing, np.float64)


def remap(v):
    """non-monotone intensity map of the second 'modality'"""
    return 1.0 - v * v + 0.15 * np.sin(9.0 * v)


def make_pair(truth, fixed_size=(48, 44, 40), fixed_spacing=(1.0, 1.0, 1.1), moving_size=(52, 50, 44),
              moving_spacing=(1.1, 0.9, 1.0), noise=0.01, seed=0):
    """(fixed, moving) Grids, float32: fixed(p) = phantom(p); moving(T(p)) = remap(phantom(p)) for the homogeneous
    ``truth`` = T (fixed -> moving physical points); both grids centred on the physical origin; seeded noise."""
    rng = np.random.default_rng(seed)
    nd = len(fixed_size)
    fo, mo = centred_origin(fixed_size, fixed_spacing), centred_origin(moving_size, moving_spacing)
    f = phantom(_points(fixed_size, fixed_spacing, fo))
    pm = _points(moving_size, moving_spacing, mo)
    inv = np.linalg.inv(np.asarray(truth, np.float64))
    src = pm @ inv[:nd, :nd].T + inv[:nd, nd]
    m = remap(phantom(src))
    f = f + noise * rng.standard_normal(f.shape)
    m = m + noise * rng.standard_normal(m.shape)
    return (Grid(f.astype(np.float32), fixed_spacing, fo), Grid(m.astype(np.float32), moving_spacing, mo))


def rigid_truth(fixed_size, fixed_spacing, angles_deg, shift):
    """homogeneous rigid matrix about the centre of a centred fixed grid (the origin)"""
    nd = len(fixed_size)
    a = np.deg2rad(np.asarray(angles_deg, np.float64))
    rot = rot_z(a[2]) @ rot_y(a[1]) @ rot_x(a[0]) if nd == 3 else rot_z(a[0])[:2, :2]
    m = np.eye(nd + 1)
    m[:nd, :nd] = rot
    m[:nd, nd] = shift
    return m
