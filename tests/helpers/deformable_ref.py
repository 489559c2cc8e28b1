"""numpy float64 restatement of DESIGN.md section 24 (B-spline free-form deformable registration by mutual
information): the field, the joint histogram under candidate control grids, the derivative table, the integer
gradient (and its unquantised float64 form), the fold count, the warp, subdivision, the regulariser and the search,
plus the phantom pair the tests register.  Written from the definition; the GPU tests compare the two bit for bit.
``fault=`` seeds one deliberate deviation, for the tests that show a gate can fail."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

import registration_ref as rr

UNIT = 1 << 16
IGNORE = 255
QD_UNIT = 1 << 15
W_UNIT = 1 << 12
MAX_POINTS = 32768
MAX_SUPPORT = 1 << 20
STEP_FACTORS = (2.0, 1.0, 0.5, 0.25)
FAULTS = ("no_level_offset", "weights_k_plus_1", "r_transposed", "empty_cells_kept", "ties_last")


# ---------------------------------------------------------------------------- the B-spline, axis by axis
def span(j, F, dim, n, fault=None):
    """k (int64) and f of the level voxels j of one axis"""
    j = np.asarray(j, np.float64)
    if dim == 1:
        return np.zeros(j.shape, np.int64), np.zeros(j.shape, np.float64)
    off = 0.0 if fault == "no_level_offset" else 0.5 * float(F - 1)
    i = j * float(F) + off
    t = (i * float(n - 3)) / float(dim - 1)
    k = np.maximum(np.minimum(np.floor(t), float(n - 4)), 0.0)
    return k.astype(np.int64), t - k


def weights(f):
    g = 1.0 - f
    f2 = f * f
    f3 = f2 * f
    sixth = 1.0 / 6.0                                         # a multiplication, as the kernels do it
    return np.stack([((g * g) * g) * sixth, ((3.0 * f3 - 6.0 * f2) + 4.0) * sixth,
                     (((3.0 * f2 - 3.0 * f3) + 3.0 * f) + 1.0) * sixth, f3 * sixth], axis=-1)


def dweights(f):
    g = 1.0 - f
    f2 = f * f
    return np.stack([(g * g) * -0.5, 1.5 * f2 - 2.0 * f, (f - 1.5 * f2) + 0.5, f2 * 0.5], axis=-1)


def axis_tables(level_zyx, full_zyx, factors_zyx, n_zyx, fault=None):
    """per axis (z, y, x): k [l], w [l, 4], dw [l, 4]"""
    out = []
    for l, d, F, n in zip(level_zyx, full_zyx, factors_zyx, n_zyx):
        k, f = span(np.arange(l), F, d, n, fault)
        if fault == "weights_k_plus_1":
            k = np.minimum(k + 1, n - 4)
        out.append((k, weights(f), dweights(f)))
    return out


def displacement(phi, level_zyx, full_zyx, factors_zyx, fault=None):
    """u [3][lz][ly][lx] (components x, y, z; mm along the fixed array axes) of the control grid phi [3][nz][ny][nx]:
    the 64 terms ((wz wy) wx) * phi added from 0, z taps outermost and x taps innermost, ascending"""
    phi = np.asarray(phi, np.float64)
    (kz, wz, _), (ky, wy, _), (kx, wx, _) = axis_tables(level_zyx, full_zyx, factors_zyx, phi.shape[1:], fault)
    u = np.zeros((3,) + tuple(level_zyx), np.float64)
    for c in range(4):
        for b in range(4):
            wzy = wz[:, c][:, None, None] * wy[:, b][None, :, None]
            for a in range(4):
                w = wzy * wx[:, a][None, None, :]
                idx = np.ix_(kz + c, ky + b, kx + a)
                for comp in range(3):
                    u[comp] = u[comp] + w * phi[comp][idx]
    for comp, d in enumerate(reversed(tuple(full_zyx))):        # component x belongs to the last array axis
        if d == 1:
            u[comp] = 0.0
    return u


# ---------------------------------------------------------------------------- sampling
def _positions(fbin, u, m, r, fault=None):
    """the non-ignored level voxels (zi, yi, xi) and their continuous moving index (cx, cy, cz)"""
    m = np.asarray(m, np.float64).reshape(3, 4)
    r = np.asarray(r, np.float64).reshape(3, 3)
    if fault == "r_transposed":
        r = r.T
    zi, yi, xi = np.nonzero(fbin != IGNORE)
    x, y, z = xi.astype(np.float64), yi.astype(np.float64), zi.astype(np.float64)
    uu = [u[a][zi, yi, xi] for a in range(3)]
    c = [(((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3]) + ((r[k, 0] * uu[0] + r[k, 1] * uu[1]) + r[k, 2] * uu[2])
         for k in range(3)]
    return (zi, yi, xi), c


def _inside(c, shape_zyx):
    n = (shape_zyx[2], shape_zyx[1], shape_zyx[0])
    ok = np.ones(c[0].shape, bool)
    for k in range(3):
        ok &= (c[k] >= 0.0) & (c[k] <= n[k] - 1.0)
    return ok


def _trilinear(mov, c, want_gradient=False):
    """value (and its derivatives by cx, cy, cz) with section 23's taps: x1 = min(x0 + 1, n - 1), corner order"""
    nz, ny, nx = mov.shape
    n = (nx, ny, nz)
    movf = mov.astype(np.float64)
    fl = [np.floor(v) for v in c]
    fr = [v - w for v, w in zip(c, fl)]
    i0 = [w.astype(np.int64) for w in fl]
    i1 = [np.minimum(i0[k] + 1, n[k] - 1) for k in range(3)]
    val = np.zeros(c[0].shape, np.float64)
    g = [np.zeros(c[0].shape, np.float64) for _ in range(3)]
    for corner in range(8):
        px = i1[0] if corner & 1 else i0[0]
        py = i1[1] if corner & 2 else i0[1]
        pz = i1[2] if corner & 4 else i0[2]
        v = movf[pz, py, px]
        ax = fr[0] if corner & 1 else 1.0 - fr[0]
        ay = fr[1] if corner & 2 else 1.0 - fr[1]
        az = fr[2] if corner & 4 else 1.0 - fr[2]
        val = val + ((ax * ay) * az) * v
        if want_gradient:
            tx, ty, tz = (ay * az) * v, (ax * az) * v, (ax * ay) * v
            g[0] = g[0] + tx if corner & 1 else g[0] - tx
            g[1] = g[1] + ty if corner & 2 else g[1] - ty
            g[2] = g[2] + tz if corner & 4 else g[2] - tz
    return (val, g) if want_gradient else val


def ffd_joint_histogram(fbin, mov, phis, full_zyx, factors_zyx, m, r, bins, mlo, mscale, fault=None, unquantised=False):
    """int64 [T][bins][bins] of the candidate grids phis [T][3][nz][ny][nx]; ``unquantised``: float64 tables with
    the weights 1 - t and t themselves (for the finite-difference test: a differentiable function of the grid)"""
    phis = np.asarray(phis, np.float64)
    out = np.zeros((len(phis), bins, bins), np.float64 if unquantised else np.int64)
    for t, phi in enumerate(phis):
        u = displacement(phi, fbin.shape, full_zyx, factors_zyx, fault)
        (zi, yi, xi), c = _positions(fbin, u, m, r, fault)
        ok = _inside(c, mov.shape)
        c = [v[ok] for v in c]
        f = fbin[zi, yi, xi].astype(np.int64)[ok]
        val = _trilinear(mov, c)
        b = np.clip((val - mlo) * mscale, 0.0, bins - 1.0)
        i = np.minimum(np.floor(b), bins - 2.0)
        if unquantised:
            i = i.astype(np.int64)
            np.add.at(out[t], (f, i), 1.0 - (b - i))
            np.add.at(out[t], (f, i + 1), b - i)
            continue
        q = np.floor((b - i) * 65536.0 + 0.5).astype(np.int64)
        i = i.astype(np.int64)
        np.add.at(out[t], (f, i), UNIT - q)
        np.add.at(out[t], (f, i + 1), q)
    return out


def metric_float(h, metric):
    """the metric of a float64 table (no overlap rule)"""
    p = h / h.sum()
    h_fm, h_f, h_m = rr.entropy(p), rr.entropy(p.sum(axis=1)), rr.entropy(p.sum(axis=0))
    return h_f + h_m - h_fm if metric == "mi" else (h_f + h_m) / h_fm


# ---------------------------------------------------------------------------- metric derivative
def derivative_table(h, metric, fault=None):
    """(Lt [B][B], D [B][B-1], max|D|, Qd int32 [B][B-1]) of one int64 table"""
    total = float(h.sum())
    p = h.astype(np.float64) / total
    pf = h.sum(axis=1).astype(np.float64) / total
    pm = h.sum(axis=0).astype(np.float64) / total
    some = h > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.where(some, np.log(np.where(some, p, 1.0)), 0.0)
        lf = np.where(pf > 0, np.log(np.where(pf > 0, pf, 1.0)), 0.0)
        lm = np.where(pm > 0, np.log(np.where(pm > 0, pm, 1.0)), 0.0)
    if metric == "mi":
        lt = (lp - lf[:, None]) - lm[None, :]
    else:
        h_fm, h_f, h_m = rr.entropy(p), rr.entropy(pf), rr.entropy(pm)
        s = (h_f + h_m) / h_fm
        lt = (((-lf[:, None]) - lm[None, :]) + s * lp) / h_fm
    if fault == "empty_cells_kept":
        floor_p = 0.5 / total                                   # an empty cell treated as half a count's worth
        lq = np.log(np.where(some, p, floor_p))
        if metric == "mi":
            lt = (lq - np.where(pf > 0, lf, np.log(floor_p))[:, None]) - np.where(pm > 0, lm, np.log(floor_p))[None, :]
        else:
            lt = (((-np.where(pf > 0, lf, np.log(floor_p))[:, None]) - np.where(pm > 0, lm, np.log(floor_p))[None, :])
                  + s * lq) / h_fm
    else:
        lt = np.where(some, lt, 0.0)
    d = lt[:, 1:] - lt[:, :-1]
    dmax = float(np.abs(d).max())
    qd = np.zeros(d.shape, np.int32) if dmax == 0.0 else np.rint(d / dmax * float(QD_UNIT)).astype(np.int32)
    return lt, d, dmax, qd


def _gradient_samples(fbin, mov, phi, full_zyx, factors_zyx, m, r, bins, mlo, mscale, fault=None):
    """per counted sample with an unclamped bin: voxel (zi, yi, xi), fixed bin, floor(b), d [3] = sum_r g_r R[r][a]"""
    rm = np.asarray(r, np.float64).reshape(3, 3)
    u = displacement(phi, fbin.shape, full_zyx, factors_zyx, fault)
    (zi, yi, xi), c = _positions(fbin, u, m, r, fault)
    ok = _inside(c, mov.shape)
    c = [v[ok] for v in c]
    zi, yi, xi = zi[ok], yi[ok], xi[ok]
    val, g = _trilinear(mov, c, True)
    b = (val - mlo) * mscale
    live = (b > 0.0) & (b < bins - 1.0)
    zi, yi, xi, b = zi[live], yi[live], xi[live], b[live]
    g = [v[live] for v in g]
    if fault == "r_transposed":
        rm = rm.T
    d = [(g[0] * rm[0, a] + g[1] * rm[1, a]) + g[2] * rm[2, a] for a in range(3)]
    return (zi, yi, xi), fbin[zi, yi, xi].astype(np.int64), np.floor(b).astype(np.int64), d


def support_size(level_zyx, n_zyx):
    s = 1
    for l, n in zip(level_zyx, n_zyx):
        s *= min(int(l), -(-4 * int(l) // (int(n) - 3)) + 1)
    return s


def ffd_gradient(fbin, mov, phi, full_zyx, factors_zyx, m, r, bins, mlo, mscale, gscale, qd, fault=None):
    """int64 [3][nz][ny][nx]: sum over the samples of Qd * G_a * Wq at each of the 64 support points"""
    phi = np.asarray(phi, np.float64)
    nz, ny, nx = phi.shape[1:]
    assert support_size(fbin.shape, phi.shape[1:]) <= MAX_SUPPORT
    (zi, yi, xi), fb, ib, d = _gradient_samples(fbin, mov, phi, full_zyx, factors_zyx, m, r, bins, mlo, mscale, fault)
    (kz, wz, _), (ky, wy, _), (kx, wx, _) = axis_tables(fbin.shape, full_zyx, factors_zyx, phi.shape[1:], fault)
    q = np.asarray(qd, np.int64)[fb, ib]
    flat = [dd == 1 for dd in reversed(tuple(full_zyx))]
    e = []
    for a in range(3):
        s = np.minimum(np.maximum(d[a] * gscale, -1.0), 1.0)
        e.append(np.zeros(q.shape, np.int64) if flat[a] else q * np.rint(s * float(QD_UNIT)).astype(np.int64))
    out = np.zeros((3, nz, ny, nx), np.int64)
    for c in range(4):
        for b in range(4):
            wzy = wz[zi, c] * wy[yi, b]
            for a in range(4):
                wq = np.rint((wzy * wx[xi, a]) * float(W_UNIT)).astype(np.int64)
                at = ((kz[zi] + c) * ny + (ky[yi] + b)) * nx + (kx[xi] + a)
                for comp in range(3):
                    # exact integer sums: bincount of float weights would round above 2^53
                    np.add.at(out[comp].reshape(-1), at, e[comp] * wq)
    return out


def gradient_float(fbin, mov, phi, full_zyx, factors_zyx, m, r, bins, mlo, mscale, d_table, counted, fault=None):
    """dS/dphi in float64 without any quantisation: sum of D[f][i] * mscale * d_a * W / counted"""
    phi = np.asarray(phi, np.float64)
    nz, ny, nx = phi.shape[1:]
    (zi, yi, xi), fb, ib, d = _gradient_samples(fbin, mov, phi, full_zyx, factors_zyx, m, r, bins, mlo, mscale, fault)
    (kz, wz, _), (ky, wy, _), (kx, wx, _) = axis_tables(fbin.shape, full_zyx, factors_zyx, phi.shape[1:], fault)
    dd = np.asarray(d_table, np.float64)[fb, ib] * mscale / float(counted)
    flat = [v == 1 for v in reversed(tuple(full_zyx))]
    out = np.zeros((3, nz * ny * nx), np.float64)
    for c in range(4):
        for b in range(4):
            for a in range(4):
                w = (wz[zi, c] * wy[yi, b]) * wx[xi, a]
                at = ((kz[zi] + c) * ny + (ky[yi] + b)) * nx + (kx[xi] + a)
                for comp in range(3):
                    if not flat[comp]:
                        out[comp] += np.bincount(at, weights=dd * d[comp] * w, minlength=nz * ny * nx)
    return out.reshape(3, nz, ny, nx)


def descale(grad_int, dmax, mscale, gscale, counted):
    """the integer gradient as dS/dphi"""
    scale = (((dmax * mscale) / gscale) / float(1 << 42)) / float(counted)
    return grad_int.astype(np.float64) * scale


# ---------------------------------------------------------------------------- folds
def jacobian(phi, level_zyx, full_zyx, factors_zyx, inv_h_xyz, fault=None):
    """(folded, min_jacobian, map float64 [lz][ly][lx]) of det(I + du/ds)"""
    phi = np.asarray(phi, np.float64)
    (kz, wz, vz), (ky, wy, vy), (kx, wx, vx) = axis_tables(level_zyx, full_zyx, factors_zyx, phi.shape[1:], fault)
    s = np.zeros((3, 3) + tuple(level_zyx), np.float64)
    for c in range(4):
        for b in range(4):
            w_zy = wz[:, c][:, None, None] * wy[:, b][None, :, None]
            w_zdy = wz[:, c][:, None, None] * vy[:, b][None, :, None]
            w_dzy = vz[:, c][:, None, None] * wy[:, b][None, :, None]
            for a in range(4):
                w0 = w_zy * vx[:, a][None, None, :]
                w1 = w_zdy * wx[:, a][None, None, :]
                w2 = w_dzy * wx[:, a][None, None, :]
                idx = np.ix_(kz + c, ky + b, kx + a)
                for comp in range(3):
                    v = phi[comp][idx]
                    s[comp, 0] = s[comp, 0] + w0 * v
                    s[comp, 1] = s[comp, 1] + w1 * v
                    s[comp, 2] = s[comp, 2] + w2 * v
    flat = [d == 1 for d in reversed(tuple(full_zyx))]
    j = [[(1.0 if a == b else 0.0) + (0.0 if flat[a] else s[a, b] * float(inv_h_xyz[b])) for b in range(3)]
         for a in range(3)]
    det = ((j[0][0] * (j[1][1] * j[2][2] - j[1][2] * j[2][1]) - j[0][1] * (j[1][0] * j[2][2] - j[1][2] * j[2][0]))
           + j[0][2] * (j[1][0] * j[2][1] - j[1][1] * j[2][0]))
    det = np.broadcast_to(det, tuple(level_zyx))
    return int((det <= 0.0).sum()), float(det.min()), np.array(det)


# ---------------------------------------------------------------------------- warp
def warp(mov, phi, full_zyx, m, r, nearest=False, default=0.0):
    """mov resampled onto the full-resolution fixed grid through the transform, with the resampler's rules"""
    u = displacement(phi, full_zyx, full_zyx, (1, 1, 1))
    fb = np.zeros(tuple(full_zyx), np.uint8)
    _, c = _positions(fb, u, m, r)
    nz, ny, nx = mov.shape
    n = (nx, ny, nz)
    inside = np.ones(c[0].shape, bool)
    for k in range(3):
        inside &= (c[k] >= -0.5) & (c[k] < n[k] - 0.5)
    movf = mov.astype(np.float64)
    val = np.full(c[0].shape, float(default), np.float64)
    ci = [v[inside] for v in c]
    if nearest:
        idx = [np.clip(np.floor(ci[k] + 0.5).astype(np.int64), 0, n[k] - 1) for k in range(3)]
        val[inside] = movf[idx[2], idx[1], idx[0]]
    else:
        fl = [np.floor(v) for v in ci]
        bi = [w.astype(np.int64) for w in fl]
        fr = [np.where(bi[k] < 0, 0.0, ci[k] - fl[k]) for k in range(3)]
        i0 = [np.maximum(bi[k], 0) for k in range(3)]
        i1 = [np.clip(bi[k] + 1, 0, n[k] - 1) for k in range(3)]
        acc = np.zeros(ci[0].shape, np.float64)
        for corner in range(8):
            px = i1[0] if corner & 1 else i0[0]
            py = i1[1] if corner & 2 else i0[1]
            pz = i1[2] if corner & 4 else i0[2]
            w = fr[0] if corner & 1 else 1.0 - fr[0]
            w = w * (fr[1] if corner & 2 else 1.0 - fr[1])
            w = w * (fr[2] if corner & 4 else 1.0 - fr[2])
            acc = acc + w * movf[pz, py, px]
        val[inside] = acc
    val = val.reshape(tuple(full_zyx))
    if mov.dtype == np.float32:
        return val.astype(np.float32)
    info = np.iinfo(mov.dtype)
    return np.clip(val, float(info.min), float(info.max)).astype(mov.dtype)     # saturate, then truncate


def displacement_field(phi, full_zyx, direction):
    """float32 [3][z][y][x]: D_f u in mm along the physical axes"""
    u = displacement(phi, full_zyx, full_zyx, (1, 1, 1))
    d = np.asarray(direction, np.float64).reshape(3, 3)
    return np.stack([((d[k, 0] * u[0] + d[k, 1] * u[1]) + d[k, 2] * u[2]).astype(np.float32) for k in range(3)])


# ---------------------------------------------------------------------------- control grids
def control_spans(size_xyz, spacing_xyz, grid_spacing, n_levels):
    """spans per level (coarse to fine), each (x, y, z): the coarsest has max(1, floor(extent / (grid_spacing
    2^(L-1)) + 0.5)) spans, extent = (size - 1) * spacing; they double per level; an axis of extent 1 keeps one span"""
    gs = np.broadcast_to(np.asarray(grid_spacing, np.float64), (len(size_xyz),))
    first = []
    for n, sp, g in zip(size_xyz, spacing_xyz, gs):
        if n == 1:
            first.append(1)
        else:
            first.append(max(1, int(np.floor((n - 1) * float(sp) / (float(g) * 2.0 ** (n_levels - 1)) + 0.5))))
    first = first + [1] * (3 - len(first))
    flat = [n == 1 for n in size_xyz] + [True] * (3 - len(size_xyz))
    out = [tuple(s if fl else s * 2 ** lv for s, fl in zip(first, flat)) for lv in range(n_levels)]
    points = int(np.prod([s + 3 for s in out[-1]]))
    if points > MAX_POINTS:
        raise ValueError(f"grid_spacing {grid_spacing!r} gives {points} control points on the finest level, at most {MAX_POINTS}")
    return out


def _refine_axis(c, axis):
    c = np.moveaxis(c, axis, -1)
    n = c.shape[-1]
    out = np.empty(c.shape[:-1] + (2 * n - 3,), np.float64)
    out[..., 0::2] = (c[..., :-1] + c[..., 1:]) / 2.0
    out[..., 1::2] = ((c[..., :-2] + 6.0 * c[..., 1:-1]) + c[..., 2:]) / 8.0
    return np.moveaxis(out, -1, axis)


def refine_grid(phi, flat_xyz=(False, False, False)):
    """uniform cubic B-spline subdivision of phi [3][nz][ny][nx]: spans doubled along x, then y, then z (not along a
    flat axis); the refined field equals the coarse one"""
    phi = np.asarray(phi, np.float64)
    for axis, fl in zip((3, 2, 1), flat_xyz):
        if not fl:
            phi = _refine_axis(phi, axis)
    return np.ascontiguousarray(phi)


def control_spacing(size_xyz, spacing_xyz, n_xyz):
    """h (mm) per axis (x, y, z); 0 on an axis of extent 1"""
    return [0.0 if d == 1 else (d - 1) * float(sp) / float(n - 3) for d, sp, n in zip(size_xyz, spacing_xyz, n_xyz)]


def regulariser(phi, h_xyz):
    """membrane energy: sum over the grid axes b of mean(|phi[k+1] - phi[k]|^2) / h_b^2 over adjacent pairs along b"""
    total = 0.0
    for axis, h in zip((3, 2, 1), h_xyz):
        if h == 0.0:
            continue
        d = np.diff(phi, axis=axis)
        pairs = d[0].size
        total = total + float((d * d).sum()) / float(pairs) / (h * h)
    return total


def regulariser_gradient(phi, h_xyz):
    g = np.zeros(phi.shape, np.float64)
    for axis, h in zip((3, 2, 1), h_xyz):
        if h == 0.0:
            continue
        d = np.diff(phi, axis=axis)
        c = 2.0 / float(d[0].size) / (h * h)
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        g[tuple(hi)] += c * d
        g[tuple(lo)] -= c * d
    return g


def r_matrix(moving_level: rr.Grid, fixed: rr.Grid, affine):
    """3 x 3: a millimetre of u (fixed array axes) -> moving level-index units"""
    nd = fixed.nd
    a = np.asarray(affine, np.float64)[:nd, :nd]
    small = np.diag(1.0 / moving_level.spacing) @ np.linalg.inv(moving_level.direction) @ a @ fixed.direction
    r = np.zeros((3, 3))
    r[:nd, :nd] = small
    return r


# ---------------------------------------------------------------------------- the registration
@dataclass
class RefDeformable:
    control: np.ndarray
    affine: np.ndarray
    value: float
    spans: List[tuple] = field(default_factory=list)
    iterations: List[int] = field(default_factory=list)
    evaluations: List[int] = field(default_factory=list)
    final_step: List[float] = field(default_factory=list)
    level_values: List[float] = field(default_factory=list)
    accepted: List[List[float]] = field(default_factory=list)  # per level: J at the start and after every accepted move
    skipped_folds: int = 0
    converged: bool = False
    folded: int = 0
    min_jacobian: float = 1.0


def pick(values, current, folds_of, fault=None):
    """index of the candidate to take or None: descending J (the earlier one on ties), the first strictly better than
    ``current`` whose fold count is 0; also the number of candidates refused for folding"""
    order = sorted(range(len(values)), key=(lambda i: (-values[i], -i)) if fault == "ties_last" else (lambda i: (-values[i], i)))
    refused = 0
    for i in order:
        if not values[i] > current:
            break
        if folds_of(i) == 0:
            return i, refused
        refused += 1
    return None, refused


def register_deformable_ref(fixed: rr.Grid, moving: rr.Grid, initial=None, grid_spacing=16.0, levels=(4, 2, 1),
                            metric="nmi", bins=32, regularisation=0.01, fixed_mask: Optional[rr.Grid] = None,
                            min_overlap=0.25, max_iterations=60, fault=None) -> RefDeformable:
    nd = fixed.nd
    a0 = np.eye(nd + 1) if initial is None else np.array(initial, np.float64)
    fvol, mvol = fixed.volume(), moving.volume()
    full = fvol.shape
    size3 = tuple(reversed(full))
    sp3 = list(fixed.spacing) + [1.0] * (3 - nd)
    flat = [d == 1 for d in size3]
    spans = control_spans(fixed.size, fixed.spacing, grid_spacing, len(levels))
    lam = float(regularisation)
    phi = None
    res = RefDeformable(None, a0, -np.inf)
    converged = True
    for lv, sp in zip(levels, spans):
        n_xyz = tuple(s + 3 for s in sp)
        phi = np.zeros((3,) + tuple(reversed(n_xyz))) if phi is None else refine_grid(phi, flat)
        assert phi.shape[1:] == tuple(reversed(n_xyz))
        ff, mf = rr.shrink_factors(fvol.shape, lv), rr.shrink_factors(mvol.shape, lv)
        fimg = rr.bin_shrink(fvol, ff)
        mimg = mvol if lv == 1 else rr.bin_shrink(mvol, mf)
        flo, fhi = float(fimg.min()), float(fimg.max())
        mlo, mhi = float(mimg.min()), float(mimg.max())
        mmean = rr.bin_shrink(fixed_mask.volume(), ff) if fixed_mask is not None else None
        fbin = rr.fixed_bins(fimg, flo, fhi, bins, mmean)
        usable = int((fbin != IGNORE).sum())
        mscale = (bins - 1) / (mhi - mlo)
        lf = rr.level_grid(fixed, fimg[0] if nd == 2 else fimg, tuple(reversed(ff))[:nd])
        lm = rr.level_grid(moving, mimg[0] if nd == 2 else mimg, tuple(reversed(mf))[:nd])
        m = rr.index_map(lm, lf, a0)
        r = r_matrix(lm, fixed, a0)
        gscale = 1.0 / ((mhi - mlo) * float(np.abs(r).sum(axis=1).max()))
        h = control_spacing(size3, sp3, n_xyz)
        inv_h = [0.0 if v == 0.0 else 1.0 / v for v in h]

        def score(grids):
            hist = ffd_joint_histogram(fbin, mimg, grids, full, ff, m, r, bins, mlo, mscale, fault)
            vals = [rr.metric_value(t, metric, min_overlap * usable) - lam * regulariser(g, h) for t, g in zip(hist, grids)]
            return hist, vals

        hist, vals = score(phi[None])
        cur_h, cur = hist[0], float(vals[0])
        assert np.isfinite(cur), "too little overlap under the initial transform"
        step = float(lv) * float(min(fixed.spacing))
        min_step = step / 32.0
        its, evs = 0, 1
        res.accepted.append([cur])
        while step >= min_step and its < max_iterations:
            _, _, dmax, qd = derivative_table(cur_h, metric, fault)
            if dmax == 0.0:
                break
            gi = ffd_gradient(fbin, mimg, phi, full, ff, m, r, bins, mlo, mscale, gscale, qd, fault)
            g = descale(gi, dmax, mscale, gscale, int(cur_h.sum()) // UNIT) - lam * regulariser_gradient(phi, h)
            gmax = float(np.abs(g).max())
            if gmax == 0.0:
                break
            d = g / gmax
            cands = np.stack([phi + (step * c) * d for c in STEP_FACTORS])
            hist, vals = score(cands)
            evs += len(cands)
            its += 1
            take, refused = pick(vals, cur, lambda i: jacobian(cands[i], fbin.shape, full, ff, inv_h)[0], fault)
            res.skipped_folds += refused
            if take is None:
                step = step / 8.0
            else:
                phi, cur, cur_h = cands[take], float(vals[take]), hist[take]
                res.accepted[-1].append(cur)
                step = step / 2.0 if STEP_FACTORS[take] == 0.25 else step * STEP_FACTORS[take]
        res.spans.append(sp)
        res.iterations.append(its)
        res.evaluations.append(evs)
        res.final_step.append(step)
        res.level_values.append(cur)
        converged = converged and step < min_step
    n_xyz = tuple(reversed(phi.shape[1:]))
    h = control_spacing(size3, sp3, n_xyz)
    res.folded, res.min_jacobian, _ = jacobian(phi, full, full, (1, 1, 1), [0.0 if v == 0.0 else 1.0 / v for v in h])
    res.control, res.value, res.converged = phi, res.level_values[-1], converged
    return res


# ---------------------------------------------------------------------------- phantom
def smooth_field(n_xyz=(6, 6, 6), amplitude=3.0, seed=1):
    """a seeded control grid [3][nz][ny][nx] in mm"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-amplitude, amplitude, size=(3,) + tuple(reversed(n_xyz)))


def field_at(phi, size_xyz, spacing, origin, pts):
    """u (mm, x y z) of the control grid over a grid of that geometry (identity direction) at physical points
    pts [..., 3]: the same B-spline evaluated at continuous indices"""
    pts = np.asarray(pts, np.float64)
    out = np.zeros(pts.shape, np.float64)
    ks, ws = [], []
    for a in range(3):
        n = phi.shape[3 - a]
        i = (pts[..., a] - origin[a]) / spacing[a]
        t = np.clip(i, 0.0, size_xyz[a] - 1.0) * float(n - 3) / float(size_xyz[a] - 1)
        k = np.minimum(np.floor(t), n - 4.0)
        ks.append(k.astype(np.int64))
        ws.append(weights(t - k))
    for c in range(4):
        for b in range(4):
            for a in range(4):
                w = ws[2][..., c] * ws[1][..., b] * ws[0][..., a]
                for comp in range(3):
                    out[..., comp] += w * phi[comp][ks[2] + c, ks[1] + b, ks[0] + a]
    return out


def make_deformed_pair(truth_phi, fixed_size=(48, 44, 40), fixed_spacing=(1.0, 1.0, 1.1), moving_size=(52, 50, 44),
                       moving_spacing=(1.1, 0.9, 1.0), noise=0.01, seed=0):
    """(fixed, moving) Grids, float32, both centred on the physical origin.  moving(q) = remap(phantom(q)) and
    fixed(p) = phantom(p + u_truth(p)): the transform that aligns them is T(p) = p + u_truth(p), fixed -> moving."""
    rng = np.random.default_rng(seed)
    fo, mo = rr.centred_origin(fixed_size, fixed_spacing), rr.centred_origin(moving_size, moving_spacing)
    pf = rr._points(fixed_size, fixed_spacing, fo)
    u = field_at(truth_phi, fixed_size, fixed_spacing, fo, pf)
    f = rr.phantom(pf + u)
    m = rr.remap(rr.phantom(rr._points(moving_size, moving_spacing, mo)))
    f = f + noise * rng.standard_normal(f.shape)
    m = m + noise * rng.standard_normal(m.shape)
    return (rr.Grid(f.astype(np.float32), fixed_spacing, fo), rr.Grid(m.astype(np.float32), moving_spacing, mo)), u


def residual(truth_u, phi, fixed: rr.Grid):
    """(mean initial, mean residual) displacement error in mm over the foreground (fixed above 20 % of its maximum)"""
    full = fixed.volume().shape
    u = displacement(phi, full, full, (1, 1, 1))
    got = np.stack([u[0], u[1], u[2]], axis=-1)
    fg = fixed.volume() > 0.2 * float(fixed.volume().max())
    before = np.sqrt((truth_u ** 2).sum(-1))[fg].mean()
    after = np.sqrt(((truth_u - got) ** 2).sum(-1))[fg].mean()
    return float(before), float(after)
