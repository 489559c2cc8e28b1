"""Float64 numpy restatement of the cubic B-spline and label-Gaussian interpolators of the resampler (DESIGN.md
section 19; kernels in segmantic_amd/csrc/resample_hq.hip), and the cases tests/test_resample_hq_host.py and
tests/test_resample_hq_gpu.py share.

* ``prefilter`` / ``bspline_eval`` restate the recursive prefilter and the 64-tap evaluate line by line;
  the host file holds them to ``scipy.ndimage.spline_filter`` / ``map_coordinates(order=3, mode="mirror")``.
* ``label_gaussian`` is the vote as DESIGN words it: erf edges, weights quantised to 2^-18, int64 scores, the largest
  score wins, the smallest label value among equal scores.
* ``hazard`` is the smallest distance of any in-range per-axis weight of an inside voxel, times 2^18, from a rounding
  boundary: a case whose hazard is far above the few 1e-10 by which two erf implementations differ has one possible
  quantisation, so the GPU result must equal the helper's bit for bit.

Arrays are [z, y, x]; index maps are 3x4, output index (x, y, z, 1) -> continuous input index (x, y, z).
Importable without a GPU.
"""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy.special import erf

POLE = math.sqrt(3.0) - 2.0
GAIN = 6.0
SCALE = float(2 ** 18)
MAX_RADIUS = 8
GRID_LANES = 2048 * 256      # SEGMI_RESAMPLE_HQ_GRID_CAP workgroups of 256 threads (include/segmi.h)
PIXELS = ("float32", "uint8", "int16", "int32", "uint16")


# ---------------------------------------------------------------------------------------------- geometry
def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def oblique_map():
    """rotation 0.2, -0.3, 0.4 rad, scales 0.7, 0.9, 0.6, offset 1.3, -0.8, 0.9"""
    m = np.zeros((3, 4))
    m[:, :3] = rotation(0.2, -0.3, 0.4) @ np.diag([0.7, 0.9, 0.6])
    m[:, 3] = [1.3, -0.8, 0.9]
    return m


def scale_map(sx, sy=None, sz=None, offset=(0.0, 0.0, 0.0)):
    m = np.zeros((3, 4))
    m[:, :3] = np.diag([sx, sx if sy is None else sy, sx if sz is None else sz])
    m[:, 3] = offset
    return m


OBLIQUE = oblique_map()
OBLIQUE_OUT = (12, 14, 17)
UPSAMPLE = scale_map(0.5)            # c = 0.5 * o
SRC_SHAPE = (11, 9, 7)
UPSAMPLE_OUT = (24, 20, 16)          # the last planes fall outside: c = 11, 9, 7 and beyond


def coords(m, out_zyx, in_zyx, border=False):
    """-> c [dz, dy, dx, 3] (x, y, z) and the inside mask; the kernel's arithmetic, product by product"""
    m = np.asarray(m, np.float64).reshape(3, 4)
    oz, oy, ox = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in out_zyx], indexing="ij")
    c = np.stack([((m[r, 0] * ox + m[r, 1] * oy) + m[r, 2] * oz) + m[r, 3] for r in range(3)], -1)
    size = np.array(in_zyx[::-1], np.float64)
    if border:
        c = np.minimum(np.maximum(c, 0.0), size - 1.0)
    inside = np.all((c >= -0.5) & (c < size - 0.5), -1)
    return c, inside


def saturate_cast(val, dtype):
    """clamp to the type's range, then truncate toward zero"""
    dtype = np.dtype(dtype)
    if not np.issubdtype(dtype, np.integer):
        return val.astype(dtype)
    info = np.iinfo(dtype)
    return np.trunc(np.clip(val, info.min, info.max)).astype(dtype)


# ---------------------------------------------------------------------------------------------- B-spline
def prefilter_lines(s):
    """s [n, ...]: the recursion along axis 0 of every line at once.  Gain first, the causal start from the exact
    mirror sum over the whole line, the anticausal start in closed form; a line of length 1 is copied."""
    s = np.asarray(s, np.float64)
    n = s.shape[0]
    if n == 1:
        return s.copy()
    z = POLE
    c = s * GAIN
    zn1 = z ** (n - 1)
    acc = c[0] + zn1 * c[n - 1]
    zk = z
    for k in range(1, n - 1):
        acc = acc + zk * (c[k] + zn1 * c[n - 1 - k])
        zk *= z
    c[0] = acc / (1.0 - zn1 * zn1)
    for k in range(1, n):
        c[k] = c[k] + z * c[k - 1]
    c[n - 1] = z / (z * z - 1.0) * (z * c[n - 2] + c[n - 1])
    for k in range(n - 2, -1, -1):
        c[k] = z * (c[k + 1] - c[k])
    return c


def prefilter(arr):
    """[z, y, x] pixels -> float64 coefficients: along x, then y, then z"""
    c = np.asarray(arr, np.float64)
    for axis in (2, 1, 0):
        c = np.moveaxis(prefilter_lines(np.moveaxis(c, axis, 0)), 0, axis)
    return np.ascontiguousarray(c)


def _mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i > n - 1, period - i, i)


def _taps(c, n):
    f = np.floor(c)
    t = c - f
    u = 1.0 - t
    t2 = t * t
    t3 = t2 * t
    w = [u * u * u / 6.0, (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0, (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0, t3 / 6.0]
    b = f.astype(np.int64) - 1
    return w, [_mirror(b + j, n) for j in range(4)]


def bspline_eval(coef, m, out_zyx, border=False, default=0.0):
    """-> the real-valued (float64) result; 64 taps, x innermost and z outermost"""
    sz, sy, sx = coef.shape
    c, inside = coords(m, out_zyx, coef.shape, border)
    cc = np.where(inside[..., None], c, 0.0)
    wx, ix = _taps(cc[..., 0], sx)
    wy, iy = _taps(cc[..., 1], sy)
    wz, iz = _taps(cc[..., 2], sz)
    val = np.zeros(inside.shape)
    for a in range(4):
        plane = np.zeros(inside.shape)
        for b in range(4):
            row = np.zeros(inside.shape)
            for k in range(4):
                row = row + wx[k] * coef[iz[a], iy[b], ix[k]]
            plane = plane + wy[b] * row
        val = val + wz[a] * plane
    return np.where(inside, val, float(default)), inside


def bspline_resample(arr, m, out_zyx, border=False, default=0.0, coef=None):
    """-> (result in arr's type, real-valued result, inside mask)"""
    real, inside = bspline_eval(prefilter(arr) if coef is None else coef, m, out_zyx, border, default)
    return saturate_cast(real, arr.dtype), real, inside


def bspline_violations(got, real, vmax, cap=0.02):
    """f32: within 1e-11 max|x| + 2^-24 |ref| of the float64 reference.  Integer: exact, except where the reference's
    real value lies within 1e-11 max|x| of an integer, and that on at most ``cap`` of the voxels."""
    tol = 1e-11 * vmax
    bad = []
    if got.shape != real.shape:
        return [f"shape {got.shape} != {real.shape}"]
    if got.dtype == np.float32:
        d = np.abs(got.astype(np.float64) - real)
        over = d > tol + 2.0 ** -24 * np.abs(real)
        if over.any():
            bad.append(f"f32: {int(over.sum())} voxels beyond the bound, max |diff| {d.max():.3e}")
        return bad
    diff = got.astype(np.int64) != saturate_cast(real, got.dtype).astype(np.int64)
    if diff.any():
        if not np.all(np.abs(real[diff] - np.round(real[diff])) <= tol):
            bad.append(f"integer: {int(diff.sum())} voxels differ, not all at a near-integer real value")
        if not diff.mean() <= cap:
            bad.append(f"integer: excused share {diff.mean():.4f} > {cap}")
    return bad


# ---------------------------------------------------------------------------------------------- label-Gaussian
def radii(sigma, alpha):
    sg = np.broadcast_to(np.asarray(sigma, np.float64), (3,))
    return [int(math.ceil(alpha * s)) for s in sg]


def _axis_weights(c, n, r, inv):
    """c [...]: -> taps i [..., 2r+1], their quantised weights q (int64) and real weights w; out-of-range taps q = -1"""
    i0 = np.floor(c + 0.5).astype(np.int64)
    i = i0[..., None] + np.arange(-r, r + 1)
    fi = i.astype(np.float64)
    w = 0.5 * (erf(((fi + 0.5) - c[..., None]) * inv) - erf(((fi - 0.5) - c[..., None]) * inv))
    q = np.floor(w * SCALE + 0.5).astype(np.int64)
    ok = (i >= 0) & (i <= n - 1)
    return i, np.where(ok, q, -1), w, ok


def label_gaussian(arr, m, out_zyx, sigma=1.0, alpha=2.0, border=False, default=0.0):
    """-> (result in arr's type, hazard, tied).  Scores are int64 sums of qz * qy * qx over the in-range window voxels
    that carry a label; the largest score wins, the smallest label value among equal scores.  ``tied`` marks the
    inside voxels where more than one label reaches the largest score."""
    sz, sy, sx = arr.shape
    sg = np.broadcast_to(np.asarray(sigma, np.float64), (3,))
    rad = radii(sigma, alpha)
    assert all(s > 0 for s in sg) and max(rad) <= MAX_RADIUS
    c, inside = coords(m, out_zyx, arr.shape, border)
    cc = np.where(inside[..., None], c, 0.0)
    axes = [_axis_weights(cc[..., a], n, rad[a], 1.0 / (sg[a] * math.sqrt(2.0))) for a, n in enumerate((sx, sy, sz))]
    hazard = np.inf
    for i, q, w, ok in axes:
        sel = ok & inside[..., None]
        if sel.any():
            frac = w[sel] * SCALE - np.floor(w[sel] * SCALE)
            hazard = min(hazard, float(np.abs(frac - 0.5).min()))
    labels = np.unique(arr)
    best = np.full(inside.shape, labels[0], arr.dtype)
    best_score = np.full(inside.shape, -1, np.int64)
    (ix, qx, _, _), (iy, qy, _, _), (iz, qz, _, _) = axes
    nvox = inside.size
    present = np.zeros(len(labels) * nvox, bool)
    scores = np.zeros(len(labels) * nvox, np.int64)
    code = np.searchsorted(labels, arr)
    voxel = np.arange(nvox)
    for a in range(iz.shape[-1]):
        for b in range(iy.shape[-1]):
            for k in range(ix.shape[-1]):
                ok = ((qz[..., a] >= 0) & (qy[..., b] >= 0) & (qx[..., k] >= 0)).reshape(-1)
                wgt = (qz[..., a] * qy[..., b] * qx[..., k]).reshape(-1)[ok]
                v = code[np.clip(iz[..., a], 0, sz - 1), np.clip(iy[..., b], 0, sy - 1), np.clip(ix[..., k], 0, sx - 1)]
                slot = v.reshape(-1)[ok] * nvox + voxel[ok]          # one slot per voxel: no index repeats
                present[slot] = True
                scores[slot] += wgt
    present = present.reshape((len(labels),) + inside.shape)
    scores = scores.reshape((len(labels),) + inside.shape)
    for li in range(len(labels)):                 # ascending label value: a later label needs a strictly larger score
        better = present[li] & (scores[li] > best_score)
        best = np.where(better, labels[li], best)
        best_score = np.where(better, scores[li], best_score)
    tied = inside & ((present & (scores == best_score[None])).sum(0) > 1)
    out = np.where(inside, best, saturate_cast(np.full(inside.shape, float(default)), arr.dtype))
    return out.astype(arr.dtype), hazard, tied


# ---------------------------------------------------------------------------------------------- shared inputs
def image_volume(pixel, shape=SRC_SHAPE, seed=3):
    """seeded integer values with |x| <= 1000 (within the type's range), as ``pixel``"""
    rng = np.random.default_rng(seed)
    info = None if pixel == "float32" else np.iinfo(pixel)
    lo, hi = (-1000, 1000) if info is None else (max(info.min, -1000), min(info.max, 1000))
    return rng.integers(lo, hi + 1, shape).astype(pixel)


def label_volume(pixel="uint8", shape=SRC_SHAPE, labels=5, seed=5):
    """random labels 0 .. labels-1, voxel by voxel: every window is mixed"""
    return np.random.default_rng(seed).integers(0, labels, shape).astype(pixel)


def slab_phantom(lo_label, hi_label, pixel="uint8", shape=(6, 5, 6)):
    """Two slabs that meet on the plane between x = 3 and x = 4, the second two voxels thick.  Under c = 0.5 o the
    output plane o = 7 lies midway, c = 3.5.  The window of 2 R + 1 = 5 taps around i0 = 4 is x = 2 .. 6; x = 6 is
    outside the buffer and dropped, which leaves two voxels of either slab at mirrored distances: equal scores."""
    a = np.full(shape, lo_label, pixel)
    a[:, :, 4:] = hi_label
    return a


SLAB_OUT = (12, 10, 12)
SLAB_TIE_PLANE = 7


# (name, volume maker, map, output size, sigma, alpha, border): the label-Gaussian cases; the host file checks the
# hazard of each, the GPU file demands bit equality on each
def label_cases():
    cases = [
        ("upsample_5", lambda: label_volume(), UPSAMPLE, UPSAMPLE_OUT, 1.0, 2.0, False),
        ("oblique_5", lambda: label_volume(), OBLIQUE, OBLIQUE_OUT, 1.0, 2.0, False),
        ("oblique_5_narrow", lambda: label_volume(), OBLIQUE, OBLIQUE_OUT, 0.6, 1.0, False),
        ("oblique_40", lambda: label_volume(labels=40), OBLIQUE, OBLIQUE_OUT, 1.5, 2.0, False),
        ("oblique_5_border", lambda: label_volume(), OBLIQUE, OBLIQUE_OUT, 1.0, 2.0, True),
        ("oblique_aniso", lambda: label_volume(), OBLIQUE, OBLIQUE_OUT, (0.8, 1.7, 0.5), 1.5, False),
        ("plane_1_9_4", lambda: label_volume(shape=(1, 9, 4)), scale_map(0.5, 0.4, 1.0, (0.1, -0.2, 0.0)), (1, 24, 9),
         1.0, 2.0, False),
        ("line_7_1_1", lambda: label_volume(shape=(7, 1, 1)), scale_map(1.0, 1.0, 0.45, (0.0, 0.0, -0.3)), (17, 1, 1),
         1.0, 2.0, False),
        ("point_1_1_1", lambda: label_volume(shape=(1, 1, 1)) + 3, scale_map(0.3), (1, 2, 3), 1.0, 2.0, False),
    ]
    for px in PIXELS:
        if px == "float32":
            mk = lambda: (label_volume("int16") * 0.5 - 1.0).astype(np.float32)      # noqa: E731
        elif np.iinfo(px).min < 0:
            mk = lambda px=px: (label_volume("int16") * 7 - 14).astype(px)           # noqa: E731
        else:
            mk = lambda px=px: (label_volume("int16") * 50).astype(px)               # noqa: E731
        cases.append((f"oblique_{px}", mk, OBLIQUE, OBLIQUE_OUT, 1.0, 2.0, False))
    return cases


# one case past one pass of the capped grid: 66 x 90 x 90 = 534 600 output voxels > GRID_LANES
CAP_SRC = (33, 45, 45)
CAP_OUT = (66, 90, 90)
CAP_MAP = scale_map(0.5, offset=(0.25, 0.25, 0.25))
CAP_SIGMA = 0.5                      # radius 1: 27 taps keep the reference of half a million voxels quick


@functools.lru_cache(maxsize=None)
def cap_label_reference():
    """(volume, expected result, hazard) of the label-Gaussian case past the grid cap, computed once per session"""
    arr = cap_label_volume()
    arr.setflags(write=False)
    out, hz, _ = label_gaussian(arr, CAP_MAP, CAP_OUT, CAP_SIGMA)
    out.setflags(write=False)
    return arr, out, hz


def cap_label_volume():
    """5 labels in blocks of 3 voxels: windows of one label and mixed windows"""
    b = np.random.default_rng(11).integers(0, 5, (11, 15, 15)).astype(np.uint8)
    return np.ascontiguousarray(b.repeat(3, 0).repeat(3, 1).repeat(3, 2))
