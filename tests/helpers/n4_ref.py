"""Literal float64 numpy restatement of the N4 / CT-scaling contract of segmantic_amd.image.modality
(DESIGN §12).  Arrays are [z, y, x] (2-D: [y, x]); every rule below is the project's definition, written
out one step at a time so that a GPU result can be checked against it.  Nothing here calls the GPU."""
from __future__ import annotations

import math

import numpy as np


# ------------------------------------------------------------------ Otsu
def otsu_counts(x, bins=200):
    """(counts int64 [bins], lo, width) over the finite voxels: bin = min(floor((v - lo) / w), bins - 1)"""
    v = np.asarray(x, np.float64).ravel()
    v = v[np.isfinite(v)]
    if v.size == 0:
        raise ValueError("no finite voxel")
    lo, hi = float(v.min()), float(v.max())
    w = (hi - lo) / bins
    if w > 0:
        b = np.minimum(np.floor((v - lo) / w), bins - 1).astype(np.int64)
    else:
        b = np.zeros(v.size, np.int64)
    return np.bincount(b, minlength=bins).astype(np.int64), lo, w


def otsu_pick(counts, lo, w):
    """threshold = lo + (k + 1) * w for the first k that maximises w0 * w1 * (mu0 - mu1)^2 with bin-centre
    class values; the sums run in bin order (the kernel's order, so the threshold is bit-equal)"""
    bins = len(counts)
    best, k_best = -1.0, 0
    n_tot = float(np.sum(counts))
    w0 = 0.0
    s0 = 0.0
    s_all = 0.0
    for i in range(bins):
        s_all += float(counts[i]) * (lo + (i + 0.5) * w)
    for k in range(bins):
        c = float(counts[k])
        w0 += c
        s0 += c * (lo + (k + 0.5) * w)
        w1 = n_tot - w0
        if w0 > 0 and w1 > 0:
            d = s0 / w0 - (s_all - s0) / w1
            var = w0 * w1 * (d * d)
        else:
            var = 0.0
        if var > best:
            best, k_best = var, k
    return lo + (k_best + 1) * w


def otsu_threshold(x, inside=0, outside=1, bins=200):
    counts, lo, w = otsu_counts(x, bins)
    thr = otsu_pick(counts, lo, w)
    v = np.asarray(x, np.float64)
    return np.where(v > thr, outside, inside).astype(np.uint8), thr, counts


# ------------------------------------------------------------------ shrink
def shrink_offsets(n, f):
    """(ns, o): output size and the input index of output voxel 0 along one axis"""
    ns = max(1, n // f)
    o = math.floor(((n - 1) - (ns - 1) * f) / 2 + 0.5)
    return ns, o


def shrink(x, f):
    """f: one factor for every axis, or per array axis ([z, y, x] order)"""
    x = np.asarray(x)
    fs = [f] * x.ndim if np.isscalar(f) else list(f)
    sl = []
    for n, fa in zip(x.shape, fs):
        ns, o = shrink_offsets(n, fa)
        sl.append(o + fa * np.arange(ns))
    return x[np.ix_(*sl)]


def shrink_geometry(size_xyz, spacing, origin, direction, f):
    """ITK's rule as we read it: the physical centres of input and output coincide"""
    d = len(size_xyz)
    fs = [f] * d if np.isscalar(f) else list(f)
    ns = [max(1, n // fa) for n, fa in zip(size_xyz, fs)]
    sp = np.array([s * fa for s, fa in zip(spacing, fs)], np.float64)
    shift = np.array([((n - 1) - (m - 1) * fa) / 2.0 for n, m, fa in zip(size_xyz, ns, fs)]) * np.asarray(spacing)
    org = np.asarray(origin, np.float64) + np.asarray(direction, np.float64).reshape(d, d) @ shift
    return ns, tuple(sp), tuple(org)


# ------------------------------------------------------------------ B-splines
def cubic_weights(t):
    t = np.asarray(t, np.float64)
    return np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6,
                     t ** 3 / 6], axis=-1)


def axis_basis(n, lat):
    """per-axis evaluation matrix B [n, lat]: index i of an axis of n voxels against `lat` control points
    (lat == 1: an axis without spline dimension, weight 1)"""
    B = np.zeros((n, lat))
    if lat == 1:
        B[:, 0] = 1.0
        return B
    m = lat - 3
    for i in range(n):
        u = i / (n - 1) * m if n > 1 else 0.0
        span = min(math.floor(u), m - 1)
        B[i, span:span + 4] = cubic_weights(u - span)
    return B


def lattice_shape(shape, spans):
    return tuple(1 if n == 1 else spans + 3 for n in shape)


def evaluate(lattice, shape):
    """the field of `lattice` on a grid of `shape` (u = i / (N - 1) * m per axis)"""
    out = np.asarray(lattice, np.float64)
    for ax, n in enumerate(shape):
        B = axis_basis(n, out.shape[ax])
        out = np.moveaxis(np.tensordot(B, out, axes=([1], [ax])), 0, ax)
    return out


def _axis_weights_f64(n, lat):
    """(span [n], weights [n, 4]) as csrc/n4.hip's axis_weights: products written out, {1, 0, 0, 0} when
    the axis has no spline dimension"""
    if lat == 1:
        w = np.zeros((n, 4))
        w[:, 0] = 1.0
        return np.zeros(n, np.int64), w
    m = lat - 3
    i = np.arange(n, dtype=np.float64)
    u = i / float(n - 1) * float(m) if n > 1 else np.zeros(n)
    s = np.minimum(np.floor(u), m - 1).astype(np.int64)
    t = u - s
    t2 = t * t
    t3 = t2 * t
    w = np.stack([(1.0 - t) * (1.0 - t) * (1.0 - t) / 6.0, (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0,
                  (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0, t3 / 6.0], axis=-1)
    return s, w


def evaluate_f32(lattice, shape):
    """n4_full_kernel's arithmetic: the z / y weights fold the [Lz, Ly, Lx] lattice into one row of Lx
    coefficients per (z, y) in f64, rounded to f32; then u = f32(x) f32(m / (nx - 1)), the cubic weights
    and the four-tap sum, left to right, all in f32.  `shape` is (nz, ny, nx); returns f32 [nz, ny, nx]."""
    lat = np.asarray(lattice, np.float64)
    nz, ny, nx = shape
    Lz, Ly, Lx = lat.shape
    sz, wz = _axis_weights_f64(nz, Lz)
    sy, wy = _axis_weights_f64(ny, Ly)
    acc = np.zeros((nz, ny, Lx))
    for a in range(4):
        iz = np.minimum(sz + a, Lz - 1)
        for b in range(4):
            iy = np.minimum(sy + b, Ly - 1)
            acc = acc + (wz[:, a][:, None] * wy[:, b][None, :])[:, :, None] * lat[iz[:, None], iy[None, :], :]
    q = acc.astype(np.float32)
    if Lx == 1:
        return np.broadcast_to(q, (nz, ny, nx)).copy()
    f = np.float32
    m = Lx - 3
    scale = f(float(m) / float(nx - 1)) if nx > 1 else f(0.0)
    u = np.arange(nx).astype(np.float32) * scale
    s = np.minimum(np.floor(u).astype(np.int64), m - 1)
    t = u - s.astype(np.float32)
    t2 = t * t
    t3 = t2 * t
    one = f(1.0)
    w0 = (one - t) * (one - t) * (one - t) / f(6.0)
    w1 = (f(3.0) * t3 - f(6.0) * t2 + f(4.0)) / f(6.0)
    w2 = (f(-3.0) * t3 + f(3.0) * t2 + f(3.0) * t + one) / f(6.0)
    w3 = t3 / f(6.0)
    out = w0 * q[:, :, s] + w1 * q[:, :, s + 1] + w2 * q[:, :, s + 2] + w3 * q[:, :, s + 3]
    assert out.dtype == np.float32
    return out


def refine_axis(P, ax):
    P = np.moveaxis(np.asarray(P, np.float64), ax, 0)
    L = P.shape[0]
    if L == 1:
        return np.moveaxis(P, 0, ax)
    m = L - 3
    out = np.empty((2 * m + 3,) + P.shape[1:])
    for j in range(2 * m + 3):
        if j % 2 == 0:
            out[j] = (P[j // 2] + P[j // 2 + 1]) / 2
        else:
            i = (j + 1) // 2
            out[j] = (P[i - 1] + 6 * P[i] + P[i + 1]) / 8
    return np.moveaxis(out, 0, ax)


def refine(P):
    for ax in range(np.ndim(P)):
        P = refine_axis(P, ax)
    return P


def _apply_axes(x, mats):
    for ax, M in enumerate(mats):
        x = np.moveaxis(np.tensordot(M, x, axes=([1], [ax])), 0, ax)
    return x


def ba_fit(r, valid, spans):
    """one BA level, the sums of ba_fit_points regrouped per axis: num = sum_p r_p w_p^3 / sum w_p^2 and
    den = sum_p w_p^2 are separable tensor contractions (w_k = wz wy wx, sum w^2 = Sz Sy Sx)"""
    shape = r.shape
    lshape = lattice_shape(shape, spans)
    Bs = [axis_basis(n, lat) for n, lat in zip(shape, lshape)]
    sw2 = np.ones(shape)
    for ax, B in enumerate(Bs):
        sw2 = sw2 * np.sum(B * B, axis=1).reshape([-1 if a == ax else 1 for a in range(len(shape))])
    alpha = np.where(valid, r, 0.0) / sw2
    num = _apply_axes(alpha, [(B ** 3).T for B in Bs])
    den = _apply_axes(valid.astype(np.float64), [(B ** 2).T for B in Bs])
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def ba_fit_points(r, valid, spans):
    """one Lee-Wolberg-Shin BA level, point by point: phi_k = r w_k / sum w^2, num[k] += w_k^2 phi_k,
    den[k] += w_k^2, lattice = num / den (0 where den is 0)"""
    shape = r.shape
    lshape = lattice_shape(shape, spans)
    Bs = [axis_basis(n, lat) for n, lat in zip(shape, lshape)]
    num = np.zeros(lshape)
    den = np.zeros(lshape)
    for idx in zip(*np.nonzero(valid)):
        ws = [Bs[a][idx[a]] for a in range(len(shape))]
        w = ws[0]
        for wa in ws[1:]:
            w = np.multiply.outer(w, wa)
        sw2 = np.sum(w * w)
        phi = r[idx] * w / sw2
        num += w * w * phi
        den += w * w
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


# ------------------------------------------------------------------ sharpening
def padded_size(bins):
    return 2 ** (int(math.ceil(math.log2(bins))) + 1) if bins & (bins - 1) else 2 * bins


def sharpen(u, bins=200, fwhm=0.15, noise=0.01):
    """ITK's SharpenImage on the values u (1-D, the fit set): returns (E [bins], sharpened values)"""
    u = np.asarray(u, np.float64)
    lo, hi = float(u.min()), float(u.max())
    slope = (hi - lo) / (bins - 1)
    c = (u - lo) / slope
    i = np.floor(c).astype(np.int64)
    fr = c - i
    H = np.zeros(bins)
    np.add.at(H, np.minimum(i, bins - 1), 1 - fr)
    ok = i + 1 < bins
    np.add.at(H, i[ok] + 1, fr[ok])
    P = padded_size(bins)
    off = (P - bins) // 2
    V = np.zeros(P)
    V[off:off + bins] = H
    fw = fwhm / slope
    e = 4 * math.log(2) / fw ** 2
    s = 2 * math.sqrt(math.log(2) / math.pi) / fw
    F = np.zeros(P)
    F[0] = s
    for n in range(1, P // 2 + 1):
        F[n] = F[P - n] = s * math.exp(-e * n * n)
    Fh = np.fft.fft(F)
    G = np.conj(Fh) / (Fh * np.conj(Fh) + noise)
    Ut = np.maximum(np.real(np.fft.ifft(np.fft.fft(V) * G)), 0)
    x = lo + (np.arange(P) - off) * slope
    num = np.real(np.fft.ifft(np.fft.fft(x * Ut) * Fh))
    den = np.real(np.fft.ifft(np.fft.fft(Ut) * Fh))
    E = np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)[off:off + bins]
    ic = np.minimum(i, bins - 1)
    last = ic >= bins - 1
    nxt = np.minimum(ic + 1, bins - 1)
    S = np.where(last, E[bins - 1], E[ic] + (E[nxt] - E[ic]) * fr)
    return E, S


HIST_FIX = 4294967296.0  # 2^32: the kernel's histogram weights are whole multiples of 2^-32


def sharpen_direct(u, bins=200, fwhm=0.15, noise=0.01):
    """`sharpen` with the arithmetic of csrc/n4.hip (its two declared departures from the FFT form): the
    splat weights are rint(w 2^32) / 2^32, summed exactly as integers, and F^, g = IDFT(G), U~ and the two
    F-convolutions are direct f64 sums over the P points, each sum running in the kernel's index order
    (one term after the other, no pairwise grouping).  Returns (E [bins], sharpened values)."""
    u = np.asarray(u, np.float64)
    lo, hi = float(u.min()), float(u.max())
    slope = (hi - lo) / (bins - 1)
    c = np.maximum((u - lo) / slope, 0.0)
    fi = np.floor(c)
    i = np.where(fi < bins - 1, fi, bins - 1).astype(np.int64)
    f1 = np.minimum(c - i, 1.0)
    H = np.zeros(bins, np.int64)
    np.add.at(H, i, np.rint((1.0 - f1) * HIST_FIX).astype(np.int64))
    ok = i + 1 < bins
    np.add.at(H, i[ok] + 1, np.rint(f1[ok] * HIST_FIX).astype(np.int64))
    P = padded_size(bins)
    off = (P - bins) // 2
    mask = P - 1
    idx = np.arange(P)
    V = np.zeros(P)
    V[off:off + bins] = H.astype(np.float64) / HIST_FIX
    fw = fwhm / slope
    e = 4.0 * math.log(2.0) / (fw * fw)
    s = 2.0 * math.sqrt(math.log(2.0) / math.pi) / fw
    cs = np.cos(2.0 * np.pi * idx / P)
    cs[[0, P // 2]] = 1.0, -1.0
    cs[[P // 4, 3 * P // 4]] = 0.0  # cospi is exact at the quarter points
    nn = np.where(idx <= P // 2, idx, P - idx).astype(np.float64)
    F = s * np.exp(-e * nn * nn)
    fh = np.zeros(P)
    for n in range(P):
        fh = fh + F[n] * cs[(n * idx) & mask]
    G = fh / (fh * fh + noise)
    a = np.zeros(P)
    for k in range(P):
        a = a + G[k] * cs[(idx * k) & mask]
    g = a / P
    a = np.zeros(P)
    for m in range(off, off + bins):
        a = a + V[m] * g[(idx - m) & mask]
    Ut = np.where(a > 0.0, a, 0.0)
    xU = (lo + (idx - off).astype(np.float64) * slope) * Ut
    nb = off + np.arange(bins)
    num = np.zeros(bins)
    den = np.zeros(bins)
    for m in range(P):
        f = F[(nb - m) & mask]
        num = num + xU[m] * f
        den = den + Ut[m] * f
    E = np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)
    last = fi >= bins - 1
    ic = np.where(last, bins - 2, fi).astype(np.int64)
    S = np.where(last, E[bins - 1], E[ic] + (E[ic + 1] - E[ic]) * (c - fi))
    return E, S


# ------------------------------------------------------------------ N4
def fit_set(img, mask):
    v = np.asarray(img, np.float64)
    with np.errstate(invalid="ignore"):
        return (np.asarray(mask) == 1) & np.isfinite(v) & (v > 0)


def n4(img, mask, iterations=(50, 50, 50, 50), control_points=4, bins=200, fwhm=0.15, noise=0.01,
       threshold=0.001, sharpen_fn=None, trace=False):
    """the whole N4 fit on the (already shrunk) image: (lattice, field on the grid, elapsed per level, CV);
    `sharpen_fn` is `sharpen` (the default) or `sharpen_direct`; with `trace`, a fifth value: per level, the
    CV after every iteration"""
    sharpen_fn = sharpen_fn or sharpen
    img = np.asarray(img, np.float64)
    valid = fit_set(img, mask)
    if valid.sum() < 2:
        raise ValueError("fewer than 2 voxels in the fit set")
    L = np.log(np.where(valid, img, 1.0))
    if L[valid].min() == L[valid].max():
        raise ValueError("constant fit set")
    spans = control_points - 3
    lattice = np.zeros(lattice_shape(img.shape, spans))
    field = np.zeros(img.shape)
    elapsed, cvs = [], []
    cv = math.inf
    for lev, max_it in enumerate(iterations):
        if lev > 0:
            lattice = refine(lattice)
            spans *= 2
        it, cv = 0, math.inf
        cvs.append([])
        while it < max_it and cv > threshold:
            U = L - field
            _, S = sharpen_fn(U[valid], bins, fwhm, noise)
            r = np.zeros(img.shape)
            r[valid] = U[valid] - S
            lattice = lattice + ba_fit(r, valid, spans)
            new = evaluate(lattice, img.shape)
            e = np.exp(field[valid] - new[valid])
            cv = float(np.std(e, ddof=1) / np.mean(e))
            cvs[-1].append(cv)
            field = new
            it += 1
        elapsed.append(it)
    if trace:
        return lattice, field, elapsed, cv, cvs
    return lattice, field, elapsed, cv


def median_filter(x):
    """radius-1 median with replicate borders ([z, y, x] or [y, x])"""
    x = np.asarray(x, np.float64)
    p = np.pad(x, 1, mode="edge")
    stack = []
    for off in np.ndindex(*(3,) * x.ndim):
        stack.append(p[tuple(slice(o, o + n) for o, n in zip(off, x.shape))])
    return np.median(np.stack(stack), axis=0)


def median_filter_slab(x, z0, z1):
    """planes [z0, z1) of median_filter(x) for a [z, y, x] volume, from those planes and their real
    neighbours only (replicate borders at the volume's own ends): a large volume checked slab by slab"""
    x = np.asarray(x)
    nz = x.shape[0]
    a, b = max(z0 - 1, 0), min(z1 + 1, nz)
    p = np.pad(np.asarray(x[a:b], np.float64), ((int(z0 == 0), int(z1 == nz)), (1, 1), (1, 1)), mode="edge")
    stack = []
    for off in np.ndindex(3, 3, 3):
        stack.append(p[off[0]:off[0] + z1 - z0, off[1]:off[1] + x.shape[1], off[2]:off[2] + x.shape[2]])
    return np.median(np.stack(stack), axis=0)


def scale_clamp_ct(x):
    """f64 value of median -> clamp [-1100, 3100] -> (v + 1100) * 255 / 4200"""
    med = median_filter(x)
    return (np.clip(med, -1100, 3100) + 1100) * 255 / 4200


def phantom(shape, seed=0, amplitude=0.3, noise=5.0):
    """three tissue classes in ellipsoids (100 / 200 / 300 + noise) on a zero background, times exp(b);
    returns (image f32, b, class labels)"""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    r2 = sum(g ** 2 / a ** 2 for g, a in zip(grids, (0.9, 0.85, 0.8)[:len(shape)]))
    r2b = sum((g - c) ** 2 / a ** 2 for g, c, a in zip(grids, (0.1, -0.1, 0.1), (0.55, 0.5, 0.45)[:len(shape)]))
    r2c = sum((g + c) ** 2 / a ** 2 for g, c, a in zip(grids, (0.2, 0.15, 0.2), (0.3, 0.25, 0.3)[:len(shape)]))
    cls = np.zeros(shape, np.int64)
    cls[r2 < 1] = 1
    cls[r2b < 1] = 2
    cls[r2c < 1] = 3
    base = np.array([0.0, 100.0, 200.0, 300.0])[cls]
    b = amplitude * np.sin(1.3 * grids[-1] + 0.4) * np.cos(0.9 * grids[-2] - 0.2)
    if len(shape) == 3:
        b = b + 0.5 * amplitude * grids[0]
    img = (base + (cls > 0) * rng.normal(0, noise, shape)) * np.exp(b)
    return img.astype(np.float32), b, cls
