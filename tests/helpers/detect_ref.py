"""numpy f64 oracle of the vertebra-landmark transforms (segmantic_amd/detect/transforms.py).

Volumes are [z, y, x] / [C, z, y, x]; points, indices and boxes are (x, y, z).  Everything is computed
literally from the definitions (whole-volume min / max, a transpose to [x, y, z] plus np.where for the
argmax), not from the closed forms the kernels use.
"""
from __future__ import annotations

import math

import numpy as np


def sigma32(label: int) -> float:
    return float(np.float32(1.6 + (label - 1.0) * 0.1))


def tail_of(label: int) -> int:
    return int(max(sigma32(label) * 4.0, 0.5) + 0.5)


def kernel_f64(label: int) -> np.ndarray:
    """gaussian_1d(sigma_L, truncated=4.0, approx="erf") in f64, at -tail .. tail"""
    s, tail = sigma32(label), tail_of(label)
    t = 0.70710678 / s
    v = [0.5 * (math.erf(t * (x + 0.5)) - math.erf(t * (x - 0.5))) for x in range(-tail, tail + 1)]
    return np.maximum(np.array(v, dtype=np.float64), 0.0)


def centroid_sums(lab: np.ndarray, k: int) -> np.ndarray:
    """i64 [k + 1, 4] = (count, sum x, sum y, sum z) of labels 0 .. k of a [z, y, x] volume"""
    lab = np.asarray(lab).astype(np.int64)
    z, y, x = np.indices(lab.shape, dtype=np.int64)
    out = np.zeros((k + 1, 4), dtype=np.int64)
    for c in range(k + 1):
        sel = lab == c
        out[c] = [int(sel.sum()), int(x[sel].sum()), int(y[sel].sum()), int(z[sel].sum())]
    return out


def centre(lab: np.ndarray, label: int):
    """(c_x, c_y, c_z) = floor(mean index), as np.average(...).astype(int)"""
    zs, ys, xs = np.nonzero(np.asarray(lab) == label)
    return tuple(int(np.average(v).astype(int)) for v in (xs, ys, zs))


def _axis(label: int, ctr: int, n: int) -> np.ndarray:
    k, t = kernel_f64(label), tail_of(label)
    v = np.zeros(n, dtype=np.float64)
    for i in range(max(ctr - t, 0), min(ctr + t, n - 1) + 1):
        v[i] = k[i - ctr + t]
    return v


def heatmap(lab: np.ndarray, k: int, gamma: float = 1000.0, smooth_3d: bool = False) -> np.ndarray:
    """f64 [k + 1, z, y, x]"""
    lab = np.asarray(lab)
    if lab.ndim == 4:
        lab = lab[0]
    d, h, w = lab.shape
    out = np.zeros((k + 1, d, h, w), dtype=np.float64)
    g = float(np.float32(gamma))
    for label in range(1, k + 1):
        if not np.any(lab == label):
            continue
        cx, cy, cz = centre(lab, label)
        kz, ky = _axis(label, cz, d), _axis(label, cy, h)
        kx = _axis(label, cx, w) if smooth_3d else (np.arange(w) == cx).astype(np.float64)
        p = kz[:, None, None] * ky[None, :, None] * kx[None, None, :]
        mn, mx = p.min(), p.max()
        out[label] = 0.0 if mx == mn else (p - mn) / (mx - mn) * g
    return out


def extract(heat: np.ndarray, threshold: float = 0.5, affine=None) -> dict:
    """{channel: point} as the reference computes it on a [C, x, y, z] array"""
    out = {}
    for c in range(1, heat.shape[0]):
        ch = np.transpose(np.asarray(heat[c], dtype=np.float64), (2, 1, 0))   # [x, y, z]
        if np.isnan(ch).any():
            raise ValueError(f"channel {c} holds NaN")
        m = ch.max()
        if m < threshold:
            continue
        xs, ys, zs = np.where(ch == m)
        p = np.array([xs[0], ys[0], zs[0]], dtype=np.float64)
        if affine is not None:
            a = np.asarray(affine, dtype=np.float64)
            p = a[:3, :3] @ p + a[:3, 3]
        out[c] = p
    return out


def bbox(x: np.ndarray):
    """[[x0, y0, z0], [x1, y1, z1]] of the voxels > 0 in any channel of [C, z, y, x] or [z, y, x]"""
    x = np.asarray(x)
    if x.ndim == 3:
        x = x[None]
    pos = np.any(x > 0, axis=0)
    if not pos.any():
        return [[0, 0, 0], [0, 0, 0]]
    zs, ys, xs = np.nonzero(pos)
    return [[int(xs.min()), int(ys.min()), int(zs.min())], [int(xs.max()) + 1, int(ys.max()) + 1, int(zs.max()) + 1]]


def embed_index(p, affine) -> np.ndarray:
    a = np.asarray(affine, dtype=np.float64)
    return np.round(np.linalg.inv(a[:3, :3]) @ (np.asarray(p, dtype=np.float64) - a[:3, 3])).astype(np.int64)
