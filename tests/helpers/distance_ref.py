"""CPU oracle of the evaluation contract (segmantic_amd/seg/evaluation.py), written from the definitions:
brute-force distance transforms for small sizes, a numpy separable exact transform (minimum over every
parabola of a line, vectorised over lines) for 64^3 - 160^3, and the metrics as numpy restates them."""
from __future__ import annotations

import math

import numpy as np


def contour(mask: np.ndarray) -> np.ndarray:
    """foreground voxels with a background face neighbour (outside the image = background)"""
    m = mask.astype(bool)
    inner = m.copy()
    for ax in range(m.ndim):
        pad = [(1, 1) if a == ax else (0, 0) for a in range(m.ndim)]
        p = np.pad(m, pad, constant_values=False)
        lo = [slice(None)] * m.ndim
        hi = [slice(None)] * m.ndim
        lo[ax] = slice(0, -2)
        hi[ax] = slice(2, None)
        inner &= p[tuple(lo)] & p[tuple(hi)]
    return m & ~inner


def edt_sq_brute(feature: np.ndarray, spacing) -> np.ndarray:
    """squared distance of every voxel to the nearest True voxel of feature (f64; inf when none)"""
    sp = np.asarray(spacing, np.float64)
    pts = np.argwhere(feature).astype(np.float64) * sp
    grid = np.indices(feature.shape).reshape(feature.ndim, -1).T.astype(np.float64) * sp
    if len(pts) == 0:
        return np.full(feature.shape, np.inf)
    out = np.empty(len(grid))
    for s in range(0, len(grid), 4096):
        g = grid[s:s + 4096]
        out[s:s + 4096] = ((g[:, None, :] - pts[None, :, :]) ** 2).sum(-1).min(1)
    return out.reshape(feature.shape)


def edt_sq_separable(feature: np.ndarray, spacing) -> np.ndarray:
    """exact separable transform: along each axis D[i] = min_j g[j] + (s (i - j))^2 (f64)"""
    g = np.where(feature, 0.0, np.inf)
    for ax, s in enumerate(spacing):
        g = np.moveaxis(g, ax, 0)
        n = g.shape[0]
        out = np.full_like(g, np.inf)
        idx = np.arange(n, dtype=np.float64)
        for j in range(n):
            w = ((idx - j) * float(s)) ** 2
            np.minimum(out, g[j][None] + w.reshape((n,) + (1,) * (g.ndim - 1)), out=out)
        g = np.moveaxis(out, 0, ax)
    return g


def directed(query_pts: np.ndarray, dist_sq: np.ndarray) -> np.ndarray:
    return np.sqrt(dist_sq[query_pts])


def metrics(pred: np.ndarray, ref: np.ndarray, spacing, percentile=95.0, edt=edt_sq_separable):
    """every value of evaluation.surface_distances for one binary pair, from the definitions"""
    a, b = pred.astype(bool), ref.astype(bool)
    if not a.any() or not b.any():
        return None
    ca, cb = contour(a), contour(b)
    da_c, db_c = edt(ca, spacing), edt(cb, spacing)     # to the contours
    da_f, db_f = edt(a, spacing), edt(b, spacing)       # to the foregrounds
    s_ab, s_ba = directed(ca, db_c), directed(cb, da_c)
    p_ab, p_ba = directed(a, db_f), directed(b, da_f)
    s = np.concatenate([s_ba, s_ab])
    p = np.concatenate([p_ba, p_ab])
    out = {
        "surface_mean": s.mean(), "surface_median": np.median(s), "surface_std": s.std(), "surface_max": s.max(),
        "pointwise_mean": p.mean(), "pointwise_median": np.median(p), "pointwise_std": p.std(),
        "pointwise_max": p.max(), "hausdorff": p.max(), "average_hausdorff": 0.5 * (p_ab.mean() + p_ba.mean()),
        "surface_mean_directed": (s_ab.mean(), s_ba.mean()),
        "n_surface": (len(s_ab), len(s_ba)),
    }
    if percentile is None:
        out["percentile_hausdorff"] = s.max()
    else:
        out["percentile_hausdorff"] = max(np.percentile(s_ab, percentile), np.percentile(s_ba, percentile))
    return out


def label_metrics(pred: np.ndarray, ref: np.ndarray, label: int, spacing, percentile=95.0):
    return metrics(pred == label, ref == label, spacing, percentile)


def known_masks():
    """the reference's tests/seg/test_evaluation.py masks, written in sitk [x, y] order, as [y, x] arrays"""
    a = np.zeros((10, 10), np.uint8)
    b = np.zeros((10, 10), np.uint8)
    a[3:6, 3:6] = 1          # sitk A[3:6, 3:6] (x, y) -> array [y, x]
    b[2:7, 1:8] = 1          # sitk B[1:8, 2:7]
    return a, b


KNOWN = {
    "surface": {"mean": 1.5214687914104121, "median": math.sqrt(2), "std": 0.5065187935237067, "max": math.sqrt(5)},
    "surface_directed": (1.25, 1.6300563079745771),
    "n_surface": (8, 20),
    "hd95": math.sqrt(5),
    "pointwise": {"mean": 0.8772983218066259, "median": 1.0, "max": math.sqrt(5)},
    "average_hausdorff": 0.5514446594213077,
    "surface_aniso": {"mean": 1.0760353644461413, "max": math.sqrt(2)},   # spacing (x, y) = (0.5, 1.0)
}
