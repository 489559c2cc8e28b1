"""Independent numpy oracle of the Nyul-Udupa standardisation contract (segmantic_amd.seg.nyul_normalize).

Exact order statistics by ``np.partition``; ranks and lerp in torch.quantile's f32 arithmetic (its lerp
is a fused multiply-add) for n <= 2^24 and numpy.quantile's f64 arithmetic above; the map in f32 with every operation rounded.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

EXACT_LIMIT = 1 << 24
F32 = np.float32


def order_stats(v: np.ndarray, ranks) -> np.ndarray:
    """exact order statistics of the f32 values ``v`` (no NaN) at ``ranks``"""
    ranks = np.unique(np.asarray(ranks, dtype=np.int64))
    part = np.partition(v, ranks)
    return dict(zip(ranks.tolist(), part[ranks].tolist()))


def _round32(x: Fraction) -> np.float32:
    """an exact rational rounded once to f32, to nearest even"""
    f = np.float32(float(x))
    if not np.isfinite(f):
        return f
    best = f
    for c in (np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))):
        if not np.isfinite(c):
            continue
        dc, db = abs(Fraction(float(c)) - x), abs(Fraction(float(best)) - x)
        if dc < db or (dc == db and int(c.view(np.int32)) % 2 == 0):
            best = c
    return F32(best)


def _fma32(a, b, c) -> np.float32:
    a, b, c = F32(a), F32(b), F32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return F32(np.float64(a) * np.float64(b) + np.float64(c))
    return _round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _lerp32(a, b, w):
    """torch's lerp as its kernels compile it: one fused multiply-add per branch"""
    a, b, w = F32(a), F32(b), F32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = F32(b - a)
        if abs(w) < F32(0.5):
            return _fma32(w, d, a)
        return _fma32(-d, F32(F32(1.0) - w), b)


def _lerp64(a, b, w):
    a, b, w = float(a), float(b), float(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float64(b) - np.float64(a)
        if w < 0.5:
            return F32(np.float64(a) + np.float64(w) * d)
        return F32(np.float64(b) - d * (np.float64(1.0) - np.float64(w)))


def ranks(q: float, n: int):
    """(lo, hi, w) of quantile q among n values, by the regime of n"""
    if n <= EXACT_LIMIT:
        rank = F32(F32(q) * F32(n - 1))
        lo, hi = int(np.trunc(rank)), int(np.ceil(rank))
        return lo, hi, F32(rank - F32(lo))
    vi = float(q) * float(n - 1)
    lo = int(np.floor(vi))
    hi = lo if vi >= n - 1 else lo + 1
    return lo, hi, vi - lo


def landmarks(values: np.ndarray, quantiles) -> np.ndarray:
    """landmarks f32 [L] of the masked values of one segment (NaN when empty or holding NaN)"""
    v = np.asarray(values, dtype=F32).reshape(-1)
    q = np.asarray(quantiles, dtype=np.float64)
    n = v.size
    if n == 0 or np.isnan(v).any():
        return np.full(q.size, np.nan, F32)
    rk = [ranks(qq, n) for qq in q]
    st = order_stats(v, [r for lo, hi, _ in rk for r in (lo, hi)])
    lerp = _lerp32 if n <= EXACT_LIMIT else _lerp64
    return np.array([lerp(st[lo], st[hi], w) for lo, hi, w in rk], dtype=F32)


def interp(x: np.ndarray, xp: np.ndarray, fp: np.ndarray) -> np.ndarray:
    """the reference's torch interp1d in f32, each operation rounded"""
    x = np.asarray(x, F32)
    xp, fp = np.asarray(xp, F32), np.asarray(fp, F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = ((fp[1:] - fp[:-1]) / (xp[1:] - xp[:-1])).astype(F32)
        b = (fp[:-1] - (m * xp[:-1]).astype(F32)).astype(F32)
        i = np.clip(np.searchsorted(xp, x.reshape(-1), side="left") - 1, 0, m.size - 1)
        y = ((m[i] * x.reshape(-1)).astype(F32) + b[i]).astype(F32)
    return y.reshape(x.shape)


def segments(img: np.ndarray, channel_wise: bool):
    a = np.asarray(img, F32)
    return [a[c] for c in range(a.shape[0])] if channel_wise else [a]


def mask_of(seg: np.ndarray, nonzero: bool) -> np.ndarray:
    return seg != 0 if nonzero else np.ones(seg.shape, bool)


def all_landmarks(img, quantiles, nonzero=False, channel_wise=False) -> np.ndarray:
    return np.stack([landmarks(s[mask_of(s, nonzero)], quantiles) for s in segments(img, channel_wise)])


def apply_with(img, lms, standard_scale, nonzero=False, channel_wise=False) -> np.ndarray:
    """the map of every segment given its landmarks (an empty mask leaves the segment unchanged)"""
    out = np.array(img, dtype=F32, copy=True)
    segs = [out[c] for c in range(out.shape[0])] if channel_wise else [out]
    for s, lm in zip(segs, lms):
        m = mask_of(s, nonzero)
        if m.any():
            s[m] = interp(s[m], lm, standard_scale)
    return out


def normalize(img, quantiles, standard_scale, nonzero=False, channel_wise=False) -> np.ndarray:
    q = np.asarray(quantiles, np.float64)
    order = np.argsort(q, kind="stable")
    q, s = q[order], np.asarray(standard_scale, np.float64)[order]
    lms = all_landmarks(img, q, nonzero, channel_wise)
    return apply_with(img, lms, s, nonzero, channel_wise)


def fit(images, quantiles, nonzero=False, channel_wise=False, s_min=0.0, s_max=100.0):
    q = np.sort(np.asarray(quantiles, np.float64), kind="stable")
    rows = np.concatenate([all_landmarks(im, q, nonzero, channel_wise) for im in images]).astype(np.float64)
    keep = np.all(np.isfinite(rows), axis=1) & (rows[:, 0] != rows[:, -1])
    lk = rows[keep]
    mapped = s_min + (lk - lk[:, :1]) * ((s_max - s_min) / (lk[:, -1:] - lk[:, :1]))
    return mapped.mean(axis=0), int(np.count_nonzero(~keep))
