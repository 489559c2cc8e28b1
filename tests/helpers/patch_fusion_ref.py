"""Numpy restatement of patch-based label fusion (``segmantic_amd/csrc/patch_fusion.hip``):
the quantiser, the candidates, the integer patch distances (by cumulative-sum box sums, or tap by tap with
``direct=True``), the denominator, the table weight, the scores with their fallback and the arg-max.  ``fault``
seeds one deviation from the definition; the exact comparison of the GPU tests must tell each from the definition
(``tests/test_patch_fusion_host.py`` shows an input for every one).  Also the phantom of the usefulness condition.

Everything is integer numpy after the quantiser; results are read-only and the callers share them."""
from __future__ import annotations

from itertools import product
from types import SimpleNamespace

import numpy as np

TABLE_ENTRIES = 1024
FAULTS = ("outside", "double_clamp", "tie_largest", "no_floor", "round_k", "no_fallback")
# "double_clamp" clamps in two steps, the patch position first: clamp(clamp(x + p) + o).  The other order,
# clamp(clamp(x + o) + p) ("double_clamp_offset_first"), is no fault at all: a candidate exists only when x + o lies
# inside the volume, where the inner clamp changes nothing.  It is kept to show exactly that.
HARMLESS = ("double_clamp_offset_first",)


# ---------------------------------------------------------------------------- step 1
def quantise(v, lo, hi, fma: bool = False) -> np.ndarray:
    """uint8 of clamp(floor((v - lo) * scale + 0.5), 0, 255) in float32, every operation rounded on its own; NaN -> 0.
    ``fma``: the seeded fault, product and + 0.5 rounded once (the exact product of two float32 and the sum with 0.5
    fit float64 for every t that the clamp does not decide anyway)."""
    v = np.asarray(v, np.float32)
    lo32, scale = np.float32(lo), np.float32(255.0 / (float(hi) - float(lo)))
    with np.errstate(invalid="ignore", over="ignore"):
        diff = v - lo32
        if fma:
            t = (diff.astype(np.float64) * np.float64(scale) + 0.5).astype(np.float32)
        else:
            t = diff * scale + np.float32(0.5)
        q = np.floor(t)
        return np.where(q > 0, np.minimum(q, np.float32(255)), np.float32(0)).astype(np.uint8)


def default_range(image) -> tuple:
    """(lo, hi): the order statistics at ranks floor(0.005 (N - 1)) and ceil(0.995 (N - 1)) of the sorted values"""
    s = np.sort(np.asarray(image, np.float32).ravel())
    n = s.size
    return float(s[int(np.floor(0.005 * (n - 1)))]), float(s[int(np.ceil(0.995 * (n - 1)))])


def table(beta: float = 1.0) -> np.ndarray:
    k = np.arange(TABLE_ENTRIES, dtype=np.float64)
    return np.floor(65536.0 * np.exp(-k / (64.0 * beta)) + 0.5).astype(np.uint32)


# ---------------------------------------------------------------------------- steps 2 - 7
def radii(shape3, radius) -> tuple:
    r = (radius,) * 3 if np.isscalar(radius) else tuple(int(v) for v in radius)
    return tuple(0 if n == 1 else int(v) for n, v in zip(shape3, r))


def _box(a: np.ndarray, r: int, axis: int) -> np.ndarray:
    """sums of 2r + 1 consecutive entries along ``axis`` (n + 2r entries -> n), by one cumulative sum"""
    if r == 0:
        return a
    c = np.cumsum(a, axis=axis)
    zero = np.zeros_like(np.take(c, [0], axis=axis))
    c = np.concatenate([zero, c], axis=axis)
    n = c.shape[axis]
    return np.take(c, range(2 * r + 1, n), axis=axis) - np.take(c, range(0, n - 2 * r - 1), axis=axis)


def _candidates(T, I, L, rp, rs, fault, direct):
    """yields (D int64 [A, d, h, w], exists bool [d, h, w], labels int64 [A, d, h, w] at x + o) per offset"""
    d, h, w = T.shape
    ext = (d, h, w)
    two_step = fault in ("double_clamp",) + HARMLESS
    if not (direct or two_step):
        Tp = np.pad(T, [(r, r) for r in rp], mode="edge")
        Ip = np.pad(I, [(0, 0)] + [(p + s, p + s) for p, s in zip(rp, rs)], mode="edge")
    Lp = np.pad(L, [(0, 0)] + [(s, s) for s in rs], mode="edge")
    grid = [np.arange(n) for n in ext]
    for o in product(*[range(-s, s + 1) for s in rs]):
        if direct or two_step:
            D = np.zeros((I.shape[0],) + ext, np.int64)
            for p in product(*[range(-r, r + 1) for r in rp]):
                ti = [np.clip(g + pp, 0, n - 1) for g, pp, n in zip(grid, p, ext)]
                if fault == "double_clamp":
                    ii = [np.clip(np.clip(g + pp, 0, n - 1) + oo, 0, n - 1) for g, oo, pp, n in zip(grid, o, p, ext)]
                elif two_step:
                    ii = [np.clip(np.clip(g + oo, 0, n - 1) + pp, 0, n - 1) for g, oo, pp, n in zip(grid, o, p, ext)]
                else:
                    ii = [np.clip(g + oo + pp, 0, n - 1) for g, oo, pp, n in zip(grid, o, p, ext)]
                D += (T[np.ix_(*ti)][None] - I[(slice(None),) + np.ix_(*ii)]) ** 2
        else:
            sl = tuple(slice(s + oo, s + oo + n + 2 * r) for s, oo, n, r in zip(rs, o, ext, rp))
            e = (Tp[None] - Ip[(slice(None),) + sl]) ** 2
            D = _box(_box(_box(e, rp[2], 3), rp[1], 2), rp[0], 1)
        inside = [(g + oo >= 0) & (g + oo < n) for g, oo, n in zip(grid, o, ext)]
        exists = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
        if fault == "outside":
            exists = np.ones(ext, bool)
        lab = Lp[(slice(None),) + tuple(slice(s + oo, s + oo + n) for s, oo, n in zip(rs, o, ext))]
        yield D, exists, lab


def check_labels(L, K: int) -> None:
    """the refusal of the kernel: the first voxel that holds a label outside 0 .. K-1, there the first atlas"""
    A = len(L)
    flat = np.stack([np.asarray(l).reshape(-1).astype(np.int64) for l in L])
    bad = (flat < 0) | (flat >= K)
    if bad.any():
        i = int(np.argmax(bad.any(axis=0)))
        a = int(np.argmax(bad[:, i]))
        raise ValueError(f"patch_fusion: atlas {a} holds the label {int(flat[a, i])}, outside 0 .. {K - 1}")


def fuse(target_q, atlas_q, atlas_labels, K: int, rp=1, rs=2, table=None, h2=None, min_h2: int = 4, fault=None,
         direct: bool = False) -> SimpleNamespace:
    """labels (dtype of the label maps), best, total (uint32) and scores (uint32 [K, ...]) of the definition.
    ``h2`` None: adaptive bandwidth with the floor npatch * min_h2."""
    assert fault is None or fault in FAULTS + HARMLESS
    shape = np.asarray(target_q).shape
    shape3 = (1,) * (3 - len(shape)) + tuple(shape)
    check_labels(atlas_labels, K)
    T = np.asarray(target_q).reshape(shape3).astype(np.int64)
    I = np.stack([np.asarray(q).reshape(shape3).astype(np.int64) for q in atlas_q])
    L = np.stack([np.asarray(l).reshape(shape3).astype(np.int64) for l in atlas_labels])
    W = np.asarray(table).astype(np.int64)
    assert W.shape == (TABLE_ENTRIES,)
    rp, rs = radii(shape3, rp), radii(shape3, rs)
    npatch = int(np.prod([2 * r + 1 for r in rp]))
    A, N = I.shape[0], T.size
    if h2 is None:
        dmin = np.full(shape3, np.iinfo(np.int64).max)
        for D, exists, _ in _candidates(T, I, L, rp, rs, fault, direct):
            dmin = np.minimum(dmin, np.where(exists[None], D, np.iinfo(np.int64).max).min(axis=0))
        den = np.maximum(dmin, 1 if fault == "no_floor" else npatch * int(min_h2))
    else:
        den = np.full(shape3, npatch * int(h2), np.int64)
    scores = np.zeros(K * N, np.int64)
    voxel = np.broadcast_to(np.arange(N).reshape(shape3)[None], (A,) + shape3)
    for D, exists, lab in _candidates(T, I, L, rp, rs, fault, direct):
        k = (2 * 64 * D + den[None]) // (2 * den[None]) if fault == "round_k" else 64 * D // den[None]
        wgt = W[np.minimum(k, TABLE_ENTRIES - 1)] * exists[None]
        scores += np.bincount((lab * N + voxel).ravel(), weights=wgt.ravel().astype(np.float64),
                              minlength=K * N).astype(np.int64)           # sums below 2^29: exact in float64
    scores = scores.reshape(K, N)
    if fault != "no_fallback":
        empty = scores.sum(axis=0) == 0
        vote = np.stack([(L.reshape(A, N) == l).sum(axis=0) for l in range(K)])
        scores = np.where(empty[None], vote, scores)
    if fault == "tie_largest":
        arg = K - 1 - np.argmax(scores[::-1], axis=0)
    else:
        arg = np.argmax(scores, axis=0)                                    # the first maximum: the smallest label
    out = SimpleNamespace(labels=arg.reshape(shape).astype(np.asarray(atlas_labels[0]).dtype),
                          best=scores.max(axis=0).reshape(shape).astype(np.uint32),
                          total=scores.sum(axis=0).reshape(shape).astype(np.uint32),
                          scores=scores.reshape((K,) + tuple(shape)).astype(np.uint32), den=den.reshape(shape))
    for a in (out.labels, out.best, out.total, out.scores, out.den):
        a.setflags(write=False)
    return out


def vote(atlas_labels, K: int) -> np.ndarray:
    """majority vote, the smallest label among equal counts"""
    L = np.stack([np.asarray(l).astype(np.int64) for l in atlas_labels])
    return np.argmax(np.stack([(L == l).sum(axis=0) for l in range(K)]), axis=0).astype(np.asarray(atlas_labels[0]).dtype)


# ---------------------------------------------------------------------------- the phantom
def shift_edge(a: np.ndarray, off) -> np.ndarray:
    """out[x] = a[clamp(x - off)]"""
    idx = [np.clip(np.arange(n) - int(o), 0, n - 1) for n, o in zip(a.shape, off)]
    return a[np.ix_(*idx)]


def phantom(shape=(12, 20, 28), classes: int = 4, atlases: int = 5, seed: int = 0, max_shift=(1, 2, 2), noise: float = 8.0,
            dtype=np.uint8) -> SimpleNamespace:
    """truth: ellipsoids of the classes 1 .. classes-1 on background 0, with class intensities spread over 0 .. 255;
    target = intensity of the truth + noise; atlas a = the truth shifted by a seeded offset (|.| <= max_shift per
    axis, never all zero when a shift is allowed), its image with a gain of 0.9 .. 1.1 and its own noise."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    truth = np.zeros(shape, np.int64)
    for c in range(1, classes):
        centre = [rng.uniform(0.25, 0.75) * n for n in shape]
        radius = [max(1.5, rng.uniform(0.18, 0.36) * n) for n in shape]
        inside = sum(((g - m) / r) ** 2 for g, m, r in zip((z, y, x), centre, radius)) <= 1.0
        truth[inside] = c
    means = 30.0 + 195.0 * rng.permutation(classes) / max(classes - 1, 1)
    target = (means[truth] + rng.normal(0.0, noise, shape)).astype(np.float32)
    images, labels, offsets = [], [], []
    for _ in range(atlases):
        off = tuple(int(rng.integers(-m, m + 1)) for m in max_shift)
        while any(max_shift) and not any(off):
            off = tuple(int(rng.integers(-m, m + 1)) for m in max_shift)
        lab = shift_edge(truth, off)
        gain = rng.uniform(0.9, 1.1)
        images.append((gain * means[lab] + rng.normal(0.0, noise, shape)).astype(np.float32))
        labels.append(lab.astype(dtype))
        offsets.append(off)
    for a in [target, truth] + images + labels:
        a.setflags(write=False)
    return SimpleNamespace(target=target, truth=truth.astype(dtype), images=images, labels=labels, offsets=offsets,
                           classes=classes)


def fuse_images(ph: SimpleNamespace, rp=1, rs=2, beta: float = 1.0, **kw) -> SimpleNamespace:
    """the phantom through the default ranges, the quantiser and ``fuse``"""
    tq = quantise(ph.target, *default_range(ph.target))
    iq = [quantise(im, *default_range(im)) for im in ph.images]
    return fuse(tq, iq, ph.labels, ph.classes, rp, rs, table(beta), **kw)
