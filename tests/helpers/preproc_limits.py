"""Inputs that drive the landmark kernels (``segmantic_amd/csrc/landmarks.hip``: centroid sums, heatmap, channel
argmax, positive box) and the Nyul kernels (``segmantic_amd/csrc/nyul.hip``: segmented radix select, the map) past
their row trips, grid caps, label tables, slot groups and rank regimes, and the arithmetic that proves it.

The limits are constants of the ``.hip`` sources.  :func:`read_limits` reads the named ones as text and carries the
three literals of the ``chunks_per_segment(...)`` calls as named numbers with the source line each must still stand
on.  The generators below have FIXED sizes (written out as numbers): a generator that followed a changed constant
would hide the change.  :func:`crossings` recomputes, from the inputs alone, every quantity that has to cross a limit
and returns one message per case that no longer does; ``tests/test_preproc_limits_host.py`` asserts that the list is
empty.

The numpy restatements (:func:`centroid_by_trips`, :func:`argmax_by_trips`, :func:`radix_select`,
:func:`rank_rule`) follow the kernels' own decomposition (trips along x, slots per pass, the regime of n).  Each
takes ``fault=``: one planted line that a kernel could get wrong beyond its tested sizes.  The host test shows that
every fault changes the result on the inputs below, i.e. that the GPU tests' comparisons would notice it.

Everything here is numpy on the host; results are read-only and cached."""
from __future__ import annotations

import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from . import detect_ref, nyul_ref

CSRC = Path(__file__).resolve().parents[2] / "segmantic_amd" / "csrc"

# name -> file of the `constexpr int kName = <integer>;` (or `<integer> << <integer>`) definitions
NAMED = {"kLmMaxLabels": "landmarks.hip", "kLmMaxWgs": "landmarks.hip", "kNyulMaxLandmarks": "nyul.hip",
         "kNyulBins": "nyul.hip", "kSlotsLds": "nyul.hip", "kHistThreads": "nyul.hip", "kExactRankLimit": "nyul.hip"}
# the bare literals: name -> (file, the text its line must hold, the numbers read out of that text)
LITERALS = {
    "pass_a_grid": ("nyul.hip", "chunks_per_segment(seg_len, segments, 512, kHistThreads)", {"pass_a_per_chip": 512}),
    "pass_bc_grid": ("nyul.hip", "chunks_per_segment(seg_len, segments, 256, kHistThreads)", {"pass_bc_per_chip": 256}),
    "map_grid": ("nyul.hip", "chunks_per_segment(seg_len, segments, 2048, 256)", {"map_per_chip": 2048}),
}
LANES = 64                                        # a wave; one wave walks one row
ROWS_PER_WG = 4                                   # waves per workgroup of the row walkers


def cdiv(a: int, b: int) -> int:
    return -(-int(a) // int(b))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def read_limits(csrc: Path = CSRC) -> SimpleNamespace:
    """the limits of the sources under ``csrc``; ``missing`` lists the literal lines that are no longer there"""
    csrc = Path(csrc)
    text = {f: (csrc / f).read_text() for f in {*NAMED.values(), *(v[0] for v in LITERALS.values())}}
    out = {}
    for name, f in NAMED.items():
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*;" % name, text[f])
        if m is None:
            raise AssertionError(f"{f} no longer defines `constexpr int {name} = <integer>;`")
        out[name] = int(m.group(1)) << int(m.group(2) or 0)
    missing = []
    for key, (f, line, numbers) in LITERALS.items():
        out.update(numbers)
        if line not in text[f]:
            missing.append(f"{f} no longer holds `{line}`: the numbers {numbers} of tests/helpers/preproc_limits.py "
                           f"describe a launch that has changed")
    return SimpleNamespace(missing=missing, **out)


def trips(w: int, v: int) -> int:
    """trips of 64 V lanes that a row of w voxels takes"""
    return cdiv(w, LANES * v)


def lm_grid(rows: int, channels: int, cap: int) -> int:
    """lm_grid of landmarks.hip: workgroups along x of the grid"""
    g = cdiv(rows, ROWS_PER_WG)
    c = cap // max(channels, 1)
    return min(g, max(c, 1))


def misaligned(offset_elements: int, itemsize: int) -> bool:
    """whether a view that starts `offset_elements` into an aligned buffer fails the V = 4 test of the launchers
    (address % (4 itemsize) == 0)"""
    return (offset_elements * itemsize) % (4 * itemsize) != 0


# ====================================================================== landmarks.hip
LABEL_DTYPES = ("uint8", "int16", "int32")
VIEW_OFFSET = 1                                   # elements between the buffer and the misaligned view

# ------------------------------------------------------------------ centroid sums
CENT_V4_SHAPE = (6, 7, 520)                       # 520 = 2 * 256 + 8: three trips at V = 4, the last with 8 voxels
CENT_V1_SHAPE = (5, 6, 203)                       # 203 = 3 * 64 + 11: four trips at V = 1, the last ragged
CENT_K = 12
CENT_DENSE_SHAPE, CENT_DENSE_K = (4, 5, 520), 255
CENT_LATE_SHAPE, CENT_LATE_K, CENT_LATE_LABEL, CENT_LATE_FROM = (3, 4, 520), 3, 2, 256


@functools.lru_cache(maxsize=None)
def cent_volume(shape, dtype: str) -> np.ndarray:
    """labels 0 .. CENT_K in runs of 1 .. 40 voxels along x (several labels per chunk, on every trip), label
    CENT_K - 1 absent"""
    d, h, w = shape
    rng = np.random.default_rng(d * 1000 + w)
    n = d * h * w
    run = rng.integers(1, 41, n)
    starts = np.cumsum(run)
    starts = starts[starts < n]
    val = rng.integers(0, CENT_K + 1, starts.size + 1)
    val[val == CENT_K - 1] = 0
    lab = val[np.searchsorted(starts, np.arange(n), side="right")].astype(dtype).reshape(shape)
    return _frozen(lab)


@functools.lru_cache(maxsize=None)
def cent_dense(dtype: str) -> np.ndarray:
    """uniformly random labels 0 .. 255: every lane of a chunk holds other labels than its neighbours"""
    lab = np.random.default_rng(255).integers(0, 256, CENT_DENSE_SHAPE).astype(dtype)
    return _frozen(lab)


@functools.lru_cache(maxsize=None)
def cent_late(dtype: str) -> np.ndarray:
    """labels 0, 1, 3 anywhere, label 2 only at x >= 256: its sum x is nonzero only through x0"""
    rng = np.random.default_rng(2)
    lab = rng.choice(np.array([0, 1, 3]), CENT_LATE_SHAPE)
    late = rng.random(CENT_LATE_SHAPE) < 0.3
    late[..., :CENT_LATE_FROM] = False
    lab[late] = CENT_LATE_LABEL
    return _frozen(lab.astype(dtype))


def distinct_per_chunk(lab: np.ndarray, v: int) -> np.ndarray:
    """distinct labels in every full chunk of 64 V voxels of every row"""
    rows = lab.reshape(-1, lab.shape[-1])
    c = LANES * v
    return np.array([np.unique(r[x0:x0 + c]).size for r in rows for x0 in range(0, rows.shape[1] - c + 1, c)])


def centroid_by_trips(lab: np.ndarray, k: int, v: int, fault=None) -> np.ndarray:
    """centroid_kernel restated: i64 [k + 1, 4], the sums of each trip of 64 V voxels taken with x local to the
    trip, plus count * x0.  fault "x0_dropped": the x0 term counts on the first trip only."""
    lab = np.asarray(lab).astype(np.int64)
    d, h, w = lab.shape
    out = np.zeros((k + 1, 4), np.int64)
    z, y = np.indices((d, h))
    for x0 in range(0, w, LANES * v):
        chunk = lab[:, :, x0:x0 + LANES * v]
        local = np.broadcast_to(np.arange(chunk.shape[2]), chunk.shape)
        cnt = np.bincount(chunk.ravel(), minlength=k + 1)[:k + 1]
        off = 0 if fault == "x0_dropped" else x0
        out[:, 0] += cnt
        out[:, 1] += cnt * off + np.bincount(chunk.ravel(), weights=local.ravel(), minlength=k + 1)[:k + 1].astype(np.int64)
        out[:, 2] += np.bincount(chunk.ravel(), weights=np.broadcast_to(y[..., None], chunk.shape).ravel(),
                                 minlength=k + 1)[:k + 1].astype(np.int64)
        out[:, 3] += np.bincount(chunk.ravel(), weights=np.broadcast_to(z[..., None], chunk.shape).ravel(),
                                 minlength=k + 1)[:k + 1].astype(np.int64)
    return out


# ------------------------------------------------------------------ heatmap
HM_TRIP_SHAPE, HM_TRIP_K = (6, 40, 520), 12
# label -> (z, y, x) of a 2 x 2 x 2 block's low corner; the centre (floor of the mean) is that corner
HM_TRIP_BLOCKS = {3: (1, 5, 250), 5: (2, 12, 255), 7: (3, 20, 256), 9: (4, 30, 262), 12: (2, 35, 500), 1: (0, 2, 515)}
HM_BIG_SHAPE, HM_BIG_K = (12, 16, 300), 255
HM_BIG_BLOCKS = {1: (2, 3, 10), 128: (6, 8, 140), 255: (9, 12, 250)}
# Covered by label 255's support (tail 108), and large enough for f32: the channel is (P - min P) / (max P - min P),
# which multiplies the rounding of P (five roundings of 2^-24 in a product of three table entries, as many again in
# min P and max P) by max P / (max P - min P).  The bound of 1e-6 gamma is 17 x 2^-24 gamma, so the factor has to stay
# under 1.4, i.e. min P <= 0.29 max P.  A volume of a few voxels per axis cannot be held to that bound by any f32
# evaluation: at (5, 6, 8) min P = 0.98 max P, the factor is 50 and correctly rounded tables still leave 4e-6 gamma.
HM_COVER_SHAPE, HM_COVER_K = (24, 30, 40), 255
HM_COVER_BLOCKS = {255: (2, 2, 3)}
HM_COVER_MAX_RATIO = 0.29
HM_STRIDE = 217                                   # words per label of the parameter table at k = 255


def _blocks(shape, blocks, dtype) -> np.ndarray:
    lab = np.zeros(shape, np.dtype(dtype))
    for c, (z, y, x) in blocks.items():
        lab[z:z + 2, y:y + 2, x:x + 2] = c
    return _frozen(lab)


@functools.lru_cache(maxsize=None)
def hm_trip_volume() -> np.ndarray:
    return _blocks(HM_TRIP_SHAPE, HM_TRIP_BLOCKS, "int16")


@functools.lru_cache(maxsize=None)
def hm_big_volume() -> np.ndarray:
    return _blocks(HM_BIG_SHAPE, HM_BIG_BLOCKS, "uint8")


@functools.lru_cache(maxsize=None)
def hm_cover_volume() -> np.ndarray:
    return _blocks(HM_COVER_SHAPE, HM_COVER_BLOCKS, "int32")


def hm_support(lab: np.ndarray, label: int):
    """[(lo, hi)] per axis (x, y, z) of the smoothed support of `label`, clipped to the volume, and whether it was
    clipped on that axis"""
    d, h, w = lab.shape
    t = detect_ref.tail_of(label)
    out = []
    for ctr, n in zip(detect_ref.centre(lab, label), (w, h, d)):
        out.append((max(ctr - t, 0), min(ctr + t, n - 1), ctr - t < 0 or ctr + t > n - 1))
    return out


# ------------------------------------------------------------------ channel argmax
AM_SHAPES = ((3, 5, 6, 520), (3, 5, 6, 203))
AM_MANY_SHAPE = (4100, 2, 3, 5)
AM_PEAK = 2.0                                     # planted maxima; the background lies in [0, 1)


@functools.lru_cache(maxsize=None)
def am_volume(shape) -> np.ndarray:
    """f32 [3, 5, 6, w].  channel 0: one maximum beyond the first trip.  channel 1: the maximum twice in one lane,
    one trip apart, the later one first in linear [z, y, x] order, and once more in another lane further on.
    channel 2: small integers, so tied everywhere."""
    c, d, h, w = shape
    step = 256 if w % 4 == 0 else 64              # voxels of one trip
    rng = np.random.default_rng(w)
    x = rng.random(shape, dtype=np.float32)
    x[0, 2, 3, step + 37] = AM_PEAK
    x[1, 4, 5, step - 56] = AM_PEAK               # first trip; late in linear order
    x[1, 0, 0, 2 * step - 56] = AM_PEAK           # the same lane one trip on; early in linear order
    x[1, 1, 1, 2 * step + 3] = AM_PEAK
    x[2] = rng.integers(0, 4, (d, h, w)).astype(np.float32)
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def am_many() -> np.ndarray:
    """f32 [4100, 2, 3, 5]: one distinct maximum per channel, at a position that varies with the channel"""
    c, d, h, w = AM_MANY_SHAPE
    x = np.random.default_rng(4100).random(AM_MANY_SHAPE, dtype=np.float32)
    i = np.arange(c)
    x[i, i % d, (i // 2) % h, (i // 7) % w] = AM_PEAK + i.astype(np.float32)
    return _frozen(x)


def am_nan_volume() -> np.ndarray:
    """am_volume of the first shape with a NaN at x >= 256 of channel 1"""
    x = am_volume(AM_SHAPES[0]).copy()
    x[1, 3, 2, 300] = np.nan
    return _frozen(x)


def argmax_points(heat: np.ndarray):
    """(max f32 [c], first (x, y, z) i64 [c, 3]) of every channel of [c, z, y, x] by detect_ref.extract (which
    skips channel 0: a dummy channel goes in front)"""
    heat = np.asarray(heat, np.float32)
    pts = detect_ref.extract(np.concatenate([np.zeros_like(heat[:1]), heat]), threshold=-np.inf)
    xyz = np.stack([pts[c + 1] for c in range(heat.shape[0])]).astype(np.int64)
    return heat.reshape(heat.shape[0], -1).max(axis=1), xyz


def argmax_by_trips(heat: np.ndarray, v: int, fault=None):
    """argmax_kernel restated: per trip of 64 V voxels along x the maximum and its first (x, y, z); a later trip
    replaces the best so far only when it is greater.  fault "later_trip_wins": when it is greater or equal."""
    heat = np.asarray(heat, np.float32)
    vals, pts = [], []
    for ch in heat:
        t = np.transpose(ch, (2, 1, 0))           # [x, y, z]: C order is the lexicographic order of (x, y, z)
        best, at = None, None
        for x0 in range(0, t.shape[0], LANES * v):
            part = t[x0:x0 + LANES * v]
            i = np.unravel_index(int(np.argmax(part)), part.shape)
            m = part[i]
            if best is None or (m >= best if fault == "later_trip_wins" else m > best):
                best, at = m, (x0 + i[0], i[1], i[2])
        vals.append(best)
        pts.append(at)
    return np.array(vals, np.float32), np.array(pts, np.int64)


# ------------------------------------------------------------------ positive box
PBOX_ROWS_SHAPE = (4, 70, 60, 8)                  # 16 800 rows against 4 * 4096 = 16 384 per pass of the grid
PBOX_ROWS_PER_PASS = 16384
PBOX_ROW = 16500                                  # the row of the only positive voxel
PBOX_TRIP_SHAPES = ((1, 3, 4, 520), (1, 3, 4, 203))
PBOX_DTYPES = ("int16", "int32", "float32")


@functools.lru_cache(maxsize=None)
def pbox_rows_volume(dtype: str) -> np.ndarray:
    """negatives everywhere in the first pass, one positive voxel in row PBOX_ROW"""
    x = np.zeros(PBOX_ROWS_SHAPE, np.dtype(dtype))
    flat = x.reshape(-1, PBOX_ROWS_SHAPE[-1])
    rng = np.random.default_rng(8)
    flat[rng.integers(0, PBOX_ROWS_PER_PASS, 300), rng.integers(0, 8, 300)] = -3
    flat[PBOX_ROW, 5] = 7
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def pbox_trip_volume(shape, dtype: str) -> np.ndarray:
    """positives only beyond the first trip (x >= 256 at V = 4, x >= 64 at V = 1), the last voxel of a row among
    them; negatives in the first trip"""
    c, d, h, w = shape
    step = 256 if w % 4 == 0 else 64
    x = np.zeros(shape, np.dtype(dtype))
    x[0, :, :, 3:step:7] = -1
    x[0, 1, 2, step + 44] = 1
    x[0, 2, 1, w - 1] = 5
    return _frozen(x)


# ====================================================================== nyul.hip
Q64 = np.linspace(0.0, 1.0, 64)
Q64.setflags(write=False)
Q64_REPEATED = np.repeat(np.linspace(0.0, 1.0, 16), 4)            # 64 quantiles, each four times: equal ranks
Q64_REPEATED.setflags(write=False)
Q3 = np.array([0.1, 0.5, 0.9])
Q11 = np.array([0.01] + [i / 10 for i in range(1, 10)] + [0.99])
# for the 2^24 case: with n - 1 = 2^24 - 6 or 2^24, tenths give whole ranks under either rule, eighths do not
Q_BIG = np.array([0.005, 0.01, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 0.99, 0.995])
WIDE_N, NARROW_N, MIXED_N = 20001, 5001, 20003
SEG3_LEN = 20000                                  # per segment of the three-segment call (vectorised)
ZERO_EVERY = 19                                   # every 19th value of an input is a zero, signs alternating
BIG_N = (1 << 24) + 3
BIG_ZEROS = {"below": 8, "above": 2}              # masked counts 2^24 - 5 and 2^24 + 1
MANY_SEGMENTS, MANY_LENS = 600, (41, 40)
MAP_SEGMENTS, MAP_LEN, MAP_L = 2100, 40, 5


def _with_zeros(v: np.ndarray) -> np.ndarray:
    v[::ZERO_EVERY] = 0.0
    v[::2 * ZERO_EVERY] = -0.0
    return _frozen(v.astype(np.float32))


def _wide(n: int, rng) -> np.ndarray:
    return (rng.choice(np.array([-1.0, 1.0]), n) * 2.0 ** rng.uniform(-40, 40, n)).astype(np.float32)


def _narrow(n: int, rng) -> np.ndarray:
    return rng.uniform(1.0, 1.25, n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def nyul_input(kind: str, n: int = 0) -> np.ndarray:
    """f32 [n], seed 1.  "wide": +-2^U(-40, 40), the ranks' order statistics spread over many top digits.
    "narrow": uniform in [1, 1.25), all under one top digit.  "mixed": two fifths wide, three fifths narrow, so some
    top digits hold one slot and one holds many.  "zero": zeros of both signs.  Every 19th value is a zero."""
    rng = np.random.default_rng(1)
    n = n or {"wide": WIDE_N, "narrow": NARROW_N, "mixed": MIXED_N}[kind]
    if kind == "wide":
        return _with_zeros(_wide(n, rng))
    if kind == "narrow":
        return _with_zeros(_narrow(n, rng))
    if kind == "mixed":
        v = np.concatenate([_wide(2 * n // 5, rng), _narrow(n - 2 * n // 5, rng)])
        return _with_zeros(rng.permutation(v))
    if kind == "zero":
        return _with_zeros(np.zeros(n, np.float32))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def nyul_three_segments() -> np.ndarray:
    """f32 [3, SEG3_LEN]: wide, narrow, all-zero (empty under nonzero)"""
    return _frozen(np.stack([nyul_input(k, SEG3_LEN) for k in ("wide", "narrow", "zero")]))


@functools.lru_cache(maxsize=None)
def _big_base() -> np.ndarray:
    rng = np.random.default_rng(24)
    x = np.exp2(rng.random(BIG_N, dtype=np.float32) * np.float32(40.0) - np.float32(20.0))
    x[1::2] *= np.float32(-1.0)                   # +-2^U(-20, 20): neighbouring order statistics lie tens of ulps apart
    x[: BIG_N // 4] = -1024.0                     # heavy constant background
    return _frozen(x)


def nyul_big(form: str) -> np.ndarray:
    """f32 [2^24 + 3] with BIG_ZEROS[form] zeros planted: longer than 2^24, masked count below or above it"""
    x = _big_base().copy()
    x[np.linspace(5, BIG_N - 7, BIG_ZEROS[form]).astype(np.int64)] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def nyul_many(seg_len: int) -> np.ndarray:
    """f32 [600, seg_len]: scaled normals, a zero column, one all-zero segment"""
    rng = np.random.default_rng(seg_len)
    x = (rng.standard_normal((MANY_SEGMENTS, seg_len)) * rng.uniform(1, 1e4, (MANY_SEGMENTS, 1))).astype(np.float32)
    x[:, 7] = 0.0
    x[333] = 0.0
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def nyul_map_many():
    """(x f32 [2100, 40], landmarks f32 [2100, 5] ascending per segment, scale f64 [5])"""
    rng = np.random.default_rng(2100)
    x = (rng.standard_normal((MAP_SEGMENTS, MAP_LEN)) * 50).astype(np.float32)
    x[:, 3] = 0.0
    lm = np.sort(rng.standard_normal((MAP_SEGMENTS, MAP_L)) * 40, axis=1).astype(np.float32)
    return _frozen(x, lm, np.linspace(-10.0, 90.0, MAP_L))


@functools.lru_cache(maxsize=None)
def nyul_map_64(pad_to_four: bool):
    """(x f32 [n], landmarks f32 [64] strictly ascending, scale f64 [64]).  x holds every landmark, each landmark
    one ulp down and up, values below the first and above the last landmark, +-inf, NaN and +-0; n % 4 == 0 when
    ``pad_to_four`` (the float4 map), else n % 4 == 1."""
    rng = np.random.default_rng(64)
    lm = np.unique((rng.standard_normal(200) * 500).astype(np.float32))[:64 * 3:3][:64]
    assert lm.size == 64
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    x = np.concatenate([lm, np.nextafter(lm, lo), np.nextafter(lm, hi),
                        np.array([lm[0] - 1, lm[0] - 1e6, lm[-1] + 1, lm[-1] + 1e6, np.inf, -np.inf, np.nan, 0.0, -0.0],
                                 np.float32)]).astype(np.float32)
    want = 0 if pad_to_four else 1
    while x.size % 4 != want:
        x = np.append(x, np.float32(12.5))
    return _frozen(rng.permutation(x), lm, np.linspace(0.0, 100.0, 64))


# the comparison rules of tests/test_nyul_gpu.py, unchanged (that module needs the device library to import)
def _same_value(a, b):
    """bit-equal, except that the sign of a zero may differ and NaN matches NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ok = (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))
    return bool(ok.all())


def _same_bits(a, b):
    """bit-equal, NaN payloads aside"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _ulps(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def f2key(v: np.ndarray) -> np.ndarray:
    """nyul.hip's order-preserving u32 key of f32 values: negatives flipped, the others with the sign bit set"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k: np.ndarray) -> np.ndarray:
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def masked(x: np.ndarray, nonzero: bool) -> np.ndarray:
    x = np.asarray(x, np.float32).reshape(-1)
    return x[x != 0] if nonzero else x


def rank_rule(q: float, n: int, limit: int, regime_n=None):
    """landmark_rank restated: (lo, hi, w) of quantile q among n masked values; torch's f32 rule when the regime
    count is at most `limit`, numpy's f64 rule above.  The regime count is n; a caller plants the fault "regime from
    the segment length" by passing the length as ``regime_n``."""
    if (n if regime_n is None else regime_n) <= limit:
        rank = np.float32(np.float32(q) * np.float32(n - 1))
        lo, hi = int(np.trunc(rank)), int(np.ceil(rank))
        return lo, hi, np.float32(rank - np.float32(lo))
    vi = float(q) * float(n - 1)
    lo = int(np.floor(vi))
    return lo, (lo if vi >= n - 1 else lo + 1), vi - lo


def all_ranks(q, n: int, limit: int) -> np.ndarray:
    """i64 [2 L]: lo and hi of every quantile, in the kernel's order"""
    return np.array([r for qq in q for r in rank_rule(qq, n, limit)[:2]], np.int64)


def landmarks_by_rule(m: np.ndarray, q, limit: int, regime_n=None) -> np.ndarray:
    """nyul_ref.landmarks with the rank rule (and the lerp that goes with it) chosen by ``regime_n``"""
    n = m.size
    rk = [rank_rule(qq, n, limit, regime_n) for qq in q]
    st = nyul_ref.order_stats(m, [r for lo, hi, _ in rk for r in (lo, hi)])
    f32 = (n if regime_n is None else regime_n) <= limit
    lerp = nyul_ref._lerp32 if f32 else nyul_ref._lerp64
    return np.array([lerp(st[lo], st[hi], w) for lo, hi, w in rk], np.float32)


PASSES = ((21, 11), (10, 11), (0, 10))            # (shift, bits) of the digit of passes A, B, C


def radix_select(m: np.ndarray, ranks: np.ndarray, slots_lds: int, fault=None) -> np.ndarray:
    """the multi-rank radix select restated: u32 keys of the order statistics of the masked values ``m`` at ``ranks``.
    Per pass, the distinct prefixes of the ranks are the slots (ascending); each slot gets the histogram of the next
    digit of the elements under its prefix, and every rank of the slot descends into the bin that holds it.
    fault "first_group_only": slots past the first ``slots_lds`` of a pass get no counts.
    fault "first_slot_of_digit": in pass C only the first slot of each top digit gets counts."""
    ks = np.sort(f2key(m)).astype(np.int64)
    prefix = np.zeros(ranks.size, np.int64)
    rem = np.asarray(ranks, np.int64).copy()
    width = 32
    for p, (shift, bits) in enumerate(PASSES):
        slots = np.unique(prefix)
        for j, pre in enumerate(slots.tolist()):
            under = ks[np.searchsorted(ks, pre):np.searchsorted(ks, pre + (1 << width) - 1, side="right")]
            hist = np.bincount((under >> shift) & ((1 << bits) - 1), minlength=1 << bits)
            if fault == "first_group_only" and p > 0 and j >= slots_lds:
                hist[:] = 0
            if fault == "first_slot_of_digit" and p == 2 and j > 0 and slots[j - 1] >> 21 == pre >> 21:
                hist[:] = 0
            cum = np.concatenate([[0], np.cumsum(hist)])
            for r in np.flatnonzero(prefix == pre):
                b = int(np.searchsorted(cum[:-1], rem[r], side="right")) - 1
                prefix[r] |= b << shift
                rem[r] -= cum[b]
        width = shift
    return prefix.astype(np.uint32)


def slot_counts(x: np.ndarray, q, nonzero: bool, limit: int) -> SimpleNamespace:
    """the slots that nyul.hip forms for one segment: ``b`` distinct pass-B prefixes (top 11 bits of the ranks' order
    statistics), ``c`` distinct pass-C prefixes (top 22 bits), ``per_digit`` the pass-C slots per top digit
    (ascending digits), ``first`` the index of each digit's first slot among the pass-C slots"""
    m = masked(x, nonzero)
    if m.size == 0:
        return SimpleNamespace(n=0, b=0, c=0, per_digit=np.zeros(0, np.int64), first=np.zeros(0, np.int64))
    keys = np.sort(f2key(m))[all_ranks(q, m.size, limit)]
    pc = np.unique(keys >> np.uint32(10))
    digits, first, per_digit = np.unique(pc >> np.uint32(11), return_index=True, return_counts=True)
    return SimpleNamespace(n=m.size, b=digits.size, c=pc.size, per_digit=per_digit, first=first)


def nyul_slot_report(L: SimpleNamespace) -> dict:
    """{(input, nonzero): (pass-B slots, pass-C slots, most pass-C slots under one top digit)} of the Q64 cases"""
    out = {}
    for kind in ("wide", "narrow", "mixed"):
        for nonzero in (False, True):
            s = slot_counts(nyul_input(kind), Q64, nonzero, L.kExactRankLimit)
            out[kind, nonzero] = (s.b, s.c, int(s.per_digit.max()))
    return out


# ====================================================================== the proof that every case crosses its limit
def crossings(L: SimpleNamespace) -> list:
    """one message per case that, with the limits ``L`` (read_limits), no longer crosses the limit its GPU test in
    tests/test_detect_limits_gpu.py or tests/test_nyul_limits_gpu.py is there for; empty when all of them do"""
    bad = list(L.missing)
    say = bad.append

    # ---- centroid sums: trips, the ragged tail, the misaligned view, the full label table, x0
    if not (CENT_V4_SHAPE[2] % 4 == 0 and trips(CENT_V4_SHAPE[2], 4) == 3 and CENT_V4_SHAPE[2] - 2 * LANES * 4 == 8):
        say(f"cent_volume({CENT_V4_SHAPE}): needs three trips of {LANES * 4} voxels at V = 4, the last with 8")
    if not (CENT_V1_SHAPE[2] % 4 != 0 and trips(CENT_V1_SHAPE[2], 1) == 4 and CENT_V1_SHAPE[2] % LANES != 0):
        say(f"cent_volume({CENT_V1_SHAPE}): needs four trips of {LANES} voxels at V = 1, the last ragged")
    for dtype in LABEL_DTYPES + ("float32",):
        if not misaligned(VIEW_OFFSET, np.dtype(dtype).itemsize):
            say(f"a view {VIEW_OFFSET} elements of {dtype} into a buffer is still aligned for V = 4")
    for shape in (CENT_V4_SHAPE, CENT_V1_SHAPE):
        lab = cent_volume(shape, "int16")
        v = 4 if shape[2] % 4 == 0 else 1
        per = distinct_per_chunk(lab, v)
        if not (per.max() >= 3 and set(np.unique(lab)) == set(range(CENT_K + 1)) - {CENT_K - 1}
                and np.unique(lab[..., (trips(shape[2], v) - 1) * LANES * v:]).size > 3):
            say(f"cent_volume({shape}): needs every label but {CENT_K - 1}, several per chunk and on the last trip")
    if CENT_DENSE_K != L.kLmMaxLabels:
        say(f"cent_dense(): k = {CENT_DENSE_K} against kLmMaxLabels = {L.kLmMaxLabels}; the case is the full label table")
    for dtype in LABEL_DTYPES:
        lab = cent_dense(dtype)
        per = distinct_per_chunk(lab, 4)
        if not (per.min() > 2 * LANES and int(lab.max()) == 255 and int(lab.min()) == 0):
            say(f"cent_dense({dtype}): {per.min()} distinct labels in a chunk; the case needs more than {2 * LANES} (no two "
                f"neighbouring lanes with one label) and the labels 0 and 255")
        late = cent_late(dtype)
        xs = np.nonzero(late == CENT_LATE_LABEL)[2]
        if not (xs.size > 100 and xs.min() >= CENT_LATE_FROM >= LANES * 4 and xs.max() >= 2 * LANES * 4):
            say(f"cent_late({dtype}): label {CENT_LATE_LABEL} must lie only at x >= {CENT_LATE_FROM} (past the first trip) "
                f"and reach the third")

    # ---- heatmap: supports across the trip boundary, the full table and the per-channel grid cap, a covered volume
    lab = hm_trip_volume()
    sup = {c: hm_support(lab, c) for c in HM_TRIP_BLOCKS}
    step = LANES * 4
    if not (HM_TRIP_SHAPE[2] % 4 == 0 and trips(HM_TRIP_SHAPE[2], 4) == 3
            and sum(s[0][0] < step <= s[0][1] for s in sup.values()) >= 4
            and {detect_ref.centre(lab, c)[0] for c in HM_TRIP_BLOCKS} >= {250, 255, 256, 262, 500, 515}
            and any(s[0][0] < 2 * step <= s[0][1] for s in sup.values())):
        say(f"hm_trip_volume(): needs centres at x = 250, 255, 256, 262, 500, 515 and supports over x = {step} and {2 * step}")
    lab = hm_big_volume()
    rows = HM_BIG_SHAPE[0] * HM_BIG_SHAPE[1]
    g = lm_grid(rows, HM_BIG_K + 1, L.kLmMaxWgs)
    if not (HM_BIG_K == L.kLmMaxLabels and g == 16 and cdiv(rows, ROWS_PER_WG * g) >= 3 and trips(HM_BIG_SHAPE[2], 4) == 2):
        say(f"hm_big_volume(): k = {HM_BIG_K}, {g} workgroups per channel for {rows} rows; the case needs k = "
            f"kLmMaxLabels, the cap of 16 and three passes of it")
    if not (detect_ref.tail_of(255) == 108 and 2 * detect_ref.tail_of(255) + 1 == HM_STRIDE
            and detect_ref.sigma32(255) == 27.0 and all(s[2] for s in hm_support(lab, 255))
            and sorted(np.unique(lab).tolist()) == [0, 1, 128, 255]):
        say(f"hm_big_volume(): label 255 needs sigma 27, tail 108 (stride {HM_STRIDE}) clipped on every axis")
    lab = hm_cover_volume()
    if not all(lo == 0 and hi == n - 1 for (lo, hi, _), n in zip(hm_support(lab, 255), HM_COVER_SHAPE[::-1])):
        say("hm_cover_volume(): the support of label 255 no longer covers the volume")
    k255 = detect_ref.kernel_f64(255)
    ratio = np.prod([min(k255[108 + lo - c], k255[108 + hi - c]) / k255[108]
                     for (lo, hi, _), c in zip(hm_support(lab, 255), detect_ref.centre(lab, 255))])
    if not 0.0 < ratio <= HM_COVER_MAX_RATIO:
        say(f"hm_cover_volume(): min P / max P = {ratio:.3f}; it must be positive (the subtraction does something) and at "
            f"most {HM_COVER_MAX_RATIO} (f32 can hold the rescaled channel to 1e-6 gamma)")

    # ---- channel argmax: maxima past the first trip, ties across it, the one-workgroup grid, NaN past it
    for shape in AM_SHAPES:
        x = am_volume(shape)
        v = 4 if shape[3] % 4 == 0 else 1
        step = LANES * v
        val, xyz = argmax_points(x)
        at = [np.argwhere(x[c] == val[c]) for c in range(3)]          # (z, y, x) in linear order
        tied = at[1][np.argsort(at[1][:, 2])] if len(at[1]) == 3 else np.zeros((3, 3), np.int64)
        if not (trips(shape[3], v) >= 3 and xyz[0, 0] >= step and len(at[0]) == 1
                and (tied[:, 2] // step).tolist() == [0, 1, 2]
                and tied[0, 2] % step // v == tied[1, 2] % step // v      # one lane, a trip apart
                and tuple(tied[0]) > tuple(tied[1])                       # the smaller x comes later in [z, y, x] order
                and xyz[1].tolist() == tied[0][::-1].tolist()
                and len(at[2]) > 100):
            say(f"am_volume({shape}): needs a maximum past x = {step}, and one tied in the same lane of two trips with the "
                f"later x first in [z, y, x] order")
    many = am_many()
    g = lm_grid(AM_MANY_SHAPE[1] * AM_MANY_SHAPE[2], AM_MANY_SHAPE[0], L.kLmMaxWgs)
    if not (AM_MANY_SHAPE[0] > L.kLmMaxWgs and g == 1 and AM_MANY_SHAPE[0] <= 65535
            and np.unique(argmax_points(many)[1], axis=0).shape[0] == 2 * 3 * 5):
        say(f"am_many(): {AM_MANY_SHAPE[0]} channels against kLmMaxWgs = {L.kLmMaxWgs}; the case needs more channels than "
            f"workgroups (one workgroup per channel) and maxima at every position")
    nan_at = np.argwhere(np.isnan(am_nan_volume()))
    if not (len(nan_at) == 1 and nan_at[0][0] == 1 and nan_at[0][3] >= LANES * 4):
        say("am_nan_volume(): needs one NaN, in channel 1 at x >= 256")

    # ---- positive box: a second pass of the capped grid, far faces from later trips
    rows = int(np.prod(PBOX_ROWS_SHAPE[:3]))
    per_pass = ROWS_PER_WG * lm_grid(rows, 1, L.kLmMaxWgs)
    for dtype in PBOX_DTYPES:
        x = pbox_rows_volume(dtype)
        r = np.nonzero((x > 0).reshape(rows, -1))[0]
        if not (per_pass == PBOX_ROWS_PER_PASS < rows and r.tolist() == [PBOX_ROW] and PBOX_ROW >= per_pass
                and (x < 0).sum() > 100):
            say(f"pbox_rows_volume({dtype}): {rows} rows, {per_pass} per pass; the only positive voxel must lie in a row "
                f"at or above {PBOX_ROWS_PER_PASS}")
        for shape in PBOX_TRIP_SHAPES:
            x = pbox_trip_volume(shape, dtype)
            v = 4 if shape[3] % 4 == 0 else 1
            xs = np.nonzero(x > 0)[3]
            if not (xs.size == 2 and xs.min() >= LANES * v and xs.max() == shape[3] - 1
                    and xs.max() // (LANES * v) == trips(shape[3], v) - 1 >= 2 and (x < 0).any()):
                say(f"pbox_trip_volume({shape}, {dtype}): positives must lie beyond the first trip and in the last")

    # ---- Nyul: the landmark limit, slot groups, the walk under one top digit
    S = L.kSlotsLds
    if not (Q64.size == Q64_REPEATED.size == L.kNyulMaxLandmarks == 64 and 2 * Q64.size == 128
            and cdiv(2 * Q64.size, S) == 8 and L.kNyulBins == 2048 and L.kHistThreads == 1024):
        say(f"Q64: {Q64.size} landmarks against kNyulMaxLandmarks = {L.kNyulMaxLandmarks}, kSlotsLds = {S}; the cases "
            f"need 128 ranks in 8 slot groups")
    if not (np.all(np.diff(Q64_REPEATED) >= 0) and np.unique(Q64_REPEATED).size == 16):
        say("Q64_REPEATED: needs 16 distinct quantiles, four times each, ascending")
    lim = L.kExactRankLimit
    for nonzero in (False, True):
        s = slot_counts(nyul_input("wide"), Q64, nonzero, lim)
        if not s.b > 4 * S:
            say(f"nyul_input('wide'), nonzero={nonzero}: {s.b} pass-B slots; the case needs more than 4 kSlotsLds = {4 * S}")
        s = slot_counts(nyul_input("narrow"), Q64, nonzero, lim)
        if not (s.per_digit.max() > 2 * S and s.first[np.argmax(s.per_digit)] < S):
            say(f"nyul_input('narrow'), nonzero={nonzero}: {s.per_digit.max()} pass-C slots under one top digit; the case "
                f"needs more than 2 kSlotsLds = {2 * S}, the first of them in group 0")
        s = slot_counts(nyul_input("mixed"), Q64, nonzero, lim)
        many = np.argmax(s.per_digit)
        if not ((s.per_digit == 1).sum() >= 3 and s.per_digit[many] > S and s.first[many] >= S and s.b > S):
            say(f"nyul_input('mixed'), nonzero={nonzero}: pass-C slots per top digit {s.per_digit.tolist()}; the case needs "
                f"three digits with one slot, one with more than kSlotsLds = {S} that starts past group 0, and more than "
                f"{S} pass-B slots")
    segs = nyul_three_segments()
    if not (SEG3_LEN % 4 == 0 and slot_counts(segs[0], Q64, True, lim).b > 4 * S
            and slot_counts(segs[1], Q64, True, lim).per_digit.max() > 2 * S
            and masked(segs[2], True).size == 0 and slot_counts(segs[2], Q64, False, lim).c <= 2):
        say("nyul_three_segments(): needs a wide, a narrow and an all-zero segment of a length that is a multiple of 4")
    for kind in ("wide", "narrow", "mixed"):
        x = nyul_input(kind)
        if not (x.size % 4 != 0 and 0 < (x == 0).sum() < x.size // 10 and np.signbit(x[x == 0]).any()):
            say(f"nyul_input({kind!r}): needs a length that is no multiple of 4 and some zeros of both signs")
    s = slot_counts(nyul_input("wide"), Q64_REPEATED, False, lim)
    r = all_ranks(Q64_REPEATED, WIDE_N, lim)
    if not (r.size == 128 and np.unique(r).size <= 32 and s.c > S):
        say("Q64_REPEATED on nyul_input('wide'): needs 128 ranks, at most 32 of them distinct, in more than kSlotsLds "
            "pass-C slots")

    # ---- Nyul: the regime follows the masked count
    for form, n_want in (("below", (1 << 24) - 5), ("above", (1 << 24) + 1)):
        n = BIG_N - BIG_ZEROS[form]
        if not (BIG_N > lim and n == n_want and (n <= lim) == (form == "below")):
            say(f"nyul_big({form!r}): length {BIG_N}, masked count {n}, kExactRankLimit = {lim}; the segment must be longer "
                f"than the limit with its masked count {form} it")
    # ---- Nyul: segment counts
    if not (MANY_SEGMENTS > L.pass_a_per_chip and MANY_SEGMENTS > L.pass_bc_per_chip and MANY_LENS[0] % 4 != 0
            and MANY_LENS[1] % 4 == 0):
        say(f"nyul_many(): {MANY_SEGMENTS} segments against {L.pass_a_per_chip} workgroups of pass A; the case needs more "
            f"segments than that, one length vectorised and one not")
    if not (MAP_SEGMENTS > L.map_per_chip and MAP_LEN % 4 == 0):
        say(f"nyul_map_many(): {MAP_SEGMENTS} segments against {L.map_per_chip} workgroups of the map")
    # ---- Nyul: the map at 64 landmarks
    for pad in (True, False):
        x, lm, scale = nyul_map_64(pad)
        if not (lm.size == L.kNyulMaxLandmarks == scale.size and np.all(np.diff(lm) > 0) and np.isin(lm, x).all()
                and np.isin(np.nextafter(lm, np.float32(np.inf)), x).all()
                and np.isin(np.nextafter(lm, np.float32(-np.inf)), x).all()
                and (x[np.isfinite(x)] < lm[0]).sum() >= 3 and (x[np.isfinite(x)] > lm[-1]).sum() >= 3
                and np.isinf(x).sum() == 2 and np.isnan(x).sum() == 1 and (x == 0).sum() == 2
                and np.signbit(x[x == 0]).sum() == 1 and (x.size % 4 == 0) == pad):
            say(f"nyul_map_64({pad}): needs 64 ascending landmarks, each with its two neighbours, both outsides, +-inf, "
                f"NaN and +-0")
    return bad
