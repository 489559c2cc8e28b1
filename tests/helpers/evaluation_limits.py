"""Inputs that drive the evaluation kernels of ``segmantic_amd/csrc/distance.hip`` (label boxes, EDT, sampler, radix
select, confusion counts) past their grid caps, their tables and the 2^24 end of the exact float32 range, and the
arithmetic that proves it.  The pattern is that of ``tests/helpers/labelvol_limits.py``.

:func:`read_limits` reads the named constants as text and carries the bare literals as named numbers together with
the function and the text each must still stand in.  The generators have FIXED sizes, written out as numbers: one
that followed a changed constant would hide the change.  :func:`crossings` recomputes, from the inputs alone, every
quantity that has to cross a limit and returns one message per generator that no longer does;
``tests/test_evaluation_limits_host.py`` asserts that the list is empty.

Everything here is numpy on the host; cached results are read-only."""
from __future__ import annotations

import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

CSRC = Path(__file__).resolve().parents[2] / "segmantic_amd" / "csrc"
SOURCE = "distance.hip"

NAMED = ("kBoxMaxLabels", "kSampleWgs", "kSelectWgs", "kSelectBins", "kSelectMaxRanks")
TICKETS = ("kFinTickets", "reduce_fin.h")        # the ticket counters that the sampler's tail shares with reduce_fin.h
FILES = (SOURCE, TICKETS[1])
# the bare literals: name -> (the entry point it stands in, the text that must be there, the numbers read out of it)
LITERALS = {
    "boxes_grid": ("segmi_label_boxes", "lv_grid(rows, 4, 1024)", {"boxes_rows_per_wg": 4, "boxes_grid_cap": 1024}),
    "sample_grid": ("segmi_edt_sample", "lv_grid(rows, 4, kSampleWgs)", {"sample_rows_per_wg": 4}),
    "confusion_grid": ("segmi_confusion_counts", "lv_grid(n, 256, 1024)",
                       {"confusion_per_wg": 256, "confusion_grid_cap": 1024}),
    "confusion_lds": ("segmi_confusion_counts", "if (k <= 64) hipLaunchKernelGGL(confusion_lds_kernel<T>",
                      {"confusion_lds_k": 64}),
    "confusion_max": ("segmi_confusion_counts", "k > 0 && k <= 4096", {"confusion_max_k": 4096}),
}
LABEL_TYPES = ("uint8", "int16", "int32")


def cdiv(a: int, b: int) -> int:
    return -(-int(a) // int(b))


def _entry(text: str, name: str) -> str:
    """the text of the extern "C" function ``name``: from its head to the first closing brace in column 0"""
    m = re.search(r"^int(?:64_t)? %s\(" % name, text, re.M)
    if m is None:
        return ""
    return text[m.start():text.index("\n}\n", m.start())]


def read_limits(csrc: Path = CSRC) -> SimpleNamespace:
    """the limits of ``distance.hip`` under ``csrc``; ``missing`` lists the literal lines that are no longer there"""
    text = (Path(csrc) / SOURCE).read_text()
    out = {}
    for name, src in [(n, text) for n in NAMED] + [(TICKETS[0], (Path(csrc) / TICKETS[1]).read_text())]:
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
        if m is None:
            raise AssertionError(f"{FILES} no longer define `constexpr int {name} = <integer>;`")
        out[name] = int(m.group(1))
    missing = []
    for key, (entry, line, numbers) in LITERALS.items():
        out.update(numbers)
        if line not in _entry(text, entry):
            missing.append(f"{SOURCE}: {entry} no longer holds `{line}`: the numbers {numbers} of "
                           f"tests/helpers/evaluation_limits.py describe a launch that has changed")
    return SimpleNamespace(missing=missing, **out)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def out_of_range(dtype: str, k: int):
    """label values of ``dtype`` that ops.label_boxes / confusion_counts with ``k`` labels must skip"""
    info = np.iinfo(dtype)
    vals = [v for v in (k, k + 1, info.max) if v <= info.max]
    if info.min < 0:
        vals += [-1, -2, info.min]
    return vals


# ------------------------------------------------------------------ label boxes
BOX_WIDTHS = (1, 63, 64, 65, 130)                 # one lane, chunk - 1, one chunk, chunk + 1, more than two chunks
BOX_CHUNK = 64                                    # lanes of a wave = voxels of a chunk of boxes_kernel
BOX_K = 6
BOX_RUN = (60, 71)                                # x range of the run of label 5: both sides of x = 64
BOX_TRIP_SHAPE = (66, 63, 70)                     # 4158 rows > 4 x 1024
BOX_ROWS_PER_TRIP = 4 * 1024
BOX_TABLE_KS = ((1, "uint8"), (255, "uint8"), (1024, "int16"), (1024, "int32"))


@functools.lru_cache(maxsize=None)
def box_width_volume(w: int, dtype: str, ndim: int = 3):
    """(pred, truth) of shape (3, 5, w) or (5, w) for k = BOX_K: labels 0 .. 2 in both, 3 in pred only, 4 in truth
    only, values >= k and (signed types) negative ones sprinkled in; label 5 is absent unless w > BOX_RUN[1], where
    it is one run over x = 60 .. 70 of one row of pred"""
    shape = (3, 5, w)[3 - ndim:]
    rng = np.random.default_rng(w * 8 + np.dtype(dtype).itemsize + ndim)
    skip = out_of_range(dtype, BOX_K)
    out = []
    for absent in (4, 3):
        a = rng.integers(0, 5, shape)
        a[a == absent] = 0
        junk = rng.random(shape) < 0.15
        a[junk] = rng.choice(skip, int(junk.sum()))
        out.append(a.astype(dtype))
    pred, truth = out
    if w >= BOX_RUN[1]:
        row = (1, 2) if ndim == 3 else (2,)
        pred[row] = 0
        pred[row + (slice(*BOX_RUN),)] = 5
    return _frozen(pred, truth)


@functools.lru_cache(maxsize=None)
def box_trip_volume(dtype: str):
    """(pred, truth, k = 4) of BOX_TRIP_SHAPE: label 1 spread over every row, label 2 only in rows that the second
    trip of the capped grid reads (row = z * h + y >= BOX_ROWS_PER_TRIP), label 3 absent"""
    d, h, w = BOX_TRIP_SHAPE
    rng = np.random.default_rng(66)
    out = []
    for _ in range(2):
        a = (rng.random((d * h, w)) < 0.2).astype(dtype)
        late = rng.choice(np.arange(BOX_ROWS_PER_TRIP, d * h), 7, replace=False)
        a[late, rng.integers(0, w, 7)] = 2
        out.append(a.reshape(d, h, w))
    out[0].reshape(d * h, w)[d * h - 1, w - 1] = 2          # the last lane of the last row
    return _frozen(*out) + (4,)


@functools.lru_cache(maxsize=None)
def box_table_volume(k: int, dtype: str):
    """(pred, truth): every label 0 .. k-1 on exactly one voxel of each (so every entry of the LDS table is touched
    once per volume), the other voxels out of range; shape (2, n, 11)"""
    rng = np.random.default_rng(k + np.dtype(dtype).itemsize)
    total = cdiv(k + 9, 22) * 22
    skip = out_of_range(dtype, k)
    out = []
    for _ in range(2):
        a = np.concatenate([np.arange(k), rng.choice(skip, total - k)])
        out.append(rng.permutation(a).astype(dtype).reshape(2, total // 22, 11))
    return _frozen(*out)


# ------------------------------------------------------------------ EDT
EXACT_F32 = 2 ** 24                               # integers up to here are float32 values
LONG = 6000
LONG_SHAPES = ((6000, 3), (3, 6000), (6000, 2, 3))        # the long axis is P2's, P3's, P1's
LONG_FEATURES = ((0, 0, 0), (7, 11, 2), (19, 1, 0))       # clipped to the shape (2-D: the first two entries)
ANISO_CASES = (((23, 31, 70), (2.0, 0.8, 0.5)), ((23, 31, 70), (0.7, 1.0, 1.9)), ((1, 600, 3), (1.0, 0.3, 7.0)))
CUT_SHAPE = (20, 22, 24)
CUT_BLOCK = (4, 15, 6, 17, 3, 20)                 # where the label lives in the first volume
CUT_BOX = (6, 12, 8, 14, 5, 16)                   # strictly inside the block: all six faces cut through the label
BORDER_BOX = (0, 12, 8, 22, 5, 24)                # second volume: three faces on the volume's border, three cut
THIN_BOXES = ((6, 7, 8, 14, 5, 16), (6, 12, 8, 9, 5, 16), (6, 12, 8, 14, 5, 6))


def long_points(shape):
    nd = len(shape)
    return sorted({tuple(min(c, n - 1) for c, n in zip(f[:nd], shape)) for f in LONG_FEATURES})


@functools.lru_cache(maxsize=None)
def long_volume(shape):
    lab = np.zeros(shape, np.uint8)
    for p in long_points(shape):
        lab[p] = 1
    return _frozen(lab)


def long_extremes(shape):
    """(smallest, largest) over the voxels of the squared distance to the nearest of long_points: integers"""
    idx = np.indices(shape).reshape(len(shape), -1).T.astype(np.int64)
    best = np.min([((idx - np.asarray(p)) ** 2).sum(1) for p in long_points(shape)], axis=0)
    return int(best.min()), int(best.max())


@functools.lru_cache(maxsize=None)
def aniso_volume(shape):
    """int16 label 5: sparse single voxels, one solid block with an interior, label 2 as a bystander"""
    rng = np.random.default_rng(shape[1])
    lab = np.zeros(shape, np.int16)
    lab[rng.random(shape) < 0.004] = 5
    lab[rng.random(shape) < 0.01] = 2
    d, h, w = shape
    lab[d // 3:d // 3 + 4, h // 2:h // 2 + 5, 1:9] = 5
    return _frozen(lab)


@functools.lru_cache(maxsize=None)
def cut_volume(kind: str):
    """int32 label 2 at density 0.7: "block" inside CUT_BLOCK only, "border" over the whole volume"""
    rng = np.random.default_rng(len(kind))
    lab = np.zeros(CUT_SHAPE, np.int32)
    if kind == "block":
        b = CUT_BLOCK
        lab[b[0]:b[1], b[2]:b[3], b[4]:b[5]] = (rng.random((b[1] - b[0], b[3] - b[2], b[5] - b[4])) < 0.7) * 2
    else:
        lab[...] = (rng.random(CUT_SHAPE) < 0.7) * 2
    return _frozen(lab)


# ------------------------------------------------------------------ sampler
SAMPLE_WIDTHS = (5, 64, 70, 130)
SAMPLE_TRIP_SHAPE = (66, 63, 5)                   # 4158 rows > 4 x kSampleWgs
SAMPLE_ROWS_PER_TRIP = 4 * 1024
SAMPLE_TICKETS = 2048                             # kFinTickets of reduce_fin.h: launches until a ticket comes round


@functools.lru_cache(maxsize=None)
def sample_case(bw: int, dtype: str, ndim: int = 3):
    """(target, query, label, box): label 3 at density 0.5 in both volumes of shape (6, 7, bw + 4) (2-D: (7, bw + 4));
    the box leaves a margin of one voxel (two along x) on every side, and the query volume holds the label on
    every voxel just outside each face of the box"""
    shape = (6, 7, bw + 4)[3 - ndim:]
    rng = np.random.default_rng(bw + ndim)
    tgt = ((rng.random(shape) < 0.5) * 3).astype(dtype)
    qry = ((rng.random(shape) < 0.8) * 3).astype(dtype)
    box = (1, 5, 1, 6, 2, 2 + bw) if ndim == 3 else (0, 1, 1, 6, 2, 2 + bw)
    q3 = qry.reshape((1,) * (3 - ndim) + shape)
    if ndim == 3:
        q3[0, 1:6, 2:2 + bw] = 3
        q3[5, 1:6, 2:2 + bw] = 3
    q3[box[0]:box[1], 0, 2:2 + bw] = 3
    q3[box[0]:box[1], 6, 2:2 + bw] = 3
    q3[box[0]:box[1], 1:6, 1] = 3
    q3[box[0]:box[1], 1:6, 2 + bw] = 3
    return _frozen(tgt, qry) + (3, box)


@functools.lru_cache(maxsize=None)
def sample_trip_case():
    """(target, query, label 1, the whole volume as box) of SAMPLE_TRIP_SHAPE: the target is the voxel (0, 0, 0), the
    query one voxel on every seventh row and the far corner, so that the largest distance is read in the second
    trip of the capped grid"""
    d, h, w = SAMPLE_TRIP_SHAPE
    tgt = np.zeros(SAMPLE_TRIP_SHAPE, np.uint8)
    tgt[0, 0, 0] = 1
    qry = np.zeros((d * h, w), np.uint8)
    rows = np.arange(0, d * h, 7)
    qry[rows, rows % w] = 1
    qry[d * h - 1, w - 1] = 1
    return _frozen(tgt, qry.reshape(d, h, w)) + (1, (0, d, 0, h, 0, w))


# ------------------------------------------------------------------ select
SELECT_SIZES = (1, 2, 131072, 131073)             # around kSelectWgs * 256: the second is one more stride
SELECT_TOP11 = 0x1FC                              # bits 31..21 of 1.0f


def select_bits(kind: str, n: int = 5000) -> np.ndarray:
    """float32 [n] built from bit patterns: "middle" share bits 31..21 and 9..0 and differ in 20..10 (the second
    pass decides), "low" share bits 31..10 (the third decides), "any" are arbitrary finite non-negative patterns,
    subnormals and zero included"""
    rng = np.random.default_rng(n + len(kind))
    if kind == "middle":
        u = (SELECT_TOP11 << 21) | (rng.integers(0, 2048, n) << 10) | 0x155
    elif kind == "low":
        u = (SELECT_TOP11 << 21) | (0x2AB << 10) | rng.integers(0, 1024, n)
    else:
        u = rng.integers(0, 0x7F800000, n)
        u[rng.random(n) < 0.05] >>= 9             # subnormals and small patterns
        u[rng.random(n) < 0.02] = 0
    return _frozen(u.astype(np.uint32).view(np.float32))


# ------------------------------------------------------------------ confusion counts
CONF_KS = ((64, "uint8"), (65, "int16"), (4096, "int32"))
CONF_N = 300_000
CONF_TRIP = 1024 * 256                            # elements of one trip of the capped grid
CONF_TRIP_N = CONF_TRIP + 1000
CONF_TRIP_K = 40


def confusion_case(k: int, dtype: str, n: int = CONF_N):
    """(pred, truth) of n labels 0 .. k-1, 70 % agreeing, the corner cells (0, 0), (k-1, k-1), (0, k-1), (k-1, 0) hit"""
    rng = np.random.default_rng(k)
    t = rng.integers(0, k, n)
    p = np.where(rng.random(n) < 0.7, t, rng.integers(0, k, n))
    t[:4], p[:4] = (0, k - 1, 0, k - 1), (0, k - 1, k - 1, 0)
    return _frozen(p.astype(dtype), t.astype(dtype))


def confusion_trip_case(dtype: str):
    """(pred, truth, k): labels 0 .. 19 in the first CONF_TRIP elements, 20 .. 39 in the tail behind them"""
    rng = np.random.default_rng(7)
    lo = rng.integers(0, 20, (2, CONF_TRIP))
    hi = rng.integers(20, CONF_TRIP_K, (2, CONF_TRIP_N - CONF_TRIP))
    both = np.concatenate([lo, hi], 1).astype(dtype)
    return _frozen(both[0], both[1]) + (CONF_TRIP_K,)


# ------------------------------------------------------------------ the proof that every generator crosses its limit
def crossings(L: SimpleNamespace) -> list:
    """one message per generator that, with the limits ``L`` (read_limits), no longer crosses the limit its GPU test
    in tests/test_evaluation_ops_gpu.py is there for; empty when all of them do"""
    bad = list(L.missing)
    # label boxes: grid trips and the LDS table
    per_trip = L.boxes_rows_per_wg * L.boxes_grid_cap
    rows = BOX_TRIP_SHAPE[0] * BOX_TRIP_SHAPE[1]
    if not (per_trip == BOX_ROWS_PER_TRIP and per_trip < rows <= 2 * per_trip):
        bad.append(f"box_trip_volume(): {rows} rows against {per_trip} per trip of boxes_kernel's grid "
                   f"(boxes_grid_cap = {L.boxes_grid_cap}); label 2 was laid out for a second trip from row {BOX_ROWS_PER_TRIP}")
    top = max(k for k, _ in BOX_TABLE_KS)
    if top != L.kBoxMaxLabels:
        bad.append(f"box_table_volume(): the largest table has {top} labels, kBoxMaxLabels = {L.kBoxMaxLabels}")
    c = BOX_CHUNK
    if not ({1, c - 1, c, c + 1} <= set(BOX_WIDTHS) and max(BOX_WIDTHS) > 2 * c and BOX_RUN[0] < c < BOX_RUN[1] - 1):
        bad.append(f"box_width_volume(): widths {BOX_WIDTHS} and the run {BOX_RUN} against chunks of {c} voxels")
    # sampler: grid trips
    per_trip = L.sample_rows_per_wg * L.kSampleWgs
    rows = SAMPLE_TRIP_SHAPE[0] * SAMPLE_TRIP_SHAPE[1]
    if not (per_trip == SAMPLE_ROWS_PER_TRIP and per_trip < rows <= 2 * per_trip):
        bad.append(f"sample_trip_case(): {rows} rows against {per_trip} per trip of sample_kernel's grid "
                   f"(kSampleWgs = {L.kSampleWgs}); the maximum was placed in a second trip from row {SAMPLE_ROWS_PER_TRIP}")
    if L.kFinTickets != SAMPLE_TICKETS:
        bad.append(f"sampler ticket test: laid out for {SAMPLE_TICKETS} tickets, kFinTickets = {L.kFinTickets}; it must "
                   f"draw every ticket twice")
    # EDT: beyond the exact float32 integers, with exact values in the same volume
    for shape in LONG_SHAPES:
        lo, hi = long_extremes(shape)
        if not (lo == 0 and hi > 2 * EXACT_F32 and max(shape) == LONG):
            bad.append(f"long_volume({shape}): squared distances {lo} .. {hi} must pass 2^25")
    # select: one stride of the histogram grid
    stride = L.kSelectWgs * 256
    if not (SELECT_SIZES[2] == stride and SELECT_SIZES[3] == stride + 1):
        bad.append(f"select sizes {SELECT_SIZES} against one stride of kSelectWgs * 256 = {stride} values")
    if L.kSelectBins != 2048:
        bad.append(f"select_bits(): patterns laid out for 11-bit digits (21 / 10 / 0), kSelectBins = {L.kSelectBins}")
    if L.kSelectMaxRanks != 4:
        bad.append(f"select tests ask for 1 .. 4 ranks and expect 5 to be refused, kSelectMaxRanks = {L.kSelectMaxRanks}")
    # confusion counts: the LDS switch, the largest table and a second trip
    ks = [k for k, _ in CONF_KS]
    if ks != [L.confusion_lds_k, L.confusion_lds_k + 1, L.confusion_max_k]:
        bad.append(f"confusion_case(): k in {ks} against the LDS switch at {L.confusion_lds_k} and the cap {L.confusion_max_k}")
    per_trip = L.confusion_per_wg * L.confusion_grid_cap
    if not (per_trip == CONF_TRIP and CONF_TRIP < CONF_TRIP_N <= 2 * CONF_TRIP and CONF_TRIP_K <= L.confusion_lds_k):
        bad.append(f"confusion_trip_case(): {CONF_TRIP_N} elements against {per_trip} per trip of the grid "
                   f"(confusion_grid_cap = {L.confusion_grid_cap}); the tail's labels start at element {CONF_TRIP}")
    return bad
