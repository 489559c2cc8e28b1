"""Inputs whose sums are EXACT, for the row reductions and the BatchNorm passes of ``segmantic_amd/csrc/norm_act.hip``
and the two finalisations behind them (``collapse_fin_kernel`` of ``reduce_fin.h``, ``fin_tail_run`` of ``fin_tail.h``),
with the float64 references of those operations and the arithmetic that says which code path every case takes.

The principle: small integers and dyadic parameters.  Every term, every f32 partial row and every float64 column sum
is then exactly representable in whatever order it is added, so the device has to return the reference's numbers bit
for bit, and one skipped or doubled voxel or row shows.  That is a PRECONDITION, not an assumption:
``tests/test_reduce_fin_host.py`` asserts, on the CPU, for every case, that each reference output survives the cast to
its storage type and back, and that every row-sized sum of |terms| stays below 2^24 units of the terms' grid.

The sizes are written out as numbers, with the path each was built for next to them.  :func:`read_limits` reads the
constants the paths depend on from the sources as text; :func:`collapse_path`, :func:`tail_path`, :func:`stats_path`
and :func:`ew_path` restate the launchers' arithmetic, and the host test asserts that no case has drifted off the path
recorded for it and that every path of :data:`PATHS` still has a case.

Everything here is numpy on the host; results are read-only."""
from __future__ import annotations

import functools
import math
import re
from pathlib import Path
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

CSRC = Path(__file__).resolve().parents[2] / "segmantic_amd" / "csrc"

# name -> file of the `constexpr int kName = <integer>;` definitions
NAMED = {"kFinBlocks": "reduce_fin.h", "kFinLdsWidth": "reduce_fin.h", "kEwCap": "norm_act.hip"}
# the bare literals: name -> (file, the text its line must hold, the numbers read out of that text)
LITERALS = {
    "fin_blocks": ("reduce_fin.h", "if ((int64_t)rows * width <= 65536) return 1;", {"one_wg_floats": 65536}),
    "fin_blocks_rows": ("reduce_fin.h", "int b = rows / 8;", {"rows_per_wg": 8}),
    "scratch_rows": ("reduce_fin.h", "constexpr int kFinScratchRows = kFinBlocks + 1;", {}),
    "reserve": ("norm_act.hip", "constexpr int kReserveRows = 2 * kFinScratchRows + 1;", {}),
    "stat_want": ("norm_act.hip", "const int want = c <= 16 ? 1024 : 512;", {"want_narrow": 1024, "want_wide": 512}),
    "stat_max": ("norm_act.hip", "int v = 4096;", {"vox_max": 4096}),
    "stat_min": ("norm_act.hip", "while (v > 64 && nvox / v < want) v >>= 1;", {"vox_min": 64}),
    "stat_table": ("norm_act.hip", "while (v < 4096 && cdiv64(nvox, v) * 3 * c > 65536) v <<= 1;", {}),
    "bwd_channels": ("norm_act.hip", "bn_act_bwd_reduce: at most 256 channels per call", {"bwd_max_c": 256}),
}
NT = 256                 # threads of every workgroup that reduces or finalises here
ALPHA = 0.25             # the PReLU slope of every case
DROP_P, DROP_SEED = 0.5, 0xC0FFEE
F32, BF16, F16 = "float32", "bfloat16", "float16"
ALL = (F32, BF16, F16)


def cdiv(a: int, b: int) -> int:
    return -(-int(a) // int(b))


def read_limits(csrc: Path = CSRC) -> SimpleNamespace:
    """the limits of the sources under ``csrc``; ``missing`` lists the literal lines that are no longer there"""
    csrc = Path(csrc)
    text = {f: (csrc / f).read_text() for f in {*NAMED.values(), *(v[0] for v in LITERALS.values())}}
    out = {}
    for name, f in NAMED.items():
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text[f])
        if m is None:
            raise AssertionError(f"{f} no longer defines `constexpr int {name} = <integer>;`")
        out[name] = int(m.group(1))
    missing = []
    for key, (f, line, numbers) in LITERALS.items():
        out.update(numbers)
        if line not in text[f]:
            missing.append(f"{f} no longer holds `{line}`: the numbers {numbers or key} of tests/helpers/reduce_cases.py "
                           f"describe a launch that has changed")
    out["reserve_rows"] = 2 * (out["kFinBlocks"] + 1) + 1
    return SimpleNamespace(missing=missing, **out)


# ------------------------------------------------------------------ restatements of the launchers' arithmetic
def fin_blocks(rows: int, width: int, L) -> int:
    """workgroups of collapse_fin_kernel (reduce_fin.h fin_blocks)"""
    if rows * width <= L.one_wg_floats:
        return 1
    return max(1, min(L.kFinBlocks, rows // L.rows_per_wg))


def stat_vox(nvox: int, c: int, L) -> int:
    """voxels per partial row of bn_stats / bn_act_bwd_reduce (norm_act.hip stat_vox)"""
    want = L.want_narrow if c <= 16 else L.want_wide
    v = L.vox_max
    while v > L.vox_min and nvox // v < want:
        v >>= 1
    while v < L.vox_max and cdiv(nvox, v) * 3 * c > L.one_wg_floats:
        v <<= 1
    return v


def _loop(n: int, unroll: int):
    """(trips of the unrolled loop, rows left to the loop after it) of a thread that owns n rows"""
    return n // unroll, n % unroll


def collapse_path(rows: int, width: int, aligned: bool, L) -> dict:
    """what collapse_fin_kernel does with a [rows][width] table: workgroups, column path, where the column sums live,
    and the loops of the thread that owns row 0 (it owns the most rows)"""
    nblk = fin_blocks(rows, width, L)
    vec = width % 4 == 0 and width // 4 <= NT and aligned
    p = {"nblk": nblk, "vec": vec, "lds": width <= L.kFinLdsWidth, "floats": rows * width}
    if vec:
        rl = NT // (width // 4)
        step = nblk * rl
        n0 = cdiv(rows, step)
        p.update(passes=1, row_lanes=rl, unrolled=_loop(n0, 8)[0], tail=_loop(n0, 8)[1], few_rows=rows < rl)
    else:
        wl = min(width, NT)
        rl = NT // wl
        step = nblk * rl
        n0 = cdiv(rows, step)
        t16, rest = _loop(n0, 16)
        p.update(passes=cdiv(width, wl), last_pass=width - (cdiv(width, wl) - 1) * wl, row_lanes=rl, unrolled16=t16,
                 unrolled4=rest // 4, tail=rest % 4, few_rows=rows < rl)
    return p


def collapse_tags(p: dict) -> set:
    t = {"collapse:one-workgroup" if p["nblk"] == 1 else "collapse:ticket",
         "collapse:lds-sums" if p["lds"] else "collapse:scratch-sums"}
    if p["vec"]:
        t.add("collapse:vec")
        if p["unrolled"]:
            t.add("collapse:vec-unrolled8")
        if p["tail"]:
            t.add("collapse:vec-tail")
        if p["unrolled"] and p["nblk"] > 1:
            t.add("collapse:vec-unrolled8-ticket")
    else:
        t.add("collapse:scalar")
        if p["unrolled16"]:
            t.add("collapse:scalar-unrolled16")
        if p["unrolled4"]:
            t.add("collapse:scalar-unrolled4")
        if p["tail"]:
            t.add("collapse:scalar-tail")
        if p["passes"] > 1:
            t.add("collapse:w0-passes")
    if p["few_rows"]:
        t.add("collapse:fewer-rows-than-lanes")
    return t


def tail_path(rows: int, width: int, L, threads: int = NT) -> dict:
    """what fin_tail_run does with the [rows][width] table of its launch (16-byte aligned: the tables are
    allocations of their own)"""
    vec = width % 4 == 0 and width // 4 <= threads
    if vec:
        rl = threads // (width // 4)
        n0 = cdiv(rows, rl)
        return {"vec": True, "passes": 1, "row_lanes": rl, "unrolled": n0 // 16, "tail": n0 % 16}
    wl = min(width, threads)
    rl = threads // wl
    n0 = cdiv(rows, rl)
    return {"vec": False, "passes": cdiv(width, wl), "row_lanes": rl, "unrolled": n0 // 8, "tail": n0 % 8}


def tail_tags(p: dict) -> set:
    k = "tail:vec" if p["vec"] else "tail:scalar"
    t = {k}
    if p["unrolled"]:
        t.add(k + "-unrolled")
    if p["tail"]:
        t.add(k + "-remainder")
    if p["passes"] > 1:
        t.add("tail:w0-passes")
    if p["row_lanes"] == 1:
        t.add("tail:one-row-lane")
    return t


def vec4_ok(c: int, ld: int, ch0: int, elem_size: int) -> bool:
    """norm_act.hip vec4_ok of a view that starts ch0 elements into a buffer the allocator aligned"""
    return c % 4 == 0 and ld % 4 == 0 and (ch0 * elem_size) % (4 * elem_size) == 0


def stats_path(case, elem_size: int, L) -> dict:
    """kernel and rows of bn_stats / bn_act_bwd_reduce for a case"""
    nvox = case.sp[0] * case.sp[1] * case.sp[2]
    v4 = vec4_ok(case.c, case.buf_c, case.ch0, elem_size)
    if v4 and case.c // 4 <= NT:
        kernel, lanes = "T4", NT // (case.c // 4)
    elif case.c <= NT:
        kernel, lanes = "T1", NT // case.c
    else:
        kernel, lanes = "wide", 1
    vpw = stat_vox(nvox, case.c, L)
    rows = cdiv(nvox, vpw)
    return {"kernel": kernel, "vpw": vpw, "rows": rows, "last": nvox - (rows - 1) * vpw, "voxel_lanes": lanes}


def ew_path(nvox: int, c: int, v4: bool, L) -> dict:
    """grid of an element-wise pass (grid_1d under kEwCap) and the passes of its grid-stride loop"""
    items = nvox * (c // 4 if v4 else c)
    grid = max(1, min(L.kEwCap, cdiv(items, NT)))
    return {"items": items, "grid": grid, "passes": cdiv(items, grid * NT), "last_pass": items - (cdiv(items, grid * NT) - 1) * grid * NT}


# ------------------------------------------------------------------ storage types on the host
def roundtrip(a: np.ndarray, dtype: str) -> np.ndarray:
    """float64 -> storage type (round to nearest even) -> float64"""
    a = np.asarray(a, np.float64)
    if dtype == F32:
        return a.astype(np.float32).astype(np.float64)
    if dtype == F16:
        return a.astype(np.float16).astype(np.float64)
    f = a.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), a), "bf16 round trip of a value that is not an f32"
    b = f.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def drop_mask(numel: int, p: float, seed: int) -> np.ndarray:
    """numpy restatement of norm_act.hip drop_mult (keep -> 1/(1-p), drop -> 0) over element indices."""
    e = np.arange(numel, dtype=np.uint64)
    h = ((e & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF
    h ^= np.uint64(seed)
    h ^= ((e >> np.uint64(32)) * 0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> np.uint64(16); h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> np.uint64(15); h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> np.uint64(16)
    keep = (h >> np.uint64(8)) >= np.uint64(int(np.float32(p) * np.float32(16777216.0)))
    return keep.astype(np.float32) / (1.0 - p)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------ part 1: synthetic partial tables
class TableCase(NamedTuple):
    name: str
    rows: int           # real rows (the callers add the reserve)
    width: int
    aligned: bool
    seed: int
    nblk: int           # workgroups the case was built for
    tags: tuple         # paths the case was built for


TABLES = (
    TableCase("5x32", 5, 32, True, 101, 1, ("collapse:one-workgroup", "collapse:vec", "collapse:fewer-rows-than-lanes")),
    # 16-byte columns of width 32: 8 column lanes, rl4 = 32 row lanes; 8 rl4 + 3 rows: lanes 0..2 own 9 rows
    TableCase("259x32", 259, 32, True, 102, 1, ("collapse:vec-unrolled8", "collapse:vec-tail")),
    TableCase("513x128", 513, 128, True, 103, 64, ("collapse:ticket", "collapse:vec")),
    TableCase("2049x32", 2049, 32, True, 104, 64, ("collapse:ticket", "collapse:vec", "collapse:vec-tail")),
    TableCase("100x768", 100, 768, True, 105, 12, ("collapse:ticket", "collapse:vec")),
    TableCase("7x6", 7, 6, True, 106, 1, ("collapse:scalar", "collapse:fewer-rows-than-lanes")),
    TableCase("40x9", 40, 9, True, 107, 1, ("collapse:scalar", "collapse:scalar-tail")),
    TableCase("1000x66", 1000, 66, True, 108, 64, ("collapse:scalar", "collapse:ticket", "collapse:scalar-unrolled4")),
    TableCase("70x1200", 70, 1200, True, 109, 8, ("collapse:scalar", "collapse:w0-passes", "collapse:ticket")),
    TableCase("20x4100", 20, 4100, True, 110, 2, ("collapse:scratch-sums", "collapse:ticket")),
    TableCase("600x4100", 600, 4100, True, 111, 64, ("collapse:scratch-sums", "collapse:ticket")),
    TableCase("2049x32-misaligned", 2049, 32, False, 112, 64, ("collapse:scalar", "collapse:ticket")),
    # beyond the issue's list: the scalar path's 16-way loop (one workgroup, 3 row lanes, 103 rows for lane 0:
    # six 16-row trips, one 4-row trip, then 3 single rows), the 16-byte path's 8-way loop under a ticket, and the benchmark's table
    TableCase("307x66", 307, 66, True, 113, 1, ("collapse:scalar-unrolled16", "collapse:scalar-unrolled4", "collapse:scalar-tail")),
    TableCase("600x768", 600, 768, True, 114, 64, ("collapse:vec-unrolled8-ticket", "collapse:vec-tail")),
    TableCase("4096x48", 4096, 48, True, 115, 64, ("collapse:ticket", "collapse:vec")),
)
TABLE_BY_NAME = {t.name: t for t in TABLES}
TABLE_MAG = 2 ** 20
TABLE_COUNT = 3 * 2 ** 20      # the `count` of the finalisations: no power of two, so the quotients round


@functools.lru_cache(maxsize=None)
def table(name: str) -> np.ndarray:
    """f32 [rows, width], integers in [-2^20, 2^20].  For the BatchNorm reading [rows][2][c] of the table the second
    half (the sums of squares) is made non-negative, except in channel 1, where it is negated: that channel's
    variance is negative before the clamp."""
    t = TABLE_BY_NAME[name]
    rng = np.random.default_rng(t.seed)
    a = rng.integers(-TABLE_MAG, TABLE_MAG + 1, (t.rows, t.width)).astype(np.float32)
    if t.width % 2 == 0:
        c = t.width // 2
        a[:, c:] = np.abs(a[:, c:])
        if c > 1:
            a[:, c + 1] = -a[:, c + 1]
    return _ro(a)


COUNT1_TABLE = (5, 32, 131)


@functools.lru_cache(maxsize=None)
def count1_table() -> np.ndarray:
    """f32 [5, 32] for count == 1, where the mean is the sum itself: sums in [-3, 3] per row and squares up to 2^20,
    so that the variance is positive (and the unbiased factor count / (count - 1), which must be skipped, would show);
    channel 1 negated as in table()"""
    rows, width, seed = COUNT1_TABLE
    rng = np.random.default_rng(seed)
    c = width // 2
    a = np.concatenate([rng.integers(-3, 4, (rows, c)), rng.integers(2 ** 10, TABLE_MAG + 1, (rows, c))], 1)
    a = a.astype(np.float32)
    a[:, c + 1] = -a[:, c + 1]
    return _ro(a)


def table_sums(a: np.ndarray) -> np.ndarray:
    """float64 column sums; exact for the integer tables (|sum| <= 4096 * 2^20 = 2^32)"""
    return a.astype(np.float64).sum(0)


def bn_params(c: int, seed: int):
    """(gamma, beta, running_mean, running_var) f32 [c]: ordinary values, not dyadic (the outputs they enter are
    held to a bound, not to equality)"""
    rng = np.random.default_rng(seed)
    g = (1 + 0.3 * rng.standard_normal(c)).astype(np.float32)
    b = (0.2 * rng.standard_normal(c)).astype(np.float32)
    rm = rng.standard_normal(c).astype(np.float32)
    rv = (0.5 + rng.random(c)).astype(np.float32)
    return _ro(g, b, rm, rv)


U32 = 2.0 ** -24         # half an f32 ulp, relative
E64 = 2.0 ** -53


def bn_finalize_ref(sums: np.ndarray, c: int, count: float, gamma, beta, rm, rv, momentum: float, eps: float) -> dict:
    """float64 restatement of fin_tail.h BnFin on exact column sums [2c], with the bound of every output.

    `mean` is ONE rounded operation on exact sums, the f32 cast of the float64 quotient: bound 0, compared with ==.
    The others take several operations, which the compiler may contract into FMAs, so each is held to a bound counted
    from its operations (u = 2^-24, e = 2^-53, every f32 / f64 operation rounds by at most u / e of its result):
      var     = q - m m with q = S2 / count, m = S1 / count: the two quotients, the product and the difference (or
                one FMA) change it by at most dvar = 4 e (|q| + m^2); the clamp at 0 is monotone.
      invstd  = f32(1 / sqrt(var + eps)): monotone in var, so it lies between f(var + dvar) and f(var - dvar), widened
                by the add, the root, the division (3 e) and the cast (u).
      scale   = gamma (x) invstd: one more f32 rounding.
      shift   = beta - f32(m) (x) scale: the product and the difference (or one FMA): 2 u of |beta| + |m scale|, plus
                |m| times the bound of scale.
      running = (1 - momentum) (x) r + momentum (x) v: the difference 1 - momentum, two products and a sum: 4 u of
                |(1 - momentum) r| + |momentum v| (5 u taken); for the variance v = f32(unbiased var) adds one cast
                (6 u taken) and momentum times the spread of var.  count == 1 skips the unbiased factor."""
    s = np.asarray(sums, np.float64)
    g, b, rm, rv = (np.asarray(a, np.float64) for a in (gamma, beta, rm, rv))
    mom, eps = float(np.float32(momentum)), float(np.float32(eps))
    m, qq = s[:c] / count, s[c:] / count
    var = qq - m * m
    dvar = 4 * E64 * (np.abs(qq) + m * m)
    f = lambda v: 1.0 / np.sqrt(np.maximum(v, 0.0) + eps)
    inv, lo, hi = f(var), f(var + dvar), f(var - dvar)
    inv_b = (hi - lo) + hi * (U32 + 4 * E64)
    m32 = m.astype(np.float32).astype(np.float64)
    scale = g * inv
    scale_b = np.abs(g) * inv_b + U32 * np.abs(g) * hi
    shift = b - m32 * scale
    shift_b = np.abs(m32) * scale_b + 2 * U32 * (np.abs(b) + np.abs(m32) * (np.abs(scale) + scale_b))
    k = count / (count - 1.0) if count > 1.0 else 1.0
    unb, unb_lo, unb_hi = (np.maximum(v, 0.0) * k for v in (var, var - dvar, var + dvar))
    run_m = (1 - mom) * rm + mom * m32
    run_m_b = 5 * U32 * (np.abs((1 - mom) * rm) + np.abs(mom * m32))
    run_v = (1 - mom) * rv + mom * unb
    run_v_b = 6 * U32 * (np.abs((1 - mom) * rv) + np.abs(mom * unb_hi)) + mom * (unb_hi - unb_lo)
    return {"mean": (m.astype(np.float32), None), "invstd": (inv, inv_b), "scale": (scale, scale_b),
            "shift": (shift, shift_b), "running_mean": (run_m, run_m_b), "running_var": (run_v, run_v_b),
            "var": var, "dvar": dvar}


def bn_bwd_finalize_ref(sums: np.ndarray, c: int, count: float) -> dict:
    """fin_tail.h BnBwdFin on exact column sums [3c]: every output is the f32 cast of a float64 sum or quotient of
    exact sums (the channel sum behind dalpha is exact too: integers below 2^53), so all of them compare with =="""
    s = np.asarray(sums, np.float64)
    return {"dbeta": s[:c].astype(np.float32), "dgamma": s[c:2 * c].astype(np.float32),
            "dalpha": np.float32(s[2 * c:3 * c].sum()),
            "coef": np.concatenate([s[:c] / count, s[c:2 * c] / count]).astype(np.float32).reshape(2, c)}


# the table that is NOT integer-valued: random f32 rows against math.fsum
FSUM_TABLE = ("513x128-random", 513, 128, 121)


@functools.lru_cache(maxsize=None)
def fsum_table():
    """(f32 [513, 128] of normal deviates over six decades, math.fsum of every column as float64, sum |v| per column)"""
    _, rows, width, seed = FSUM_TABLE
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((rows, width)) * 10.0 ** rng.uniform(-3, 3, (rows, width))).astype(np.float32)
    d = a.astype(np.float64)
    want = np.array([math.fsum(d[:, j].tolist()) for j in range(width)])
    return _ro(a, want, np.abs(d).sum(0))


# ------------------------------------------------------------------ parts 2 and 3: activations
class ActCase(NamedTuple):
    name: str
    c: int
    sp: tuple           # (d, h, w); n = 1
    buf_c: int          # channels of the buffer the case is a view of (== c: dense)
    ch0: int            # first channel of the view
    dtypes: tuple
    seed: int
    want: dict          # the path it was built for: stats_path() entries (per storage type where they differ)


def _w(kernel, vpw, rows, last, lanes):
    return {"kernel": kernel, "vpw": vpw, "rows": rows, "last": last, "voxel_lanes": lanes}


STATS_CASES = (
    # 585 voxels, rows of 64: one and two channel groups, 256 and 128 voxel lanes against 64-voxel rows
    ActCase("c4", 4, (5, 9, 13), 4, 0, ALL, 201, _w("T4", 64, 10, 9, 256)),
    ActCase("c8", 8, (5, 9, 13), 8, 0, ALL, 202, _w("T4", 64, 10, 9, 128)),
    ActCase("c16-ragged", 16, (37, 41, 43), 16, 0, ALL, 203, _w("T4", 64, 1020, 15, 64)),
    ActCase("c64", 64, (24, 32, 36), 64, 0, ALL, 204, _w("T4", 128, 216, 128, 16)),
    ActCase("c256", 256, (5, 8, 64), 256, 0, ALL, 205, _w("T4", 64, 40, 64, 4)),
    ActCase("c512", 512, (4, 5, 9), 512, 0, ALL, 206, _w("T4", 64, 3, 52, 2)),
    # 300 channels are 75 groups of four: still <T,4>; only a misaligned view of them takes the wide kernel
    ActCase("c300", 300, (3, 5, 7), 300, 0, ALL, 207, _w("T4", 64, 2, 41, 3)),
    ActCase("c300-misaligned", 300, (3, 5, 7), 304, 1, ALL, 208, _w("wide", 64, 2, 41, 1)),
    ActCase("c1028", 1028, (3, 4, 5), 1028, 0, ALL, 209, _w("wide", 64, 1, 60, 1)),
    ActCase("c3", 3, (5, 6, 7), 3, 0, ALL, 210, _w("T1", 64, 4, 18, 85)),
    ActCase("c16-view48", 16, (5, 9, 13), 48, 8, ALL, 211, _w("T4", 64, 10, 9, 64)),
    ActCase("c16-misaligned", 16, (5, 9, 13), 20, 1, (F32,), 212, _w("T1", 64, 10, 9, 16)),
)
# the bias gradient folds in the statistics launch up to 256 channels and in a launch of its own beyond
BIAS_TAIL_MAX_C = 256

REDUCE_CASES = (
    ActCase("c16-375rows", 16, (30, 40, 20), 16, 0, ALL, 301, _w("T4", 64, 375, 64, 64)),
    ActCase("c256", 256, (5, 8, 64), 256, 0, ALL, 302, _w("T4", 64, 40, 64, 4)),
    ActCase("c255", 255, (3, 7, 11), 255, 0, ALL, 303, _w("T1", 64, 4, 39, 1)),
    ActCase("c130", 130, (5, 9, 13), 130, 0, ALL, 304, _w("T1", 64, 10, 9, 1)),
    ActCase("c3", 3, (5, 6, 7), 3, 0, ALL, 305, _w("T1", 64, 4, 18, 85)),
    ActCase("c32-ragged", 32, (33, 47, 65), 32, 0, ALL, 306, _w("T4", 256, 394, 207, 32)),
    ActCase("c16-view48", 16, (5, 9, 13), 48, 8, ALL, 307, _w("T4", 64, 10, 9, 64)),
)
# fin_tail_run of the reduce launch, per case: (vector columns, unrolled trips, remainder, passes)
REDUCE_TAIL_WANT = {
    "c16-375rows": {"vec": True, "passes": 1, "row_lanes": 21, "unrolled": 1, "tail": 2},
    "c256": {"vec": True, "passes": 1, "row_lanes": 1, "unrolled": 2, "tail": 8},
    "c255": {"vec": False, "passes": 3, "row_lanes": 1, "unrolled": 0, "tail": 4},
    "c130": {"vec": False, "passes": 2, "row_lanes": 1, "unrolled": 1, "tail": 2},
    "c3": {"vec": False, "passes": 1, "row_lanes": 28, "unrolled": 0, "tail": 1},
    "c32-ragged": {"vec": True, "passes": 1, "row_lanes": 10, "unrolled": 2, "tail": 8},
    "c16-view48": {"vec": True, "passes": 1, "row_lanes": 21, "unrolled": 0, "tail": 1},
}
REDUCE_REFUSED_C = 257
MODES = ("prelu", "plain", "dropout")       # slope 0.25 / no activation / dropout 0.5 in front of the slope
# only shapes that test_bn_backward_as_one_launch_matches_the_three_calls launches: (c, spatial, n)
FUSED_CASES = ((48, (5, 6, 7), 2, 401), (64, (16, 16, 16), 8, 402))

EW_BIG = ActCase("c16-two-passes", 16, (70, 64, 64), 16, 0, ALL, 501, {})
EW_BIG_WANT = {"items": 1146880, "grid": 4096, "passes": 2, "last_pass": 98304}
EW_VIEWS = (ActCase("c16-view48", 16, (5, 9, 13), 48, 8, ALL, 502, {}),
            ActCase("c16-misaligned", 16, (5, 9, 13), 20, 1, (F32,), 503, {}),
            ActCase("c3", 3, (5, 6, 7), 3, 0, ALL, 504, {}))
EVAL_AFFINE_C = (3, 300)

PATHS = (
    "collapse:one-workgroup", "collapse:ticket", "collapse:vec", "collapse:scalar", "collapse:lds-sums",
    "collapse:scratch-sums", "collapse:vec-unrolled8", "collapse:vec-unrolled8-ticket", "collapse:vec-tail",
    "collapse:scalar-unrolled16", "collapse:scalar-unrolled4", "collapse:scalar-tail", "collapse:w0-passes",
    "collapse:fewer-rows-than-lanes",
    "tail:vec", "tail:vec-unrolled", "tail:vec-remainder", "tail:scalar", "tail:scalar-unrolled",
    "tail:scalar-remainder", "tail:w0-passes", "tail:one-row-lane",
    "stats:T4", "stats:T1", "stats:wide", "stats:ragged-last-row", "stats:more-lanes-than-voxels", "stats:strided",
    "stats:vpw-64", "stats:vpw-128", "stats:vpw-256", "bias:in-launch", "bias:separate-fold",
    "ew:second-pass", "ew:strided", "ew:scalar",
)


def nvox(case) -> int:
    return case.sp[0] * case.sp[1] * case.sp[2]


def stats_tags(case, p: dict) -> set:
    t = {"stats:" + p["kernel"], "stats:vpw-%d" % p["vpw"]}
    if p["last"] != p["vpw"]:
        t.add("stats:ragged-last-row")
    if p["voxel_lanes"] > p["vpw"]:
        t.add("stats:more-lanes-than-voxels")
    if case.buf_c != case.c:
        t.add("stats:strided")
    return t


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def act_inputs(seed: int, n_vox: int, c: int):
    """x in [-8, 8] and dy in [-4, 4], integers, f32 [n_vox, c]; mean in [-2, 2], invstd in {0.5, 1}, gamma in
    {2, -1}, beta in [-3, 3], f32 [c]"""
    rng = np.random.default_rng(seed)
    d = SimpleNamespace(
        x=_ints(rng, -8, 8, (n_vox, c)), dy=_ints(rng, -4, 4, (n_vox, c)), mean=_ints(rng, -2, 2, c),
        invstd=rng.choice(np.float32([0.5, 1.0]), c), gamma=rng.choice(np.float32([2.0, -1.0]), c),
        beta=_ints(rng, -3, 3, c))
    _ro(*vars(d).values())
    return d


@functools.lru_cache(maxsize=None)
def ew_inputs(seed: int, n_vox: int, c: int):
    """what the element-wise passes take beyond act_inputs: scale in {2, -0.5}, integer shift and residual in
    [-3, 3], coef rows of multiples of 0.5 in [-1, 1] and of 0.25 in [-0.5, 0.5]"""
    rng = np.random.default_rng(seed + 7919)
    d = SimpleNamespace(
        scale=rng.choice(np.float32([2.0, -0.5]), c), shift=_ints(rng, -3, 3, c), res=_ints(rng, -3, 3, (n_vox, c)),
        coef=np.stack([_ints(rng, -2, 2, c) * np.float32(0.5), _ints(rng, -2, 2, c) * np.float32(0.25)]))
    _ro(*vars(d).values())
    return d


def mode_args(mode: str, n_vox: int, c: int):
    """(slope or None, dropout mask f64 [n_vox, c] or None, the dropout argument of the ops)"""
    if mode == "plain":
        return None, None, (0.0, 0)
    if mode == "prelu":
        return ALPHA, None, (0.0, 0)
    return ALPHA, drop_mask(n_vox * c, DROP_P, DROP_SEED).reshape(n_vox, c).astype(np.float64), (DROP_P, DROP_SEED)


def stats_terms(x: np.ndarray):
    """(x, x^2) in float64; grids (1, 1)"""
    x = x.astype(np.float64)
    return (x, x * x), (1.0, 1.0)


def bwd_terms(d, alpha: Optional[float], mask):
    """the three terms of bn_act_bwd_reduce per element, float64 [n_vox, c], and their grids:
    xhat = (x - mean) invstd, z = (xhat gamma + beta) m, dz = (z <= 0 ? alpha dy : dy) m:
    dz, dz xhat, dy z [z <= 0] (the last only with a slope)"""
    x, dy = d.x.astype(np.float64), d.dy.astype(np.float64)
    m = 1.0 if mask is None else mask
    xh = (x - d.mean.astype(np.float64)) * d.invstd.astype(np.float64)
    z = (xh * d.gamma.astype(np.float64) + d.beta.astype(np.float64)) * m
    if alpha is None:
        dz, t2 = dy * m, np.zeros_like(dy)
    else:
        neg = ~(z > 0)
        dz, t2 = np.where(neg, alpha * dy, dy) * m, np.where(neg, dy * z, 0.0)
    return (dz, dz * xh, t2), (0.25, 0.125, 0.5)


def fwd_ref(x, scale, shift, alpha, mask, res):
    """y = prelu((x scale + shift) m) + r in float64; scale / shift None: identity"""
    z = x.astype(np.float64)
    if scale is not None:
        z = z * scale.astype(np.float64) + shift.astype(np.float64)
    if mask is not None:
        z = z * mask
    if alpha is not None:
        z = np.where(z > 0, z, alpha * z)
    return z if res is None else z + res.astype(np.float64)


def dx_ref(d, coef, alpha, mask):
    """dx = gamma invstd (dz - c0 - xhat c1) in float64"""
    (dz, _, _), _ = bwd_terms(d, alpha, mask)
    xh = (d.x.astype(np.float64) - d.mean.astype(np.float64)) * d.invstd.astype(np.float64)
    c = coef.astype(np.float64)
    return d.gamma.astype(np.float64) * d.invstd.astype(np.float64) * (dz - c[0] - xh * c[1])


def dx_f32_ref(d, coef32, alpha, mask, real=np.float64):
    """dx for a coef that is NOT dyadic (the f32 quotients of real sums), as f32 values in float64: the operations of
    common.h bn_bwd_apply_elem, which is compiled without contraction, with its two roundings where they fall:
    t = f32(dz - c0), then f32(fma(-xhat, c1, t)); xhat, dz and the factor gamma invstd (a signed power of two) are
    exact.  Both float64 steps are exact before they are rounded (a 5-bit xhat times a 24-bit c1, and sums of values
    between 2^-45 and 2^4), which the host test confirms by repeating them in a wider type (`real`)."""
    (dz, _, _), _ = bwd_terms(d, alpha, mask)
    xh = (d.x.astype(np.float64) - d.mean.astype(np.float64)) * d.invstd.astype(np.float64)
    c = np.asarray(coef32, np.float32).astype(real)
    t = (dz.astype(real) - c[0]).astype(np.float32).astype(real)
    f = (-xh.astype(real) * c[1] + t).astype(np.float32).astype(real)
    return (d.gamma.astype(real) * d.invstd.astype(real)) * f


def row_sum_bound(terms, grids, vpw: int) -> float:
    """the largest sum of |term| over one partial row of `vpw` voxels, in units of the term's grid: below 2^24, every
    f32 partial sum of the row is exact in any order"""
    worst = 0.0
    for t, g in zip(terms, grids):
        a = np.abs(t)
        pad = (-a.shape[0]) % vpw
        if pad:
            a = np.concatenate([a, np.zeros((pad, a.shape[1]))])
        worst = max(worst, float(a.reshape(-1, vpw, a.shape[1]).sum(1).max()) / g)
    return worst


def on_grid(a: np.ndarray, grid: float) -> bool:
    q = np.asarray(a, np.float64) / grid
    return bool(np.array_equal(q, np.round(q)))


def eval_affine_ref(gamma, beta, rm, rv, eps: float):
    """bn_eval_affine in float64 with the bound of its f32 operations (u = 2^-24): invstd = 1 / sqrtf(rv + eps)
    is an add (u, halved by the root), a root (within 1 ulp = 2 u) and a division (within 2.5 ulp = 5 u): 7.5 u;
    scale = gamma invstd adds u: 9 u taken; shift = beta - rm scale: |rm| times the bound of scale, the product and
    the difference (or one FMA): 2 u of |beta| + |rm scale|"""
    g, b, rm, rv = (np.asarray(a, np.float64) for a in (gamma, beta, rm, rv))
    inv = 1.0 / np.sqrt(rv + float(np.float32(eps)))
    scale = g * inv
    scale_b = 9 * U32 * np.abs(scale)
    shift = b - rm * scale
    shift_b = np.abs(rm) * scale_b + 2 * U32 * (np.abs(b) + np.abs(rm * scale) + np.abs(rm) * scale_b)
    return (scale, scale_b), (shift, shift_b)
