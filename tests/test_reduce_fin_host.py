"""The preconditions of tests/test_reduce_fin_gpu.py, checked on the CPU: the generators of
tests/helpers/reduce_cases.py give inputs whose references are exact in every storage type and whose partial sums are
exact in f32 in any order, and every case still takes the code path it was built for.  If a generator ever breaks
one of these, THIS test fails; the equalities of the GPU test are not to be loosened instead."""
import numpy as np
import pytest

from tests.helpers import reduce_cases as rc

L = rc.read_limits()
ELEM = {rc.F32: 4, rc.BF16: 2, rc.F16: 2}


def test_the_literals_the_cases_were_computed_from_still_stand():
    assert L.missing == []
    assert (L.kFinBlocks, L.kFinLdsWidth, L.kEwCap, L.one_wg_floats, L.reserve_rows) == (64, 4096, 4096, 65536, 131)


@pytest.mark.parametrize("t", rc.TABLES, ids=lambda t: t.name)
def test_table_cases_stay_on_their_collapse_path(t):
    p = rc.collapse_path(t.rows, t.width, t.aligned, L)
    assert p["nblk"] == t.nblk, p
    tags = rc.collapse_tags(p)
    assert set(t.tags) <= tags, (sorted(set(t.tags) - tags), p)
    a = rc.table(t.name)
    assert a.dtype == np.float32 and not a.flags.writeable
    assert np.array_equal(a, np.round(a)) and float(np.abs(a).max()) <= rc.TABLE_MAG
    assert a.min() < -rc.TABLE_MAG // 2 and a.max() > rc.TABLE_MAG // 2            # both signs, the full magnitude
    # exact in float64 in any order: the sum of magnitudes stays below 2^53
    assert float(np.abs(a.astype(np.float64)).sum(0).max()) < 2.0 ** 53
    if t.width % 2 == 0 and t.width > 2:      # the channel whose variance is negative before the clamp, and one that is not
        c = t.width // 2
        r = rc.bn_finalize_ref(rc.table_sums(a), c, rc.TABLE_COUNT, *rc.bn_params(c, t.seed), 0.1, 1e-5)
        assert r["var"][1] + r["dvar"][1] < 0 and (r["var"] - r["dvar"] > 0).any()


def test_the_issues_table_sizes():
    """the sizes the cases were asked for, as floats and workgroups"""
    want = {"5x32": (160, 1), "513x128": (65664, 64), "2049x32": (65568, 64), "100x768": (76800, 12),
            "1000x66": (66000, 64), "70x1200": (84000, 8), "20x4100": (82000, 2), "600x4100": (2460000, 64),
            "2049x32-misaligned": (65568, 64)}
    for name, (floats, nblk) in want.items():
        t = rc.TABLE_BY_NAME[name]
        p = rc.collapse_path(t.rows, t.width, t.aligned, L)
        assert (p["floats"], p["nblk"]) == (floats, nblk), name
    p = rc.collapse_path(70, 1200, True, L)
    assert not p["vec"] and (p["passes"], p["last_pass"]) == (5, 176)
    p = rc.collapse_path(2049, 32, False, L)
    assert not p["vec"] and rc.collapse_path(2049, 32, True, L)["vec"]
    p = rc.collapse_path(259, 32, True, L)
    assert (p["row_lanes"], p["unrolled"], p["tail"]) == (32, 1, 1) and 259 == 8 * p["row_lanes"] + 3
    assert not rc.collapse_path(20, 4100, True, L)["lds"] and rc.collapse_path(70, 1200, True, L)["lds"]
    # a cap of 32 workgroups leaves every case on a ticket: the results do not depend on the partition
    assert rc.fin_blocks(4096, 48, L) == 64


def test_the_random_table_is_not_integer_valued():
    a, want, mag = rc.fsum_table()
    assert a.dtype == np.float32 and not np.array_equal(a, np.round(a))
    assert rc.collapse_path(a.shape[0], a.shape[1], True, L)["nblk"] == 64
    assert np.all(np.abs(want) <= mag)


@pytest.mark.parametrize("case", rc.STATS_CASES + rc.REDUCE_CASES, ids=lambda c: c.name)
def test_activation_cases_stay_on_their_path(case):
    for dt in case.dtypes:
        assert rc.stats_path(case, ELEM[dt], L) == case.want, dt
    assert case.ch0 + case.c <= case.buf_c
    if case.name == "c16-view48":         # 16 bytes into the buffer for the 16-bit types
        assert case.ch0 * ELEM[rc.BF16] == 16


def test_reduce_cases_stay_on_their_tail_path():
    for case in rc.REDUCE_CASES:
        assert case.c <= L.bwd_max_c < rc.REDUCE_REFUSED_C
        assert rc.tail_path(case.want["rows"], 3 * case.c, L) == rc.REDUCE_TAIL_WANT[case.name], case.name


def test_every_listed_path_has_a_case():
    have = set()
    for t in rc.TABLES:
        have |= rc.collapse_tags(rc.collapse_path(t.rows, t.width, t.aligned, L))
    for case in rc.REDUCE_CASES:
        have |= rc.tail_tags(rc.tail_path(case.want["rows"], 3 * case.c, L))
        for dt in case.dtypes:
            have |= rc.stats_tags(case, rc.stats_path(case, ELEM[dt], L))
    for case in rc.STATS_CASES:
        for dt in case.dtypes:
            p = rc.stats_path(case, ELEM[dt], L)
            have |= rc.stats_tags(case, p)
            have.add("bias:in-launch" if case.c <= rc.BIAS_TAIL_MAX_C else "bias:separate-fold")
            if case.c <= rc.BIAS_TAIL_MAX_C:      # the bias gradient's tail over the [rows][2c] table
                have |= rc.tail_tags(rc.tail_path(p["rows"], 2 * case.c, L))
    big = rc.ew_path(rc.nvox(rc.EW_BIG), rc.EW_BIG.c, True, L)
    assert big == rc.EW_BIG_WANT
    if big["passes"] == 2 and 0 < big["last_pass"] < big["grid"] * rc.NT:
        have.add("ew:second-pass")
    for case in rc.EW_VIEWS:
        v4 = all(rc.vec4_ok(case.c, case.buf_c, case.ch0, ELEM[dt]) for dt in case.dtypes)
        have.add("ew:strided" if case.buf_c != case.c else "ew:dense")
        if not v4:
            have.add("ew:scalar")
    assert sorted(set(rc.PATHS) - have) == []
    assert rc.nvox(rc.EW_BIG) * rc.EW_BIG.c == 4587520          # the largest tensor of the GPU test


def _exact(ref, dtypes, what):
    for dt in dtypes:
        assert np.array_equal(rc.roundtrip(ref, dt), ref), f"{what} is not exact in {dt}"


@pytest.mark.parametrize("case", rc.STATS_CASES, ids=lambda c: c.name)
def test_statistics_sums_are_exact(case):
    d = rc.act_inputs(case.seed, rc.nvox(case), case.c)
    assert d.x.min() == -8 and d.x.max() == 8 and np.array_equal(d.x, np.round(d.x)) and not d.x.flags.writeable
    _exact(d.x.astype(np.float64), case.dtypes, "x")
    terms, grids = rc.stats_terms(d.x)
    assert rc.row_sum_bound(terms, grids, case.want["vpw"]) < 2.0 ** 24


@pytest.mark.parametrize("mode", rc.MODES)
@pytest.mark.parametrize("case", rc.REDUCE_CASES, ids=lambda c: c.name)
def test_backward_sums_are_exact(case, mode):
    n = rc.nvox(case)
    d = rc.act_inputs(case.seed, n, case.c)
    assert d.dy.min() == -4 and d.dy.max() == 4 and set(np.unique(d.invstd)) <= {0.5, 1.0}
    assert set(np.unique(d.gamma)) <= {2.0, -1.0} and np.abs(d.mean).max() <= 2 and np.abs(d.beta).max() <= 3
    _exact(d.dy.astype(np.float64), case.dtypes, "dy")
    alpha, mask, _ = rc.mode_args(mode, n, case.c)
    if mask is not None:
        assert set(np.unique(mask)) == {0.0, 2.0} and 0.45 < (mask > 0).mean() < 0.55
    terms, grids = rc.bwd_terms(d, alpha, mask)
    for t, g in zip(terms, grids):
        assert rc.on_grid(t, g) and float(np.abs(t).max()) <= 184           # 4 * 2 * (10 * 2 + 3), the dropped-in factor 2
    assert rc.row_sum_bound(terms, grids, case.want["vpw"]) < 2.0 ** 24
    assert rc.row_sum_bound(terms, grids, 4096) < 2.0 ** 24                 # and for the largest rows stat_vox can pick
    if alpha is not None:
        assert np.any(terms[2] != 0)


@pytest.mark.parametrize("c,sp,n,seed", rc.FUSED_CASES)
def test_one_launch_backward_is_exact(c, sp, n, seed):
    nv = n * sp[0] * sp[1] * sp[2]
    d = rc.act_inputs(seed, nv, c)
    for alpha in (rc.ALPHA, None):
        terms, grids = rc.bwd_terms(d, alpha, None)
        assert rc.row_sum_bound(terms, grids, 4096) < 2.0 ** 24
        sums = np.concatenate([t.sum(0) for t in terms])
        coef = rc.bn_bwd_finalize_ref(sums, c, nv)["coef"]
        # the coef of real sums is not dyadic: dx_f32_ref places the kernel's two f32 roundings, and its float64
        # operations in between must be exact (the same values in 64-bit-mantissa arithmetic)
        got = rc.dx_f32_ref(d, coef, alpha, None)
        wide = rc.dx_f32_ref(d, coef, alpha, None, real=np.longdouble)
        assert got.dtype == np.float64 and np.array_equal(got, wide.astype(np.float64))
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
        # a count of 2^15 voxels gives a dyadic coef and no rounding at all; 420 voxels do round
        assert bool(np.any(got != rc.dx_ref(d, coef, alpha, None))) == (nv & (nv - 1) != 0)


@pytest.mark.parametrize("case", (rc.EW_BIG,) + rc.EW_VIEWS, ids=lambda c: c.name)
def test_elementwise_references_are_exact_in_every_storage_type(case):
    n = rc.nvox(case)
    d, e = rc.act_inputs(case.seed, n, case.c), rc.ew_inputs(case.seed, n, case.c)
    assert set(np.unique(e.scale)) <= {2.0, -0.5} and rc.on_grid(e.coef[0], 0.5) and rc.on_grid(e.coef[1], 0.25)
    assert np.array_equal(e.shift, np.round(e.shift)) and np.array_equal(e.res, np.round(e.res))
    for mode in rc.MODES:
        alpha, mask, _ = rc.mode_args(mode, n, case.c)
        for res in (None, e.res):
            _exact(rc.fwd_ref(d.x, e.scale, e.shift, alpha, mask, res), case.dtypes, f"y ({mode})")
        _exact(rc.dx_ref(d, e.coef, alpha, mask), case.dtypes, f"dx ({mode})")
    _exact(rc.fwd_ref(d.x, None, None, None, None, e.res), case.dtypes, "a + b")


def test_roundtrip_rounds_to_nearest_even():
    # bf16 keeps 8 significant bits: ties go to the even neighbour
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 257.0, 259.0, -0.125, 1.0 + 2.0 ** -8 + 2.0 ** -20])
    assert rc.roundtrip(a, rc.BF16).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 256.0, 260.0, -0.125, 1.0 + 2.0 ** -7]
    assert rc.roundtrip(np.array([2049.0]), rc.F16).tolist() == [2048.0]


def test_drop_mask_restates_the_hash():
    """three values of norm_act.hip's drop_mult worked by hand with Python integers"""
    def one(e, seed, p):
        h = (e * 0x9E3779B1 & 0xFFFFFFFF) ^ seed ^ ((e >> 32) * 0x85EBCA77 & 0xFFFFFFFF)
        h ^= h >> 16; h = h * 0x7FEB352D & 0xFFFFFFFF
        h ^= h >> 15; h = h * 0x846CA68B & 0xFFFFFFFF
        h ^= h >> 16
        return 1 / (1 - p) if (h >> 8) >= int(p * 16777216) else 0.0
    m = rc.drop_mask(1000, rc.DROP_P, rc.DROP_SEED)
    assert m.tolist() == [one(e, rc.DROP_SEED, rc.DROP_P) for e in range(1000)]
