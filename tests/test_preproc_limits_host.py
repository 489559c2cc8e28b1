"""The inputs of tests/helpers/preproc_limits.py cross the limits their GPU tests are there for, and the comparisons
of those tests bite (no GPU needed).  The limits are read from landmarks.hip and nyul.hip; a changed constant or an
edited literal fails here with a message that names the case which no longer crosses its limit.  Each planted fault
is one line in a numpy restatement of a kernel's own decomposition; on the inputs of the GPU tests it must change the
result that those tests compare with the oracle."""
import shutil

import numpy as np
import pytest

from tests.helpers import detect_ref as dref
from tests.helpers import nyul_ref as nref
from tests.helpers import preproc_limits as lim


def test_every_case_crosses_its_limit():
    L = lim.read_limits()
    assert not L.missing, "\n".join(L.missing)
    bad = lim.crossings(L)
    assert not bad, "\n".join(bad)


def test_the_limits_are_the_ones_the_cases_were_sized_for():
    L = lim.read_limits()
    assert (L.kLmMaxLabels, L.kLmMaxWgs) == (255, 4096)
    assert (L.kNyulMaxLandmarks, L.kNyulBins, L.kSlotsLds, L.kHistThreads, L.kExactRankLimit) == \
        (64, 2048, 16, 1024, 1 << 24)
    assert (L.pass_a_per_chip, L.pass_bc_per_chip, L.map_per_chip) == (512, 256, 2048)


def _doctored(tmp_path, file, old, new):
    for f in {*lim.NAMED.values(), *(v[0] for v in lim.LITERALS.values())}:
        shutil.copy(lim.CSRC / f, tmp_path / f)
    text = (tmp_path / file).read_text()
    assert text.count(old) == 1, (file, old)
    (tmp_path / file).write_text(text.replace(old, new))
    return lim.read_limits(tmp_path)


@pytest.mark.parametrize("name, old, new, case", [
    ("kLmMaxLabels", "= 255;", "= 511;", "cent_dense()"),
    ("kLmMaxWgs", "= 4096;", "= 8192;", "hm_big_volume()"),
    ("kSlotsLds", "= 16;", "= 32;", "nyul_input('wide')"),
    ("kNyulMaxLandmarks", "= 64;", "= 128;", "Q64"),
    ("kExactRankLimit", "= 1 << 24;", "= 1 << 25;", "nyul_big('above')"),
])
def test_a_doubled_constant_is_reported_with_its_case(tmp_path, name, old, new, case):
    L = _doctored(tmp_path, lim.NAMED[name], f"constexpr int {name} {old}", f"constexpr int {name} {new}")
    assert getattr(L, name) == 2 * getattr(lim.read_limits(), name) + (name == "kLmMaxLabels")
    bad = lim.crossings(L)
    assert bad and any(m.startswith(case) for m in bad), bad


@pytest.mark.parametrize("key", sorted(lim.LITERALS))
def test_an_edited_grid_literal_is_reported(tmp_path, key):
    file, line, numbers = lim.LITERALS[key]
    number = str(next(iter(numbers.values())))
    L = _doctored(tmp_path, file, line, line.replace(f" {number},", f" {2 * int(number)},"))
    bad = lim.crossings(L)
    assert len(bad) == 1 and file in bad[0] and line in bad[0], bad


# ------------------------------------------------------------------ landmarks: the restatements and their faults
@pytest.mark.parametrize("dtype", lim.LABEL_DTYPES)
def test_centroid_restatement_and_the_dropped_x0(dtype):
    cases = [(lim.cent_volume(lim.CENT_V4_SHAPE, dtype), lim.CENT_K), (lim.cent_volume(lim.CENT_V1_SHAPE, dtype), lim.CENT_K),
             (lim.cent_dense(dtype), lim.CENT_DENSE_K), (lim.cent_late(dtype), lim.CENT_LATE_K)]
    for lab, k in cases:
        assert lab.dtype == np.dtype(dtype) and not lab.flags.writeable
        want = dref.centroid_sums(lab, k)
        assert int(want[:, 0].sum()) == lab.size
        for v in ((4, 1) if lab.shape[2] % 4 == 0 else (1,)):     # the misaligned view walks a V = 4 shape at V = 1
            assert np.array_equal(lim.centroid_by_trips(lab, k, v), want)
            got = lim.centroid_by_trips(lab, k, v, fault="x0_dropped")
            present = want[:, 0] > 0
            assert np.array_equal(got[:, (0, 2, 3)], want[:, (0, 2, 3)])
            assert (got[present, 1] < want[present, 1]).all(), "a label whose sum x survives the fault checks nothing"
    late = dref.centroid_sums(lim.cent_late(dtype), lim.CENT_LATE_K)[lim.CENT_LATE_LABEL]
    assert late[1] >= late[0] * lim.CENT_LATE_FROM > 0            # all of its sum x is past the first trip


@pytest.mark.parametrize("shape", lim.AM_SHAPES)
def test_argmax_restatement_and_the_later_trip(shape):
    x = lim.am_volume(shape)
    val, xyz = lim.argmax_points(x)
    # the reference order against plain numpy: the first maximum of the [x, y, z] array in C order
    for c in range(shape[0]):
        t = np.transpose(x[c], (2, 1, 0))
        assert tuple(xyz[c]) == np.unravel_index(int(np.argmax(t)), t.shape) and val[c] == t.max()
    for v in ((4, 1) if shape[3] % 4 == 0 else (1,)):
        got_val, got_xyz = lim.argmax_by_trips(x, v)
        assert np.array_equal(got_val, val) and np.array_equal(got_xyz, xyz)
        bad_val, bad_xyz = lim.argmax_by_trips(x, v, fault="later_trip_wins")
        assert np.array_equal(bad_val, val)
        assert np.array_equal(bad_xyz[0], xyz[0])                 # a single maximum cannot tell
        assert bad_xyz[1, 0] > xyz[1, 0] and bad_xyz[2, 0] > xyz[2, 0]


def test_argmax_many_channels_and_nan_inputs():
    x = lim.am_many()
    val, xyz = lim.argmax_points(x)
    i = np.arange(lim.AM_MANY_SHAPE[0])
    assert np.array_equal(val, (lim.AM_PEAK + i).astype(np.float32)) and np.unique(val).size == val.size
    assert np.array_equal(xyz, np.stack([(i // 7) % 5, (i // 2) % 3, i % 2], 1))
    n = lim.am_nan_volume()
    assert np.isnan(n).sum() == 1 and np.isnan(n[1]).any()
    with pytest.raises(ValueError, match="channel 2"):            # the dummy channel shifts the number by one
        lim.argmax_points(n)


def test_boxes_of_the_positive_box_cases():
    for dtype in lim.PBOX_DTYPES:
        x = lim.pbox_rows_volume(dtype)
        c, zy = divmod(lim.PBOX_ROW, 70 * 60)
        assert dref.bbox(x) == [[5, zy % 60, zy // 60], [6, zy % 60 + 1, zy // 60 + 1]]
        # the first pass of the grid alone finds nothing
        assert dref.bbox(x.reshape(-1, 8)[:lim.PBOX_ROWS_PER_PASS].reshape(1, 1, -1, 8)) == [[0, 0, 0], [0, 0, 0]]
        for shape in lim.PBOX_TRIP_SHAPES:
            x = lim.pbox_trip_volume(shape, dtype)
            step = 256 if shape[3] % 4 == 0 else 64
            assert dref.bbox(x) == [[step + 44, 1, 1], [shape[3], 3, 3]]
            assert dref.bbox(x[..., :step]) == [[0, 0, 0], [0, 0, 0]]                    # the first trip alone: nothing
            assert dref.bbox(x[..., :2 * step])[1][0] == step + 45                        # the far face is the last trip's


def test_heatmap_cases_have_their_centres_and_tails():
    lab = lim.hm_trip_volume()
    for c, (z, y, x) in lim.HM_TRIP_BLOCKS.items():
        assert dref.centre(lab, c) == (x, y, z)
    lab = lim.hm_big_volume()
    assert [dref.centre(lab, c)[0] for c in (1, 128, 255)] == [10, 140, 250]
    assert lim.hm_support(lab, 255) == [(142, 299, True), (0, 15, True), (0, 11, True)]
    assert lim.hm_support(lab, 1)[0] == (4, 16, False) and lim.hm_support(lab, 128)[0] == (140 - 57, 140 + 57, False)
    assert dref.kernel_f64(255).size == lim.HM_STRIDE


@pytest.mark.parametrize("label", [1, 12, 128, 255])
def test_kernel_tables_are_rounded_once(label):
    """the device tables against the f64 closed form rounded to f32: at most one ulp (the two erf implementations),
    in the tail of the widest table too, where differences formed in f32 were off by 1 %"""
    from segmantic_amd.detect.transforms import gaussian_kernel_1d, heatmap_sigma
    k = gaussian_kernel_1d(heatmap_sigma(label)).numpy()
    want = dref.kernel_f64(label)
    assert k.dtype == np.float32 and k.size == 2 * dref.tail_of(label) + 1 and (k > 0).all()
    np.testing.assert_allclose(k, want, rtol=2.0 ** -23, atol=0)
    assert np.array_equal(k, k[::-1]) and int(k.argmax()) == dref.tail_of(label)


# ------------------------------------------------------------------ Nyul: slots, the select and its faults
def test_slot_counts_of_the_64_landmark_inputs():
    L = lim.read_limits()
    report = lim.nyul_slot_report(L)
    print("\n".join(f"{k[0]:7s} nonzero={k[1]!s:5s} pass B {v[0]:3d}  pass C {v[1]:3d}  most under one top digit {v[2]:3d}"
                    for k, v in report.items()))
    S = L.kSlotsLds
    for nonzero in (False, True):
        assert report["wide", nonzero][0] > 4 * S and report["wide", nonzero][1] > 6 * S
        assert report["narrow", nonzero][2] > 2 * S
        assert report["mixed", nonzero][0] > S and report["mixed", nonzero][2] > S
    assert report["narrow", True][0] == 1                          # all under one top digit once the zeros are masked


@pytest.mark.parametrize("nonzero", [False, True])
@pytest.mark.parametrize("kind", ["wide", "narrow", "mixed"])
def test_select_restatement_and_the_slot_faults(kind, nonzero):
    L = lim.read_limits()
    m = lim.masked(lim.nyul_input(kind), nonzero)
    ranks = lim.all_ranks(lim.Q64, m.size, L.kExactRankLimit)
    assert ranks.size == 128 and ranks.min() == 0 and ranks.max() == m.size - 1
    want = np.sort(lim.f2key(m))[ranks]
    # the keys order as the values do, and np.partition names the same order statistics
    assert lim._same_value(lim.key2f(want), np.partition(m, np.unique(ranks))[ranks])
    assert np.array_equal(lim.radix_select(m, ranks, L.kSlotsLds), want)
    first_group = lim.radix_select(m, ranks, L.kSlotsLds, fault="first_group_only")
    first_slot = lim.radix_select(m, ranks, L.kSlotsLds, fault="first_slot_of_digit")
    assert (first_group != want).any(), "no rank lies past the first kSlotsLds slots"
    if kind == "wide":
        # past 4 groups in pass B: most ranks are lost
        assert (first_group != want).sum() > 64
    else:
        assert (first_slot != want).sum() > 2 * L.kSlotsLds, "no top digit holds several pass-C slots"
    # and through the lerp: the landmarks that the GPU test compares change too
    for faulty in (first_group, first_slot if kind != "wide" else first_group):
        lo, hi = lim.key2f(faulty[0::2]), lim.key2f(faulty[1::2])
        w = [lim.rank_rule(q, m.size, L.kExactRankLimit)[2] for q in lim.Q64]
        got = np.array([nref._lerp32(a, b, ww) for a, b, ww in zip(lo, hi, w)], np.float32)
        assert not lim._same_value(got, nref.landmarks(m, lim.Q64))


def test_landmarks_by_rule_is_the_reference_and_repeated_quantiles_repeat():
    L = lim.read_limits()
    for kind in ("wide", "narrow", "mixed"):
        for nonzero in (False, True):
            m = lim.masked(lim.nyul_input(kind), nonzero)
            for q in (lim.Q64, lim.Q64_REPEATED):
                assert lim._same_value(lim.landmarks_by_rule(m, q, L.kExactRankLimit), nref.landmarks(m, q))
    rep = nref.landmarks(lim.nyul_input("wide"), lim.Q64_REPEATED).reshape(16, 4)
    assert (rep == rep[:, :1]).all() and np.unique(rep).size == 16


def test_the_regime_follows_the_masked_count():
    L = lim.read_limits()
    limit = L.kExactRankLimit
    for form, f32_rule in (("below", True), ("above", False)):
        x = lim.nyul_big(form)
        assert not (lim._big_base() == 0).any()
        m = lim.masked(x, True)
        assert x.size == lim.BIG_N > limit and m.size == lim.BIG_N - lim.BIG_ZEROS[form]
        assert (m.size <= limit) == f32_rule
        want = nref.landmarks(m, lim.Q_BIG)
        assert lim._same_value(lim.landmarks_by_rule(m, lim.Q_BIG, limit), want)
        if f32_rule:
            # the planted fault: the regime of the segment length (numpy's f64 rule) on a masked count under 2^24
            wrong = lim.landmarks_by_rule(m, lim.Q_BIG, limit, regime_n=x.size)
            assert not lim._same_value(wrong, want)
            assert (wrong != want).sum() >= 4
            # plain numpy on both sides: the f64 rule is np.quantile's, and the f32 rule's integer ranks are not
            assert np.array_equal(wrong, np.quantile(m.astype(np.float64), lim.Q_BIG).astype(np.float32))
        else:
            assert np.array_equal(want, np.quantile(m.astype(np.float64), lim.Q_BIG).astype(np.float32))


def test_segment_and_map_inputs():
    for n in lim.MANY_LENS:
        x = lim.nyul_many(n)
        assert x.shape == (lim.MANY_SEGMENTS, n) and not x[333].any() and (x[:, 7] == 0).all()
        lm = nref.all_landmarks(x, lim.Q3, True, True)
        assert np.isnan(lm[333]).all() and np.isfinite(np.delete(lm, 333, 0)).all()
        assert np.unique(lm[:, 1]).size > 590                      # no two segments alike
    x, lm, scale = lim.nyul_map_many()
    assert x.shape == (lim.MAP_SEGMENTS, lim.MAP_LEN) and lm.shape == (lim.MAP_SEGMENTS, lim.MAP_L)
    assert (np.diff(lm, axis=1) > 0).all()
    out = nref.apply_with(x, lm, scale, True, True)
    assert np.isfinite(out).all() and (out[:, 3] == 0).all() and (out[:, :3] != x[:, :3]).all()
    # a map that used the landmarks of segment 0 throughout (or of the segment before) would differ on almost all
    assert (out[1:] != nref.apply_with(x[1:], lm[:-1], scale, True, True)).mean() > 0.9
    for pad in (True, False):
        x, lm, scale = lim.nyul_map_64(pad)
        out = nref.apply_with(x[None], lm[None], scale, False)[0]
        on = np.flatnonzero(np.isin(x, lm))
        assert on.size == 64
        assert np.allclose(np.sort(out[on]), scale, rtol=0, atol=1e-3)                 # a landmark maps to its scale value
        assert np.isnan(out).sum() == 1 and np.isinf(out).sum() == 2
        masked_out = nref.apply_with(x[None], lm[None], scale, True)[0]
        z = x == 0
        assert np.array_equal(masked_out[z].view(np.uint32), x[z].view(np.uint32)) and (out[z] != 0).all()
