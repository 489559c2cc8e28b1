"""The generators of tests/helpers/evaluation_limits.py cross the limits their GPU tests are there for, and the
oracles added to tests/helpers/distance_ref.py reject the faults seeded into them (no GPU needed).  A changed
constant or an edited literal of csrc/distance.hip fails here, with a message that names the generator, instead
of turning tests/test_evaluation_ops_gpu.py into a test of the easy path."""
import shutil

import numpy as np
import pytest

from tests.helpers import distance_ref as ref
from tests.helpers import evaluation_limits as lim


def test_every_generator_crosses_its_limit():
    L = lim.read_limits()
    assert (L.kBoxMaxLabels, L.kSampleWgs, L.kSelectWgs, L.kSelectBins, L.kSelectMaxRanks) == (1024, 1024, 512, 2048, 4)
    bad = lim.crossings(L)
    assert not bad, "\n".join(bad)


def _doctored(tmp_path, old, new, file=lim.SOURCE):
    """a copy of the sources with one edit"""
    for f in lim.FILES:
        shutil.copy(lim.CSRC / f, tmp_path / f)
    text = (tmp_path / file).read_text()
    assert text.count(old) == 1, old
    (tmp_path / file).write_text(text.replace(old, new))
    return lim.read_limits(tmp_path)


@pytest.mark.parametrize("name, generator", [("kBoxMaxLabels", "box_table_volume()"), ("kSampleWgs", "sample_trip_case()"),
                                             ("kSelectWgs", "select sizes"), ("kSelectBins", "select_bits()"),
                                             ("kSelectMaxRanks", "select tests"), ("kFinTickets", "sampler ticket test")])
def test_a_doubled_constant_is_reported_with_its_generator(tmp_path, name, generator):
    value = getattr(lim.read_limits(), name)
    L = _doctored(tmp_path, f"constexpr int {name} = {value};", f"constexpr int {name} = {2 * value};",
                  lim.TICKETS[1] if name == lim.TICKETS[0] else lim.SOURCE)
    assert getattr(L, name) == 2 * value
    bad = lim.crossings(L)
    assert len(bad) == 1 and name in bad[0] and bad[0].startswith(generator), bad


@pytest.mark.parametrize("key", sorted(lim.LITERALS))
def test_an_edited_literal_is_reported(tmp_path, key):
    entry, line, _ = lim.LITERALS[key]
    text = (lim.CSRC / lim.SOURCE).read_text()
    at = text.index(line, text.index(f" {entry}("))
    edited = line.replace("1024", "2048").replace("64)", "32)").replace("4096", "8192").replace("kSampleWgs", "512")
    assert edited != line
    for f in lim.FILES:
        shutil.copy(lim.CSRC / f, tmp_path / f)
    (tmp_path / lim.SOURCE).write_text(text[:at] + edited + text[at + len(line):])
    bad = lim.crossings(lim.read_limits(tmp_path))
    assert len(bad) == 1 and entry in bad[0] and line in bad[0], bad


def test_a_literal_in_another_entry_point_does_not_count(tmp_path):
    # the confusion grid's line also reads `1024`: moving the boxes literal there must still be reported
    L = _doctored(tmp_path, "lv_grid(rows, 4, 1024)", "lv_grid(rows, 8, 1024)")
    assert len(L.missing) == 1 and "segmi_label_boxes" in L.missing[0]


# ---------------------------------------------------------------------------- label boxes
def test_box_volumes_cross_the_chunk_edges_and_the_second_trip():
    for w in lim.BOX_WIDTHS:
        for dtype in lim.LABEL_TYPES:
            pred, truth = lim.box_width_volume(w, dtype)
            assert pred.shape == truth.shape == (3, 5, w) and pred.dtype == truth.dtype == np.dtype(dtype)
            boxes, counts = ref.label_boxes(pred, truth, lim.BOX_K)
            skipped = lambda a: int(((a.astype(np.int64) < 0) | (a.astype(np.int64) >= lim.BOX_K)).sum())
            assert int(counts[:, 0].sum()) + skipped(pred) == pred.size and int(counts[:, 1].sum()) + skipped(truth) == truth.size
            if w > 1:
                assert skipped(pred) > 0 and skipped(truth) > 0
                assert counts[3, 0] > 0 and counts[3, 1] == 0 and counts[4, 0] == 0 and counts[4, 1] > 0
            if dtype != "uint8" and w > 1:
                assert (pred < 0).any() and (truth < 0).any()
            if w == 130:
                assert boxes[5].tolist() == [1, 2, 2, 3, 60, 71] and counts[5].tolist() == [11, 0]
            else:
                assert boxes[5].tolist() == [0] * 6 and counts[5].tolist() == [0, 0]      # the absent label
    pred, truth = lim.box_width_volume(130, "int16", 2)
    assert pred.shape == (5, 130) and ref.label_boxes(pred, truth, lim.BOX_K)[0][5].tolist() == [0, 1, 2, 3, 60, 71]
    d, h, w = lim.BOX_TRIP_SHAPE
    assert d * h == 4158
    for dtype in lim.LABEL_TYPES:
        pred, truth, k = lim.box_trip_volume(dtype)
        for a in (pred, truth):
            rows = np.flatnonzero((a.reshape(d * h, w) == 2).any(1))
            assert rows.size >= 7 and rows.min() >= lim.BOX_ROWS_PER_TRIP
        boxes, counts = ref.label_boxes(pred, truth, k)
        assert boxes[2][0] == 65 and boxes[2][1] == 66 and boxes[2][5] == w and boxes[3].tolist() == [0] * 6
        assert boxes[1].tolist() == [0, d, 0, h, 0, w]


def test_box_tables_hold_every_label_once():
    for k, dtype in lim.BOX_TABLE_KS:
        pred, truth = lim.box_table_volume(k, dtype)
        assert pred.dtype == np.dtype(dtype) and not np.array_equal(pred, truth)
        boxes, counts = ref.label_boxes(pred, truth, k)
        assert (counts == 1).all() and ((boxes[:, 1::2] - boxes[:, 0::2]) >= 1).all()
        assert pred.size > k and ((pred.astype(np.int64) >= k) | (pred.astype(np.int64) < 0)).sum() == pred.size - k


def test_label_boxes_oracle_on_a_known_volume():
    pred = np.zeros((4, 5, 6), np.int16)
    truth = np.zeros((4, 5, 6), np.int16)
    pred[1, 2, 3] = 1
    truth[3, 0, 5] = 1
    truth[2, 2, 2] = -1
    boxes, counts = ref.label_boxes(pred, truth, 3)
    assert boxes.tolist() == [[0, 4, 0, 5, 0, 6], [1, 4, 0, 3, 3, 6], [0] * 6]
    assert counts.tolist() == [[119, 118], [1, 1], [0, 0]]


# ---------------------------------------------------------------------------- EDT
def test_long_volumes_pass_2_24_and_the_restatement_stays_inside_three_roundings():
    """the float32 restatement against the float64 brute force: equal below 2^24, within three roundings beyond"""
    u = 2.0 ** -24
    bound = (1 + u) ** 3 - 1
    for shape in lim.LONG_SHAPES:
        lab = lim.long_volume(shape)
        assert int(lab.sum()) == len(lim.long_points(shape)) == 3
        want = ref.edt_sq_brute(lab == 1, (1.0,) * len(shape))
        lo, hi = lim.long_extremes(shape)
        assert (want.min(), want.max()) == (lo, hi) and hi > 2 ** 25
        got = ref.edt_sq_passes_f32(lab == 1).astype(np.float64)
        small = want < lim.EXACT_F32
        assert small.sum() > 1000 and (~small).sum() > 1000
        assert np.array_equal(got[small], want[small])
        worst = float((np.abs(got - want)[~small] / (bound * want[~small])).max())
        print(f"{shape}: restatement error at most {worst:.4f} of three float32 roundings")
        assert 0 < worst <= 1.0                     # rounded somewhere, never more than the bound


def test_restatement_is_the_exact_transform_on_small_volumes():
    rng = np.random.default_rng(3)
    for shape in ((9, 11, 14), (13, 17)):
        f = rng.random(shape) < 0.05
        assert np.array_equal(ref.edt_sq_passes_f32(f).astype(np.float64), ref.edt_sq_brute(f, (1.0,) * len(shape)))
    assert np.isinf(ref.edt_sq_passes_f32(np.zeros((3, 4), bool))).all()


def test_brute_force_on_index_differences_equals_the_separable_oracle():
    rng = np.random.default_rng(4)
    f = rng.random((6, 9, 12)) < 0.05
    sp = tuple(float(np.float32(s)) for s in (2.0, 0.8, 0.5))
    a, b = ref.edt_sq_brute(f, sp), ref.edt_sq_separable(f, sp)
    assert np.abs(a - b).max() <= 8 * 2.0 ** -53 * a.max()
    assert ref.edt_sq_brute(f, (1.0, 1.0, 1.0))[tuple(np.argwhere(f)[0])] == 0.0


def _box_cases():
    return (("block", lim.CUT_BOX), ("border", lim.BORDER_BOX)) + tuple(("block", b) for b in lim.THIN_BOXES)


def test_cut_boxes_cut_and_the_contour_there_needs_the_outside():
    b, c = lim.CUT_BLOCK, lim.CUT_BOX
    assert all(b[2 * a] < c[2 * a] and c[2 * a + 1] < b[2 * a + 1] for a in range(3))
    for kind, box in (("block", lim.CUT_BOX), ("border", lim.BORDER_BOX)):
        lab = lim.cut_volume(kind)
        sl = ref.box_slices(box)
        m = lab == 2
        # every face of the box holds label voxels, and the contour of the cropped label differs from the crop of
        # the contour: a kernel that stopped looking at the box's faces would be caught
        for a in range(3):
            for side in (0, -1):
                assert np.take(m[sl], side, axis=a).any()
        assert not np.array_equal(ref.contour(m)[sl], ref.contour(m[sl]))
        assert ref.contour(m)[sl].any() and (m[sl] & ~ref.contour(m)[sl]).any()
    z0, z1, y0, y1, x0, x1 = lim.BORDER_BOX
    assert z0 == 0 and y1 == lim.CUT_SHAPE[1] and x1 == lim.CUT_SHAPE[2] and z1 < lim.CUT_SHAPE[0] and y0 > 0 and x0 > 0
    for a, box in enumerate(lim.THIN_BOXES):
        assert box[2 * a + 1] - box[2 * a] == 1


@pytest.mark.parametrize("fault", ["no_z_faces", "outside_is_foreground", "no_sign"])
def test_the_edt_comparison_rejects_a_seeded_fault(fault):
    """what tests/test_evaluation_ops_gpu.py compares exactly (finite pattern, values, sign bits) differs under each
    fault on the very cases it runs"""
    caught = []
    for kind, box in _box_cases():
        lab = lim.cut_volume(kind)
        want, sign = ref.signed_edt_sq(lab, 2, 1, (1.0, 1.0, 1.0), box)
        bad, bad_sign = ref.signed_edt_sq(lab, 2, 1, (1.0, 1.0, 1.0), box, fault=fault)
        caught.append(not np.array_equal(want, bad) or not np.array_equal(sign, bad_sign))
    # z faces: every 3-D case with more than a slab; outside: the box on the volume's border; sign: every case
    assert caught[1] and (caught[0] or fault == "outside_is_foreground")
    assert all(caught) or fault != "no_sign"
    # the faults are faults of the 3-D contour and of the border only
    flat = lim.sample_case(70, "uint8", 2)[1]
    assert np.array_equal(ref.contour(flat == 3), ref.contour(flat == 3, "no_z_faces"))


@pytest.mark.parametrize("fault", ["no_z_faces", "outside_is_foreground", "no_clamp"])
def test_the_sampler_comparison_rejects_a_seeded_fault(fault):
    """count and sorted values, compared exactly by the GPU test, differ under each fault on its own cases"""
    caught = []
    for bw in lim.SAMPLE_WIDTHS:
        tgt, qry, label, box = lim.sample_case(bw, "int16")
        dist, sign = ref.signed_edt_sq(tgt, label, 1, (1.0, 1.0, 1.0), box)
        signed = np.where(sign, -dist, dist).astype(np.float32)
        for query in (0, 1):
            want = np.sort(ref.query_values(signed, qry, label, query, box))
            bad = np.sort(ref.query_values(signed, qry, label, query, box, fault=fault))
            caught.append((query, not np.array_equal(want, bad)))
    if fault == "no_clamp":
        assert all(c for q, c in caught if q == 0) and not any(c for q, c in caught if q == 1)
    elif fault == "no_z_faces":
        assert all(c for q, c in caught if q == 1) and not any(c for q, c in caught if q == 0)
    else:
        # the sample boxes lie inside their volumes, so the border fault shows on a whole-volume box only
        assert not any(c for _, c in caught)
        tgt, qry, label, box = lim.sample_trip_case()
        full = np.ones(lim.SAMPLE_TRIP_SHAPE, np.uint8)
        assert ref.contour(full == 1).sum() > 0 == ref.contour(full == 1, fault).sum()


def test_sample_cases_surround_the_box_and_place_the_maximum_late():
    for bw in lim.SAMPLE_WIDTHS:
        for ndim in (2, 3):
            tgt, qry, label, box = lim.sample_case(bw, "uint8", ndim)
            q3 = (qry == label).reshape((1,) * (3 - ndim) + qry.shape)
            z0, z1, y0, y1, x0, x1 = box
            assert x1 - x0 == bw and q3[z0:z1, y0:y1, x0 - 1].all() and q3[z0:z1, y0:y1, x1].all()
            assert q3[z0:z1, y0 - 1, x0:x1].all() and q3[z0:z1, y1, x0:x1].all()
            if ndim == 3:
                assert q3[z0 - 1, y0:y1, x0:x1].all() and q3[z1, y0:y1, x0:x1].all()
            # the voxels outside are not queries, but they decide the contour on the faces
            sl = ref.box_slices(box, ndim)
            assert not np.array_equal(ref.contour(qry == label)[sl], ref.contour((qry == label)[sl]))
            assert 0 < ref.contour(qry == label)[sl].sum() < (qry == label)[sl].sum()
    tgt, qry, label, box = lim.sample_trip_case()
    d, h, w = lim.SAMPLE_TRIP_SHAPE
    dist, _ = ref.signed_edt_sq(tgt, label, 1, (1.0, 1.0, 1.0), box)
    q = qry == label
    rows = np.flatnonzero(q.reshape(d * h, w).any(1))
    assert (rows < lim.SAMPLE_ROWS_PER_TRIP).sum() > 100 and (rows >= lim.SAMPLE_ROWS_PER_TRIP).sum() >= 2
    best = np.unravel_index(np.argmax(np.where(q, dist, -1.0)), q.shape)
    assert best == (d - 1, h - 1, w - 1) and best[0] * h + best[1] >= lim.SAMPLE_ROWS_PER_TRIP
    first_trip = q.copy().reshape(d * h, w)
    first_trip[lim.SAMPLE_ROWS_PER_TRIP:] = False
    assert dist[first_trip.reshape(q.shape)].max() < dist[best]


def test_sample_stats_oracle():
    (n, s, q, mx), (es, eq) = ref.sample_stats(np.asarray([4.0, 0.0, 9.0, 2.0], np.float32))
    assert (n, q, mx) == (4, 15.0, 3.0) and s == 2.0 + 3.0 + np.sqrt(2.0) and es == 4 * 2.0 ** -52 * s and eq == 4 * 2.0 ** -52 * 15
    assert ref.sample_stats(np.zeros(0, np.float32)) == ((0, 0.0, 0.0, 0.0), (0.0, 0.0))
    signed = np.asarray([[-0.0, -4.0], [1.0, 9.0]], np.float32)
    lab = np.asarray([[3, 3], [3, 0]], np.uint8)
    assert ref.query_values(signed, lab, 3, 0).tolist() == [0.0, 0.0, 1.0]
    assert not np.signbit(ref.query_values(signed, lab, 3, 0)).any()
    assert ref.query_values(signed, lab, 3, 1).tolist() == [0.0, 4.0, 1.0]
    assert ref.query_values(signed, lab, 3, 0, fault="no_clamp").tolist() == [0.0, 4.0, 1.0]


# ---------------------------------------------------------------------------- select and confusion counts
def test_select_patterns_leave_the_decision_to_the_later_passes():
    bits = lambda v: v.view(np.uint32)
    m = bits(lim.select_bits("middle"))
    assert np.unique(m >> 21).tolist() == [lim.SELECT_TOP11] and np.unique(m & 1023).size == 1
    assert np.unique((m >> 10) & 2047).size > 1500
    lo = bits(lim.select_bits("low"))
    assert np.unique(lo >> 10).size == 1 and np.unique(lo & 1023).size > 900
    for n in lim.SELECT_SIZES:
        a = lim.select_bits("any", n)
        assert a.shape == (n,) and np.isfinite(a).all() and not np.signbit(a).any()
        # float order is bit-pattern order for non-negative values: what the radix select relies on
        assert np.array_equal(np.argsort(a, kind="stable"), np.argsort(bits(a), kind="stable"))
    a = lim.select_bits("any", lim.SELECT_SIZES[2])
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert ((a > 0) & (a < tiny)).any() and (a == 0).any() and np.unique(bits(a) >> 21).size > 500


def test_confusion_cases_cover_the_switch_the_cap_and_the_tail():
    L = lim.read_limits()
    assert [k for k, _ in lim.CONF_KS] == [L.confusion_lds_k, L.confusion_lds_k + 1, L.confusion_max_k]
    for k, dtype in lim.CONF_KS:
        p, t = lim.confusion_case(k, dtype, 5000)
        assert p.dtype == np.dtype(dtype) and int(p.max()) == k - 1 == int(t.max()) and int(p.min()) == 0 == int(t.min())
        assert {(0, 0), (k - 1, k - 1), (0, k - 1), (k - 1, 0)} <= set(zip(t[:4].tolist(), p[:4].tolist()))
    p, t, k = lim.confusion_trip_case("uint8")
    assert p.size == lim.CONF_TRIP_N == L.confusion_per_wg * L.confusion_grid_cap + 1000
    assert max(p[:lim.CONF_TRIP].max(), t[:lim.CONF_TRIP].max()) < 20 <= min(p[lim.CONF_TRIP:].min(), t[lim.CONF_TRIP:].min())
