"""CPU proof of what the unequal-spacing GPU tests (tests/test_morphology_aniso_gpu.py) lean on, on the very
inputs they use (tests/helpers/morphology_aniso_cases.py): under the exact spacings the three forms of the oracle
agree bit for bit, nothing hangs on rounding and ties come in bulk; each deliberate fault of the step-by-step
form changes the result on the inputs meant to catch it; the tested radii have voxels exactly on them; under the
inexact spacings few voxels are near-ties and the step-by-step form itself keeps the two-tier rule; the slab and
the cliff drive the envelope stack to the line's length and empty it in one step."""
import numpy as np
import pytest

from tests.helpers import morphology_aniso_cases as C
from tests.helpers import morphology_ref as ref


def _id(v):
    return "x".join(f"{s:g}" for s in v) if isinstance(v, tuple) and v and isinstance(v[0], float) else None


def _feature(name):
    return C.volume(name) != 0


# ------------------------------------------------------------------ the sets themselves
def test_the_sets_hold_what_the_issue_names():
    assert {(2.0, 1.0, 0.5), (0.25, 1.0, 4.0), (5.0, 0.75, 0.75)} <= set(C.EXACT_3D) and C.EXACT_2D == (1.0, 0.5)
    assert {(5.0, 0.7, 0.7), (1.3, 0.7, 1.1), (6.0, 0.4, 1.0)} <= set(C.INEXACT_3D) and C.INEXACT_2D == (0.7, 1.1)
    shapes = {n: C.volume(n).shape for n in C.NAMES_3D + C.NAMES_2D}
    assert shapes["scattered_lo"] == shapes["scattered_hi"] == shapes["ellipsoid"] == (20, 24, 28)
    d, h, w = shapes["scattered_hi"]
    assert d * w > 512 and (d * w) % 256 and h * w > 512 and (h * w) % 256      # ragged last workgroup in P2 and P3
    assert shapes["wide"][2] > 64 and shapes["wide"][2] % 64
    assert shapes["bd1"][0] == 1 and shapes["bd2"][0] == 2 and shapes["flat"] == (40, 70)
    assert {C.volume(n).dtype for n in C.NAMES_3D} == {np.dtype(np.uint8), np.dtype(np.int16), np.dtype(np.int32)}
    for name, density in (("scattered_lo", 0.004), ("scattered_hi", 0.03)):
        assert 0.8 * density <= _feature(name).mean() <= 1.2 * density
    for name in C.NAMES_3D + C.NAMES_2D:                   # every predicate has features and non-features
        if name in ("staircase", "cliff"):
            continue
        for mode, _, _, feature in C.predicates(C.volume(name)):
            assert 0 < feature.sum() < feature.size, (name, mode)


# ------------------------------------------------------------------ exact spacings
@pytest.mark.parametrize("name,spacing", C.exact_pairs(), ids=_id)
def test_exact_spacings_three_forms_agree_and_nothing_hangs_on_rounding(name, spacing):
    feature = _feature(name)
    ib, db = ref.nearest_brute(feature, spacing)
    is_, ds = ref.nearest_separable(feature, spacing)
    ie, de, _ = ref.nearest_envelope(feature, spacing)
    assert np.array_equal(ib, is_) and np.array_equal(ib, ie)
    assert np.array_equal(db, ds) and np.array_equal(db, de)
    assert not ref.near_tie(feature, spacing).any()
    got = C.oracle(name, spacing, "FT_NONZERO")
    assert np.array_equal(got[0], ib) and np.array_equal(got[1], db)


@pytest.mark.parametrize("name,spacing", [(n, sp) for n, sp in C.exact_pairs()
                                          if n in ("scattered_hi", "cliff", "bd1", "bd2", "flat")], ids=_id)
def test_exact_spacings_dense_predicates_separable_equals_brute(name, spacing):
    """the dense predicates of the larger inputs are compared with the separable form on the device side"""
    lab = C.volume(name)
    for mode, _, _, feature in C.predicates(lab):
        if mode == "FT_ZERO" or (mode == "FT_NOT_EQUAL" and lab.size < 4000):
            ib, db = ref.nearest_brute(feature, spacing)
            is_, ds = ref.nearest_separable(feature, spacing)
            assert np.array_equal(ib, is_) and np.array_equal(db, ds), mode


@pytest.mark.parametrize("spacing", C.EXACT_3D + [C.EXACT_2D], ids=_id)
def test_exact_spacings_have_ties_in_bulk(spacing):
    dense = "flat" if len(spacing) == 2 else "scattered_hi"
    share = (ref.features_at_minimum(_feature(dense), spacing) >= 2).mean()
    print(f"{dense}: {share:.3%} of the voxels have two or more features at the minimum")
    assert share >= C.TIE_SHARE
    if len(spacing) == 3:
        for name in ("scattered_lo", "wide", "bd1", "bd2"):
            share = (ref.features_at_minimum(_feature(name), spacing) >= 2).mean()
            print(f"{name}: {share:.3%}")
            assert share >= C.TIE_SHARE_SPARSE, name


# ------------------------------------------------------------------ the deliberate faults
@pytest.mark.parametrize("fault", ref.ENVELOPE_FAULTS)
def test_each_index_fault_is_caught_by_its_inputs(fault):
    pairs = C.fault_pairs(fault)
    assert {sp for _, sp in pairs} == set(C.EXACT_3D) | {C.EXACT_2D}          # under every exact spacing
    for name, spacing in pairs:
        feature = _feature(name)
        want_i, want_d = C.oracle(name, spacing, "FT_NONZERO")
        got_i, got_d, _ = ref.nearest_envelope(feature, spacing, fault)
        changed = int((got_i != want_i).sum()), int((got_d != want_d).sum())
        print(fault, name, spacing, "indices / distances changed:", changed)
        if fault == "drop_hx":
            assert changed[1] > 0, (name, spacing)
        else:
            assert changed[0] > 0, (name, spacing)


def _six(lab, radius, spacing, applied):
    return {"nearest": ref.nearest_label(lab, spacing), "expand": ref.expand_labels(lab, radius, spacing),
            "dilate": ref.dilate_labels(lab, radius, spacing, applied),
            "erode": ref.erode_labels(lab, radius, spacing, applied),
            "open": ref.open_labels(lab, radius, spacing, applied),
            "close": ref.close_labels(lab, radius, spacing, applied)}


def _on_radius_counts(lab, spacing, radius, applied):
    """(background voxels whose nearest feature, labelled voxels whose nearest other voxel) lies exactly on radius"""
    feature = lab != 0 if applied is None else np.isin(lab, applied)
    _, dsq = ref.nearest_separable(feature, spacing)
    zero = int((ref.on_radius(dsq, radius) & (lab == 0)).sum())
    labelled = 0
    for L in ([int(v) for v in np.unique(lab) if v] if applied is None else applied):
        _, d = ref.nearest_separable(lab != L, spacing)
        labelled += int((ref.on_radius(d, radius) & (lab == L)).sum())
    return zero, labelled


@pytest.mark.parametrize("name,spacing,radius,applied", [c for c in C.LABEL_CASES if c[2] != C.BEYOND], ids=_id)
def test_label_cases_have_voxels_on_the_radius_and_the_open_ball_shows(name, spacing, radius, applied):
    lab = C.volume(name)
    zero, labelled = _on_radius_counts(lab, spacing, radius, None)
    print(f"exactly on radius {radius}: {zero} background voxels, {labelled} labelled voxels")
    assert zero >= C.ON_RADIUS_MIN and labelled >= C.ON_RADIUS_MIN
    if applied is not None:                                 # the subset has some of its own
        zero, labelled = _on_radius_counts(lab, spacing, radius, list(applied))
        print(f"applied {applied}: {zero} background voxels, {labelled} labelled voxels")
        assert zero > 0 and labelled > 0
    want = _six(lab, radius, spacing, applied)
    with ref.radius_open():
        faulty = _six(lab, radius, spacing, applied)
    assert np.array_equal(ref.expand_labels(lab, radius, spacing), want["expand"])      # the fault is gone again
    changed = [n for n in want if not np.array_equal(want[n], faulty[n])]
    print("the open ball changes", changed)
    assert "expand" in changed and "dilate" in changed and "erode" in changed


def test_label_cases_cover_what_the_issue_names():
    first = [(r, a) for n, sp, r, a in C.LABEL_CASES if n == "ellipsoid" and sp == (2.0, 1.0, 0.5)]
    assert {r for r, _ in first} == {1.0, 2.0, 2.5, 5.0, C.BEYOND}
    assert {a is None for _, a in first} == {True, False}
    assert any(n in ("mixed", "scattered_hi") for n, *_ in C.LABEL_CASES)
    diagonal = max(sum((s * e) ** 2 for s, e in zip(sp, C.DEFAULT)) ** 0.5 for sp in C.EXACT_3D)
    assert C.BEYOND > diagonal                              # larger than the volume under every spacing


# ------------------------------------------------------------------ inexact spacings
@pytest.mark.parametrize("name,spacing", C.inexact_pairs(), ids=_id)
def test_inexact_spacings_near_ties_are_few_and_the_envelope_keeps_the_two_tier_rule(name, spacing):
    lab = C.volume(name)
    sp3 = ref.spacing3(spacing, lab.ndim)
    shape3 = (1,) + lab.shape if lab.ndim == 2 else lab.shape
    gz, gy, gx = np.indices(shape3)
    for mode, _, _, feature in C.predicates(lab):
        if not C.fits_brute(name, mode):
            continue
        near = ref.near_tie(feature, spacing)
        print(f"{mode}: near-tie share {near.mean():.2e}")
        assert near.mean() <= C.NEAR_TIE_CAP, mode
        want_i, want_d = C.oracle(name, spacing, mode)
        got_i, got_d, _ = ref.nearest_envelope(feature, spacing)
        clear = ~near
        assert np.array_equal(got_i[clear], want_i[clear]), mode
        assert np.array_equal(got_d[clear], want_d[clear]), mode
        assert got_i.min() >= 0 and feature.reshape(-1)[got_i].all()
        iz, iy, ix = np.unravel_index(got_i.reshape(shape3), shape3)
        at_index = ref.dist_sq(gz - iz, gy - iy, gx - ix, sp3).reshape(lab.shape)
        assert np.all(np.abs(at_index - want_d) <= ref.REL * want_d), mode
        assert np.all((got_d == at_index) | (got_d == want_d)), mode


def test_clinical_label_case_stays_well_below_the_flag_cap():
    flags = C.general_flags(C.volume("clinical"), C.CLINICAL, C.CLINICAL_RADIUS, C.CLINICAL_APPLIED)
    for name, f in flags.items():
        print(f"{name}: flagged share {f.mean():.2e}")
        assert f.mean() <= C.FLAG_CAP / 2, name
    assert len(np.unique(C.volume("clinical"))) == 5


# ------------------------------------------------------------------ stack depth
@pytest.mark.parametrize("spacing", C.EXACT_3D + C.INEXACT_3D[:1], ids=_id)
def test_slab_and_staircase_fill_the_stack_and_the_cliff_empties_it(spacing):
    for name in ("slab", "staircase"):
        d, h, w = C.volume(name).shape
        stats = ref.nearest_envelope(_feature(name), spacing)[2]
        assert (stats.depth2, stats.depth3) == (h, d), (name, stats)           # as deep as the line
        assert (stats.pops2, stats.pops3) == (0, 0), (name, stats)
    d, h, w = C.volume("cliff").shape
    stats = ref.nearest_envelope(_feature("cliff"), spacing)[2]
    assert stats.pops2 >= h - 2 and stats.pops3 >= d - 2, stats                 # all but the lowest entry in one step
    assert stats.depth2 >= h - 1 and stats.depth3 >= d - 1, stats


# ------------------------------------------------------------------ equal in-plane spacings
def test_in_plane_order_is_exact_when_sy_equals_sx():
    """what the inexact-spacing inputs exposed: an f64 second pass prefers the feature at (-6, 7) over the one
    at (9, 2) by one bit and hands the wrong one to the third pass, where both are bit-equal.  With sy == sx
    the second pass counts voxels, and all three forms agree with the definition."""
    lab, spacing, voxel, winner = C.pythagorean_case()
    s = spacing[1]
    assert 6 * 6 + 7 * 7 == 9 * 9 + 2 * 2
    assert (s * 6) ** 2 + (s * 7) ** 2 < (s * 9) ** 2 + (s * 2) ** 2          # the bit that misled the second pass
    sp3 = ref.spacing3(spacing, 3)
    assert ref.dist_sq(1, -6, 7, sp3) == ref.dist_sq(1, 9, 2, sp3)
    feature = lab != 0
    assert not ref.near_tie(feature, spacing)[voxel]
    for nearest in (ref.nearest_brute, ref.nearest_separable, ref.nearest_envelope):
        assert nearest(feature, spacing)[0][voxel] == winner, nearest.__name__
    assert ref.nearest_label(lab, spacing)[voxel] == 4
