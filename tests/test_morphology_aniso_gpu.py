"""The unequal-spacing path of the feature transform and the label morphology held to exact results.  Under
spacings whose f64 arithmetic is exact every voxel's index, squared distance and label is compared with the
brute-force oracle at zero tolerance, ties and voxels exactly on the radius included; under spacings that round
the two-tier rule leaves no voxel out.  tests/test_morphology_aniso_host.py shows on the CPU that these inputs
(tests/helpers/morphology_aniso_cases.py) have the ties, the on-radius voxels and the stack depths meant here and
that each deliberate fault of the step-by-step oracle shows up on them."""
import numpy as np
import pytest
import torch

from tests.helpers import morphology_aniso_cases as C
from tests.helpers import morphology_ref as ref
from tests.test_morphology_gpu import _check_general, _dev, _ft, _m, _ops, _six

pytestmark = pytest.mark.gpu


def _id(v):
    return "x".join(f"{s:g}" for s in v) if isinstance(v, tuple) and v and isinstance(v[0], float) else None


def _table(labels):
    table = np.zeros(65536, np.uint8)
    table[list(labels)] = 1
    return table


def _transform(lab, mode, spacing, label=0, labels=None, box=None, dist_sqrt=False):
    return _ft(lab, getattr(_ops(), mode), spacing, label=label, table=None if labels is None else _table(labels),
               box=box, dist_sqrt=dist_sqrt)


def _assert_bits(got_d, want_dsq, what):
    want = want_dsq.astype(np.float32)
    assert got_d.dtype == np.float32 and np.array_equal(got_d.view(np.int32), want.view(np.int32)), what


def _within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    return np.all((got >= np.nextafter(want, np.float32(-np.inf))) & (got <= np.nextafter(want, np.float32(np.inf))))


# ------------------------------------------------------------------ (a) exact spacings: every voxel, zero tolerance
@pytest.mark.parametrize("name,spacing", C.exact_pairs(), ids=_id)
def test_exact_spacings_index_and_distance_on_every_voxel(name, spacing):
    lab = C.volume(name)
    for mode, label, labels, _ in C.predicates(lab):
        want_i, want_d = C.oracle(name, spacing, mode)
        got_i, got_d = _transform(lab, mode, spacing, label, labels)
        assert np.array_equal(got_i, want_i), (mode, int((got_i != want_i).sum()))
        _assert_bits(got_d, want_d, mode)
    want_i, want_d = C.oracle(name, spacing, "FT_NONZERO")
    got_i, got_r = _transform(lab, "FT_NONZERO", spacing, dist_sqrt=True)
    assert np.array_equal(got_i, want_i) and _within_one_ulp(got_r, np.sqrt(want_d))
    planes = _ops().morph_index_planes(_dev(want_i)).cpu().numpy()
    assert np.array_equal(planes, ref.index_planes(want_i))


BOXES = [("scattered_hi", sp, (3, 17, 2, 21, 4, 25)) for sp in C.EXACT_3D] + \
        [("ellipsoid", C.EXACT_3D[0], (1, 19, 5, 23, 2, 20)), ("wide", C.EXACT_3D[2], (2, 8, 1, 10, 30, 101)),
         ("flat", C.EXACT_2D, (3, 38, 5, 66))]


@pytest.mark.parametrize("name,spacing,box", BOXES, ids=_id)
def test_exact_spacings_through_a_box_cut_on_every_side(name, spacing, box):
    lab = C.volume(name)
    assert all(box[2 * a] > 0 and box[2 * a + 1] < lab.shape[a] for a in range(lab.ndim))
    full = (0, 1) + box if lab.ndim == 2 else box
    shape3 = (1,) + lab.shape if lab.ndim == 2 else lab.shape
    sub_shape = tuple(full[2 * a + 1] - full[2 * a] for a in range(3))
    for mode, label, labels, _ in C.predicates(lab):
        wi, wd = C.oracle(name, spacing, mode, box)
        z, y, x = np.unravel_index(np.maximum(wi.reshape(sub_shape), 0), sub_shape)
        wi_full = np.where(wi.reshape(sub_shape) >= 0,
                           ((z + full[0]) * shape3[1] + (y + full[2])) * shape3[2] + (x + full[4]), -1)
        got_i, got_d = _transform(lab, mode, spacing, label, labels, box=list(full))
        assert got_i.shape == wi.shape
        assert np.array_equal(got_i, wi_full.reshape(wi.shape)), (mode, int((got_i != wi_full.reshape(wi.shape)).sum()))
        _assert_bits(got_d, wd, mode)


# ------------------------------------------------------------------ (b) exact spacings: the six label operations
@pytest.mark.parametrize("name,spacing,radius,applied", C.LABEL_CASES, ids=_id)
def test_exact_spacings_label_operations_on_every_voxel(name, spacing, radius, applied):
    lab = C.volume(name)
    applied = None if applied is None else list(applied)
    got, want = _six(_m(), lab, radius, spacing, applied), _six(ref, lab, radius, spacing, applied)
    for op in want:
        assert got[op].dtype == lab.dtype and got[op].shape == lab.shape
        assert np.array_equal(got[op], want[op]), (op, int((got[op] != want[op]).sum()))
    assert not np.array_equal(want["expand"], lab) and not np.array_equal(want["erode"], lab)


# ------------------------------------------------------------------ (c) inexact spacings: the two-tier rule
@pytest.mark.parametrize("name,spacing", C.inexact_pairs(), ids=_id)
def test_inexact_spacings_two_tier_rule_on_every_voxel(name, spacing):
    """Where no two features are told apart by rounding alone (relative 1e-9) the device names the oracle's
    feature and its distance bit for bit; elsewhere it names a feature within 1e-9 of the minimum and the
    distance of the feature it names (or the oracle's)."""
    lab = C.volume(name)
    sp3 = ref.spacing3(spacing, lab.ndim)
    shape3 = (1,) + lab.shape if lab.ndim == 2 else lab.shape
    gz, gy, gx = np.indices(shape3)
    for mode, label, labels, feature in C.predicates(lab):
        if not C.fits_brute(name, mode):
            continue
        near = ref.near_tie(feature, spacing)
        print(f"{mode}: near-tie share {near.mean():.2e}")
        assert near.mean() <= C.NEAR_TIE_CAP, mode                    # before the device is asked
        want_i, want_d = C.oracle(name, spacing, mode)
        got_i, got_d = _transform(lab, mode, spacing, label, labels)
        clear = ~near
        assert np.array_equal(got_i[clear], want_i[clear]), (mode, int((got_i[clear] != want_i[clear]).sum()))
        want32 = want_d.astype(np.float32)
        assert np.array_equal(got_d[clear].view(np.int32), want32[clear].view(np.int32)), mode
        assert got_i.min() >= 0 and got_i.max() < lab.size and feature.reshape(-1)[got_i].all(), mode
        iz, iy, ix = np.unravel_index(got_i.reshape(shape3), shape3)
        at_index = ref.dist_sq(gz - iz, gy - iy, gx - ix, sp3).reshape(lab.shape)
        assert np.all(np.abs(at_index - want_d) <= ref.REL * want_d), mode
        assert np.all((got_d == at_index.astype(np.float32)) | (got_d == want32)), mode


def test_in_plane_order_is_exact_when_sy_equals_sx():
    """thick slices: two features of one plane 85 voxel units away, (-6, 7) and (9, 2); the smaller raster
    index wins although the f64 in-plane sums differ in the last bit the other way"""
    lab, spacing, voxel, winner = C.pythagorean_case()
    want_i, want_d = ref.nearest_brute(lab != 0, spacing)
    clear = ~ref.near_tie(lab != 0, spacing)
    assert clear[voxel] and want_i[voxel] == winner
    got_i, got_d = _transform(lab, "FT_NONZERO", spacing)
    assert got_i[voxel] == winner
    assert np.array_equal(got_i[clear], want_i[clear])
    _assert_bits(got_d[clear], want_d[clear], "distance")
    assert _m().nearest_label(lab, spacing)[voxel] == 4


def test_clinical_spacing_label_operations():
    """thick slices, 5.0 x 0.7 x 0.7: the label operations on every voxel the oracle does not flag; the host
    tests hold the flagged share of this case below half the cap ``_check_general`` asserts"""
    _check_general(C.volume("clinical"), C.CLINICAL, C.CLINICAL_RADIUS, C.CLINICAL_APPLIED)


# ------------------------------------------------------------------ (d) P1 beyond one pass of its grid
def test_first_pass_takes_a_second_trip_through_its_grid():
    """2100 x 2000 rows of 2 voxels: 4 200 000 rows against the 4 194 304 one pass of the capped grid covers, so
    the last 5696 rows are done in a second trip.  Unit spacing; the oracle is scipy's transform, so the tie
    rule is not checked here."""
    from scipy import ndimage
    shape = (2100, 2000, 2)
    rows_per_pass = (1 << 20) * 4
    assert rows_per_pass < shape[0] * shape[1] and (shape[0] * shape[1]) % rows_per_pass
    rs = np.random.RandomState(31)
    feature = rs.random_sample(shape) < 1e-3
    second = feature.reshape(-1, 2)[rows_per_pass:]
    assert second.any() and not second.all() and second.any(axis=1).sum() >= 5
    lab = feature.astype(np.uint8)
    want = np.rint(ndimage.distance_transform_edt(~feature) ** 2).astype(np.int64)
    got_i, got_d = _transform(lab, "FT_NONZERO", None)
    assert np.array_equal(got_d, want.astype(np.float32)) and want.max() < 1 << 24
    assert got_i.min() >= 0 and got_i.max() < feature.size and feature.reshape(-1)[got_i].all()
    iz, iy, ix = np.unravel_index(got_i.astype(np.int64), shape)
    gz, gy, gx = np.meshgrid(*[np.arange(s, dtype=np.int64) for s in shape], indexing="ij", sparse=True)
    assert np.array_equal((gz - iz) ** 2 + (gy - iy) ** 2 + (gx - ix) ** 2, want)


# ------------------------------------------------------------------ (e) labels outside the table
# int32 values outside 0 .. 65535: negative, the first value past the table, values whose low 16 bits are a label
# of the table (2, 5, 65535), and the ends of the type
OUTSIDE32 = [-1, -3, -65534, -(1 << 31), 65536, 65538, 65541, 70000, (1 << 31) - 1]


@pytest.mark.parametrize("dtype,outside", [(np.int16, [-1, -3, -32768]), (np.int32, OUTSIDE32)], ids=["int16", "int32"])
def test_labels_outside_the_table_are_not_features(dtype, outside):
    """the table also holds every non-zero entry a wrapped value would hit (its low 16 bits), so a label
    outside 0 .. 65535 that is looked up at all shows as a feature"""
    spacing = C.EXACT_3D[0]
    rs = np.random.RandomState(41)
    lab = ref.scattered(C.DEFAULT, 0.03, 42, 5, dtype)
    spots = rs.random_sample(lab.shape) < 0.03
    lab[spots] = rs.choice(np.asarray(outside, dtype), size=int(spots.sum()))
    inside = [2, 5]
    if dtype == np.int32:
        inside.append(65535)
        lab[rs.random_sample(lab.shape) < 0.005] = 65535
    wrapped = sorted({v & 0xFFFF for v in outside} - {0})
    assert all((lab == v).any() for v in outside + inside)
    assert not np.isin(lab, [v for v in wrapped if v not in inside]).any()      # no voxel holds those by right
    feature = np.isin(lab, inside)
    want_i, want_d = ref.nearest_brute(feature, spacing)
    got_i, got_d = _transform(lab, "FT_TABLE", spacing, labels=inside + wrapped)
    assert np.array_equal(got_i, want_i), int((got_i != want_i).sum())
    _assert_bits(got_d, want_d, "table")
    for label in (-3, -1):
        for mode, mask in (("FT_EQUAL", lab == label), ("FT_NOT_EQUAL", lab != label)):
            want_i, want_d = (ref.nearest_brute if mode == "FT_EQUAL" else ref.nearest_separable)(mask, spacing)
            got_i, got_d = _transform(lab, mode, spacing, label=label)
            assert np.array_equal(got_i, want_i), (mode, label)
            _assert_bits(got_d, want_d, (mode, label))


# ------------------------------------------------------------------ (f) repeatability
def test_three_calls_give_identical_bits():
    lab = C.volume("scattered_hi")
    ops = _ops()
    first = None
    for _ in range(3):
        index, dist = ops.feature_transform(_dev(lab), ops.FT_NONZERO, C.CLINICAL, with_dist=True)
        labels = _m().dilate_labels(lab, 2.0, C.CLINICAL)
        torch.cuda.synchronize()
        now = (index.cpu().numpy(), dist.cpu().numpy().view(np.int32), labels)
        if first is None:
            first = now
        assert all(np.array_equal(a, b) for a, b in zip(first, now))
