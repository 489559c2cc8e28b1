"""csrc/n4.hip beyond one grid pass and beyond the default settings ("Tests"): every grid-stride
loop makes a second pass, the sharpening runs at P = 4 .. 1024, four levels, a complete 2-D fit, levels that
stop before their cap, fit-set exclusions, the non-vector Otsu and evaluation kernels, per-axis shrink factors.
The reference is the float64 numpy oracle of tests/helpers/n4_ref.py; the bounds on f64 quantities are
1000 x D_case, the deviation between the oracle's FFT form and the kernel's arithmetic restated in numpy
(tests/helpers/n4_cases.py, measured on the CPU by tests/test_modality_host.py)."""
import functools

import numpy as np
import pytest
import torch

from segmantic_amd import ops
from segmantic_amd.image import modality
from segmantic_amd.image.processing import Image
from tests.helpers import n4_cases as cases
from tests.helpers import n4_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

RED_PASS = 1024 * 256          # threads of the N4 reduction kernels (n4_eval, n4_hist, n4_sharpened)
OTSU_PASS = 2048 * 256 * 4     # floats per pass of the vector Otsu kernels
GATHER_PASS = 65536 * 256      # voxels per pass of n4_shrink and ct_scale


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _offset_view(a):
    """a contiguous device copy of `a` whose storage starts one element into an allocation: aligned to the
    element only, which selects the non-vector kernels"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


# ------------------------------------------------------------------ 1. reduction kernels past one pass
def test_reduction_kernels_make_a_second_pass(record_property):
    c = cases.fit_case("big")
    assert c.img.size == 332640 > RED_PASS
    L, v = cases.log_image(c.img, c.mask)
    Ld = _dev(L)
    lat, field, elapsed, cv = ops.n4_fit(Ld, c.iterations, threshold=0.0, want_field=True)
    assert np.array_equal(c.field, ref.evaluate(c.lattice, c.img.shape))
    cases.check_fit(record_property, c, lat, elapsed, cv, field)
    lat2, field2, elapsed2, cv2 = ops.n4_fit(Ld, c.iterations, threshold=0.0, want_field=True)
    assert torch.equal(lat, lat2) and torch.equal(field, field2) and elapsed == elapsed2 and cv == cv2
    s = cases.sharpen_case("big", cases.DEFAULT_SETTINGS)
    E, S = ops.n4_sharpen(Ld)
    cases.check(record_property, "big_E", E, s.E, s.b_E)
    cases.check(record_property, "big_S", S, cases.full(s.S, v), s.b_S)
    E2, S2 = ops.n4_sharpen(Ld)
    assert torch.equal(E, E2) and torch.equal(S.nan_to_num(7.0), S2.nan_to_num(7.0))


# ------------------------------------------------------------------ 2. sharpening sizes
@pytest.mark.parametrize("settings", cases.SHARPEN_SETTINGS, ids=lambda s: "bins%d" % s[0])
def test_sharpening_and_fit_at_other_settings(settings, record_property):
    bins, fwhm, noise, cp = settings
    s = cases.sharpen_case("seed7", settings)
    Ld = _dev(s.L)
    E, S = ops.n4_sharpen(Ld, bins, fwhm, noise)
    cases.check(record_property, "E", E, s.E, s.b_E)
    cases.check(record_property, "S", S, cases.full(s.S, s.valid), s.b_S)
    if bins == 2:
        # no fit: at two bins the sharpened value is U itself up to rounding, the residual is noise and the
        # oracle's two forms stop at different iterations (test_modality_host.test_fit_at_two_bins_is_rounding_noise)
        return
    c = cases.fit_case("bins%d" % bins)
    lat, _, elapsed, cv = ops.n4_fit(Ld, c.iterations, cp, bins, fwhm, noise, 0.0)
    assert tuple(lat.shape) == c.lattice.shape
    cases.check_fit(record_property, c, lat, elapsed, cv)


def test_filter_setters_reach_the_kernels(record_property):
    c = cases.fit_case("bins257")
    bins, fwhm, noise, cp = c.settings
    filt = modality.N4BiasFieldCorrectionImageFilter()
    filt.SetMaximumNumberOfIterations(list(c.iterations))
    filt.SetConvergenceThreshold(0.0)
    filt.SetNumberOfHistogramBins(bins)
    filt.SetBiasFieldFullWidthAtHalfMaximum(fwhm)
    filt.SetWienerFilterNoise(noise)
    filt.SetNumberOfControlPoints(cp)
    out = filt.Execute(Image(c.img), Image(c.mask))
    cases.check_fit(record_property, c, filt.GetLogBiasFieldControlPointLattice(), filt.GetElapsedIterations(),
                    filt.GetCurrentConvergenceMeasurement(), key="setters")
    cases.check_divided(record_property, "setters_output", out.numpy(), c.img, c.lattice, c.b_lattice)


# ------------------------------------------------------------------ 3. four levels and 2-D
def test_four_levels(record_property):
    c = cases.fit_case("levels4")
    L, _ = cases.log_image(c.img, c.mask)
    lat, field, elapsed, cv = ops.n4_fit(_dev(L), c.iterations, threshold=0.0, want_field=True)
    assert tuple(lat.shape) == (11, 11, 11)
    cases.check_fit(record_property, c, lat, elapsed, cv, field)


def test_complete_two_dimensional_fit(record_property):
    c = cases.fit_case("2d")
    assert c.img.shape == (90, 110)
    L, _ = cases.log_image(c.img, c.mask)
    lat, field, elapsed, cv = ops.n4_fit(_dev(L), c.iterations, threshold=0.0, want_field=True)
    assert tuple(lat.shape) == (1, 7, 7) and tuple(field.shape) == (90, 110)
    cases.check_fit(record_property, c, lat, elapsed, cv, field)
    # bias_correct on a 2-D Image: Otsu, shrink by 2, three levels of four iterations, default threshold
    b = cases.fit_case("2d-bias-correct")
    img, _ = cases.fit_input("2d")
    out = modality.bias_correct(Image(img, spacing=(0.9, 1.1)), shrink_factor=2, num_fitting_levels=3,
                                num_iterations=4)
    assert out.data.dtype == torch.float32 and tuple(out.data.shape) == (90, 110) and out.spacing == (0.9, 1.1)
    cases.check_divided(record_property, "2d_bias_correct", out.numpy(), img, b.lattice, b.b_lattice)


# ------------------------------------------------------------------ 4. stopping before the cap
def test_levels_stop_before_their_cap(record_property):
    c = cases.fit_case("stop")
    assert sum(e < cap for e, cap in zip(c.elapsed, c.iterations)) >= 2
    filt = modality.N4BiasFieldCorrectionImageFilter()
    filt.SetMaximumNumberOfIterations(list(c.iterations))
    filt.SetConvergenceThreshold(c.threshold)
    filt.Execute(Image(c.img), Image(c.mask))
    assert filt.GetConvergenceThreshold() == c.threshold
    assert filt.GetElapsedIterations() == c.elapsed == [3, 15, 5]
    cases.check_fit(record_property, c, filt.GetLogBiasFieldControlPointLattice(), filt.GetElapsedIterations(),
                    filt.GetCurrentConvergenceMeasurement())


# ------------------------------------------------------------------ 5. fit-set exclusions
def test_fit_set_exclusions(record_property):
    img, mask = cases.poisoned_phantom()
    c = cases.fit_case("poisoned")
    want, v = cases.log_image(c.img, c.mask)
    inside = c.mask == 1
    with np.errstate(invalid="ignore"):
        kinds = [np.isnan(c.img), np.isposinf(c.img), c.img == 0, c.img < 0, np.isneginf(c.img)]
    for k in kinds:  # every kind of excluded voxel survives the shrink, inside the mask
        assert (k & inside).sum() >= 2 and not (k & v).any()
    si, sm, lg = ops.n4_shrink(_dev(img), [2, 2, 2], mask=_dev(mask), want_log=True)
    assert np.array_equal(si.cpu().numpy(), c.img, equal_nan=True) and np.array_equal(sm.cpu().numpy(), c.mask)
    got = lg.cpu().numpy()
    assert np.array_equal(np.isnan(got), ~v)
    assert (np.abs(got[v] - want[v]) <= 2 * np.spacing(np.abs(want[v]))).all()
    lat, field, elapsed, cv = ops.n4_fit(lg, c.iterations, threshold=0.0, want_field=True)
    cases.check_fit(record_property, c, lat, elapsed, cv, field)
    # the same through the filter: the image's own NaN / Inf / non-positive voxels leave the fit set
    filt = modality.N4BiasFieldCorrectionImageFilter()
    filt.SetMaximumNumberOfIterations(list(c.iterations))
    filt.SetConvergenceThreshold(0.0)
    filt.Execute(Image(c.img), Image(c.mask))
    assert np.array_equal(filt.GetLogBiasFieldControlPointLattice(), lat.cpu().numpy())


# ------------------------------------------------------------------ 6. Otsu
@functools.lru_cache(maxsize=None)
def _otsu_volume():
    rng = np.random.default_rng(60)
    x = rng.normal(10.0, 3.0, (129, 127, 131)).astype(np.float32)
    x[40:60] = 12.25                      # whole waves in one bin: the wave-uniform count
    x[3, 5, 7:90] = np.nan
    x[100, 2:60, 9] = np.inf
    x[101, 2:60, 9] = -np.inf
    x[-1, -1, -1] = 31.0                  # the ragged tail's one element decides the maximum
    return x


def _check_otsu(x_dev, x, bins=200):
    counts, stats = ops.otsu(x_dev, bins)
    rc, lo, w = ref.otsu_counts(x, bins)
    assert np.array_equal(counts.cpu().numpy(), rc)
    s = stats.cpu().numpy()
    thr = ref.otsu_pick(rc, lo, w)
    assert s[0] == lo and s[1] == w and s[2] == thr and s[3] == np.isfinite(x).sum()
    return thr


def test_otsu_past_one_pass_vector_and_scalar_kernels():
    x = _otsu_volume()
    assert x.size == 2146173 > OTSU_PASS and x.size % 4 == 1
    assert x[np.isfinite(x)].max() == 31.0 and x[-1, -1, -1] == 31.0
    xd = _dev(x)
    assert xd.data_ptr() % 16 == 0
    thr = _check_otsu(xd, x)
    _check_otsu(_offset_view(x), x)
    mask, thr_r, _ = ref.otsu_threshold(x)
    got = modality.otsu_threshold(Image(xd))
    assert got.threshold == thr == thr_r and np.array_equal(got.numpy(), mask)


@pytest.mark.parametrize("bins", [2, 64, 256, 512])
def test_otsu_bins_and_values(bins):
    img, _, _ = ref.phantom((23, 30, 27), seed=3)
    img[0, 0, :5] = np.nan
    _check_otsu(_dev(img), img, bins)
    _check_otsu(_offset_view(img), img, bins)
    for inside, outside in ((0, 1), (1, 0), (3, 200)):
        mask, thr, _ = ref.otsu_threshold(img, inside, outside, bins)
        got = modality.otsu_threshold(Image(img), inside_value=inside, outside_value=outside, bins=bins)
        assert got.threshold == thr and np.array_equal(got.numpy(), mask)


def test_otsu_corner_cases():
    for vals in ([5.0], [2.0, -1.0], [0.5, 3.0, 1.0], [7.0] * 1000, [np.nan, 4.0, np.inf, 4.0, 4.0]):
        x = np.asarray(vals, np.float32)
        for xd in (_dev(x), _offset_view(x)):
            thr = _check_otsu(xd, x)
        for inside, outside in ((0, 1), (1, 0)):
            mask, thr_r, _ = ref.otsu_threshold(x[None], inside, outside)
            got = modality.otsu_threshold(Image(x[None]), inside, outside)
            assert thr == thr_r == got.threshold and np.array_equal(got.numpy(), mask)
    # an all-equal image has bin width 0: every count in bin 0, threshold = the value, nothing above it
    counts, stats = ops.otsu(_dev(np.full((9, 11), 7.0, np.float32)))
    assert counts.cpu().numpy()[0] == 99 and counts.cpu().numpy()[1:].sum() == 0
    assert stats.cpu().numpy().tolist() == [7.0, 0.0, 7.0, 99.0]


# ------------------------------------------------------------------ 7. shrink
@pytest.mark.parametrize("factors", [(1, 2, 3), (3, 1, 2), (25, 2, 1), (2, 40, 19)])
def test_shrink_per_axis_factors(factors):
    rng = np.random.default_rng(70)
    shape = (20, 33, 18)
    x = rng.normal(50, 20, size=shape).astype(np.float32)
    m = (rng.random(shape) > 0.4).astype(np.uint8)
    f = list(factors)   # array order [z, y, x]
    img, msk, lg = ops.n4_shrink(_dev(x), f, mask=_dev(m), want_log=True)
    assert tuple(img.shape) == tuple(max(1, n // fa) for n, fa in zip(shape, f))
    assert np.array_equal(img.cpu().numpy(), ref.shrink(x, f)) and np.array_equal(msk.cpu().numpy(), ref.shrink(m, f))
    want, v = cases.log_image(ref.shrink(x, f), ref.shrink(m, f))
    got = lg.cpu().numpy()
    assert np.array_equal(np.isnan(got), ~v)
    assert (np.abs(got[v] - want[v]) <= 2 * np.spacing(np.abs(want[v]))).all()
    im = Image(x, spacing=[0.5, 1.0, 2.0], origin=[1.0, 2.0, 3.0])
    f_xyz = f[::-1]
    s = modality.shrink(im, f_xyz)
    ns, sp, org = ref.shrink_geometry(im.GetSize(), im.spacing, im.origin, im.direction, f_xyz)
    # the same f64 expression on both sides: exact, so the (x, y, z) reversal cannot hide in a tolerance
    assert s.GetSize() == tuple(ns) and s.spacing == tuple(sp) and s.origin == tuple(org)
    assert np.array_equal(s.numpy(), ref.shrink(x, f))


@functools.lru_cache(maxsize=None)
def _gather_volume():
    """(258, 256, 255) f32 in [-1500, 3500): one voxel more than a pass of n4_shrink / ct_scale in plane 257"""
    rng = np.random.default_rng(80)
    x = rng.random((258, 256, 255), dtype=np.float32) * np.float32(5000.0) - np.float32(1500.0)
    assert x.size == 16842240 > GATHER_PASS and GATHER_PASS // (256 * 255) == 257
    x[:2, :40] = -1400.0          # medians below and above the clamp range, in the first and the last slab
    x[1, 100:140] = 3300.5
    x[256:, 200:] = 3400.0
    return x


def test_shrink_past_one_pass():
    x = _gather_volume().copy()
    x[0, 0, :9] = np.nan
    x[257, 255, 250:] = np.inf     # in the second pass
    x[257, 200, 100:110] = np.nan
    rng = np.random.default_rng(81)
    m = (rng.random(x.shape, dtype=np.float32) > 0.25).astype(np.uint8)
    m[257, 200:, :] = 1
    img, msk, lg = ops.n4_shrink(_dev(x), [1, 1, 1], mask=_dev(m), want_log=True)
    assert np.array_equal(img.cpu().numpy(), x, equal_nan=True)
    assert np.array_equal(msk.cpu().numpy(), m)
    del img, msk
    want, v = cases.log_image(x, m)
    got = lg.cpu().numpy()
    assert v[257, 200:].any() and not v[257, 200, 100:110].any()
    assert np.array_equal(np.isnan(got), ~v)
    assert (np.abs(got[v] - want[v]) <= 2 * np.spacing(np.abs(want[v]))).all()


# ------------------------------------------------------------------ 8. CT scale past one pass
def _ulps(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def test_ct_scale_past_one_pass():
    x = _gather_volume()
    got = ops.ct_scale(_dev(x)).cpu().numpy()
    for z0, z1 in ((0, 3), (254, 258)):
        med = ref.median_filter_slab(x, z0, z1)
        m32 = med.astype(np.float32)
        assert np.array_equal(m32.astype(np.float64), med)
        inside = (med > -1100) & (med < 3100)
        assert inside.any() and not inside.all()
        # the median bit-exact: clamp and scale restated in f32 give the kernel's value, inside the clamp
        # range and outside it
        f32 = (np.clip(m32, np.float32(-1100), np.float32(3100)) + np.float32(1100)) * np.float32(255.0 / 4200.0)
        assert np.array_equal(got[z0:z1], f32)
        want = ((np.clip(med, -1100, 3100) + 1100) * 255 / 4200).astype(np.float32)
        assert _ulps(got[z0:z1], want).max() <= 1


# ------------------------------------------------------------------ 9. full-resolution evaluation
@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_full_resolution_evaluation_wide_lattice_and_scalar_division(scale, record_property):
    rng = np.random.default_rng(90)
    lat = scale * rng.normal(0, 0.3, (35, 35, 35))
    shape = (40, 36, 48)          # R = 8192 // 35 rows per block, lx close to nx, nx % 4 == 0
    x = rng.uniform(1, 100, shape).astype(np.float32)
    bound, d = cases.evaluate_bound(lat, shape)
    record_property("evaluate_f32_deviation", d)
    latd = _dev(lat)
    f = ops.n4_evaluate(latd, shape).cpu().numpy()
    cases.check(record_property, "field_f32", f, ref.evaluate(lat, shape), bound)
    record_property("bit_identical_to_evaluate_f32", bool(np.array_equal(f, ref.evaluate_f32(lat, shape))))
    cases.check_divided(record_property, "vector", ops.n4_evaluate(latd, shape, _dev(x)).cpu().numpy(), x, lat, 0.0)
    xo = _offset_view(x)
    assert xo.data_ptr() % 16 == 4 and shape[2] % 4 == 0
    cases.check_divided(record_property, "scalar", ops.n4_evaluate(latd, shape, xo).cpu().numpy(), x, lat, 0.0)
