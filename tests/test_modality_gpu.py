"""N4 bias-field correction, Otsu, shrink and CT scaling (csrc/n4.hip, image/modality.py) on the MI355X
against the float64 numpy oracle of tests/helpers/n4_ref.py.  The bounds on f64 quantities are 1000 x the
deviation between the oracle's two forms and the f32 evaluation's are 4 x that of its numpy restatement
(tests/helpers/n4_cases.py; DESIGN §12, "Tests"); tests/test_modality_sweep_gpu.py covers the other paths."""
import subprocess
import sys
from pathlib import Path

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
ROOT = Path(__file__).resolve().parent.parent


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _logs(img, mask):
    v = ref.fit_set(img, mask)
    return np.where(v, np.log(np.where(v, img.astype(np.float64), 1.0)), np.nan), v


def test_otsu_counts_threshold_and_mask_exact():
    rng = np.random.default_rng(0)
    img, _, _ = ref.phantom((23, 30, 27), seed=3)
    img[0, 0, :5] = np.nan
    img[1, 2, 3] = np.inf
    for x in (img, img[5], rng.normal(size=(17, 19)).astype(np.float32)):
        counts, stats = ops.otsu(_dev(x), 200)
        rc, lo, w = ref.otsu_counts(x, 200)
        mask, thr, _ = ref.otsu_threshold(x)
        assert np.array_equal(counts.cpu().numpy(), rc)
        s = stats.cpu().numpy()
        assert s[0] == lo and s[1] == w and s[2] == thr and s[3] == np.isfinite(x).sum()
        got = modality.otsu_threshold(Image(x))
        assert got.data.dtype == torch.uint8 and not got.data.is_cuda
        assert np.array_equal(got.numpy(), mask)


@pytest.mark.parametrize("shape", [(20, 33, 18), (9, 10, 11), (31, 16)])
def test_shrink_bit_exact_with_user_mask(shape):
    rng = np.random.default_rng(1)
    x = rng.normal(50, 20, size=shape).astype(np.float32)
    m = (rng.random(shape) > 0.4).astype(np.uint8)
    for f in (1, 2, 3, 4, 5):
        img, msk, lg = ops.n4_shrink(_dev(x), [f] * len(shape), mask=_dev(m), want_log=True)
        assert np.array_equal(img.cpu().numpy(), ref.shrink(x, f))
        assert np.array_equal(msk.cpu().numpy(), ref.shrink(m, f))
        want, _ = _logs(ref.shrink(x, f), ref.shrink(m, f))
        got = lg.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=1e-15, atol=0)
        im = Image(x, spacing=[0.5, 1.0, 2.0][:len(shape)], origin=[1.0, 2.0, 3.0][:len(shape)])
        s = modality.shrink(im, f)
        ns, sp, org = ref.shrink_geometry(im.GetSize(), im.spacing, im.origin, im.direction, f)
        assert s.GetSize() == tuple(ns) and s.spacing == tuple(sp) and s.origin == tuple(org)
        assert np.array_equal(s.numpy(), ref.shrink(x, f))


def test_sharpening_step_against_oracle(record_property):
    s = cases.sharpen_case("seed2", cases.DEFAULT_SETTINGS)   # phantom (40, 48, 44), seed 2, Otsu mask
    assert s.L.shape == (40, 48, 44)
    E, S = ops.n4_sharpen(_dev(s.L))
    cases.check(record_property, "E", E, s.E, s.b_E)
    cases.check(record_property, "S", S, cases.full(s.S, s.valid), s.b_S)


@pytest.mark.parametrize("shape,spans", [((24, 30, 27), 1), ((24, 30, 27), 2), ((24, 30, 27), 4),
                                         ((24, 30, 27), 8), ((64, 64, 64), 32), ((1, 37, 41), 4),
                                         ((10, 12, 9), 16)])
def test_bspline_fit_against_oracle(shape, spans, record_property):
    rng = np.random.default_rng(spans)
    r = rng.normal(size=shape)
    valid = rng.random(shape) > 0.3
    r_nan = np.where(valid, r, np.nan)
    got = ops.n4_bspline_fit(_dev(r_nan), spans)
    want = ref.ba_fit(r, valid, spans)
    # one BA step: 1000 x the relative deviation between the oracle's separable and point-by-point forms
    # at these spans on a small grid
    d = cases.ba_deviation(spans, two_d=shape[0] == 1)
    record_property("d_ba_forms_relative", d)
    cases.check(record_property, "lattice", got, want, cases.bound(d, 1.0) * np.abs(want).max())


def test_refine_then_evaluate_equals_coarse_field(record_property):
    rng = np.random.default_rng(4)
    for lat in (rng.normal(0, 0.3, (4, 5, 7)), rng.normal(0, 0.3, (1, 6, 5))):
        fine = ops.n4_refine(_dev(lat))
        want_fine = ref.refine(lat)
        # at most three products and additions of exact coefficients per axis: a few ulps of max |lattice|
        assert np.abs(fine.cpu().numpy() - want_fine).max() <= 16 * 2.0 ** -53 * np.abs(lat).max()
        shape = (13, 22, 17) if lat.shape[0] > 1 else (22, 17)
        shape3 = (1,) + shape if len(shape) == 2 else shape
        a = ops.n4_evaluate(fine, shape).cpu().numpy()
        bound, _ = cases.evaluate_bound(want_fine, shape3)
        # the coarse lattice's field: refinement preserves it to 1e-12 (tests/test_modality_host.py)
        cases.check(record_property, "field", a, ref.evaluate(lat, shape3).reshape(shape), bound + 1e-12)


def test_full_resolution_evaluation_and_division(record_property):
    rng = np.random.default_rng(5)
    lat = rng.normal(0, 0.3, (11, 11, 11))
    shape = (97, 130, 161)
    x = rng.uniform(1, 100, shape).astype(np.float32)
    f = ops.n4_evaluate(_dev(lat), shape).cpu().numpy()
    want = ref.evaluate(lat, shape)
    cases.check(record_property, "field", f, want, cases.evaluate_bound(lat, shape)[0])
    y = ops.n4_evaluate(_dev(lat), shape, _dev(x)).cpu().numpy()
    cases.check_divided(record_property, "divided", y, x, lat, 0.0)
    lat2 = rng.normal(0, 0.3, (1, 7, 7))
    f2 = ops.n4_evaluate(_dev(lat2), (64, 48)).cpu().numpy()
    cases.check(record_property, "field_2d", f2, ref.evaluate(lat2, (1, 64, 48))[0],
                cases.evaluate_bound(lat2, (1, 64, 48))[0])
    # a CPU-side Image: the field comes back on the CPU
    filt = modality.N4BiasFieldCorrectionImageFilter()
    filt._lattice = _dev(lat)
    im = filt.GetLogBiasFieldAsImage(Image(np.zeros((33, 40, 64), np.float32)))
    assert not im.data.is_cuda
    cases.check(record_property, "field_cpu_image", im.numpy(), ref.evaluate(lat, (33, 40, 64)),
                cases.evaluate_bound(lat, (33, 40, 64))[0])


def _phantom_case(shape=(48, 56, 52), seed=7):
    img, b, cls = ref.phantom(shape, seed=seed)
    return img, b, cls


def test_bias_correct_log_field_against_oracle_fixed_iterations(record_property):
    img, _, _ = _phantom_case()
    c = cases.fit_case("fixed-654")   # the phantom and its Otsu mask shrunk by 2, iterations (6, 5, 4)
    si, sm, lat_r = c.img, c.mask, c.lattice
    filt = modality.N4BiasFieldCorrectionImageFilter()
    filt.SetMaximumNumberOfIterations([6, 5, 4])
    filt.SetConvergenceThreshold(0.0)
    out = filt.Execute(Image(si), Image(sm))
    assert filt.GetElapsedIterations() == c.elapsed == [6, 5, 4]
    cases.check_fit(record_property, c, filt.GetLogBiasFieldControlPointLattice(), filt.GetElapsedIterations(),
                    filt.GetCurrentConvergenceMeasurement())
    full = filt.GetLogBiasFieldAsImage(Image(img)).numpy()
    want = ref.evaluate(lat_r, img.shape)
    cases.check(record_property, "full_field", full, want, cases.evaluate_bound(lat_r, img.shape)[0] + c.b_lattice)
    cases.check_divided(record_property, "output", out.numpy(), si, lat_r, c.b_lattice)


def test_bias_correct_default_threshold_iteration_counts(record_property):
    # default threshold 0.001; the oracle's CV stays at or above 0.00165 through every capped level
    # (level 2: 0.0252, 0.0255, 0.0191, 0.0073, 0.0030, 0.00165), so the counts are the caps
    c = cases.fit_case("seed11-436")   # phantom (40, 44, 36), seed 11, shrunk by 2, iterations (4, 3, 6)
    filt = modality.N4BiasFieldCorrectionImageFilter()
    filt.SetMaximumNumberOfIterations([4, 3, 6])
    filt.Execute(Image(c.img), Image(c.mask))
    assert filt.GetElapsedIterations() == c.elapsed == [4, 3, 6]
    cases.check_fit(record_property, c, filt.GetLogBiasFieldControlPointLattice(), filt.GetElapsedIterations(),
                    filt.GetCurrentConvergenceMeasurement())


def test_bias_correct_end_to_end_and_repeatable(record_property):
    img, b, cls = _phantom_case()
    im = Image(img, spacing=(1.0, 1.2, 0.8))
    # default threshold: level 2 stops after 5 iterations (oracle CV 0.00120, then 0.00095)
    a = modality.bias_correct(im, shrink_factor=2, num_fitting_levels=3, num_iterations=8)
    c = modality.bias_correct(im, shrink_factor=2, num_fitting_levels=3, num_iterations=8)
    assert a.data.dtype == torch.float32 and not a.data.is_cuda and a.spacing == im.spacing
    assert torch.equal(a.data, c.data)
    mask, _, _ = ref.otsu_threshold(img)
    e = cases.fit_case("end-to-end-888")   # the same phantom and mask shrunk by 2, iterations (8, 8, 8)
    assert e.elapsed == [8, 8, 5]
    cases.check_divided(record_property, "output", a.numpy(), img, e.lattice, e.b_lattice)
    for k in (1, 2, 3):
        s = cls == k
        assert a.numpy()[s].std() / a.numpy()[s].mean() < img[s].std() / img[s].mean()
    # with a user mask (an int16 mask: label 1 only)
    m16 = (mask.astype(np.int16) * 1)
    d = modality.bias_correct(Image(img), Image(m16), shrink_factor=2, num_fitting_levels=2, num_iterations=3)
    assert torch.isfinite(d.data).all()


def test_value_errors():
    z = np.zeros((8, 9, 10), np.float32)
    with pytest.raises(ValueError):
        modality.bias_correct(Image(z), Image(np.ones_like(z, dtype=np.uint8)), shrink_factor=1)
    c = np.full((8, 9, 10), 7.0, np.float32)
    with pytest.raises(ValueError):
        modality.bias_correct(Image(c), Image(np.ones_like(c, dtype=np.uint8)), shrink_factor=1)
    with pytest.raises(ValueError):
        modality.N4BiasFieldCorrectionImageFilter().SetSplineOrder(2)


def _ulps(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("shape,dtype", [((17, 23, 29), np.float32), ((41, 37), np.float32),
                                         ((12, 15, 16), np.int16)])
def test_scale_clamp_ct(shape, dtype):
    rng = np.random.default_rng(6)
    x = rng.uniform(-1500, 3500, shape)
    x = np.round(x).astype(dtype) if dtype == np.int16 else x.astype(np.float32)
    med = ref.median_filter(x.astype(np.float32))
    got_med_scaled = modality.scale_clamp_ct(Image(x))
    assert got_med_scaled.data.dtype == torch.float32 and not got_med_scaled.data.is_cuda
    want = ((np.clip(med, -1100, 3100) + 1100) * 255 / 4200).astype(np.float32)
    assert _ulps(got_med_scaled.numpy(), want).max() <= 1
    # the median itself, bit-exact: outside the clamp range scale_clamp_ct is constant, so probe it inside
    y = rng.uniform(-1000, 3000, shape).astype(np.float32)
    got = ops.ct_scale(_dev(y)).cpu().numpy()
    m = ref.median_filter(y).astype(np.float32)
    assert np.array_equal(got, (m + np.float32(1100)) * np.float32(255.0 / 4200.0))
    back = modality.unscale_ct(got_med_scaled).numpy()
    np.testing.assert_allclose(back, np.clip(med, -1100, 3100), atol=1e-3)


def test_cli_n4_and_ct_scale(tmp_path):
    from segmantic_amd.data.imageio import read_image, write_image
    img, _, _ = ref.phantom((20, 24, 22), seed=9)
    ct = np.random.default_rng(2).uniform(-1500, 3500, (10, 12, 14)).astype(np.float32)
    aff = np.diag([0.8, 0.9, 1.1, 1.0])
    (tmp_path / "mr").mkdir()
    (tmp_path / "ct").mkdir()
    write_image(tmp_path / "mr" / "a.nii.gz", img, aff)
    write_image(tmp_path / "ct" / "b.nii.gz", ct, aff)
    script = str(ROOT / "scripts" / "modality.py")
    r = subprocess.run([sys.executable, script, "n4", str(tmp_path / "mr"), str(tmp_path / "mr_out"),
                        "--shrink-factor", "2", "--levels", "2", "--iterations", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, gaff = read_image(tmp_path / "mr_out" / "a.nii.gz")
    arr, _ = read_image(tmp_path / "mr" / "a.nii.gz")
    want = modality.bias_correct(Image(np.asarray(arr, np.float32)), shrink_factor=2, num_fitting_levels=2,
                                 num_iterations=3).numpy()
    assert np.array_equal(np.asarray(got, np.float32), want) and np.allclose(gaff, aff)
    r = subprocess.run([sys.executable, script, "ct-scale", str(tmp_path / "ct"), str(tmp_path / "ct_out")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, gaff = read_image(tmp_path / "ct_out" / "b.nii.gz")
    arr, _ = read_image(tmp_path / "ct" / "b.nii.gz")
    assert np.array_equal(np.asarray(got, np.float32),
                          modality.scale_clamp_ct(Image(np.asarray(arr, np.float32))).numpy())
    assert np.allclose(gaff, aff)
