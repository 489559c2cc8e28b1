"""The cubic B-spline and label-Gaussian resamplers (segmantic_amd/csrc/resample_hq.hip) on the
MI355X against the float64 restatement of tests/helpers/resample_hq_ref.py, which tests/test_resample_hq_host.py holds
to scipy.

Bounds.  Coefficients: 1e-11 max|x| -- the prefilter's L-infinity gain is 3 per axis, 27 in 3-D, and a few tens of f64
roundings on top give about 1e-13 max|x|; the bound leaves a hundredfold margin.  f32 output: that plus the final
rounding, 2^-24 |ref|.  Integer output: exact, except where the reference's real value lies within 1e-11 max|x| of an
integer, on at most 2 % of the voxels.  Label-Gaussian: bit equality, on cases whose hazard the host file checked.
MEASURED lines print the observed figure next to the bound (``pytest -s``)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.image import processing as P  # noqa: E402
from tests.helpers import infer_ref as R  # noqa: E402
from tests.helpers import resample_hq_ref as H  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
MAPS = {"oblique": (H.OBLIQUE, H.OBLIQUE_OUT), "upsample": (H.UPSAMPLE, H.UPSAMPLE_OUT)}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _coef_gate(name, got, x):
    vmax = float(np.abs(x).max()) if x.size else 0.0
    ref = ndimage.spline_filter(x.astype(np.float64), order=3, output=np.float64, mode="mirror")
    d = float(np.abs(got - ref).max())
    print(f"MEASURED coefficients {name}: {d:.3e} (bound {1e-11 * vmax:.3e})")
    assert got.dtype == np.float64 and got.shape == x.shape
    assert d <= 1e-11 * vmax


def _bspline_gate(name, got, x, m, out, border=False, default=0.0):
    vmax = float(np.abs(x).max())
    want, real, inside = H.bspline_resample(x, m, out, border, default)
    assert got.dtype == x.dtype
    bad = H.bspline_violations(got, real, vmax)
    if got.dtype == np.float32:
        print(f"MEASURED bspline {name}: max |diff| {np.abs(got.astype(np.float64) - real).max():.3e} "
              f"(bound {1e-11 * vmax:.3e} + 2^-24 |ref|)")
    else:
        print(f"MEASURED bspline {name}: {int((got != want).sum())} of {got.size} voxels differ")
    assert bad == [], bad
    assert np.array_equal(got[~inside], want[~inside])           # outside: the cast default, exactly
    return inside


# ------------------------------------------------------------------ B-spline
@pytest.mark.parametrize("pixel", H.PIXELS)
def test_bspline_every_pixel_type(pixel):
    x = H.image_volume(pixel)
    src = _dev(x)
    coef = ops.bspline_coefficients(src)
    _coef_gate(pixel, _host(coef), x)
    for name, (m, out) in MAPS.items():
        got = ops.resample3d_bspline(src, out, m, default=-7.5)
        inside = _bspline_gate(f"{pixel} {name}", _host(got), x, m, out, default=-7.5)
        assert inside.any() and (~inside).any()
        again = ops.resample3d_bspline(src, out, m, default=-7.5, coef=coef)
        assert torch.equal(got, again)                            # coef= gives the bits of recomputing
        bord = _host(ops.resample3d_bspline(src, out, m, default=-7.5, border=True, coef=coef))
        assert _bspline_gate(f"{pixel} {name} border", bord, x, m, out, border=True, default=-7.5).all()


def test_bspline_saturates_then_truncates():
    """a random pattern of the type's extremes overshoots between samples on both sides: the cast clamps"""
    x = (np.random.default_rng(14).integers(0, 2, H.SRC_SHAPE) * 255).astype(np.uint8)
    got = _host(ops.resample3d_bspline(_dev(x), H.OBLIQUE_OUT, H.OBLIQUE))
    _, real, inside = H.bspline_resample(x, H.OBLIQUE, H.OBLIQUE_OUT)
    assert (real[inside] < -1.0).sum() > 20 and (real[inside] > 256.0).sum() > 20
    _bspline_gate("u8 overshoot", got, x, H.OBLIQUE, H.OBLIQUE_OUT)


@pytest.mark.parametrize("shape,m,out", [
    ((1, 9, 4), H.scale_map(0.5, 0.4, 1.0, (0.1, -0.2, 0.0)), (1, 24, 9)),
    ((1, 9, 4), np.c_[H.rotation(0.2, -0.3, 0.4) @ np.diag([0.3, 0.5, 0.2]), [0.5, 1.0, -0.1]], (2, 14, 9)),   # a tilted plane
    ((7, 1, 1), H.scale_map(1.0, 1.0, 0.45, (0.0, 0.0, -0.3)), (17, 1, 1)),
    ((1, 1, 1), H.scale_map(0.3), (1, 2, 3)),
])
def test_bspline_axes_of_extent_one(shape, m, out):
    for pixel in ("float32", "int16"):
        x = H.image_volume(pixel, shape, seed=8)
        src = _dev(x)
        _coef_gate(f"{shape} {pixel}", _host(ops.bspline_coefficients(src)), x)
        inside = _bspline_gate(f"{shape} {pixel}", _host(ops.resample3d_bspline(src, out, m)), x, m, out)
        assert inside.any()


@pytest.mark.parametrize("shape", [(2, 57, 58), (3, 58, 57), (58, 2, 64), (57, 3, 65), (2, 65, 130), (130, 2, 3)])
def test_prefilter_line_lengths(shape):
    """57 is the longest line whose causal start sums the whole line, 58 the first that stops at the horizon; rows of
    64, 65 and 130 samples are one, two and three chunks of the x pass"""
    x = np.random.default_rng(9).uniform(-250.0, 250.0, shape).astype(np.float32)
    _coef_gate(str(shape), _host(ops.bspline_coefficients(_dev(x))), x)


def test_prefilter_many_rows():
    """more rows than fit one workgroup per compute unit, four rows per workgroup, the last one partly empty"""
    x = np.random.default_rng(10).integers(-1000, 1001, (67, 69, 5)).astype(np.int16)
    _coef_gate("(67, 69, 5)", _host(ops.bspline_coefficients(_dev(x))), x)


def test_bspline_past_the_grid_cap():
    x = np.random.default_rng(12).uniform(-1000.0, 1000.0, H.CAP_SRC).astype(np.float32)
    assert np.prod(H.CAP_OUT) > ops.RESAMPLE_HQ_GRID_LANES
    got = _host(ops.resample3d_bspline(_dev(x), H.CAP_OUT, H.CAP_MAP, default=5.0))
    inside = _bspline_gate("cap", got, x, H.CAP_MAP, H.CAP_OUT, default=5.0)
    assert inside.reshape(-1)[ops.RESAMPLE_HQ_GRID_LANES:].any()


def test_bspline_constant_and_ramp():
    const = np.full(H.SRC_SHAPE, 321.0, np.float32)
    got = _host(ops.resample3d_bspline(_dev(const), H.OBLIQUE_OUT, H.OBLIQUE, border=True))
    assert np.abs(got.astype(np.float64) - 321.0).max() <= 1e-11 * 321.0 + 2.0 ** -24 * 321.0
    # A cubic spline reproduces a linear function; the mirror boundary bends the ramp back, and that disturbance decays
    # by |sqrt(3) - 2| = 0.268 per sample: 20 samples from every face it is below 0.268^20 = 3.7e-12 of max|x|, within
    # the 1e-11 max|x| of the coefficients.  So there the ramp itself is the reference, to 2e-11 max|x| + 2^-24 |ref|.
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in (52, 52, 52)], indexing="ij")
    ramp = (3.0 * x - 2.0 * y + 5.0 * z + 1.0).astype(np.float32)              # exact in f32
    m = np.zeros((3, 4))
    m[:, :3] = H.rotation(0.2, -0.3, 0.4) * 0.2
    m[:, 3] = [25.0, 25.0, 25.0]
    out = (7, 8, 9)
    c, inside = H.coords(m, out, ramp.shape)
    size = np.array(ramp.shape[::-1], np.float64)
    assert np.all((c >= 20.0) & (c <= size - 21.0))
    want = 3.0 * c[..., 0] - 2.0 * c[..., 1] + 5.0 * c[..., 2] + 1.0
    vmax = float(np.abs(ramp).max())
    got = _host(ops.resample3d_bspline(_dev(ramp), out, m)).astype(np.float64)
    d = np.abs(got - want)
    print(f"MEASURED ramp: max |got - ramp| {d.max():.3e} (bound {2e-11 * vmax:.3e} + 2^-24 |ref|)")
    assert np.all(d <= 2e-11 * vmax + 2.0 ** -24 * np.abs(want))


# ------------------------------------------------------------------ label-Gaussian
@pytest.mark.parametrize("case", H.label_cases(), ids=lambda c: c[0])
def test_label_gaussian_equals_the_helper(case):
    name, make, m, out, sigma, alpha, border = case
    arr = make()
    want, hz, _ = H.label_gaussian(arr, m, out, sigma, alpha, border, default=9.0)
    assert hz >= 1e-6
    got = _host(ops.resample3d_label_gaussian(_dev(arr), out, m, sigma=sigma, alpha=alpha, default=9.0, border=border))
    _, inside = H.coords(m, out, arr.shape, border)
    print(f"MEASURED label-gaussian {name}: {int((got != want).sum())} of {got.size} voxels differ, hazard {hz:.2e}")
    assert got.dtype == arr.dtype and np.array_equal(got, want)
    if border:
        assert inside.all()
    elif not inside.all():
        assert np.all(got[~inside] == 9)


def test_label_gaussian_ties_go_to_the_smaller_label():
    for lo, hi in ((3, 7), (7, 3)):
        arr = H.slab_phantom(lo, hi)
        want, hz, tied = H.label_gaussian(arr, H.UPSAMPLE, H.SLAB_OUT)
        assert hz >= 1e-6 and tied.sum() == 99 and tied[:, :, H.SLAB_TIE_PLANE].sum() == 99
        got = _host(ops.resample3d_label_gaussian(_dev(arr), H.SLAB_OUT, H.UPSAMPLE))
        assert np.all(got[tied] == 3)
        assert np.array_equal(got, want)


def test_label_gaussian_past_the_grid_cap():
    arr, want, hz = H.cap_label_reference()
    assert hz >= 1e-6 and want.size > ops.RESAMPLE_HQ_GRID_LANES
    got = _host(ops.resample3d_label_gaussian(_dev(arr), H.CAP_OUT, H.CAP_MAP, sigma=H.CAP_SIGMA))
    assert np.array_equal(got, want)
    tail = want.reshape(-1)[ops.RESAMPLE_HQ_GRID_LANES:]
    assert len(np.unique(tail)) > 1


def test_label_gaussian_refuses_a_window_beyond_the_radius_limit():
    src = _dev(H.label_volume())
    for sigma, alpha in ((3.0, 3.0), ((1.0, 1.0, 4.1), 2.0), (0.0, 2.0), (-1.0, 2.0), (float("nan"), 2.0), (1.0, 0.0)):
        with pytest.raises(RuntimeError, match="resample3d_label_gaussian"):
            ops.resample3d_label_gaussian(src, H.OBLIQUE_OUT, H.OBLIQUE, sigma=sigma, alpha=alpha)
    got = ops.resample3d_label_gaussian(src, H.OBLIQUE_OUT, H.OBLIQUE, sigma=4.0, alpha=2.0)     # radius 8: the limit
    want, hz, _ = H.label_gaussian(H.label_volume(), H.OBLIQUE, H.OBLIQUE_OUT, 4.0, 2.0)
    assert hz >= 1e-6 and np.array_equal(_host(got), want)


# ------------------------------------------------------------------ through the public interface
def test_processing_resample_bspline():
    x = H.image_volume("int16")
    img = P.Image(x, (1.0, 2.0, 0.5), (4.0, -2.0, 8.0))
    got = P.resample(img, (0.5, 0.5, 0.25), interpolator=P.sitkBSpline)
    assert got.GetSize() == (14, 36, 22) and got.GetSpacing() == (0.5, 0.5, 0.25) and got.GetPixelID() == P.sitkInt16
    m = H.scale_map(0.5, 0.25, 0.5)
    _bspline_gate("processing.resample", got.numpy(), x, m, (22, 36, 14))
    lin = P.resample(img, (0.5, 0.5, 0.25))                        # the default is still linear
    assert R.resample_violations(lin.numpy(), R.resample_ref(x, m, (22, 36, 14)), R.resample_ref(x, m, (22, 36, 14), return_real=True), False) == []


def test_processing_resample_to_ref_label_gaussian():
    lab = H.label_volume()
    moving = P.Image(lab, (1.0, 2.0, 0.5), (4.0, -2.0, 8.0))
    fixed = P.Image(np.zeros((10, 30, 12), np.float32), (0.5, 0.5, 0.25), (4.25, -1.0, 8.0))
    got = P.resample_to_ref(moving, fixed, nearest=False, interpolator=P.sitkLabelGaussian)
    m = H.scale_map(0.5, 0.25, 0.5, (0.25, 0.5, 0.0))
    want, hz, _ = H.label_gaussian(lab, m, (10, 30, 12))
    assert hz >= 1e-6
    assert got.GetSize() == (12, 30, 10) and got.GetOrigin() == fixed.GetOrigin() and got.GetPixelID() == P.sitkUInt8
    assert np.array_equal(got.numpy(), want)
    got = P.resample_to_ref(moving, fixed, False, interpolator=P.sitkLabelGaussian, sigma=(0.75, 1.5, 1.0), alpha=1.5)
    want, hz, _ = H.label_gaussian(lab, m, (10, 30, 12), (0.75, 1.5, 1.0), 1.5)
    assert hz >= 1e-6 and np.array_equal(got.numpy(), want)


def test_processing_two_dimensional():
    x = H.image_volume("float32", (1, 9, 11), seed=13)
    img = P.Image(x[0], (1.0, 2.0))
    got = P.resample(img, (0.5, 0.5), interpolator=P.sitkBSpline)
    assert got.GetDimension() == 2 and got.GetSize() == (22, 36)
    m = H.scale_map(0.5, 0.25, 1.0)
    _bspline_gate("2-D", got.numpy()[None], x, m, (1, 36, 22))
    lab = H.label_volume(shape=(1, 9, 11))
    got = P.resample(P.Image(lab[0], (1.0, 2.0)), (0.5, 0.5), interpolator=P.sitkLabelGaussian, sigma=(1.0, 0.75))
    want, hz, _ = H.label_gaussian(lab, m, (1, 36, 22), (1.0, 0.75, 0.75))
    assert hz >= 1e-6 and np.array_equal(got.numpy()[None], want)


@pytest.mark.parametrize("interp", ["bspline", "label-gaussian"])
def test_script_on_nifti_files(tmp_path, interp):
    x = H.label_volume("int16") if interp == "label-gaussian" else H.image_volume("int16")
    P.write_image(P.Image(x, (1.0, 2.0, 0.5), (4.0, -2.0, 8.0)), tmp_path / "moving.nii.gz")
    P.write_image(P.Image(np.zeros((10, 30, 12), np.uint8), (0.5, 0.5, 0.25), (4.25, -1.0, 8.0)), tmp_path / "fixed.nii.gz")
    extra = ["--sigma", "0.75", "--alpha", "2"] if interp == "label-gaussian" else []
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "interpolate_to_reference.py"), str(tmp_path / "moving.nii.gz"),
                        str(tmp_path / "fixed.nii.gz"), str(tmp_path / "out.nii.gz"), "--interpolator", interp, *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = P.read_image(tmp_path / "out.nii.gz")
    assert out.GetSize() == (12, 30, 10) and out.GetPixelID() == P.sitkInt16
    assert np.allclose(out.GetSpacing(), (0.5, 0.5, 0.25)) and np.allclose(out.GetOrigin(), (4.25, -1.0, 8.0))
    m = H.scale_map(0.5, 0.25, 0.5, (0.25, 0.5, 0.0))
    if interp == "bspline":
        _bspline_gate("script", out.numpy(), x, m, (10, 30, 12))
    else:
        want, hz, _ = H.label_gaussian(x, m, (10, 30, 12), 0.75, 2.0)
        assert hz >= 1e-6 and np.array_equal(out.numpy(), want)


# ------------------------------------------------------------------ the linear and nearest paths keep their bits
@pytest.mark.parametrize("pixel", H.PIXELS)
def test_linear_and_nearest_unchanged(pixel):
    x = H.image_volume(pixel)
    for name, (m, out) in MAPS.items():
        for nearest in (False, True):
            got = _host(ops.resample3d(_dev(x), out, m, nearest=nearest))
            ref = R.resample_ref(x, m, out, nearest=nearest)
            real = R.resample_ref(x, m, out, nearest=nearest, return_real=True)
            assert R.resample_violations(got, ref, real, nearest) == [], (name, nearest)
