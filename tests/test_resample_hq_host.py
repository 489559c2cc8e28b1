"""Host checks of the B-spline and label-Gaussian resamplers, no GPU: the numpy helper
against scipy, the hazard of every label-Gaussian case the GPU file demands bit equality on, the keyword checks of
``image.processing``, ``read_image`` / ``write_image`` and the command-line script."""
import math
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import ndimage

from segmantic_amd.image import processing as P
from tests.helpers import resample_hq_ref as H

ROOT = Path(__file__).resolve().parent.parent
SCRIPT = str(ROOT / "scripts" / "interpolate_to_reference.py")


# ------------------------------------------------------------------ the helper's B-spline is scipy's
@pytest.mark.parametrize("shape", [(5, 7, 6), (1, 9, 4), (2, 3, 33)])
def test_helper_bspline_agrees_with_scipy(shape):
    x = np.random.default_rng(1).uniform(-250.0, 250.0, shape)
    vmax = float(np.abs(x).max())
    coef = H.prefilter(x)
    ref = ndimage.spline_filter(x, order=3, output=np.float64, mode="mirror")
    d = float(np.abs(coef - ref).max())
    print(f"MEASURED prefilter {shape}: {d:.3e} (bound {1e-11 * vmax:.3e})")
    assert d <= 1e-11 * vmax
    # an oblique map that reaches every part of the inside region, the half voxel beyond the end samples included
    m = np.zeros((3, 4))
    m[:, :3] = H.rotation(0.1, -0.15, 0.2) @ np.diag([0.43, 0.37, 0.51])
    m[:, 3] = [-0.45, -0.3, -0.4]
    out = tuple(int(2.6 * s) + 2 for s in shape)
    real, inside = H.bspline_eval(coef, m, out)
    c, _ = H.coords(m, out, shape)
    assert inside.sum() >= 10 and (~inside).any() or shape[0] == 1
    pts = c[inside][:, ::-1].T                                   # scipy wants (z, y, x) rows
    want = ndimage.map_coordinates(x, pts, order=3, mode="mirror", output=np.float64)
    d = float(np.abs(real[inside] - want).max())
    print(f"MEASURED evaluate {shape}: {d:.3e} over {int(inside.sum())} points")
    assert d <= 1e-11 * vmax
    assert np.all(real[~inside] == 0.0)


def test_helper_bspline_reproduces_constants_and_ramps():
    coef = H.prefilter(np.full((4, 5, 6), 7.0))
    assert np.abs(coef - 7.0).max() <= 1e-11 * 7.0              # the filter has unit DC gain
    real, inside = H.bspline_eval(coef, H.OBLIQUE, (6, 7, 8))
    assert np.abs(real[inside] - 7.0).max() <= 1e-11 * 7.0


def test_gate_rejects_a_linear_interpolation():
    """the comparison the GPU file uses tells a cubic result from a trilinear one"""
    from tests.helpers import infer_ref
    x = H.image_volume("int16")
    vmax = float(np.abs(x).max())
    got, real, _ = H.bspline_resample(x, H.OBLIQUE, H.OBLIQUE_OUT)
    assert H.bspline_violations(got, real, vmax) == []
    lin = infer_ref.resample_ref(x, H.OBLIQUE, H.OBLIQUE_OUT)
    assert H.bspline_violations(lin, real, vmax)
    xf = x.astype(np.float32)
    gotf, realf, _ = H.bspline_resample(xf, H.OBLIQUE, H.OBLIQUE_OUT)
    assert H.bspline_violations(gotf, realf, vmax) == []
    assert H.bspline_violations(gotf + np.float32(1e-3), realf, vmax)


# ------------------------------------------------------------------ label-Gaussian: helper and hazards
def _scalar_vote(arr, m, out_zyx, sigma, alpha):
    """the vote voxel by voxel with math.erf and Python integers"""
    sz, sy, sx = arr.shape
    sg = np.broadcast_to(np.asarray(sigma, np.float64), (3,))
    rad = H.radii(sigma, alpha)
    inv = [1.0 / (s * math.sqrt(2.0)) for s in sg]
    c, inside = H.coords(m, out_zyx, arr.shape)
    out = np.zeros(out_zyx, arr.dtype)
    for idx in np.ndindex(*out_zyx):
        if not inside[idx]:
            continue
        taps = []
        for a, n in enumerate((sx, sy, sz)):
            ca = float(c[idx][a])
            i0 = math.floor(ca + 0.5)
            row = []
            for i in range(i0 - rad[a], i0 + rad[a] + 1):
                if 0 <= i <= n - 1:
                    w = 0.5 * (math.erf(((i + 0.5) - ca) * inv[a]) - math.erf(((i - 0.5) - ca) * inv[a]))
                    row.append((i, math.floor(w * H.SCALE + 0.5)))
            taps.append(row)
        score = {}
        for iz, qz in taps[2]:
            for iy, qy in taps[1]:
                for ix, qx in taps[0]:
                    v = arr[iz, iy, ix].item()
                    score[v] = score.get(v, 0) + qz * qy * qx
        top = max(score.values())
        out[idx] = min(v for v, s in score.items() if s == top)
    return out


def test_helper_vote_equals_the_voxel_by_voxel_restatement():
    arr = H.label_volume(labels=40)
    got, hz, _ = H.label_gaussian(arr, H.OBLIQUE, (6, 7, 9), 1.5, 2.0)
    assert hz >= 1e-6
    assert np.array_equal(got, _scalar_vote(arr, H.OBLIQUE, (6, 7, 9), 1.5, 2.0))
    arr = H.label_volume()
    got, _, _ = H.label_gaussian(arr, H.UPSAMPLE, H.UPSAMPLE_OUT, 1.0, 2.0)
    assert np.array_equal(got, _scalar_vote(arr, H.UPSAMPLE, H.UPSAMPLE_OUT, 1.0, 2.0))


def test_every_label_case_is_far_from_a_rounding_boundary():
    """hazard >= 1e-6: two erf implementations a few ulp apart move w * 2^18 by about 1e-10, so no rounding can flip"""
    seen = {}
    for name, make, m, out, sigma, alpha, border in H.label_cases():
        arr = make()
        _, hz, _ = H.label_gaussian(arr, m, out, sigma, alpha, border)
        seen[name] = hz
        print(f"MEASURED hazard {name}: {hz:.3e}")
    seen["cap"] = H.cap_label_reference()[2]
    for lo, hi in ((3, 7), (7, 3)):
        seen[f"slab_{lo}_{hi}"] = H.label_gaussian(H.slab_phantom(lo, hi), H.UPSAMPLE, H.SLAB_OUT)[1]
    assert all(hz >= 1e-6 for hz in seen.values()), seen
    assert seen["upsample_5"] > 0.01 and 1e-5 < seen["oblique_5"] < 1e-3        # the figures of the design note


def test_forty_label_case_overflows_a_table_of_eight():
    """every inside window of the 40-label case holds more than eight distinct labels"""
    arr = H.label_volume(labels=40)
    c, inside = H.coords(H.OBLIQUE, H.OBLIQUE_OUT, arr.shape)
    i0 = np.floor(c + 0.5).astype(np.int64)
    fewest = 99
    for idx in zip(*np.nonzero(inside)):
        x, y, z = i0[idx]
        win = arr[max(z - 3, 0):z + 4, max(y - 3, 0):y + 4, max(x - 3, 0):x + 4]
        fewest = min(fewest, len(np.unique(win)))
    assert fewest > 8, fewest


def test_helper_ties_go_to_the_smaller_label():
    for lo, hi in ((3, 7), (7, 3)):
        got, _, tied = H.label_gaussian(H.slab_phantom(lo, hi), H.UPSAMPLE, H.SLAB_OUT)
        _, inside = H.coords(H.UPSAMPLE, H.SLAB_OUT, (6, 5, 6))
        assert np.array_equal(tied, inside & (np.arange(12) == H.SLAB_TIE_PLANE))      # c = 3.5: midway between the slabs
        assert tied.sum() == 11 * 9 and np.all(got[tied] == 3)
        assert np.all(got[:, :, 6][inside[:, :, 6]] == lo) and np.all(got[:, :, 8][inside[:, :, 8]] == hi)


# ------------------------------------------------------------------ C-ABI, constants
def test_abi_and_grid_cap_constant():
    from segmantic_amd import _lib, ops
    hdr = (ROOT / "include" / "segmi.h").read_text()
    for name in ("segmi_bspline_workspace", "segmi_bspline_prefilter", "segmi_resample3d_bspline",
                 "segmi_resample3d_label_gaussian"):
        assert re.search(rf"^(?:int|int64_t)\s+{name}\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    cap = int(re.search(r"#define SEGMI_RESAMPLE_HQ_GRID_CAP (\d+)", hdr).group(1))
    assert ops.RESAMPLE_HQ_GRID_LANES == cap * 256 == H.GRID_LANES
    assert np.prod(H.CAP_OUT) > H.GRID_LANES
    assert _lib.lib.segmi_bspline_workspace(7, 9, 11) == 8 * 7 * 9 * 11
    mk = (ROOT / "segmantic_amd" / "csrc" / "Makefile").read_text()
    assert "resample_hq.hip" in mk and re.search(r"build/resample_hq\.o: CXXFLAGS \+= -ffp-contract=off", mk)


def test_ops_refuse_cpu_tensors():
    from segmantic_amd import ops
    x = torch.zeros((2, 3, 4))
    for call in (lambda: ops.bspline_coefficients(x), lambda: ops.resample3d_bspline(x, (2, 3, 4), np.eye(4)[:3]),
                 lambda: ops.resample3d_label_gaussian(x, (2, 3, 4), np.eye(4)[:3])):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


# ------------------------------------------------------------------ processing: keywords
def test_interpolator_names_and_keyword_checks_come_before_any_gpu_work(monkeypatch):
    assert (P.sitkLinear, P.sitkNearestNeighbor, P.sitkBSpline, P.sitkLabelGaussian) == \
        ("linear", "nearest", "bspline", "label-gaussian")

    def touched():
        raise AssertionError("the GPU was asked for before the keywords were checked")
    monkeypatch.setattr(P.torch.cuda, "is_available", touched)
    img = P.Image(np.zeros((4, 5, 6), np.float32), (1.0, 1.0, 2.0))
    ref = P.Image(np.zeros((4, 5, 6), np.float32))
    bad = [dict(interpolator="cubic"), dict(nearest=True, interpolator=P.sitkLinear),
           dict(nearest=True, interpolator=P.sitkBSpline), dict(nearest=True, interpolator=P.sitkLabelGaussian),
           dict(sigma=2.0), dict(alpha=1.0), dict(interpolator=P.sitkBSpline, sigma=0.5),
           dict(interpolator=P.sitkNearestNeighbor, alpha=3.0), dict(interpolator=P.sitkLabelGaussian, sigma=0.0),
           dict(interpolator=P.sitkLabelGaussian, sigma=(1.0, 1.0)), dict(interpolator=P.sitkLabelGaussian, alpha=-1.0)]
    for kw in bad:
        nearest = kw.pop("nearest", False)
        with pytest.raises(ValueError):
            P.resample(img, (1.0, 1.0, 1.0), nearest, **kw)
        with pytest.raises(ValueError):
            P.resample_to_ref(img, ref, nearest, **kw)
        with pytest.raises(ValueError):
            P.apply_transform(img, ref, None, nearest, **kw)
    # a consistent request passes the checks and reaches the device query
    for kw in (dict(), dict(interpolator=P.sitkBSpline), dict(interpolator=P.sitkLabelGaussian, sigma=0.7, alpha=1.5),
               dict(interpolator=P.sitkLabelGaussian, sigma=(1.0, 1.0, 0.5))):
        with pytest.raises(AssertionError, match="before the keywords"):
            P.resample(img, (1.0, 1.0, 1.0), **kw)
    with pytest.raises(AssertionError, match="before the keywords"):
        P.resample_to_ref(img, ref, True, interpolator=P.sitkNearestNeighbor)
    with pytest.raises(TypeError):
        P.resample(img, (1.0, 1.0, 1.0), False, P.sitkBSpline)          # keyword-only


# ------------------------------------------------------------------ read_image / write_image
def _oblique_image():
    rng = np.random.default_rng(2)
    r = H.rotation(0.3, -0.2, 0.5)
    return P.Image(rng.integers(-500, 500, (4, 5, 6)).astype(np.int16), (0.7, 1.1, 2.5), (12.5, -30.0, 7.25), r.reshape(-1))


@pytest.mark.parametrize("suffix", [".nii.gz", ".mha", ".nrrd"])
def test_read_write_round_trip_oblique_3d(tmp_path, suffix):
    img = _oblique_image()
    P.write_image(img, tmp_path / f"a{suffix}")
    back = P.read_image(tmp_path / f"a{suffix}")
    assert back.GetDimension() == 3 and back.GetPixelID() == P.sitkInt16
    assert np.array_equal(back.numpy(), img.numpy())
    tol = 1e-5 if suffix == ".nii.gz" else 1e-12                 # NIfTI stores the affine in float32
    assert np.allclose(back.spacing, img.spacing, rtol=tol, atol=0)
    assert np.allclose(back.origin, img.origin, rtol=tol, atol=0)
    assert np.allclose(back.direction, img.direction, rtol=0, atol=tol)


def test_read_write_round_trip_2d(tmp_path):
    a = 0.4
    direction = (math.cos(a), -math.sin(a), math.sin(a), math.cos(a))
    img = P.Image(np.random.default_rng(4).uniform(0, 1, (5, 7)).astype(np.float32), (0.5, 1.5), (3.0, -4.0), direction)
    P.write_image(img, tmp_path / "s.nii")
    back = P.read_image(tmp_path / "s.nii")
    assert back.GetDimension() == 2 and back.GetSize() == (7, 5) and back.GetPixelID() == P.sitkFloat32
    assert np.array_equal(back.numpy(), img.numpy())
    assert np.allclose(back.spacing, img.spacing, rtol=1e-5) and np.allclose(back.origin, img.origin, rtol=1e-5)
    assert np.allclose(back.direction, direction, atol=1e-5)
    P.write_image(img, tmp_path / "s.mha")                       # a 3-D-only format: one slice
    one = P.read_image(tmp_path / "s.mha")
    assert one.GetSize() == (7, 5, 1) and np.array_equal(one.numpy()[0], img.numpy())
    assert np.allclose(one.spacing[:2], img.spacing) and np.allclose(one.origin[:2], img.origin)
    assert np.allclose(np.asarray(one.direction).reshape(3, 3)[:2, :2].reshape(-1), direction)


def test_read_image_refuses_a_pixel_type_images_do_not_have(tmp_path):
    from segmantic_amd.data import imageio
    imageio.write_image(tmp_path / "u.nii", np.zeros((2, 2, 2), np.uint32), np.eye(4))
    with pytest.raises(ValueError, match="pixel type"):
        P.read_image(tmp_path / "u.nii")
    imageio.write_image(tmp_path / "d.nii", np.ones((2, 2, 2), np.float64), np.eye(4))
    assert P.read_image(tmp_path / "d.nii").GetPixelID() == P.sitkFloat32


# ------------------------------------------------------------------ the script
def _cli(*args):
    return subprocess.run([sys.executable, SCRIPT, *args], capture_output=True, text=True, timeout=600)


def test_script_help_and_argument_errors(tmp_path):
    r = _cli("--help")
    assert r.returncode == 0, r.stderr
    for word in ("--interpolator", "--nearest", "--sigma", "--alpha", "MOVING", "FIXED", "OUTPUT"):
        assert word in r.stdout, word
    r = _cli("a.nii", "b.nii", str(tmp_path / "c.nii"), "--interpolator", "cubic")
    assert r.returncode != 0 and "--interpolator must be one of" in r.stderr and not (tmp_path / "c.nii").exists()
    r = _cli("a.nii", "b.nii", str(tmp_path / "c.nii"), "--nearest", "--interpolator", "bspline")
    assert r.returncode != 0 and "nearest=True contradicts" in r.stderr
