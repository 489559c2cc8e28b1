"""N4 / CT-scaling on the host: the float64 oracle of tests/helpers/n4_ref.py checked on its own, the
command line's parsing, and the C-ABI entries of image/modality.py."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
from typer.testing import CliRunner

from segmantic_amd.image import modality
from tests.helpers import n4_ref as ref

ROOT = Path(__file__).resolve().parent.parent
N4_SYMBOLS = ("segmi_otsu_workspace_bytes", "segmi_otsu", "segmi_n4_shrink", "segmi_n4_workspace_bytes",
              "segmi_n4_fit", "segmi_n4_sharpen", "segmi_n4_bspline_fit", "segmi_n4_refine", "segmi_n4_evaluate",
              "segmi_ct_scale")


def test_public_interface_matches_reference_signatures():
    import inspect
    sig = inspect.signature(modality.bias_correct)
    assert list(sig.parameters) == ["input", "mask", "shrink_factor", "num_fitting_levels", "num_iterations"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, 4, 4, 50]
    assert list(inspect.signature(modality.scale_clamp_ct).parameters) == ["img"]
    assert list(inspect.signature(modality.unscale_ct).parameters) == ["img"]
    with pytest.raises(ValueError):
        modality.N4BiasFieldCorrectionImageFilter().SetSplineOrder(4)


def test_c_abi_declared_and_bound():
    header = (ROOT / "include" / "segmi.h").read_text()
    from segmantic_amd import _lib
    for name in N4_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_cubic_weights_sum_to_one():
    t = np.linspace(0, 1, 1001)
    w = ref.cubic_weights(t)
    assert np.abs(w.sum(axis=-1) - 1).max() < 1e-15
    assert (w >= 0).all()


@pytest.mark.parametrize("shape", [(4, 5, 7), (1, 6, 9), (6, 1, 4)])
def test_refinement_preserves_the_field(shape):
    rng = np.random.default_rng(0)
    P = rng.normal(size=shape)
    grid = (13, 11, 17)
    grid = tuple(1 if s == 1 else g for s, g in zip(shape, grid))
    a = ref.evaluate(P, grid)
    b = ref.evaluate(ref.refine(P), grid)
    assert np.abs(a - b).max() < 1e-12
    fine = ref.refine(P)
    assert fine.shape == tuple(1 if s == 1 else 2 * (s - 3) + 3 for s in shape)


def test_ba_fit_separable_equals_point_by_point():
    rng = np.random.default_rng(1)
    r = rng.normal(size=(7, 6, 9))
    valid = rng.random(r.shape) > 0.3
    for spans in (1, 2, 4, 8):
        assert np.abs(ref.ba_fit(r, valid, spans) - ref.ba_fit_points(r, valid, spans)).max() < 1e-13


def test_otsu_threshold_between_modes():
    rng = np.random.default_rng(2)
    x = np.where(rng.random((30, 40)) > 0.6, 300.0, 100.0) + rng.normal(0, 10, (30, 40))
    mask, thr, counts = ref.otsu_threshold(x.astype(np.float32))
    assert 100 < thr < 300  # between the modes (first maximum: the low end of the empty gap)
    assert np.array_equal(mask == 1, x > 200)  # the bright class exactly
    assert counts.sum() == x.size
    assert np.array_equal(mask == 1, x.astype(np.float32) > thr)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 31, 64])
@pytest.mark.parametrize("f", [1, 2, 3, 4, 5])
def test_shrink_indices_and_geometry(n, f):
    ns, o = ref.shrink_offsets(n, f)
    assert ns == max(1, n // f)
    idx = o + f * np.arange(ns)
    assert idx.min() >= 0 and idx.max() < n
    # the physical centre of the kept indices is the input's centre up to half a voxel
    assert abs((idx[0] + idx[-1]) / 2 - (n - 1) / 2) <= 0.5
    size, spacing, origin = (n, 5), (0.7, 1.3), (10.0, -4.0)
    ns2, sp, org = ref.shrink_geometry(size, spacing, origin, (1.0, 0.0, 0.0, 1.0), f)
    assert sp[0] == pytest.approx(f * 0.7)
    # output centre == input centre
    assert org[0] + (ns2[0] - 1) * sp[0] / 2 == pytest.approx(origin[0] + (n - 1) * spacing[0] / 2)
    x = np.arange(n * 5).reshape(5, n)
    assert ref.shrink(x, f).shape == (max(1, 5 // f), ns)


def test_sharpening_tends_to_identity():
    rng = np.random.default_rng(3)
    u = rng.uniform(0, 5, 20000)
    E, S = ref.sharpen(u, bins=200, fwhm=1e-3, noise=1e-12)
    centres = 0 + np.arange(200) * (5 / 199)
    ok = E != 0
    assert ok.mean() > 0.95
    assert np.abs(E[ok] - centres[ok]).max() < 1e-3 * 5
    assert np.abs(S - u).max() < 2e-2


def test_cli_parses():
    import importlib.util
    spec = importlib.util.spec_from_file_location("modality_cli", ROOT / "scripts" / "modality.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    runner = CliRunner()
    r = runner.invoke(cli.app, ["n4", "--help"])
    assert r.exit_code == 0
    for opt in ("--mask-dir", "--shrink-factor", "--levels", "--iterations", "--write-log-field"):
        assert opt in r.output
    r = runner.invoke(cli.app, ["ct-scale", "--help"])
    assert r.exit_code == 0 and "--inverse" in r.output
    r = runner.invoke(cli.app, ["n4", "/nonexistent_dir_for_test", "/tmp/out_n4_test", "--levels", "x"])
    assert r.exit_code != 0
    assert cli._log_field_name("a.nii.gz") == "a_logfield.nii.gz"


def test_oracle_n4_recovers_the_phantom_field():
    img, b, cls = ref.phantom((48, 56, 52), seed=7)
    mask, _, _ = ref.otsu_threshold(img)
    si, sm = ref.shrink(img, 2), ref.shrink(mask, 2)
    lat, _, elapsed, cv = ref.n4(si, sm, iterations=(20, 20, 20), threshold=0.0)
    assert elapsed == [20, 20, 20]
    field = ref.evaluate(lat, img.shape)
    v = ref.fit_set(img, mask)
    d = (field - field[v].mean()) - (b - b[v].mean())
    rms = math.sqrt(float((d[v] ** 2).mean()))
    # measured: rms 0.0060 against a field of rms 0.128; within-class CV ratios 0.35 / 0.36 / 0.32.
    # bounds: rms < 0.012 (2x), every class's CV at most half of the input's
    assert rms < 0.012
    corr = img / np.exp(field)
    for k in (1, 2, 3):
        s = cls == k
        assert corr[s].std() / corr[s].mean() < 0.5 * (img[s].std() / img[s].mean())


def test_oracle_rejects_degenerate_fit_sets():
    z = np.zeros((5, 6, 7))
    with pytest.raises(ValueError):
        ref.n4(z, np.ones_like(z))
    with pytest.raises(ValueError):
        ref.n4(np.full((5, 6, 7), 3.0), np.ones((5, 6, 7)))


def test_no_gpu_raises_runtime_error(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from segmantic_amd.image.processing import Image
    with pytest.raises(RuntimeError):
        modality.scale_clamp_ct(Image(np.zeros((4, 4), np.float32)))
    with pytest.raises(RuntimeError):
        modality.bias_correct(Image(np.ones((4, 4, 4), np.float32)))
