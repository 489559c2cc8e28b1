"""Evaluation (seg/evaluation.py) on the host: the CPU oracle, the known answers, Image indexing in sitk
order and argument validation.  Needs no GPU."""
import math

import numpy as np
import pytest
import torch

from segmantic_amd.image.processing import make_image
from segmantic_amd.seg import evaluation
from tests.helpers import distance_ref as ref


def _rand_masks(rng, shape, p=0.15):
    return rng.random(shape) < p


@pytest.mark.parametrize("shape,spacing", [((7, 9), (1.0, 1.0)), ((5, 6, 7), (1.0, 1.0, 1.0)),
                                           ((4, 7, 6), (2.0, 0.8, 0.5)), ((9, 5), (0.5, 1.3))])
def test_separable_oracle_matches_brute_force(shape, spacing):
    rng = np.random.default_rng(1)
    for _ in range(3):
        f = _rand_masks(rng, shape, 0.1)
        np.testing.assert_allclose(ref.edt_sq_separable(f, spacing), ref.edt_sq_brute(f, spacing), rtol=1e-12)
    empty = np.zeros(shape, bool)
    assert np.isinf(ref.edt_sq_separable(empty, spacing)).all()


def test_separable_oracle_matches_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    f = _rand_masks(rng, (20, 17, 23), 0.05)
    sp = (2.0, 0.8, 0.5)
    want = ndi.distance_transform_edt(~f, sampling=sp) ** 2
    np.testing.assert_allclose(ref.edt_sq_separable(f, sp), want, rtol=1e-9, atol=1e-9)


def test_contour_is_the_face_neighbour_erosion():
    m = np.zeros((5, 5), bool)
    m[1:4, 1:4] = True
    c = ref.contour(m)
    assert c.sum() == 8 and not c[2, 2]
    full = np.ones((3, 4), bool)            # the image border counts as background
    assert ref.contour(full).sum() == 3 * 4 - 2


def test_known_answers_through_the_oracle():
    a, b = ref.known_masks()
    k = ref.KNOWN
    same = ref.metrics(a, a, (1.0, 1.0))
    for key in ("surface_mean", "surface_median", "surface_std", "surface_max"):
        assert same[key] == 0.0
    m = ref.metrics(a, b, (1.0, 1.0))
    for key, v in k["surface"].items():
        assert m["surface_" + key] == pytest.approx(v, rel=1e-15)
    assert m["n_surface"] == k["n_surface"]
    assert m["surface_mean_directed"] == pytest.approx(k["surface_directed"], rel=1e-15)
    assert m["percentile_hausdorff"] == pytest.approx(k["hd95"], rel=1e-15)
    for key, v in k["pointwise"].items():
        assert m["pointwise_" + key] == pytest.approx(v, rel=1e-15)
    assert m["average_hausdorff"] == pytest.approx(k["average_hausdorff"], rel=1e-15)
    an = ref.metrics(a, b, (1.0, 0.5))        # spacing (x, y) = (0.5, 1.0) per array axis [y, x]
    assert an["surface_mean"] == pytest.approx(k["surface_aniso"]["mean"], rel=1e-15)
    assert an["surface_max"] == pytest.approx(k["surface_aniso"]["max"], rel=1e-15)


def test_image_indexing_in_sitk_order():
    im = make_image((10, 8), spacing=(0.5, 1.0))
    im[3:6, 2:4] = 1                       # x 3..5, y 2..3
    assert im.data.shape == (8, 10)
    ys, xs = np.nonzero(im.numpy())
    assert set(ys.tolist()) == {2, 3} and set(xs.tolist()) == {3, 4, 5}
    assert im[4, 3] == 1 and im[3, 4] == 0
    sub = im[3:6, :]
    assert sub.GetSize() == (3, 8) and sub.GetSpacing() == (0.5, 1.0)
    row = im[:, 2]
    assert row.GetSize() == (10,) and row.GetSpacing() == (0.5,)
    im3 = make_image((4, 5, 6))
    im3[1, 2, 3] = 7
    assert im3.data[3, 2, 1] == 7 and im3[1, 2, 3] == 7
    with pytest.raises(IndexError):
        im[1, 2, 3]
    with pytest.raises(TypeError):
        im[1.5, 2]


def test_argument_validation():
    a = np.zeros((4, 5, 6), np.uint8)
    with pytest.raises(ValueError, match="shape mismatch"):
        evaluation.hausdorff_surface_distance(a, np.zeros((4, 5, 7), np.uint8))
    with pytest.raises(ValueError, match="spacing"):
        evaluation.hausdorff_pointwise_distance(a, a, spacing=(1.0, 1.0))
    with pytest.raises(ValueError, match="2-D or 3-D"):
        evaluation.surface_distances(np.zeros((2, 3, 4, 5), np.uint8), np.zeros((2, 3, 4, 5), np.uint8))
    with pytest.raises(ValueError, match="2-D or 3-D"):
        evaluation.surface_distances(np.zeros(5, np.uint8), np.zeros(5, np.uint8))
    with pytest.raises(ValueError, match="spacing"):
        evaluation.surface_distances(a, a, spacing=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="integers"):
        evaluation.surface_distances(a.astype(np.float32), a.astype(np.float32))
    with pytest.raises(ValueError, match="shape mismatch"):
        evaluation.confusion_matrix(3, np.zeros(4, np.int32), np.zeros(5, np.int32))


def test_label_bytes():
    from segmantic_amd import ops
    assert ops.label_bytes(torch.zeros(1, dtype=torch.uint8)) == 1
    assert ops.label_bytes(torch.zeros(1, dtype=torch.int16)) == 2
    assert ops.label_bytes(torch.zeros(1, dtype=torch.int32)) == 4
    for dt in (torch.int64, torch.float32, torch.bool):
        with pytest.raises(ValueError, match="label_bytes"):
            ops.label_bytes(torch.zeros(1, dtype=dt))


def test_percentile_interpolation_matches_numpy():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 6, 101):
        v = np.sort(rng.random(n) ** 2)
        for p in (0.0, 50.0, 95.0, 100.0):
            q = p / 100.0
            lo = math.floor(q * (n - 1))
            pair = np.array([v[lo], v[min(lo + 1, n - 1)]])
            assert evaluation._pct_host(n, q, pair) == np.percentile(np.sqrt(v), p)
        mid = np.array([v[(n - 1) // 2], v[n // 2]])
        assert evaluation._median_host(n, mid) == np.median(np.sqrt(v))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU error")
def test_no_gpu_raises_runtime_error():
    a, b = ref.known_masks()
    for call in (lambda: evaluation.hausdorff_surface_distance(a, b),
                 lambda: evaluation.hausdorff_pointwise_distance(a, b),
                 lambda: evaluation.surface_distances(a, b, num_classes=2),
                 lambda: evaluation.confusion_matrix(2, a.reshape(-1), b.reshape(-1))):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
