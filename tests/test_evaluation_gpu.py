"""Evaluation kernels (csrc/distance.hip) and seg/evaluation.py on the MI355X against the CPU oracle of
tests/helpers/distance_ref.py."""
import csv
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from segmantic_amd import ops
from segmantic_amd.image.processing import make_image
from segmantic_amd.seg import evaluation
from tests.helpers import distance_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent


def _edt(labels_np, label, feature, spacing_zyx, box=None, dtype=torch.uint8):
    lab = torch.from_numpy(np.ascontiguousarray(labels_np)).to(dtype).to(DEV)
    shp = (1,) + labels_np.shape if labels_np.ndim == 2 else labels_np.shape
    box = box or [0, shp[0], 0, shp[1], 0, shp[2]]
    bd, bh, bw = box[1] - box[0], box[3] - box[2], box[5] - box[4]
    dist = torch.empty(bd * bh * bw, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.edt_workspace_bytes(box), dtype=torch.uint8, device=DEV)
    sp3 = ([1.0] + list(spacing_zyx)) if labels_np.ndim == 2 else list(spacing_zyx)
    ops.edt_sq(lab, label, feature, box, sp3, dist, ws)
    out = dist.reshape(bd, bw, bh).permute(0, 2, 1).cpu().numpy()
    return out if labels_np.ndim == 3 else out[0]


def _want(labels_np, label, feature, spacing, box=None):
    m = labels_np == label
    f = ref.contour(m) if feature else m
    if box is not None:
        sl = tuple(slice(box[2 * a], box[2 * a + 1]) for a in range(3))
        m, f = m[sl], f[sl]
    return ref.edt_sq_brute(f, spacing), m


def _check_edt(labels_np, label, spacing, exact, box=None):
    for feature in (0, 1):
        got = _edt(labels_np, label, feature, spacing, box)
        want, inside = _want(labels_np, label, feature, spacing, box)
        if feature:   # signed contour map: the label's voxels carry the sign bit
            assert np.array_equal(np.signbit(got), inside)
            got = np.abs(got)
        if exact:
            assert np.array_equal(got, want.astype(np.float32)), np.abs(got - want).max()
        else:
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), fin)
            np.testing.assert_allclose(got[fin], want[fin], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("shape", [(13, 17), (1, 23), (9, 11, 14), (5, 1, 8), (16, 3, 70)])
def test_edt_against_brute_force_unit_spacing(shape):
    rng = np.random.default_rng(7)
    for p in (0.02, 0.2, 0.6):
        lab = (rng.random(shape) < p).astype(np.uint8) * 3
        _check_edt(lab, 3, (1.0,) * len(shape), exact=True)


def test_edt_special_masks():
    shape = (8, 10, 12)
    single = np.zeros(shape, np.uint8)
    single[3, 4, 5] = 1
    full = np.ones(shape, np.uint8)
    faces = np.zeros(shape, np.uint8)
    faces[0, 2, 3] = faces[-1, 5, 6] = faces[4, 0, 7] = faces[2, -1, 1] = faces[6, 3, 0] = faces[1, 8, -1] = 1
    planes = np.zeros(shape, np.uint8)
    planes[2] = 1                     # empty lines and planes everywhere else
    planes[:, :, 9] = 1
    for lab in (single, full, faces, planes):
        _check_edt(lab, 1, (1.0, 1.0, 1.0), exact=True)
        _check_edt(lab, 1, (2.0, 0.8, 0.5), exact=False)
    none = np.zeros(shape, np.uint8)
    none[0, 0, 0] = 2
    assert np.isinf(_edt(none, 1, 1, (1.0, 1.0, 1.0))).all()


@pytest.mark.parametrize("spacing", [(2.0, 0.8, 0.5), (0.7, 1.0, 1.9)])
def test_edt_anisotropic_and_2d(spacing):
    rng = np.random.default_rng(11)
    lab = (rng.random((7, 12, 15)) < 0.1).astype(np.int32) * 5
    _check_edt(lab, 5, spacing, exact=False)
    lab2 = (rng.random((19, 13)) < 0.1).astype(np.uint8)
    _check_edt(lab2, 1, spacing[1:], exact=False)
    _check_edt(lab2, 1, (1.0, 1.0), exact=True)


def test_edt_on_a_box_and_every_label_type():
    rng = np.random.default_rng(5)
    lab = np.zeros((20, 22, 24), np.int32)
    lab[4:15, 6:17, 3:20] = (rng.random((11, 11, 17)) < 0.3) * 2
    box = [4, 15, 6, 17, 3, 20]
    for dt in (torch.uint8, torch.int16, torch.int32):
        for feature in (0, 1):
            got = np.abs(_edt(lab, 2, feature, (1.0, 1.0, 1.0), box, dt))
            want, _ = _want(lab, 2, feature, (1.0, 1.0, 1.0), box)
            assert np.array_equal(got, want.astype(np.float32))


def _blobs(rng, shape, n, label=1):
    zz, yy, xx = np.indices(shape)
    out = np.zeros(shape, np.uint8)
    for _ in range(n):
        c = rng.random(3) * np.asarray(shape)
        r = rng.random(3) * 0.15 * np.asarray(shape) + 2
        out[((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1] = label
    return out


@pytest.mark.parametrize("n", [96, 160])
def test_edt_and_sampler_against_separable_oracle(n):
    rng = np.random.default_rng(n)
    shape = (n - 3, n, n + 5)
    a, b = _blobs(rng, shape, 6), _blobs(rng, shape, 6)
    sp = (2.0, 0.8, 0.5)
    got = np.abs(_edt(b, 1, 1, sp))
    want = ref.edt_sq_separable(ref.contour(b == 1), sp)
    np.testing.assert_allclose(got, want, rtol=1e-6)
    res = evaluation.surface_distances(a, b, num_classes=2, spacing=sp, percentile=95.0)
    m = ref.metrics(a == 1, b == 1, sp, 95.0)
    for key in evaluation.RESULT_KEYS[:-2]:
        assert res[key][1] == pytest.approx(m[key], rel=1e-6, abs=1e-9), key


def _known_images(spacing=None):
    a = make_image((10, 10), spacing=spacing)
    b = make_image((10, 10), spacing=spacing)
    a[3:6, 3:6] = 1
    b[1:8, 2:7] = 1
    return a, b


def test_reference_tests_restated():
    a, b = _known_images()
    same = evaluation.hausdorff_surface_distance(a, a)
    assert all(v == 0.0 for v in same.values())
    same_p = evaluation.hausdorff_pointwise_distance(a, a)
    assert all(v == 0.0 for v in same_p.values())
    d = evaluation.hausdorff_surface_distance(a, b)
    assert d["max"] >= 2.0 and all(v > 0 for v in d.values())


def test_known_answers():
    k = ref.KNOWN
    a, b = _known_images()
    s = evaluation.hausdorff_surface_distance(a, b)
    for key, v in k["surface"].items():
        assert s[key] == pytest.approx(v, rel=1e-12), key
    p = evaluation.hausdorff_pointwise_distance(a, b)
    for key, v in k["pointwise"].items():
        assert p[key] == pytest.approx(v, rel=1e-12), key
    m = evaluation.surface_distances(a.data, b.data, num_classes=2, percentile=95.0)
    assert m["percentile_hausdorff"][1] == pytest.approx(k["hd95"], rel=1e-12)
    assert m["average_hausdorff"][1] == pytest.approx(k["average_hausdorff"], rel=1e-12)
    assert math.isnan(m["surface_mean"][0])
    an, bn = _known_images(spacing=(0.5, 1.0))
    sa = evaluation.hausdorff_surface_distance(an, bn)
    assert sa["mean"] == pytest.approx(k["surface_aniso"]["mean"], rel=1e-12)
    assert sa["max"] == pytest.approx(k["surface_aniso"]["max"], rel=1e-12)
    with pytest.raises(ValueError, match="empty"):
        evaluation.hausdorff_surface_distance(a, make_image((10, 10)))


def test_surface_distances_multilabel():
    rng = np.random.default_rng(3)
    shape = (40, 45, 50)
    ref_l = np.zeros(shape, np.int16)
    pred_l = np.zeros(shape, np.int16)
    for c, lab in ((1, ref_l), (2, ref_l), (1, pred_l), (2, pred_l)):
        blob = _blobs(rng, shape, 2, label=1).astype(bool)
        lab[blob & (lab == 0)] = c
    ref_l[10, 5:30, 7:40] = 3                   # one voxel thick
    pred_l[11, 6:31, 7:38] = 3
    pred_l[30:33, 30:34, 2:5] = 5               # only in pred -> NaN; label 4 absent from both
    sp = (1.0, 1.0, 1.0)
    for pct in (50.0, 95.0, 100.0):
        res = evaluation.surface_distances(pred_l, ref_l, num_classes=6, spacing=sp, percentile=pct)
        for c in (1, 2, 3):
            m = ref.metrics(pred_l == c, ref_l == c, sp, pct)
            for key in evaluation.RESULT_KEYS[:-2]:
                assert res[key][c] == pytest.approx(m[key], rel=1e-6, abs=1e-9), (c, key)
            assert res["n_pred"][c] == (pred_l == c).sum() and res["n_ref"][c] == (ref_l == c).sum()
        for c in (0, 4, 5):
            assert all(math.isnan(res[key][c]) for key in evaluation.RESULT_KEYS[:-2])
        assert res["n_pred"][5] == 3 * 4 * 3 and res["n_ref"][5] == 0 and res["n_pred"][4] == 0
        if pct == 100.0:
            assert np.array_equal(res["percentile_hausdorff"][1:4], res["surface_max"][1:4])
        again = evaluation.surface_distances(pred_l, ref_l, num_classes=6, spacing=sp, percentile=pct)
        for key in res:
            assert np.array_equal(res[key], again[key], equal_nan=True), key


def _select(vals_np, ranks):
    v = torch.from_numpy(vals_np.astype(np.float32)).to(DEV)
    n = torch.tensor([len(vals_np)], dtype=torch.int64, device=DEV)
    r = torch.tensor(ranks, dtype=torch.int64, device=DEV)
    out = torch.empty(len(ranks), dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.select_workspace_bytes(len(ranks)), dtype=torch.uint8, device=DEV)
    ops.select_f32(v if len(vals_np) else torch.empty(1, device=DEV), n, r, out, ws)
    return out.cpu().numpy()


def test_order_statistics_against_sort():
    rng = np.random.default_rng(9)
    cases = [rng.random(1), rng.random(2), rng.random(7) * 100, rng.random(10) * 3,
             rng.integers(0, 4, 5000).astype(np.float32), np.zeros(777, np.float32),
             (rng.random(10 ** 7) ** 3 * 1e4).astype(np.float32)]
    for v in cases:
        v = v.astype(np.float32)
        s = np.sort(v)
        n = len(v)
        ranks = sorted({0, (n - 1) // 2, n // 2, n - 1})[:4]
        assert np.array_equal(_select(v, ranks), s[ranks])
    assert np.isnan(_select(np.zeros(0, np.float32), [0])).all()


@pytest.mark.parametrize("k", [2, 3, 16, 32, 100])
def test_confusion_matrix(k):
    rng = np.random.default_rng(k)
    t = rng.integers(0, k, 100_003)
    p = np.where(rng.random(t.shape) < 0.7, t, rng.integers(0, k, t.shape))
    want = np.bincount(t * k + p, minlength=k * k).reshape(k, k)
    dts = [np.int16, np.int32] + ([np.uint8] if k <= 255 else [])
    for dt in dts:
        cm = evaluation.confusion_matrix(k, p.astype(dt), t.astype(dt))
        assert cm.dtype == np.float64 and np.array_equal(cm, want)
    with pytest.raises(ValueError, match="outside"):
        evaluation.confusion_matrix(k, p.astype(np.int32), (t + k).astype(np.int32))


def test_confusion_matrix_reference_2d():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 4, (32, 48))
    cm = evaluation.confusion_matrix(4, y, y)
    assert np.array_equal(np.diag(cm), np.bincount(y.reshape(-1), minlength=4))
    assert (cm - np.diag(np.diag(cm)) == 0).all()


def test_crop_larger_than_2_31_bytes():
    d, h, w = 520, 1024, 1024
    truth = torch.ones((d, h, w), dtype=torch.uint8, device=DEV)
    pred = torch.zeros((d, h, w), dtype=torch.uint8, device=DEV)
    v = (3, 2, 1)
    pred[v] = 1
    box = [0, d, 0, h, 0, w]
    nvox = d * h * w
    assert nvox * 4 > 2 ** 31
    dist = torch.empty(nvox, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.edt_workspace_bytes(box), dtype=torch.uint8, device=DEV)
    ops.edt_sq(pred, 1, 1, box, (1.0, 1.0, 1.0), dist, ws)
    g = torch.Generator().manual_seed(0)
    zz = torch.randint(0, d, (4000,), generator=g)
    yy = torch.randint(0, h, (4000,), generator=g)
    xx = torch.randint(0, w, (4000,), generator=g)
    zz[:4] = torch.tensor([d - 1, 0, d - 1, 3])
    yy[:4] = torch.tensor([h - 1, 0, 0, 2])
    xx[:4] = torch.tensor([w - 1, 0, w - 1, 1])
    idx = ((zz * w + xx) * h + yy).to(DEV)          # [z][x][y] layout
    got = dist[idx].abs().cpu().numpy().astype(np.float64)
    want = ((zz - v[0]) ** 2 + (yy - v[1]) ** 2 + (xx - v[2]) ** 2).numpy().astype(np.float64)
    assert np.array_equal(got, want)
    del dist, ws
    res = evaluation.surface_distances(pred, truth, num_classes=2, percentile=None)
    far = math.sqrt((d - 1 - v[0]) ** 2 + (h - 1 - v[1]) ** 2 + (w - 1 - v[2]) ** 2)
    assert res["pointwise_max"][1] == far and res["hausdorff"][1] == far
    assert res["n_pred"][1] == 1 and res["n_ref"][1] == nvox


def test_evaluate_segmentations_script(tmp_path):
    from segmantic_amd.data.imageio import read_image, write_image
    spec = importlib.util.spec_from_file_location("evaluate_segmentations", ROOT / "scripts" / "evaluate_segmentations.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(4)
    (tmp_path / "pred").mkdir()
    (tmp_path / "ref").mkdir()
    affine = np.diag([0.8, 1.2, 2.0, 1.0])
    affine[:3, 3] = (4.0, -3.0, 10.0)
    shape = (24, 30, 36)
    for case in ("a", "b"):
        r = np.zeros(shape, np.uint8)
        p = np.zeros(shape, np.uint8)
        for c in (1, 2):
            r[_blobs(rng, shape, 2).astype(bool) & (r == 0)] = c
            p[_blobs(rng, shape, 2).astype(bool) & (p == 0)] = c
        write_image(tmp_path / "pred" / f"{case}.nii.gz", p, affine)
        write_image(tmp_path / "ref" / f"{case}.nii.gz", r, affine)
    out = tmp_path / "scores.csv"
    mod.main(tmp_path / "pred", tmp_path / "ref", out, "*.nii.gz", "1,2")
    rows = list(csv.DictReader(open(out)))
    assert len(rows) == 4
    for row in rows:
        p, aff = read_image(tmp_path / "pred" / f"{row['case']}.nii.gz")
        r, _ = read_image(tmp_path / "ref" / f"{row['case']}.nii.gz")
        sp = mod.spacing_zyx(aff)
        assert sp == pytest.approx([2.0, 1.2, 0.8])
        c = int(row["label"])
        a, b = p == c, r == c
        m = ref.metrics(a, b, sp, 95.0)
        inter = (a & b).sum()
        assert float(row["dice"]) == pytest.approx(2 * inter / (a.sum() + b.sum()), rel=1e-12)
        assert float(row["false_negative_error"]) == pytest.approx((b.sum() - inter) / b.sum(), rel=1e-12)
        assert float(row["false_positive_error"]) == pytest.approx((a.sum() - inter) / a.sum(), rel=1e-12)
        for col, key in (("hausdorff", "hausdorff"), ("average_hausdorff", "average_hausdorff"),
                         ("hd95", "percentile_hausdorff"), ("surface_mean", "surface_mean")):
            assert float(row[col]) == pytest.approx(m[key], rel=1e-6), col
    with pytest.raises(RuntimeError):
        mod.evaluate(tmp_path / "pred", tmp_path / "ref", out, "*.mha")
