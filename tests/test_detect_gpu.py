"""Vertebra-landmark kernels on the MI355X against the numpy f64 oracle (tests/helpers/detect_ref.py):
centroid sums exactly, heatmaps within 1e-6 gamma, argmax points to 1e-12, bounding boxes exactly, and the
reference's load -> embed -> one-hot -> extract -> save round trip on its own geometry."""
import json

import numpy as np
import pytest
import torch

from segmantic_amd import ops
from segmantic_amd.detect.transforms import (BoundingBoxd, EmbedVert, ExtractVertPosition, LoadVert, SaveVert,
                                             VertHeatMap)
from tests.helpers import detect_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _ellipsoids(shape, k, seed, dtype=np.uint8, border=True):
    """seeded label volume [z, y, x] of k ellipsoids, some cut by the border"""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    lab = np.zeros(shape, dtype=dtype)
    for c in range(1, k + 1):
        ctr = rng.uniform(0, 1, 3) * np.array(shape)
        if border and c % 3 == 0:
            ctr[c % 3 - 1] = 0.0
        rad = rng.uniform(0.1, 0.25, 3) * np.array(shape) + 1
        lab[((z - ctr[0]) / rad[0]) ** 2 + ((y - ctr[1]) / rad[1]) ** 2 + ((x - ctr[2]) / rad[2]) ** 2 <= 1] = c
    return lab


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
@pytest.mark.parametrize("shape", [(37, 41, 53), (1, 64, 64), (160, 160, 160)])
def test_centroid_sums_exact(dtype, shape):
    k = 9
    lab = _ellipsoids(shape, k - 2, seed=sum(shape), dtype=dtype)   # labels k-1, k absent
    lab.reshape(-1)[-1] = k - 2
    sums, flag = ops.label_centroids(torch.from_numpy(lab).to(DEV), k)
    np.testing.assert_array_equal(sums.cpu().numpy(), ref.centroid_sums(lab, k))
    assert int(flag.item()) == 0


def test_centroid_sums_one_label_fills_the_volume():
    lab = np.full((19, 23, 64), 3, dtype=np.int16)
    sums, flag = ops.label_centroids(torch.from_numpy(lab).to(DEV), 4)
    np.testing.assert_array_equal(sums.cpu().numpy(), ref.centroid_sums(lab, 4))
    assert int(flag.item()) == 0


@pytest.mark.parametrize("dtype,bad", [(np.uint8, 6), (np.int16, -1), (np.int32, 1 << 20), (np.uint8, 255)])
def test_out_of_range_labels_raise(dtype, bad):
    lab = _ellipsoids((17, 20, 24), 5, seed=1, dtype=dtype)
    lab[16, 19, 23] = bad
    _, flag = ops.label_centroids(torch.from_numpy(lab).to(DEV), 5)
    assert int(flag.item()) == 1
    with pytest.raises(ValueError, match="outside"):
        VertHeatMap(keys="l", label_names=["a"] * 5)({"l": torch.from_numpy(lab[None]).to(DEV)})


def _check_heatmap(lab, k, gamma, smooth_3d):
    out = VertHeatMap(keys="l", gamma=gamma, label_names=[f"v{i}" for i in range(k)], smooth_3d=smooth_3d)(
        {"l": lab})["l"]
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (k + 1,) + np.shape(lab)[-3:]
    got = out.cpu().numpy()
    want = ref.heatmap(lab, k, gamma, smooth_3d)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * gamma)
    lab3 = np.asarray(lab)[0] if np.ndim(lab) == 4 else np.asarray(lab)
    for c in range(k + 1):
        if c == 0 or not np.any(lab3 == c):
            assert not np.any(got[c].view(np.uint32)), f"channel {c} is not bit-zero"
        elif not smooth_3d:
            cx = ref.centre(lab3, c)[0]
            assert not np.any(np.delete(got[c], cx, axis=2)), f"channel {c} has values off the slice x = {cx}"
    return got


@pytest.mark.parametrize("smooth_3d", [False, True])
@pytest.mark.parametrize("shape", [(37, 41, 53), (48, 40, 64)])
def test_heatmap_against_oracle(smooth_3d, shape):
    lab = _ellipsoids(shape, 10, seed=5, dtype=np.int16)   # labels 9 and 10 absent below
    lab[lab >= 9] = 0
    got = _check_heatmap(lab[None], 12, 1000.0, smooth_3d)
    assert np.isclose(got.max(), 1000.0)


@pytest.mark.parametrize("smooth_3d", [False, True])
def test_heatmap_labels_at_borders(smooth_3d):
    lab = np.zeros((24, 28, 32), dtype=np.uint8)
    lab[0:2, 0:3, 0:2] = 1          # corner: support clipped on every axis
    lab[22:24, 10:14, 29:32] = 2    # far faces
    lab[10:12, 26:28, 14:16] = 3
    _check_heatmap(lab, 3, 250.0, smooth_3d)


@pytest.mark.parametrize("smooth_3d", [False, True])
def test_heatmap_support_covers_the_volume(smooth_3d):
    lab = np.zeros((5, 5, 5), dtype=np.int32)
    lab[1:4, 1:4, 1:4] = 2
    got = _check_heatmap(lab, 2, 1000.0, smooth_3d)
    if smooth_3d:   # min P > 0: the corner is 0 after the rescale, every voxel of the channel is touched
        assert got[2].min() == 0.0 and np.count_nonzero(got[2]) == 117   # all but the 8 corners


def test_heatmap_int64_input_converted():
    lab = _ellipsoids((20, 24, 28), 4, seed=9, dtype=np.int64)
    _check_heatmap(lab, 4, 1000.0, False)


def test_heatmap_repeatable():
    lab = torch.from_numpy(_ellipsoids((64, 64, 64), 6, seed=3)).to(DEV)
    hm = VertHeatMap(keys="l", label_names=["x"] * 6, smooth_3d=True)
    a, b = hm({"l": lab})["l"], hm({"l": lab})["l"]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _extract(heat, threshold=0.5, affine=None):
    d = {"h": torch.from_numpy(np.ascontiguousarray(heat)).to(DEV)}
    if affine is not None:
        d["h_meta_dict"] = {"affine": affine}
    return ExtractVertPosition(keys="h", threshold=threshold)(d)["h"]


def _same_points(got, want, tol=1e-12):
    assert set(got) == set(want)
    for c in want:
        np.testing.assert_allclose(got[c], want[c], rtol=0, atol=tol)


def test_extract_tie_break_is_the_reference_order():
    heat = np.zeros((2, 6, 7, 8), dtype=np.float32)
    # linear [z, y, x] order picks (z=1, y=2, x=5) first; (x, y, z) order picks x = 3 at z = 4
    heat[1, 1, 2, 5] = 9.0
    heat[1, 4, 6, 3] = 9.0
    got = _extract(heat)
    np.testing.assert_array_equal(got[1], [3.0, 6.0, 4.0])
    _same_points(got, ref.extract(heat))


def test_extract_threshold_zeros_inf_and_nan():
    a = np.array([[0.0, -0.9, 0.0, 2.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 3.0], [0.0] * 4], np.float64)
    heat = np.zeros((6, 5, 4, 6), dtype=np.float32)
    heat[1, 2, 3, 4] = 0.5                                   # max == threshold: kept
    heat[2, 1, 1, 1] = np.nextafter(np.float32(0.5), np.float32(0))   # just below: skipped
    heat[3] = -0.0                                           # +-0 ties: first (x, y, z) is the origin
    heat[3, 0, 0, 0] = -0.0
    heat[3, 3, 2, 0] = 0.0
    heat[4] = -np.inf                                        # all -inf: below any threshold
    heat[5, 4, 3, 5] = 7.0
    got = _extract(heat, threshold=0.5, affine=a)
    want = ref.extract(heat, 0.5, a)
    assert set(want) == {1, 5}
    _same_points(got, want)
    got0 = _extract(heat, threshold=-1.0)
    want0 = ref.extract(heat, -1.0)
    assert set(want0) == {1, 2, 3, 5}
    _same_points(got0, want0)
    np.testing.assert_array_equal(got0[3], [0.0, 0.0, 0.0])
    heat[2, 3, 2, 1] = np.nan
    with pytest.raises(ValueError, match="channel 2"):
        _extract(heat)


def test_extract_on_heatmaps_against_oracle():
    lab = _ellipsoids((40, 48, 56), 8, seed=11)
    heat = VertHeatMap(keys="l", label_names=["v"] * 9)({"l": lab})["l"]
    a = np.array([[0.0, 0.85, 0.0, -1.0], [-1.0, 0.0, 0.0, -1.0], [0.0, 0.0, 2.5, 1.0], [0, 0, 0, 1.0]])
    got = ExtractVertPosition(keys="h")({"h": heat, "h_meta_dict": {"affine": a}})["h"]
    _same_points(got, ref.extract(heat.cpu().numpy(), 0.5, a))
    assert set(got) == {c for c in range(1, 10) if np.any(lab == c)}


def test_extract_odd_extents_and_repeatable():
    rng = np.random.default_rng(4)
    heat = rng.integers(0, 5, (4, 9, 11, 13)).astype(np.float32)   # many ties
    first = _extract(heat)
    _same_points(first, ref.extract(heat))
    for _ in range(3):
        again = _extract(heat)
        assert all(np.array_equal(again[c], first[c]) for c in first)


def test_boundingbox_golden(golden_dir):
    g = json.loads((golden_dir / "reference_detect.json").read_text())
    nx, ny, nz = g["size_xyz"]
    arr = np.zeros((1, nz, ny, nx), dtype=np.float32)
    d = BoundingBoxd(keys="image", result="result", bbox="bbox")({"image": arr})
    assert d["result"]["bbox"] == [[0, 0, 0], [0, 0, 0]]
    (z0, z1), (y0, y1), (x0, x1) = g["bbox_case"]["fill_zyx"]
    arr[0, z0:z1, y0:y1, x0:x1] = 1
    d = BoundingBoxd(keys="image")({"image": torch.from_numpy(arr).to(DEV)})
    assert d["result"]["bbox"] == g["bbox_case"]["bbox_xyz"]


@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.int16, np.int32, np.float64, np.int64, np.bool_])
@pytest.mark.parametrize("shape", [(2, 33, 35, 37), (3, 32, 48, 64), (40, 41, 43)])
def test_boundingbox_random_sparse(dtype, shape):
    rng = np.random.default_rng(len(shape) + shape[-1])
    x = np.zeros(shape, dtype=dtype)
    idx = tuple(rng.integers(0, n, 6) for n in shape)
    x[idx] = 1
    if dtype in (np.float32, np.int16, np.int32, np.float64, np.int64):
        x[tuple(rng.integers(0, n, 50) for n in shape)] = -3   # negatives are not positive
        x[idx] = 1
    got = BoundingBoxd(keys="x")({"x": x})["result"]["bbox"]
    assert got == ref.bbox(x)


def test_boundingbox_nan_and_negative_zero():
    x = np.zeros((2, 10, 12, 16), dtype=np.float32)
    x[0, 0, 0, 0] = np.nan
    x[1, 9, 11, 15] = -0.0
    x[0, 9, 0, 15] = -np.inf
    assert BoundingBoxd(keys="x")({"x": x})["result"]["bbox"] == [[0, 0, 0], [0, 0, 0]]
    x[1, 4, 5, 6] = np.float32(1e-30)
    x[0, 7, 2, 3] = np.inf
    assert BoundingBoxd(keys="x")({"x": x})["result"]["bbox"] == [[3, 2, 4], [7, 6, 8]] == ref.bbox(x)


def test_round_trip_on_reference_geometry(tmp_path, golden_dir):
    g = json.loads((golden_dir / "reference_detect.json").read_text())
    a = np.array(g["affine_ras"])
    nx, ny, nz = g["size_xyz"]
    vert_file = tmp_path / "points.json"
    vert_file.write_text(json.dumps(g["landmarks"]))
    d = {"vert": vert_file, "image": torch.zeros(nz, ny, nx, device=DEV), "image_meta_dict": {"affine": a}}
    d = LoadVert(keys="vert")(d)
    d = EmbedVert(keys="vert", ref_key="image")(d)
    emb = d["vert"]
    assert emb.is_cuda and float(emb.max()) == 2.0
    d["vert"] = torch.nn.functional.one_hot(emb.long(), 3).permute(3, 0, 1, 2).float().contiguous()
    d = ExtractVertPosition(keys="vert", threshold=0.5)(d)
    SaveVert(keys="vert", output_dir=str(tmp_path), print_log=False)(d)
    out = tmp_path / "points" / "points_trans.json"
    verts = json.loads(out.read_text())
    assert set(verts) == set(g["landmarks"])
    for name, p in g["landmarks"].items():
        np.testing.assert_allclose(verts[name], p, atol=1e-4)
