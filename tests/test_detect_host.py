"""Vertebra-landmark transforms on the host: landmark file IO, EmbedVert's index maths, the Gaussian kernel
tables and the refusals raised before any device work."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from segmantic_amd.detect.transforms import (BoundingBoxd, EmbedVert, ExtractVertPosition, LoadVert, SaveVert,
                                             VertHeatMap, gaussian_kernel_1d, heatmap_sigma)
from segmantic_amd.detect.transforms import output_filename
from tests.helpers import detect_ref as ref


@pytest.fixture
def golden(golden_dir):
    return json.loads((golden_dir / "reference_detect.json").read_text())


def _write(tmp_path: Path, name: str, points) -> Path:
    f = tmp_path / name
    f.write_text(json.dumps(points))
    return f


def test_loadvert_numbers_sorted_names_from_one(tmp_path, golden):
    f = _write(tmp_path, "points.json", golden["landmarks"])
    d = LoadVert(keys="vert", meta_key_postfix="meta")({"vert": f})
    assert set(d["vert"]) == {1, 2}
    np.testing.assert_array_equal(d["vert"][1], golden["landmarks"]["point_0"])
    np.testing.assert_array_equal(d["vert"][2], golden["landmarks"]["point_1"])
    assert d["vert_meta"]["id_map"] == golden["landmark_ids"]
    assert d["vert_meta"]["filename_or_obj"] == f


def test_loadvert_numeric_and_mixed_names(tmp_path):
    d = LoadVert(keys="v")({"v": _write(tmp_path, "a.json", {"7": [1, 2, 3], "01": [4, 5, 6], "12": [0, 0, 0]})})
    assert d["v_meta_dict"]["id_map"] == {"7": 7, "01": 1, "12": 12}
    np.testing.assert_array_equal(d["v"][1], [4, 5, 6])
    d = LoadVert(keys="v")({"v": _write(tmp_path, "b.json", {"L2": [0, 0, 1], "3": [0, 0, 2], "L1": [0, 0, 3]})})
    assert d["v_meta_dict"]["id_map"] == {"3": 1, "L1": 2, "L2": 3}
    np.testing.assert_array_equal(d["v"][2], [0, 0, 3])


def test_output_filename_layout(tmp_path):
    out = tmp_path / "out"
    assert output_filename("points.json", out, "trans", ".json") == out / "points" / "points_trans.json"
    assert output_filename("/data/a/ct.nii.gz", out, "trans", ".json") == out / "ct" / "ct_trans.json"
    assert output_filename("/data/a/ct.nii.gz", out, "p", ".json", separate_folder=False) == out / "ct_p.json"
    assert output_filename("/data/a/b/ct.seg.nrrd", out, "p", ".json", data_root_dir="/data") == \
        out / "a" / "b" / "ct.seg" / "ct.seg_p.json"
    assert output_filename("/data/a/ct.nii.gz", out, "", ".json", data_root_dir="/data", separate_folder=False) == \
        out / "a" / "ct.json"


def test_load_save_round_trip(tmp_path, golden):
    f = _write(tmp_path, "points.json", golden["landmarks"])
    d = LoadVert(keys="vert")({"vert": f})
    SaveVert(keys="vert", output_dir=tmp_path / "out", print_log=False)(d)
    back = json.loads((tmp_path / "out" / "points" / "points_trans.json").read_text())
    assert back == golden["landmarks"]
    # no meta dict: names are str(id), subjects a running index
    sv = SaveVert(keys="vert", output_dir=tmp_path / "idx", output_postfix="x", separate_folder=False,
                  print_log=False)
    sv({"vert": {3: np.array([1.0, 2.0, 3.0])}})
    sv({"vert": {4: np.array([0.5, 0.0, 0.0])}})
    assert json.loads((tmp_path / "idx" / "0_x.json").read_text()) == {"3": [1.0, 2.0, 3.0]}
    assert json.loads((tmp_path / "idx" / "1_x.json").read_text()) == {"4": [0.5, 0.0, 0.0]}


def test_savevert_collects_write_failures(tmp_path):
    blocker = tmp_path / "file"
    blocker.write_text("")
    sv = SaveVert(keys=["a", "b"], output_dir=blocker, print_log=False)
    with pytest.raises(RuntimeError, match="cannot write vertices"):
        sv({"a": {1: [0.0, 0.0, 0.0]}, "a_meta_dict": {"filename_or_obj": "x.json"},
            "b": {1: [0.0, 0.0, 0.0]}, "b_meta_dict": {"filename_or_obj": "y.json"}})


def test_embedvert_golden_geometry(tmp_path, golden):
    a = np.array(golden["affine_ras"])
    nx, ny, nz = golden["size_xyz"]
    img = np.zeros((nz, ny, nx), dtype=np.float32)
    f = _write(tmp_path, "points.json", golden["landmarks"])
    d = LoadVert(keys="vert")({"vert": f, "image": img, "image_meta_dict": {"affine": a}})
    d = EmbedVert(keys="vert", ref_key="image")(d)
    out = d["vert"]
    assert out.shape == img.shape and out.dtype == img.dtype
    assert out.min() == 0 and out.max() == 2 and np.count_nonzero(out) == 2
    for name, i in golden["landmark_ids"].items():
        x, y, z = ref.embed_index(golden["landmarks"][name], a)
        assert out[z, y, x] == i
    np.testing.assert_array_equal(d["vert_meta_dict"]["affine"], a)
    # [1, z, y, x] in, [1, z, y, x] out
    d = EmbedVert(keys="vert", ref_key="image")({**d, "vert": {1: golden["landmarks"]["point_0"]}, "image": img[None]})
    assert d["vert"].shape == (1, nz, ny, nx)


def test_embedvert_rounds_half_to_even():
    a = np.diag([2.0, 2.0, 2.0, 1.0])
    img = np.zeros((4, 8, 8), dtype=np.int16)
    # continuous indices 2.5 -> 2, 3.5 -> 4, 0.5 -> 0
    d = EmbedVert(keys="v", ref_key="im")({"v": {5: [5.0, 7.0, 1.0]}, "im": img, "im_meta_dict": {"affine": a}})
    assert d["v"][0, 4, 2] == 5 and np.count_nonzero(d["v"]) == 1
    assert EmbedVert.indices({1: [5.0, 7.0, 1.0]}, a, img.shape)[1] == (2, 4, 0)


@pytest.mark.parametrize("p", [[-0.6, 0.0, 0.0], [8.0, 0.0, 0.0], [0.0, 3.6, 0.0], [0.0, 0.0, -2.0]])
def test_embedvert_refuses_points_outside(p):
    img = np.zeros((2, 4, 8), dtype=np.uint8)
    with pytest.raises(ValueError, match="outside the volume"):
        EmbedVert(keys="v", ref_key="im")({"v": {1: p}, "im": img})


@pytest.mark.parametrize("label,tail", [(1, 6), (4, 8), (10, 10)])
def test_kernel_tables_against_closed_form_erf(label, tail):
    k = gaussian_kernel_1d(heatmap_sigma(label))
    assert k.dtype == torch.float32 and k.numel() == 2 * tail + 1
    assert ref.tail_of(label) == tail
    s = float(np.float32(1.6 + (label - 1) * 0.1))
    want = [0.5 * (math.erf((x + 0.5) / (s * math.sqrt(2))) - math.erf((x - 0.5) / (s * math.sqrt(2))))
            for x in range(-tail, tail + 1)]
    np.testing.assert_allclose(k.numpy(), want, rtol=1e-6, atol=1e-7)  # erf differences near 1: f32 cancellation
    np.testing.assert_allclose(k.numpy(), ref.kernel_f64(label), rtol=1e-6, atol=1e-7)  # erf differences near 1: f32 cancellation
    assert torch.equal(k, k.flip(0)) and int(k.argmax()) == tail


def test_heatmap_refusals_before_device_work():
    names = ["L1", "L2", "L3"]
    hm = VertHeatMap(keys="lab", label_names=names)
    with pytest.raises(ValueError, match="one-hot"):
        hm({"lab": np.zeros((2, 4, 4, 4), dtype=np.uint8)})
    with pytest.raises(ValueError, match="outside"):
        hm({"lab": np.full((1, 4, 4, 4), 4, dtype=np.int64)})
    with pytest.raises(ValueError, match="outside"):
        hm({"lab": np.full((4, 4, 4), -1, dtype=np.int8)})
    with pytest.raises(ValueError, match="label volume"):
        hm({"lab": np.zeros((4, 4), dtype=np.uint8)})
    with pytest.raises(ValueError, match="at most 255"):
        VertHeatMap(keys="lab", label_names=[str(i) for i in range(256)])({"lab": np.zeros((2, 2, 2), np.uint8)})


def test_other_refusals_before_device_work():
    with pytest.raises(ValueError, match="heatmap"):
        ExtractVertPosition(keys="h")({"h": np.zeros((4, 4, 4), np.float32)})
    with pytest.raises(KeyError):
        ExtractVertPosition(keys="h")({})
    assert ExtractVertPosition(keys="h", allow_missing_keys=True)({}) == {}
    with pytest.raises(ValueError, match="BoundingBoxd"):
        BoundingBoxd(keys="im")({"im": np.zeros((4, 4), np.float32)})
    with pytest.raises(ValueError, match="EmbedVert"):
        EmbedVert(keys="v", ref_key="im")({"v": {}, "im": np.zeros((2, 3, 3, 3), np.float32)})


def test_oracle_known_answers(golden):
    c = golden["bbox_case"]
    nx, ny, nz = golden["size_xyz"]
    arr = np.zeros((1, nz, ny, nx), dtype=np.float32)
    assert ref.bbox(arr) == [[0, 0, 0], [0, 0, 0]]
    (z0, z1), (y0, y1), (x0, x1) = c["fill_zyx"]
    arr[0, z0:z1, y0:y1, x0:x1] = 1
    assert ref.bbox(arr) == c["bbox_xyz"]
    lab = np.zeros((5, 6, 7), np.int32)
    lab[1:3, 2, 4:7] = 2
    assert ref.centre(lab, 2) == (5, 2, 1)
    np.testing.assert_array_equal(ref.centroid_sums(lab, 2)[2], [6, 30, 12, 9])
