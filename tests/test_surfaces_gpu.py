"""Label surfaces on the MI355X against the numpy oracle of tests/helpers/surface_ref.py.  Every tolerance is
derived, none is measured."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.helpers import surface_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 1, 1), (1, 37, 70), (33, 47, 65), (48, 48, 48), (5, 9, 200), (9, 1, 1)]


def _extract(*a, **k):
    from segmantic_amd.image.surfaces import extract_surfaces
    return extract_surfaces(*a, **k)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check_exact(lab, got, labels):
    for c in labels:
        want = ref.surface_nets(lab, c)
        s = got[c]
        assert s.faces.dtype == np.int32 and s.vertices.dtype == np.float32
        assert s.faces.shape == want["faces"].shape and s.vertices.shape == want["index"].shape, c
        assert np.array_equal(s.faces, want["faces"]), c
        assert np.array_equal(_bits(s.vertices), _bits(want["index"])), c


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_bit_equal_to_the_oracle(shape, dtype):
    for classes, density, seed in ((1, 0.5, 1), (4, 0.1, 2), (4, 1.0, 3)):
        lab = ref.noise(shape, classes, density, seed, dtype)
        before = lab.copy()
        got = _extract(lab)
        present = [c for c in range(1, classes + 1) if (lab == c).any()]
        assert sorted(got) == present
        _check_exact(lab, got, present)
        assert np.array_equal(lab, before)


@pytest.mark.parametrize("shape", [(33, 47, 65), (5, 9, 200)])
def test_many_classes(shape):
    lab = ref.noise(shape, 200, 0.7, 7, np.uint8)
    got = _extract(lab)
    present = [c for c in range(1, 201) if (lab == c).any()]
    assert sorted(got) == present
    _check_exact(lab, got, present)
    big = lab.astype(np.int32) * 300                   # values up to 60000
    got = _extract(big, selected=[300, 3000, 60000])
    _check_exact(big, got, [300, 3000, 60000])


def test_borders_full_empty_and_absent():
    lab = np.zeros((7, 8, 70), np.uint8)
    lab[0], lab[-1], lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1] = 1, 1, 1, 1, 1, 1
    _check_exact(lab, _extract(lab), [1])
    full = np.ones((6, 5, 67), np.int16)
    got = _extract(full)
    _check_exact(full, got, [1])
    assert ref.euler_characteristic(got[1].vertices.shape[0], got[1].faces) == 2
    assert abs(got[1].volume - full.size) <= got[1].vertices.shape[0]
    assert _extract(np.zeros((4, 5, 6), np.uint8)) == {}
    got = _extract(full, selected=[1, 9])
    assert got[9].vertices.shape == (0, 3) and got[9].faces.shape == (0, 3)
    assert got[9].vertices.dtype == np.float32 and got[9].faces.dtype == np.int32 and got[9].area == 0.0
    _check_exact(full, got, [1])
    # every selected label absent: the launches run over no chunk at all
    got = _extract(full, selected=[9])
    assert sorted(got) == [9] and got[9].vertices.shape == (0, 3) and got[9].faces.shape == (0, 3)
    got = _extract(torch.from_numpy(full).cuda(), selected=[7, 9], smooth_iterations=2)
    assert sorted(got) == [7, 9] and all(s.vertices.is_cuda and s.faces.shape == (0, 3) for s in got.values())


def test_topology_from_the_device_output():
    for lab, chi in ((ref.ball(), 2), (ref.torus(), 0), (np.ones((5, 6, 7), np.uint8), 2)):
        s = _extract(lab)[1]
        assert ref.directed_edge_balance(s.faces)
        assert ref.euler_characteristic(s.vertices.shape[0], s.faces) == chi
    lab = ref.noise((12, 13, 70), 3, 0.6, 9)
    for s in _extract(lab).values():
        assert ref.directed_edge_balance(s.faces)
    two = np.zeros((4, 4, 4), np.uint8)
    two[1, 1, 1] = two[2, 2, 2] = 1
    assert ref.directed_edge_balance(_extract(two)[1].faces)


@pytest.mark.parametrize("iterations", [1, 5, 20])
def test_relaxation_against_float64(iterations):
    for lab, lam in ((ref.noise((17, 19, 70), 3, 0.5, 4), 0.5), (ref.ball(), 1.0), (ref.torus(), 0.3)):
        got = _extract(lab, smooth_iterations=iterations, relaxation=lam)
        tol = iterations * 2.0 ** -18 + float(np.spacing(np.float32(max(lab.shape)))) / 2
        for c, s in got.items():
            want = ref.surface_nets(lab, c, iterations, lam)
            assert np.array_equal(s.faces, want["faces"])
            err = np.abs(s.vertices.astype(np.float64) - want["index"]).max()
            print(f"T={iterations} label {c}: max error {err:.3e} (bound {tol:.3e})")
            assert err <= tol
            o = s.vertices.astype(np.float64) - (want["cells"] - 1)
            # exactly within the cell: the clamped offset lies in [0, 1], cell - 1 and cell are float32 numbers
            # and rounding is monotone; the identity geometry and this subtraction are exact
            assert (o >= 0).all() and (o <= 1).all()


def test_physical_coordinates():
    lab = ref.noise((20, 21, 70), 2, 0.5, 6)
    spacing, origin = (0.7, 1.3, 2.9), (-103.5, 40.25, 977.0)
    a, b = math.radians(25.0), math.radians(-40.0)
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    direction = (rz @ rx).reshape(-1)
    got = _extract(lab, spacing=spacing, origin=origin, direction=direction)
    from segmantic_amd.image.processing import Image
    img = _extract(Image(torch.from_numpy(lab), spacing, origin, direction))
    for c, s in got.items():
        want = ref.physical(ref.surface_nets(lab, c)["index"], spacing, origin, direction)
        ulp = float(np.spacing(np.float32(np.abs(want).max())))
        err = np.abs(s.vertices.astype(np.float64) - want).max()
        print(f"label {c}: max error {err:.3e} (one ulp {ulp:.3e})")
        assert err <= ulp
        assert np.array_equal(_bits(img[c].vertices.numpy()), _bits(s.vertices))


def test_measures():
    spacing = (0.5, 1.25, 2.0)
    for lab in (ref.ball(), ref.torus(), ref.noise((15, 16, 70), 3, 0.6, 8)):
        got = _extract(lab, spacing=spacing, smooth_iterations=2)
        for c, s in got.items():
            area, vol, abs_area, abs_vol = ref.measures(s.vertices, s.faces)
            f = s.faces.shape[0]
            print(f"label {c}: area {s.area!r} vs {area!r}, volume {s.volume!r} vs {vol!r}")
            assert abs(s.area - area) <= f * 2.0 ** -52 * abs_area
            assert abs(s.volume - vol) <= f * 2.0 ** -52 * abs_vol
            voxel = spacing[0] * spacing[1] * spacing[2]
            assert s.volume > 0
            assert abs(s.volume - float((lab == c).sum()) * voxel) <= s.vertices.shape[0] * voxel


def test_repeatable_and_device_tensors():
    lab = ref.noise((20, 30, 130), 5, 0.6, 10, np.int16)
    a = _extract(lab, smooth_iterations=3, spacing=(0.9, 1.1, 1.7))
    b = _extract(lab, smooth_iterations=3, spacing=(0.9, 1.1, 1.7))
    assert sorted(a) == sorted(b)
    for c in a:
        assert np.array_equal(_bits(a[c].vertices), _bits(b[c].vertices)) and np.array_equal(a[c].faces, b[c].faces)
        assert a[c].area == b[c].area and a[c].volume == b[c].volume
    t = torch.from_numpy(lab).cuda()
    keep = t.clone()
    d = _extract(t, smooth_iterations=3, spacing=(0.9, 1.1, 1.7))
    assert torch.equal(t, keep)
    for c in a:
        assert d[c].vertices.is_cuda and d[c].faces.is_cuda
        assert np.array_equal(_bits(d[c].vertices.cpu().numpy()), _bits(a[c].vertices))
        assert np.array_equal(d[c].faces.cpu().numpy(), a[c].faces)
    h = _extract(torch.from_numpy(lab))
    assert all(not s.vertices.is_cuda for s in h.values())
    # other integer types are read as int32, the unsigned wide tensor types included
    for other in (lab.astype(np.uint16), lab.astype(np.int64), lab.astype(np.int8)):
        o = _extract(torch.from_numpy(other))
        assert sorted(o) == sorted(h)
        assert all(torch.equal(o[c].faces, h[c].faces) and torch.equal(o[c].vertices, h[c].vertices) for c in h)


def test_script_end_to_end(tmp_path):
    from segmantic_amd.data.imageio import read_image, write_image
    from segmantic_amd.image.labels import save_tissue_list
    from segmantic_amd.image.surfaces import read_ply

    sys.path.insert(0, str(ROOT / "scripts"))
    try:
        from visualize_label_surfaces import affine_geometry
    finally:
        sys.path.pop(0)
    lab = ref.noise((14, 15, 70), 3, 0.5, 12, np.uint8)
    lab[lab == 3] = 4                                   # label 3 is absent
    affine = np.array([[0.0, -1.5, 0.0, 10.0], [0.8, 0.0, 0.0, -20.0], [0.0, 0.0, 2.5, 5.0], [0, 0, 0, 1.0]])
    write_image(tmp_path / "seg.nii.gz", lab, affine)
    save_tissue_list({"Background": 0, "Bone": 1, "Fat": 2}, tmp_path / "tissues.txt")
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "visualize_label_surfaces.py"),
                          str(tmp_path / "seg.nii.gz"), str(tmp_path / "out"), str(tmp_path / "tissues.txt"),
                          "--smooth", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "Processing label   1 : Bone" in out.stdout and "Processing label   4 : label_004" in out.stdout
    assert sorted(p.name for p in (tmp_path / "out").glob("*.ply")) == ["Bone.ply", "Fat.ply", "label_004.ply"]
    arr, aff = read_image(tmp_path / "seg.nii.gz")
    sp, og, dr = affine_geometry(aff)
    want = _extract(np.ascontiguousarray(arr), None, sp, og, dr, 2, 0.5)
    for c, name in ((1, "Bone"), (2, "Fat"), (4, "label_004")):
        assert read_ply(tmp_path / "out" / f"{name}.ply") == want[c]
    # a selected label that is absent writes no file
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "visualize_label_surfaces.py"),
                          str(tmp_path / "seg.nii.gz"), str(tmp_path / "out2"), str(tmp_path / "none.txt"),
                          "--selected-tissues", "3", "--selected-tissues", "2"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr
    assert sorted(p.name for p in (tmp_path / "out2").glob("*.ply")) == ["label_002.ply"]
