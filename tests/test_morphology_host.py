"""CPU tests of the morphology contract: the two forms of the oracle against each other and against scipy,
the tie rule on hand-made cases, properties of opening and closing, argument validation, the refusal without a
device and the command line's argument handling."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests.helpers import morphology_ref as ref

ROOT = Path(__file__).resolve().parent.parent
SCRIPT = str(ROOT / "scripts" / "label_morphology.py")
ANISO = (1.3, 0.7, 1.1)


def _blobs(shape, seed, n=4):
    return ref.ellipsoids(shape, n, seed, lo=1.5, hi=4.5, margin=2.0)


# ------------------------------------------------------------------ the oracle against itself and scipy
@pytest.mark.parametrize("shape,seed", [((12, 13, 14), 0), ((16, 12, 20), 1), ((20, 20, 20), 2), ((17, 23), 3),
                                        ((20, 12), 4)])
@pytest.mark.parametrize("spacing", [None, 0.7], ids=["unit", "iso0.7"])
def test_oracle_forms_agree_bit_for_bit(shape, seed, spacing):
    lab = _blobs(shape, seed)
    for feature in (lab != 0, lab == 0, lab != 1):
        ib, db = ref.nearest_brute(feature, spacing)
        is_, ds = ref.nearest_separable(feature, spacing)
        assert np.array_equal(ib, is_)
        assert np.array_equal(db, ds)


@pytest.mark.parametrize("shape,seed,spacing", [((12, 13, 14), 5, ANISO), ((18, 14, 16), 6, ANISO),
                                                ((19, 21), 7, (0.7, 1.1))])
def test_oracle_forms_agree_for_unequal_spacings(shape, seed, spacing):
    """bit for bit wherever rounding cannot decide: outside the voxels the oracle flags"""
    lab = _blobs(shape, seed)
    feature = lab != 0
    ib, db = ref.nearest_brute(feature, spacing)
    is_, ds = ref.nearest_separable(feature, spacing)
    flagged = ref.ambiguous(feature, np.arange(feature.size).reshape(feature.shape), spacing)
    assert flagged.mean() <= 1e-3
    assert np.array_equal(ib[~flagged], is_[~flagged])
    assert np.array_equal(db[~flagged], ds[~flagged])
    np.testing.assert_allclose(ds, db, rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape,seed,sampling", [((14, 15, 16), 8, None), ((14, 15, 16), 9, ANISO),
                                                 ((21, 19), 10, None), ((21, 19), 11, (0.7, 1.1)),
                                                 ((16, 16, 16), 12, 0.7)])
def test_oracle_distances_equal_scipy(shape, seed, sampling):
    lab = _blobs(shape, seed)
    for nearest in (ref.nearest_brute, ref.nearest_separable):
        dist, dsq, index = ref.distance_transform_edt(lab, sampling, nearest)
        want = ndimage.distance_transform_edt(lab, sampling=sampling)
        np.testing.assert_allclose(dist, want, rtol=1e-12, atol=0)
        assert np.all(dist[lab == 0] == 0)


@pytest.mark.parametrize("spacing", [None, ANISO])
def test_oracle_index_is_a_feature_at_the_minimum_distance(spacing):
    lab = _blobs((14, 12, 16), 13)
    feature = lab != 0
    for nearest in (ref.nearest_brute, ref.nearest_separable):
        index, dsq = nearest(feature, spacing)
        assert index.min() >= 0 and feature.reshape(-1)[index].all()
        z, y, x = np.unravel_index(index, feature.shape)
        gz, gy, gx = np.indices(feature.shape)
        got = ref.dist_sq(gz - z, gy - y, gx - x, ref.spacing3(spacing, 3))
        assert np.array_equal(got, dsq)
        want = ndimage.distance_transform_edt(~feature, sampling=spacing) ** 2
        np.testing.assert_allclose(dsq, want, rtol=1e-12, atol=1e-12)


def test_oracle_without_features():
    empty = np.zeros((5, 6, 7), bool)
    for nearest in (ref.nearest_brute, ref.nearest_separable):
        index, dsq = nearest(empty)
        assert np.all(index == -1) and np.all(np.isinf(dsq))
    assert np.all(ref.index_planes(np.full((3, 4), -1, np.int32)) == -1)


# ------------------------------------------------------------------ the tie rule
def _winner(lab, voxel, spacing=None):
    out = {}
    for name, nearest in (("brute", ref.nearest_brute), ("separable", ref.nearest_separable)):
        index, _ = nearest(lab != 0, spacing)
        out[name] = int(lab.reshape(-1)[index[voxel]])
    assert out["brute"] == out["separable"]
    return out["brute"]


@pytest.mark.parametrize("spacing", [None, ANISO], ids=["unit", "aniso"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_tie_midway_between_two_labels_along_each_axis(axis, spacing):
    lab = np.zeros((7, 7, 7), np.uint8)
    lo, hi = [3, 3, 3], [3, 3, 3]
    lo[axis], hi[axis] = 1, 5
    lab[tuple(lo)] = 9          # the smaller coordinate carries the larger label: the index decides, not the value
    lab[tuple(hi)] = 2
    assert _winner(lab, (3, 3, 3), spacing) == 9
    assert ref.expand_labels(lab, 2 * max(ANISO), spacing)[3, 3, 3] == 9


@pytest.mark.parametrize("spacing", [None, ANISO], ids=["unit", "aniso"])
def test_tie_at_the_centre_of_four_and_of_eight(spacing):
    for plane in range(3):                 # four labels at the corners of a square in each coordinate plane
        lab = np.zeros((7, 7, 7), np.uint8)
        value = 9
        axes = [a for a in range(3) if a != plane]
        for da in (2, 4):
            for db in (2, 4):
                pos = [3, 3, 3]
                pos[axes[0]], pos[axes[1]] = da, db
                lab[tuple(pos)] = value    # raster order of the assignments: the first one has the smallest index
                value -= 1
        assert _winner(lab, (3, 3, 3), spacing) == 9
    lab = np.zeros((7, 7, 7), np.uint8)
    value = 9
    for z in (2, 4):
        for y in (2, 4):
            for x in (2, 4):
                lab[z, y, x] = value
                value -= 1
    assert _winner(lab, (3, 3, 3), spacing) == 9
    # z dominates y dominates x: remove the winner and the next one in raster order takes over
    lab[2, 2, 2] = 0
    lab[4, 4, 4] = 0
    assert _winner(lab, (3, 3, 3), spacing) == 8          # (2, 2, 4)
    lab2 = np.zeros((9, 9), np.uint8)
    lab2[2, 2], lab2[2, 6], lab2[6, 2], lab2[6, 6] = 4, 3, 2, 1
    index, _ = ref.nearest_separable(lab2 != 0, (0.7, 1.1))
    assert index[4, 4] == 2 * 9 + 2


# ------------------------------------------------------------------ properties of the operations
@pytest.mark.parametrize("spacing", [None, ANISO], ids=["unit", "aniso"])
@pytest.mark.parametrize("radius", [1.0, 2.5])
def test_open_never_adds_close_never_removes(radius, spacing):
    lab = _blobs((16, 18, 20), 14, n=5)
    opened = ref.open_labels(lab, radius, spacing)
    assert np.all((opened == lab) | (opened == 0))
    closed = ref.close_labels(lab, radius, spacing)
    assert np.array_equal(closed[lab != 0], lab[lab != 0])
    eroded = ref.erode_labels(lab, radius, spacing)
    assert np.all((eroded == lab) | (eroded == 0))
    grown = ref.dilate_labels(lab, radius, spacing)
    assert np.array_equal(grown[lab != 0], lab[lab != 0])
    sub = ref.dilate_labels(lab, radius, spacing, applied_labels=[2])
    assert set(np.unique(sub[lab == 0])) <= {0, 2}


def test_radius_zero_is_the_identity_and_the_border_does_not_erode():
    lab = _blobs((12, 12, 12), 15)
    for op in (ref.dilate_labels, ref.erode_labels, ref.open_labels, ref.close_labels, ref.expand_labels):
        assert np.array_equal(op(lab, 0), lab)
    full = np.full((6, 6, 6), 3, np.uint8)
    assert np.array_equal(ref.erode_labels(full, 2.0), full)          # no voxel differs: nothing erodes
    full[0, 0, 0] = 0
    assert ref.erode_labels(full, 1.0).sum() == 3 * (6 ** 3 - 1 - 3)   # the three face neighbours of the corner


@pytest.mark.parametrize("spacing", [None, ANISO], ids=["unit", "aniso"])
def test_oracle_erosion_on_the_grown_box_equals_the_whole_volume(spacing):
    lab = ref.ellipsoids((20, 22, 24), 6, 16, lo=2.0, hi=7.0, margin=0.0)      # labels touch the border
    for radius in (1.0, 2.5, 6.0):
        assert np.array_equal(ref.erode_labels(lab, radius, spacing, crop=True), ref.erode_labels(lab, radius, spacing))


def test_expand_labels_reaches_exactly_the_radius():
    lab = np.zeros((1, 9, 9), np.uint8)
    lab[0, 4, 4] = 5
    out = ref.expand_labels(lab, np.sqrt(2.0))
    assert out.sum() == 5 * 9                                         # 3 x 3: the diagonal lies at sqrt(2)
    out = ref.expand_labels(lab, 1.4)
    assert out.sum() == 5 * 5


# ------------------------------------------------------------------ the package surface without a device
def test_argument_validation():
    from segmantic_amd.seg import morphology as m
    lab = np.zeros((4, 5, 6), np.uint8)
    for bad in (-1.0, float("inf"), float("nan"), "2", None, True):
        for fn in (m.dilate_labels, m.erode_labels, m.open_labels, m.close_labels, m.expand_labels):
            with pytest.raises(ValueError):
                fn(lab, bad)
    with pytest.raises(ValueError):
        m.DilateLabels(-2.0)
    with pytest.raises(ValueError):
        m.ErodeLabels(1.0, is_onehot=True)
    with pytest.raises(ValueError, match="spacing"):
        m.erode_labels(lab, 1.0, spacing=(1.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        m.erode_labels(lab, 1.0, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        m.distance_transform_edt(lab, sampling=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError):
        m.distance_transform_edt(lab, return_distances=False, return_indices=False)
    with pytest.raises(ValueError):
        m.expand_labels(np.zeros((4, 5, 6), np.float32), 1.0)         # label maps hold integers
    with pytest.raises(ValueError):
        m.expand_labels(np.zeros((2, 3, 4, 5, 6), np.uint8), 1.0)
    with pytest.raises(ValueError, match="applied_labels"):
        m.dilate_labels(lab, 1.0, applied_labels=[70000])
    with pytest.raises(ValueError, match="one-hot"):
        m.OpenLabels(1.0)(np.zeros((3, 4, 5, 6), np.uint8))            # a 3-channel input is taken to be one-hot


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is present")
def test_no_device_is_refused():
    from segmantic_amd.seg import morphology as m
    lab = np.zeros((4, 5, 6), np.uint8)
    calls = [lambda: m.distance_transform_edt(lab), lambda: m.nearest_label(lab), lambda: m.expand_labels(lab, 1),
             lambda: m.dilate_labels(lab, 1), lambda: m.erode_labels(lab, 1), lambda: m.open_labels(lab, 1),
             lambda: m.close_labels(lab, 1), lambda: m.CloseLabelsd("seg", 1.0)({"seg": lab}),
             lambda: m.DistanceTransformEDTd("seg")({"seg": lab})]
    for call in calls:
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


def test_library_declares_the_morphology_entries():
    from segmantic_amd import _lib, ops
    for name in ("segmi_feature_transform", "segmi_feature_transform_workspace_bytes", "segmi_morph_gather",
                 "segmi_morph_erode_select", "segmi_morph_index_planes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert ops.feature_transform_workspace_bytes((3, 4, 5)) == 2 * 256
    assert ops.feature_transform_workspace_bytes((64, 64)) == 2 * 64 * 64 * 4


def test_morphology_kernels_do_not_spill_registers(tmp_path):
    """the code-object metadata of the built library: no morphology kernel spills or uses scratch"""
    import re
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    so = ROOT / "segmantic_amd" / "csrc" / "libsegmi.so"
    if not (so.exists() and Path(f"{llvm}/llvm-objdump").exists()):
        pytest.skip("library or llvm tools not present")
    shutil.copy(so, tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    seen = {}
    for f in sorted(tmp_path.glob("lib.so.*gfx950")):
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", str(f)], capture_output=True, text=True).stdout
        for name, scratch, spill in re.findall(
                r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S):
            if re.search(r"ft_p[123]_kernel|morph_\w+_kernel", name):
                seen[name] = (int(scratch), int(spill))
    assert len(seen) >= 14, sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen


# ------------------------------------------------------------------ the command line
def _cli(*args):
    return subprocess.run([sys.executable, SCRIPT, *args], capture_output=True, text=True, timeout=600)


def test_cli_help_and_argument_errors(tmp_path):
    r = _cli("--help")
    assert r.returncode == 0 and "--radius" in r.stdout and "--op" in r.stdout
    (tmp_path / "in").mkdir()
    r = _cli(str(tmp_path / "in"), str(tmp_path / "out"), "--op", "shrink", "--radius", "1")
    assert r.returncode != 0 and "--op" in r.stdout + r.stderr
    r = _cli(str(tmp_path / "in"), str(tmp_path / "out"), "--op", "erode", "--radius", "-1")
    assert r.returncode != 0 and "--radius" in r.stdout + r.stderr
    r = _cli(str(tmp_path / "in"), str(tmp_path / "out"), "--op", "expand", "--radius", "1", "--labels", "1", "2")
    assert r.returncode != 0 and "--labels" in r.stdout + r.stderr
    r = _cli(str(tmp_path / "in"), str(tmp_path / "out"), "--op", "erode")
    assert r.returncode != 0                                          # --radius is required
    r = _cli(str(tmp_path / "in"), str(tmp_path / "out"), "--op", "erode", "--radius", "1")
    assert r.returncode != 0 and "no label map" in r.stdout + r.stderr


def test_cli_reads_the_spacing_per_array_axis():
    sys.path.insert(0, str(ROOT / "scripts"))
    try:
        import label_morphology as cli
    finally:
        sys.path.pop(0)
    affine = np.diag([0.5, 0.75, 2.0, 1.0])                            # voxel axes x, y, z in mm
    assert cli.array_spacing(affine) == (2.0, 0.75, 0.5)
    assert cli._spread_labels(["a", "b", "--labels", "1", "2", "3", "--op", "erode"]) == \
        ["a", "b", "--labels", "1", "--labels", "2", "--labels", "3", "--op", "erode"]
    with pytest.raises(ValueError):
        cli.array_spacing(np.zeros((4, 4)))
