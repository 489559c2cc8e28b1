"""Device results of the feature transform and the label morphology against the float64 / int64 oracle
(tests/helpers/morphology_ref.py): bit for bit when all spacings are equal, and on every voxel that rounding
cannot decide when they are not."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.helpers import morphology_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ANISO = (1.3, 0.7, 1.1)
ANISO2 = (0.7, 1.1)
RADII = [0.0, 1.0, math.sqrt(2.0), 2.5, 500.0]
CAP = 1e-3            # largest share of voxels the oracle may flag as decided by rounding


def _m():
    from segmantic_amd.seg import morphology
    return morphology


def _ops():
    from segmantic_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _volume(shape, seed, dtype=np.uint8, n=6, values=None):
    """seeded ellipsoids, some of them cut by the array border"""
    scale = min(shape) / 48.0
    return ref.ellipsoids(shape, n, seed, lo=3.0 * scale, hi=9.0 * scale, margin=0.0, dtype=dtype, values=values)


def _ft(lab, mode, spacing, label=0, table=None, box=None, dist_sqrt=False):
    ops = _ops()
    sp = ref.spacing3(spacing, lab.ndim)
    tab = None if table is None else _dev(table)
    index, dist = ops.feature_transform(_dev(lab), mode, sp, label=label, table=tab, box=box, with_dist=True,
                                        dist_sqrt=dist_sqrt)
    torch.cuda.synchronize()
    return index.cpu().numpy(), dist.cpu().numpy()


VOLUMES = [((40, 36, 44), np.uint8, 0), ((31, 64, 65), np.int16, 1), ((24, 130, 20), np.int32, 2),
           ((70, 33), np.uint8, 3), ((64, 129), np.int16, 4), ((1, 50), np.int32, 5)]


# ------------------------------------------------------------------ equal spacings: bit for bit
@pytest.mark.parametrize("spacing", [None, 0.7], ids=["unit", "iso0.7"])
@pytest.mark.parametrize("shape,dtype,seed", VOLUMES)
def test_feature_transform_is_exact_for_every_predicate(shape, dtype, seed, spacing):
    ops = _ops()
    lab = _volume(shape, seed, dtype)
    table = np.zeros(65536, np.uint8)
    table[[2, 5]] = 1
    cases = [(ops.FT_NONZERO, 0, None, lab != 0), (ops.FT_ZERO, 0, None, lab == 0),
             (ops.FT_EQUAL, 3, None, lab == 3), (ops.FT_NOT_EQUAL, 1, None, lab != 1),
             (ops.FT_TABLE, 0, table, np.isin(lab, [2, 5]))]
    for mode, label, tab, feature in cases:
        want_i, want_d = ref.nearest_separable(feature, spacing)
        got_i, got_d = _ft(lab, mode, spacing, label=label, table=tab)
        assert np.array_equal(got_i, want_i), (mode, int((got_i != want_i).sum()))
        assert np.array_equal(got_d, want_d.astype(np.float32)), mode


def test_feature_transform_96_cubed_and_a_box():
    lab = _volume((96, 96, 96), 6, np.uint8, n=10)
    want_i, want_d = ref.nearest_separable(lab != 0)
    got_i, got_d = _ft(lab, _ops().FT_NONZERO, None)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_d, want_d.astype(np.float32))
    box = [10, 70, 5, 96, 33, 80]
    sub = lab[10:70, 5:96, 33:80]
    wi, wd = ref.nearest_separable(sub != 2)
    z, y, x = np.unravel_index(np.maximum(wi, 0), sub.shape)
    wi_full = np.where(wi >= 0, ((z + 10) * 96 + (y + 5)) * 96 + (x + 33), -1)
    gi, gd = _ft(lab, _ops().FT_NOT_EQUAL, None, label=2, box=box)
    assert gi.shape == sub.shape
    assert np.array_equal(gi, wi_full)
    assert np.array_equal(gd, wd.astype(np.float32))


def test_no_feature_and_a_single_feature():
    m = _m()
    lab = np.zeros((9, 10, 11), np.uint8)
    gi, gd = _ft(lab, _ops().FT_NONZERO, None)
    assert np.all(gi == -1) and np.all(np.isposinf(gd))
    for op in (m.nearest_label, lambda a: m.expand_labels(a, 3.0), lambda a: m.dilate_labels(a, 3.0),
               lambda a: m.erode_labels(a, 3.0), lambda a: m.open_labels(a, 3.0), lambda a: m.close_labels(a, 3.0)):
        assert np.array_equal(op(lab), lab)
    ones = np.ones((6, 7, 8), np.int16)
    dist, idx = m.distance_transform_edt(ones, return_indices=True)          # no zero voxel anywhere
    assert np.all(np.isposinf(dist)) and np.all(idx == -1) and idx.shape == (3, 6, 7, 8) and idx.dtype == np.int32
    lab[4, 5, 6] = 7
    gi, gd = _ft(lab, _ops().FT_NONZERO, ANISO)
    assert np.all(gi == (4 * 10 + 5) * 11 + 6)
    gz, gy, gx = np.indices(lab.shape)
    assert np.array_equal(gd, ref.dist_sq(gz - 4, gy - 5, gx - 6, ANISO).astype(np.float32))
    assert np.all(m.nearest_label(lab) == 7)
    assert np.array_equal(m.erode_labels(lab, 1.0), np.zeros_like(lab))
    assert np.array_equal(m.erode_labels(np.full((5, 5, 5), 2, np.uint8), 3.0), np.full((5, 5, 5), 2, np.uint8))


def test_ties_go_to_the_smallest_raster_index():
    m = _m()
    for axis in range(3):
        lab = np.zeros((7, 7, 7), np.uint8)
        lo, hi = [3, 3, 3], [3, 3, 3]
        lo[axis], hi[axis] = 1, 5
        lab[tuple(lo)], lab[tuple(hi)] = 9, 2
        for spacing in (None, ANISO):
            assert m.nearest_label(lab, spacing)[3, 3, 3] == 9
            assert np.array_equal(m.nearest_label(lab, spacing), ref.nearest_label(lab, spacing))
    lab = np.zeros((7, 7, 7), np.uint8)
    value = 9
    for z in (2, 4):
        for y in (2, 4):
            for x in (2, 4):
                lab[z, y, x] = value
                value -= 1
    for spacing in (None, ANISO):
        assert m.nearest_label(lab, spacing)[3, 3, 3] == 9
        assert np.array_equal(m.nearest_label(lab, spacing), ref.nearest_label(lab, spacing))
    lab2 = np.zeros((9, 9), np.uint8)
    lab2[2, 2], lab2[2, 6], lab2[6, 2], lab2[6, 6] = 4, 3, 2, 1
    for spacing in (None, ANISO2):
        assert m.nearest_label(lab2, spacing)[4, 4] == 4
        assert np.array_equal(m.nearest_label(lab2, spacing), ref.nearest_label(lab2, spacing))


@pytest.mark.parametrize("spacing", [None, 0.7], ids=["unit", "iso0.7"])
@pytest.mark.parametrize("shape,dtype,seed", VOLUMES[:5])
def test_distance_transform_edt_against_the_oracle(shape, dtype, seed, spacing):
    m = _m()
    lab = _volume(shape, seed, dtype)
    dist64, dsq, index = ref.distance_transform_edt(lab, spacing)
    got_sq, got_idx = m.distance_transform_edt(lab, spacing, return_indices=True, squared=True)
    assert got_sq.dtype == np.float32 and got_idx.dtype == np.int32
    assert np.array_equal(got_sq, dsq.astype(np.float32))
    assert np.array_equal(got_idx, ref.index_planes(index))
    if spacing is None:
        assert np.array_equal(got_sq, np.round(got_sq))
    got = m.distance_transform_edt(lab, spacing)
    want = dist64.astype(np.float32)                                   # within 1 ulp of float32
    assert np.all((got >= np.nextafter(want, np.float32(-np.inf))) & (got <= np.nextafter(want, np.float32(np.inf))))
    assert np.all(got[lab == 0] == 0)
    only_idx = m.distance_transform_edt(lab, spacing, return_distances=False, return_indices=True)
    assert np.array_equal(only_idx, got_idx)


def _six(mod, lab, radius, spacing, applied):
    return {"nearest": mod.nearest_label(lab, spacing), "expand": mod.expand_labels(lab, radius, spacing),
            "dilate": mod.dilate_labels(lab, radius, spacing, applied),
            "erode": mod.erode_labels(lab, radius, spacing, applied),
            "open": mod.open_labels(lab, radius, spacing, applied),
            "close": mod.close_labels(lab, radius, spacing, applied)}


@pytest.mark.parametrize("radius", RADII, ids=lambda r: f"r{r:.3g}")
@pytest.mark.parametrize("spacing", [None, 0.7], ids=["unit", "iso0.7"])
@pytest.mark.parametrize("shape,dtype,seed,applied", [((40, 36, 44), np.uint8, 10, None),
                                                      ((30, 41, 37), np.int16, 11, [2, 5, 6]),
                                                      ((70, 65), np.int32, 12, None), ((66, 70), np.uint8, 13, [1, 3])])
def test_label_operations_are_exact(shape, dtype, seed, applied, spacing, radius):
    lab = _volume(shape, seed, dtype)
    got, want = _six(_m(), lab, radius, spacing, applied), _six(ref, lab, radius, spacing, applied)
    for name in want:
        assert got[name].dtype == lab.dtype and got[name].shape == lab.shape
        assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()))
    if radius == 0.0:
        for name in ("expand", "dilate", "erode", "open", "close"):
            assert np.array_equal(got[name], lab)


def test_large_label_values_and_labels_beyond_the_box_table():
    lab = _volume((28, 30, 32), 14, np.int32, n=5, values=[3, 1500, 40000, 7, 65535])
    got, want = _six(_m(), lab, 2.5, None, [1500, 7, 65535]), _six(ref, lab, 2.5, None, [1500, 7, 65535])
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    got, want = _six(_m(), lab, 1.0, None, None), _six(ref, lab, 1.0, None, None)
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    with pytest.raises(ValueError):
        _m().erode_labels(np.full((4, 4, 4), 70000, np.int32), 1.0)


def test_96_cubed_expand_and_erode():
    lab = _volume((96, 96, 96), 15, np.uint8, n=6)
    assert np.array_equal(_m().expand_labels(lab, 2.5), ref.expand_labels(lab, 2.5))
    assert np.array_equal(_m().erode_labels(lab, 2.5), ref.erode_labels(lab, 2.5))


def test_256_cubed_with_16_labels():
    """lines as long as a workgroup's 256 lanes, many workgroups per pass and 16 grown label boxes.  The
    erosion oracle works on each label's box grown by one voxel (shown equal to the whole volume in the host
    tests); the device grows its boxes by ceil(radius / spacing) + 1."""
    lab = ref.ellipsoids((256, 256, 256), 16, 16, lo=12.0, hi=48.0, margin=0.0)
    assert len(np.unique(lab)) >= 12
    m = _m()
    assert np.array_equal(m.expand_labels(lab, 2.5), ref.expand_labels(lab, 2.5))
    assert np.array_equal(m.erode_labels(lab, 2.5), ref.erode_labels(lab, 2.5, crop=True))


# ------------------------------------------------------------------ unequal spacings
def _issue_volume():
    return ref.ellipsoids((48, 48, 48), 8, 7, lo=3.0, hi=9.0, margin=6.0)


def _check_general(lab, spacing, radius, applied):
    m = _m()
    ops = _ops()
    sp3 = ref.spacing3(spacing, lab.ndim)
    # ---- the oracle side, and its cap, before anything is compared
    feature = lab != 0
    want_i, want_d = ref.nearest_separable(feature, spacing)
    flag_expand = ref.ambiguous(feature, lab, spacing, radius) & (lab == 0)
    flag_nearest = ref.ambiguous(feature, lab, spacing) & (lab == 0)
    sub_feature = np.isin(lab, applied)
    flag_dilate = ref.ambiguous(sub_feature, lab, spacing, radius) & (lab == 0)

    def erode_flags(a):
        out = np.zeros(a.shape, bool)
        for L in applied:
            if (a == L).any():
                out |= ref.ambiguous(a != L, None, spacing, radius) & (a == L)
        return out

    flag_erode = erode_flags(lab)
    want_erode = ref.erode_labels(lab, radius, spacing, applied)
    want_dilate = ref.dilate_labels(lab, radius, spacing, applied)
    flag_open2 = ref.ambiguous(np.isin(want_erode, applied), want_erode, spacing, radius) & (want_erode == 0)
    flag_close2 = erode_flags(want_dilate)
    flags = {"expand": flag_expand, "nearest": flag_nearest, "dilate": flag_dilate, "erode": flag_erode,
             "open stage 2": flag_open2, "close stage 2": flag_close2}
    for name, f in flags.items():
        print(f"{name}: flagged share {f.mean():.3e}")
        assert f.mean() <= CAP, name
    # ---- distances and indices
    got_i, got_d = _ft(lab, ops.FT_NONZERO, spacing)
    print("max relative error of the squared distance", float(np.max(np.abs(got_d - want_d) / np.maximum(want_d, 1e-30))))
    np.testing.assert_allclose(got_d, want_d, rtol=1e-6, atol=0)
    assert got_i.min() >= 0 and feature.reshape(-1)[got_i].all()
    shape3 = (1,) + lab.shape if lab.ndim == 2 else lab.shape
    iz, iy, ix = np.unravel_index(got_i.reshape(shape3), shape3)
    gz, gy, gx = np.indices(shape3)
    at_index = ref.dist_sq(gz - iz, gy - iy, gx - ix, sp3).reshape(lab.shape)
    np.testing.assert_allclose(at_index, want_d, rtol=1e-6, atol=0)
    # ---- label outputs on every voxel rounding cannot decide
    pairs = {"expand": (m.expand_labels(lab, radius, spacing), ref.expand_labels(lab, radius, spacing)),
             "nearest": (m.nearest_label(lab, spacing), ref.nearest_label(lab, spacing)),
             "dilate": (m.dilate_labels(lab, radius, spacing, applied), want_dilate),
             "erode": (m.erode_labels(lab, radius, spacing, applied), want_erode),
             # the second stage of opening / closing, from the oracle's first stage
             "open stage 2": (m.dilate_labels(want_erode, radius, spacing, applied),
                              ref.dilate_labels(want_erode, radius, spacing, applied)),
             "close stage 2": (m.erode_labels(want_dilate, radius, spacing, applied),
                               ref.erode_labels(want_dilate, radius, spacing, applied))}
    for name, (got, want) in pairs.items():
        keep = ~flags[name]
        assert np.array_equal(got[keep], want[keep]), (name, int((got[keep] != want[keep]).sum()))
    # ---- opening and closing are the stated compositions of the device's own stages
    got_erode, got_dilate = pairs["erode"][0], pairs["dilate"][0]
    assert np.array_equal(m.open_labels(lab, radius, spacing, applied),
                          m.dilate_labels(got_erode, radius, spacing, applied))
    assert np.array_equal(m.close_labels(lab, radius, spacing, applied),
                          np.where(lab != 0, lab, m.erode_labels(got_dilate, radius, spacing, applied)))


def test_unequal_spacings_3d():
    _check_general(_issue_volume(), ANISO, 2.5, [1, 2, 3, 4, 5, 6, 7, 8])


def test_unequal_spacings_3d_applied_subset():
    _check_general(_issue_volume(), ANISO, 2.5, [2, 5, 7])


def test_unequal_spacings_2d():
    lab = ref.ellipsoids((90, 80), 8, 7, lo=3.0, hi=9.0, margin=6.0)
    _check_general(lab, ANISO2, 2.5, [1, 2, 3, 4, 5, 6, 7, 8])


# ------------------------------------------------------------------ other checks
def test_repeated_calls_are_bit_identical():
    m = _m()
    lab = _volume((50, 52, 54), 20, np.uint8)
    for spacing in (None, ANISO):
        first = _six(m, lab, 2.5, spacing, None)
        d0, i0 = m.distance_transform_edt(lab, spacing, return_indices=True)
        for _ in range(3):
            again = _six(m, lab, 2.5, spacing, None)
            for name in first:
                assert np.array_equal(first[name], again[name]), name
            d1, i1 = m.distance_transform_edt(lab, spacing, return_indices=True)
            assert np.array_equal(d0, d1) and np.array_equal(i0, i1)


def test_containers_and_channel_axis():
    m = _m()
    lab = _volume((20, 24, 28), 21, np.int16)
    want = m.open_labels(lab, 1.5, ANISO)
    assert isinstance(want, np.ndarray)
    cpu = m.open_labels(torch.from_numpy(lab), 1.5, ANISO)
    assert isinstance(cpu, torch.Tensor) and cpu.device.type == "cpu" and cpu.dtype == torch.int16
    gpu = m.open_labels(torch.from_numpy(lab).cuda(), 1.5, ANISO)
    assert gpu.is_cuda and gpu.dtype == torch.int16
    assert np.array_equal(cpu.numpy(), want) and np.array_equal(gpu.cpu().numpy(), want)
    wide = m.erode_labels(lab.astype(np.int64), 1.5)                    # other integer types come back as they came
    assert wide.dtype == np.int64 and np.array_equal(wide, m.erode_labels(lab, 1.5))
    mask = m.distance_transform_edt(lab != 0)
    assert np.array_equal(mask, m.distance_transform_edt(lab))
    d_gpu, i_gpu = m.distance_transform_edt(torch.from_numpy(lab).cuda(), ANISO, return_indices=True)
    d_np, i_np = m.distance_transform_edt(lab, ANISO, return_indices=True)
    assert d_gpu.is_cuda and i_gpu.is_cuda and i_gpu.dtype == torch.int32
    assert np.array_equal(d_gpu.cpu().numpy(), d_np) and np.array_equal(i_gpu.cpu().numpy(), i_np)
    before = lab.copy()
    m.close_labels(lab, 2.0)
    assert np.array_equal(lab, before)                                  # the input is never modified
    with_channel = m.ErodeLabels(1.5, ANISO)(lab[None])
    assert with_channel.shape == (1,) + lab.shape
    assert np.array_equal(with_channel[0], m.erode_labels(lab, 1.5, ANISO))
    with pytest.raises(ValueError, match="one-hot"):
        m.ErodeLabels(1.5)(np.stack([lab, lab]))


def test_transform_classes_on_dictionaries():
    m = _m()
    lab = _volume((22, 26, 30), 22, np.uint8)
    data = {"seg": lab, "other": 5}
    for cls, fn in ((m.DilateLabelsd, m.dilate_labels), (m.ErodeLabelsd, m.erode_labels),
                    (m.OpenLabelsd, m.open_labels), (m.CloseLabelsd, m.close_labels)):
        out = cls("seg", 2.0, spacing=ANISO, applied_labels=[1, 2, 3])(data)
        assert out["other"] == 5 and out["seg"] is not lab
        assert np.array_equal(out["seg"], fn(lab, 2.0, ANISO, [1, 2, 3]))
    out = m.DistanceTransformEDTd(["seg"], sampling=ANISO)(data)
    assert np.array_equal(out["seg"], m.distance_transform_edt(lab, ANISO))
    assert np.array_equal(m.DistanceTransformEDT()(lab[None])[0], m.distance_transform_edt(lab))
    with pytest.raises(KeyError):
        m.OpenLabelsd("missing", 1.0)(data)


def test_cli_round_trip(tmp_path):
    from segmantic_amd.data.nifti import read_nifti, write_nifti
    m = _m()
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    affine = np.diag([0.7, 1.1, 1.3, 1.0])                               # voxel axes x, y, z -> array spacing (1.3, 1.1, 0.7)
    vols = {"a.nii.gz": _volume((20, 24, 22), 23, np.uint8), "b.nii.gz": _volume((18, 18, 26), 24, np.int16)}
    for name, v in vols.items():
        write_nifti(in_dir / name, v, affine)
    script = str(ROOT / "scripts" / "label_morphology.py")
    runs = [("open", ["--labels", "1", "2"], lambda v: m.open_labels(v, 2.0, (1.3, 1.1, 0.7), [1, 2])),
            ("expand", [], lambda v: m.expand_labels(v, 2.0, (1.3, 1.1, 0.7)))]
    for op, extra, fn in runs:
        out_dir = tmp_path / op
        r = subprocess.run([sys.executable, script, str(in_dir), str(out_dir), "--op", op, "--radius", "2.0", *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        for name, v in vols.items():
            got, aff = read_nifti(out_dir / name)
            assert got.dtype == v.dtype and np.allclose(aff, affine)
            assert np.array_equal(got, fn(v))
            assert not np.array_equal(got, v)
