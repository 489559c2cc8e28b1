"""``segmi_elastic_warp_crop_patches`` and the sampler around it against the float64 oracle of
tests/helpers/elastic_ref.py.

The bounds are those of tests/test_augment_gpu.py with the elastic coordinate term added; their derivation
sits with the gates in ``elastic_ref`` (``displacement_error``, ``coord_error``, ``image_gate``,
``label_gate``), which tests/test_elastic_host.py holds to five seeded faults and to the 1 % cap of the label
exemption.  MEASURED lines print the observed error next to the bound (``pytest -s``)."""
import json
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.seg import augment as aug  # noqa: E402
from tests.helpers import augment_ref as ar  # noqa: E402
from tests.helpers import elastic_ref as er  # noqa: E402

DEV = "cuda:0"
STORE = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _measured(name, err, bound):
    print(f"MEASURED {name}: {err:.3e} (bound {bound:.3e})")


def _device_volume(image, label):
    """[C, D, H, W] / [D, H, W] float64 host arrays -> the NDHWC f32 image and [1, D, H, W] label the kernels read"""
    imd = torch.from_numpy(np.ascontiguousarray(image.transpose(1, 2, 3, 0), dtype=np.float32))[None].to(DEV)
    lad = torch.from_numpy(np.ascontiguousarray(label, dtype=np.float32))[None].to(DEV)
    return imd, lad


def _dev_ctrl(ctrl):
    return torch.from_numpy(np.ascontiguousarray(ctrl, dtype=np.float32)).to(DEV)


def _xyz(m):
    return None if m is None else aug.to_index_map_xyz(m)


@pytest.fixture(scope="module")
def vol():
    """the volume of the kernel tests and the quantities of its bounds, made once"""
    image, label = er.volume()
    imd, lad = _device_volume(image, label)
    vmax = float(np.abs(image).max())
    # Lipschitz constant of the trilinear interpolant along one axis: the largest neighbour step
    lip = max(float(np.abs(np.diff(image, axis=a)).max()) for a in (1, 2, 3))
    return {"image": image, "label": label, "imd": imd, "lad": lad, "vmax": vmax, "lip": lip}


@pytest.fixture(scope="module")
def cases():
    return er.kernel_cases(aug)


def _run(imd, lad, starts, flips, m, ctrl, roi, dtype, c):
    out = torch.full((len(starts),) + tuple(roi) + (c,), 7.0, device=DEV).to(dtype)
    olab = torch.full((len(starts),) + tuple(roi), 7.0, device=DEV)
    ops.elastic_warp_crop_patches(imd, lad, starts, flips, _xyz(m), _dev_ctrl(ctrl), out, olab)
    torch.cuda.synchronize()
    return out, olab


def _check_against_oracle(name, image, label, out, olab, starts, flips, m, ctrl, roi, dtype, vmax, lip):
    """image bound 3 delta lip + 16 EPS32 vmax + one storage rounding; labels equal except within 2 delta of a
    .5 boundary.  delta (``elastic_ref.coord_error``) is the derived f32 error of the source coordinate: that of
    the B-spline evaluation -- t and f, the weights, the 64-term sums of magnitude <= A, the addition to a --
    carried through the affine map's row sum, plus the affine arithmetic's own error."""
    shape = image.shape[1:]
    delta = er.coord_error(ctrl, m, shape)
    assert delta <= 5e-4, delta                  # a looser bound could not tell a wrong tap from rounding
    got = out.float().cpu().numpy()
    gl = olab.cpu().numpy()
    worst, tol = -1.0, 0.0
    for w, (st, fl) in enumerate(zip(starts, flips)):
        ri, rl, src = er.elastic_warp_crop(image, label, ctrl, m, st[1:], roi)
        ri, rl, src = ar.flip(ri, fl), ar.flip(rl, fl), ar.flip(src, fl)
        err, tol = er.image_gate(got[w].transpose(3, 0, 1, 2), ri, delta, lip, vmax, STORE[dtype])
        worst = max(worst, err)
        assert err <= tol, (name, w, st, fl, err, tol)
        assert er.label_gate(gl[w], rl, src, shape, delta) == 0, (name, w)
    _measured(f"elastic {name} {STORE[dtype]} delta {delta:.2e}", worst, tol)


# ----------------------------------------------------------------------------- kernel against oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_float64_oracle(vol, cases, dtype):
    """33 x 29 x 41 two-channel volume, 16 patches of 16 x 12 x 20 with all 8 flip codes and starts inside,
    partly outside and fully outside; grids (4, 4, 4) (one span: the k clamp acts at the last voxel),
    (7, 7, 7) and (4, 5, 9), each with the identity and a rotation + zoom map, A at the default and at the
    largest value the no-fold check admits.  On the anisotropic (4, 5, 9) grid the default amplitude gives
    L of about 1.9, a field the sampler's no-fold check refuses; the kernel is defined for any grid and is
    held to the oracle on it all the same (``elastic_ref.control`` draws the grid directly)."""
    assert len(cases) == 12
    for name, ctrl, m in cases:
        out, olab = _run(vol["imd"], vol["lad"], er.STARTS, er.FLIPS, m, ctrl, er.ROI, dtype, er.CHANNELS)
        _check_against_oracle(name, vol["image"], vol["label"], out, olab, er.STARTS, er.FLIPS, m, ctrl, er.ROI,
                              dtype, vol["vmax"], vol["lip"])
        assert float(out[4].float().abs().max()) == 0.0 and float(olab[4].abs().max()) == 0.0   # fully outside


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_field_is_bit_identical_to_the_affine_gather(vol, dtype):
    m = er.rotation_zoom_map(aug)
    for n in er.GRIDS:
        out, olab = _run(vol["imd"], vol["lad"], er.STARTS, er.FLIPS, m, np.zeros((3,) + n, np.float32), er.ROI,
                         dtype, er.CHANNELS)
        ref, rlab = torch.empty_like(out), torch.empty_like(olab)
        ops.warp_crop_patches(vol["imd"], vol["lad"], er.STARTS, er.FLIPS, _xyz(m), ref, rlab)
        torch.cuda.synchronize()
        assert torch.equal(out, ref) and torch.equal(olab, rlab), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_integer_shift_is_bit_identical_to_the_plain_crop(vol, dtype):
    """constant control grid with integer entries, identity map: the crop at the shifted starts, on the voxels
    whose shifted position is inside the volume (elsewhere the elastic gather clamps and the crop pads)"""
    shift = (2, -3, 1)
    for n in er.GRIDS:
        ctrl = np.empty((3,) + n, np.float32)
        for a in range(3):
            ctrl[a] = shift[a]
        out, olab = _run(vol["imd"], vol["lad"], er.STARTS, er.FLIPS, None, ctrl, er.ROI, dtype, er.CHANNELS)
        shifted = [[s[0], s[1] + shift[0], s[2] + shift[1], s[3] + shift[2]] for s in er.STARTS]
        ref, rlab = torch.empty_like(out), torch.empty_like(olab)
        ops.crop_patches(vol["imd"], vol["lad"], shifted, er.FLIPS, ref, rlab)
        torch.cuda.synchronize()
        compared = 0
        for w, (st, fl) in enumerate(zip(er.STARTS, er.FLIPS)):
            idx = [np.arange(er.ROI[d]) + st[1 + d] for d in range(3)]
            ok = [(i >= 0) & (i < er.VOLUME[d]) & (i + shift[d] >= 0) & (i + shift[d] < er.VOLUME[d])
                  for d, i in enumerate(idx)]
            both = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
            both = torch.from_numpy(np.ascontiguousarray(ar.flip(both, fl))).to(DEV)
            assert torch.equal(out[w][both], ref[w][both]) and torch.equal(olab[w][both], rlab[w][both]), (n, w)
            compared += int(both.sum())
        assert compared > 10000


def test_more_than_16_crops_per_call(vol):
    """37 crops = three launches give what one call per crop gives"""
    rng = np.random.RandomState(0)
    starts = [[0, int(rng.randint(-6, 28)), int(rng.randint(-6, 24)), int(rng.randint(-6, 34))] for _ in range(37)]
    flips = [int(v) for v in rng.randint(0, 8, 37)]
    _name, ctrl, m = er.kernel_cases(aug)[6]                       # (7, 7, 7), rotation + zoom, default A
    roi = (8, 6, 10)
    out, olab = _run(vol["imd"], vol["lad"], starts, flips, m, ctrl, roi, torch.float32, er.CHANNELS)
    for w in range(37):
        o1, l1 = _run(vol["imd"], vol["lad"], starts[w:w + 1], flips[w:w + 1], m, ctrl, roi, torch.float32,
                      er.CHANNELS)
        assert torch.equal(out[w], o1[0]) and torch.equal(olab[w], l1[0]), w


def test_the_grid_cap():
    """(16, 16, 16) = 4096 control points = 48 KB of LDS runs and matches the oracle; (16, 16, 17) raises, from the
    wrapper and from the C entry point"""
    from segmantic_amd import _lib
    shape, roi = (30, 26, 34), (12, 10, 16)
    image, label = er.volume(shape, 1, 5)
    imd, lad = _device_volume(image, label)
    vmax = float(np.abs(image).max())
    lip = max(float(np.abs(np.diff(image, axis=a)).max()) for a in (1, 2, 3))
    ctrl = er.control(shape, (16, 16, 16), None, 3)
    starts, flips = [[0, 2, 3, 4], [0, 18, 16, 18], [0, -3, 20, 25], [0, 9, -4, 7]], [0, 7, 2, 5]
    out, olab = _run(imd, lad, starts, flips, None, ctrl, roi, torch.float32, 1)
    _check_against_oracle("grid (16, 16, 16)", image, label, out, olab, starts, flips, None, ctrl, roi,
                          torch.float32, vmax, lip)
    big = torch.zeros((3, 16, 16, 17), device=DEV)
    with pytest.raises(ValueError, match="4096"):
        ops.elastic_warp_crop_patches(imd, lad, starts, flips, None, big, out, olab)
    a, b = ops.act(imd), ops.act(out)
    st = np.asarray(starts, dtype=np.int32)
    import ctypes as C
    rc = _lib.lib.segmi_elastic_warp_crop_patches(C.byref(a), lad.data_ptr(), st.ctypes.data_as(C.c_void_p), None, 4,
                                                  None, big.data_ptr(), 16, 16, 17, 0, C.byref(b), olab.data_ptr(),
                                                  None)
    assert rc == -1 and "control grid" in _lib.last_error()                  # SEGMI_EINVAL
    rc = _lib.lib.segmi_elastic_warp_crop_patches(C.byref(a), lad.data_ptr(), st.ctypes.data_as(C.c_void_p), None, 4,
                                                  None, big.data_ptr(), 3, 16, 16, 0, C.byref(b), olab.data_ptr(),
                                                  None)
    assert rc == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_two_dimensional_volume(dtype):
    """1 x 37 x 41 volume, 1 x 16 x 16 patches, grid (4, 6, 6): the d0 coordinate never moves"""
    shape, roi, n = (1, 37, 41), (1, 16, 16), (4, 6, 6)
    image, label = er.volume(shape, 2, 6)
    imd, lad = _device_volume(image, label)
    vmax = float(np.abs(image).max())
    lip = max(float(np.abs(np.diff(image, axis=a)).max()) for a in (2, 3))
    # every component drawn non-zero, d0 included: the kernel has to ignore it
    ctrl = np.random.RandomState(8).uniform(-1.0, 1.0, (3,) + n).astype(np.float32)
    m = np.eye(4)
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1.0]])
    ctr = np.eye(4)
    ctr[:3, 3] = [0, 18, 20]
    m = ctr @ rot @ np.linalg.inv(ctr)
    starts = [[0, 0, 3, 5], [0, 0, 25, 30], [0, 0, -5, 10], [0, 0, 11, -6], [0, 0, 40, 40], [0, 0, 10, 12]]
    flips = [0, 2, 4, 6, 0, 7]
    for mm in (None, m):
        out, olab = _run(imd, lad, starts, flips, mm, ctrl, roi, dtype, 2)
        _check_against_oracle(f"2-D {'affine' if mm is not None else 'identity'}", image, label, out, olab, starts,
                              flips, mm, ctrl, roi, dtype, vmax, lip)
        src, _a = er.elastic_coords(ctrl, mm, shape, starts[0][1:], roi)
        assert np.all(src[0] == 0.0)


# -------------------------------------------------------------------------------------- whole sampler
class _Net:
    device = torch.device(DEV)
    num_classes = 3
    spatial_size, num_samples, flip_prob = [24, 20, 16], 3, 0.5
    augment_spatial, augment_intensity = True, True
    augment_elastic = {"prob": 1.0}


def _sampler_cache():
    from tests.test_augment_gpu import _cache
    return _cache([(40, 36, 44), (40, 36, 44)], 2, 23)


def test_make_batch_matches_the_reference_chain():
    """two cached 40 x 36 x 44 volumes, num_samples 3, spatial + elastic (prob 1) + intensity: the records of
    ``draw_batch`` through ``elastic_ref.reference_chain``, with the bounds of test_augment_gpu's chain test and
    the warp bound widened by the elastic coordinate term only; the same seed twice is bit-identical"""
    from segmantic_amd.seg import trainer
    from tests.test_augment_gpu import INT_RTOL, KS_TIGHT, _spike_after_gibbs_ill_posed
    roi = tuple(_Net.spatial_size)
    cache, host = _sampler_cache()
    seed = 1
    records = trainer.draw_batch(_Net, cache, [0, 1], np.random.RandomState(seed))
    batch = trainer.apply_batch(_Net, cache, records)
    again = trainer.make_batch(_Net, cache, [0, 1], np.random.RandomState(seed))
    torch.cuda.synchronize()
    assert torch.equal(batch["image"], again["image"]) and torch.equal(batch["label"], again["label"])
    assert all(r["elastic"] is not None and r["elastic"].shape == (3, 7, 7, 7) for r in records)
    assert any(r["spatial"] is not None for r in records)                # the seed composes a field with a map
    got_i = batch["image"].cpu().numpy()
    got_l = batch["label"].cpu().numpy()[:, 0]
    assert got_i.shape == (6, 2) + roi
    row, compared, worst = 0, 0, 0.0
    for rec in records:
        image, label = host[rec["vid"]]
        ri, rl, src = er.reference_chain(image, label, rec, roi)
        shp = image.shape[1:]
        lip = max(float(np.abs(np.diff(image, axis=a)).max()) for a in (1, 2, 3))
        delta = er.coord_error(rec["elastic"], rec["spatial"], shp)
        delta_affine = er.affine_coord_error(rec["spatial"], shp)
        for i in range(len(rec["starts"])):
            g, want = got_i[row + i], ri[i]
            assert er.label_gate(got_l[row + i], rl[i], src[i], shp, delta) == 0
            scale = max(1.0, float(np.abs(want).max()))
            # test_augment_gpu's chain bound for a warped record is 5e-3 scale: the affine coordinate error passes
            # through x ** gamma, and with gamma = 0.5 next to the patch minimum an error e becomes sqrt(e range).
            # That bound is kept as it is; the elastic evaluation adds its own coordinate term
            # 3 (delta - delta_affine) lip to the gathered value, and only that is added here.  INT_RTOL and KS_TIGHT
            # are inside the 5e-3 as before
            assert INT_RTOL + KS_TIGHT < 5e-3
            tol = 5e-3 * scale + 3.0 * (delta - delta_affine) * lip
            if _spike_after_gibbs_ill_posed(want, rec["intensity"], i):
                continue
            compared += 1
            err = float(np.abs(g - want).max())
            worst = max(worst, err / tol)
            assert err <= tol, (rec["vid"], i, rec["flips"][i], err, tol)
        row += len(rec["starts"])
    assert row == 6 and compared >= 4
    print(f"MEASURED elastic chain: worst error / bound {worst:.3e}")


def test_the_prefetcher_builds_the_same_batches(monkeypatch):
    """SEGMI_PREFETCH=1: the control grid's upload and the gather run on the side stream; the batches equal the
    plain ones bit for bit"""
    from segmantic_amd.seg import trainer
    cache, _host = _sampler_cache()
    plain = []
    rng = np.random.RandomState(5)
    for ids in ([0, 1], [1, 0], [0, 1]):
        b = trainer.make_batch(_Net, cache, ids, rng)
        plain.append((b["image"].clone(), b["label"].clone()))
    monkeypatch.setenv("SEGMI_PREFETCH", "1")
    pre = trainer.BatchPrefetcher(_Net, cache)
    assert pre.enabled
    rng = np.random.RandomState(5)
    for k, ids in enumerate(([0, 1], [1, 0], [0, 1])):
        h = pre.prepare(ids, rng)
        b = pre.take(h)
        assert torch.equal(b["image"], plain[k][0]) and torch.equal(b["label"], plain[k][1]), k
        pre.release(h)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ training smoke
def test_three_training_steps_with_the_option_on(tmp_path):
    """``fit`` on the tiny configuration of the e2e tests (24^3 volumes, 16^3 patches, channels (16, 32, 64)):
    six training volumes = three steps; the loss is finite and the weights change"""
    from oracle.unet_ref import synthetic_batch
    from segmantic_amd.data.nifti import write_nifti
    from segmantic_amd.seg import trainer
    from segmantic_amd.seg.dataset import PairedDataSet
    from segmantic_amd.seg.monai_unet import Net, _ckpt_name
    root = tmp_path / "data"
    (root / "image").mkdir(parents=True)
    (root / "label").mkdir()
    n = 7
    for i in range(n):
        img, lab = synthetic_batch(1, 24, 3, seed=20 + i)
        write_nifti(root / "image" / f"c{i}.nii.gz",
                    (img[0, 0].numpy() * 100 + 300).astype(np.float32).transpose(2, 1, 0), np.eye(4))
        write_nifti(root / "label" / f"c{i}.nii.gz", lab[0, 0].numpy().astype(np.uint8).transpose(2, 1, 0), np.eye(4))
    dl = {"labels": {"1": "a", "2": "b"},
          "training": [{"image": f"image/c{i}.nii.gz", "label": f"label/c{i}.nii.gz"} for i in range(n - 1)],
          "validation": [{"image": f"image/c{n - 1}.nii.gz", "label": f"label/c{n - 1}.nii.gz"}],
          "test": [f"image/c{n - 1}.nii.gz"]}
    (root / "dataset.json").write_text(json.dumps(dl))
    torch.manual_seed(7)
    net = Net(num_classes=3, spatial_size=[16, 16, 16], channels=(16, 32, 64), strides=(2, 2))
    net.dataset = PairedDataSet.load_from_json(root / "dataset.json")
    net.num_samples = 2
    net.augment_spatial = True
    net.augment_elastic = {"prob": 1.0, "control_points": 5, "max_displacement": 0.5}
    before = {k: v.detach().clone().cpu() for k, v in net.state_dict().items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        trainer.fit(net, tmp_path / "out", 1, 5, [0], _ckpt_name)
    rows = (tmp_path / "out" / "logs" / "metrics.csv").read_text().strip().splitlines()
    assert len(rows) == 2 and np.isfinite(float(rows[1].split(",")[1]))
    after = net.state_dict()
    changed = [k for k in before if before[k].dtype.is_floating_point and not torch.equal(before[k], after[k].cpu())]
    assert len(changed) > 10, changed
