"""``segmi_degrade_augment`` (noise, blur, brightness, low resolution) and the sampler around it
against the float64 oracle of tests/helpers/degrade_ref.py.

Bound, everywhere: ``|got - ref| <= INT_RTOL max(1, max |ref|)`` with ``INT_RTOL = 2e-5``, the bound
tests/test_augment_gpu.py holds the f32 elementwise chain to (``degrade_ref.gate``, which tests/test_degrade_host.py
holds to six seeded faults).  The measured error of every case is recorded as a property.

No launch of the entry point caps its grid and loops: every workgroup takes a fixed share (1024 elements of the
pointwise and copy kernels, 4096 of the lowres gather, one tile of the blur), so there is no case past a cap; the
shapes below take several workgroups with a ragged last one in each kernel."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import _lib, ops  # noqa: E402
from segmantic_amd.seg import augment as aug  # noqa: E402
from tests.helpers import degrade_ref as dr  # noqa: E402

DEV = "cuda:0"
SENTINEL = 7.0


def _ops_args(d):
    low = d.get("lowres")
    return d.get("noise"), d.get("blur"), d.get("brightness"), None if low is None else (low[0], low[-1])


def _run(x, d):
    """[n, C, d0, d1, d2] float64 -> the same after ``ops.degrade_augment`` with the draws ``d``; the patches sit
    between two guard patches that must keep their bits"""
    n = x.shape[0]
    nd = np.ascontiguousarray(x.transpose(0, 2, 3, 4, 1), dtype=np.float32)
    buf = torch.full((n + 2,) + nd.shape[1:], SENTINEL, device=DEV)
    buf[1:-1] = torch.from_numpy(nd).to(DEV)
    ops.degrade_augment(buf[1:-1], *_ops_args(d))
    torch.cuda.synchronize()
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
    return buf[1:-1].cpu().numpy().astype(np.float64).transpose(0, 4, 1, 2, 3), nd


def _hold(record_property, name, got, ref):
    err, tol = dr.gate(got, ref)
    record_property(f"{name} error / bound", err / tol)
    print(f"MEASURED {name}: {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (name, err, tol)


def _selected(d, i):
    return any(d.get(k) is not None and bool(d[k][0][i]) for k in ("noise", "blur", "brightness", "lowres"))


def _against_chain(record_property, name, x, d):
    got, nd = _run(x, d)
    for i in range(x.shape[0]):
        if _selected(d, i):
            _hold(record_property, f"{name} patch {i}", got[i], dr.degrade_chain(x[i], d, i))
        else:
            assert np.array_equal(got[i].transpose(1, 2, 3, 0).astype(np.float32), nd[i]), (name, i)   # bits kept
    return got


# ------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("shape,c", [((5, 6, 7), 1), ((16, 32, 32), 2)])
def test_noise_alone(record_property, shape, c):
    """on zeros and on a ramp, seeds 0 and 0xFFFFFFFF: the field is that of (seed, NDHWC element index)"""
    per = int(np.prod(shape)) * c
    ramp = (np.arange(per, dtype=np.float64) / per * 4.0 - 2.0).reshape(shape + (c,)).transpose(3, 0, 1, 2)
    x = np.stack([np.zeros_like(ramp), np.zeros_like(ramp), ramp, ramp, ramp]).astype(np.float32).astype(np.float64)
    d = {"noise": (np.array([1, 1, 1, 1, 0], np.uint8), np.array([0.1, 0.03, 0.1, 0.0625, 0.1], np.float32),
                   np.array([0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 5], np.uint32))}
    got = _against_chain(record_property, f"noise {shape} c{c}", x, d)
    # on zeros the result is the scaled field itself
    want = np.sqrt(float(np.float32(0.1))) * dr.noise_field(0, x[0].shape)
    _hold(record_property, f"noise field {shape} c{c}", got[0], want)


# ------------------------------------------------------------------------------------------- blur
@pytest.mark.parametrize("shape,sigma,c", [(s, g, 1) for s, g in dr.BLUR_CASES] + [((33, 35, 37), 1.0, 2)])
def test_blur_alone(record_property, shape, sigma, c):
    """the five host cases (R from 2 to 8, R larger than the extent, a 2-D patch) and 33 x 35 x 37 with two
    distinct channels: more than one tile with a ragged remainder on every axis; the second patch is not selected"""
    x = dr.patches(2, shape, c, 11)
    d = {"blur": (np.array([1, 0], np.uint8), np.full(2, sigma, np.float32))}
    _against_chain(record_property, f"blur {shape} sigma {sigma}", x, d)


# ----------------------------------------------------------------------------------------- lowres
@pytest.mark.parametrize("shape,m", [((9, 10, 16), (5, 10, 8)), ((9, 10, 16), (1, 1, 1)), ((1, 17, 19), (1, 9, 10))])
def test_lowres_alone(record_property, shape, m):
    x = dr.patches(2, shape, 2, 12)
    d = {"lowres": (np.array([1, 0], np.uint8), np.full(2, 0.5, np.float32), np.tile(np.asarray([m], np.int32), (2, 1)))}
    _against_chain(record_property, f"lowres {shape} m {m}", x, d)


def test_lowres_onto_the_fine_grid_keeps_every_bit():
    x = dr.patches(2, (9, 10, 16), 2, 13)
    x[0, 0, 0, 0, 0] = -0.0
    d = {"lowres": (np.ones(2, np.uint8), np.ones(2, np.float32), np.tile(np.asarray([[9, 10, 16]], np.int32), (2, 1)))}
    got, nd = _run(x, d)
    assert np.array_equal(got.transpose(0, 2, 3, 4, 1).astype(np.float32).view(np.uint32), nd.view(np.uint32))


# ------------------------------------------------------------------------------------------ chain
def _combo_draws(n, shape, seed, bits):
    d = dr.draws(n, shape, seed)
    for k, name in enumerate(("noise", "blur", "brightness", "lowres")):
        d[name] = (np.asarray([(b >> k) & 1 for b in bits], np.uint8),) + d[name][1:]
    return d


def test_all_sixteen_combinations(record_property):
    """12 x 13 x 14 patches with two channels, patch i takes the transforms of the bits of i (sigma up to 2.0);
    patch 0 is selected by nothing and keeps its bits"""
    shape = (12, 13, 14)
    x = dr.patches(16, shape, 2, 14)
    _against_chain(record_property, "combination", x, _combo_draws(16, shape, 3, list(range(16))))


def test_more_than_16_patches(record_property):
    """20 patches = two launches, mixed flags, the workspace sized for the larger launch"""
    shape = (9, 10, 16)
    bits = [int(v) for v in np.random.RandomState(2).randint(0, 16, 20)]
    bits[17], bits[19] = 15, 10                                 # the second launch blurs and gathers too
    x = dr.patches(20, shape, 1, 15)
    _against_chain(record_property, "20 patches", x, _combo_draws(20, shape, 4, bits))


# -------------------------------------------------------------------------------------- refusals
def test_argument_refusals():
    shape = (6, 7, 8)
    x = torch.full((17,) + shape + (1,), SENTINEL, device=DEV)
    on = np.ones(17, np.uint8)
    with pytest.raises(ValueError, match="sigma"):
        ops.degrade_augment(x[:2], blur=(on[:2], np.array([1.0, 2.2], np.float32)))
    ws = torch.empty(int(_lib.lib.segmi_degrade_workspace(16, *shape, 1)), dtype=torch.uint8, device=DEV)
    assert ws.numel() == 16 * 6 * 7 * 8 * 4
    sig = np.full(17, 2.2, np.float32)
    mul = np.full(17, 1.5, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(count, blur_sigma, workspace):
        return _lib.lib.segmi_degrade_augment(C.c_void_p(x.data_ptr()), count, *shape, 1, None, None, None,
                                              None if blur_sigma is None else p(on),
                                              None if blur_sigma is None else p(blur_sigma), p(on), p(mul), None, None,
                                              workspace, None)
    assert call(2, sig, C.c_void_p(ws.data_ptr())) == -1 and "sigma" in _lib.last_error()          # SEGMI_EINVAL
    assert call(17, None, C.c_void_p(ws.data_ptr())) == -1 and "patches" in _lib.last_error()
    sig[:] = 1.0
    assert call(2, sig, None) == -1 and "workspace" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all())                          # nothing was launched
    # no flag set: nothing to do, with or without a workspace
    off = np.zeros(17, np.uint8)
    assert _lib.lib.segmi_degrade_augment(C.c_void_p(x.data_ptr()), 16, *shape, 1, None, None, None, None, None,
                                          p(off), p(mul), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all())


# -------------------------------------------------------------------------------------- whole sampler
class _Net:
    device = torch.device(DEV)
    num_classes = 3
    spatial_size = [24, 20, 16]
    augment_intensity = False


ALWAYS = {k: {"prob": 1.0} for k in ("noise", "blur", "brightness", "lowres")}


def _smooth_cache(shapes, c):
    """``tests.test_augment_gpu._cache`` with smooth images (slopes of at most 0.02 per voxel), so that the warp
    gather's f32 coordinate error stays below the bound (see ``test_make_batch_matches_the_reference_chain``)"""
    from tests.test_augment_gpu import _cache
    cache, host = _cache(shapes, c, 31)
    for k, shp in enumerate(shapes):
        z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shp], indexing="ij")
        img = np.stack([0.8 * np.sin(z / 40.0 + ch) * np.cos(y / 50.0 - ch) + 0.5 * np.sin(x / 35.0 + 2.0 * ch) + ch
                        for ch in range(c)]).astype(np.float32)
        t = torch.from_numpy(img)
        cache.items[k]["image"] = t.to(DEV)
        cache.items[k]["image_ndhwc"] = t.permute(1, 2, 3, 0).contiguous()[None].to(DEV)
        host[k] = (img.astype(np.float64), host[k][1])
    return cache, host


@pytest.fixture(scope="module")
def smooth():
    return _smooth_cache([(40, 36, 30), (34, 28, 26)], 2)


# (augment_degrade, flip_prob, augment_spatial, num_samples, seed); the seeds give draws in which every transform
# fires at least once (asserted below) and, with augment_spatial, a warp
CHAIN = [(ALWAYS, 0.5, False, 4, 0), (ALWAYS, 1.0, True, 4, 1), (True, 0.5, False, 20, 1), (True, 0.5, True, 20, 2),
         (ALWAYS, 0.5, True, 20, 2)]


@pytest.mark.parametrize("value,flip_prob,spatial,num_samples,seed", CHAIN)
def test_make_batch_matches_the_reference_chain(record_property, smooth, value, flip_prob, spatial, num_samples, seed):
    """2 volumes x num_samples patches of 24 x 20 x 16 through ``degrade_ref.reference_chain``.  The intensity
    transforms are off here: AdjustContrast's x ** gamma with gamma < 1 turns an f32 rounding e next to the patch
    minimum into sqrt(e), which no f32 chain in front of it can hold to INT_RTOL (tests/test_augment_gpu.py carries
    5e-3 for its warped records for that reason); ``test_the_order_with_the_intensity_transforms`` covers them.  The
    volumes are smooth, so that the gather's own f32 coordinate error (3 delta lip + 16 EPS32 vmax of
    ``elastic_ref.image_gate``) takes at most half of INT_RTOL, where the bound is at least INT_RTOL: asserted on the inputs below.
    The label equals the option-off label of the same records, and so does every image nothing fired for."""
    from segmantic_amd.seg import trainer
    from tests.helpers import elastic_ref as er
    cache, host = smooth
    roi = tuple(_Net.spatial_size)

    class N(_Net):
        augment_spatial, augment_degrade = spatial, value
    N.num_samples, N.flip_prob = num_samples, flip_prob
    records = trainer.draw_batch(N, cache, [0, 1], np.random.RandomState(seed))
    batch = trainer.apply_batch(N, cache, records)
    plain = trainer.apply_batch(N, cache, [dict(r, degrade=None) for r in records])
    torch.cuda.synchronize()
    assert torch.equal(batch["label"], plain["label"])
    got_i, plain_i = batch["image"].cpu().numpy(), plain["image"].cpu().numpy()
    assert got_i.shape == (2 * num_samples, 2) + roi
    fired = np.zeros(4, int)
    row = 0
    for rec in records:
        image, label = host[rec["vid"]]
        ri, rl = dr.reference_chain(image, label, rec, roi)
        if rec["spatial"] is None:
            assert np.array_equal(batch["label"].cpu().numpy()[row:row + num_samples, 0], rl)
        else:
            lip = max(float(np.abs(np.diff(image, axis=a)).max()) for a in (1, 2, 3))
            vmax = float(np.abs(image).max())
            gather = 3.0 * er.affine_coord_error(rec["spatial"], image.shape[1:]) * lip + 16.0 * er.EPS32 * vmax
            assert gather <= dr.INT_RTOL / 2, gather
        d = rec["degrade"]
        fired += [int(np.asarray(d[k][0]).sum()) for k in ("noise", "blur", "brightness", "lowres")]
        for i in range(num_samples):
            if _selected(d, i):
                _hold(record_property, f"chain volume {rec['vid']} patch {i}", got_i[row + i], ri[i])
            else:
                assert np.array_equal(got_i[row + i], plain_i[row + i])
        row += num_samples
    assert fired.min() >= 1, fired
    if spatial:
        assert any(r["spatial"] is not None for r in records)
    if flip_prob == 1.0:
        assert all(f == 7 for r in records for f in r["flips"])


def test_the_order_with_the_intensity_transforms(smooth):
    """gather -> degrade -> intensity -> k-space: ``apply_batch`` with everything on equals, bit for bit, the plain
    gather followed by ``ops.degrade_augment`` and the intensity / k-space ops with their flipped parameters"""
    from segmantic_amd.seg import trainer
    cache, _host = smooth
    roi = list(_Net.spatial_size)

    class N(_Net):
        augment_spatial, augment_intensity, augment_degrade = True, True, ALWAYS
        num_samples, flip_prob = 4, 0.5
    records = trainer.draw_batch(N, cache, [0, 1], np.random.RandomState(3))
    assert any(np.asarray(t[0]).any() for r in records for t in r["intensity"])
    full = trainer.apply_batch(N, cache, records)["image"]
    bare = trainer.apply_batch(N, cache, [dict(r, degrade=None, intensity=None) for r in records])["image"]
    row = 0
    for rec in records:
        x = bare[row:row + 4].permute(0, 2, 3, 4, 1).contiguous()
        ops.degrade_augment(x, *_ops_args(rec["degrade"]))
        con, hist, bias, gibbs, spike = aug.flip_params(rec["intensity"], rec["flips"], roi)
        ops.intensity_augment(x, con, hist, bias)
        ops.kspace_augment(x, gibbs, spike, rec["flips"])
        torch.cuda.synchronize()
        assert torch.equal(full[row:row + 4], x.permute(0, 4, 1, 2, 3)), rec["vid"]
        assert not torch.equal(full[row:row + 4], bare[row:row + 4])
        row += 4


# ------------------------------------------------------------------------------------ end to end
def test_training_with_the_option_on(tmp_path):
    """``train()`` with ``augmentation: {augment_degrade: true}`` on the tiny configuration of the e2e tests (24^3
    volumes, 16^3 patches, channels (16, 32, 64)): it runs, the loss is finite and a checkpoint is written"""
    from segmantic_amd.seg.monai_unet import train
    from tests.test_e2e_gpu import _write_dataset
    datalist = _write_dataset(tmp_path / "data")
    out = tmp_path / "results"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = train(datalist=datalist, output_dir=out, spatial_size=[16, 16, 16], channels=(16, 32, 64), strides=(2, 2),
                    max_epochs=2, mixed_precision=False, num_samples=2, gpu_ids=[0],
                    augmentation={"augment_degrade": True})
    assert net.augment_degrade == aug.degrade_config(True) and not net.config_augmentation
    assert len(list(out.glob("epoch=*-val_loss=*-val_dice=*.ckpt"))) >= 1
    rows = (out / "logs" / "metrics.csv").read_text().strip().splitlines()
    assert len(rows) == 3 and all(np.isfinite(float(r.split(",")[1])) for r in rows[1:])
