"""Host checks of the elastic deformation: the float64 oracle
(tests/helpers/elastic_ref.py) against the spline's defining properties and against the host evaluation of
``seg/augment.py``, the inverse that carries the crop centre, the option's validation, the order of the
draws, and the gates of tests/test_elastic_gpu.py: they reject five seeded faults, and the label gate
exempts at most 1 % of any patch."""
import numpy as np
import pytest
import torch

from segmantic_amd.seg import augment as aug
from segmantic_amd.seg import trainer
from tests.helpers import augment_ref as ar
from tests.helpers import elastic_ref as er


def _points(shape, n, seed):
    rng = np.random.RandomState(seed)
    pts = rng.uniform(0, 1, (n, 3)) * (np.asarray(shape) - 1)
    corners = np.array([[0, 0, 0], np.asarray(shape) - 1.0])
    return np.concatenate([pts, corners])


# ------------------------------------------------------------------------------- spline properties
@pytest.mark.parametrize("n", [(4, 4, 4), (7, 7, 7), (4, 5, 9)])
def test_a_constant_grid_gives_that_constant_everywhere(n):
    shape = (33, 29, 41)
    ctrl = np.empty((3,) + n)
    ctrl[0], ctrl[1], ctrl[2] = 1.5, -0.25, 3.0
    u = er.displacement(ctrl, shape, _points(shape, 200, 0))
    assert np.abs(u - [1.5, -0.25, 3.0]).max() < 1e-14


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_grid_linear_in_the_control_index_gives_a_displacement_linear_in_t(axis):
    """control value = index along ``axis``: sum_j (k + j) w_j(f) = k + f + 1 = t + 1"""
    shape, n = (33, 29, 41), (5, 7, 9)
    idx = np.arange(n[axis], dtype=np.float64).reshape([-1 if a == axis else 1 for a in range(3)])
    ctrl = np.broadcast_to(idx, n)[None].repeat(3, 0)
    pts = _points(shape, 200, 1)
    t = pts[:, axis] * (n[axis] - 3) / (shape[axis] - 1)
    u = er.displacement(ctrl, shape, pts)
    assert np.abs(u - (t + 1.0)[:, None]).max() < 1e-13
    # the last voxel: the k clamp acts (t = n - 3 exactly) and the value is still t + 1
    last = np.zeros(3)
    last[axis] = shape[axis] - 1
    assert abs(er.displacement(ctrl, shape, last[None])[0, 0] - (n[axis] - 2)) < 1e-13


def test_an_axis_of_extent_one_is_inert():
    shape, n = (1, 37, 41), (4, 6, 6)
    ctrl = np.random.RandomState(2).uniform(-1, 1, (3,) + n)
    pts = _points(shape, 100, 3)
    u = er.displacement(ctrl, shape, pts)
    assert np.all(u[:, 0] == 0.0) and np.abs(u[:, 1:]).max() > 0.05
    # t = 0 on that axis: f = 0 weighs control points 0..2 with 1/6, 4/6, 1/6 and never reads point 3
    other = ctrl.copy()
    other[:, 3] += 5.0
    assert np.array_equal(er.displacement(other, shape, pts), u)
    assert np.array_equal(aug.elastic_displacement(ctrl, shape, pts)[:, 0], np.zeros(len(pts)))


@pytest.mark.parametrize("shape,n", [((33, 29, 41), (4, 4, 4)), ((33, 29, 41), (4, 5, 9)), ((1, 37, 41), (4, 6, 6)),
                                      ((40, 36, 44), (16, 16, 16))])
def test_the_host_evaluation_of_augment_equals_the_oracle(shape, n):
    """two formulations (the four polynomials in f; the cardinal B-spline of the distance), integer voxels
    included (the last one, where k is clamped)"""
    ctrl = np.random.RandomState(4).uniform(-2, 2, (3,) + n)
    pts = np.concatenate([_points(shape, 300, 5), np.floor(_points(shape, 100, 6))])
    assert np.abs(aug.elastic_displacement(ctrl, shape, pts) - er.displacement(ctrl, shape, pts)).max() < 1e-13


# ----------------------------------------------------------------------------------------- inverse
def _field_with_lipschitz_bound(shape, n, lip, seed):
    h = [(d - 1) / (k - 3) for d, k in zip(shape, n)]
    amp = lip / (2.0 * sum(1.0 / v for v in h))
    cfg = aug.elastic_config({"prob": 1.0, "control_points": list(n), "max_displacement": amp})
    assert abs(aug.elastic_amplitudes(shape, cfg)[1] - lip) < 1e-12
    return aug.draw_elastic(np.random.RandomState(seed), shape, cfg)


@pytest.mark.parametrize("lip", [0.3, 0.9])
@pytest.mark.parametrize("with_map", [False, True])
def test_forward_point_elastic_inverts_the_pull_back(lip, with_map):
    shape, n = (40, 36, 44), (7, 7, 7)
    m = er.rotation_zoom_map(aug, shape) if with_map else None
    mm = np.eye(4) if m is None else m
    checked = 0
    for seed in range(3):
        ctrl = _field_with_lipschitz_bound(shape, n, lip, seed)
        for s in _points(shape, 40, 10 + seed)[:40] * 0.6 + 0.2 * (np.asarray(shape) - 1):   # central source voxels
            p = aug.forward_point_elastic(m, ctrl, shape, s)
            if np.any(p < 0) or np.any(p > np.asarray(shape) - 1):
                continue                       # outside the volume the field is that of the nearest voxel inside
            back = mm[:3, :3] @ (p + er.displacement(ctrl, shape, p[None])[0]) + mm[:3, 3]
            assert np.abs(back - s).max() < 1e-6, (seed, s, back)
            checked += 1
    assert checked >= 60
    # without a field it is forward_point
    if with_map:
        zero = np.zeros((3,) + n, np.float32)
        assert np.allclose(aug.forward_point_elastic(m, zero, shape, (7, 8, 9)), aug.forward_point(m, (7, 8, 9)),
                           atol=1e-12)


# -------------------------------------------------------------------------------------- validation
def test_option_normal_form_and_defaults():
    assert aug.elastic_config(False) is None and aug.elastic_config(None) is None
    assert aug.elastic_config(True) == {"prob": 0.2, "control_points": (7, 7, 7), "max_displacement": None}
    cfg = aug.elastic_config({"prob": 1, "control_points": [4, 5, 9], "max_displacement": 1.5})
    assert cfg == {"prob": 1.0, "control_points": (4, 5, 9), "max_displacement": (1.5, 1.5, 1.5)}
    # the default amplitude is 0.12 control spacings and gives L = 0.72 on an isotropic grid
    amp, lip = aug.elastic_amplitudes((37, 37, 37), aug.elastic_config(True))
    assert np.allclose(amp, 0.12 * 36 / 4) and abs(lip - 0.72) < 1e-12
    amp, _ = aug.elastic_amplitudes((1, 37, 41), aug.elastic_config({"max_displacement": [3.0, 0.5, 0.5]}))
    assert amp[0] == 0.0 and amp[1] == 0.5


@pytest.mark.parametrize("bad,match", [
    ({"probability": 0.2}, "unknown keys"),
    ({"prob": 1.5}, "prob"),
    ({"prob": "often"}, "prob"),
    ({"control_points": 3}, "control_points"),
    ({"control_points": [7, 7]}, "control_points"),
    ({"control_points": 6.5}, "control_points"),
    ({"control_points": [16, 16, 17]}, "control_points"),          # 4352 > 4096
    ({"max_displacement": -1.0}, "max_displacement"),
    ({"max_displacement": [1.0, 2.0]}, "max_displacement"),
    ("yes", "augment_elastic"),
])
def test_option_validation_raises(bad, match):
    with pytest.raises(ValueError, match=match):
        aug.elastic_config(bad)


def test_the_network_validates_the_option_when_it_is_set():
    from segmantic_amd.seg.monai_unet import Net, train
    net = Net(num_classes=3, channels=(4, 8), strides=(2,))
    assert net.augment_elastic is False
    net.augment_elastic = True
    assert net.augment_elastic["control_points"] == (7, 7, 7)
    with pytest.raises(ValueError, match="unknown keys"):
        net.augment_elastic = {"sigma": 3}
    net.augment_elastic = False
    assert net.augment_elastic is False
    # train(): the option rides in the augmentation dictionary and is checked before anything else runs
    with pytest.raises(ValueError, match="control_points"):
        train(datalist="none.json", output_dir="none", num_classes=3,
              augmentation={"augment_elastic": {"control_points": 2}})


def test_the_no_fold_check_and_the_grid_cap_raise():
    shape = (33, 29, 41)
    for n in er.GRIDS:
        ok = er.largest_amplitude(shape, n)
        aug.elastic_amplitudes(shape, aug.elastic_config({"control_points": list(n), "max_displacement": ok}))
        with pytest.raises(ValueError, match="max_displacement"):
            aug.elastic_amplitudes(shape, aug.elastic_config({"control_points": list(n),
                                                             "max_displacement": ok * 1.002}))
    assert aug.elastic_config({"control_points": 16})["control_points"] == (16, 16, 16)     # 4096: the cap itself
    with pytest.raises(ValueError, match="4096"):
        aug.elastic_config({"control_points": [16, 16, 17]})
    # a fold-prone draw is refused by draw_elastic as well
    with pytest.raises(ValueError, match="fold"):
        aug.draw_elastic(np.random.RandomState(0), shape, aug.elastic_config({"prob": 1.0, "max_displacement": 9.0}))


def test_the_bundle_resolver_still_refuses_monai_elastic_transforms():
    from segmantic_amd.utils.bundle import Compose, TransformSpec, plan_augmentation
    for name in ("Rand3DElasticd", "monai.transforms.Rand3DElastic", "Rand2DElasticd"):
        comp = Compose([TransformSpec(name, {"keys": ["image", "label"], "sigma_range": [5, 7],
                                             "magnitude_range": [50, 150]})])
        with pytest.raises(ValueError, match="Gaussian-smoothed.*augment_elastic"):
            plan_augmentation(comp)


# -------------------------------------------------------------------------------------- draw order
def _host_cache(shapes, seed):
    """cache items as ``trainer.CachedVolumes`` builds them, on the host, with a host ``lookup``"""
    class Cache:
        items = []

        @staticmethod
        def lookup(item, positions):
            return item["class_all"][torch.from_numpy(np.asarray(positions, dtype=np.int64))].numpy()
    cache = Cache()
    cache.items = []
    rng = np.random.RandomState(seed)
    for shp in shapes:
        lab = torch.from_numpy(rng.randint(0, 3, shp)).float()
        flat = lab.reshape(-1).long()
        idx = [torch.nonzero(flat == k).reshape(-1) for k in range(3)]
        counts = np.array([int(t.numel()) for t in idx], dtype=np.int64)
        cache.items.append({"label": lab[None], "class_all": torch.cat(idx), "class_counts": counts,
                            "class_offsets": np.concatenate([[0], np.cumsum(counts)[:-1]])})
    return cache


def _todays_draws(rng, net, cache, vol_ids, extra_rand):
    """the individual draw functions in the order the sampler has always called them"""
    roi = list(net.spatial_size)
    for vid in vol_ids:
        it = cache.items[vid]
        spatial = aug.draw_spatial(rng, it["label"].shape[1:]) if net.augment_spatial else None
        if extra_rand:
            rng.rand()
        starts = trainer.crop_centers(rng, it, roi, net.num_samples, net.num_classes, spatial, None)
        for _ in starts:
            rng.rand(), rng.rand(), rng.rand()
        if net.augment_intensity:
            aug.draw_intensity(rng, len(starts), roi)


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.parametrize("spatial", [False, True])
def test_draw_order(spatial):
    cache = _host_cache([(20, 18, 22), (17, 21, 25)], 0)

    class N:
        spatial_size, num_samples, num_classes, flip_prob = [8, 8, 8], 3, 3, 0.2
        augment_spatial, augment_intensity = spatial, True
    for seed in range(4):
        # off (attribute absent, or False): the records and the generator are those of today's sequence
        r1, r2 = np.random.RandomState(seed), np.random.RandomState(seed)
        recs = trainer.draw_batch(N, cache, [0, 1], r1)
        _todays_draws(r2, N, cache, [0, 1], extra_rand=False)
        assert _same_state(r1, r2)
        assert all(r["elastic"] is None for r in recs)

        class Off(N):
            augment_elastic = False
        r3 = np.random.RandomState(seed)
        recs_off = trainer.draw_batch(Off, cache, [0, 1], r3)
        assert _same_state(r1, r3)
        assert all(a["starts"] == b["starts"] and a["flips"] == b["flips"] for a, b in zip(recs, recs_off))

        # on with prob 0: exactly one extra rand() per volume, directly after draw_spatial
        class Never(N):
            augment_elastic = {"prob": 0.0}
        r4, r5 = np.random.RandomState(seed), np.random.RandomState(seed)
        recs_never = trainer.draw_batch(Never, cache, [0, 1], r4)
        _todays_draws(r5, N, cache, [0, 1], extra_rand=True)
        assert _same_state(r4, r5) and not _same_state(r4, r1)
        assert all(r["elastic"] is None for r in recs_never)

    # on with prob 1: one rand(), then one uniform(size=n) per component in the order d0, d1, d2
    class Always(N):
        augment_elastic = {"prob": 1.0, "control_points": [5, 6, 7]}
    r6, r7 = np.random.RandomState(9), np.random.RandomState(9)
    rec = trainer.draw_batch(Always, cache, [1], r6)[0]
    shape = cache.items[1]["label"].shape[1:]
    sp = aug.draw_spatial(r7, shape) if spatial else None
    assert r7.rand() < 1.0
    amp, _ = aug.elastic_amplitudes(shape, aug.elastic_config(Always.augment_elastic))
    want = np.stack([r7.uniform(-a, a, size=(5, 6, 7)) for a in amp]).astype(np.float32)
    assert rec["elastic"].dtype == np.float32 and np.array_equal(rec["elastic"], want)
    assert (sp is None) == (rec["spatial"] is None)
    assert all(np.abs(rec["elastic"][a]).max() <= amp[a] for a in range(3))


# ----------------------------------------------------------- the gates of the GPU test: seeded faults
def _gate_inputs():
    image, label = er.volume()
    vmax = float(np.abs(image).max())
    lip = max(float(np.abs(np.diff(image, axis=a)).max()) for a in (1, 2, 3))
    return image, label, vmax, lip


@pytest.mark.parametrize("fault", er.FAULTS)
def test_the_gates_reject_seeded_faults(fault):
    """the faulty oracle's output stands in for the kernel's: both gates of tests/test_elastic_gpu.py see it,
    on an inside patch of the (7, 7, 7) and the (4, 5, 9) case with the rotation + zoom map"""
    image, label, vmax, lip = _gate_inputs()
    cases = {name: (ctrl, m) for name, ctrl, m in er.kernel_cases(aug)}
    for name in ("grid(7, 7, 7) affine Adefault", "grid(4, 5, 9) affine Amax"):
        ctrl, m = cases[name]
        delta = er.coord_error(ctrl, m, er.VOLUME)
        for w in (0, 8):                                        # inside starts, flip codes 0 and 0
            st = er.STARTS[w][1:]
            ri, rl, src = er.elastic_warp_crop(image, label, ctrl, m, st, er.ROI)
            bi, bl, _ = er.elastic_warp_crop(image, label, ctrl, m, st, er.ROI, fault=fault)
            err, tol = er.image_gate(bi, ri, delta, lip, vmax)
            assert err > 10 * tol, (name, fault, err, tol)           # the image gate rejects it
            assert er.label_gate(bl, rl, src, er.VOLUME, delta) > 0, (name, fault)    # and so does the label gate
            # the unfaulted oracle passes its own gates
            assert er.image_gate(ri, ri, delta, lip, vmax)[0] <= 0 and er.label_gate(rl, rl, src, er.VOLUME, delta) == 0


def test_the_label_gate_exempts_at_most_one_percent_of_any_patch():
    """the inputs of test_elastic_gpu's kernel test: delta <= 5e-4 voxel, and near_half(src, 2 delta) holds on
    at most 1 % of every patch -- the gate may leave out this much and no more"""
    worst_share, worst_delta = 0.0, 0.0
    for name, ctrl, m in er.kernel_cases(aug):
        delta = er.coord_error(ctrl, m, er.VOLUME)
        worst_delta = max(worst_delta, delta)
        assert delta <= 5e-4, (name, delta)
        for st in er.STARTS:
            src, _a = er.elastic_coords(ctrl, m, er.VOLUME, st[1:], er.ROI)
            share = float(ar.near_half(src, er.VOLUME, 2 * delta).mean())
            worst_share = max(worst_share, share)
            assert share <= 0.01, (name, st, share)
    print(f"MEASURED label exclusion: worst share {worst_share:.4%}, worst delta {worst_delta:.3e}")
