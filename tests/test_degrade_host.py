"""Host checks of the ``augment_degrade`` augmentation: the float64 oracle
(tests/helpers/degrade_ref.py) against the hash's known answers, the normal distribution, scipy's Gaussian filter
and the low-resolution gather's defining properties; the option's validation; the order of the sampler's random
draws; the bundle's refusals; and the gate of tests/test_degrade_gpu.py against seeded faults."""
import numpy as np
import pytest

from segmantic_amd.seg import augment as aug
from segmantic_amd.seg import trainer
from tests.helpers import degrade_ref as dr
from tests.test_elastic_host import _host_cache, _same_state, _todays_draws


# ------------------------------------------------------------------------------------------ noise
def test_hash_known_answers():
    assert int(dr.hash32(0, 0)) == 0x0
    assert int(dr.hash32(0, 1)) == 0x688990C0
    assert int(dr.hash32(1, 0)) == 0x6D523710
    # k wraps in uint32 arithmetic
    assert int(dr.hash32(2 ** 32 + 1, 0)) == 0x6D523710


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


@pytest.mark.parametrize("seed", dr.NOISE_SEEDS)
def test_noise_statistics(seed):
    """[16, 32, 32, 2] patch: mean, variance, fourth moment, the lag-1 correlation along each of the four axes and
    the correlation with the field of seed + 1, each within 5 standard errors of a standard normal's (variance of
    g^2 is 2, of g^4 is 105 - 9 = 96; a correlation of N independent pairs has standard error 1 / sqrt(N))"""
    shape = (16, 32, 32, 2)
    g = dr.gauss(seed, int(np.prod(shape)))
    n = g.size
    stats = {"mean": g.mean() / np.sqrt(1.0 / n), "variance": (g.var() - 1.0) / np.sqrt(2.0 / n),
             "fourth": ((g ** 4).mean() - 3.0) / np.sqrt(96.0 / n)}
    f = g.reshape(shape)
    for axis in range(4):
        a, b = np.take(f, np.arange(shape[axis] - 1), axis), np.take(f, np.arange(1, shape[axis]), axis)
        stats[f"lag1 axis {axis}"] = _corr(a.ravel(), b.ravel()) * np.sqrt(a.size)
    stats["seed + 1"] = _corr(g, dr.gauss((seed + 1) & 0xFFFFFFFF, n)) * np.sqrt(n)
    print(f"MEASURED noise seed {seed:#x}: worst {max(abs(v) for v in stats.values()):.2f} standard errors")
    for name, v in stats.items():
        assert abs(v) <= 5.0, (hex(seed), name, v)
    # the field is a function of (seed, element): the NDHWC index
    c4 = dr.noise_field(seed, (2, 3, 4, 5))
    assert np.array_equal(c4.transpose(1, 2, 3, 0).ravel(), dr.gauss(seed, 120))


# ------------------------------------------------------------------------------------------- blur
@pytest.mark.parametrize("shape,sigma", dr.BLUR_CASES)
def test_blur_oracle_equals_scipy(shape, sigma):
    import scipy.ndimage as ndi
    x = np.random.RandomState(sum(shape)).randn(2, *shape)
    want = np.stack([ndi.gaussian_filter(v, sigma, mode="reflect", truncate=4.0) for v in x])
    assert np.abs(dr.blur(x, sigma) - want).max() <= 1e-12
    radius, w = dr.blur_weights(sigma)
    assert radius == int(np.floor(4.0 * sigma + 0.5)) and len(w) == 2 * radius + 1 and abs(w.sum() - 1.0) < 1e-15
    # the reflect index for any i, also beyond one period (R larger than the extent)
    assert dr.reflect(np.arange(-9, 9), 3).tolist() == [2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2]


# ----------------------------------------------------------------------------------------- lowres
def test_lowres_properties():
    x = np.random.RandomState(3).randn(2, 9, 10, 16)
    assert np.array_equal(dr.lowres(x, (9, 10, 16)), x)                       # m == n: the identity
    one = dr.lowres(x, (1, 1, 1))                                              # m = 1: the constant x[floor(n / 2)]
    assert np.abs(one - x[:, 4:5, 5:6, 8:9]).max() == 0.0
    assert dr.lowres_src(9, 5).tolist() == [0, 2, 4, 6, 8]
    assert dr.lowres_src(16, 1).tolist() == [8] and dr.lowres_src(7, 7).tolist() == list(range(7))
    # one axis coarse, the others passed through: that axis alone is interpolated
    y = dr.lowres(x, (5, 10, 16))
    s0, s1, f = dr.lowres_axis(9, 5)
    assert np.abs(y - ((1 - f)[None, :, None, None] * x[:, s0] + f[None, :, None, None] * x[:, s1])).max() < 1e-15
    assert f.min() >= 0.0 and f.max() <= 1.0 and f[0] == 0.0
    # a coarse sample reproduces its own fine voxel where the fine voxel sits on it (n = 3 m: voxel 3 j + 1)
    z = np.random.RandomState(4).randn(1, 12, 1, 1)
    assert np.allclose(dr.lowres(z, (4, 1, 1))[:, 1::3], z[:, dr.lowres_src(12, 4)])
    assert aug.lowres_extents((9, 10, 16), [0.5, 1.0, 0.01]).tolist() == [[5, 5, 8], [9, 10, 16], [1, 1, 1]]
    assert aug.lowres_extents((1, 17, 19), [0.5]).tolist() == [[1, 9, 10]]


# ----------------------------------------------------------------------------------------- option
DEFAULTS = {"noise": {"prob": 0.1, "variance": (0.0, 0.1)}, "blur": {"prob": 0.2, "sigma": (0.5, 1.0)},
            "brightness": {"prob": 0.15, "multiplier": (0.75, 1.25)}, "lowres": {"prob": 0.25, "zoom": (0.5, 1.0)}}


def test_option_normal_form_and_defaults():
    assert aug.degrade_config(False) is None and aug.degrade_config(None) is None
    assert aug.degrade_config(True) == DEFAULTS and aug.degrade_config({}) == DEFAULTS
    cfg = aug.degrade_config({"noise": False, "blur": True, "brightness": {"prob": 1}, "lowres": {"zoom": [0.25, 0.5]}})
    assert cfg == {"noise": None, "blur": DEFAULTS["blur"], "brightness": {"prob": 1.0, "multiplier": (0.75, 1.25)},
                   "lowres": {"prob": 0.25, "zoom": (0.25, 0.5)}}
    assert aug.degrade_config({"blur": {"sigma": [2.0, 2.0]}})["blur"]["sigma"] == (2.0, 2.0)     # the cap itself
    assert aug.degrade_config({k: False for k in DEFAULTS}) is None                               # nothing left on
    assert aug.degrade_config(aug.degrade_config(True)) == DEFAULTS                               # idempotent


@pytest.mark.parametrize("bad,match", [
    ({"sharpen": True}, "unknown keys"),
    ({"noise": {"sigma": 1.0}}, "noise.*unknown keys"),
    ({"noise": {"prob": 1.5}}, "noise.prob"),
    ({"blur": {"prob": -0.1}}, "blur.prob"),
    ({"lowres": {"prob": "often"}}, "lowres.prob"),
    ({"noise": {"variance": [0.1, 0.0]}}, "noise.variance"),
    ({"noise": {"variance": [-0.1, 0.1]}}, "noise.variance"),
    ({"noise": {"variance": 0.1}}, "noise.variance"),
    ({"blur": {"sigma": [0.0, 1.0]}}, "blur.sigma"),
    ({"blur": {"sigma": [0.5, 2.2]}}, "blur.sigma"),
    ({"blur": {"sigma": [0.5, 1.0, 1.5]}}, "blur.sigma"),
    ({"brightness": {"multiplier": [0.5, float("inf")]}}, "brightness.multiplier"),
    ({"brightness": {"multiplier": [float("nan"), 1.0]}}, "brightness.multiplier"),
    ({"lowres": {"zoom": [0.0, 1.0]}}, "lowres.zoom"),
    ({"lowres": {"zoom": [0.5, 1.5]}}, "lowres.zoom"),
    ({"lowres": "coarse"}, "lowres"),
    ("yes", "augment_degrade"),
])
def test_option_validation_raises_by_name(bad, match):
    with pytest.raises(ValueError, match=match):
        aug.degrade_config(bad)


def test_the_network_validates_the_option_when_it_is_set():
    from segmantic_amd.seg.monai_unet import Net, train
    net = Net(num_classes=3, channels=(4, 8), strides=(2,))
    assert net.augment_degrade is False
    net.augment_degrade = True
    assert net.augment_degrade == DEFAULTS
    with pytest.raises(ValueError, match="unknown keys"):
        net.augment_degrade = {"gamma": True}
    assert net.augment_degrade == DEFAULTS                 # a refused value leaves the option as it was
    net.augment_degrade = False
    assert net.augment_degrade is False
    # train(): the option rides in the augmentation dictionary and is checked before anything else runs
    with pytest.raises(ValueError, match="blur.sigma"):
        train(datalist="none.json", output_dir="none", num_classes=3,
              augmentation={"augment_degrade": {"blur": {"sigma": [0.5, 3.0]}}})


def test_the_bundle_resolver_still_refuses_the_monai_counterparts():
    from segmantic_amd.utils.bundle import Compose, TransformSpec, plan_augmentation
    for name in ("RandGaussianNoised", "RandGaussianSmoothd", "RandScaleIntensityd",
                 "monai.transforms.RandGaussianNoise"):
        comp = Compose([TransformSpec(name, {"keys": ["image"], "prob": 0.1})])
        with pytest.raises(ValueError, match=f"{name.split('.')[-1]}.*augment_degrade"):
            plan_augmentation(comp)


# -------------------------------------------------------------------------------------- draw order
def _restated_degrade(rng, n, roi, cfg):
    """the draws of one volume in the stated order: per enabled transform rand(n), uniform(range, n) and, for the
    noise, randint(0, 2**32, n, uint32); the lowres extents follow from the zoom"""
    out = {}
    for name, field in (("noise", "variance"), ("blur", "sigma"), ("brightness", "multiplier"), ("lowres", "zoom")):
        c = cfg[name]
        if c is None:
            out[name] = None
            continue
        on = (rng.rand(n) < c["prob"]).astype(np.uint8)
        val = rng.uniform(c[field][0], c[field][1], n).astype(np.float32)
        if name == "noise":
            out[name] = (on, val, rng.randint(0, 2 ** 32, n, dtype=np.uint32))
        elif name == "lowres":
            m = [[1 if r == 1 else max(1, int(np.floor(r * float(z) + 0.5))) for r in roi] for z in val]
            out[name] = (on, val, np.asarray(m, dtype=np.int32))
        else:
            out[name] = (on, val)
    return out


def _draws_with_degrade(rng, net, cache, vol_ids, cfg):
    """today's sequence per volume, then the degrade draws directly after the intensity draws"""
    roi = list(net.spatial_size)
    out = []
    for vid in vol_ids:
        it = cache.items[vid]
        spatial = aug.draw_spatial(rng, it["label"].shape[1:]) if net.augment_spatial else None
        starts = trainer.crop_centers(rng, it, roi, net.num_samples, net.num_classes, spatial, None)
        for _ in starts:
            rng.rand(), rng.rand(), rng.rand()
        if net.augment_intensity:
            aug.draw_intensity(rng, len(starts), roi)
        out.append(_restated_degrade(rng, len(starts), roi, cfg))
    return out


def _same_draws(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert len(a[k]) == len(b[k]) and all(x.dtype == y.dtype and np.array_equal(x, y)
                                                  for x, y in zip(a[k], b[k])), k


@pytest.mark.parametrize("spatial,intensity", [(False, True), (True, True), (True, False)])
def test_draw_order(spatial, intensity):
    cache = _host_cache([(20, 18, 22), (17, 21, 25)], 0)

    class N:
        spatial_size, num_samples, num_classes, flip_prob = [8, 8, 8], 3, 3, 0.2
        augment_spatial, augment_intensity = spatial, intensity
    for seed in range(4):
        # off (attribute absent, or False): the records and the generator are those of today's sequence
        r1, r2 = np.random.RandomState(seed), np.random.RandomState(seed)
        recs = trainer.draw_batch(N, cache, [0, 1], r1)
        _todays_draws(r2, N, cache, [0, 1], extra_rand=False)
        assert _same_state(r1, r2)
        assert all(r["degrade"] is None for r in recs)

        class Off(N):
            augment_degrade = False
        r3 = np.random.RandomState(seed)
        recs_off = trainer.draw_batch(Off, cache, [0, 1], r3)
        assert _same_state(r1, r3)
        assert all(a["starts"] == b["starts"] and a["flips"] == b["flips"] and b["degrade"] is None
                   for a, b in zip(recs, recs_off))

        # on: the four transforms' draws directly after the intensity draws, per volume
        for value in (True, {"blur": False}, {"noise": False, "lowres": {"prob": 1.0, "zoom": [0.3, 0.6]}},
                      {"noise": {"prob": 1}, "blur": False, "brightness": False, "lowres": False}):
            class On(N):
                augment_degrade = value
            cfg = aug.degrade_config(value)
            r4, r5 = np.random.RandomState(seed), np.random.RandomState(seed)
            recs_on = trainer.draw_batch(On, cache, [0, 1], r4)
            want = _draws_with_degrade(r5, N, cache, [0, 1], cfg)
            assert _same_state(r4, r5) and not _same_state(r4, r1)
            assert recs_on[0]["starts"] == recs[0]["starts"]          # volume 0's crops precede every new draw
            for rec, w in zip(recs_on, want):
                _same_draws(rec["degrade"], w)
                for name in ("noise", "blur", "brightness", "lowres"):
                    assert (rec["degrade"][name] is None) == (cfg[name] is None)         # false: its draws are absent
    d = aug.draw_degrade(np.random.RandomState(1), 5, (1, 17, 19), aug.degrade_config({"lowres": {"prob": 1.0}}))
    on, zoom, m = d["lowres"]
    assert on.all() and m.dtype == np.int32 and (m[:, 0] == 1).all()
    assert m.tolist() == [[1, max(1, int(np.floor(17 * float(z) + 0.5))), max(1, int(np.floor(19 * float(z) + 0.5)))]
                          for z in zoom]


# ------------------------------------------------------------- the gate of the GPU test: seeded faults
def _gate_draws(n):
    """every transform on, with parameters at which each seeded fault shows: sigma 1.0 (ceil(3 sigma) = 3 against
    R = 4), multiplier 1.2, variance 0.05, the (9, 10, 16) patch on the coarse grid (5, 10, 8)"""
    on = np.ones(n, np.uint8)
    return {"noise": (on, np.full(n, 0.05, np.float32), np.arange(n, dtype=np.uint32) + 41),
            "blur": (on, np.full(n, 1.0, np.float32)), "brightness": (on, np.full(n, 1.2, np.float32)),
            "lowres": (on, np.full(n, 0.5, np.float32), np.tile(np.asarray([[5, 10, 8]], np.int32), (n, 1)))}


@pytest.mark.parametrize("fault", dr.FAULTS)
def test_the_gate_rejects_seeded_faults(fault):
    """the faulty oracle's output stands in for the kernel's"""
    x = dr.patches(2, (9, 10, 16), 2, 5)
    d = _gate_draws(2)
    for i in range(2):
        ref = dr.degrade_chain(x[i], d, i)
        err, tol = dr.gate(dr.degrade_chain(x[i], d, i, fault=fault), ref)
        assert err > 10 * tol, (fault, err, tol)
        assert dr.gate(ref.astype(np.float32), ref)[0] <= tol       # the oracle rounded to f32 passes


def test_the_gate_rejects_a_skipped_second_chunk():
    """20 patches, the last 4 left as they came (the second launch of 16 never made)"""
    x = dr.patches(20, (9, 10, 16), 1, 6)
    d = _gate_draws(20)
    ref = np.stack([dr.degrade_chain(x[i], d, i) for i in range(20)])
    got = ref.copy()
    got[16:] = x[16:]
    err, tol = dr.gate(got, ref)
    assert err > 10 * tol
    assert all(dr.gate(got[i], ref[i])[0] == 0.0 for i in range(16))
