"""The N4 cases shared by tests/test_modality_host.py and the GPU tests, and the bounds derived from them
("Tests").  Every fit case runs the numpy oracle twice, with the FFT form of the sharpening
(`n4_ref.sharpen`, the contract) and with the kernel's arithmetic (`n4_ref.sharpen_direct`); the deviation
between the two, D_case, is what a GPU bound is derived from.  Results are cached and must not be modified."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from . import n4_ref as ref

MARGIN = 1000.0        # on D_case: device exp / log / cospi an ulp or two from numpy's, other summation orders
ZERO_D_REL = 1e-13     # of the quantity's max magnitude, where the two forms coincide (D_case == 0)
F64_CAP_REL = 1e-7     # no bound on an f64 quantity may exceed this fraction of its max magnitude

# (bins, fwhm, noise, control_points): P = 128, 256, 512, 1024, 1024 and 4
SHARPEN_SETTINGS = [(64, 0.15, 0.01, 4), (128, 0.3, 0.01, 5), (256, 0.15, 0.1, 4), (257, 0.1, 0.01, 6),
                    (512, 0.15, 0.001, 4), (2, 0.15, 0.01, 4)]
DEFAULT_SETTINGS = (200, 0.15, 0.01, 4)

# stopping before the cap: see FIT_CASES["stop"]
STOP_CAPS = (3, 20, 20)
STOP_THRESHOLD = 0.00095


def bound(d, magnitude):
    """the bound on an f64 quantity from its D_case and its max magnitude.  D_case is one sample: where it
    is only a few ulps of the quantity (the CV of the "poisoned" case: 8.7e-18, five ulps), the two forms
    agree that closely by luck, the bound is correspondingly tight, and another numpy or libm may move it"""
    b = MARGIN * d if d > 0 else ZERO_D_REL * magnitude
    assert b <= F64_CAP_REL * magnitude, (d, magnitude)
    return b


@functools.lru_cache(maxsize=None)
def shrunk_phantom(shape=(48, 56, 52), seed=7, factor=2):
    """(image, Otsu mask) of a phantom, both shrunk"""
    img, _, _ = ref.phantom(shape, seed=seed)
    mask, _, _ = ref.otsu_threshold(img)
    return ref.shrink(img, factor), ref.shrink(mask, factor)


@functools.lru_cache(maxsize=None)
def poisoned_phantom():
    """(image, user mask) at full size: NaN, +Inf, 0 and negative voxels inside the mask, at voxels that the
    shrink by 2 keeps (odd indices: o = 1 on every axis of (48, 56, 52)) and at some that it drops"""
    img, _, _ = ref.phantom((48, 56, 52), seed=7)
    mask, _, _ = ref.otsu_threshold(img)
    img = img.copy()
    mask = mask.copy()
    mask[20:30, 20:36, 18:34] = 1
    img[21, 25, 21:29] = np.nan
    img[23, 27, 20:30:3] = np.inf
    img[25, 21:35, 25] = 0.0
    img[27, 29, 19:33] = -3.0
    img[22, 24, 22] = np.nan      # dropped by the shrink
    img[25:29, 30:34, 27] = -np.inf
    return img, mask


def fit_input(name):
    """(image, mask) that a fit or sharpening case runs on, by the input's name"""
    if name == "big":
        img, _, _ = ref.phantom((66, 72, 70), seed=21)
        mask, _, _ = ref.otsu_threshold(img)
        return img, mask
    if name == "2d":
        img, _, _ = ref.phantom((90, 110), seed=3)
        mask, _, _ = ref.otsu_threshold(img)
        return img, mask
    if name == "2d-shrunk":
        img, mask = fit_input("2d")
        return ref.shrink(img, 2), ref.shrink(mask, 2)
    if name == "seed11":
        return shrunk_phantom((40, 44, 36), 11)
    if name == "poisoned":
        img, mask = poisoned_phantom()
        return ref.shrink(img, 2), ref.shrink(mask, 2)
    if name == "seed2":   # the (40, 48, 44) seed-2 phantom of test_sharpening_step_against_oracle
        img, _, _ = ref.phantom((40, 48, 44), seed=2)
        mask, _, _ = ref.otsu_threshold(img)
        return img, mask
    return shrunk_phantom()


# name -> (input, iterations, threshold, (bins, fwhm, noise, control_points))
FIT_CASES = {
    "big": ("big", (2, 2), 0.0, DEFAULT_SETTINGS),
    "levels4": ("seed7", (2, 2, 2, 2), 0.0, DEFAULT_SETTINGS),
    "2d": ("2d", (4, 4, 3), 0.0, DEFAULT_SETTINGS),
    "2d-bias-correct": ("2d-shrunk", (4, 4, 4), 0.001, DEFAULT_SETTINGS),
    "stop": ("seed7", STOP_CAPS, STOP_THRESHOLD, DEFAULT_SETTINGS),
    "poisoned": ("poisoned", (3, 3), 0.0, DEFAULT_SETTINGS),
    # the cases of tests/test_modality_gpu.py
    "fixed-654": ("seed7", (6, 5, 4), 0.0, DEFAULT_SETTINGS),
    "seed11-436": ("seed11", (4, 3, 6), 0.001, DEFAULT_SETTINGS),
    "end-to-end-888": ("seed7", (8, 8, 8), 0.001, DEFAULT_SETTINGS),
}
for _s in SHARPEN_SETTINGS[:-1]:  # no fit at bins = 2: see test_modality_host.test_fit_at_two_bins_is_rounding_noise
    FIT_CASES["bins%d" % _s[0]] = ("seed7", (3, 3), 0.0, _s)


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """the oracle's two runs of a fit case and their deviation: .img, .mask, .iterations, .threshold,
    .settings, .lattice / .field / .elapsed / .cv / .trace (FFT form), .direct (the same of the direct form),
    .d_lattice, .d_field, .d_cv (D_case) and .b_lattice, .b_field, .b_cv (the derived bounds)"""
    inp, iterations, threshold, (bins, fwhm, noise, cp) = FIT_CASES[name]
    img, mask = fit_input(inp)
    kw = dict(iterations=iterations, control_points=cp, bins=bins, fwhm=fwhm, noise=noise, threshold=threshold,
              trace=True)
    a = ref.n4(img, mask, **kw)
    b = ref.n4(img, mask, sharpen_fn=ref.sharpen_direct, **kw)
    c = SimpleNamespace(name=name, img=img, mask=mask, iterations=iterations, threshold=threshold,
                        settings=(bins, fwhm, noise, cp), lattice=a[0], field=a[1], elapsed=a[2], cv=a[3],
                        trace=a[4], direct=SimpleNamespace(lattice=b[0], field=b[1], elapsed=b[2], cv=b[3],
                                                           trace=b[4]))
    assert a[2] == b[2], (name, a[2], b[2])
    c.d_lattice = float(np.abs(a[0] - b[0]).max())
    c.d_field = float(np.abs(a[1] - b[1]).max())
    c.d_cv = abs(a[3] - b[3])
    c.b_lattice = bound(c.d_lattice, float(np.abs(a[0]).max()))
    c.b_field = bound(c.d_field, float(np.abs(a[1]).max()))
    c.b_cv = bound(c.d_cv, abs(a[3]))
    return c


def log_image(img, mask):
    """(log values with NaN off the fit set, the fit set)"""
    v = ref.fit_set(img, mask)
    return np.where(v, np.log(np.where(v, np.asarray(img, np.float64), 1.0)), np.nan), v


@functools.lru_cache(maxsize=None)
def sharpen_case(inp, settings):
    """one sharpening of the input's log image in both forms: .L, .valid, .E, .S (FFT form), .range, .d_E and
    .d_S (D_case, absolute) and the bounds .b_E, .b_S"""
    img, mask = fit_input(inp)
    L, v = log_image(img, mask)
    bins, fwhm, noise = settings[:3]
    E, S = ref.sharpen(L[v], bins, fwhm, noise)
    Ed, Sd = ref.sharpen_direct(L[v], bins, fwhm, noise)
    c = SimpleNamespace(L=L, valid=v, E=E, S=S, Ed=Ed, Sd=Sd, range=float(L[v].max() - L[v].min()))
    c.d_E = float(np.abs(E - Ed).max())
    c.d_S = float(np.abs(S - Sd).max())
    c.b_E = bound(c.d_E, float(np.abs(E).max()))
    c.b_S = bound(c.d_S, float(np.abs(S).max()))
    return c


@functools.lru_cache(maxsize=None)
def ba_deviation(spans, two_d=False):
    """max |ba_fit - ba_fit_points| / max |ba_fit| on a small grid at `spans` spans: the relative deviation
    between the separable and the point-by-point form of one BA step"""
    rng = np.random.default_rng(100 + spans)
    shape = (1, 9, 11) if two_d else (7, 6, 9)
    r = rng.normal(size=shape)
    valid = rng.random(shape) > 0.3
    a = ref.ba_fit(r, valid, spans)
    return float(np.abs(a - ref.ba_fit_points(r, valid, spans)).max() / np.abs(a).max())


def evaluate_bound(lattice, shape3):
    """(bound, deviation) of the f32 evaluation: 4 x max |evaluate_f32 - evaluate|, at least 2^-22 max |lattice|"""
    lat = np.asarray(lattice, np.float64)
    d = float(np.abs(ref.evaluate_f32(lat, shape3).astype(np.float64) - ref.evaluate(lat, shape3)).max())
    return max(4.0 * d, 2.0 ** -22 * float(np.abs(lat).max())), d


# ------------------------------------------------------------------ checks shared by the GPU tests
def deviation(got, want):
    """max |got - want| over every element; NaN positions must coincide"""
    got = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    if nan.all():
        return 0.0
    return float(np.abs(got[~nan] - want[~nan]).max())


def check(record_property, key, got, want, bound):
    d = deviation(got, want)
    record_property(key + "_bound", bound)
    record_property(key + "_gpu", d)
    print(f"{key}: bound {bound:.3e}, MI355X {d:.3e}")
    assert d <= bound, (key, d, bound)
    return d


def full(values, valid):
    out = np.full(valid.shape, np.nan)
    out[valid] = values
    return out


def lat3(lattice):
    lattice = np.asarray(lattice)
    return lattice if lattice.ndim == 3 else lattice[None]


def check_fit(record_property, c, lat, elapsed, cv, field=None, key=None):
    key = key or c.name
    assert elapsed == c.elapsed
    check(record_property, key + "_lattice", lat, lat3(c.lattice), c.b_lattice)
    check(record_property, key + "_cv", np.float64(cv), np.float64(c.cv), c.b_cv)
    if field is not None:
        check(record_property, key + "_field", field, c.field, c.b_field)


def check_divided(record_property, key, got, x, lattice, b_lattice):
    """x / exp(field) in f32: the field is off by at most the f32 evaluation bound plus the lattice's own bound
    (the cubic weights are a convex combination), then expf and the division, 4 ulp of the f32 output"""
    shape3 = (1,) + x.shape if x.ndim == 2 else x.shape
    b_eval, _ = evaluate_bound(lat3(lattice), shape3)
    bf = b_eval + b_lattice
    want = x.astype(np.float64) / np.exp(ref.evaluate(lat3(lattice), shape3).reshape(x.shape))
    tol = np.abs(want) * np.expm1(bf) + 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    excess = np.abs(got - want) / tol
    record_property(key + "_field_bound", bf)
    record_property(key + "_gpu_over_tolerance", float(excess.max()))
    print(f"{key}: field bound {bf:.3e}, MI355X max |dev| / tolerance {excess.max():.3f}")
    assert excess.max() <= 1.0
