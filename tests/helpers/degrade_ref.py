"""Float64 numpy restatement of the ``augment_degrade`` training augmentation, written from
its definition, and the gate the GPU test holds the kernels to.

Patches are [C, d0, d1, d2] float64 arrays, as in ``augment_ref``; the kernels see them as dense NDHWC, so the
element index of voxel (z, y, x), channel ch is ``e = ((z*rh + y)*rw + x)*c + ch``.

* noise: ``x[e] += sqrt(variance) g(seed, e)``; ``g`` is Box-Muller over the counter hash of ``k = 2e + j``
  (``j`` = 0, 1; uint32 arithmetic): ``h = k*0x9E3779B1 ^ seed; h ^= h>>16; h *= 0x7feb352d; h ^= h>>15;
  h *= 0x846ca68b; h ^= h>>16``; ``u1 = ((h_0>>8) + 1) 2^-24``, ``u2 = (h_1>>8) 2^-24``,
  ``g = sqrt(-2 ln u1) cos(2 pi u2)``.
* blur: separable over the spatial axes of extent > 1, ``R = floor(4 sigma + 0.5)``,
  ``w_k = exp(-k^2 / (2 sigma^2))`` normalised to sum 1, border ``reflect``: index ``i`` -> ``m = i mod 2n``,
  ``m < n ? m : 2n - 1 - m``.
* brightness: ``x *= multiplier``.
* lowres: per axis of extent ``n`` and coarse extent ``m``: coarse sample ``j`` is the fine voxel
  ``src(j) = floor((2j + 1) n / (2m))``; fine voxel ``i`` has ``t = clamp((i + 0.5) m/n - 0.5, 0, m - 1)``,
  ``j0 = min(floor(t), max(m - 2, 0))``, ``f = t - j0`` and the value ``(1 - f) v[src(j0)] + f v[src(min(j0 + 1,
  m - 1))]``; an axis with ``m == n`` passes through.

``fault=`` seeds one fault (tests/test_degrade_host.py shows that the gate rejects each): ``"zero_pad"`` pads the
blur with zeros instead of reflecting, ``"radius_3sigma"`` truncates it at ``ceil(3 sigma)``, ``"swap_uniforms"``
takes ``u1`` from ``j = 1`` and ``u2`` from ``j = 0``, ``"rounding_src"`` rounds ``src`` to nearest instead of
taking the floor, ``"brightness_before_blur"`` multiplies the input by the brightness before the blur and leaves
the noise unscaled.
"""
from __future__ import annotations

import numpy as np

from tests.helpers import augment_ref as ar
from tests.helpers import elastic_ref as er

INT_RTOL = 2e-5      # the bound of tests/test_augment_gpu.py's f32 elementwise chain, relative to max(1, max |ref|)
FAULTS = ("zero_pad", "radius_3sigma", "swap_uniforms", "rounding_src", "brightness_before_blur")
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ noise
def hash32(k, seed):
    """the counter hash on uint32 values held in uint64 arrays"""
    k = np.asarray(k, dtype=np.uint64) & M32
    h = ((k * np.uint64(0x9E3779B1)) & M32) ^ (np.uint64(int(seed)) & M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & M32
    h ^= h >> np.uint64(16)
    return h


def gauss(seed, count: int, fault=None) -> np.ndarray:
    """g(seed, e) for e = 0 .. count - 1, float64"""
    e = np.arange(count, dtype=np.uint64)
    h0, h1 = hash32(2 * e, seed), hash32(2 * e + 1, seed)
    if fault == "swap_uniforms":
        h0, h1 = h1, h0
    u1 = ((h0 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (h1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise_field(seed, shape_cdhw, fault=None) -> np.ndarray:
    """the standard-normal field of one patch, as [C, d0, d1, d2] (the element index runs over NDHWC)"""
    c, rd, rh, rw = shape_cdhw
    return gauss(seed, c * rd * rh * rw, fault).reshape(rd, rh, rw, c).transpose(3, 0, 1, 2)


# ------------------------------------------------------------------------------------------- blur
def reflect(i, n: int):
    m = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def blur_weights(sigma: float, fault=None):
    sigma = float(sigma)
    radius = int(np.ceil(3.0 * sigma)) if fault == "radius_3sigma" else int(np.floor(4.0 * sigma + 0.5))
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * sigma * sigma))
    return radius, w / w.sum()


def blur(x: np.ndarray, sigma: float, fault=None) -> np.ndarray:
    """[C, d0, d1, d2] -> the same shape"""
    radius, w = blur_weights(sigma, fault)
    x = np.asarray(x, dtype=np.float64)
    for axis in (1, 2, 3):
        n = x.shape[axis]
        if n == 1:
            continue
        out = np.zeros_like(x)
        for k in range(-radius, radius + 1):
            idx = np.arange(n) + k
            if fault == "zero_pad":
                ok = (idx >= 0) & (idx < n)
                shape = [1, 1, 1, 1]
                shape[axis] = n
                out += w[k + radius] * np.take(x, np.clip(idx, 0, n - 1), axis=axis) * ok.reshape(shape)
            else:
                out += w[k + radius] * np.take(x, reflect(idx, n), axis=axis)
        x = out
    return x


# ----------------------------------------------------------------------------------------- lowres
def lowres_src(n: int, m: int, fault=None) -> np.ndarray:
    j = np.arange(m, dtype=np.int64)
    if fault == "rounding_src":
        return np.clip(np.rint((j + 0.5) * n / m).astype(np.int64), 0, n - 1)
    return ((2 * j + 1) * n) // (2 * m)


def lowres_axis(n: int, m: int, fault=None):
    """(source voxel of the lower tap, of the upper tap, fraction) for fine voxels 0 .. n - 1"""
    src = lowres_src(n, m, fault)
    t = np.clip((np.arange(n) + 0.5) * m / n - 0.5, 0.0, m - 1.0)
    j0 = np.minimum(np.floor(t).astype(np.int64), max(m - 2, 0))
    return src[j0], src[np.minimum(j0 + 1, m - 1)], t - j0


def lowres(x: np.ndarray, m3, fault=None) -> np.ndarray:
    """[C, d0, d1, d2] and the coarse extents (m0, m1, m2) -> the same shape (the tensor product, axis by axis)"""
    x = np.asarray(x, dtype=np.float64)
    for a in range(3):
        n, m = x.shape[a + 1], int(m3[a])
        if m == n:
            continue
        s0, s1, f = lowres_axis(n, m, fault)
        shape = [1, 1, 1, 1]
        shape[a + 1] = n
        f = f.reshape(shape)
        x = (1.0 - f) * np.take(x, s0, axis=a + 1) + f * np.take(x, s1, axis=a + 1)
    return x


# ------------------------------------------------------------------------------------------ chain
def degrade_chain(x: np.ndarray, draws, i: int, fault=None) -> np.ndarray:
    """noise, blur, brightness, lowres of ``augment.draw_degrade``'s draws for patch ``i`` ([C, d0, d1, d2], as
    the gather wrote it)"""
    x = np.asarray(x, dtype=np.float64)
    noise, blr, bright, low = (draws.get(k) for k in ("noise", "blur", "brightness", "lowres"))
    n_on = noise is not None and bool(noise[0][i])
    b_on = blr is not None and bool(blr[0][i])
    r_on = bright is not None and bool(bright[0][i])
    l_on = low is not None and bool(low[0][i])
    early = fault == "brightness_before_blur" and r_on and b_on
    if early:
        x = x * float(bright[1][i])
    if n_on:
        x = x + np.sqrt(float(noise[1][i])) * noise_field(int(noise[2][i]), x.shape, fault)
    if b_on:
        x = blur(x, float(blr[1][i]), fault)
    if r_on and not early:
        x = x * float(bright[1][i])
    if l_on:
        x = lowres(x, low[-1][i], fault)
    return x


def reference_chain(image, label, record, roi):
    """One volume's patches from a record of ``trainer.draw_batch``: ``augment_ref``'s (elastic +) (warp +) crop,
    the flip (the gather flips), this chain on the flipped patch, and ``augment_ref.intensity_chain`` in the
    unflipped frame its draws are made for.  Returns images [n, C, *roi] and labels [n, *roi]."""
    imgs, labs = [], []
    for i, (st, fl) in enumerate(zip(record["starts"], record["flips"])):
        if record.get("elastic") is not None:
            x, lab, _src = er.elastic_warp_crop(image, label, record["elastic"], record["spatial"], st, roi)
        elif record["spatial"] is not None:
            x, lab, _src = ar.warp_crop(image, label, record["spatial"], st, roi)
        else:
            x, lab = ar.crop(image, label, st, roi)
        if record.get("degrade") is not None:
            x = ar.flip(degrade_chain(ar.flip(x, fl), record["degrade"], i), fl)
        if record["intensity"] is not None:
            x = ar.intensity_chain(x, record["intensity"], i)
        imgs.append(ar.flip(x, fl))
        labs.append(ar.flip(lab, fl))
    return np.stack(imgs), np.stack(labs)


# ------------------------------------------------------------------------------------------- gate
def gate(got, ref):
    """(error, bound): ``max |got - ref|`` and ``INT_RTOL max(1, max |ref|)``.  The f32 kernels round each of at
    most 33 operations per element at R = 8 (17 products and sums per blurred axis are the longest run; the
    noise's log, sqrt and cos are within 2 ulp each), about 33 * 2^-24 = 2e-6 of the largest magnitude."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max()), INT_RTOL * max(1.0, float(np.abs(ref).max()))


# ------------------------------------------------------------------------- the tests' shared inputs
BLUR_CASES = [((7, 9, 11), 0.5), ((3, 5, 33), 1.0), ((1, 17, 19), 0.8), ((2, 3, 4), 2.0), ((5, 6, 7), 1.37)]
NOISE_SEEDS = (0, 1, 2, 7, 99, 12345, 0xDEADBEEF, 0xFFFFFFFF)


def patches(n, shape, c, seed):
    """[n, C, d0, d1, d2] f32-representable float64 patches with distinct channels"""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, c, *shape) * (1.0 + np.arange(c).reshape(1, c, 1, 1, 1)) + np.arange(c).reshape(1, c, 1, 1, 1)
    return x.astype(np.float32).astype(np.float64)


def draws(n, shape, seed, which="nbrl", sigma=(0.5, 2.0)):
    """draws in ``augment.draw_degrade``'s form with every transform of ``which`` (n = noise, b = blur,
    r = brightness, l = lowres) on for every patch"""
    rng = np.random.RandomState(seed)
    on, off = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    zoom = rng.uniform(0.3, 0.9, n).astype(np.float32)
    ext = np.asarray(shape, dtype=np.float64)[None]
    m = np.where(ext > 1, np.maximum(1.0, np.floor(ext * zoom[:, None].astype(np.float64) + 0.5)), 1.0).astype(np.int32)
    return {"noise": (on if "n" in which else off, rng.uniform(0.0, 0.1, n).astype(np.float32),
                      rng.randint(0, 2 ** 32, n, dtype=np.uint32)),
            "blur": (on if "b" in which else off, rng.uniform(sigma[0], sigma[1], n).astype(np.float32)),
            "brightness": (on if "r" in which else off, rng.uniform(0.75, 1.25, n).astype(np.float32)),
            "lowres": (on if "l" in which else off, zoom, m)}
