"""Float64 numpy references of the training augmentation (seg/augment.py, csrc/augment.hip), written from MONAI's documented semantics of the transforms the
reference pipeline composes: SpatialPad + RandCropByLabelClasses + RandFlip, the rotate / zoom
index map (the project's one-resample form), AdjustContrast, HistogramShift, BiasField, GibbsNoise
and KSpaceSpikeNoise.

Patches are [C, d0, d1, d2] float64 arrays; flips are bit 0 = d0, bit 1 = d1, bit 2 = d2.
``reference_chain`` applies them in the reference's order, the flip last.
"""
from __future__ import annotations

import numpy as np
from numpy.polynomial.legendre import leggrid3d

AX = (-3, -2, -1)


def flip(x: np.ndarray, code: int) -> np.ndarray:
    """RandFlip along the spatial axes selected by ``code`` (the last three axes of ``x``)."""
    axes = tuple(AX[d] for d in range(3) if code & (1 << d))
    return np.flip(x, axes) if axes else x


def crop(image: np.ndarray, label, start, roi):
    """SpatialPad + crop: ``roi`` voxels from ``start`` (may lie outside the volume: zeros there).
    image [C, D, H, W], label [D, H, W] or None."""
    shp = image.shape[1:]
    idx = [np.arange(roi[d]) + int(start[d]) for d in range(3)]
    ok = [(i >= 0) & (i < shp[d]) for d, i in enumerate(idx)]
    cl = [np.clip(i, 0, shp[d] - 1) for d, i in enumerate(idx)]
    inside = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
    img = np.where(inside, image[:, cl[0][:, None, None], cl[1][None, :, None], cl[2][None, None, :]], 0.0)
    lab = None
    if label is not None:
        lab = np.where(inside, label[cl[0][:, None, None], cl[1][None, :, None], cl[2][None, None, :]], 0.0)
    return img.astype(np.float64), lab


def warp_coords(m_d012: np.ndarray, start, roi):
    """Continuous source index (d0, d1, d2) of every patch voxel, float64, and the mask of the
    voxels inside the augmented volume's extent (the rest is SpatialPad)."""
    zz, yy, xx = np.meshgrid(*[np.arange(roi[d]) + int(start[d]) for d in range(3)], indexing="ij")
    a = np.stack([zz, yy, xx]).astype(np.float64)
    src = np.einsum("ij,j...->i...", m_d012[:3, :3], a) + m_d012[:3, 3][:, None, None, None]
    return src, a


def warp_crop(image: np.ndarray, label, m_d012: np.ndarray, start, roi):
    """Index-map warp + crop: trilinear image sampling with the position clamped into the volume
    (padding_mode="border"), nearest label (round half up, as the kernel's (int)(c + 0.5)); zeros
    outside the augmented volume.  Returns (image, label, src coordinates)."""
    shp = image.shape[1:]
    src, a = warp_coords(m_d012, start, roi)
    inside = np.ones(a.shape[1:], bool)
    for d in range(3):
        inside &= (a[d] >= 0) & (a[d] < shp[d])
    c = [np.clip(src[d], 0, shp[d] - 1) for d in range(3)]
    i0 = [np.floor(c[d]).astype(np.int64) for d in range(3)]
    i1 = [np.minimum(i0[d] + 1, shp[d] - 1) for d in range(3)]
    f = [c[d] - i0[d] for d in range(3)]
    out = np.zeros((image.shape[0],) + tuple(roi))
    for bz in (0, 1):
        for by in (0, 1):
            for bx in (0, 1):
                w = ((f[0] if bz else 1 - f[0]) * (f[1] if by else 1 - f[1]) * (f[2] if bx else 1 - f[2]))
                iz, iy, ix = (i1[0] if bz else i0[0]), (i1[1] if by else i0[1]), (i1[2] if bx else i0[2])
                out += w[None] * image[:, iz, iy, ix]
    out = np.where(inside[None], out, 0.0)
    lab = None
    if label is not None:
        n = [np.minimum(np.floor(c[d] + 0.5).astype(np.int64), shp[d] - 1) for d in range(3)]
        lab = np.where(inside, label[n[0], n[1], n[2]], 0.0).astype(np.float64)
    return out, lab, src


def near_half(src: np.ndarray, shape, eps: float) -> np.ndarray:
    """Voxels whose clamped float64 coordinate lies within ``eps`` of a .5 boundary on some axis:
    the only places a nearest-neighbour pick may differ from one made in f32."""
    m = np.zeros(src.shape[1:], bool)
    for d in range(3):
        c = np.clip(src[d], 0, shape[d] - 1)
        m |= np.abs(c - np.floor(c) - 0.5) < eps
    return m


def adjust_contrast(x: np.ndarray, gamma: float) -> np.ndarray:
    """AdjustContrast: ((x - min) / (range + 1e-7)) ** gamma * range + min, min / max of the whole patch."""
    mn = x.min()
    rng = x.max() - mn
    return ((x - mn) / (rng + 1e-7)) ** float(gamma) * rng + mn


def histogram_shift(x: np.ndarray, ctrl) -> np.ndarray:
    """HistogramShift: np.interp from linspace(min, max, n) onto ctrl scaled to [min, max]."""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    mn, mx = x.min(), x.max()
    if not mx > mn:
        return x.copy()
    xp = np.linspace(0.0, 1.0, len(ctrl)) * (mx - mn) + mn
    return np.interp(x, xp, ctrl * (mx - mn) + mn)


def bias_coef_grid(coef20) -> np.ndarray:
    """the 20 coefficients -> the 4x4x4 leggrid3d array (i + j + k <= 3, in MONAI's fill order)"""
    cm = np.zeros((4, 4, 4))
    k = 0
    for a in range(4):
        for b in range(4 - a):
            for c in range(4 - a - b):
                cm[a, b, c] = float(coef20[k])
                k += 1
    return cm


def bias_field(x: np.ndarray, coef20) -> np.ndarray:
    """BiasField (degree 3): x * exp(leggrid3d(linspace(-1, 1, n) per axis)); same field for every channel."""
    coords = [np.linspace(-1.0, 1.0, n) for n in x.shape[1:]]
    return x * np.exp(leggrid3d(coords[0], coords[1], coords[2], bias_coef_grid(coef20)))[None]


def _shifted_fft(v):
    return np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(v, axes=AX), axes=AX), axes=AX)


def _shifted_ifft(k):
    return np.fft.fftshift(np.fft.ifftn(np.fft.ifftshift(k, axes=AX), axes=AX), axes=AX).real


def mirror(i, n: int):
    """centred-spectrum bin of frequency -k when bin i holds frequency k"""
    return (n - np.asarray(i)) % n if n % 2 == 0 else n - 1 - np.asarray(i)


def gibbs_radius(alpha: float, shape) -> float:
    return (1.0 - float(alpha)) * max(shape) * np.sqrt(2.0) / 2.0


def gibbs(x: np.ndarray, alpha: float, flip_code: int = 0) -> np.ndarray:
    """GibbsNoise: the centred spectrum outside radius (1 - alpha) * max(shape) * sqrt(2) / 2 of
    (n - 1) / 2 is zeroed, channel by channel.  ``flip_code``: the mask is evaluated at the
    mirrored bin of the flagged axes (a patch flipped before the transform)."""
    shp = x.shape[1:]
    r = gibbs_radius(alpha, shp)
    idx = []
    for d in range(3):
        i = np.arange(shp[d])
        if flip_code & (1 << d):
            i = mirror(i, shp[d])
        idx.append(i - (shp[d] - 1) / 2.0)
    dist = np.sqrt(idx[0][:, None, None] ** 2 + idx[1][None, :, None] ** 2 + idx[2][None, None, :] ** 2)
    return np.stack([_shifted_ifft(_shifted_fft(v) * (dist <= r)) for v in x])


def spike_intensity(k: np.ndarray, u: float) -> float:
    return float(np.log(np.abs(k) + 1e-10).mean() * 2.5 * (0.95 + 0.15 * float(u)))


def spike(x: np.ndarray, loc, u: float) -> np.ndarray:
    """KSpaceSpikeNoise on log|K| of the centred spectrum, channel by channel: bin ``loc`` gets
    log-magnitude mean(log(|K| + 1e-10)) * 2.5 * (0.95 + 0.15 u), every phase is kept."""
    out = []
    for v in x:
        k = _shifted_fft(v)
        log_abs = np.log(np.abs(k) + 1e-10)
        phase = np.angle(k)
        log_abs[tuple(int(t) for t in loc)] = spike_intensity(k, u)
        out.append(_shifted_ifft(np.exp(log_abs) * np.exp(1j * phase)))
    return np.stack(out)


def gibbs_unshifted(x: np.ndarray, alpha: float, flip_code: int = 0) -> np.ndarray:
    """``gibbs`` as the kernel evaluates it: on plain fftn(x), plain bin j <-> centred bin
    (j + n // 2) mod n."""
    shp = x.shape[1:]
    r = gibbs_radius(alpha, shp)
    idx = []
    for d in range(3):
        i = (np.arange(shp[d]) + shp[d] // 2) % shp[d]
        if flip_code & (1 << d):
            i = mirror(i, shp[d])
        idx.append(i - (shp[d] - 1) / 2.0)
    dist = np.sqrt(idx[0][:, None, None] ** 2 + idx[1][None, :, None] ** 2 + idx[2][None, None, :] ** 2)
    return np.stack([np.fft.ifftn(np.fft.fftn(v) * (dist <= r)).real for v in x])


def spike_unshifted(x: np.ndarray, loc, u: float) -> np.ndarray:
    """``spike`` as the kernel evaluates it: on plain fftn(x) at plain bin (loc - n // 2) mod n,
    the magnitude replaced and the phase kept."""
    shp = x.shape[1:]
    j = tuple((int(loc[d]) - shp[d] // 2) % shp[d] for d in range(3))
    out = []
    for v in x:
        k = np.fft.fftn(v)
        a = np.exp(spike_intensity(k, u))
        k[j] = a * k[j] / abs(k[j]) if abs(k[j]) > 0 else a
        out.append(np.fft.ifftn(k).real)
    return np.stack(out)


def intensity_chain(x: np.ndarray, draws, i: int, flip_code: int = 0) -> np.ndarray:
    """The five transforms of ``augment.draw_intensity``'s draws for patch ``i`` in the reference's
    order (contrast, histogram shift, bias field, Gibbs, spike).  ``flip_code`` only moves the
    Gibbs mask (the other parameters are taken as given)."""
    (con, gam), (hon, ctrl), (bon, coef), *ks = draws
    if con[i]:
        x = adjust_contrast(x, gam[i])
    if hon[i]:
        x = histogram_shift(x, ctrl[i])
    if bon[i]:
        x = bias_field(x, coef[i])
    if ks:
        (gon, alpha), (son, loc, u) = ks
        if gon[i]:
            x = gibbs(x, alpha[i], flip_code)
        if son[i]:
            x = spike(x, loc[i], u[i])
    return x


def reference_chain(image: np.ndarray, label: np.ndarray, record, roi):
    """One volume's patches as the reference pipeline makes them from ``trainer.draw_batch``'s
    record: (warp +) SpatialPad + crop -> contrast -> histogram shift -> bias field -> Gibbs ->
    spike -> flip.  image [C, D, H, W] f64, label [D, H, W].  Returns images [n, C, *roi], labels
    [n, *roi] and, for a warped record, the float64 source coordinates [n, 3, *roi] (else None)."""
    imgs, labs, srcs = [], [], []
    for i, (st, fl) in enumerate(zip(record["starts"], record["flips"])):
        if record["spatial"] is None:
            x, lab = crop(image, label, st, roi)
            srcs.append(None)
        else:
            x, lab, src = warp_crop(image, label, record["spatial"], st, roi)
            srcs.append(flip(src, fl))
        if record["intensity"] is not None:
            x = intensity_chain(x, record["intensity"], i)
        imgs.append(flip(x, fl))
        labs.append(flip(lab, fl))
    return np.stack(imgs), np.stack(labs), (None if srcs[0] is None else np.stack(srcs))
