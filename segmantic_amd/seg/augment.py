"""Random draws of the training augmentation (reference ``src/segmantic/seg/monai_unet.py:178-217``).

The arithmetic runs in ``csrc/augment.hip``; this module only draws the parameters the way
MONAI's transforms do and composes the spatial ones into one index map:

* ``augment_spatial``: ``RandRotated(prob=0.2, range_z=0.4)``, ``range_x``, ``range_y`` (one
  rotation each, about the volume centre, angle ~ U(-0.4, 0.4) rad), then
  ``RandZoomd(prob=0.2, min_zoom=0.8, max_zoom=1.3, keep_size=True)`` (one factor for all axes).
  The reference resamples the whole volume once per transform; here the four index maps are
  composed and applied inside the patch gather (one interpolation instead of up to four, no
  whole-volume passes; "area" zoom interpolation of the image is approximated by trilinear).
* ``augment_intensity``: ``RandAdjustContrastd(prob=0.2, gamma=(0.5, 4.5))``,
  ``RandHistogramShiftd(prob=0.2, num_control_points=10)``, ``RandBiasFieldd(prob=0.2)``,
  ``RandGibbsNoised(prob=0.2, alpha=(0, 1))``, ``RandKSpaceSpikeNoised(prob=0.2)`` per patch (the
  spike intensity's default range, 0.95..1.1 x 2.5 x mean log|K|, is evaluated on the device from a
  host-drawn U(0,1)).
* ``RandFlipd`` runs last in the reference, after the k-space transforms.  Here the flips happen
  in the crop gather and the intensity / k-space transforms then run with parameters mirrored by
  the flips (``flip_params``; the Gibbs mask is mirrored inside ``ops.kspace_augment``), which
  gives the same patch without a separate flip pass.

* ``augment_elastic`` (not in the reference; off by default): a smooth non-rigid deformation composed
  into the same gather (``segmi_elastic_warp_crop_patches``).  The field lives in
  the index space of the augmented volume, so every crop of one volume in one batch shares it, as
  they share the affine map.  ``n = (n0, n1, n2) >= 4`` control points along (d0, d1, d2) carry a
  displacement in voxels each; the displacement is the uniform cubic B-spline, tensor product over the
  axes: for an axis of extent ``dim > 1``, ``t = i (n_a - 3) / (dim - 1)``, ``k = min(floor(t),
  n_a - 4)``, ``f = t - k``, and the four uniform cubic B-spline basis functions of ``f`` weigh control
  points ``k .. k+3``; the volume spans the ``n_a - 3`` interior spans and ``h_a = (dim - 1) / (n_a - 3)``
  is the control spacing in voxels.  An axis of extent 1 uses ``t = 0`` and its displacement component
  is 0.  A patch voxel's integer augmented index ``a`` becomes ``a' = a + u(a)`` and the source index
  is ``M a'`` (``M`` = the affine pull-back, or the identity); clamping, trilinear image, nearest label
  and the SpatialPad region (decided on the integer ``a``) are those of the affine gather.  The
  control displacements of component ``a`` are U(-A_a, A_a), ``A_a = max_displacement`` (default
  ``0.12 h_a``).  The derivative of a cubic B-spline is a convex combination of neighbouring control
  differences, so ``|du_a/di_b| <= 2 A_a / h_b``; ``L = max_a sum_b 2 A_a / h_b < 1`` is required (the
  default gives 0.72): then ``I + grad u`` is invertible and ``forward_point_elastic`` contracts at rate L.
  At most 4096 control points (three f32 planes in LDS).

* ``augment_degrade`` (not in the reference; off by default): additive Gaussian noise, Gaussian blur, a
  brightness multiplier and simulated low resolution, in that order, on the f32 patches as the gather
  wrote them (flipped already), before the intensity transforms (``segmi_degrade_augment``, DESIGN.md
  section 20).  One draw per patch is shared by its channels; the label is never touched.  Noise:
  ``x[e] += sqrt(variance) g(seed, e)`` with ``g`` a counter-hash Box-Muller normal of the element index.
  Blur: separable Gaussian, ``sigma`` in voxels, radius ``floor(4 sigma + 0.5) <= 8``, scipy's ``reflect``
  border.  Brightness: ``x *= multiplier``.  Lowres: nearest down onto ``m = max(1, floor(n zoom + 0.5))``
  samples per axis, linear back up.  ``degrade_config`` validates the option, ``draw_degrade`` draws it.

Spatial axes: the cached volumes are [C, d0, d1, d2]; ``range_x`` rotates about d0, ``range_y``
about d1, ``range_z`` about d2, as MONAI names the axes of a channel-first array.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np


def _rot(axis: int, angle: float) -> np.ndarray:
    """4x4 rotation about spatial axis `axis` (0,1,2 = d0,d1,d2) of coordinates ordered (d0,d1,d2)."""
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(4)
    a, b = [(1, 2), (0, 2), (0, 1)][axis]
    m[a, a], m[a, b], m[b, a], m[b, b] = c, -s, s, c
    return m


def draw_spatial(rng: np.random.RandomState, shape) -> Optional[np.ndarray]:
    """4x4 map from an index of the augmented volume to the source index, both in (d0, d1, d2)
    order, or None when no spatial transform fired."""
    ctr = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    to_c, from_c = np.eye(4), np.eye(4)
    to_c[:3, 3], from_c[:3, 3] = -ctr, ctr
    m = np.eye(4)
    fired = False
    # reference order: rotate about z (d2), then x (d0), then y (d1), then zoom.  The augmented
    # image is Z(Ry(Rx(Rz(I)))), so an output index is pulled back through zoom, Ry, Rx, Rz.
    stages = []
    for axis in (2, 0, 1):
        if rng.rand() < 0.2:
            stages.append(_rot(axis, -float(rng.uniform(-0.4, 0.4))))   # pull-back = inverse rotation
            fired = True
        else:
            stages.append(None)
    zoom = None
    if rng.rand() < 0.2:
        zoom = float(rng.uniform(0.8, 1.3))
        fired = True
    if not fired:
        return None
    if zoom is not None:
        z = np.eye(4)
        z[0, 0] = z[1, 1] = z[2, 2] = 1.0 / zoom
        m = z @ m
    for st in reversed(stages):          # Ry, Rx, Rz pull-backs
        if st is not None:
            m = st @ m
    return from_c @ m @ to_c


def to_index_map_xyz(m_d012: np.ndarray) -> np.ndarray:
    """(d0,d1,d2)-ordered 4x4 -> the kernel's row-major 3x4 over (x=d2, y=d1, z=d0)."""
    p = np.zeros((4, 4))
    p[0, 2] = p[1, 1] = p[2, 0] = p[3, 3] = 1.0       # (x,y,z,1) -> (d0,d1,d2,1)
    mm = p.T @ m_d012 @ p                              # p is its own inverse (a swap)
    return mm[:3, :].copy()


def forward_point(m_d012: np.ndarray, pt) -> np.ndarray:
    """Source index -> index in the augmented volume (inverse of the pull-back map)."""
    inv = np.linalg.inv(m_d012)
    return (inv @ np.array([pt[0], pt[1], pt[2], 1.0]))[:3]


ELASTIC_MAX_CONTROL = 4096          # control points of one field: three f32 planes = 48 KB of LDS
_ELASTIC_KEYS = ("prob", "control_points", "max_displacement")


def _triple(v, what, kind):
    vals = list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * 3
    if len(vals) != 3:
        raise ValueError(f"augment_elastic: '{what}' must be one value or one per axis (d0, d1, d2), got {v!r}")
    out = []
    for x in vals:
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or (
                kind is int and float(x) != int(x)):
            raise ValueError(f"augment_elastic: '{what}' must be {'an integer' if kind is int else 'a number'}"
                             f" or three of them, got {v!r}")
        out.append(kind(x))
    return tuple(out)


def elastic_config(value) -> Optional[dict]:
    """The ``augment_elastic`` option in normal form: None when off (False / None), else
    ``{"prob": float, "control_points": (n0, n1, n2), "max_displacement": None | (a0, a1, a2)}``.
    ``True`` = ``prob 0.2``, ``control_points 7``, ``max_displacement`` 0.12 control spacings.  Unknown keys
    and out-of-range values raise ``ValueError``; what depends on a volume's extents (the no-fold
    condition) is checked by ``elastic_amplitudes``."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"augment_elastic must be False, True or a dictionary with keys {_ELASTIC_KEYS}, "
                         f"got {value!r}")
    unknown = [k for k in value if k not in _ELASTIC_KEYS]
    if unknown:
        raise ValueError(f"augment_elastic: unknown keys {unknown}; accepted: {list(_ELASTIC_KEYS)}")
    prob = value.get("prob", 0.2)
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0.0 <= float(prob) <= 1.0:
        raise ValueError(f"augment_elastic: 'prob' must be a probability in [0, 1], got {prob!r}")
    n = _triple(value.get("control_points", 7), "control_points", int)
    if min(n) < 4:
        raise ValueError(f"augment_elastic: 'control_points' needs at least 4 points per axis (one cubic span), "
                         f"got {n}")
    if n[0] * n[1] * n[2] > ELASTIC_MAX_CONTROL:
        raise ValueError(f"augment_elastic: 'control_points' {n} = {n[0] * n[1] * n[2]} points, more than the "
                         f"{ELASTIC_MAX_CONTROL} the kernel holds in LDS")
    amp = value.get("max_displacement")
    if amp is not None:
        amp = _triple(amp, "max_displacement", float)
        if not all(np.isfinite(a) and a >= 0.0 for a in amp):
            raise ValueError(f"augment_elastic: 'max_displacement' must be finite and >= 0 (voxels), got {amp}")
    return {"prob": float(prob), "control_points": n, "max_displacement": amp}


def elastic_amplitudes(shape, cfg: dict) -> Tuple[np.ndarray, float]:
    """(A, L): the displacement amplitude per component in voxels and the bound
    ``L = max_a sum_b 2 A_a / h_b`` of ``|grad u|`` for a volume of extents ``shape``.  Raises unless
    ``L < 1`` (the field could fold).  An axis of extent 1 carries no displacement and no derivative."""
    shape = [int(v) for v in shape]
    n = cfg["control_points"]
    live = np.array([d > 1 for d in shape])
    h = np.array([(d - 1) / (k - 3) if d > 1 else np.inf for d, k in zip(shape, n)], dtype=np.float64)
    if cfg["max_displacement"] is None:
        amp = np.where(live, 0.12 * np.where(live, h, 0.0), 0.0)
    else:
        amp = np.where(live, np.asarray(cfg["max_displacement"], dtype=np.float64), 0.0)
    lip = float(np.max(2.0 * amp * np.sum(1.0 / h)))
    if not lip < 1.0:
        raise ValueError(f"augment_elastic: 'max_displacement' {tuple(float(a) for a in amp)} voxels with control "
                         f"spacing {tuple(float(v) for v in h)} voxels (volume {tuple(shape)}, control_points "
                         f"{tuple(n)}) gives max_a sum_b 2 A_a / h_b = {lip:.3f} >= 1: the deformation could fold; "
                         f"lower 'max_displacement' or use fewer control points")
    return amp, lip


def draw_elastic(rng: np.random.RandomState, shape, cfg: dict) -> Optional[np.ndarray]:
    """Control displacements [3, n0, n1, n2] f32 (components and grid axes in (d0, d1, d2) order) of one
    volume's field, or None when it did not fire (then nothing but the one ``rand()`` is drawn)."""
    if not rng.rand() < cfg["prob"]:
        return None
    amp, _lip = elastic_amplitudes(shape, cfg)
    n = cfg["control_points"]
    return np.stack([rng.uniform(-a, a, size=n) for a in amp]).astype(np.float32)


def _bspline_basis(f: np.ndarray) -> np.ndarray:
    """the four uniform cubic B-spline basis functions of f, stacked on a new first axis"""
    return np.stack([(1.0 - f) ** 3, 3.0 * f ** 3 - 6.0 * f ** 2 + 4.0,
                     -3.0 * f ** 3 + 3.0 * f ** 2 + 3.0 * f + 1.0, f ** 3]) / 6.0


def elastic_displacement(ctrl: np.ndarray, shape, points) -> np.ndarray:
    """u at ``points`` [..., 3] (indices of the augmented volume in (d0, d1, d2) order, float64; a
    position outside the volume takes the displacement of the nearest position inside)."""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64)
    n = ctrl.shape[1:]
    ks, ws = [], []
    for a in range(3):
        dim = int(shape[a])
        t = np.clip(pts[..., a], 0.0, dim - 1.0) * (n[a] - 3) / (dim - 1) if dim > 1 else np.zeros(pts.shape[:-1])
        k = np.minimum(np.floor(t).astype(np.int64), n[a] - 4)
        ks.append(k)
        ws.append(_bspline_basis(t - k))
    u = np.zeros(pts.shape[:-1] + (3,))
    for i in range(4):
        for j in range(4):
            for l in range(4):
                w = ws[0][i] * ws[1][j] * ws[2][l]
                u += w[..., None] * np.moveaxis(ctrl[:, ks[0] + i, ks[1] + j, ks[2] + l], 0, -1)
    u[..., [int(shape[a]) <= 1 for a in range(3)]] = 0.0
    return u


def forward_point_elastic(m_d012: Optional[np.ndarray], ctrl: np.ndarray, shape, pt) -> np.ndarray:
    """Source index -> index in the augmented volume under the composed map ``s = M (p + u(p))``
    (``m_d012`` None = identity): the fixed point of ``p = M^-1 s - u(p)``, iterated in float64 from
    ``M^-1 s`` until the update is below 1e-9 voxel.  The no-fold condition makes it a contraction."""
    q = np.asarray(pt, dtype=np.float64)[:3] if m_d012 is None else forward_point(m_d012, pt)
    p = q.copy()
    for _ in range(1000):
        nxt = q - elastic_displacement(ctrl, shape, p)
        done = float(np.abs(nxt - p).max()) < 1e-9
        p = nxt
        if done:
            return p
    raise RuntimeError("augment_elastic: the crop centre's fixed-point iteration did not converge in 1000 steps "
                       "(the field's gradient bound is too close to 1)")


DEGRADE_MAX_SIGMA = 2.0             # blur radius floor(4 sigma + 0.5) <= 8, the halo the kernel stages
_DEGRADE_DEFAULTS = {
    "noise": {"prob": 0.1, "variance": (0.0, 0.1)},
    "blur": {"prob": 0.2, "sigma": (0.5, 1.0)},
    "brightness": {"prob": 0.15, "multiplier": (0.75, 1.25)},
    "lowres": {"prob": 0.25, "zoom": (0.5, 1.0)},
}


def _number(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))


def _degrade_entry(name: str, value) -> Optional[dict]:
    """one transform of ``augment_degrade`` in normal form: None (off) or ``{prob, <range field>: (lo, hi)}``"""
    defaults = _DEGRADE_DEFAULTS[name]
    field = next(k for k in defaults if k != "prob")
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"augment_degrade: '{name}' must be false, true or a dictionary with keys "
                         f"{list(defaults)}, got {value!r}")
    unknown = [k for k in value if k not in defaults]
    if unknown:
        raise ValueError(f"augment_degrade: '{name}': unknown keys {unknown}; accepted: {list(defaults)}")
    prob = value.get("prob", defaults["prob"])
    if not _number(prob) or not 0.0 <= float(prob) <= 1.0:
        raise ValueError(f"augment_degrade: '{name}.prob' must be a probability in [0, 1], got {prob!r}")
    rng = value.get(field, defaults[field])
    ok = isinstance(rng, (list, tuple, np.ndarray)) and len(rng) == 2 and all(_number(v) for v in rng)
    if not ok or not all(np.isfinite(float(v)) for v in rng) or float(rng[0]) > float(rng[1]):
        raise ValueError(f"augment_degrade: '{name}.{field}' must be two finite ascending numbers [low, high], "
                         f"got {rng!r}")
    lo, hi = float(rng[0]), float(rng[1])
    if name == "noise" and lo < 0.0:
        raise ValueError(f"augment_degrade: 'noise.variance' must be >= 0, got {rng!r}")
    if name == "blur" and (lo <= 0.0 or hi > DEGRADE_MAX_SIGMA):
        raise ValueError(f"augment_degrade: 'blur.sigma' must lie in (0, {DEGRADE_MAX_SIGMA}] voxels (the kernel "
                         f"stages a halo of floor(4 sigma + 0.5) <= 8 voxels), got {rng!r}")
    if name == "lowres" and (lo <= 0.0 or hi > 1.0):
        raise ValueError(f"augment_degrade: 'lowres.zoom' must lie in (0, 1], got {rng!r}")
    return {"prob": float(prob), field: (lo, hi)}


def degrade_config(value) -> Optional[dict]:
    """The ``augment_degrade`` option in normal form: None when off (False / None, or every transform off),
    else a dictionary with the four keys ``noise``, ``blur``, ``brightness``, ``lowres``, each None (that
    transform is off and draws nothing) or ``{"prob": float, <field>: (low, high)}`` with the field
    ``variance`` / ``sigma`` (voxels) / ``multiplier`` / ``zoom``.  ``True`` = all four with the defaults
    ``{0.1, [0, 0.1]}``, ``{0.2, [0.5, 1.0]}``, ``{0.15, [0.75, 1.25]}``, ``{0.25, [0.5, 1.0]}``.  In a dictionary a
    missing key means that transform's defaults, ``False`` switches it off, ``True`` means its defaults and a
    dictionary overrides single fields.  Unknown keys and out-of-range values raise ``ValueError`` by name."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"augment_degrade must be False, True or a dictionary with keys {list(_DEGRADE_DEFAULTS)}, "
                         f"got {value!r}")
    unknown = [k for k in value if k not in _DEGRADE_DEFAULTS]
    if unknown:
        raise ValueError(f"augment_degrade: unknown keys {unknown}; accepted: {list(_DEGRADE_DEFAULTS)}")
    cfg = {name: _degrade_entry(name, value.get(name, True)) for name in _DEGRADE_DEFAULTS}
    return cfg if any(v is not None for v in cfg.values()) else None


def lowres_extents(roi, zoom) -> np.ndarray:
    """coarse extents int32[n, 3] for patch extents ``roi`` and zooms [n]: ``max(1, floor(extent zoom + 0.5))``,
    1 for an axis of extent 1"""
    z = np.asarray(zoom, dtype=np.float64).reshape(-1, 1)
    ext = np.asarray([int(r) for r in roi], dtype=np.float64).reshape(1, 3)
    m = np.maximum(1.0, np.floor(ext * z + 0.5))
    return np.where(ext > 1, np.minimum(m, ext), 1.0).astype(np.int32)


def draw_degrade(rng: np.random.RandomState, n: int, roi, cfg: dict) -> dict:
    """Per-patch draws of ``augment_degrade`` for ``ops.degrade_augment``, vectorised over the ``n`` patches, per
    enabled transform and in this order: ``noise`` = (on, variance, seed uint32), ``blur`` = (on, sigma),
    ``brightness`` = (on, multiplier), ``lowres`` = (on, zoom, m int32[n, 3]); a transform that is off is None
    and draws nothing.  Each transform draws ``rand(n) < prob``, then ``uniform(range, n)`` (kept as f32, the
    value the device is given); noise also ``randint(0, 2**32, n)``."""
    out = {"noise": None, "blur": None, "brightness": None, "lowres": None}
    c = cfg["noise"]
    if c is not None:
        on = (rng.rand(n) < c["prob"]).astype(np.uint8)
        var = rng.uniform(c["variance"][0], c["variance"][1], n).astype(np.float32)
        out["noise"] = (on, var, rng.randint(0, 2 ** 32, n, dtype=np.uint32))
    c = cfg["blur"]
    if c is not None:
        on = (rng.rand(n) < c["prob"]).astype(np.uint8)
        out["blur"] = (on, rng.uniform(c["sigma"][0], c["sigma"][1], n).astype(np.float32))
    c = cfg["brightness"]
    if c is not None:
        on = (rng.rand(n) < c["prob"]).astype(np.uint8)
        out["brightness"] = (on, rng.uniform(c["multiplier"][0], c["multiplier"][1], n).astype(np.float32))
    c = cfg["lowres"]
    if c is not None:
        on = (rng.rand(n) < c["prob"]).astype(np.uint8)
        zoom = rng.uniform(c["zoom"][0], c["zoom"][1], n).astype(np.float32)
        out["lowres"] = (on, zoom, lowres_extents(roi, zoom))
    return out


def draw_intensity(rng: np.random.RandomState, n: int, roi=None):
    """Per-patch draws: (contrast, hist, bias) for ``ops.intensity_augment`` and, when ``roi`` is
    given, (gibbs, spike) for ``ops.kspace_augment``."""
    con = (rng.rand(n) < 0.2).astype(np.uint8)
    gam = rng.uniform(0.5, 4.5, n).astype(np.float32)
    hon = (rng.rand(n) < 0.2).astype(np.uint8)
    ctrl = np.tile(np.linspace(0.0, 1.0, 10), (n, 1))
    for i in range(n):
        for k in range(1, 9):                         # RandHistogramShift.randomize
            ctrl[i, k] = rng.uniform(ctrl[i, k - 1], ctrl[i, k + 1])
    bon = (rng.rand(n) < 0.2).astype(np.uint8)
    coef = rng.uniform(0.0, 0.1, (n, 20)).astype(np.float32)
    out = ((con, gam), (hon, ctrl.astype(np.float32)), (bon, coef))
    if roi is None:
        return out
    gon = (rng.rand(n) < 0.2).astype(np.uint8)
    alpha = rng.uniform(0.0, 1.0, n).astype(np.float32)
    son = (rng.rand(n) < 0.2).astype(np.uint8)
    loc = np.stack([rng.randint(0, int(r), n) for r in roi], 1).astype(np.int32)
    u = rng.rand(n).astype(np.float32)
    return out + ((gon, alpha), (son, loc, u))


def mirror_index(i, n: int):
    """Index of the k-space bin that a flip of an n-long axis moves bin ``i`` of the CENTRED
    spectrum (``fftshift(fftn(ifftshift(x)))``) to: frequency k goes to -k, i.e. ``(n - i) mod n``
    for even n and ``n - 1 - i`` for odd n."""
    return (n - np.asarray(i)) % n if n % 2 == 0 else n - 1 - np.asarray(i)


def flip_params(intensity, flips, roi):
    """The draws of ``draw_intensity`` (made for the unflipped patch) rewritten for a patch whose
    axes were already flipped by ``flips`` (bit 0 = d0, bit 1 = d1, bit 2 = d2).

    The reference flips last (``RandFlipd`` after the k-space transforms); the crop kernels flip
    during the gather, before the intensity transforms run.  With these parameters the result is
    the same: flip(T(x, p)) == T(flip(x), p').  Contrast and histogram shift do not depend on
    position.  The bias field's Legendre term of degree i in an axis is odd in that axis when i is
    odd: those coefficients are negated (axes of one voxel excepted).  The spike moves to the
    mirrored bin (``mirror_index``).  The Gibbs mask is centred at (n - 1) / 2, which is not symmetric under the mirror for even n:
    ``ops.kspace_augment`` takes the flips and evaluates the mask at the mirrored bin itself."""
    con, hist, (bon, coef), *ks = intensity
    flips = np.asarray(flips, dtype=np.int64)
    if not flips.any():
        return intensity
    coef = np.array(coef, dtype=np.float32, copy=True)
    k = 0
    for a in range(4):                                  # leggrid3d order, as bias_field_kernel reads it
        for b in range(4 - a):
            for c in range(4 - a - b):
                for d, deg in enumerate((a, b, c)):
                    # linspace(-1, 1, 1) == [-1] is no symmetric grid; a flip of 1 voxel is no flip
                    if deg % 2 == 1 and int(roi[d]) > 1:
                        coef[:, k] = np.where((flips & (1 << d)) != 0, -coef[:, k], coef[:, k])
                k += 1
    out = (con, hist, (bon, coef))
    if not ks:
        return out
    gibbs, (son, loc, u) = ks
    loc = np.array(loc, dtype=np.int32, copy=True)
    for d in range(3):
        fl = (flips & (1 << d)) != 0
        loc[:, d] = np.where(fl, mirror_index(loc[:, d], int(roi[d])), loc[:, d])
    return out + (gibbs, (son, loc, u))
