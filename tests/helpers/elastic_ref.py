"""Float64 numpy restatement of the elastic deformation of the training sampler,
written from its definition, and the gates the GPU test holds the kernel to.

Definition.  The field lives in the index space of the augmented volume.  ``ctrl`` is [3, n0, n1, n2]:
a displacement in voxels per control point, components and grid axes in (d0, d1, d2) order.  For an axis
of extent ``dim > 1``: ``t = i (n - 3) / (dim - 1)``, ``k = min(floor(t), n - 4)``, ``f = t - k``, and
control points ``k .. k+3`` are weighted by the uniform cubic B-spline at ``f``; the displacement is the
tensor product over the axes.  An axis of extent 1 uses ``t = 0`` and its component is 0.  A patch voxel
with integer augmented index ``a`` samples the source at ``M (a + u(a))``; clamping, trilinear image,
nearest label and the SpatialPad zeros (decided on ``a``) are those of ``augment_ref.warp_crop``.

The weights are written here through the cardinal cubic B-spline ``beta3`` (a function of the distance to
the control point), not through the four polynomials in ``f`` the kernel and ``seg/augment.py`` use.

``fault=`` injects one seeded fault into the evaluation (tests/test_elastic_host.py shows that the gates
reject each of them): ``"swap_axes"`` reads the control grid with its last two axes swapped,
``"reverse_weights"`` reverses the four weights, ``"after_affine"`` adds the displacement after the affine
map, ``"permute_components"`` rotates the displacement components, ``"wrong_t"`` scales ``t`` by
``n / dim`` instead of ``(n - 3) / (dim - 1)``.
"""
from __future__ import annotations

import numpy as np

from tests.helpers import augment_ref as ar

EPS32 = 2.0 ** -24
FAULTS = ("swap_axes", "reverse_weights", "after_affine", "permute_components", "wrong_t")


def beta3(x):
    """cardinal cubic B-spline: 2/3 - x^2 + |x|^3 / 2 on |x| < 1, (2 - |x|)^3 / 6 on 1 <= |x| < 2, else 0"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x < 1.0, 2.0 / 3.0 - x ** 2 + x ** 3 / 2.0, np.where(x < 2.0, (2.0 - x) ** 3 / 6.0, 0.0))


def _axis(points_a, dim, n, fault):
    """span index k [...] and the four weights [4, ...] of one axis"""
    pts = np.asarray(points_a, dtype=np.float64)
    if dim > 1:
        t = pts * n / dim if fault == "wrong_t" else pts * (n - 3) / (dim - 1)
    else:
        t = np.zeros_like(pts)
    k = np.clip(np.floor(t).astype(np.int64), 0, n - 4)
    f = t - k
    # control point k + j sits at spline coordinate j - 1 of the span [0, 1]
    w = np.stack([beta3(f - (j - 1)) for j in range(4)])
    if fault == "reverse_weights":
        w = w[::-1]
    return k, w


def displacement(ctrl, shape, points, fault=None):
    """u [..., 3] at ``points`` [..., 3] (augmented-volume indices, (d0, d1, d2) order)"""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    if fault == "swap_axes":
        ctrl = np.ascontiguousarray(ctrl.transpose(0, 1, 3, 2)).reshape(ctrl.shape)
    pts = np.asarray(points, dtype=np.float64)
    n = ctrl.shape[1:]
    kw = [_axis(pts[..., a], int(shape[a]), n[a], fault) for a in range(3)]
    u = np.zeros(pts.shape[:-1] + (3,))
    for i in range(4):
        for j in range(4):
            for l in range(4):
                w = kw[0][1][i] * kw[1][1][j] * kw[2][1][l]
                c = ctrl[:, kw[0][0] + i, kw[1][0] + j, kw[2][0] + l]        # [3, ...]
                u += w[..., None] * np.moveaxis(c, 0, -1)
    for a in range(3):
        if int(shape[a]) <= 1:
            u[..., a] = 0.0
    if fault == "permute_components":
        u = u[..., [1, 2, 0]]
    return u


def elastic_coords(ctrl, m_d012, shape, start, roi, fault=None):
    """float64 source coordinates [3, *roi] and the integer augmented indices [3, *roi]"""
    m = np.eye(4) if m_d012 is None else np.asarray(m_d012, dtype=np.float64)
    zz, yy, xx = np.meshgrid(*[np.arange(roi[d]) + int(start[d]) for d in range(3)], indexing="ij")
    a = np.stack([zz, yy, xx]).astype(np.float64)
    # the field is only defined (and only used) inside the volume: evaluate it at the clipped index
    inside_idx = np.stack([np.clip(a[d], 0, shape[d] - 1) for d in range(3)], -1)
    u = np.moveaxis(displacement(ctrl, shape, inside_idx, fault), -1, 0)
    lin = lambda p: np.einsum("ij,j...->i...", m[:3, :3], p) + m[:3, 3][:, None, None, None]  # noqa: E731
    if fault == "after_affine":
        return lin(a) + u, a
    return lin(a + u), a


def sample(image, label, src, a):
    """``augment_ref.warp_crop``'s sampling at given coordinates: clamp, trilinear, nearest label
    (round half up), zeros where the integer index ``a`` is outside the volume"""
    shp = image.shape[1:]
    inside = np.ones(a.shape[1:], bool)
    for d in range(3):
        inside &= (a[d] >= 0) & (a[d] < shp[d])
    c = [np.clip(src[d], 0, shp[d] - 1) for d in range(3)]
    i0 = [np.floor(c[d]).astype(np.int64) for d in range(3)]
    i1 = [np.minimum(i0[d] + 1, shp[d] - 1) for d in range(3)]
    f = [c[d] - i0[d] for d in range(3)]
    out = np.zeros((image.shape[0],) + tuple(a.shape[1:]))
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
    return out, lab


def elastic_warp_crop(image, label, ctrl, m, start, roi, fault=None):
    """(image [C, *roi], label [*roi] or None, source coordinates [3, *roi]) of one unflipped patch;
    ``m`` is the (d0, d1, d2)-ordered 4x4 pull-back map or None for the identity."""
    src, a = elastic_coords(ctrl, m, image.shape[1:], start, roi, fault)
    img, lab = sample(image, label, src, a)
    return img, lab, src


def reference_chain(image, label, record, roi):
    """``augment_ref.reference_chain`` for a record of ``trainer.draw_batch`` that may carry an ``elastic``
    field: (elastic +) warp + SpatialPad + crop -> intensity chain -> flip."""
    if record.get("elastic") is None:
        return ar.reference_chain(image, label, record, roi)
    imgs, labs, srcs = [], [], []
    for i, (st, fl) in enumerate(zip(record["starts"], record["flips"])):
        x, lab, src = elastic_warp_crop(image, label, record["elastic"], record["spatial"], st, roi)
        if record["intensity"] is not None:
            x = ar.intensity_chain(x, record["intensity"], i)
        imgs.append(ar.flip(x, fl))
        labs.append(ar.flip(lab, fl))
        srcs.append(ar.flip(src, fl))
    return np.stack(imgs), np.stack(labs), np.stack(srcs)


# ------------------------------------------------------------------------------------------ gates
def affine_coord_error(m, shape):
    """``_coord_error_bound`` of tests/test_augment_gpu.py: the f32 error of the affine part (12 entries
    rounded, three products and three sums per row) for indices up to max(shape) + 32"""
    m = np.eye(4) if m is None else m
    row = np.abs(m[:3, :3]).sum(1) * (max(shape) + 32) + np.abs(m[:3, 3])
    return float(8 * EPS32 * row.max())


def displacement_error(ctrl, shape):
    """Bound of the f32 error of ``a + u(a)`` per axis, from the arithmetic of the definition in f32 with
    A = max |ctrl|, n = the largest grid extent:

    * ``t = i * s``: s is rounded once and the product once, ``f = t - k`` once more: |df| <= 3 EPS (n - 3).
      The derivative of a cubic B-spline is a convex combination of neighbouring control differences,
      each at most 2 A, so over three axes this moves u by at most 3 * 2 A * 3 EPS (n - 3);
    * a weight is a cubic in f on [0, 1] with coefficients of magnitude <= 6, scaled by 1/6: its roundings act on
      intermediates of magnitude <= 6 before the scaling (6 f^2 reaches 6), i.e. <= 1 after it: about 6 EPS
      absolute, taken as 8 EPS;
    * the four-tap sum of one axis, in any association: four weight errors (8 EPS each) on values <= A
      plus 4 products and 3 sums rounded at magnitudes <= A (or, in the difference form, on differences
      <= 2 A with three weights): at most 64 EPS A; the sums of the next axis pass the error on with
      weights that sum to 1, three axes give 3 * 64 EPS A;
    * the addition ``a + u`` rounds once at magnitude <= max(shape) + A.
    """
    amp = float(np.abs(np.asarray(ctrl, dtype=np.float64)).max())
    n = max(ctrl.shape[1:])
    return EPS32 * ((18.0 * (n - 3) + 192.0) * amp + max(shape) + amp)


def coord_error(ctrl, m, shape):
    """delta: bound of the f32 error of the source coordinate = the affine map's row sum times the error
    of ``a + u`` plus the affine arithmetic's own error (indices within 32 of the volume: A < 32)"""
    mm = np.eye(4) if m is None else m
    return float(np.abs(mm[:3, :3]).sum(1).max() * displacement_error(ctrl, shape) + affine_coord_error(m, shape))


ULP = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}


def image_gate(got, ref, delta, lip, vmax, store="f32"):
    """(worst excess error, bound): the coordinate error on each of three axes times the interpolant's
    slope, the f32 lerps (7, each rounding at most vmax * EPS32 twice), and the one storage rounding"""
    tol = 3.0 * delta * lip + 16.0 * EPS32 * vmax
    err = np.abs(np.asarray(got, dtype=np.float64) - ref) - ULP[store] * np.abs(ref)
    return float(err.max()), float(tol)


def label_gate(got, ref, src, shape, delta):
    """number of label picks that differ where the float64 coordinate is NOT within 2 delta of a .5 boundary"""
    bad = np.asarray(got) != np.asarray(ref)
    return int((bad & ~ar.near_half(src, shape, 2.0 * delta)).sum())


# ------------------------------------------------------------------------- the GPU test's inputs
VOLUME = (33, 29, 41)
CHANNELS = 2
ROI = (16, 12, 20)
# n, z, y, x: inside, partly outside and fully outside the volume (SpatialPad zeros); flip code = index % 8
STARTS = [[0, 3, 5, 7], [0, 17, 17, 21], [0, -5, 4, 9], [0, 25, 22, 30], [0, -16, -12, -20], [0, 40, 0, 0],
          [0, 0, -13, 45], [0, 8, 6, -7], [0, 10, 9, 11], [0, -1, -1, -1], [0, 17, 17, 21], [0, 6, 10, 14],
          [0, -4, 12, 26], [0, 14, 0, 0], [0, 0, 15, 0], [0, 2, 2, 21]]
FLIPS = [i % 8 for i in range(16)]
GRIDS = [(4, 4, 4), (7, 7, 7), (4, 5, 9)]


def volume(shape=VOLUME, c=CHANNELS, seed=11):
    """(image [C, *shape] f32-representable float64, label [*shape] in 0..3)"""
    rng = np.random.RandomState(seed)
    img = rng.randn(c, *shape).astype(np.float32).astype(np.float64)
    lab = rng.randint(0, 4, shape).astype(np.float64)
    return img, lab


def largest_amplitude(shape, n):
    """the largest scalar max_displacement the no-fold check admits, less 0.1 %"""
    h = [(d - 1) / (k - 3) for d, k in zip(shape, n) if d > 1]
    return 0.999 / (2.0 * sum(1.0 / v for v in h))


def rotation_zoom_map(aug, shape=VOLUME):
    """the first map of ``augment.draw_spatial`` (seeds 0, 1, ...) that rotates about >= 2 axes and zooms"""
    seed = 0
    while True:
        m = aug.draw_spatial(np.random.RandomState(seed), shape)
        seed += 1
        if m is None:
            continue
        off = np.abs(m[:3, :3] - np.diag(np.diag(m[:3, :3]))) > 1e-6
        if abs(np.linalg.det(m[:3, :3]) - 1) > 1e-3 and np.count_nonzero(off) >= 4:
            return m


def control(shape, n, amplitude, seed):
    """control displacements drawn as ``augment.draw_elastic`` draws them: U(-A_a, A_a) per component in the
    order d0, d1, d2, A_a = ``amplitude`` or, for None, the default 0.12 control spacings.  Drawn directly:
    the kernel is defined for any grid, and on the anisotropic (4, 5, 9) grid the default amplitude is one
    the sampler's no-fold check would refuse."""
    rng = np.random.RandomState(seed)
    h = [(d - 1) / (k - 3) if d > 1 else 0.0 for d, k in zip(shape, n)]
    amp = [0.12 * v for v in h] if amplitude is None else [float(amplitude) if d > 1 else 0.0 for d in shape]
    return np.stack([rng.uniform(-a, a, size=tuple(n)) for a in amp]).astype(np.float32)


def kernel_cases(aug):
    """(name, ctrl, map) of the kernel-against-oracle test: each grid x {identity, rotation + zoom} x
    {default A, the largest admitted A}"""
    m = rotation_zoom_map(aug)
    out = []
    for gi, n in enumerate(GRIDS):
        for mi, mm in enumerate((None, m)):
            for ai, amp in enumerate((None, largest_amplitude(VOLUME, n))):
                ctrl = control(VOLUME, n, amp, 100 + 10 * gi + 2 * mi + ai)
                out.append((f"grid{n} {'affine' if mm is not None else 'identity'} "
                            f"{'Amax' if amp else 'Adefault'}", ctrl, mm))
    return out
