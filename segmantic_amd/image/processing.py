"""Drop-in for ``segmantic.image.processing`` (reference ``src/segmantic/image/processing.py``)
without SimpleITK: a minimal ``Image`` (voxel tensor + spacing / origin / direction, the subset of
``sitk.Image`` the reference touches) and ``resample`` / ``apply_transform`` /
``resample_to_ref`` running the ITK-semantics HIP kernels (``segmi_resample3d``, and for the
``sitkBSpline`` / ``sitkLabelGaussian`` interpolators ``segmi_resample3d_bspline`` /
``segmi_resample3d_label_gaussian``) instead of ITK's CPU ``ResampleImageFilter``.  ``read_image`` /
``write_image`` carry an ``Image`` to and from a file.  ``make_image / extract_slices / pad / crop_center / crop`` are host
metadata / slicing helpers, as in the reference (``:10-46, :123-156``).
"""
from __future__ import annotations

import math
from typing import Any, List, Optional, Sequence, Union

import numpy as np
import torch

# pixel ids (names follow SimpleITK)
sitkUInt8, sitkInt16, sitkUInt16, sitkInt32, sitkFloat32 = "uint8", "int16", "uint16", "int32", "float32"
_TORCH = {"uint8": torch.uint8, "int16": torch.int16, "uint16": torch.uint16, "int32": torch.int32,
          "float32": torch.float32}
_NAME = {v: k for k, v in _TORCH.items()}
# interpolators (names follow SimpleITK)
sitkLinear, sitkNearestNeighbor, sitkBSpline, sitkLabelGaussian = "linear", "nearest", "bspline", "label-gaussian"
_INTERPOLATORS = (sitkLinear, sitkNearestNeighbor, sitkBSpline, sitkLabelGaussian)


class Image:
    """Voxel grid in physical space.  ``data`` is a torch tensor indexed [z, y, x] (2-D: [y, x]),
    size / spacing / origin are (x, y, z) tuples, direction a row-major d x d matrix."""

    def __init__(self, data: Union[torch.Tensor, np.ndarray], spacing: Optional[Sequence[float]] = None,
                 origin: Optional[Sequence[float]] = None, direction: Optional[Sequence[float]] = None):
        if isinstance(data, np.ndarray):
            data = torch.from_numpy(np.ascontiguousarray(data))
        self.data = data
        d = data.dim()
        self.spacing = tuple(float(s) for s in (spacing if spacing is not None else [1.0] * d))
        self.origin = tuple(float(s) for s in (origin if origin is not None else [0.0] * d))
        self.direction = tuple(float(v) for v in (direction if direction is not None
                                                  else np.eye(d).reshape(-1)))
        if len(self.spacing) != d or len(self.origin) != d or len(self.direction) != d * d:
            raise ValueError("shape and spacing must have same dimension")

    # --- sitk-like accessors
    def GetDimension(self) -> int:
        return self.data.dim()

    def GetSize(self):
        return tuple(int(s) for s in reversed(self.data.shape))

    def GetSpacing(self):
        return self.spacing

    def GetOrigin(self):
        return self.origin

    def GetDirection(self):
        return self.direction

    def GetPixelID(self) -> str:
        return _NAME[self.data.dtype]

    def SetSpacing(self, s):
        self.spacing = tuple(float(v) for v in s)

    def SetOrigin(self, o):
        self.origin = tuple(float(v) for v in o)

    def SetDirection(self, d):
        self.direction = tuple(float(v) for v in d)

    def CopyInformation(self, other: "Image"):
        self.spacing, self.origin, self.direction = other.spacing, other.origin, other.direction

    def numpy(self) -> np.ndarray:
        return self.data.detach().cpu().numpy()

    # --- pixel access in sitk index order: x first (ints and slices)
    def _index(self, key):
        key = key if isinstance(key, tuple) else (key,)
        d = self.data.dim()
        if len(key) > d:
            raise IndexError(f"{len(key)} indices for a {d}-D image")
        for k in key:
            if not isinstance(k, (int, np.integer, slice)):
                raise TypeError(f"Image indices are ints or slices, not {type(k).__name__}")
        return (slice(None),) * (d - len(key)) + tuple(reversed(key))

    def __getitem__(self, key):
        """``image[x, y, z]`` -> pixel value; with slices -> an ``Image`` over that region (a view;
        the spacing of the kept axes, origin and direction carried over unchanged)."""
        idx = self._index(key)
        sub = self.data[idx]
        if sub.dim() == 0:
            return sub.item()
        kept = [a for a, k in zip(range(self.data.dim() - 1, -1, -1), idx) if isinstance(k, slice)]
        kept = sorted(kept)  # (x, y, z) axis numbers of the kept array axes
        dd = self.data.dim()
        direction = np.asarray(self.direction).reshape(dd, dd)[np.ix_(kept, kept)].reshape(-1)
        return Image(sub, [self.spacing[a] for a in kept], [self.origin[a] for a in kept], direction)

    def __setitem__(self, key, value):
        """``image[3:6, 3:6] = 1`` in sitk index order (x first)."""
        if isinstance(value, Image):
            value = value.data
        self.data[self._index(key)] = value


def make_image(shape: Sequence[int], spacing: Optional[Sequence[float]] = None,
               value: Union[int, float] = 0, pixel_type: Any = sitkUInt8) -> Image:
    """Create (2D/3D) image with specified shape (x, y[, z]) and spacing (reference ``:10-24``)."""
    if spacing and len(shape) != len(spacing):
        raise ValueError("shape and spacing must have same dimension")
    data = torch.full(tuple(reversed([int(s) for s in shape])), value, dtype=_TORCH[pixel_type])
    return Image(data, spacing)


def extract_slices(image: Image, axis: int = 2) -> List[Image]:
    """2D slices of a 3D image; ``axis`` (x=0,y=1,z=2) is perpendicular to the slices (``:27-46``)."""
    dim = 2 - axis
    keep = [a for a in range(3) if a != axis]
    out = []
    for k in range(image.data.shape[dim]):
        sl = image.data.select(dim, k)
        direction = np.asarray(image.direction).reshape(3, 3)[np.ix_(keep, keep)].reshape(-1)
        out.append(Image(sl, [image.spacing[a] for a in keep], [image.origin[a] for a in keep],
                         direction))
    return out


def _index_map(moving: Image, out_spacing, out_origin, out_direction, transform) -> np.ndarray:
    """3x4 affine: output index (x,y,z,1) -> continuous index in ``moving``."""
    nd = moving.GetDimension()
    d_out = np.asarray(out_direction, np.float64).reshape(nd, nd)
    d_in = np.asarray(moving.direction, np.float64).reshape(nd, nd)
    a = d_out @ np.diag(np.asarray(out_spacing, np.float64))      # index -> physical (linear)
    t = np.asarray(out_origin, np.float64)
    if transform is not None:
        tm = np.asarray(transform, np.float64)
        a = tm[:nd, :nd] @ a
        t = tm[:nd, :nd] @ t + tm[:nd, nd]
    inv = np.diag(1.0 / np.asarray(moving.spacing, np.float64)) @ np.linalg.inv(d_in)
    m = np.zeros((3, 4))
    m[:nd, :nd] = inv @ a
    m[:nd, 3] = inv @ (t - np.asarray(moving.origin, np.float64))
    if nd == 2:
        m[2, 2] = 1.0
    return m


def _interpolator(nearest: bool, interpolator, sigma, alpha) -> str:
    """The interpolator a call asks for, checked on the host: ``None`` means what ``nearest`` says."""
    if interpolator is None:
        interpolator = sitkNearestNeighbor if nearest else sitkLinear
    if interpolator not in _INTERPOLATORS:
        raise ValueError(f"unknown interpolator {interpolator!r}: one of {', '.join(_INTERPOLATORS)}")
    if nearest and interpolator != sitkNearestNeighbor:
        raise ValueError(f"nearest=True contradicts interpolator={interpolator!r}")
    if interpolator != sitkLabelGaussian and not (np.all(np.asarray(sigma) == 1.0) and alpha == 2.0):
        raise ValueError(f"sigma / alpha belong to interpolator={sitkLabelGaussian!r}, not to {interpolator!r}")
    if interpolator == sitkLabelGaussian:
        sg = np.asarray(sigma, np.float64)
        if sg.shape not in ((), (2,), (3,)) or not np.all(sg > 0) or not alpha > 0:
            raise ValueError(f"sigma (a number or one per axis) and alpha must be positive, got {sigma!r}, {alpha!r}")
    return interpolator


def _resample_to_grid(moving: Image, size, spacing, origin, direction, transform, nearest: bool,
                      device=None, interpolator=None, sigma=1.0, alpha=2.0) -> Image:
    from .. import ops
    interpolator = _interpolator(nearest, interpolator, sigma, alpha)
    nd = moving.GetDimension()
    if nd not in (2, 3):
        raise ValueError("resample supports 2D / 3D images")
    sg = np.asarray(sigma, np.float64)
    if sg.ndim and sg.shape != (nd,):
        raise ValueError(f"sigma has {sg.size} entries for a {nd}-D image")
    sg = np.broadcast_to(sg, (nd,))
    sg = np.concatenate([sg, np.full(3 - nd, sg.min())])      # 2-D: the z axis has extent 1, its sigma is idle
    dev = device or (moving.data.device if moving.data.is_cuda else torch.device("cuda:0"))
    if not torch.cuda.is_available():
        raise RuntimeError("segmantic_amd resample runs on an MI355X (no CPU path)")
    src = moving.data.to(dev).contiguous()
    m = _index_map(moving, spacing, origin, direction, transform)
    if nd == 2:
        src = src.unsqueeze(0)
        out_zyx = (1, int(size[1]), int(size[0]))
    else:
        out_zyx = (int(size[2]), int(size[1]), int(size[0]))
    if interpolator == sitkBSpline:
        dst = ops.resample3d_bspline(src, out_zyx, m, default=0.0)
    elif interpolator == sitkLabelGaussian:
        dst = ops.resample3d_label_gaussian(src, out_zyx, m, sigma=sg, alpha=alpha, default=0.0)
    else:
        dst = ops.resample3d(src, out_zyx, m, nearest=interpolator == sitkNearestNeighbor, default=0.0)
    if nd == 2:
        dst = dst[0]
    if not moving.data.is_cuda and device is None:
        dst = dst.cpu()
    return Image(dst, spacing, origin, direction)


def resample(image: Image, target_spacing: Sequence[float], nearest: bool = False, *, interpolator=None,
             sigma=1.0, alpha=2.0) -> Image:
    """resample (2D/3D) image to a target spacing (reference ``:49-71``): size' =
    ceil(size * spacing / target), same origin / direction, identity transform, default pixel 0,
    output pixel type = input pixel type.  ``interpolator``: ``sitkLinear``, ``sitkNearestNeighbor``,
    ``sitkBSpline`` or ``sitkLabelGaussian`` (``None``: what ``nearest`` says); ``sigma`` (in voxels of
    ``image``, a number or one per axis x, y[, z]) and ``alpha`` shape the label-Gaussian window."""
    _interpolator(nearest, interpolator, sigma, alpha)
    size = list(image.GetSize())
    spacing = list(image.GetSpacing())
    for d in range(image.GetDimension()):
        size[d] = math.ceil(size[d] * spacing[d] / target_spacing[d])
        spacing[d] = float(target_spacing[d])
    return _resample_to_grid(image, size, spacing, image.GetOrigin(), image.GetDirection(), None,
                             nearest, interpolator=interpolator, sigma=sigma, alpha=alpha)


def apply_transform(moving_image: Image, fixed_image: Image, transform: Optional[np.ndarray],
                    nearest: bool, *, interpolator=None, sigma=1.0, alpha=2.0) -> Image:
    """Resample ``moving_image`` onto the grid of ``fixed_image``; ``transform`` (homogeneous
    (d+1)x(d+1) matrix or None = identity) maps fixed -> moving physical points (``:74-98``).
    ``interpolator`` / ``sigma`` / ``alpha`` as in ``resample``."""
    return _resample_to_grid(moving_image, fixed_image.GetSize(), fixed_image.GetSpacing(),
                             fixed_image.GetOrigin(), fixed_image.GetDirection(), transform, nearest,
                             interpolator=interpolator, sigma=sigma, alpha=alpha)


def resample_to_ref(moving_image: Image, fixed_image: Image, nearest: bool, *, interpolator=None, sigma=1.0,
                    alpha=2.0) -> Image:
    """resample (2D/3D) image to a reference grid (reference ``:101-120``)."""
    return apply_transform(moving_image, fixed_image, None, nearest, interpolator=interpolator, sigma=sigma,
                           alpha=alpha)


_LPS_TO_RAS = np.diag([-1.0, -1.0, 1.0, 1.0])


def read_image(path) -> Image:
    """Read a NIfTI / MetaImage / NRRD file (``data.imageio``) as an ``Image``.  The file's RAS affine becomes ITK's
    LPS geometry: spacing = the length of each voxel axis, direction = the unit axes as columns, origin = the
    position of voxel 0.  A 2-D file gives a 2-D image with the in-plane 2 x 2 part of that geometry.  float64
    voxels are narrowed to float32; other pixel types than the five of ``Image`` are refused."""
    from ..data import imageio
    arr, affine = imageio.read_image(path)
    if arr.dtype == np.float64:
        arr = arr.astype(np.float32)
    if arr.dtype.name not in _TORCH:
        raise ValueError(f"{path}: pixel type {arr.dtype} is not one of {', '.join(_TORCH)}")
    if arr.ndim not in (2, 3):
        raise ValueError(f"{path}: {arr.ndim}-D data; images are 2-D or 3-D")
    nd = arr.ndim
    a = _LPS_TO_RAS @ np.asarray(affine, np.float64)
    spacing = np.sqrt((a[:nd, :nd] ** 2).sum(0))
    spacing[spacing == 0] = 1.0
    return Image(arr, spacing, a[:nd, 3], (a[:nd, :nd] / spacing).reshape(-1))


def write_image(image: Image, path) -> None:
    """Write an ``Image`` to a NIfTI / MetaImage / NRRD file: the inverse of ``read_image`` (a 2-D image is written
    as a 2-D NIfTI, and as a single slice in the formats that are 3-D only)."""
    from ..data import imageio
    nd = image.GetDimension()
    a = np.eye(4)
    a[:nd, :nd] = np.asarray(image.direction, np.float64).reshape(nd, nd) * np.asarray(image.spacing, np.float64)
    a[:nd, 3] = image.origin
    arr = image.numpy()
    if nd == 2 and not str(path).lower().endswith((".nii", ".nii.gz")):
        arr = arr[None]
    imageio.write_image(path, arr, _LPS_TO_RAS @ a)


def pad(image: Image, target_size: Sequence[int], value: float = 0) -> Image:
    """Pad to the target size.  NB the reference computes ``delta = max(s, t) - t`` (``:125-126``),
    i.e. it pads only when the image is LARGER than the target; restated as is."""
    size = image.GetSize()
    delta = [max(s, t) - t for s, t in zip(size, target_size)]
    if any(delta):
        lo = [(d + 1) // 2 for d in delta]
        hi = [d - p for d, p in zip(delta, lo)]
        padding = []
        for l, h in zip(lo, hi):            # F.pad wants last dim first = x first
            padding += [l, h]
        data = torch.nn.functional.pad(image.data, padding, value=value)
        origin = np.asarray(image.origin) - np.asarray(image.direction).reshape(len(size), -1) @ (
            np.asarray(lo) * np.asarray(image.spacing))
        return Image(data, image.spacing, origin, image.direction)
    return image


def crop_center(image: Image, target_size: Sequence[int]) -> Image:
    """Crop to the target size, centred (reference ``:136-146``)."""
    size = image.GetSize()
    delta = [max(s, t) - t for s, t in zip(size, target_size)]
    if any(delta):
        lo = [(d + 1) // 2 for d in delta]
        return crop(image, lo, [s - d for s, d in zip(size, delta)])
    return image


def crop(img: Image, target_offset: Sequence[int], target_size: Sequence[int]) -> Image:
    """Crop to offset / size given in (x, y, z) (reference ``:149-156``)."""
    nd = img.GetDimension()
    sl = tuple(slice(int(target_offset[d]), int(target_offset[d]) + int(target_size[d]))
               for d in reversed(range(nd)))
    origin = np.asarray(img.origin) + np.asarray(img.direction).reshape(nd, nd) @ (
        np.asarray(target_offset, np.float64) * np.asarray(img.spacing))
    data = img.data[sl]
    keep = [d for d in range(nd) if int(target_size[d]) > 0]
    return Image(data, img.spacing, origin, img.direction)
