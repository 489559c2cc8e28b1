"""MRI and CT preprocessing on the MI355X: a drop-in for the reference's ``segmantic.image.modality``
(``bias_correct``, ``scale_clamp_ct``, ``unscale_ct``) on :class:`segmantic_amd.image.processing.Image`.

Arrays are [z, y, x] (2-D: [y, x]); spacing and origin are (x, y, z).  Results keep the input's geometry
and device (a CPU image comes back on the CPU); the computation always runs on the GPU
(``csrc/n4.hip``), and without one every function raises ``RuntimeError``.

The contract (restated in float64 by ``tests/helpers/n4_ref.py``).  SimpleITK is not a
dependency, so none of it has been checked against ITK: each rule is this project's definition, and the
ones marked *reading* are how we read ITK, not verified facts.

- Otsu (``otsu_threshold``): 200 equal bins over [min, max] of the finite voxels, bin = min(floor((v - min)
  / w), 199), exact counts; the bin k maximising the between-class variance with bin-centre class values
  (first maximum wins); threshold = min + (k + 1) w, the upper edge of bin k (*reading*); ``outside_value``
  where v > threshold, ``inside_value`` elsewhere.  The N4 mask is therefore the bright part of the image.
- Shrink (``shrink``, *reading* of ITK's ShrinkImageFilter): ns = max(1, n // f) per axis; output voxel j
  takes input voxel j f + o, o = floor(((n - 1) - (ns - 1) f) / 2 + 0.5); spacing f * spacing; the origin
  moves so that the physical centres of input and output coincide.
- Fit set: the shrunk voxels with mask == 1, input > 0 and finite input; ``ValueError`` when it has fewer
  than 2 voxels or one log value.  N4 works on L = log(input) there.
- Levels: level l has m = (c0 - 3) 2^l spans per axis (c0 control points), m + 3 control points; axes of
  size 1 carry no spline dimension.  The log-field lattice starts at 0.  Per level, while iterations <
  max[l] and CV > threshold (CV = +inf at the start of each level): sharpen U = L - field, fit the residual
  U - sharpened(U) with one BA level, add that lattice, re-evaluate the field, CV = sample std (N - 1) /
  mean of exp(old - new) over the fit set.  Between levels the lattice is refined by exact cubic
  subdivision (the same function).
- Sharpening (*reading* of ITK's SharpenImage): slope = (max U - min U) / (bins - 1), linear splatting
  into the histogram, zero padding to P = 2^(ceil(log2 bins) + 1) at offset (P - bins) // 2, Gaussian
  F[n] = s exp(-e n^2) wrapped symmetrically (fw = FWHM / slope, e = 4 ln2 / fw^2, s = 2 sqrt(ln2 / pi) /
  fw), Wiener filter conj(F^) / (|F^|^2 + noise), U~ = max(Re IDFT(H^ G), 0), E = (x U~ (*) F) /
  (U~ (*) F) (0 where the denominator is 0), each value's E interpolated linearly (E[bins - 1] at the
  last bin).
- BA fit (Lee-Wolberg-Shin): u = i / (n - 1) m, span min(floor u, m - 1), cubic B-spline weights w_k;
  num[k] += w_k^2 phi_k with phi_k = r w_k / sum w^2, den[k] += w_k^2, lattice = num / den (0 where
  den = 0).
- Full resolution (``GetLogBiasFieldAsImage``, *reading* of how SimpleITK maps the lattice onto the
  reference image): the lattice is evaluated at u = i / (N - 1) m over the reference's own index range,
  so the shrunk grid's origin plays no part; ``bias_correct`` returns input / exp(log field) as float32.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import torch

from .. import ops
from .processing import Image

__all__ = ["bias_correct", "scale_clamp_ct", "unscale_ct", "shrink", "otsu_threshold",
           "N4BiasFieldCorrectionImageFilter"]


def _device(image: Image) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("segmantic_amd.image.modality runs on an MI355X (no CPU path)")
    return image.data.device if image.data.is_cuda else torch.device("cuda:0")


def _home(t: torch.Tensor, like: Image) -> torch.Tensor:
    return t if like.data.is_cuda else t.cpu()


def _f32(image: Image, dev) -> torch.Tensor:
    if image.GetDimension() not in (2, 3):
        raise ValueError("modality functions support 2-D and 3-D images")
    return image.data.to(dev).to(torch.float32).contiguous()


def _factors(image: Image, factor) -> list:
    """shrink factors in array ([z, y, x]) order from an int or an (x, y, z) sequence"""
    d = image.GetDimension()
    f = [int(factor)] * d if np.isscalar(factor) else [int(v) for v in factor]
    if len(f) != d or min(f) < 1:
        raise ValueError("one shrink factor >= 1 per axis")
    return list(reversed(f)) if not np.isscalar(factor) else f


def _shrunk_geometry(image: Image, f_zyx):
    d = image.GetDimension()
    f = list(reversed(f_zyx))  # (x, y, z)
    size = image.GetSize()
    ns = [max(1, n // fa) for n, fa in zip(size, f)]
    shift = np.array([((n - 1) - (m - 1) * fa) / 2.0 for n, m, fa in zip(size, ns, f)]) * np.asarray(image.spacing)
    origin = np.asarray(image.origin) + np.asarray(image.direction).reshape(d, d) @ shift
    spacing = [s * fa for s, fa in zip(image.spacing, f)]
    return spacing, origin


def shrink(image: Image, factor: Union[int, Sequence[int]]) -> Image:
    """``sitk.Shrink``: one factor for every axis, or one per axis in (x, y, z) order.  The pixel type is
    kept; values travel through the gather as float32 (exact for integers up to 2^24 in magnitude)."""
    dev = _device(image)
    f = _factors(image, factor)
    img, _, _ = ops.n4_shrink(_f32(image, dev), f, want_mask=False)
    if image.data.dtype != torch.float32:
        img = img.to(image.data.dtype)
    spacing, origin = _shrunk_geometry(image, f)
    return Image(_home(img, image), spacing, origin, image.direction)


def otsu_threshold(image: Image, inside_value: int = 0, outside_value: int = 1, bins: int = 200) -> Image:
    """``sitk.OtsuThreshold(image, inside_value, outside_value, bins)``: uint8, ``outside_value`` where the
    voxel is above the threshold (see the module docstring for the rule)."""
    dev = _device(image)
    x = _f32(image, dev)
    _, stats = ops.otsu(x, bins)
    if float(stats[3]) == 0:
        raise ValueError("otsu_threshold: the image has no finite voxel")
    _, mask, _ = ops.n4_shrink(x, [1] * x.dim(), otsu_stats=stats, inside=inside_value, outside=outside_value,
                               want_image=False)
    out = Image(_home(mask, image), image.spacing, image.origin, image.direction)
    out.threshold = float(stats[2])
    return out


def _mask_u8(mask: Image, like: torch.Tensor) -> torch.Tensor:
    m = mask.data.to(like.device)
    if tuple(m.shape) != tuple(like.shape):
        raise ValueError("the mask must have the image's size")
    return m.contiguous() if m.dtype == torch.uint8 else (m == 1).to(torch.uint8).contiguous()


class N4BiasFieldCorrectionImageFilter:
    """The subset of SimpleITK's N4 filter that the reference uses (spline order 3 only).
    ``Execute(image, mask)`` fits the log bias field on the given grid and returns image / exp(field);
    ``GetLogBiasFieldAsImage(reference)`` evaluates the fitted lattice over another image's index range."""

    def __init__(self):
        self._iterations = [50, 50, 50, 50]
        self._threshold = 0.001
        self._bins = 200
        self._fwhm = 0.15
        self._noise = 0.01
        self._control_points = 4
        self._lattice: Optional[torch.Tensor] = None
        self._elapsed: list = []
        self._cv = float("inf")

    # --- settings
    def SetMaximumNumberOfIterations(self, iterations: Sequence[int]):
        it = [int(v) for v in iterations]
        if not it or min(it) < 0:
            raise ValueError("one non-negative iteration count per fitting level")
        self._iterations = it

    def GetMaximumNumberOfIterations(self):
        return list(self._iterations)

    def SetConvergenceThreshold(self, v: float):
        self._threshold = float(v)

    def GetConvergenceThreshold(self) -> float:
        return self._threshold

    def SetNumberOfHistogramBins(self, n: int):
        if not 2 <= int(n) <= ops.N4_MAX_BINS:
            raise ValueError(f"2 <= bins <= {ops.N4_MAX_BINS}")
        self._bins = int(n)

    def GetNumberOfHistogramBins(self) -> int:
        return self._bins

    def SetBiasFieldFullWidthAtHalfMaximum(self, v: float):
        if not v > 0:
            raise ValueError("the FWHM must be positive")
        self._fwhm = float(v)

    def GetBiasFieldFullWidthAtHalfMaximum(self) -> float:
        return self._fwhm

    def SetWienerFilterNoise(self, v: float):
        if not v >= 0:
            raise ValueError("the Wiener filter noise must be >= 0")
        self._noise = float(v)

    def GetWienerFilterNoise(self) -> float:
        return self._noise

    def SetNumberOfControlPoints(self, n):
        c = [int(v) for v in n] if not np.isscalar(n) else [int(n)]
        if len(set(c)) != 1 or c[0] < 4:
            raise ValueError("one number of control points (>= 4) for every axis")
        self._control_points = c[0]

    def GetNumberOfControlPoints(self) -> int:
        return self._control_points

    def SetSplineOrder(self, order: int):
        if int(order) != 3:
            raise ValueError("only cubic B-splines (spline order 3) are supported")

    def GetSplineOrder(self) -> int:
        return 3

    # --- fitting
    def _fit_log(self, logimg: torch.Tensor) -> None:
        lat, _, elapsed, cv = ops.n4_fit(logimg, self._iterations, self._control_points, self._bins, self._fwhm,
                                         self._noise, self._threshold)
        self._lattice, self._elapsed, self._cv = lat, elapsed, cv

    def Execute(self, image: Image, mask: Optional[Image] = None) -> Image:
        dev = _device(image)
        x = _f32(image, dev)
        m = _mask_u8(mask, x) if isinstance(mask, Image) else None
        _, _, logimg = ops.n4_shrink(x, [1] * x.dim(), mask=m, want_image=False, want_mask=False, want_log=True)
        self._fit_log(logimg)
        out = ops.n4_evaluate(self._lattice, x.shape, x)
        return Image(_home(out, image), image.spacing, image.origin, image.direction)

    def _need_fit(self):
        if self._lattice is None:
            raise RuntimeError("the filter has not been executed")

    def GetLogBiasFieldAsImage(self, reference: Image) -> Image:
        self._need_fit()
        dev = _device(reference)
        shape = tuple(reference.data.shape)
        out = ops.n4_evaluate(self._lattice.to(dev), shape)
        return Image(_home(out, reference), reference.spacing, reference.origin, reference.direction)

    def GetLogBiasFieldControlPointLattice(self) -> np.ndarray:
        """the control points of the log bias field, f64 [Lz, Ly, Lx] (axes of size 1 have one point)"""
        self._need_fit()
        return self._lattice.cpu().numpy()

    def GetElapsedIterations(self) -> list:
        """iterations run at each fitting level"""
        return list(self._elapsed)

    def GetCurrentConvergenceMeasurement(self) -> float:
        return self._cv


def bias_correct(input: Image, mask: Optional[Image] = None, shrink_factor: int = 4, num_fitting_levels: int = 4,
                 num_iterations: int = 50) -> Image:
    """Perform N4 bias correction on MRI (the reference's signature and defaults).

    Without an ``Image`` mask the mask is ``otsu_threshold(input, 0, 1, 200)``.  Input and mask are shrunk
    by ``shrink_factor`` along every axis, N4 is fitted with ``[num_iterations] * num_fitting_levels``
    iterations, and the result is input / exp(log bias field) at full resolution, float32.  The Otsu
    threshold runs on the float32 copy of the input."""
    dev = _device(input)
    x = _f32(input, dev)
    f = [int(shrink_factor)] * x.dim()
    if isinstance(mask, Image):
        _, _, logimg = ops.n4_shrink(x, f, mask=_mask_u8(mask, x), want_image=False, want_mask=False, want_log=True)
    else:
        _, stats = ops.otsu(x, 200)
        _, _, logimg = ops.n4_shrink(x, f, otsu_stats=stats, want_image=False, want_mask=False, want_log=True)
    corrector = N4BiasFieldCorrectionImageFilter()
    corrector.SetMaximumNumberOfIterations([num_iterations] * num_fitting_levels)
    corrector._fit_log(logimg)
    out = ops.n4_evaluate(corrector._lattice, x.shape, x)
    return Image(_home(out, input), input.spacing, input.origin, input.direction)


def scale_clamp_ct(img: Image) -> Image:
    """Prepare CT images: median (radius 1) -> clamp to [-1100, 3100] -> scale to [0, 255].

    The reference's ``sitk.Clamp(-1100, 3100)`` drops its image argument; this is the intended behaviour,
    the clamp of the median-filtered image.  The median uses replicate borders (ITK's zero-flux Neumann
    condition) and is exact; clamp and scale run in float32 as (v + 1100) * fl(255 / 4200), each operation
    rounded, within 1 ulp of the float64 value of (v + 1100) * 255 / 4200.  The output is float32 for every input pixel type: whether SimpleITK keeps an integer input's
    type here is unverified, and float32 keeps the scaled values' fractions."""
    dev = _device(img)
    x = _f32(img, dev)
    out = ops.ct_scale(x)
    return Image(_home(out, img), img.spacing, img.origin, img.direction)


def unscale_ct(img: Image) -> Image:
    """Invert ``scale_clamp_ct``, except for the clamping: 4200 / 255 * v - 1100 (float32, on the GPU)."""
    dev = _device(img)
    x = img.data.to(dev).to(torch.float32)
    out = (1100.0 + 3100.0) / 255.0 * x - 1100.0
    return Image(_home(out, img), img.spacing, img.origin, img.direction)
