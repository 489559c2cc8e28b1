"""Label-map transforms on the MI355X: connected components, the clean-up transforms MONAI runs on the CPU
(``KeepLargestConnectedComponent``, ``RemoveSmallObjects``, ``FillHoles``) and the reference's ``MapLabels``
/ ``MapLabelsd`` (``src/segmantic/seg/transforms.py:91-127``), computed by the HIP kernels of
``csrc/components.hip``.  There is no CPU fallback: with no GPU every entry raises ``RuntimeError``.
(``SelectBestEnsemble`` of the same reference file lives in ``seg/monai_unet.py`` / ``csrc/ensemble.hip``.)

Contract
--------
MONAI and scikit-image are not part of this project; the definitions below are the specification and the
tests check them against a numpy restatement (``tests/helpers/components_ref.py``) with exact equality.

* Arrays are ``[z, y, x]`` (3-D) or ``[y, x]`` (2-D) label maps of an integer type; ``uint8``, ``int16`` and
  ``int32`` are read in place, ``bool`` is read as ``uint8`` and other integer types as ``int32``.  A volume
  holds fewer than ``2^31`` voxels (``ValueError`` otherwise).
* **Connectivity** ``c`` in ``1..ndim``, as ``scipy.ndimage.generate_binary_structure(ndim, c)``: neighbours
  differ by at most 1 along every axis and along at most ``c`` axes (3-D: 6 / 18 / 26, 2-D: 4 / 8).
  ``None`` means ``ndim`` (full connectivity, MONAI's and scikit-image's default).
* **Component**: a maximal set of voxels that carry the *same* value and are linked by neighbour steps.  With
  ``background=0`` the voxels equal to 0 belong to no component; one pass labels the components of all
  classes at once.  ``background=None`` labels the 0-regions too.
* **Canonical numbering**: components are numbered ``1..n`` in raster order (z, then y, then x) of their
  first voxel.  For a binary mask this is ``scipy.ndimage.label``'s numbering.
* **Size**: the voxel count.  **Largest**: components of one class are ordered by (size descending, first
  voxel ascending); MONAI leaves ties to ``argsort``, here the earlier component wins.
* **Hole**: a component of the 0-region under connectivity ``c`` that contains no voxel on the array border
  and whose neighbouring non-zero voxels (same ``c``) all carry one single value ``L``.  It is filled with
  ``L`` when ``L`` is in ``applied_labels`` (default: every label).  A 0-region bordered by two or more
  classes, or touching the border, stays 0.
* The clean-up transforms index per-class tables: label values must lie in ``0..65535`` (``ValueError``
  otherwise; this check is their one host synchronisation, and ``uint8`` inputs skip it).
  ``connected_components`` only compares values and takes any.
* ``MapLabels``: ``lookup`` of length ``max(mapping) + 1`` with unmapped entries 0; the result is
  ``lookup[img]`` as ``int64`` (or ``out_dtype``).  A value ``>= len(lookup)`` raises ``IndexError`` as in the
  reference; so does a negative value (torch would wrap it round -- a deliberate deviation).
* numpy arrays in -> numpy out, tensors in -> tensors on the input's device out,
  :class:`~segmantic_amd.image.processing.Image` in -> ``Image`` out with the geometry copied.  The input
  is never modified.

Deviations from MONAI: the tie rule above; one-hot inputs are refused (``ValueError``) because the predict
chain produces label maps; there is no bundle-configuration hook.
"""
from __future__ import annotations

from typing import Dict, Hashable, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .._arrays import MAX_LABEL, ArrayLike, Image, _back, _is_integer, _raw, _require_gpu, _to_device, _wrap

MAX_VOXELS = 2 ** 31
MAX_COMPONENTS = 8
_NEEDS_GPU = "segmantic_amd.seg.transforms needs an MI355X"


def _ops():
    from .. import ops
    return ops


# ------------------------------------------------------------------ host-side validation and conversion
def _check_labels(x: ArrayLike, what: str = "labels"):
    """shape / dtype checks that need neither a copy nor the device -> the raw array"""
    a = _raw(x)
    shape = tuple(int(s) for s in a.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"{what}: label maps are 2-D [y, x] or 3-D [z, y, x], got shape {shape}")
    if not _is_integer(a):
        raise ValueError(f"{what}: label maps must hold integers, got {a.dtype}")
    n = 1
    for s in shape:
        n *= s
    if n == 0:
        raise ValueError(f"{what}: empty label map of shape {shape}")
    if n >= MAX_VOXELS:
        raise ValueError(f"{what}: {n} voxels; a label map holds fewer than 2^31")
    return a


def _check_connectivity(connectivity, ndim: int) -> int:
    if connectivity is None:
        return ndim
    if isinstance(connectivity, bool) or int(connectivity) != connectivity or not 1 <= int(connectivity) <= ndim:
        raise ValueError(f"connectivity must be an integer in 1 .. {ndim} for a {ndim}-D label map, got {connectivity!r}")
    return int(connectivity)


def _check_applied(applied_labels) -> Optional[list]:
    if applied_labels is None:
        return None
    if isinstance(applied_labels, (int, np.integer)):
        applied_labels = [applied_labels]
    out = sorted({int(v) for v in applied_labels})
    if any(v < 0 or v > MAX_LABEL for v in out):
        raise ValueError(f"applied_labels must lie in 0 .. {MAX_LABEL}, got {out}")
    return out


# ------------------------------------------------------------------ functions
def connected_components(labels: ArrayLike, connectivity: Optional[int] = None, background: Optional[int] = 0):
    """-> (components int32, n): the canonical component number ``1..n`` of every voxel (0 for voxels of no
    component) and the count.  ``background`` is 0 or ``None`` (label the 0-regions too).  Reading ``n`` is
    the one host synchronisation."""
    a = _check_labels(labels)
    c = _check_connectivity(connectivity, len(a.shape))
    if background not in (0, None):
        raise ValueError(f"background must be 0 or None, got {background!r}")
    dev = _require_gpu(_NEEDS_GPU)
    ops = _ops()
    t = _to_device(a, dev)
    root = ops.cc_label(t, c, with_background=background is None)
    comp, n = ops.cc_compact(root)
    return _wrap(labels, comp), int(n.item())


def component_sizes(labels: ArrayLike, connectivity: Optional[int] = None):
    """-> int64 [n]: voxel counts of the components in canonical order."""
    a = _check_labels(labels)
    c = _check_connectivity(connectivity, len(a.shape))
    dev = _require_gpu(_NEEDS_GPU)
    ops = _ops()
    root = ops.cc_label(_to_device(a, dev), c)
    size = ops.cc_sizes(root).reshape(-1)
    # sizes sit at the roots, and the roots in raster order are the canonical order
    sizes = size[size > 0].to(torch.int64)
    if isinstance(_raw(labels), np.ndarray):
        return sizes.cpu().numpy()
    return sizes.to(_raw(labels).device)


def keep_largest_connected_component(labels: ArrayLike, applied_labels: Optional[Sequence[int]] = None,
                                     independent: bool = True, connectivity: Optional[int] = None,
                                     num_components: int = 1):
    """Keep the ``num_components`` largest components of every applied class (default: every non-zero
    label); the other voxels of those classes become 0.  ``independent=False`` takes the applied classes as
    one foreground: the largest components of their union are kept, with the per-voxel classes unchanged."""
    a = _check_labels(labels)
    c = _check_connectivity(connectivity, len(a.shape))
    applied = _check_applied(applied_labels)
    if isinstance(num_components, bool) or int(num_components) != num_components or \
            not 1 <= int(num_components) <= MAX_COMPONENTS:
        raise ValueError(f"num_components must be an integer in 1 .. {MAX_COMPONENTS}, got {num_components!r}")
    dev = _require_gpu(_NEEDS_GPU)
    ops = _ops()
    t = _to_device(a, dev, check_range=True)
    if applied is not None:
        applied = [v for v in applied if v != 0]
        if not applied:
            return _back(labels, t.clone())
    if independent:
        root = ops.cc_label(t, c)
        out = ops.cc_keep_largest(t, root, ops.cc_sizes(root), applied, True, int(num_components))
    else:
        if applied is None:
            mask = (t != 0).to(torch.uint8)
        else:
            # an applied label that the volume's storage type cannot hold is absent from the volume
            info = torch.iinfo(t.dtype)
            held = [v for v in applied if info.min <= v <= info.max]
            if not held:
                return _back(labels, t.clone())
            mask = torch.isin(t, torch.tensor(held, dtype=t.dtype, device=dev)).to(torch.uint8)
        root = ops.cc_label(mask, c)
        out = ops.cc_keep_largest(t, root, ops.cc_sizes(root), None, False, int(num_components))
    return _back(labels, out)


def remove_small_objects(labels: ArrayLike, min_size: int = 64, connectivity: Optional[int] = 1):
    """Voxels of components with fewer than ``min_size`` voxels become 0."""
    a = _check_labels(labels)
    c = _check_connectivity(connectivity, len(a.shape))
    if isinstance(min_size, bool) or int(min_size) != min_size or int(min_size) < 0:
        raise ValueError(f"min_size must be an integer >= 0, got {min_size!r}")
    dev = _require_gpu(_NEEDS_GPU)
    ops = _ops()
    t = _to_device(a, dev, check_range=True)
    root = ops.cc_label(t, c)
    return _back(labels, ops.cc_remove_small(t, root, ops.cc_sizes(root), int(min_size)))


def fill_holes(labels: ArrayLike, applied_labels: Optional[Sequence[int]] = None,
               connectivity: Optional[int] = None):
    """Fill every hole (see the module docstring) with the label that encloses it."""
    a = _check_labels(labels)
    c = _check_connectivity(connectivity, len(a.shape))
    applied = _check_applied(applied_labels)
    dev = _require_gpu(_NEEDS_GPU)
    ops = _ops()
    t = _to_device(a, dev, check_range=True)
    if applied is not None:
        applied = [v for v in applied if v != 0]
        if not applied:
            return _back(labels, t.clone())
    root = ops.cc_label(t, c, with_background=True)
    return _back(labels, ops.cc_fill_holes(t, root, applied, c))


# ------------------------------------------------------------------ MONAI-style callables
def _channel_first(x: ArrayLike, is_onehot) -> Tuple[ArrayLike, tuple]:
    """[d, h, w] / [h, w] as they are; channel-first [1, d, h, w] / [1, h, w] without the channel.
    -> (the label map, the shape to give the result)"""
    if is_onehot:
        raise ValueError("is_onehot=True: one-hot inputs are not supported, pass the label map (argmax)")
    a = _raw(x)
    shape = tuple(int(s) for s in a.shape)
    if len(shape) == 4 or (len(shape) == 3 and shape[0] == 1):
        if shape[0] != 1:
            raise ValueError(f"is_onehot: a {shape[0]}-channel input is taken to be one-hot, which is not "
                             f"supported; pass the label map (argmax)")
        if isinstance(x, Image):
            raise ValueError("an Image carries no channel axis")
        return a[0], shape
    return x, shape


def _restore(out, shape: tuple):
    if isinstance(out, Image) or tuple(out.shape) == shape:
        return out
    return out.reshape(shape)


class KeepLargestConnectedComponent:
    """MONAI's ``KeepLargestConnectedComponent`` on a label map."""

    def __init__(self, applied_labels: Optional[Sequence[int]] = None, is_onehot: Optional[bool] = None,
                 independent: bool = True, connectivity: Optional[int] = None, num_components: int = 1) -> None:
        if is_onehot:
            raise ValueError("is_onehot=True: one-hot inputs are not supported, pass the label map (argmax)")
        self.applied_labels = _check_applied(applied_labels)
        self.independent, self.connectivity, self.num_components = independent, connectivity, num_components

    def __call__(self, img: ArrayLike):
        x, shape = _channel_first(img, None)
        return _restore(keep_largest_connected_component(x, self.applied_labels, self.independent,
                                                         self.connectivity, self.num_components), shape)


class RemoveSmallObjects:
    """MONAI's ``RemoveSmallObjects`` on a label map."""

    def __init__(self, min_size: int = 64, connectivity: int = 1, independent_channels: bool = True) -> None:
        if isinstance(min_size, bool) or int(min_size) != min_size or int(min_size) < 0:
            raise ValueError(f"min_size must be an integer >= 0, got {min_size!r}")
        self.min_size, self.connectivity = int(min_size), connectivity

    def __call__(self, img: ArrayLike):
        x, shape = _channel_first(img, None)
        return _restore(remove_small_objects(x, self.min_size, self.connectivity), shape)


class FillHoles:
    """MONAI's ``FillHoles`` on a label map."""

    def __init__(self, applied_labels: Optional[Sequence[int]] = None, connectivity: Optional[int] = None) -> None:
        self.applied_labels = _check_applied(applied_labels)
        self.connectivity = connectivity

    def __call__(self, img: ArrayLike):
        x, shape = _channel_first(img, None)
        return _restore(fill_holes(x, self.applied_labels, self.connectivity), shape)


class MapLabels:
    """The reference's ``MapLabels``: ``lookup[img]`` with ``lookup[k] = mapping[k]`` and 0 elsewhere."""

    def __init__(self, mapping: Mapping[int, int], out_dtype=torch.int64) -> None:
        if not mapping:
            raise ValueError("mapping is empty")
        keys = [int(k) for k in mapping]
        if min(keys) < 0:
            raise ValueError(f"mapping keys must be >= 0, got {min(keys)}")
        if isinstance(out_dtype, (np.dtype, type)) or isinstance(out_dtype, str):
            out_dtype = torch.from_numpy(np.empty(0, np.dtype(out_dtype))).dtype
        if out_dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
            raise ValueError(f"out_dtype must be uint8, int16, int32 or int64, got {out_dtype}")
        info = torch.iinfo(out_dtype)
        self.lookup = torch.zeros(max(keys) + 1, dtype=torch.int64)
        for k, v in mapping.items():
            if not info.min <= int(v) <= info.max:
                raise ValueError(f"mapping value {v} does not fit {out_dtype}")
            self.lookup[int(k)] = int(v)
        self.out_dtype = out_dtype
        self._device_lookup: Dict[torch.device, torch.Tensor] = {}

    def __call__(self, img: ArrayLike):
        a = _raw(img)
        if not _is_integer(a):
            raise ValueError(f"MapLabels: label maps must hold integers, got {a.dtype}")
        if int(np.prod(tuple(a.shape), dtype=np.int64)) == 0:
            raise ValueError("MapLabels: empty input")
        dev = _require_gpu(_NEEDS_GPU)
        ops = _ops()
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        t = t.to(dev)
        if t.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
            t = t.to(torch.int64)
        t = t.contiguous()
        n = self.lookup.numel()
        if not (t.dtype == torch.uint8 and n >= 256):
            # the one host synchronisation: no index may leave the table
            lo, hi = torch.stack(torch.aminmax(t)).tolist()
            if lo < 0 or hi >= n:
                raise IndexError(f"MapLabels: values {lo} .. {hi} index a lookup table of {n} entries")
        if dev not in self._device_lookup:
            self._device_lookup[dev] = self.lookup.to(dev)
        return _wrap(img, ops.map_labels(t, self._device_lookup[dev], out_dtype=self.out_dtype))


class _Dict:
    """dictionary form: apply ``self.converter`` to every key"""

    def __init__(self, keys, allow_missing_keys: bool = False) -> None:
        self.keys = (keys,) if isinstance(keys, (str, bytes)) or not isinstance(keys, (list, tuple)) else tuple(keys)
        if not self.keys:
            raise ValueError("keys is empty")
        self.allow_missing_keys = allow_missing_keys

    def __call__(self, data: Mapping[Hashable, ArrayLike]) -> Dict[Hashable, ArrayLike]:
        d = dict(data)
        for key in self.keys:
            if key not in d:
                if self.allow_missing_keys:
                    continue
                raise KeyError(f"key {key!r} is missing and allow_missing_keys is False")
            d[key] = self.converter(d[key])
        return d


class KeepLargestConnectedComponentd(_Dict):
    def __init__(self, keys, applied_labels=None, is_onehot=None, independent=True, connectivity=None,
                 num_components=1, allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = KeepLargestConnectedComponent(applied_labels, is_onehot, independent, connectivity,
                                                       num_components)


class RemoveSmallObjectsd(_Dict):
    def __init__(self, keys, min_size: int = 64, connectivity: int = 1, independent_channels: bool = True,
                 allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = RemoveSmallObjects(min_size, connectivity, independent_channels)


class FillHolesd(_Dict):
    def __init__(self, keys, applied_labels=None, connectivity=None, allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = FillHoles(applied_labels, connectivity)


class MapLabelsd(_Dict):
    def __init__(self, mapping: Mapping[int, int], keys, allow_missing_keys: bool = False,
                 out_dtype=torch.int64) -> None:
        super().__init__(keys, allow_missing_keys)
        self.converter = MapLabels(mapping, out_dtype)
