"""Vertebra-landmark transforms on the MI355X (``csrc/landmarks.hip``).

Port of the reference's ``segmantic.detect.transforms`` on plain dicts (MONAI is not a dependency):
values are numpy arrays or torch tensors, geometry lives in ``<key>_<meta_key_postfix>`` dicts holding
``"affine"`` (4x4, voxel index (x, y, z) -> RAS mm) and ``"filename_or_obj"``.

Arrays here are ``[z, y, x]`` or ``[C, z, y, x]``; the reference sees MONAI arrays ``[C, x, y, z]`` with the
same affine.  Every index it reports -- landmark indices, argmax tie-breaks, bounding boxes -- is therefore
stated in (x, y, z) order, so a file gives the same numbers through both.

- ``LoadVert`` / ``SaveVert``: landmark JSON files ``{name: [x, y, z]}``.
- ``EmbedVert``: landmarks written into a zero volume of a reference image's geometry.
- ``VertHeatMap``: per-label Gaussian heatmaps from a label volume (two GPU passes, closed form).
- ``ExtractVertPosition``: one world-space point per heatmap channel (one GPU pass).
- ``BoundingBoxd``: the box of the positive voxels (one GPU pass).

Deviations from the reference, all where it crashes or is silently wrong: ``EmbedVert`` refuses a landmark
outside the volume, ``ExtractVertPosition`` refuses a channel holding NaN, ``VertHeatMap`` refuses one-hot
input and labels outside [0, K].  ``VertHeatMap`` smooths as the reference does (along y and z only) unless
``smooth_3d`` is set.
"""
from __future__ import annotations

import json
import logging
import os
import traceback
from pathlib import Path
from typing import Dict, Hashable, Iterable, Mapping, Sequence, Union

import numpy as np
import torch

from .. import ops

__all__ = ["LoadVert", "SaveVert", "EmbedVert", "ExtractVertPosition", "BoundingBoxd", "VertHeatMap",
           "gaussian_kernel_1d", "heatmap_sigma"]

DEFAULT_POST_FIX = "meta_dict"   # MONAI's PostFix.meta()
FILENAME_OR_OBJ = "filename_or_obj"
PathLike = Union[str, os.PathLike]


class MapTransform:
    """Dictionary transform over ``keys`` (one key or a sequence of keys)."""

    def __init__(self, keys, allow_missing_keys: bool = False) -> None:
        self.keys = tuple(keys) if isinstance(keys, (list, tuple)) else (keys,)
        self.allow_missing_keys = allow_missing_keys

    def key_iterator(self, d: Mapping) -> Iterable[Hashable]:
        for k in self.keys:
            if k in d:
                yield k
            elif not self.allow_missing_keys:
                raise KeyError(f"key {k!r} is not in the data and allow_missing_keys is False")


def _device_of(x) -> torch.device:
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _to_tensor(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x)))


def _affine(meta: Mapping):
    if meta and "affine" in meta:
        a = meta["affine"]
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        return np.asarray(a, dtype=np.float64)
    return None


# ------------------------------------------------------------------ landmark files
class LoadVert(MapTransform):
    """``d[key]``: path of a ``{name: [x, y, z]}`` JSON file -> ``{id: np.ndarray}``.  Names that all parse
    with ``int()`` are their own ids; otherwise the sorted names are numbered from 1.  ``d[key + "_" +
    meta_key_postfix] = {"filename_or_obj": path, "id_map": {name: id}}``."""

    def __init__(self, keys, meta_key_postfix: str = DEFAULT_POST_FIX) -> None:
        super().__init__(keys, False)
        self.meta_key_postfix = meta_key_postfix

    def __call__(self, data: Mapping) -> Dict:
        d = dict(data)
        for key in self.key_iterator(d):
            filename = d[key]
            points = json.loads(Path(filename).read_text())
            try:
                id_map = {n: int(n) for n in points}
            except ValueError:
                id_map = {n: i for i, n in enumerate(sorted(points), start=1)}
            d[key] = {id_map[n]: np.asarray(points[n]) for n in points}
            d[f"{key}_{self.meta_key_postfix}"] = {FILENAME_OR_OBJ: filename, "id_map": id_map}
        return d


def output_filename(subject: PathLike, output_dir: PathLike, postfix: str, ext: str, data_root_dir: PathLike = "",
                    separate_folder: bool = True) -> Path:
    """``output_dir/[<rel>/][<stem>/]<stem>_<postfix><ext>`` (MONAI's FolderLayout): ``stem`` drops one
    extension, two when the last is ``.gz``; ``rel`` is the subject's directory relative to
    ``data_root_dir`` when that is given."""
    filedir, name = os.path.split(os.fspath(subject))
    stem, e = os.path.splitext(name)
    if e == ".gz":
        stem, _ = os.path.splitext(stem)
    out = Path(output_dir)
    if data_root_dir and filedir:
        out = out / os.path.relpath(filedir, os.fspath(data_root_dir))
    if separate_folder:
        out = out / stem
    return out / (f"{stem}_{postfix}{ext}" if postfix else f"{stem}{ext}")


class SaveVert(MapTransform):
    """Writes ``d[key]`` (``{id: point}``) as ``{name: [x, y, z]}`` JSON, names through the meta dict's
    ``id_map`` (``str(id)`` without one), to :func:`output_filename` of the meta dict's
    ``filename_or_obj`` (or a running index).  Directories are created; write failures are collected and
    raised as one ``RuntimeError``."""

    def __init__(self, keys, meta_key_postfix: str = DEFAULT_POST_FIX, output_dir: PathLike = "./",
                 output_postfix: str = "trans", output_ext: str = ".json", data_root_dir: PathLike = "",
                 separate_folder: bool = True, print_log: bool = True) -> None:
        super().__init__(keys, False)
        self.meta_key_postfix = meta_key_postfix
        self.output_dir, self.output_postfix, self.output_ext = output_dir, output_postfix, output_ext
        self.data_root_dir, self.separate_folder = data_root_dir, separate_folder
        self.verbose = print_log
        self._data_index = 0

    def __call__(self, data: Mapping) -> Dict:
        err = []
        d = dict(data)
        log = logging.getLogger(self.__class__.__name__)
        for key in self.key_iterator(d):
            meta = d.get(f"{key}_{self.meta_key_postfix}") or {}
            subject = meta[FILENAME_OR_OBJ] if FILENAME_OR_OBJ in meta else str(self._data_index)
            self._data_index += 1
            filename = output_filename(subject, self.output_dir, self.output_postfix, self.output_ext,
                                       self.data_root_dir, self.separate_folder)
            verts = d[key]
            id_map = meta.get("id_map") or {str(i): i for i in verts}
            name_of = {v: k for k, v in id_map.items()}
            out = {name_of.get(i, str(i)): [float(c) for c in np.asarray(p).reshape(-1)] for i, p in verts.items()}
            try:
                filename.parent.mkdir(parents=True, exist_ok=True)
                filename.write_text(json.dumps(out))
                if self.verbose:
                    log.info(f"wrote {filename}")
            except Exception as e:
                err.append(traceback.format_exc())
                log.debug(e, exc_info=True)
                log.info(f"{self.__class__.__name__}: unable to write {filename}.")
        if err:
            raise RuntimeError(f"{self.__class__.__name__} cannot write vertices:\n" + "\n".join(err))
        return d


# ------------------------------------------------------------------ landmarks into a volume
class EmbedVert(MapTransform):
    """Writes each landmark's id into a zero volume of ``d[ref_key]``'s spatial shape and dtype (``[z, y,
    x]``, or ``[1, z, y, x]`` when the reference image is) at index ``np.round(inv(A[:3, :3]) @ (p -
    A[:3, 3]))`` (f64, half to even; an (x, y, z) index).  A landmark outside the volume raises
    ``ValueError``.  Host logic and one scatter: no kernel."""

    def __init__(self, keys, ref_key: str, meta_key_postfix: str = DEFAULT_POST_FIX) -> None:
        super().__init__(keys, False)
        self.ref_key = ref_key
        self.meta_key_postfix = meta_key_postfix

    @staticmethod
    def indices(vertices: Mapping, affine, spatial_zyx) -> Dict[int, tuple]:
        """{id: (x, y, z)} voxel index of every landmark; ValueError when one lies outside the volume"""
        a = np.eye(4) if affine is None else affine
        rot_inv = np.linalg.inv(a[:3, :3])
        t = a[:3, 3]
        ext = tuple(int(v) for v in spatial_zyx[::-1])
        out = {}
        for label, p in vertices.items():
            idx = np.round(rot_inv @ (np.asarray(p, dtype=np.float64) - t)).astype(np.int64)
            if idx.shape != (3,) or np.any(idx < 0) or np.any(idx >= ext):
                raise ValueError(f"EmbedVert: landmark {label} at {np.asarray(p).tolist()} has voxel index (x, y, z) "
                                 f"{idx.tolist()}, outside the volume of extent {list(ext)}")
            out[label] = tuple(int(v) for v in idx)
        return out

    def __call__(self, data: Mapping) -> Dict:
        d = dict(data)
        ref = d[self.ref_key]
        affine = _affine(d.get(f"{self.ref_key}_{self.meta_key_postfix}"))
        shape = tuple(ref.shape)
        if len(shape) == 4 and shape[0] == 1:
            spatial = shape[1:]
        elif len(shape) == 3:
            spatial = shape
        else:
            raise ValueError(f"EmbedVert: the reference image is [z, y, x] or [1, z, y, x], not {list(shape)}")
        for k in self.keys:
            pos = {}   # voxel -> id, later landmarks win as in sequential assignment
            for label, (x, y, z) in self.indices(d[k], affine, spatial).items():
                pos[(z, y, x)] = label
            if isinstance(ref, torch.Tensor):
                out = torch.zeros(shape, dtype=ref.dtype, device=ref.device)
                if pos:
                    zyx = torch.tensor(list(pos.keys()), dtype=torch.int64).t().to(ref.device)
                    out[(..., zyx[0], zyx[1], zyx[2])] = torch.tensor(list(pos.values())).to(ref.dtype).to(ref.device)
            else:
                out = np.zeros(shape, dtype=np.asarray(ref).dtype)
                for (z, y, x), label in pos.items():
                    out[..., z, y, x] = label
            d[k] = out
            meta_key = f"{k}_{self.meta_key_postfix}"
            d[meta_key] = {**(d.get(meta_key) or {}), "affine": np.eye(4) if affine is None else affine,
                           "original_channel_dim": "no_channel" if len(shape) == 3 else 0}
        return d


# ------------------------------------------------------------------ heatmap -> points
class ExtractVertPosition(MapTransform):
    """``d[key]``: f32 heatmap ``[C, z, y, x]`` -> ``{channel: np.ndarray(3)}`` for channels 1 .. C-1 whose
    max ``m`` is not below ``threshold`` (compared in f64): the first voxel equal to ``m`` in the reference's
    order -- the lexicographically smallest (x, y, z) -- mapped through the meta dict's affine in f64 (the raw
    index without one).  ``-0.0 == 0.0``.  A channel holding NaN raises ``ValueError``.  One GPU pass and one
    host synchronisation."""

    def __init__(self, keys, allow_missing_keys: bool = False, threshold: float = 0.5,
                 meta_key_postfix: str = DEFAULT_POST_FIX) -> None:
        super().__init__(keys, allow_missing_keys)
        self.threshold = threshold
        self.meta_key_postfix = meta_key_postfix

    def __call__(self, data: Mapping) -> Dict:
        d = dict(data)
        for key in self.key_iterator(d):
            img = _to_tensor(d[key])
            if img.dim() != 4:
                raise ValueError(f"ExtractVertPosition: {key!r} is a [C, z, y, x] heatmap, not {list(img.shape)}")
            vertices = {}
            c = int(img.shape[0])
            if c > 1:
                x = img[1:].to(device=_device_of(img), dtype=torch.float32).contiguous()
                keys, nan = ops.channel_argmax(x)
                keys_h = keys.cpu().numpy().view(np.uint64)
                bad = np.flatnonzero(nan.cpu().numpy())
                if bad.size:
                    raise ValueError(f"ExtractVertPosition: channel {int(bad[0]) + 1} of {key!r} holds NaN")
                vals, xyz = ops.decode_argmax_keys(keys_h, img.shape[1:])
                for i in range(c - 1):
                    if float(vals[i]) < float(self.threshold):
                        continue
                    vertices[i + 1] = xyz[i].astype(np.float64)
            a = _affine(d.get(f"{key}_{self.meta_key_postfix}"))
            if a is not None:
                vertices = {i: a[:3, :3] @ p + a[:3, 3] for i, p in vertices.items()}
            d[key] = vertices
        return d


class BoundingBoxd(MapTransform):
    """``d[result][bbox] = [[x0, y0, z0], [x1, y1, z1]]``, the half-open box of the voxels > 0 in any channel
    of ``d[key]`` (``[C, z, y, x]`` or ``[z, y, x]``), in (x, y, z) order as generate_spatial_bounding_box
    gives it for MONAI arrays.  NaN and -0.0 are not positive; an image without one gives six zeros."""

    def __init__(self, keys, result: str = "result", bbox: str = "bbox") -> None:
        super().__init__(keys)
        self.result = result
        self.bbox = bbox

    def __call__(self, data: Mapping) -> Dict:
        d = dict(data)
        for key in self.keys:
            x = _to_tensor(d[key])
            if x.dim() not in (3, 4):
                raise ValueError(f"BoundingBoxd: {key!r} is [C, z, y, x] or [z, y, x], not {list(x.shape)}")
            if x.dtype == torch.bool:
                x = x.to(torch.uint8)
            elif x.dtype not in (torch.float32, torch.uint8, torch.int16, torch.int32):
                x = (x > 0).to(torch.uint8)
            box = ops.positive_bbox(x.to(_device_of(x)).contiguous()).cpu().tolist()
            if d.get(self.result) is None:
                d[self.result] = dict()
            d[self.result][self.bbox] = [box[:3], box[3:]]
        return d


# ------------------------------------------------------------------ label volume -> heatmap
def heatmap_sigma(label: int) -> float:
    """sigma of label L's Gaussian, f32(1.6 + (L - 1) * 0.1) as the reference passes it to MONAI"""
    return float(np.float32(1.6 + (label - 1.0) * 0.1))


def gaussian_kernel_1d(sigma: float) -> torch.Tensor:
    """MONAI's gaussian_1d(sigma, truncated=4.0, approx="erf"), unnormalised, as f32: values at -tail .. tail,
    tail = int(max(4 sigma, 0.5) + 0.5).  sigma is taken as f32, the erf differences are formed in f64 and rounded
    once: formed in f32 they carry the absolute error of an erf near 1, which at sigma 27 (label 255) is 1 % of a
    tail value and 3e-5 gamma in the heatmap."""
    s = float(torch.as_tensor(sigma, dtype=torch.float))
    tail = int(max(s * 4.0, 0.5) + 0.5)
    x = torch.arange(-tail, tail + 1, dtype=torch.double)
    t = 0.70710678 / abs(s)
    return (0.5 * ((t * (x + 0.5)).erf() - (t * (x - 0.5)).erf())).clamp(min=0).float()


_PARAMS: Dict[tuple, torch.Tensor] = {}


def _heatmap_params(device: torch.device, k: int, gamma: float) -> torch.Tensor:
    """the kernel's parameter buffer (segmi.h, segmi_vert_heatmap), cached per (device, K, gamma)"""
    g = np.float32(gamma)
    key = (str(device), k, int(g.view(np.int32)))
    buf = _PARAMS.get(key)
    if buf is None:
        tables = [gaussian_kernel_1d(heatmap_sigma(lab)).numpy() for lab in range(1, k + 1)]
        stride = max([t.size for t in tables] + [1])
        words = np.zeros(ops.HEATMAP_TABLE_OFFSET + (k + 1) * stride, dtype=np.int32)
        words[0], words[1], words[2] = k, stride, g.view(np.int32)
        tab = words[ops.HEATMAP_TABLE_OFFSET:].view(np.float32)
        for lab, t in enumerate(tables, start=1):
            words[ops.HEATMAP_TAIL_OFFSET + lab] = t.size // 2
            tab[lab * stride:lab * stride + t.size] = t
        buf = torch.from_numpy(words).to(device)
        _PARAMS[key] = buf
    return buf


class VertHeatMap(MapTransform):
    """Label volume ``[1, z, y, x]`` or ``[z, y, x]`` -> f32 heatmap ``[K + 1, z, y, x]`` on the GPU, K =
    ``len(label_names)``.  Channel 0 and absent labels are 0.  For a present label L: centre c = floor(mean
    index) per axis (exact integer sums), P = k_L[z - c_z] k_L[y - c_y] on the slice x = c_x (the
    reference smooths its channel-less [X, Y, Z] slice, which MONAI reads as X channels of a 2-D image),
    or times k_L[x - c_x] everywhere when ``smooth_3d``; k_L = gaussian_kernel_1d(heatmap_sigma(L)), support
    clipped at the borders.  Then (P - min P) / (max P - min P) * gamma over the channel (a constant channel
    is 0).  Labels outside [0, K] and one-hot input raise ``ValueError``.  uint8 / int16 / int32 volumes are
    read in place; other integer dtypes are converted to int32 after a range check, floats truncated as the
    reference's ``torch.long`` conversion does.  Two GPU passes and one host synchronisation (the label
    range flag)."""

    def __init__(self, keys, gamma: float = 1000.0, label_names: Sequence[str] = (), smooth_3d: bool = False) -> None:
        super().__init__(keys)
        self.label_names = list(label_names)
        self.gamma = gamma
        self.smooth_3d = smooth_3d

    def __call__(self, data: Mapping) -> Dict:
        d = dict(data)
        for k in self.keys:
            d[k] = self.heatmap(d[k])
        return d

    def heatmap(self, labels) -> torch.Tensor:
        k = len(self.label_names)
        if k > ops.LANDMARK_MAX_LABELS:
            raise ValueError(f"VertHeatMap: at most {ops.LANDMARK_MAX_LABELS} labels, got {k}")
        x = _to_tensor(labels)
        if x.dim() == 4:
            if x.shape[0] != 1:
                raise ValueError(f"VertHeatMap: one-hot input ({x.shape[0]} channels) is not supported; "
                                 f"pass the label volume [1, z, y, x]")
            x = x[0]
        if x.dim() != 3 or min(x.shape) == 0:
            raise ValueError(f"VertHeatMap: a [1, z, y, x] or [z, y, x] label volume, not {list(np.shape(labels))}")
        if x.dtype not in (torch.uint8, torch.int16, torch.int32):
            if x.is_floating_point():
                x = x.to(torch.int64)
            lo, hi = int(x.min()), int(x.max())
            if lo < 0 or hi > k:
                raise ValueError(f"VertHeatMap: label values [{lo}, {hi}] outside [0, {k}]")
            x = x.to(torch.int32)
        dev = _device_of(x)
        x = x.to(dev).contiguous()
        sums, flag = ops.label_centroids(x, k)
        out = ops.vert_heatmap(_heatmap_params(dev, k, self.gamma), k, sums, flag, x.shape, self.smooth_3d)
        if int(flag.item()):
            raise ValueError(f"VertHeatMap: label values outside [0, {k}]")
        return out
