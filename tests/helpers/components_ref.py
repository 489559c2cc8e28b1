"""numpy oracle of ``segmantic_amd.seg.transforms``: connected components and the label clean-up
transforms, written directly from the definitions of DESIGN.md section 13 (and the module docstring).

* labelling: every voxel of a component starts with its own linear index and repeatedly takes the minimum
  over its equal-valued neighbours until nothing changes, so it ends with the index of the component's
  first voxel (raster order); fine up to about 48^3;
* canonical numbering: 1..n in raster order of the first voxels;
* the four transforms: a Python loop over components.
"""
from __future__ import annotations

import itertools

import numpy as np

_BIG = np.iinfo(np.int64).max


def offsets(ndim: int, connectivity: int):
    """neighbour offsets of scipy.ndimage.generate_binary_structure(ndim, connectivity), centre excluded"""
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim)
            if 0 < sum(1 for v in o if v) <= connectivity]


def _shifted(a: np.ndarray, off, fill):
    """b[p] = a[p + off], `fill` where p + off leaves the array"""
    out = np.full_like(a, fill)
    src, dst = [], []
    for o, n in zip(off, a.shape):
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n + min(-o, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def check_connectivity(ndim: int, connectivity):
    c = ndim if connectivity is None else connectivity
    if not 1 <= c <= ndim:
        raise ValueError("connectivity")
    return c


def roots(labels: np.ndarray, connectivity=None, background=0) -> np.ndarray:
    """int64 array: linear index of the first voxel of each voxel's component, -1 outside every component"""
    labels = np.asarray(labels)
    c = check_connectivity(labels.ndim, connectivity)
    active = np.ones(labels.shape, bool) if background is None else labels != background
    idx = np.arange(labels.size, dtype=np.int64).reshape(labels.shape)
    cur = np.where(active, idx, _BIG)
    lab = labels.astype(np.int64)
    offs = offsets(labels.ndim, c)
    same = []
    for o in offs:
        nb_lab = _shifted(lab, o, 0)
        nb_act = _shifted(active, o, False)
        same.append(active & nb_act & (nb_lab == lab))
    while True:
        new = cur
        for o, s in zip(offs, same):
            new = np.where(s, np.minimum(new, _shifted(cur, o, _BIG)), new)
        if np.array_equal(new, cur):
            break
        cur = new
        # a voxel's value is the index of a voxel of its own component: taking that voxel's value as well
        # (pointer jumping) changes nothing at the fixed point and shortens long paths
        flat = cur.ravel()
        hop = np.where(flat != _BIG, flat[np.where(flat != _BIG, flat, 0)], _BIG)
        cur = np.minimum(flat, hop).reshape(cur.shape)
    return np.where(active, cur, -1)


def canonical(root: np.ndarray):
    """(components int32 numbered 1..n in raster order of the first voxels, n)"""
    flat = root.ravel()
    first = np.flatnonzero(flat == np.arange(flat.size))
    lut = np.zeros(flat.size + 1, np.int64)
    lut[first] = np.arange(1, first.size + 1)
    return lut[flat].reshape(root.shape).astype(np.int32), int(first.size)


def renumber_canonical(comp: np.ndarray) -> np.ndarray:
    """any component map (0 = none) renumbered canonically"""
    flat = np.asarray(comp).ravel()
    vals, first = np.unique(flat, return_index=True)
    keep = vals != 0
    vals, first = vals[keep], first[keep]
    out = np.zeros(flat.shape, np.int32)
    for k, v in enumerate(vals[np.argsort(first)]):
        out[flat == v] = k + 1
    return out.reshape(np.shape(comp))


def connected_components(labels, connectivity=None, background=0):
    return canonical(roots(labels, connectivity, background))


def component_sizes(labels, connectivity=None) -> np.ndarray:
    comp, n = connected_components(labels, connectivity)
    return np.bincount(comp.ravel(), minlength=n + 1)[1:].astype(np.int64)


def _components(root: np.ndarray):
    """[(first voxel, size)] of every component, in raster order of the first voxels"""
    flat = root.ravel()
    first, counts = np.unique(flat[flat >= 0], return_counts=True)
    return list(zip(first.tolist(), counts.tolist()))


def keep_largest_connected_component(labels, applied_labels=None, independent=True, connectivity=None,
                                     num_components=1):
    labels = np.asarray(labels)
    out = labels.copy()
    flat_lab = labels.ravel()
    if applied_labels is None:
        applied = sorted(int(v) for v in np.unique(labels) if v != 0)
    else:
        applied = sorted({int(v) for v in applied_labels if int(v) != 0})
    if independent:
        root = roots(labels, connectivity)
        for cls in applied:
            comps = [(f, s) for f, s in _components(root) if flat_lab[f] == cls]
            comps.sort(key=lambda fs: (-fs[1], fs[0]))      # size descending, first voxel ascending
            kept = {f for f, _ in comps[:num_components]}
            out[(labels == cls) & ~np.isin(root, list(kept))] = 0
    else:
        mask = np.isin(labels, applied)
        root = roots(mask.astype(np.uint8), connectivity)
        comps = sorted(_components(root), key=lambda fs: (-fs[1], fs[0]))
        kept = {f for f, _ in comps[:num_components]}
        out[mask & ~np.isin(root, list(kept))] = 0
    return out


def remove_small_objects(labels, min_size=64, connectivity=1):
    labels = np.asarray(labels)
    out = labels.copy()
    root = roots(labels, connectivity)
    for f, s in _components(root):
        if s < min_size:
            out[root == f] = 0
    return out


def fill_holes(labels, applied_labels=None, connectivity=None):
    labels = np.asarray(labels)
    c = check_connectivity(labels.ndim, connectivity)
    out = labels.copy()
    root = roots(labels, c, background=None)
    border = np.zeros(labels.shape, bool)
    for ax in range(labels.ndim):
        sl = [slice(None)] * labels.ndim
        sl[ax] = 0
        border[tuple(sl)] = True
        sl[ax] = -1
        border[tuple(sl)] = True
    lab = labels.astype(np.int64)
    flat_lab = labels.ravel()
    for f, _ in _components(root):
        if flat_lab[f] != 0:
            continue
        region = root == f
        if (region & border).any():
            continue
        around = set()
        for o in offsets(labels.ndim, c):
            # values of the voxels at p + o for p in the region
            around |= set(np.unique(_shifted(lab, o, 0)[region]).tolist())
        around.discard(0)
        if len(around) != 1:
            continue
        value = around.pop()
        if applied_labels is None or value in {int(v) for v in applied_labels}:
            out[region] = value
    return out


def map_labels(mapping, img, dtype=np.int64):
    """the reference's MapLabels: lookup of length max(mapping) + 1, unmapped entries 0, lookup[img]"""
    lookup = np.zeros(max(mapping) + 1, np.int64)
    for k, v in mapping.items():
        lookup[k] = v
    return lookup[np.asarray(img).astype(np.int64)].astype(dtype)
