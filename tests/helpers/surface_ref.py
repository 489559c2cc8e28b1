"""numpy restatement of the discrete-surface-nets contract of ``segmantic_amd/image/surfaces.py`` (DESIGN.md
section 14).  Float32 positions exactly as specified, relaxation in float64, area and volume with ``math.fsum``."""
from __future__ import annotations

import math
from collections import Counter

import numpy as np


def _corners(labels: np.ndarray, c: int):
    """corner[a][b][e] = P[k+a, j+b, i+e] over all cells, each of shape (d+1, h+1, w+1)"""
    d, h, w = labels.shape
    P = np.pad(labels == c, 1)
    return [[[P[a:a + d + 1, b:b + h + 1, e:e + w + 1] for e in (0, 1)] for b in (0, 1)] for a in (0, 1)]


def surface_nets(labels: np.ndarray, c: int, iterations: int = 0, relaxation: float = 0.5):
    """-> dict(cells int [V, 3] (x, y, z), offsets (float32 for T = 0, float64 after relaxation) [V, 3],
    index float32 / float64 [V, 3] (x, y, z), faces int32 [F, 3])"""
    C = _corners(labels, c)
    total = sum(C[a][b][e].astype(np.int32) for a in (0, 1) for b in (0, 1) for e in (0, 1))
    active = (total > 0) & (total < 8)
    nv = int(active.sum())
    vid = np.full(active.shape, -1, np.int64)
    vid[active] = np.arange(nv)                     # boolean indexing walks in raster order
    # doubled midpoints of the crossing edges: integer sums (x, y, z) and their number
    s = np.zeros(active.shape + (3,), np.int32)
    n = np.zeros(active.shape, np.int32)
    for a in (0, 1):
        for b in (0, 1):
            for cross, mid in ((C[a][b][0] != C[a][b][1], (1, 2 * b, 2 * a)),       # x-edge at y = b, z = a
                               (C[a][0][b] != C[a][1][b], (2 * b, 1, 2 * a)),       # y-edge at x = b, z = a
                               (C[0][a][b] != C[1][a][b], (2 * b, 2 * a, 1))):      # z-edge at x = b, y = a
                s += cross[..., None].astype(np.int32) * np.asarray(mid, np.int32)
                n += cross
    kz, jy, ix = np.nonzero(active)
    cells = np.stack([ix, jy, kz], 1)
    offs = s[active].astype(np.float32) / (2 * n[active]).astype(np.float32)[:, None]
    # faces: the edge from the cell's lowest corner along x / y / z
    c0 = C[0][0][0]
    keys, quads = [], []
    raster = np.arange(active.size).reshape(active.shape)

    def nb(dk, dj, di):
        """vid of the cell at (k + dk, j + dj, i + di) for every cell (-1 outside)"""
        out = np.full(active.shape, -1, np.int64)
        zs = slice(max(-dk, 0), active.shape[0] - max(dk, 0))
        ys = slice(max(-dj, 0), active.shape[1] - max(dj, 0))
        xs = slice(max(-di, 0), active.shape[2] - max(di, 0))
        zt = slice(max(dk, 0), active.shape[0] + min(dk, 0))
        yt = slice(max(dj, 0), active.shape[1] + min(dj, 0))
        xt = slice(max(di, 0), active.shape[2] + min(di, 0))
        out[zs, ys, xs] = vid[zt, yt, xt]
        return out

    cycles = (
        (C[0][0][1], [(-1, -1, 0), (-1, 0, 0), (0, 0, 0), (0, -1, 0)]),    # x-edge: (y-,z-) (y+,z-) (y+,z+) (y-,z+)
        (C[0][1][0], [(-1, 0, -1), (0, 0, -1), (0, 0, 0), (-1, 0, 0)]),    # y-edge: (z-,x-) (z+,x-) (z+,x+) (z-,x+)
        (C[1][0][0], [(0, -1, -1), (0, -1, 0), (0, 0, 0), (0, 0, -1)]),    # z-edge: (x-,y-) (x+,y-) (x+,y+) (x-,y+)
    )
    for axis, (upper, cyc) in enumerate(cycles):
        cross = c0 != upper
        if not cross.any():
            continue
        q = np.stack([nb(*o)[cross] for o in cyc], 1)
        rev = ~c0[cross]
        q[rev] = q[rev][:, ::-1]
        keys.append(raster[cross] * 3 + axis)
        quads.append(q)
    if keys:
        keys = np.concatenate(keys)
        quads = np.concatenate(quads)[np.argsort(keys, kind="stable")]
        assert (quads >= 0).all(), "every cell around a crossing edge is active"
        faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    if iterations > 0:
        # neighbours through mixed cell faces, in the order -x +x -y +y -z +z
        def mixed(sel):
            t = sum(C[a][b][e].astype(np.int32) for (a, b, e) in sel)
            return (t > 0) & (t < 4)
        face_sel = [[(a, b, 0) for a in (0, 1) for b in (0, 1)], [(a, b, 1) for a in (0, 1) for b in (0, 1)],
                    [(a, 0, e) for a in (0, 1) for e in (0, 1)], [(a, 1, e) for a in (0, 1) for e in (0, 1)],
                    [(0, b, e) for b in (0, 1) for e in (0, 1)], [(1, b, e) for b in (0, 1) for e in (0, 1)]]
        steps = [(0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)]
        nbr = np.stack([np.where(mixed(fs)[active], nb(*st)[active], -1) for fs, st in zip(face_sel, steps)], 1)
        assert ((nbr >= 0).sum(1) >= 3).all()
        e = np.asarray([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.float64)
        o = offs.astype(np.float64)
        for _ in range(iterations):
            acc = np.zeros_like(o)
            for q in range(6):
                has = nbr[:, q] >= 0
                acc[has] += o[nbr[has, q]] + e[q]
            m = acc / (nbr >= 0).sum(1)[:, None]
            o = np.clip(o + relaxation * (m - o), 0.0, 1.0)
        offs = o
        index = (cells - 1).astype(np.float64) + offs
    else:
        index = (cells - 1).astype(np.float32) + offs
    return {"cells": cells, "offsets": offs, "index": index, "faces": faces}


def physical(index: np.ndarray, spacing, origin, direction) -> np.ndarray:
    """origin + Direction (spacing o index) in float64 (not rounded)"""
    sp = np.asarray(spacing, np.float64)
    D = np.asarray(direction, np.float64).reshape(3, 3)
    return np.asarray(origin, np.float64) + (index.astype(np.float64) * sp) @ D.T


def measure_terms(vertices: np.ndarray, faces: np.ndarray):
    """per-triangle (2 x area, 6 x signed volume) in float64, the operations in the kernel's order"""
    p = vertices.astype(np.float64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    vol = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2])) \
        + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
    u, w = b - a, c - a
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return np.sqrt((nx * nx + ny * ny) + nz * nz), vol


def measures(vertices: np.ndarray, faces: np.ndarray):
    """(area, volume, sum |area terms| / 2, sum |volume terms| / 6) with math.fsum"""
    ar, vo = measure_terms(vertices, faces)
    return (math.fsum(ar) / 2.0, math.fsum(vo) / 6.0, math.fsum(np.abs(ar)) / 2.0, math.fsum(np.abs(vo)) / 6.0)


def directed_edge_balance(faces: np.ndarray) -> bool:
    """every directed edge a->b occurs exactly as often as b->a"""
    cnt = Counter()
    for i, j in ((0, 1), (1, 2), (2, 0)):
        for a, b in zip(faces[:, i].tolist(), faces[:, j].tolist()):
            cnt[(a, b)] += 1
    return all(cnt[(b, a)] == n for (a, b), n in cnt.items())


def euler_characteristic(n_vertices: int, faces: np.ndarray) -> int:
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    return n_vertices - len(np.unique(e, axis=0)) + len(faces)


# ------------------------------------------------------------------ test volumes
def ball(n: int = 24, r: float = 8.3) -> np.ndarray:
    z, y, x = np.ogrid[:n, :n, :n]
    c = (n - 1) / 2
    return (((z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2) <= r * r).astype(np.uint8)


def torus(n: int = 32, R: float = 9.0, r: float = 3.6) -> np.ndarray:
    z, y, x = np.ogrid[:n, :n, :n]
    c = (n - 1) / 2
    q = np.sqrt((y - c) ** 2 + (x - c) ** 2) - R
    return ((q * q + (z - c) ** 2) <= r * r).astype(np.uint8)


def noise(shape, classes: int, density: float, seed: int, dtype=np.uint8) -> np.ndarray:
    """labels 1 .. classes on a `density` share of the voxels"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, classes + 1, size=shape)
    lab[rng.random(shape) >= density] = 0
    return lab.astype(dtype)
