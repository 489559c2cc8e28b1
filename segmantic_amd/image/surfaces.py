"""Label surfaces on the MI355X: one closed triangle mesh per tissue of a label volume, written as binary PLY
(the reference's ``scripts/visualize_label_surfaces.py``, which hands the work to VTK's
``vtkDiscreteFlyingEdges3D``).  The meshes are computed by the HIP kernels of ``csrc/surfaces.hip``; there is no
CPU fallback: with no GPU :func:`extract_surfaces` raises ``RuntimeError`` (after validating its input).

Contract: discrete surface nets
-------------------------------
VTK is not part of this project and its flying-edges case table cannot be checked here, so the words below are
the specification; ``tests/helpers/surface_ref.py`` restates them in numpy and the tests compare bit for bit.

* **Input**: a 3-D label volume ``L[z, y, x]`` (``uint8`` / ``int16`` / ``int32`` are read in place, ``bool`` is
  read as ``uint8`` and other integer types as ``int32``), never modified.  2-D or non-integer input raises
  ``ValueError``; label values must lie in ``0..65535`` (``ValueError`` otherwise, one range check as in
  ``seg/transforms.py``).
* **Padded lattice**: for one label ``c``, ``P`` is ``L == c`` padded by one layer of ``False`` on every side, so
  an object that touches the border gets a closed surface.  Lattice point ``(k, j, i)`` is voxel
  ``(k-1, j-1, i-1)``.
* **Cells**: one per 2x2x2 block of lattice points, cell ``(k, j, i)`` with ``0 <= k <= d`` etc. and corners
  ``P[k..k+1, j..j+1, i..i+1]``.  ``(d+1)(h+1)(w+1)`` must stay below ``2^31`` (``ValueError``).  A cell is
  *active* when its corners are neither all set nor all clear.
* **Vertices**: one per active cell, numbered ``0..V-1`` in raster order (z, y, x) of the cells.  The position is
  the mean of the midpoints of the cell's *crossing* edges (cell edges whose ends differ), held as a cell-local
  offset ``o = float32(s) / float32(2 n)`` in ``[0, 1]^3`` (``s``: integer sum of the doubled midpoints, ``n``:
  number of crossing edges; one IEEE division per component).  Index coordinate (voxel centres at integers)
  ``= float32(cell - 1) + o``.
* **Faces**: one quad per crossing lattice edge, joining the four cells around the edge, split into two
  triangles.  For an x-edge whose lower end is set the cycle is the cells at ``(y-,z-), (y+,z-), (y+,z+),
  (y-,z+)``; y-edge: ``(z-,x-), (z+,x-), (z+,x+), (z-,x+)``; z-edge: ``(x-,y-), (x+,y-), (x+,y+), (x-,y+)``;
  when the upper end is the set one the cycle is read backwards (``q3, q2, q1, q0``).  The normal therefore
  points from ``c`` to not-``c``.  Split: ``(q0, q1, q2), (q0, q2, q3)``.  Order: by the raster index of the cell
  whose lowest corner is the edge's lower end, then x-, y-, z-edge.  ``faces`` is ``int32 [F, 3]`` with
  ``F = 2 x`` the number of crossing edges.
* **Relaxation** (``smooth_iterations = T >= 0``, ``relaxation = lambda in [0, 1]``): Jacobi sweeps on the local
  offsets.  A vertex's neighbours are the face-adjacent active cells whose shared cell face is mixed (3 to 6 of
  them); ``m`` is the mean of ``o_u + e_uv`` (``e_uv``: the unit step to the neighbour) summed in the order -x,
  +x, -y, +y, -z, +z, and ``o_v' = clamp(o_v + lambda (m - o_v), 0, 1)``.  The clamp keeps every vertex inside its
  cell, so the surface never leaves the band of mixed cells and the surfaces of different labels cannot cross.
* **Physical coordinates**: ``p_xyz = origin + Direction (spacing o index_xyz)``, evaluated in float64 from the
  float32 index coordinate and rounded once to float32.  ``vertices`` is ``float32 [V, 3]`` in ``(x, y, z)``.
* **Measures**: surface area and enclosed volume ``1/6 sum p0 . (p1 x p2)`` of the emitted mesh in physical units,
  float64 sums in a fixed order (repeated calls are bit-identical).

Consequences: every directed mesh edge ``a->b`` occurs exactly as often as ``b->a`` (closed, consistently
oriented) on any input; at ambiguous configurations (two voxels that touch along an edge or at a corner) an edge is
used twice in each direction: surface nets are non-manifold there by construction, and this is not "fixed".
``V - E + F`` is 2 for a ball or a full volume and 0 for a torus; the signed volume is positive and differs from
the voxel count times the voxel volume by at most ``V`` voxel volumes.

Deviations from the reference script: surface nets instead of flying edges (a vertex per mixed cell, not per
crossing edge); the edge-collapse decimation below instead of ``vtkDecimatePro`` (off by default); the default
selection is every label present in ``1..max`` (the reference's ``range(1, max_label)`` drops the largest); a selected label
that is absent yields an empty mesh and no file.

Contract: decimation (``decimate = r``, :func:`decimate_surface`)
-----------------------------------------------------------------
``vtkDecimatePro`` is a sequential priority-queue algorithm with no defined output; this is a round-based edge
collapse over independent sets, parallel and deterministic.  ``tests/helpers/decimate_ref.py`` restates it in
float64 Python and the device produces the same integer mesh.  Input: vertices float32 ``[V, 3]`` and faces int32
``[F, 3]``, consistently oriented, ``V < 2^23`` per mesh (``ValueError`` above: the claim key keeps 23 bits for the
vertex).  Positions never change, output vertices are a subset of the input's, all arithmetic is float64 on the
float32 positions and no product is contracted into an FMA.  ``target = ceil((1 - r) F)``; rounds ``t = 0, 1, ...``
run while live faces ``> target``, ``t < max_rounds`` and the previous round collapsed something.

1. **Stars**: a live vertex's live incident faces (one entry per face slot), ascending; ``N(u)`` the other
   vertices of those faces; the valence of ``u`` is the number of entries.
2. **Regular** ``u``: the star is a single closed fan of 3 .. 32 faces: every neighbour occurs exactly once as
   successor and once as predecessor of ``u`` in its faces, no face holds ``u`` twice, and following successors
   visits all of them in one cycle.  Everything else is *pinned* (the doubled edges of surface nets, open borders,
   very high valence): never removed, never the receiver of a collapse.
3. **Quadrics**, once, before round 0: ``Q_u = sum`` over ``u``'s faces ``(a, b, c)``, ascending from 0.0, of
   ``p p^T``, ``p = (n, -((n_x a_x + n_y a_y) + n_z a_z))``, ``n = (b - a) x (c - a)`` with
   ``n_x = u_y w_z - u_z w_y`` etc. (``u = b - a``, ``w = c - a``): no square root, the weight is the squared
   doubled area.  Ten coefficients ``xx xy xz xw yy yz yw zz zw ww``.  A collapse ``u -> v`` sets ``Q_v += Q_u``.
4. **Candidates**: for a regular ``u`` a neighbour ``v`` is admissible when ``v`` is regular; exactly two live
   faces hold both; the valences of ``u`` and ``v`` sum to at least 7 (``v`` keeps 3 faces or more: the valence of a
   pinned shared vertex counts the faces of every sheet that meets there, so the next rule alone would let a
   sheet shrink to two triangles on the same three vertices); ``N(u)`` and ``N(v)`` share exactly two vertices
   (link condition); both of them have valence >= 4 (a tetrahedron is irreducible); and every face of ``u``
   without ``v`` keeps ``(n0_x n1_x + n0_y n1_y) + n0_z n1_z > 0`` between its normal and its normal with ``v`` in
   ``u``'s slot.  With ``q = Q_u + Q_v`` (coefficient by coefficient) and ``v = (x, y, z)``:
   ``r0 = ((q_xx x + q_xy y) + q_xz z) + q_xw``, ``r1``, ``r2`` likewise from the rows of y and z,
   ``r3 = ((q_xw x + q_yw y) + q_zw z) + q_ww``, ``cost = ((x r0 + y r1) + z r2) + r3``, and a cost that is not
   ``> 0`` counts as 0.  ``u``'s choice is the admissible ``v`` with the smallest
   ``(float32(cost) bits >> 23, v)``.
5. **Independent set**: ``key(u) = bucket << 55 | mix32(u, t) << 23 | u`` (``u`` numbered within its mesh) with
   ``mix32(u, t)``: ``x = u * 0x9E3779B1 + t * 0x85EBCA77 + 0x165667B1``; ``x ^= x >> 15``; ``x *= 0x2C1B3C6D``;
   ``x ^= x >> 12``; ``x *= 0x297A2D39``; ``x ^= x >> 15`` in 32-bit unsigned arithmetic.  Every candidate writes
   ``min(key)`` into the slots of ``u`` and all ``N(u)``; ``u`` collapses when all of them hold its key.  Two
   winners have disjoint closed 1-rings, so the result does not depend on the order of execution.
6. **Apply**: faces with ``u`` and ``v`` die, ``u``'s other faces get ``v`` in ``u``'s slot, ``u`` dies.

Output: live vertices and faces in their original relative order, renumbered.  ``V - E + F``, the number of
components and the balance of directed edges are kept, no face has a repeated vertex and no two faces share
their three vertices.  The labels of a volume form one batch: every launch serves all of them, a mesh at or under
its target yields no candidate, and one device-to-host copy per round carries the live-face counts.

Arrays come back where the input lived: numpy in -> numpy out, tensors in -> tensors on the input's device.
Host synchronisations per volume: the range check, the label boxes and the vertex / face totals, whatever the
number of labels; with decimation, one more per round and one for the output totals.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

# the module, not its names: image/__init__.py imports this file, possibly while _arrays is still importing Image
from .. import _arrays
from .processing import Image

MAX_LABEL = 65535
MAX_CELLS = 2 ** 31
_NEEDS_GPU = "segmantic_amd.image.surfaces needs an MI355X"


@dataclass
class Surface:
    """``vertices`` float32 [V, 3] (x, y, z), ``faces`` int32 [F, 3], ``area`` and ``volume`` in physical units."""

    vertices: Union[np.ndarray, torch.Tensor]
    faces: Union[np.ndarray, torch.Tensor]
    area: float = 0.0
    volume: float = 0.0

    def __eq__(self, other) -> bool:
        if not isinstance(other, Surface):
            return NotImplemented
        return (np.array_equal(_host(self.vertices), _host(other.vertices))
                and np.array_equal(_host(self.faces), _host(other.faces))
                and self.area == other.area and self.volume == other.volume)


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def surface_file_name(label: int, tissues: Optional[Dict[int, str]] = None) -> str:
    """``<tissue name>.ply`` when the tissue list names the label, otherwise ``label_{label:03d}.ply``"""
    name = tissues[label] if tissues and label in tissues else f"label_{label:03d}"
    return f"{name}.ply"


# ------------------------------------------------------------------ validation
def _check_volume(labels: _arrays.ArrayLike):
    """checks that need neither a copy nor the device -> the raw array"""
    a = _arrays._raw(labels)
    shape = tuple(int(s) for s in a.shape)
    if len(shape) != 3:
        raise ValueError(f"label surfaces need a 3-D [z, y, x] label volume, got shape {shape}")
    if not _arrays._is_integer(a):
        raise ValueError(f"label volumes must hold integers, got {a.dtype}")
    if min(shape) == 0:
        raise ValueError(f"empty label volume of shape {shape}")
    if (shape[0] + 1) * (shape[1] + 1) * (shape[2] + 1) >= MAX_CELLS:
        raise ValueError(f"(d+1)(h+1)(w+1) must stay below 2^31, got shape {shape}")
    return a


def _value_range(a):
    """(min, max) of the volume where it lives: the one range check"""
    if isinstance(a, np.ndarray):
        return int(a.min()), int(a.max())
    if a.dtype not in _arrays._IN_PLACE and a.dtype != torch.int64:
        a = a.to(torch.int64)          # bool, int8 and the unsigned wide types, which aminmax does not take
    lo, hi = torch.stack(torch.aminmax(a)).tolist()
    return int(lo), int(hi)


def _check_selected(selected) -> Optional[list]:
    if selected is None:
        return None
    if isinstance(selected, (int, np.integer)):
        selected = [selected]
    out = sorted({int(v) for v in selected})
    if not out:
        return None
    if out[0] < 1 or out[-1] > MAX_LABEL:
        raise ValueError(f"selected labels must lie in 1 .. {MAX_LABEL}, got {out}")
    return out


def _geometry(labels: _arrays.ArrayLike, spacing, origin, direction):
    if isinstance(labels, Image):
        spacing = labels.spacing if spacing is None else spacing
        origin = labels.origin if origin is None else origin
        direction = labels.direction if direction is None else direction
    sp = np.asarray([1.0] * 3 if spacing is None else spacing, np.float64).reshape(-1)
    og = np.asarray([0.0] * 3 if origin is None else origin, np.float64).reshape(-1)
    dr = np.asarray(np.eye(3) if direction is None else direction, np.float64).reshape(-1)
    if sp.size != 3 or og.size != 3 or dr.size != 9:
        raise ValueError("spacing and origin are (x, y, z) triples and direction a row-major 3 x 3 matrix")
    return sp, og, dr


# ------------------------------------------------------------------ extraction
def _check_decimate(reduction, max_rounds) -> float:
    if isinstance(reduction, bool) or not isinstance(reduction, (int, float, np.integer, np.floating)):
        raise ValueError(f"the decimation reduction must be a number in [0, 1), got {reduction!r}")
    r = float(reduction)
    if not 0.0 <= r < 1.0:                              # NaN fails both comparisons
        raise ValueError(f"the decimation reduction must lie in [0, 1), got {reduction!r}")
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or int(max_rounds) < 1:
        raise ValueError(f"the decimation round limit must be an integer >= 1, got {max_rounds!r}")
    return r


def extract_surfaces(labels: _arrays.ArrayLike, selected: Optional[Sequence[int]] = None, spacing=None, origin=None,
                     direction=None, smooth_iterations: int = 0, relaxation: float = 0.5, decimate: float = 0.0,
                     decimate_max_rounds: int = 128) -> Dict[int, Surface]:
    """One discrete-surface-nets mesh per label (see the module docstring).  ``selected`` defaults to every label
    present in ``1..max``; a selected label that is absent maps to an empty :class:`Surface`.  ``decimate = r`` in
    ``(0, 1)`` decimates every mesh towards ``ceil((1 - r) F)`` faces after relaxation and the physical transform
    (0.8 is the reference's setting); with 0 the decimation code is not entered."""
    a = _check_volume(labels)
    reduction = _check_decimate(decimate, decimate_max_rounds)
    sel = _check_selected(selected)
    sp, og, dr = _geometry(labels, spacing, origin, direction)
    if isinstance(smooth_iterations, bool) or int(smooth_iterations) != smooth_iterations or int(smooth_iterations) < 0:
        raise ValueError(f"smooth_iterations must be an integer >= 0, got {smooth_iterations!r}")
    if not 0.0 <= float(relaxation) <= 1.0:
        raise ValueError(f"relaxation must lie in [0, 1], got {relaxation!r}")
    lo, hi = _value_range(a)
    if lo < 0 or hi > MAX_LABEL:
        raise ValueError(f"label values must lie in 0 .. {MAX_LABEL}, the volume holds {lo} .. {hi}")
    dev = _arrays._require_gpu(_NEEDS_GPU, near=a)
    from .. import ops

    t = _arrays._to_device(a, dev)

    def empty() -> Surface:
        return Surface(_arrays._wrap(a, torch.empty((0, 3), dtype=torch.float32, device=dev)),
                       _arrays._wrap(a, torch.empty((0, 3), dtype=torch.int32, device=dev)), 0.0, 0.0)

    todo = list(range(1, hi + 1)) if sel is None else sel
    if not todo:
        return {}
    boxes = ops.surface_boxes(t, todo).cpu().numpy()                       # host synchronisation: boxes
    present = boxes[:, 1] > boxes[:, 0]
    if sel is None:
        todo = [c for c, p in zip(todo, present) if p]
        boxes = np.ascontiguousarray(boxes[present])
    if not todo:
        return {}
    ws = torch.empty(ops.surface_workspace_bytes(t.shape, todo, boxes), dtype=torch.uint8, device=dev)
    starts_dev = ops.surface_count(t, todo, boxes, ws)
    starts = starts_dev.cpu().numpy()                                      # host synchronisation: totals
    if starts[-1, 0]:
        raise ValueError("the selected labels' meshes hold 2^31 vertices or faces or more")
    nv, nf = int(starts[-2, 0]), int(starts[-2, 1])
    T = int(smooth_iterations)
    offs, cells, nbr, faces = ops.surface_emit(t, todo, boxes, ws, nv, nf, with_neighbours=T > 0)
    verts = ops.surface_relax(offs, cells, nbr, T, float(relaxation), og, dr, sp)
    if reduction > 0.0 and nf > 0:
        verts, faces, _, starts_dev, starts = ops.decimate_meshes(verts, faces, starts_dev, starts, reduction,
                                                                  int(decimate_max_rounds))
    measures = ops.surface_measure(verts, faces, starts_dev).cpu().numpy()
    verts, faces = _arrays._wrap(a, verts), _arrays._wrap(a, faces)
    out: Dict[int, Surface] = {}
    for l, c in enumerate(todo):
        v0, f0, v1, f1 = (int(x) for x in (starts[l, 0], starts[l, 1], starts[l + 1, 0], starts[l + 1, 1]))
        if v1 == v0:
            out[c] = empty()
        else:
            out[c] = Surface(verts[v0:v1], faces[f0:f1], float(measures[l, 0]), float(measures[l, 1]))
    return out


def decimate_surface(surface: Surface, reduction: float, max_rounds: int = 128) -> Surface:
    """Decimate any :class:`Surface` (for example one from :func:`read_ply`) as the module docstring defines;
    ``area`` and ``volume`` are those of the decimated mesh.  Tensors on the device stay there, numpy input gives
    numpy output; ``reduction = 0`` returns ``surface`` itself."""
    r = _check_decimate(reduction, max_rounds)
    v, f = surface.vertices, surface.faces
    for x in (v, f):
        if not isinstance(x, (np.ndarray, torch.Tensor)):
            raise TypeError(f"expected numpy arrays or torch tensors, not {type(x).__name__}")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"a surface holds vertices [V, 3] and faces [F, 3], got {tuple(v.shape)} and {tuple(f.shape)}")
    integer = not (f.is_floating_point() or f.is_complex()) if isinstance(f, torch.Tensor) else f.dtype.kind in "iu"
    if not integer:
        raise ValueError(f"faces must hold integers, got {f.dtype}")
    nv, nf = int(v.shape[0]), int(f.shape[0])
    if nf:
        lo, hi = (int(f.min()), int(f.max()))            # on the host for host arrays
        if lo < 0 or hi >= nv:
            raise ValueError(f"faces index vertices {lo} .. {hi}, the surface has {nv}")
    if nv >= 2 ** 23:
        raise ValueError(f"decimation takes meshes of fewer than 2^23 vertices, got {nv}")
    if r == 0.0 or nf == 0:
        return surface
    dev = _arrays._require_gpu(_NEEDS_GPU, near=v if isinstance(v, torch.Tensor) else f)
    from .. import ops

    vt = _arrays._tensor(v).to(dev, torch.float32).contiguous()
    ft = _arrays._tensor(f).to(dev, torch.int32).contiguous()
    starts = np.asarray([[0, 0], [nv, nf], [0, 0]], np.int32)
    ov, of, _, out_starts, _ = ops.decimate_meshes(vt, ft, torch.from_numpy(starts).to(dev), starts, r, int(max_rounds))
    m = ops.surface_measure(ov, of, out_starts).cpu().numpy()
    return Surface(_arrays._wrap(v, ov), _arrays._wrap(f, of), float(m[0, 0]), float(m[0, 1]))


# ------------------------------------------------------------------ PLY
_PLY_HEAD = ("ply\nformat binary_little_endian 1.0\ncomment segmantic_amd label surface\n"
             "comment area {area!r}\ncomment volume {volume!r}\n"
             "element vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
             "element face {nf}\nproperty list uchar int vertex_indices\nend_header\n")
_FACE_DT = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def ply_header(surface: Surface) -> bytes:
    return _PLY_HEAD.format(area=float(surface.area), volume=float(surface.volume), nv=int(surface.vertices.shape[0]),
                            nf=int(surface.faces.shape[0])).encode("ascii")


def write_ply(path, surface: Surface) -> None:
    """Binary little-endian PLY with float x / y / z vertices and ``uchar int`` face lists, the layout
    ``vtkPLYWriter`` produces in binary mode; area and volume travel as comments."""
    v = np.ascontiguousarray(_host(surface.vertices), dtype="<f4").reshape(-1, 3)
    f = _host(surface.faces).reshape(-1, 3)
    rec = np.empty(f.shape[0], dtype=_FACE_DT)
    rec["n"] = 3
    rec["v"] = f
    with open(path, "wb") as fh:
        fh.write(ply_header(surface))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def read_ply(path) -> Surface:
    """Read a PLY written by :func:`write_ply` (numpy arrays)."""
    raw = Path(path).read_bytes()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    head = raw[:end].decode("ascii")
    if "format binary_little_endian 1.0" not in head or "property list uchar int vertex_indices" not in head:
        raise ValueError(f"{path}: only the binary little-endian triangle PLY of write_ply is supported")
    nv = int(re.search(r"^element vertex (\d+)$", head, re.M).group(1))
    nf = int(re.search(r"^element face (\d+)$", head, re.M).group(1))
    pos = end + len(b"end_header\n")
    if len(raw) != pos + 12 * nv + 13 * nf:
        raise ValueError(f"{path}: payload of {len(raw) - pos} bytes, {12 * nv + 13 * nf} expected")
    v = np.frombuffer(raw, dtype="<f4", count=3 * nv, offset=pos).reshape(nv, 3).astype(np.float32)
    rec = np.frombuffer(raw, dtype=_FACE_DT, count=nf, offset=pos + 12 * nv)
    if nf and (rec["n"] != 3).any():
        raise ValueError(f"{path}: only triangles are supported")
    f = np.ascontiguousarray(rec["v"]).astype(np.int32).reshape(nf, 3)
    area = re.search(r"^comment area (\S+)$", head, re.M)
    volume = re.search(r"^comment volume (\S+)$", head, re.M)
    return Surface(v, f, float(area.group(1)) if area else 0.0, float(volume.group(1)) if volume else 0.0)
