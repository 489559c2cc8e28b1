"""Python / float64 restatement of the mesh decimation of segmantic_amd.image.surfaces:
round-based edge collapse over independent sets.  Every floating-point sum is written out in the order the kernels
use; nothing on the cost path goes through np.sum / dot / cross.  The device must produce the same integer mesh."""
from __future__ import annotations

import bisect
import math
import struct

import numpy as np

MAX_VALENCE = 32
NO_KEY = (1 << 64) - 1


def mix32(u: int, t: int) -> int:
    x = (u * 0x9E3779B1 + t * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    x = (x * 0x297A2D39) & 0xFFFFFFFF
    x ^= x >> 15
    return x


def bucket(cost: float) -> int:
    """float32(cost) bits >> 23: the power-of-two bucket of a cost >= 0"""
    try:
        return struct.unpack("<I", struct.pack("<f", cost))[0] >> 23
    except OverflowError:
        return 255


def _normal(a, b, c):
    """(b - a) x (c - a)"""
    ux, uy, uz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    wx, wy, wz = c[0] - a[0], c[1] - a[1], c[2] - a[2]
    return (uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx)


def _face_quadric(a, b, c):
    """p p^T, p = (n, -n.a): xx xy xz xw yy yz yw zz zw ww"""
    nx, ny, nz = _normal(a, b, c)
    pw = -((nx * a[0] + ny * a[1]) + nz * a[2])
    return (nx * nx, nx * ny, nx * nz, nx * pw, ny * ny, ny * nz, ny * pw, nz * nz, nz * pw, pw * pw)


def _cost(q, p):
    x, y, z = p
    r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3]
    r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6]
    r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8]
    r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9]
    cost = ((x * r0 + y * r1) + z * r2) + r3
    return cost if cost > 0.0 else 0.0


def target_faces(n_faces: int, reduction: float) -> int:
    return math.ceil((1.0 - float(reduction)) * n_faces)


def decimate(vertices, faces, reduction: float, max_rounds: int = 128, cache: bool = True):
    """-> dict(vertices f32 [V', 3], faces i32 [F', 3], kept i32 [V'], target, history (collapses per round)).
    ``cache=False`` recomputes every ring and every choice in every round (the definition as written);
    ``cache=True`` recomputes only what a collapse can have changed, and must give the same mesh."""
    V = np.asarray(vertices)
    Fa = np.asarray(faces)
    nV, nF = V.shape[0], Fa.shape[0]
    target = target_faces(nF, reduction)
    if reduction == 0.0 or nF == 0:
        return {"vertices": V, "faces": Fa, "kept": np.arange(nV, dtype=np.int32), "target": target, "history": []}
    assert nV < 2 ** 23
    P = [tuple(r) for r in V.astype(np.float32).astype(np.float64).tolist()]
    F = [list(r) for r in Fa.astype(np.int64).tolist()]
    live_f = [True] * nF
    live_v = [True] * nV
    star = [[] for _ in range(nV)]                     # one entry per slot, ascending face number
    for f, t in enumerate(F):
        for u in t:
            star[u].append(f)
    Q = []
    for u in range(nV):
        q = [0.0] * 10
        for f in star[u]:
            k = _face_quadric(P[F[f][0]], P[F[f][1]], P[F[f][2]])
            for j in range(10):
                q[j] += k[j]
        Q.append(q)

    def ring_of(u):
        """successors of u in its faces when the star is one closed fan of 3 .. 32 faces, else None (pinned)"""
        st = star[u]
        d = len(st)
        if not live_v[u] or d < 3 or d > MAX_VALENCE:
            return None
        link = {}
        preds = set()
        for f in st:
            a, b, c = F[f]
            s, p = (b, c) if a == u else ((c, a) if b == u else (a, b))
            if s == u or p == u or s == p or s in link or p in preds:
                return None
            link[s] = p
            preds.add(p)
        if preds != set(link):
            return None
        first = next(iter(link))
        cur, n = link[first], 1
        while cur != first:
            cur, n = link[cur], n + 1
        return list(link) if n == d else None

    def neighbours(u):
        return {w for f in star[u] for w in F[f] if w != u}

    def choice_of(u):
        """(bucket, v) of the admissible v with the smallest (bucket, v), or None"""
        ru = ring[u]
        best = None
        for v in ru:
            rv = ring[v]
            if rv is None or len(star[u]) + len(star[v]) < 7:
                continue
            if sum(1 for f in star[u] if v in F[f]) != 2:
                continue
            shared = set(ru) & set(rv)
            if len(shared) != 2 or any(len(star[x]) < 4 for x in shared):
                continue
            ok = True
            for f in star[u]:
                t = F[f]
                if v in t:
                    continue
                n0 = _normal(P[t[0]], P[t[1]], P[t[2]])
                r = [v if x == u else x for x in t]
                n1 = _normal(P[r[0]], P[r[1]], P[r[2]])
                if not ((n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2] > 0.0):
                    ok = False
                    break
            if not ok:
                continue
            k = (bucket(_cost([Q[u][j] + Q[v][j] for j in range(10)], P[v])), v)
            if best is None or k < best:
                best = k
        return best

    ring = [None] * nV
    choice = [None] * nV
    ring_dirty = set(range(nV))
    choice_dirty = set(range(nV))
    n_live = nF
    history = []
    for t in range(int(max_rounds)):
        if n_live <= target:
            break
        if not cache:
            ring_dirty = set(range(nV))
            choice_dirty = set(range(nV))
        for u in ring_dirty:
            ring[u] = ring_of(u)
        for u in choice_dirty:
            choice[u] = choice_of(u) if ring[u] is not None else None
        ring_dirty, choice_dirty = set(), set()
        cands = {}
        slot = {}
        for u in range(nV):
            if choice[u] is None:
                continue
            key = (choice[u][0] << 55) | (mix32(u, t) << 23) | u
            cands[u] = key
            for w in [u] + ring[u]:
                if slot.get(w, NO_KEY) > key:
                    slot[w] = key
        winners = [u for u, key in cands.items() if all(slot[w] == key for w in [u] + ring[u])]
        history.append(len(winners))
        if not winners:
            break
        touched = set()
        for u in winners:
            touched.add(u)
            touched.update(ring[u])
        for w in touched:
            choice_dirty.add(w)
            choice_dirty.update(neighbours(w))
        for u in winners:
            v = choice[u][1]
            for f in star[u]:
                tri = F[f]
                if v in tri:
                    live_f[f] = False
                    n_live -= 1
                    for x in tri:
                        if x != u:
                            star[x].remove(f)
                else:
                    tri[tri.index(u)] = v
                    bisect.insort(star[v], f)
            star[u] = []
            for j in range(10):
                Q[v][j] += Q[u][j]
            live_v[u] = False
        ring_dirty = touched
        for w in touched:
            choice_dirty.update(neighbours(w))
    kept = np.asarray([u for u in range(nV) if live_v[u]], np.int32)
    remap = -np.ones(nV, np.int64)
    remap[kept] = np.arange(len(kept))
    out_f = np.asarray([F[f] for f in range(nF) if live_f[f]], np.int64).reshape(-1, 3)
    return {"vertices": np.ascontiguousarray(V[kept]), "faces": remap[out_f].astype(np.int32), "kept": kept,
            "target": target, "history": history}


# ------------------------------------------------------------------ invariants, computed from a mesh alone
def n_components(n_vertices: int, faces: np.ndarray) -> int:
    parent = list(range(n_vertices))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b, c in np.asarray(faces).tolist():
        ra = find(a)
        parent[find(b)] = ra
        parent[find(c)] = ra
    return len({find(i) for i in range(n_vertices)})


def no_degenerate_or_repeated_face(faces: np.ndarray) -> bool:
    f = np.asarray(faces)
    if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any():
        return False
    return len(np.unique(np.sort(f, 1), axis=0)) == len(f)


def faces_are_ordered_subset(faces_in: np.ndarray, faces_out: np.ndarray, kept: np.ndarray) -> bool:
    """every output face, in input numbering, comes from an input face with the same untouched slots, and the
    order of the surviving faces is the input's: walk both lists once"""
    back = np.asarray(kept)[np.asarray(faces_out)]
    kept_set = set(np.asarray(kept).tolist())
    i = 0
    fin = np.asarray(faces_in)
    for row in back.tolist():
        while i < len(fin):
            src = fin[i].tolist()
            i += 1
            if all(s == r or s not in kept_set for s, r in zip(src, row)):
                break
        else:
            return False
    return True
