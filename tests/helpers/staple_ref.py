"""Multi-label STAPLE as DESIGN.md section 22 defines it, in numpy (int64 / float64), and a seeded rater generator.

Every float64 operation of the E-step is one numpy operation, so it is rounded on its own as on the device; every
sum is an integer.  ``fault`` selects a deliberately wrong variant, used to show that the exact comparison of the
GPU tests catches it."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

Q = 1 << 24
FAULTS = ("descending", "row_total", "truncate", "largest_tie", "stop_le", "prior_rater0")


class RefResult(NamedTuple):
    labels: np.ndarray        # [*shape], dtype of the input
    sums: np.ndarray          # int64 [R, L, L]
    prior: np.ndarray         # float64 [L]
    iterations: int
    converged: bool
    q: np.ndarray             # int64 [N, L], the last E-step
    theta: np.ndarray         # float64 [R, L, L] of the last M-step

    @property
    def posterior(self) -> np.ndarray:      # float32 [L, *shape]
        p = (self.q.astype(np.float64) / float(Q)).astype(np.float32)
        return np.ascontiguousarray(p.T).reshape((p.shape[1],) + self.labels.shape)


def vote(D: np.ndarray, L: int, largest_tie: bool = False) -> np.ndarray:
    """most frequent label per voxel of D [R, N]; ties go to the smallest label"""
    counts = np.zeros((D.shape[1], L), dtype=np.int64)
    for r in range(D.shape[0]):
        counts[np.arange(D.shape[1]), D[r]] += 1
    if largest_tie:
        return (L - 1 - np.argmax(counts[:, ::-1], axis=1)).astype(np.int64)
    return np.argmax(counts, axis=1).astype(np.int64)


def m_step(D: np.ndarray, q: np.ndarray, L: int) -> np.ndarray:
    """S[r][l][s] = sum of q_i[s] over the voxels with D_r(i) = l, exact in int64"""
    i, s = np.nonzero(q)
    v = q[i, s]
    hi, lo = (v >> 12).astype(np.float64), (v & 0xFFF).astype(np.float64)   # each partial sum stays below 2^53
    S = np.zeros((D.shape[0], L, L), dtype=np.int64)
    for r in range(D.shape[0]):
        key = D[r][i] * L + s
        S[r] = ((np.bincount(key, weights=hi, minlength=L * L).astype(np.int64) << 12)
                + np.bincount(key, weights=lo, minlength=L * L).astype(np.int64)).reshape(L, L)
    return S


def theta_of(S: np.ndarray, fault: Optional[str] = None) -> np.ndarray:
    Sf = S.astype(np.float64)
    if fault == "row_total":
        T = S.sum(axis=2, keepdims=True).astype(np.float64)                  # per rater and row: wrong
    else:
        T = np.broadcast_to(S[0].sum(axis=0).astype(np.float64)[None, None, :], S.shape)
    out = np.zeros_like(Sf)
    np.divide(Sf, T, out=out, where=T != 0)
    return out


def e_step(D: np.ndarray, theta: np.ndarray, prior: np.ndarray, fault: Optional[str] = None) -> np.ndarray:
    R, N = D.shape
    p = np.repeat(prior[None, :], N, axis=0)
    order = range(R - 1, -1, -1) if fault == "descending" else range(R)
    for r in order:
        p = p * theta[r][D[r]]
    tot = p[:, 0].copy()
    for s in range(1, p.shape[1]):
        tot = tot + p[:, s]
    W = np.zeros_like(p)                                # tot = 0 (a given prior of tiny size only): q = 0
    np.divide(p, tot[:, None], out=W, where=(tot > 0)[:, None])
    if fault == "truncate":
        return np.floor(W * 16777216.0).astype(np.int64)
    return np.floor(W * 16777216.0 + 0.5).astype(np.int64)


def staple_ref(labels, num_classes: int, prior=None, max_iterations: int = 100, tolerance: float = 1e-5,
               fault: Optional[str] = None) -> RefResult:
    assert fault is None or fault in FAULTS
    labels = [np.asarray(a) for a in labels]
    shape, dtype = labels[0].shape, labels[0].dtype
    D = np.stack([a.reshape(-1).astype(np.int64) for a in labels])
    R, N = D.shape
    L = int(num_classes)
    assert D.min() >= 0 and D.max() < L
    if prior is None:
        src = D[:1] if fault == "prior_rater0" else D
        prior = np.bincount(src.reshape(-1), minlength=L).astype(np.float64) / float(src.shape[0] * N)
    else:
        prior = np.asarray(prior, dtype=np.float64).copy()
    q = np.zeros((N, L), dtype=np.int64)
    q[np.arange(N), vote(D, L, fault == "largest_tie")] = Q
    S = m_step(D, q, L)
    theta = theta_of(S, fault)
    it, converged = 0, False
    while True:
        q = e_step(D, theta, prior, fault)
        S = m_step(D, q, L)
        new = theta_of(S, fault)
        it += 1
        delta = float(np.max(np.abs(new - theta)))
        theta = new
        if (delta <= tolerance) if fault == "stop_le" else (delta < tolerance):
            converged = True
            break
        if it == max_iterations:
            break
    out = np.argmax(q, axis=1).astype(dtype).reshape(shape)
    return RefResult(out, S, prior, it, converged, q, theta)


def make_raters(shape, num_classes: int, accuracies, seed: int, dtype=np.uint8, truth_labels=None):
    """(truth, [rater volumes]): truth drawn per voxel (uniformly from ``truth_labels``, default all), rater r
    right with probability accuracies[r], else a uniformly drawn other label"""
    rng = np.random.default_rng(seed)
    L = int(num_classes)
    n = int(np.prod(shape))
    pool = np.arange(L) if truth_labels is None else np.asarray(truth_labels)
    truth = pool[rng.integers(0, len(pool), size=n)].astype(np.int64)
    raters = []
    for a in accuracies:
        right = rng.random(n) < a
        other = (truth + rng.integers(1, L, size=n)) % L
        raters.append(np.where(right, truth, other).astype(dtype).reshape(shape))
    return truth.astype(dtype).reshape(shape), raters
