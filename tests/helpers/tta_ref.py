"""float64 oracles and error bounds of the test-time-augmentation kernels (tests/test_tta_host.py,
tests/test_tta_gpu.py), written from the definitions in DESIGN.md section 17.

Oracles (numpy float64): ``ref_accumulate``, ``ref_finalize``, ``ref_label_means``, ``ref_mirror_tta``.
``f32_accumulate`` / ``f32_finalize`` restate the kernels' stated operation order in numpy float32; the host
tests hold them against the oracles with the bounds below, the GPU tests hold the kernels to the same bounds.

Error bounds
------------
u = 2^-24 is the unit roundoff of float32: one rounded operation has relative error <= u; ``expf`` and ``logf``
of the device (and numpy's float32 ones) are accurate to 1 ulp, i.e. relative error <= 2u.  Logits are assumed
to span less than 80 per voxel, so no ``expf`` underflows.  First-order terms only; K classes, M passes.

One pass, channel c, with d_c = l_c - m <= 0 and p_c = e_c / s:
  * the subtraction rounds d_c by u|d_c|, which changes e_c by the relative amount u|d_c| = u ln(1 / (p_c s))
    <= u ln(1 / p_c)                                                       (s >= 1: the maximum gives e = 1);
  * expf: 2u relative;
  * s: K - 1 sequential adds of positive terms, (K - 1)u relative, plus the weighted mean of the terms' own
    errors: 2u (expf) + u sum_c p_c |d_c| <= 2u + u ln K                     (sum_c p_c |d_c| = H(p) - ln s <= ln K);
  * the division: u.
  so  |dp_c| <= p_c (a + u ln(1 / p_c))  with  a = (K + 4 + ln K) u,  and since p ln(1/p) <= 1/e and p <= 1,
  |dp_c| <= a + u / e.

Accumulator after M passes: the pass errors add up, and the add of pass i >= 2 rounds a sum <= i by <= i u:
  ``acc_bound``  = M (a + u / e) + (M (M + 1) / 2 - 1) u     (absolute, per channel).

Final probability q_c = acc_c / S, S = sum_c acc_c:
  * acc_c relative: a + u ln(1 / q_c) (p ln(1/p) is concave, so the passes' log terms are bounded by the one of
    their mean) + (M - 1) u for the M - 1 adds of positive terms;
  * S relative: the weighted mean of those, a + u ln K + (M - 1) u, plus (K - 1) u for its own K - 1 adds;
  * the division: u.
  so  |dq_c| <= q_c (A + u ln(1 / q_c))  with  A = (3 K + 8 + 3 ln K + 2 (M - 1)) u,  and
  ``prob_bound`` = A + u / e                                                (absolute; 78.7 u for K = 16, M = 8).
  For ``tta_finalize`` alone, on scores that are exact float32 inputs, only S and the division act:
  A_fin = K u, no log term: ``finalize_prob_bound`` = K u.

Entropy -(sum_c t_c) / ln K with t_c = q_c ln q_c.  With q_c known to the relative error eps_c = A + u ln(1/q_c),
  t_c changes by eps_c q_c (|ln q_c| + 1); logf adds 2u |t_c| and the product u |t_c|; the K - 1 sequential adds
  (K - 1) u sum_c |t_c|.  Summed over c with sum q_c = 1, sum |t_c| = H <= ln K, q ln(1/q) <= 1/e and
  q ln^2(1/q) <= 4 / e^2:
      |dh| <= A (ln K + 1) + u (4 K / e^2 + ln K) + (K + 2) u ln K
  and the final division by logf(K) adds u + 2u relative to a value <= 1:
  ``entropy_bound`` = |dh| / ln K + 3 u                                      (131 u for K = 16, M = 8).
  The clamp to [0, 1] can only move the result towards the true value.

The restatement run on N(0, 3^2) logits, M = 8, K in {2, 3, 16, 17, 40} deviates by at most 2.5 u (probability)
and 6.6 u (entropy): the bounds are worst cases, 20 to 30 times above what random rounding gives.

Labels are compared exactly except at voxels whose float64 top-two margin is below twice the probability bound
(either side of the margin can move by the bound); ``check_labels`` asserts that at most 0.1 % of the voxels
are excused that way.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
MAX_EXCUSED = 1e-3


# ---------------------------------------------------------------------------- bounds
def _a(K: int) -> float:
    return (K + 4 + math.log(K)) * U


def acc_bound(K: int, M: int) -> float:
    return M * (_a(K) + U / math.e) + (M * (M + 1) / 2 - 1) * U


def _rel_A(K: int, M: int) -> float:
    return (3 * K + 8 + 3 * math.log(K) + 2 * (M - 1)) * U


def prob_bound(K: int, M: int) -> float:
    return _rel_A(K, M) + U / math.e


def finalize_prob_bound(K: int) -> float:
    return K * U


def _entropy_bound(K: int, A: float) -> float:
    lnk = math.log(K)
    dh = A * (lnk + 1) + U * (4 * K / math.e ** 2 + lnk) + (K + 2) * U * lnk
    return dh / lnk + 3 * U


def entropy_bound(K: int, M: int) -> float:
    return _entropy_bound(K, _rel_A(K, M))


def finalize_entropy_bound(K: int) -> float:
    return _entropy_bound(K, K * U)


# ---------------------------------------------------------------------------- float64 oracles
def _axes(mask: int):
    return tuple(a for a in range(3) if mask & (1 << a))


def unmirror(vol: np.ndarray, mask: int) -> np.ndarray:
    """[d, h, w, ...] of the mirrored volume -> the same in the original orientation"""
    ax = _axes(mask)
    return np.flip(vol, ax) if ax else vol


def ref_softmax(logits: np.ndarray) -> np.ndarray:
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def ref_accumulate(logits_passes, masks) -> np.ndarray:
    """logits_passes[i]: [d, h, w, K] of pass i (on the volume mirrored by masks[i]) -> sum of the un-mirrored
    softmaxes, float64"""
    acc = None
    for lg, m in zip(logits_passes, masks):
        p = unmirror(ref_softmax(lg), m)
        acc = p.copy() if acc is None else acc + p
    return acc


def ref_finalize(scores: np.ndarray):
    """scores [..., K] >= 0 -> (labels int64, confidence, entropy, probs) in float64"""
    sc = np.asarray(scores, np.float64)
    K = sc.shape[-1]
    s = sc.sum(-1, keepdims=True)
    empty = s[..., 0] == 0
    q = sc / np.where(s == 0, 1.0, s)
    q[empty] = 0.0
    q[empty, 0] = 1.0
    labels = q.argmax(-1)                               # numpy: the first maximum
    conf = np.take_along_axis(q, labels[..., None], -1)[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)
    ent = np.clip(-t.sum(-1) / math.log(K), 0.0, 1.0)
    return labels, conf, ent, q


def ref_label_means(labels: np.ndarray, values: np.ndarray, k: int):
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    val = np.asarray(values, np.float64).reshape(-1)
    ok = (lab >= 0) & (lab < k)
    counts = np.bincount(lab[ok], minlength=k).astype(np.int64)
    sums = np.array([math.fsum(val[ok & (lab == c)]) for c in range(k)], np.float64)
    return sums, counts


def ref_mirror_tta(logits_passes, masks):
    """the whole of ``mirror_tta_inference`` after the network: (labels, confidence, entropy, probs)"""
    return ref_finalize(ref_accumulate(logits_passes, masks))


# ---------------------------------------------------------------------------- float32 restatement
def _seq_sum(x: np.ndarray) -> np.ndarray:
    """sum over the last axis in ascending index order, every add rounded to float32"""
    s = x[..., 0].copy()
    for c in range(1, x.shape[-1]):
        s = (s + x[..., c]).astype(np.float32)
    return s


def f32_softmax(logits: np.ndarray) -> np.ndarray:
    l = np.asarray(logits, np.float32)
    e = np.exp((l - l.max(-1, keepdims=True)).astype(np.float32)).astype(np.float32)
    return (e / _seq_sum(e)[..., None]).astype(np.float32)


def f32_accumulate(logits_passes, masks, mirror=unmirror) -> np.ndarray:
    acc = None
    for lg, m in zip(logits_passes, masks):
        p = mirror(f32_softmax(lg), m)
        acc = p.copy() if acc is None else (acc + p).astype(np.float32)
    return acc


def f32_finalize(scores: np.ndarray, divide_by=None, last_max=False, normalise=True):
    """the kernel's operation order in float32.  The keyword arguments plant faults for the host tests:
    ``divide_by`` a constant instead of s, the last maximum instead of the first, the entropy left un-normalised."""
    sc = np.asarray(scores, np.float32)
    K = sc.shape[-1]
    s = _seq_sum(sc)
    empty = s == 0
    den = np.where(empty, np.float32(1), s) if divide_by is None else np.full_like(s, divide_by)
    q = (sc / den[..., None]).astype(np.float32)
    q[empty] = 0.0
    q[empty, 0] = 1.0
    labels = (K - 1 - q[..., ::-1].argmax(-1)) if last_max else q.argmax(-1)
    conf = np.take_along_axis(q, labels[..., None], -1)[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(q > 0, (q * np.log(np.where(q > 0, q, np.float32(1))).astype(np.float32)), np.float32(0))
    h = _seq_sum(t.astype(np.float32))
    ent = (-h / np.log(np.float32(K))).astype(np.float32) if normalise else (-h).astype(np.float32)
    ent = np.clip(ent, 0.0, 1.0) if normalise else ent
    return labels, conf, ent, q


# ---------------------------------------------------------------------------- gates
def check_close(got, ref, bound: float, what: str) -> float:
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))))
    print(f"{what}: max error {err / U:.2f} u against a bound of {bound / U:.1f} u")
    assert err <= bound, f"{what}: max error {err:.3e} ({err / U:.1f} u) above the bound {bound:.3e} ({bound / U:.1f} u)"
    return err


def check_labels(got, ref_probs, bound: float, what: str = "labels") -> float:
    """exact agreement with the float64 first maximum, except where the float64 top-two margin is below
    2 * bound; returns the excused share and asserts it stays below MAX_EXCUSED"""
    q = np.asarray(ref_probs, np.float64)
    K = q.shape[-1]
    ref = q.argmax(-1)
    top2 = np.partition(q, K - 2, axis=-1)[..., K - 2:]
    margin = top2[..., 1] - top2[..., 0]
    close = margin < 2 * bound
    share = float(close.mean())
    print(f"{what}: {int(close.sum())} of {close.size} voxels within 2 x bound of a tie (share {share:.2e})")
    assert share <= MAX_EXCUSED, f"{what}: {share:.2e} of the voxels are near-ties, above the cap {MAX_EXCUSED}"
    got = np.asarray(got).astype(np.int64)
    bad = (got != ref) & ~close
    assert not bad.any(), f"{what}: {int(bad.sum())} voxels differ from the float64 argmax away from ties"
    # a voxel excused as a near-tie must still carry one of the two leading classes
    if close.any():
        second = np.argsort(-q, axis=-1, kind="stable")[..., 1]
        assert np.all((got == ref) | (got == second) | ~close), f"{what}: a near-tie voxel carries a third class"
    return share


# ---------------------------------------------------------------------------- shared inputs
SHAPES = [(5, 6, 7), (1, 9, 4), (8, 8, 8), (3, 1, 66)]
CLASSES = [2, 3, 16, 17, 40]
ALL_MASKS = list(range(8))


def case_seed(shape, K: int) -> int:
    return 1000 * SHAPES.index(tuple(shape)) + K


def make_logits(shape, K: int, seed: int, passes: int = 8):
    """per-pass logits N(0, 3^2), float32, [passes][d, h, w, K]"""
    rng = np.random.default_rng(seed)
    return [(3.0 * rng.standard_normal(tuple(shape) + (K,))).astype(np.float32) for _ in range(passes)]


def special_scores(K: int) -> np.ndarray:
    """scores [n, K] float32 for ``tta_finalize``: an all-zero voxel, single-class voxels (first and last class),
    a uniform voxel, an exact two-way tie of the maximum, sums far from any pass count, then seeded random rows
    with zeros in them"""
    rows = [np.zeros(K)]
    for c in (0, K - 1):
        r = np.zeros(K); r[c] = 3.25; rows.append(r)
    rows.append(np.full(K, 0.625))
    r = np.full(K, 0.125); r[K - 1] = 2.0; r[max(0, K - 2)] = 2.0; rows.append(r)     # tie: class K - 2 wins
    r = np.full(K, 0.25); r[0] = 1.5; r[1 % K] = 1.5; rows.append(r)                  # tie: class 0 wins
    rng = np.random.default_rng(77 + K)
    rnd = rng.random((58, K)) * rng.choice([0.01, 0.7, 8.0, 300.0], size=(58, 1))    # sums != M
    rnd[rng.random((58, K)) < 0.2] = 0.0
    return np.concatenate([np.stack(rows), rnd]).astype(np.float32)
