"""The inputs, spacings and radii of the unequal-spacing morphology tests, in one place: the host tests
(tests/test_morphology_aniso_host.py) establish on the oracle alone every property the GPU tests
(tests/test_morphology_aniso_gpu.py) lean on, for these very inputs."""
from __future__ import annotations

import functools

import numpy as np

from tests.helpers import morphology_ref as ref

DEFAULT = (20, 24, 28)     # P2 has 20 * 28 = 560 lines, P3 24 * 28 = 672: three workgroups each, the last ragged

# Spacings whose f64 arithmetic is exact: every spacing is a small multiple of a power of two, so each product
# (s d)^2, each sum of three of them and each term of the envelope test is a multiple of 2^-8 far below 2^53.
# All three oracle forms and the kernels then compute the same real numbers, ties included.
EXACT_3D = [(2.0, 1.0, 0.5), (0.25, 1.0, 4.0), (5.0, 0.75, 0.75)]
EXACT_2D = (1.0, 0.5)
# Spacings that round.  (5.0, 0.7, 0.7) is the clinical thick-slice case: sy == sx != sz still takes the f64 path.
INEXACT_3D = [(5.0, 0.7, 0.7), (1.3, 0.7, 1.1), (6.0, 0.4, 1.0)]
INEXACT_2D = (0.7, 1.1)
NEAR_TIE_CAP = 1e-2        # largest share of voxels whose nearest feature may hang on rounding (a condition)
TIE_SHARE = 0.02           # smallest share of voxels with two or more features at exactly the minimum: the denser
#                            scattered input and the 2-D one, under every exact spacing
TIE_SHARE_SPARSE = 0.005   # the same for the other scattered inputs, whose features are fewer

_BUILDERS = {
    "scattered_lo": lambda: ref.scattered(DEFAULT, 0.004, 7, 5, np.uint8),
    "scattered_hi": lambda: ref.scattered(DEFAULT, 0.03, 2, 5, np.int16),
    "slab": lambda: ref.slab(DEFAULT, 9, 15, 3, 5, np.int32),
    "staircase": lambda: ref.staircase((6, 12, 36), 3, np.uint8),
    "cliff": lambda: ref.cliff((6, 10, 64), np.int16),
    "ellipsoid": lambda: ref.ellipsoids(DEFAULT, 3, 5, lo=7.0, hi=13.0, margin=3.0, dtype=np.uint8),
    "wide": lambda: ref.scattered((9, 11, 131), 0.01, 5, 5, np.int16),          # bw > 64 and ragged
    "bd1": lambda: ref.scattered((1, 30, 34), 0.03, 6, 5, np.int32),
    "bd2": lambda: ref.scattered((2, 30, 34), 0.03, 7, 5, np.uint8),
    "flat": lambda: ref.scattered((40, 70), 0.02, 8, 5, np.uint8),              # 2-D
    # ellipsoids with scattered points in the background: labelled voxels at every depth and ties in bulk
    "mixed": lambda: _mixed(),
    "clinical": lambda: ref.ellipsoids(DEFAULT, 4, 4, lo=3.0, hi=7.0, margin=3.0, dtype=np.uint8),
}
NAMES_3D = ["scattered_lo", "scattered_hi", "slab", "staircase", "cliff", "ellipsoid", "wide", "bd1", "bd2"]
NAMES_2D = ["flat"]
SCATTERED = ["scattered_lo", "scattered_hi"]      # the two densities of the issue


def _mixed():
    lab = ref.ellipsoids(DEFAULT, 3, 5, lo=7.0, hi=13.0, margin=3.0, dtype=np.int16)
    pts = ref.scattered(DEFAULT, 0.02, 9, 5, np.int16)
    return np.where(lab != 0, lab, pts)


@functools.lru_cache(maxsize=None)
def _cached(name: str) -> np.ndarray:
    a = _BUILDERS[name]()
    a.setflags(write=False)
    return a


def volume(name: str) -> np.ndarray:
    """the named input, built once and read-only"""
    return _cached(name)


def exact_pairs():
    """(input name, exact spacing) of the zero-tolerance tests"""
    return [(n, sp) for n in NAMES_3D for sp in EXACT_3D] + [(n, EXACT_2D) for n in NAMES_2D]


def inexact_pairs():
    """(input name, inexact spacing) of the two-tier tests"""
    names = ["scattered_lo", "scattered_hi", "wide", "bd1"]
    return [(n, sp) for n in names for sp in INEXACT_3D] + [("flat", INEXACT_2D)]


BRUTE_MAX = 1 << 25       # voxels x features up to which ``oracle`` is the brute-force form


@functools.lru_cache(maxsize=None)
def oracle(name: str, spacing: tuple, mode: str, box=None):
    """(index, squared distance) of the named input and predicate, computed once: ``ref.nearest_brute``, or for
    the dense predicates of the larger inputs under exact spacings ``ref.nearest_separable``, which the host
    tests show to equal it bit for bit there.  ``box`` (z0 z1 y0 y1 x0 x1; y0 y1 x0 x1 in 2-D) restricts the
    input to a sub-array."""
    lab = volume(name)
    if box is not None:
        lab = lab[tuple(slice(box[2 * a], box[2 * a + 1]) for a in range(lab.ndim))]
    feature = {m: f for m, _, _, f in predicates(lab)}[mode]
    brute = box is not None or fits_brute(name, mode)
    assert brute or is_exact(spacing), "inexact spacings are compared with the brute-force form only"
    index, dsq = (ref.nearest_brute if brute else ref.nearest_separable)(feature, spacing)
    index.setflags(write=False)
    dsq.setflags(write=False)
    return index, dsq


def fits_brute(name: str, mode: str) -> bool:
    feature = {m: f for m, _, _, f in predicates(volume(name))}[mode]
    return feature.size * int(feature.sum()) <= BRUTE_MAX


def is_exact(spacing) -> bool:
    return tuple(spacing) in EXACT_3D or tuple(spacing) == EXACT_2D


TABLE_LABELS = [2, 5]


def predicates(lab: np.ndarray):
    """(mode name, label, table labels or None, feature mask) for the five predicates of the transform"""
    return [("FT_NONZERO", 0, None, lab != 0), ("FT_ZERO", 0, None, lab == 0), ("FT_EQUAL", 3, None, lab == 3),
            ("FT_NOT_EQUAL", 1, None, lab != 1), ("FT_TABLE", 0, TABLE_LABELS, np.isin(lab, TABLE_LABELS))]


# Which (input, exact spacing) pairs each deliberate fault of ``nearest_envelope`` must show up on (features:
# lab != 0).  The tie faults need ties in the pass concerned: the slab, the cliff and the solid ellipsoids have
# none in a row, and the staircase has them in P2 only where sy == sx.  Under (0.25, 1, 4) x is the coarse axis:
# two columns of a row equally far from a voxel are 4 mm or more away and the nearest feature is hardly ever one
# of them, so only the long rows of "wide" and the two planes of "bd2" are required to show "right_on_tie"; the
# 51 features of "scattered_lo" never show it.
_TIED = ["scattered_lo", "scattered_hi", "wide", "bd1", "bd2"]


def fault_pairs(fault: str):
    if fault == "fill_on_equal":
        return [(n, sp) for n in _TIED + ["ellipsoid"] for sp in EXACT_3D] + [("flat", EXACT_2D)]
    if fault == "right_on_tie":
        return ([(n, sp) for n in _TIED[1:] for sp in (EXACT_3D[0], EXACT_3D[2])]
                + [(n, EXACT_3D[1]) for n in ("wide", "bd2")] + [("flat", EXACT_2D)])
    assert fault == "drop_hx"
    return exact_pairs()


# (input, spacing, radius, applied subset) of the exact label-operation tests.  Every radius but BEYOND has at
# least ON_RADIUS_MIN background voxels and as many labelled voxels exactly on it (asserted by the host tests):
# the scattered points are one voxel each, so only the smallest spacing is such a radius for them.
BEYOND = 500.0
ON_RADIUS_MIN = 50
LABEL_CASES = (
    [("ellipsoid", EXACT_3D[0], r, a) for r in (1.0, 2.0, 2.5, 5.0, BEYOND) for a in (None, (1, 3))]
    + [("mixed", EXACT_3D[0], r, a) for r in (1.0, 2.5) for a in (None, (2, 5))]
    + [("scattered_hi", EXACT_3D[0], 0.5, None)]
    + [("ellipsoid", EXACT_3D[2], r, (1, 3)) for r in (1.5, 3.75)]
    + [("mixed", EXACT_3D[1], r, None) for r in (1.0, 2.0)]
    + [("flat", EXACT_2D, 0.5, None)]
)

# the label operations under the clinical spacing keep the flag-and-skip method of the equal-spacing file, whose
# cap is 1e-3; this case stays below half of it (asserted by the host tests)
CLINICAL = INEXACT_3D[0]
CLINICAL_RADIUS = 2.0
CLINICAL_APPLIED = [1, 2, 3, 4]
FLAG_CAP = 1e-3


def general_flags(lab, spacing, radius, applied):
    """the voxels the flag-and-skip comparison of the label operations leaves out, per operation: the same
    flags ``_check_general`` of tests/test_morphology_gpu.py computes before it asks the device"""
    feature = lab != 0

    def erode_flags(a):
        out = np.zeros(a.shape, bool)
        for L in applied:
            if (a == L).any():
                out |= ref.ambiguous(a != L, None, spacing, radius) & (a == L)
        return out

    want_erode = ref.erode_labels(lab, radius, spacing, applied)
    want_dilate = ref.dilate_labels(lab, radius, spacing, applied)
    return {"expand": ref.ambiguous(feature, lab, spacing, radius) & (lab == 0),
            "nearest": ref.ambiguous(feature, lab, spacing) & (lab == 0),
            "dilate": ref.ambiguous(np.isin(lab, applied), lab, spacing, radius) & (lab == 0),
            "erode": erode_flags(lab),
            "open stage 2": ref.ambiguous(np.isin(want_erode, applied), want_erode, spacing, radius) & (want_erode == 0),
            "close stage 2": erode_flags(want_dilate)}


def pythagorean_case():
    """-> (labels, spacing, voxel, winner): two features of plane 0 at the in-plane offsets (-6, 7) and (9, 2)
    from ``voxel`` of plane 1, both 85 voxel units away.  Under (5, 0.7, 0.7) their full f64 distances are
    bit-equal, so ``winner``, the one with the smaller raster index, is nearest; the f64 in-plane sums
    (0.7 * 6)^2 + (0.7 * 7)^2 and (0.7 * 9)^2 + (0.7 * 2)^2 differ in the last bit in favour of the other."""
    lab = np.zeros((2, 16, 8), np.uint8)
    lab[0, 0, 5], lab[0, 15, 0] = 4, 9
    return lab, CLINICAL, (1, 9, 7), (0 * 16 + 0) * 8 + 5
