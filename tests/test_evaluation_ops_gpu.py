"""Every entry point of csrc/distance.hip called directly on the MI355X (label boxes, EDT, sampler, radix select,
confusion counts) at the grid caps, tables and chunk edges that tests/helpers/evaluation_limits.py lays out and
tests/test_evaluation_limits_host.py proves are crossed, against the oracles of tests/helpers/distance_ref.py.
Integer results and the unit-spacing transform are compared bit for bit; every other tolerance is derived where it
is used, and the observed maximum is printed as a fraction of it."""
import math

import numpy as np
import pytest
import torch

from segmantic_amd import ops
from segmantic_amd.seg import evaluation
from tests.helpers import distance_ref as ref
from tests.helpers import evaluation_limits as lim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32}
U32, U64 = 2.0 ** -24, 2.0 ** -53                # unit roundoff of float32 and float64
SENTINEL = -7.0
UNIT = (1.0, 1.0, 1.0)


def _t(a, dtype=None) -> torch.Tensor:
    t = torch.from_numpy(np.array(a))            # a copy: the cached inputs are read-only
    return (t if dtype is None else t.to(TORCH[dtype])).to(DEV)


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _box3(shape, box=None):
    shp = (1,) * (3 - len(shape)) + tuple(shape)
    return tuple(box) if box is not None else (0, shp[0], 0, shp[1], 0, shp[2])


def _extents(box):
    return box[1] - box[0], box[3] - box[2], box[5] - box[4]


# ---------------------------------------------------------------------------- 1. label boxes
def _label_boxes(pred, truth, k):
    p, t = _t(pred), _t(truth)
    out = []
    for fill in (-7, 11):                         # two calls over different stale contents
        boxes = torch.full((k, 6), fill, dtype=torch.int32, device=DEV)
        counts = torch.full((k, 2), fill, dtype=torch.int64, device=DEV)
        ops.label_boxes(p, t, k, boxes, counts)
        out.append((boxes.cpu().numpy(), counts.cpu().numpy()))
    assert np.array_equal(p.cpu().numpy(), pred) and np.array_equal(t.cpu().numpy(), truth)       # inputs untouched
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])          # equal bits
    return out[0]


def _check_boxes(pred, truth, k):
    boxes, counts = _label_boxes(pred, truth, k)
    want_b, want_c = ref.label_boxes(pred, truth, k)
    assert np.array_equal(counts, want_c), np.argwhere(counts != want_c)[:5]
    assert np.array_equal(boxes, want_b), np.argwhere(boxes != want_b)[:5]
    return boxes, counts


@pytest.mark.parametrize("dtype", lim.LABEL_TYPES)
@pytest.mark.parametrize("w", lim.BOX_WIDTHS)
def test_label_boxes_widths_and_chunk_edges(w, dtype):
    """rows of 1, 63, 64, 65 and 130 voxels against the 64-lane chunks; out-of-range and negative values count for
    nothing; label 3 is in pred only, 4 in truth only, 5 absent or one run across x = 64"""
    pred, truth = lim.box_width_volume(w, dtype)
    boxes, counts = _check_boxes(pred, truth, lim.BOX_K)
    if w > 1:
        assert counts[3, 0] > 0 and counts[3, 1] == 0 and counts[4, 0] == 0 and counts[4, 1] > 0
    if w == 130:
        assert boxes[5].tolist() == [1, 2, 2, 3, 60, 71] and counts[5].tolist() == [11, 0]
    else:
        assert boxes[5].tolist() == [0] * 6 and counts[5].tolist() == [0, 0]


def test_label_boxes_2d():
    for w in (65, 130):
        pred, truth = lim.box_width_volume(w, "int16", 2)
        boxes, counts = _check_boxes(pred, truth, lim.BOX_K)
        assert (boxes[counts.sum(1) > 0, :2] == [0, 1]).all()    # [h, w] is read as one slice z = 0
    assert _check_boxes(*lim.box_width_volume(130, "uint8", 2), lim.BOX_K)[0][5].tolist() == [0, 1, 2, 3, 60, 71]


@pytest.mark.parametrize("dtype", lim.LABEL_TYPES)
def test_label_boxes_second_trip_of_the_capped_grid(dtype):
    """4158 rows against 4 x 1024 per trip: label 2 lives in rows 4096 .. 4157 only"""
    pred, truth, k = lim.box_trip_volume(dtype)
    boxes, counts = _check_boxes(pred, truth, k)
    assert counts[2].min() >= 7 and boxes[2][:2].tolist() == [65, 66] and boxes[3].tolist() == [0] * 6


@pytest.mark.parametrize("k, dtype", lim.BOX_TABLE_KS)
def test_label_boxes_table(k, dtype):
    """k = 1, 255 and kBoxMaxLabels = 1024: every label on one voxel of each volume, so every entry of the LDS table
    is written and every other voxel is out of range"""
    pred, truth = lim.box_table_volume(k, dtype)
    boxes, counts = _check_boxes(pred, truth, k)
    assert (counts == 1).all()


def test_label_boxes_refuses_a_table_past_the_cap():
    pred, truth = lim.box_table_volume(1024, "int32")
    p, t = _t(pred), _t(truth)
    boxes = torch.zeros((1025, 6), dtype=torch.int32, device=DEV)
    counts = torch.zeros((1025, 2), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"label_boxes: 1 <= k <= 1024"):
        ops.label_boxes(p, t, 1025, boxes, counts)
    with pytest.raises(RuntimeError, match=r"label_boxes: 1 <= k <= 1024"):
        ops.label_boxes(p, t, 0, boxes, counts)


# ---------------------------------------------------------------------------- 2. EDT
def _edt(labels_np, label, feature, spacing, box=None, dtype=None):
    """ops.edt_sq over the box as a signed float32 array in array order ([z, y, x]; 2-D input: [y, x]); the spacing
    is per array axis and reaches the kernel as float32"""
    lab = _t(labels_np, dtype)
    box = _box3(labels_np.shape, box)
    bd, bh, bw = _extents(box)
    dist = torch.full((bd * bh * bw,), math.nan, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.edt_workspace_bytes(box), dtype=torch.uint8, device=DEV)
    sp3 = [1.0] * (3 - labels_np.ndim) + list(spacing)
    ops.edt_sq(lab, label, feature, box, sp3, dist, ws)
    out = dist.reshape(bd, bw, bh).permute(0, 2, 1).cpu().numpy()
    return out if labels_np.ndim == 3 else out[0]


@pytest.mark.parametrize("shape", lim.LONG_SHAPES)
def test_edt_unit_spacing_beyond_2_24(shape):
    """6000-long lines on P2, P3 and P1 in turn, squared distances up to 3.6e7 > 2^24.

    Bit for bit the result is the float64 restatement of the three passes that rounds to float32 after each
    (ref.edt_sq_passes_f32): that is what the integer path computes once heights are rounded float32 values.
    Against the true squared distance `want` the error is at most ((1 + 2^-24)^3 - 1) * want: each pass computes
    min_j (g_j + (t - j)^2) exactly from the heights g_j it is given and rounds once (relative 2^-24 at most); all
    terms are non-negative, so if every g_j is off by a factor within (1 + e) then so is every candidate and so is
    their minimum; three passes, three factors.  Below 2^24 nothing is rounded and the result is exact."""
    lab = lim.long_volume(shape)
    unit = (1.0,) * len(shape)
    restated = ref.edt_sq_passes_f32(lab == 1)
    want = ref.edt_sq_brute(lab == 1, unit)
    small = want < lim.EXACT_F32
    bound = ((1 + U32) ** 3 - 1) * want
    assert want.max() > 2 ** 25 and small.sum() > 1000
    for feature in (0, 1):
        got = _edt(lab, 1, feature, unit)
        assert np.array_equal(np.signbit(got), (lab == 1) if feature else np.zeros(shape, bool))
        got = np.abs(got)
        assert np.array_equal(_bits(got), _bits(restated)), np.abs(got.astype(np.float64) - restated).max()
        assert np.array_equal(got[small].astype(np.float64), want[small])
        err = np.abs(got.astype(np.float64) - want)
        worst = float((err[~small] / bound[~small]).max())
        print(f"edt {shape} feature {feature}: error at most {worst:.4f} of the three-rounding bound")
        assert (err <= bound).all()


def _aniso_bound(want, shape, sp):
    """|got - want| for the general-spacing path, `want` being ref.edt_sq_brute at the float32 spacings.

    Relative part: three float32 roundings as in the unit case, (1 + 2^-24)^3.  In float64: P1 rounds dz = dist * sz
    and dz * dz (2); each envelope pass evaluates g + w2 * (t - v) * (t - v) with 3 roundings (w2 = s * s is exact:
    24-bit factors) and may stop its walk at a neighbour whose computed value is within those roundings of the
    better one (6 more); two passes: 2 + 2 * 9 = 20 factors (1 + 2^-53).  The reference's own 4 roundings are added.
    Absolute part: the pop test compares (Fq - Fb)(vb - va) with (Fb - Fa)(q - vb), F = g + w2 v^2 <= Fmax computed
    with 3 roundings; each side is off by at most 9 * 2^-53 * Fmax * (its index difference), their difference D by at
    most 10 * 2^-53 * Fmax * (q - va) with second-order terms, and a parabola b dropped or kept against the sign of D
    costs at most |D| / (q - va) <= 10 * 2^-53 * Fmax at any t (a - b and q - b are linear in t and cross at that
    height).  A chain of such near-ties is no longer than the line, Fmax <= the squared diagonal of the volume (with
    its float32 roundings), and there are two envelope passes."""
    rel = (1 + U32) ** 3 * (1 + U64) ** 20 - 1 + ((1 + U64) ** 4 - 1)
    diag2 = sum((float(s) * (n - 1)) ** 2 for s, n in zip(sp, shape)) * (1 + U32) ** 3
    return rel * want + 2 * 10 * U64 * diag2 * max(shape)


@pytest.mark.parametrize("shape, spacing", lim.ANISO_CASES)
def test_edt_other_spacings_within_the_derived_bound(shape, spacing):
    lab = lim.aniso_volume(shape)
    sp = tuple(float(np.float32(s)) for s in spacing)            # what the kernel receives
    for feature in (0, 1):
        got = _edt(lab, 5, feature, sp)
        want, sign = ref.signed_edt_sq(lab, 5, feature, sp)
        assert np.array_equal(np.signbit(got), sign)
        got = np.abs(got).astype(np.float64)
        assert np.isfinite(want).all() and np.array_equal(got == 0, want == 0)
        bound = _aniso_bound(want, shape, sp)
        err = np.abs(got - want)
        nz = want > 0
        print(f"edt {shape} at {spacing} feature {feature}: error at most {float((err[nz] / bound[nz]).max()):.4f} "
              f"of the derived bound ({float((bound[nz] / want[nz]).max()):.3e} relative at most)")
        assert (err <= bound).all()


@pytest.mark.parametrize("dtype", lim.LABEL_TYPES)
@pytest.mark.parametrize("kind, box", [("block", lim.CUT_BOX), ("border", lim.BORDER_BOX)])
def test_edt_on_a_box_that_cuts_through_the_label(kind, box, dtype):
    """the feature set is contour(full volume)[box]: whether a voxel on a face of the box is contour depends on its
    neighbour outside the box, or on the volume's border being background"""
    lab = lim.cut_volume(kind)
    for feature in (0, 1):
        got = _edt(lab, 2, feature, UNIT, box, dtype)
        want, sign = ref.signed_edt_sq(lab, 2, feature, UNIT, box)
        assert np.array_equal(np.signbit(got), sign)
        assert np.array_equal(np.abs(got), want.astype(np.float32))


def test_edt_degenerate_boxes():
    lab = lim.cut_volume("block")
    for box in lim.THIN_BOXES:                                   # extent 1 along z, y, x
        for feature in (0, 1):
            got = _edt(lab, 2, feature, UNIT, box)
            want, sign = ref.signed_edt_sq(lab, 2, feature, UNIT, box)
            assert np.array_equal(np.signbit(got), sign) and np.array_equal(np.abs(got), want.astype(np.float32))
    solid = np.full(lim.CUT_SHAPE, 2, np.uint8)                  # the whole box inside the label
    inside = _edt(solid, 2, 1, UNIT, lim.CUT_BOX)
    assert np.isinf(inside).all() and np.signbit(inside).all()   # no contour in the box: -inf everywhere
    assert np.array_equal(_bits(_edt(solid, 2, 0, UNIT, lim.CUT_BOX)), np.zeros(inside.shape, np.uint32))
    for feature in (0, 1):                                       # a label value that is absent
        none = _edt(lab, 9, feature, UNIT, lim.CUT_BOX, "int16")
        assert np.isinf(none).all() and not np.signbit(none).any()


# ---------------------------------------------------------------------------- 3. sampler
def _sample(tgt, qry, label, query, box, dtype=None, calls=1, room=8):
    """the kernel's own signed map of `tgt` over the box (array order) and, per call on ONE workspace,
    (stats f64[4], values f32[queries + room] pre-filled with SENTINEL, n_values)"""
    T, Q = _t(tgt, dtype), _t(qry, dtype)
    box = _box3(tgt.shape, box)
    bd, bh, bw = _extents(box)
    dist = torch.empty(bd * bh * bw, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.edt_workspace_bytes(box), dtype=torch.uint8, device=DEV)
    ops.edt_sq(T, label, 1, box, UNIT, dist, ws)
    dist_np = dist.reshape(bd, bw, bh).permute(0, 2, 1).cpu().numpy()
    dist_np = dist_np if tgt.ndim == 3 else dist_np[0]
    cap = int((qry[ref.box_slices(box, qry.ndim)] == label).sum()) + room
    runs = []
    for _ in range(calls):
        stats = torch.full((4,), math.nan, dtype=torch.float64, device=DEV)
        vals = torch.full((cap,), SENTINEL, dtype=torch.float32, device=DEV)
        nv = torch.zeros(1, dtype=torch.int64, device=DEV)
        ops.edt_sample(dist, Q, label, query, box, stats, ws, vals, nv)
        runs.append((stats, vals, nv))
    bare = torch.full((4,), math.nan, dtype=torch.float64, device=DEV)
    ops.edt_sample(dist, Q, label, query, box, bare, ws)         # no values: the same sums in the same order
    assert np.array_equal(Q.cpu().numpy(), np.asarray(qry, Q.cpu().numpy().dtype))
    runs = [(s.cpu().numpy(), v.cpu().numpy(), int(n.cpu())) for s, v, n in runs]
    assert np.array_equal(_bits(bare.cpu().numpy()), _bits(runs[-1][0]))
    return dist_np, runs


def _check_sample(dist_np, run, qry, label, query, box, what):
    """count and max exact; sum and sum of squares within count * 2^-52 * sum|terms| of the exactly rounded sums
    (the bound of test_surfaces_gpu.py::test_measures: both sides add the same correctly rounded terms, only the
    order differs); the compacted values are the query values as a multiset, bit for bit"""
    stats, vals, nv = run
    d2 = ref.query_values(dist_np, qry, label, query, _box3(qry.shape, box))
    (n, s, q, mx), (es, eq) = ref.sample_stats(d2)
    assert stats[0] == n and nv == n, (what, stats[0], nv, n)
    assert stats[3] == mx, (what, stats[3], mx)
    assert abs(stats[1] - s) <= es and abs(stats[2] - q) <= eq, (what, stats, s, q)
    if n and s > 0:
        print(f"sampler {what}: n = {n}, sum off by {abs(stats[1] - s) / es:.3f}, squares by {abs(stats[2] - q) / eq:.3f} "
              f"of their bounds")
    assert np.array_equal(_bits(np.sort(vals[:n])), _bits(np.sort(d2))), what
    assert (vals[n:] == SENTINEL).all(), what
    return n, d2


@pytest.mark.parametrize("bw, dtype", list(zip(lim.SAMPLE_WIDTHS, ("uint8", "int16", "int32", "uint8"))))
@pytest.mark.parametrize("query", [0, 1])
def test_sampler_box_inside_a_volume(bw, dtype, query):
    """box widths 5, 64, 70, 130 against the 64-lane chunks; the query label sits on every voxel just outside each
    face of the box: none of them is counted, all of them decide which face voxels are contour"""
    tgt, qry, label, box = lim.sample_case(bw, dtype)
    dist_np, runs = _sample(tgt, qry, label, query, box, dtype)
    n, d2 = _check_sample(dist_np, runs[0], qry, label, query, box, f"bw {bw} {dtype} query {query}")
    inside = int((qry[ref.box_slices(box)] == label).sum())
    assert 0 < n <= inside < int((qry == label).sum()) and (n < inside) == bool(query)
    assert (d2 > 0).any() and (d2 == 0).any()


@pytest.mark.parametrize("query", [0, 1])
def test_sampler_2d_and_the_one_workgroup_grid(query):
    tgt, qry, label, box = lim.sample_case(70, "int16", 2)
    dist_np, runs = _sample(tgt, qry, label, query, box)
    assert _check_sample(dist_np, runs[0], qry, label, query, box, f"2-D query {query}")[0] > 0
    few = (0, 1, 2, 5, 2, 72)                                    # 3 rows: one workgroup, one idle wave
    dist_np, runs = _sample(tgt, qry, label, query, few)
    assert _check_sample(dist_np, runs[0], qry, label, query, few, f"2-D 3 rows query {query}")[0] > 0


def test_sampler_without_queries_in_the_box():
    tgt, qry, label, box = lim.sample_case(70, "uint8")
    empty = qry.copy()
    empty[ref.box_slices(box)] = 0                               # the label stays just outside every face
    assert (empty == label).sum() > 0
    for query in (0, 1):
        dist_np, runs = _sample(tgt, empty, label, query, box)
        stats, vals, nv = runs[0]
        assert stats.tolist() == [0.0, 0.0, 0.0, 0.0] and nv == 0 and (vals == SENTINEL).all()


def test_sampler_foreground_queries_inside_the_target():
    """query 0 with the target's own voxels as queries: interior voxels hold negative values and contour voxels
    -0.0; each contributes exactly 0"""
    tgt, _, label, box = lim.sample_case(64, "int32")
    dist_np, runs = _sample(tgt, tgt, label, 0, box)
    stats, vals, nv = runs[0]
    q = (tgt == label)[ref.box_slices(box)]
    stored = dist_np[q]
    assert np.signbit(stored).all() and (stored == 0).any()      # -0.0 on the contour
    assert stats.tolist() == [float(q.sum()), 0.0, 0.0, 0.0] and nv == q.sum()
    assert np.array_equal(_bits(vals[:nv]), np.zeros(nv, np.uint32)) and (vals[nv:] == SENTINEL).all()
    _check_sample(dist_np, runs[0], tgt, label, 0, box, "queries inside the target")


@pytest.mark.parametrize("query", [0, 1])
def test_sampler_second_trip_of_the_capped_grid(query):
    """4158 rows against 4 x kSampleWgs per trip; the largest distance belongs to the last row"""
    tgt, qry, label, box = lim.sample_trip_case()
    dist_np, runs = _sample(tgt, qry, label, query, box)
    _check_sample(dist_np, runs[0], qry, label, query, box, f"two trips query {query}")
    assert runs[0][0][3] == math.sqrt(65 ** 2 + 62 ** 2 + 4 ** 2)


def test_sampler_repeated_on_one_workspace():
    """three launches in a row share the partial table of one workspace: bit-identical statistics (fixed-order
    tail), the same values as a multiset, and every launch right (a ticket left non-zero would keep the next launch
    that draws it from ever finishing its statistics)"""
    tgt, qry, label, box = lim.sample_case(130, "int16")
    for query in (0, 1):
        dist_np, runs = _sample(tgt, qry, label, query, box, calls=3)
        for run in runs:
            _check_sample(dist_np, run, qry, label, query, box, f"repeat query {query}")
            assert np.array_equal(_bits(run[0]), _bits(runs[0][0]))
            assert np.array_equal(_bits(np.sort(run[1])), _bits(np.sort(runs[0][1])))


def test_sampler_tickets_come_back_to_zero():
    """every ticket drawn at least twice, on a grid of several workgroups, each launch into its own statistics row:
    when a ticket comes round again it must count from zero, or that launch never writes its row"""
    tgt, qry, label, box = lim.sample_case(5, "uint8")
    T, Q = _t(tgt), _t(qry)
    bd, bh, bw = _extents(box)
    assert bd * bh > 8                                           # more than two workgroups
    dist = torch.empty(bd * bh * bw, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.edt_workspace_bytes(box), dtype=torch.uint8, device=DEV)
    ops.edt_sq(T, label, 1, box, UNIT, dist, ws)
    launches = 2 * lim.SAMPLE_TICKETS + 9
    stats = torch.full((launches, 4), math.nan, dtype=torch.float64, device=DEV)
    for i in range(launches):
        ops.edt_sample(dist, Q, label, 1, box, stats[i], ws)
    got = stats.cpu().numpy()
    assert got[0, 0] == ref.contour(qry == label)[ref.box_slices(box)].sum() > 0
    assert np.array_equal(_bits(got), _bits(np.tile(got[0], (launches, 1))))


# ---------------------------------------------------------------------------- 4. select
def _select(buf, n, ranks, ws=None):
    """ops.select_f32 over the first n values of buf (n = 0: one stale value); returns the device tensor"""
    v = _t(np.asarray(buf, np.float32)) if len(buf) else torch.full((1,), 3.0, dtype=torch.float32, device=DEV)
    n_t = torch.tensor([n], dtype=torch.int64, device=DEV)
    r = torch.tensor(list(ranks), dtype=torch.int64, device=DEV)
    out = torch.full((len(ranks),), SENTINEL, dtype=torch.float32, device=DEV)
    if ws is None:
        ws = torch.empty(ops.select_workspace_bytes(len(ranks)), dtype=torch.uint8, device=DEV)
    ops.select_f32(v, n_t, r, out, ws)
    return out


def _check_select(buf, n, ranks, ws=None):
    got = _select(buf, n, ranks, ws).cpu().numpy()
    s = np.sort(np.asarray(buf, np.float32)[:n])
    want = s[np.clip(np.asarray(ranks), 0, n - 1)]
    assert np.array_equal(_bits(got), _bits(want)), (n, ranks, got, want)


def _spread(n):
    return sorted({0, n // 3, (n - 1) // 2, n // 2, n - 1})[:4]


@pytest.mark.parametrize("kind", ["middle", "low"])
def test_select_decided_by_the_later_passes(kind):
    """all values share the first digit (and, for "low", the second): the first histogram has one bin"""
    v = lim.select_bits(kind)
    n = len(v)
    _check_select(v, n, _spread(n))
    _check_select(v, n, [n // 2 - 1, n // 2])


@pytest.mark.parametrize("n", lim.SELECT_SIZES)
def test_select_around_one_stride_of_the_grid(n):
    v = lim.select_bits("any", n)
    _check_select(v, n, _spread(n))
    _check_select(v, n, [n - 1])


def test_select_equal_values_zeros_and_subnormals():
    _check_select(np.full(3000, 2.5, np.float32), 3000, [0, 1499, 1500, 2999])
    tiny = np.arange(0, 60, dtype=np.uint32).repeat(7).view(np.float32)       # 0 and the smallest subnormals
    tiny = np.random.default_rng(1).permutation(tiny)
    assert tiny.max() < np.finfo(np.float32).tiny
    _check_select(tiny, len(tiny), [0, 6, 7, len(tiny) - 1])
    _check_select(tiny, len(tiny), [200, 201])


def test_select_infinite_tails_and_a_count_below_the_buffer():
    """the two ways evaluation._run calls it: an +inf tail inside n that the ranks never reach, and n[0] smaller than
    the buffer with unrelated values behind it"""
    v = lim.select_bits("any", 4000)
    with_tail = np.concatenate([v[:1000], np.full(500, np.inf, np.float32), v[1000:]])
    n_fin = len(v)
    _check_select(with_tail, len(with_tail), [0, n_fin // 2 - 1, n_fin // 2, n_fin - 1])
    got = _select(with_tail, len(with_tail), [n_fin - 1, n_fin]).cpu().numpy()
    assert np.isfinite(got[0]) and got[1] == np.inf
    for junk in (0.0, np.inf, 1e-42):
        buf = np.concatenate([v[:1500], np.full(2500, junk, np.float32)])
        _check_select(buf, 1500, [0, 749, 750, 1499])
        _check_select(buf, 1, [0, 5])


def test_select_rank_counts_repeats_and_clamps():
    v = lim.select_bits("any", 777)
    n = len(v)
    for ranks in ([5], [5, 5], [0, n - 1, 0], [400, 400, 400, 400], [n - 1, 0, 388, 388]):
        _check_select(v, n, ranks)
    _check_select(v, n, [-5, n + 10])                            # clamped to the ends
    _check_select(v, n, [-1, n, n - 1, 0])
    assert np.isnan(_select(np.zeros(0, np.float32), 0, [0, 3]).cpu().numpy()).all()
    assert np.isnan(_select(v, 0, [0]).cpu().numpy()).all()


def test_select_refuses_five_ranks():
    ws = torch.empty(ops.select_workspace_bytes(4), dtype=torch.uint8, device=DEV)
    assert ops.select_workspace_bytes(5) == 0 and ops.select_workspace_bytes(0) == 0
    with pytest.raises(RuntimeError, match=r"select_f32: 1 <= n_ranks <= 4"):
        _select(lim.select_bits("any", 100), 100, [0, 1, 2, 3, 4], ws)


def test_select_back_to_back_on_one_workspace():
    """4, 1 and 3 ranks in a row on one workspace with nothing read in between: each call leaves the histograms it
    used cleared and the state of the ranks it does not use ignored"""
    ws = torch.empty(ops.select_workspace_bytes(4), dtype=torch.uint8, device=DEV).fill_(0xAB)
    a, b = lim.select_bits("any", 5000), lim.select_bits("middle")
    calls = [(a, [0, 1234, 2500, 4999]), (b, [2500]), (a, [17, 17, 4000]), (b, [0, 4999, 2499, 2500])]
    outs = [_select(v, len(v), r, ws) for v, r in calls]
    for (v, r), out in zip(calls, outs):
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(np.sort(v)[r]))


# ---------------------------------------------------------------------------- 5. confusion counts
def _confusion(pred, truth, k):
    p, t = _t(pred), _t(truth)
    cm = torch.full((k, k), -7, dtype=torch.int64, device=DEV)
    ops.confusion_counts(p, t, k, cm)
    assert np.array_equal(p.cpu().numpy(), pred) and np.array_equal(t.cpu().numpy(), truth)
    return cm.cpu().numpy()


def _want_confusion(pred, truth, k):
    p, t = pred.astype(np.int64), truth.astype(np.int64)
    ok = (p >= 0) & (p < k) & (t >= 0) & (t < k)
    return np.bincount(t[ok] * k + p[ok], minlength=k * k).reshape(k, k), int(ok.sum())


@pytest.mark.parametrize("k, dtype", lim.CONF_KS)
def test_confusion_counts_at_the_switch_and_the_cap(k, dtype):
    """k = 64 (the last LDS table), 65 (the first global one) and 4096 (the largest)"""
    pred, truth = lim.confusion_case(k, dtype)
    want, n_ok = _want_confusion(pred, truth, k)
    got = _confusion(pred, truth, k)
    assert n_ok == pred.size and np.array_equal(got, want)
    assert got[0, 0] > 0 and got[k - 1, k - 1] > 0 and got[0, k - 1] > 0 and got[k - 1, 0] > 0


def test_confusion_counts_refuses_a_table_past_the_cap():
    pred, truth = lim.confusion_case(64, "int32", 1000)
    cm = torch.zeros(16, dtype=torch.int64, device=DEV)
    for k in (4097, 0):
        with pytest.raises(RuntimeError, match=r"confusion_counts: 1 <= k <= 4096"):
            ops.confusion_counts(_t(pred), _t(truth), k, cm)


@pytest.mark.parametrize("dtype", lim.LABEL_TYPES)
def test_confusion_counts_second_trip_of_the_capped_grid(dtype):
    """1024 x 256 + 1000 elements: the cells of labels 20 .. 39 are filled by the tail alone"""
    pred, truth, k = lim.confusion_trip_case(dtype)
    want, n_ok = _want_confusion(pred, truth, k)
    got = _confusion(pred, truth, k)
    assert np.array_equal(got, want) and got[20:, 20:].sum() == 1000 and got[:20, 20:].sum() == 0 == got[20:, :20].sum()


@pytest.mark.parametrize("k, dtype", [(8, "uint8"), (100, "int16"), (65, "int32")])
def test_confusion_counts_every_voxel_in_one_cell(k, dtype):
    n = 100_000
    pred, truth = np.full(n, 5, dtype), np.full(n, 3, dtype)
    got = _confusion(pred, truth, k)
    want = np.zeros((k, k), np.int64)
    want[3, 5] = n
    assert np.array_equal(got, want)
    assert _confusion(pred[:1], truth[:1], k)[3, 5] == 1


@pytest.mark.parametrize("k, dtype", [(7, "uint8"), (7, "int16"), (70, "int16"), (70, "int32")])
def test_confusion_counts_skips_labels_out_of_range(k, dtype):
    rng = np.random.default_rng(k)
    n = 50_000
    skip = np.asarray(lim.out_of_range(dtype, k))
    both = rng.integers(0, k, (2, n))
    for a in both:
        junk = rng.random(n) < 0.1
        a[junk] = rng.choice(skip, int(junk.sum()))
    pred, truth = both[0].astype(dtype), both[1].astype(dtype)
    want, n_ok = _want_confusion(pred, truth, k)
    got = _confusion(pred, truth, k)
    assert 0.7 * n < n_ok < 0.9 * n and np.array_equal(got, want) and int(got.sum()) == n_ok
    with pytest.raises(ValueError, match="outside"):
        evaluation.confusion_matrix(k, pred, truth)
    ok = (pred.astype(np.int64) >= 0) & (pred.astype(np.int64) < k) & (truth.astype(np.int64) >= 0) & (truth.astype(np.int64) < k)
    assert np.array_equal(evaluation.confusion_matrix(k, pred[ok], truth[ok]), want.astype(np.float64))


# ---------------------------------------------------------------------------- 6. through evaluation.py
def _check_metrics(pred, truth, c, k, pct):
    """evaluation.surface_distances against ref.metrics at unit spacing, where every squared distance is an exact
    float32 integer and both sides take correctly rounded float64 square roots of the same numbers.

    max, hausdorff: the same number, equality.  percentile, median: np.percentile's lerp restated, at most 3
    roundings per side after the square roots: 8 * 2^-53 relative.  Means: sums of n terms in another order plus
    one division per side: (n + 2) * 2^-52 relative.  std: the package takes sqrt(sum d^2 / n - mean^2) where the sum of
    the integers d^2 is exact; the variance is off by at most E = 2 * (2 n + 6) * 2^-52 * sum d^2 / n on both sides
    together (mean^2 carries twice the mean's error, and mean^2 + var = sum d^2 / n), and |sqrt a - sqrt b| is at most
    sqrt|a - b| and at most |a - b| / sqrt b."""
    res = evaluation.surface_distances(pred, truth, num_classes=k, spacing=UNIT[3 - pred.ndim:], percentile=pct)
    m = ref.metrics(pred == c, truth == c, UNIT[3 - pred.ndim:], pct)
    a, b = pred == c, truth == c
    n_s = sum(m["n_surface"])
    n_p = int(a.sum() + b.sum())
    for key in ("surface_max", "pointwise_max", "hausdorff"):
        assert res[key][c] == m[key], key
    for key in ("percentile_hausdorff", "surface_median", "pointwise_median"):
        assert abs(res[key][c] - m[key]) <= 8 * U64 * m[key], (key, res[key][c], m[key])
    for key, n in (("surface_mean", n_s), ("pointwise_mean", n_p), ("average_hausdorff", n_p)):
        assert abs(res[key][c] - m[key]) <= (n + 2) * 2 * U64 * m[key], (key, res[key][c], m[key])
    for key, n in (("surface_std", n_s), ("pointwise_std", n_p)):
        mean, std = m[key.replace("std", "mean")], m[key]
        e = 2 * (2 * n + 6) * 2 * U64 * (mean * mean + std * std)
        bound = min(math.sqrt(e), e / std if std > 0 else math.inf) + 2 * U64 * std
        print(f"{key} n = {n}: {res[key][c]!r} vs {std!r}, {abs(res[key][c] - std) / bound if bound else 0:.3f} of the bound")
        assert abs(res[key][c] - std) <= bound, (key, res[key][c], std)
    assert res["n_pred"][c] == a.sum() and res["n_ref"][c] == b.sum()
    return res, m


@pytest.mark.parametrize("pct", [0.0, 37.5, 100.0])
def test_surface_distances_of_one_and_two_voxel_contours(pct):
    """percentile and median at n = 1 and n = 2: ranks lo + 1 = n must clamp, and the median ranks coincide"""
    shape = (8, 9, 12)
    one_p, one_r = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    one_p[2, 3, 4] = 1
    one_r[5, 3, 8] = 1
    res, m = _check_metrics(one_p, one_r, 1, 2, pct)
    assert m["n_surface"] == (1, 1) and res["percentile_hausdorff"][1] == 5.0 == res["surface_median"][1]
    assert res["surface_std"][1] == 0.0 and res["pointwise_mean"][1] == 5.0
    two_p = one_p.copy()
    two_p[6, 7, 1] = 1
    res, m = _check_metrics(two_p, one_r, 1, 2, pct)
    assert m["n_surface"] == (2, 1)
    far = math.sqrt(1 + 16 + 49)
    assert res["percentile_hausdorff"][1] == pytest.approx(5.0 + (far - 5.0) * pct / 100.0, rel=8 * U64)
    flat_p, flat_r = np.zeros((9, 12), np.int16), np.zeros((9, 12), np.int16)
    flat_p[3, 4] = flat_p[7, 1] = 1
    flat_r[3, 8] = flat_r[0, 0] = 1
    assert _check_metrics(flat_p, flat_r, 1, 2, pct)[1]["n_surface"] == (2, 2)


@pytest.mark.parametrize("pct", [0.0, 37.5, 100.0])
def test_surface_distances_of_a_label_inside_its_reference(pct):
    """pred's label lies wholly inside ref's: every point-wise distance from pred is 0, the other direction is not"""
    truth = np.zeros((10, 12, 14), np.uint8)
    pred = np.zeros((10, 12, 14), np.uint8)
    truth[2:8, 2:9, 3:12] = 2
    pred[3:6, 3:6, 4:8] = 2
    pred[0, 0, 0] = 1                                             # a bystander in pred only
    res, m = _check_metrics(pred, truth, 2, 3, pct)
    n_in, n_out = int((pred == 2).sum()), int((truth == 2).sum())
    out_mean = m["pointwise_mean"] * (n_in + n_out) / n_out      # the mean of the non-zero direction alone
    assert res["average_hausdorff"][2] == pytest.approx(0.5 * out_mean, rel=(n_out + 4) * 2 * U64)
    assert res["pointwise_median"][2] == m["pointwise_median"] and res["hausdorff"][2] > 1
    assert math.isnan(res["surface_mean"][1]) and res["n_pred"][1] == 1 and res["n_ref"][1] == 0


def test_surface_distances_of_mixed_label_types():
    """uint8 against int16: both are read as int32, and the result is that of either type alone"""
    rng = np.random.default_rng(8)
    shape = (9, 10, 11)
    pred = (rng.random(shape) < 0.3).astype(np.uint8) * 2
    truth = (rng.random(shape) < 0.3).astype(np.int16) * 2
    res, _ = _check_metrics(pred, truth, 2, 3, 37.5)
    same = evaluation.surface_distances(pred.astype(np.int32), truth.astype(np.int32), num_classes=3, spacing=UNIT,
                                        percentile=37.5)
    for key in res:
        assert np.array_equal(res[key], same[key], equal_nan=True), key
    swapped = evaluation.surface_distances(pred.astype(np.int16), truth.astype(np.uint8), num_classes=3, spacing=UNIT,
                                           percentile=37.5)
    for key in res:
        assert np.array_equal(res[key], swapped[key], equal_nan=True), key
