"""The row reductions and BatchNorm passes of norm_act.hip and the two finalisations behind them
(collapse_fin_kernel, fin_tail_run) against float64 references, on inputs whose sums are EXACT
(tests/helpers/reduce_cases.py): small integers and dyadic parameters, so that every term, every f32 partial row and
every float64 column sum is representable in any order of summation and the device has to return the reference's
numbers bit for bit.  tests/test_reduce_fin_host.py holds the preconditions (exactness in every storage type, partial
sums below 2^24 units of their grid, every case on the path it was built for); nothing here may be loosened when a
generator breaks them.

Values that one rounded operation defines on exact sums (mean, coef, dgamma, dbeta, dalpha, the bias gradient, y, dx)
are compared with ==.  Values that take several operations, which the compiler may contract (invstd, scale, shift, the
running statistics, bn_eval_affine), are held to the bounds derived in the docstrings of reduce_cases.bn_finalize_ref
and reduce_cases.eval_affine_ref.  Every launch runs twice and has to repeat itself bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from tests.helpers import reduce_cases as rc  # noqa: E402

DEV = "cuda:0"
L = rc.read_limits()
TORCH = {rc.F32: torch.float32, rc.BF16: torch.bfloat16, rc.F16: torch.float16}
SENTINEL = 77.0          # exact in every storage type; what a wider buffer holds outside a view
NAN = float("nan")
MOMENTUM, EPS = 0.1, 1e-5


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)        # a copy: the helper's arrays are read-only


def host(t) -> np.ndarray:
    return t.detach().to(torch.float64).cpu().numpy()


def nan_like(*sizes):
    return [torch.full(s if isinstance(s, tuple) else (s,), NAN, device=DEV) for s in sizes]


def view_of(case, a, dtype):
    """(buffer [1, d, h, w, buf_c] holding SENTINEL outside channels ch0 .. ch0 + c, the NDHWC view of those
    channels holding `a` [n_vox, c], or SENTINEL when a is None)"""
    buf = torch.full((1,) + case.sp + (case.buf_c,), SENTINEL, device=DEV, dtype=TORCH[dtype])
    view = buf[..., case.ch0:case.ch0 + case.c]
    if a is not None:
        view.copy_(dev(a).reshape(view.shape))
    return buf, view


def expect_buffer(case, ref):
    """float64 [n_vox, buf_c]: what view_of's buffer must hold once the view has been written with ref"""
    out = np.full((rc.nvox(case), case.buf_c), SENTINEL)
    out[:, case.ch0:case.ch0 + case.c] = ref
    return out


def case_params(d):
    return [dev(a) for a in (d.mean, d.invstd, d.gamma, d.beta)]


def cases_by_dtype(cases):
    return [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in cases for dt in c.dtypes]


# ------------------------------------------------------------------ 1. the two finalisations on synthetic tables
def upload_table(a: np.ndarray, aligned: bool):
    """the [rows + reserve][width] f32 buffer the finalisations take, NaN behind the real rows (nothing may read the
    reserve before writing it); misaligned: a view one float into a larger allocation"""
    rows, width = a.shape
    total = (rows + L.reserve_rows) * width
    buf = torch.full((total + 4,), NAN, device=DEV)
    tbl = buf[0:total] if aligned else buf[1:1 + total]
    assert (tbl.data_ptr() % 16 == 0) == aligned
    tbl[:rows * width] = dev(a).reshape(-1)
    return buf, tbl, rows + L.reserve_rows


def run_bn_finalize(tbl, rows_arg, c, count, g, b, rm, rv):
    mean, invstd, scale, shift = nan_like(c, c, c, c)
    rmd, rvd = dev(rm), dev(rv)
    ops.bn_finalize(tbl, rows_arg, c, count, dev(g), dev(b), rmd, rvd, MOMENTUM, EPS, mean, invstd, scale, shift)
    torch.cuda.synchronize()
    return {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "running_mean": rmd, "running_var": rvd}


def check_bn_finalize(got, again, ref):
    for name, (want, bound) in ((k, v) for k, v in ref.items() if isinstance(v, tuple)):
        g = host(got[name])
        assert torch.equal(got[name], again[name]), f"{name} does not repeat itself"
        if bound is None:
            bad = np.flatnonzero(g != want.astype(np.float64))
            assert bad.size == 0, f"{name}: {bad.size} channels differ, first {bad[:4]}: {g[bad[:4]]} != {want[bad[:4]]}"
        else:
            r = np.abs(g - want) / bound
            assert np.isfinite(g).all() and float(r.max()) <= 1.0, \
                f"{name}: worst |error| / bound = {float(r.max()):.3g} at channel {int(r.argmax())}"


@pytest.mark.parametrize("t", [t for t in rc.TABLES if t.width % 2 == 0], ids=lambda t: t.name)
def test_bn_finalize_folds_a_synthetic_table_exactly(t):
    """collapse_fin_kernel + BnFin on a [rows][2][c] table of integers up to 2^20: `mean` is exactly the f32 cast of
    the float64 quotient of the exact column sum; invstd, scale, shift and the running statistics within the bounds of
    reduce_cases.bn_finalize_ref.  Channel 1 has a negative variance before the clamp."""
    a, c = rc.table(t.name), t.width // 2
    g, b, rm, rv = rc.bn_params(c, t.seed)
    _, tbl, rows_arg = upload_table(a, t.aligned)
    ref = rc.bn_finalize_ref(rc.table_sums(a), c, rc.TABLE_COUNT, g, b, rm, rv, MOMENTUM, EPS)
    got = run_bn_finalize(tbl, rows_arg, c, rc.TABLE_COUNT, g, b, rm, rv)
    again = run_bn_finalize(tbl, rows_arg, c, rc.TABLE_COUNT, g, b, rm, rv)
    check_bn_finalize(got, again, ref)
    assert torch.equal(tbl[:a.size].reshape(a.shape), dev(a))            # the rows themselves are only read


def test_bn_finalize_with_a_count_of_one_skips_the_unbiased_factor():
    a = rc.count1_table()
    c = a.shape[1] // 2
    g, b, rm, rv = rc.bn_params(c, 1)
    _, tbl, rows_arg = upload_table(a, True)
    ref = rc.bn_finalize_ref(rc.table_sums(a), c, 1.0, g, b, rm, rv, MOMENTUM, EPS)
    assert (ref["var"] > 1000).sum() == c - 1 and ref["var"][1] < 0
    got, again = (run_bn_finalize(tbl, rows_arg, c, 1.0, g, b, rm, rv) for _ in range(2))
    check_bn_finalize(got, again, ref)


@pytest.mark.parametrize("t", [t for t in rc.TABLES if t.width % 3 == 0], ids=lambda t: t.name)
def test_bn_act_bwd_finalize_folds_a_synthetic_table_exactly(t):
    """collapse_fin_kernel + BnBwdFin on a [rows][3][c] table: dgamma, dbeta, dalpha (the fixed-order sum over
    channels, at channel counts that are no multiple of 256 too) and coef are f32 casts of exact float64 values"""
    a, c = rc.table(t.name), t.width // 3
    _, tbl, rows_arg = upload_table(a, t.aligned)
    ref = rc.bn_bwd_finalize_ref(rc.table_sums(a), c, rc.TABLE_COUNT)

    def run():
        dg, db, da, coef = nan_like(c, c, 1, (2, c))
        ops.bn_act_bwd_finalize(tbl, rows_arg, c, rc.TABLE_COUNT, None, None, dg, db, da, coef)
        torch.cuda.synchronize()
        return {"dgamma": dg, "dbeta": db, "dalpha": da, "coef": coef}

    got, again = run(), run()
    check_bwd_outputs(got, again, ref)


def check_bwd_outputs(got, again, ref, names=("dgamma", "dbeta", "dalpha", "coef")):
    for name in names:
        g, want = host(got[name]), np.asarray(ref[name], np.float64).reshape(got[name].shape)
        assert torch.equal(got[name], again[name]), f"{name} does not repeat itself"
        bad = np.argwhere(g != want)
        assert len(bad) == 0, f"{name}: {len(bad)} values differ, first at {bad[0]}: {g[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


def test_a_table_that_is_not_integer_valued_against_fsum():
    """random f32 rows over six decades, count = 1, so that `mean` is the f32 cast of the column sum: both stages add
    in float64, rows - 1 additions per column, each within 2^-53 of a partial sum bounded by the sum of |v|; the cast
    adds half an f32 ulp"""
    a, want, mag = rc.fsum_table()
    c = a.shape[1] // 2
    g, b, rm, rv = rc.bn_params(c, 2)
    _, tbl, rows_arg = upload_table(a, True)
    got, again = (run_bn_finalize(tbl, rows_arg, c, 1.0, g, b, rm, rv) for _ in range(2))
    assert torch.equal(got["mean"], again["mean"])
    m = host(got["mean"])
    bound = a.shape[0] * 2.0 ** -53 * mag[:c]
    bound = bound + 0.5 * np.spacing((np.abs(want[:c]) + bound).astype(np.float32)).astype(np.float64)
    r = np.abs(m - want[:c]) / bound
    assert float(r.max()) <= 1.0, f"worst |error| / bound = {float(r.max()):.3g}"


# ------------------------------------------------------------------ 2. the producers: rows and totals
def check_rows(part, real_rows, terms, grids, what):
    """part [rows, k, c] f32 of the device: every entry of the real rows a multiple of its term's grid, the float64
    column totals equal to the reference's exactly"""
    rows = host(part[:real_rows])
    assert np.isfinite(rows).all(), what
    for k, (t, g) in enumerate(zip(terms, grids)):
        assert rc.on_grid(rows[:, k], g), f"{what}: term {k} has row entries off its grid of {g}"
        got, want = rows[:, k].sum(0), t.sum(0)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: term {k}: {bad.size} channel totals differ, first channel {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("case,dtype", cases_by_dtype(rc.STATS_CASES))
def test_bn_stats_and_bias_grad_rows_and_totals(case, dtype):
    """sum x and sum x^2 per channel from bn_stats (then the exact mean through bn_finalize) and the same tensor
    through bias_grad, whose db must be the f32 cast of the exact sum"""
    n, c = rc.nvox(case), case.c
    d = rc.act_inputs(case.seed, n, c)
    terms, grids = rc.stats_terms(d.x)
    buf, xv = view_of(case, d.x, dtype)
    before = buf.clone()
    rows_arg = ops.bn_stats_rows(xv)
    assert rows_arg - L.reserve_rows == case.want["rows"] == rc.stats_path(case, xv.element_size(), L)["rows"]

    def stats():
        part = torch.full((rows_arg, 2, c), NAN, device=DEV)
        ops.bn_stats(xv, part)
        torch.cuda.synchronize()
        return part

    part, part2 = stats(), stats()
    assert torch.equal(part[:case.want["rows"]], part2[:case.want["rows"]])
    check_rows(part, case.want["rows"], terms, grids, "bn_stats")
    sums = np.concatenate([t.sum(0) for t in terms])
    g, b, rm, rv = rc.bn_params(c, case.seed)
    ref = rc.bn_finalize_ref(sums, c, n, g, b, rm, rv, MOMENTUM, EPS)
    check_bn_finalize(run_bn_finalize(part, rows_arg, c, n, g, b, rm, rv),
                      run_bn_finalize(part2, rows_arg, c, n, g, b, rm, rv), ref)

    def bias():
        ws = torch.full((rows_arg, 2, c), NAN, device=DEV)
        db, = nan_like(c)
        ops.bias_grad(xv, db, ws)
        torch.cuda.synchronize()
        return db, ws

    (db, ws), (db2, _) = bias(), bias()
    assert torch.equal(db, db2)
    check_rows(ws, case.want["rows"], terms, grids, "bias_grad")
    want = terms[0].sum(0).astype(np.float32).astype(np.float64)
    bad = np.flatnonzero(host(db) != want)
    assert bad.size == 0, f"db: {bad.size} channels differ, first {bad[0]}: {host(db)[bad[0]]} != {want[bad[0]]}"
    assert torch.equal(buf, before)


@functools.lru_cache(maxsize=None)
def bwd_reference(seed, n, c, mode):
    d = rc.act_inputs(seed, n, c)
    alpha, mask, drop = rc.mode_args(mode, n, c)
    terms, grids = rc.bwd_terms(d, alpha, mask)
    sums = np.concatenate([t.sum(0) for t in terms])
    return terms, grids, rc.bn_bwd_finalize_ref(sums, c, n), alpha, drop


@pytest.mark.parametrize("mode", rc.MODES)
@pytest.mark.parametrize("case,dtype", cases_by_dtype(rc.REDUCE_CASES))
def test_bn_act_bwd_reduce_rows_totals_and_both_finalisations(case, dtype, mode):
    """sum dz, sum dz xhat, sum dy z [z <= 0] from bn_act_bwd_reduce: finalised by its own last workgroup
    (fin_tail_run) and by bn_act_bwd_finalize (collapse_fin_kernel), both exact"""
    n, c = rc.nvox(case), case.c
    d = rc.act_inputs(case.seed, n, c)
    terms, grids, ref, alpha, drop = bwd_reference(case.seed, n, c, mode)
    (_, xv), (_, dyv) = view_of(case, d.x, dtype), view_of(case, d.dy, dtype)
    mean, invstd, gamma, beta = case_params(d)
    ad = torch.full((1,), alpha, device=DEV) if alpha is not None else None
    rows_arg = ops.bn_act_bwd_rows(xv)
    real = case.want["rows"]
    assert rows_arg - L.reserve_rows == real == rc.stats_path(case, xv.element_size(), L)["rows"]

    def run(fin):
        part = torch.full((rows_arg, 3, c), NAN, device=DEV)
        dg, db, da, coef = nan_like(c, c, 1, (2, c))
        ops.bn_act_bwd_reduce(dyv, xv, mean, invstd, gamma, beta, ad, part, dropout=drop,
                              fin=(n, dg, db, da, coef) if fin else None)
        if not fin:
            ops.bn_act_bwd_finalize(part, rows_arg, c, n, gamma, invstd, dg, db, da, coef)
        torch.cuda.synchronize()
        return part, {"dgamma": dg, "dbeta": db, "dalpha": da, "coef": coef}

    for fin in (False, True):
        (part, got), (part2, again) = run(fin), run(fin)
        assert torch.equal(part[:real], part2[:real])
        check_rows(part, real, terms, grids, f"bn_act_bwd_reduce (fin={fin})")
        check_bwd_outputs(got, again, ref)


def test_bn_act_bwd_reduce_refuses_257_channels():
    c = rc.REDUCE_REFUSED_C
    x = torch.zeros((1, 2, 2, 2, c), device=DEV)
    p = torch.zeros(c, device=DEV)
    part = torch.zeros((ops.bn_act_bwd_rows(x), 3, c), device=DEV)
    with pytest.raises(RuntimeError, match="bn_act_bwd_reduce: at most 256 channels per call"):
        ops.bn_act_bwd_reduce(x, x, p, p, p, p, None, part)


@pytest.mark.parametrize("dtype", rc.ALL)
@pytest.mark.parametrize("with_alpha", [True, False], ids=["prelu", "plain"])
@pytest.mark.parametrize("c,sp,n,seed", rc.FUSED_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_bn_act_bwd_fused_sums_and_dx(c, sp, n, seed, with_alpha, dtype):
    """the one-launch backward: exact sums and outputs, and dx exactly the two f32 roundings of
    reduce_cases.dx_f32_ref on the coef its own sums give, rounded once more to the storage type"""
    nv = n * sp[0] * sp[1] * sp[2]
    d = rc.act_inputs(seed, nv, c)
    terms, grids, ref, alpha, _ = bwd_reference(seed, nv, c, "prelu" if with_alpha else "plain")
    xd, dyd = (dev(a, TORCH[dtype]).reshape((n,) + sp + (c,)) for a in (d.x, d.dy))
    mean, invstd, gamma, beta = case_params(d)
    ad = torch.full((1,), alpha, device=DEV) if with_alpha else None
    dx_buf = torch.empty_like(xd)
    assert ops.bn_act_bwd_fused_ok(dyd, xd, dx_buf)
    rows_arg, wgs = ops.bn_act_bwd_fused_rows(xd), ops.bn_act_bwd_fused_wgs(xd)
    assert 1 <= wgs <= rows_arg - L.reserve_rows

    def run():
        part = torch.zeros((rows_arg, 3, c), device=DEV)
        dg, db, da, coef = nan_like(c, c, 1, (2, c))
        dx = torch.full_like(xd, NAN)
        ops.bn_act_bwd_fused(dyd, xd, dx, mean, invstd, gamma, beta, ad, part, (nv, dg, db, da if with_alpha else None, coef))
        torch.cuda.synchronize()
        return part, dx, {"dgamma": dg, "dbeta": db, "dalpha": da, "coef": coef}

    (part, dx, got), (part2, dx2, again) = run(), run()
    assert torch.equal(part[:wgs], part2[:wgs]) and torch.equal(dx, dx2)
    check_rows(part, wgs, terms, grids, "bn_act_bwd_fused")
    # without a slope dalpha is not passed and not written
    check_bwd_outputs(got, again, ref, ("dgamma", "dbeta", "dalpha", "coef") if with_alpha else ("dgamma", "dbeta", "coef"))
    want = rc.roundtrip(rc.dx_f32_ref(d, ref["coef"], alpha, None), dtype)
    assert torch.equal(dx.reshape(nv, c).to(torch.float64), dev(want, torch.float64))


# ------------------------------------------------------------------ 3. the element-wise passes
BIG_OPS = ("fwd-prelu-res", "fwd-plain", "fwd-dropout-res", "fwd-dropout", "add", "apply-prelu", "apply-plain",
           "apply-dropout", "cast-up", "cast-down", "cast-same")


@functools.lru_cache(maxsize=None)
def ew_reference(seed, n, c, op):
    """f32 [n, c] of the exact reference of one element-wise op (exact in f32: the host test)"""
    d, e = rc.act_inputs(seed, n, c), rc.ew_inputs(seed, n, c)
    kind, _, rest = op.partition("-")
    if kind == "fwd":
        alpha, mask, _ = rc.mode_args(rest.split("-")[0], n, c)
        ref = rc.fwd_ref(d.x, e.scale, e.shift, alpha, mask, e.res if rest.endswith("res") else None)
    elif kind == "add":
        ref = rc.fwd_ref(d.x, None, None, None, None, e.res)
    elif kind == "apply":
        alpha, mask, _ = rc.mode_args(rest, n, c)
        ref = rc.dx_ref(d, e.coef, alpha, mask)
    else:
        ref = d.x.astype(np.float64)
    out = ref.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), ref)
    out.setflags(write=False)
    return out


def run_ew(case, dtype, op):
    """one element-wise op on views of `case`; returns (output buffer as float64 [n_vox, buf_c] twice, reference)"""
    n, c = rc.nvox(case), case.c
    d, e = rc.act_inputs(case.seed, n, c), rc.ew_inputs(case.seed, n, c)
    kind, _, rest = op.partition("-")
    ins = []

    def inp(a, dt=dtype):
        buf, v = view_of(case, a, dt)
        ins.append((buf, buf.clone()))
        return v

    outs = []
    for _ in range(2):
        if kind == "fwd":
            mode = rest.split("-")[0]
            alpha, _, drop = rc.mode_args(mode, n, c)
            ad = torch.full((1,), alpha, device=DEV) if alpha is not None else None
            obuf, ov = view_of(case, None, dtype)
            ops.bn_act_fwd(inp(d.x), ov, dev(e.scale), dev(e.shift), ad, inp(e.res) if rest.endswith("res") else None,
                           dropout=drop)
        elif kind == "add":
            obuf, ov = view_of(case, None, dtype)
            ops.add(inp(d.x), inp(e.res), ov)
        elif kind == "apply":
            alpha, _, drop = rc.mode_args(rest, n, c)
            ad = torch.full((1,), alpha, device=DEV) if alpha is not None else None
            obuf, ov = view_of(case, None, dtype)
            ops.bn_act_bwd_apply(inp(d.dy), inp(d.x), ov, *case_params(d), ad, dev(e.coef), dropout=drop)
        else:       # cast_copy between f32 and the storage type
            src, dst = {"down": (rc.F32, dtype), "up": (dtype, rc.F32), "same": (dtype, dtype)}[rest]
            obuf, ov = view_of(case, None, dst)
            ops.cast_copy(inp(d.x, src), ov)
        torch.cuda.synchronize()
        outs.append(obuf)
    for buf, before in ins:
        assert torch.equal(buf, before), f"{op}: an input buffer was written"
    assert torch.equal(outs[0], outs[1]), f"{op} does not repeat itself"
    return outs[0], ew_reference(case.seed, n, c, op)


def check_ew(case, got_buf, ref, op):
    want = dev(expect_buffer(case, ref.astype(np.float64)), torch.float64)
    got = got_buf.reshape(-1, case.buf_c).to(torch.float64)
    bad = (got != want).nonzero()
    assert len(bad) == 0, (f"{op}: {len(bad)} elements differ, first (voxel, buffer channel) {bad[0].tolist()}: "
                           f"{float(got[tuple(bad[0])])} != {float(want[tuple(bad[0])])}")


@pytest.mark.parametrize("op", BIG_OPS)
@pytest.mark.parametrize("dtype", rc.ALL)
def test_elementwise_passes_past_one_grid_pass(dtype, op):
    """16 channels at 70 x 64 x 64: 1 146 880 four-channel groups against one pass of kEwCap x 256, so the
    grid-stride loop takes a second, partial pass (cast_copy works element by element: five passes)"""
    buf, ref = run_ew(rc.EW_BIG, dtype, op)
    check_ew(rc.EW_BIG, buf, ref, op)


@pytest.mark.parametrize("op", BIG_OPS)
@pytest.mark.parametrize("case,dtype", cases_by_dtype(rc.EW_VIEWS))
def test_elementwise_passes_on_strided_and_misaligned_views(case, dtype, op):
    """inputs and output as channel slices of wider buffers (or 3 channels: the scalar kernels); the bytes of the
    output buffer outside the view stay as they were"""
    buf, ref = run_ew(case, dtype, op)
    check_ew(case, buf, ref, op)


@pytest.mark.parametrize("c", rc.EVAL_AFFINE_C)
def test_bn_eval_affine_against_float64(c):
    g, b, rm, rv = rc.bn_params(c, 600 + c)
    (scale, sb), (shift, hb) = rc.eval_affine_ref(g, b, rm, rv, EPS)

    def run(gamma, beta):
        s, h = nan_like(c, c)
        ops.bn_eval_affine(gamma, beta, dev(rm), dev(rv), EPS, s, h)
        torch.cuda.synchronize()
        return s, h

    (s, h), (s2, h2) = run(dev(g), dev(b)), run(dev(g), dev(b))
    assert torch.equal(s, s2) and torch.equal(h, h2)
    for name, got, want, bound in (("scale", s, scale, sb), ("shift", h, shift, hb)):
        r = np.abs(host(got) - want) / bound
        assert float(r.max()) <= 1.0, f"{name}: worst |error| / bound = {float(r.max()):.3g}"
    # no affine parameters: gamma = 1, beta = 0
    one, zero = np.ones(c, np.float32), np.zeros(c, np.float32)
    (scale, sb), (shift, hb) = rc.eval_affine_ref(one, zero, rm, rv, EPS)
    s, h = run(None, None)
    assert float((np.abs(host(s) - scale) / sb).max()) <= 1.0 and float((np.abs(host(h) - shift) / hb).max()) <= 1.0
