"""CPU half of the inference data-path sweep: the references of tests/helpers/infer_ref.py agree with the existing
oracles, every gate of tests/test_infer_sweep_gpu.py rejects a wrong implementation (the references computed under a
switchable fault, on the sweep's own inputs), and the case tables meet the conditions they state."""
import numpy as np
import pytest
import torch

from oracle.resample_ref import ref_resample_grid
from oracle.sliding_ref import ref_sliding_window_inference
from tests.helpers import infer_ref as R


def case(name):
    return next(c for c in R.BLEND_CASES if c.name == name)


def blend_pair(c, fault=None, gate=False):
    """(violations of the faulty reference against the true one) through the GPU file's comparison function"""
    cache, per_dim, wins, imp = R.blend_inputs(c)
    _, g = R.lanes_per_voxel(c.k, c.dtype)
    l, cn, lab, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), c.roi, c.image, imp)
    ref = {"logits": l, "count": cn, "labels": lab}
    if fault is None:
        got = ref
    else:
        with R.fault(fault):
            fl, fc, flab, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), c.roi, c.image, imp, g=g)
        got = {"logits": fl, "count": fc, "labels": flab}
    f64 = None
    if gate:
        l64, c64, _, sabs, cover = R.blend_ref(cache, per_dim, 0, len(wins), c.roi, c.image, imp, dtype=np.float64)
        f64 = (l64, R.gaussian_bound(sabs, c64, cover))
    return R.blend_violations(got, ref, f64)


# ------------------------------------------------------------------------------------------------ cross-checks
@pytest.mark.parametrize("name,mode", [("two-0.5", "constant"), ("clamped-0.5", "constant"), ("padded-bf16", "constant"),
                                       ("two-0.5-gauss", "gaussian"), ("clamped-0.5-gauss", "gaussian"),
                                       ("padded", "gaussian")])
def test_blend_reference_equals_the_sliding_window_oracle(name, mode):
    c = case(name)
    cache, per_dim, wins, imp = R.blend_inputs(c)
    cache = np.nan_to_num(cache)
    index = {}

    def predictor(x):      # the oracle hands the windows over in schedule order: answer with the cache's entries
        out = []
        for _ in range(x.shape[0]):
            out.append(torch.from_numpy(cache[len(index)]).permute(3, 0, 1, 2))
            index[len(index)] = 1
        return torch.stack(out)

    ref, cnt, wins_o = ref_sliding_window_inference(torch.zeros((1, 1) + c.image), c.roi, 4, predictor, c.overlap, mode)
    assert len(wins_o) == len(wins)
    l, cn, lab, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), c.roi, c.image, imp)
    want = ref[0].permute(1, 2, 3, 0).numpy()
    assert np.array_equal(cn, cnt[0, 0].numpy())
    if mode == "constant":
        assert np.array_equal(l, want)
    else:
        l64, c64, _, sabs, cover = R.blend_ref(cache, per_dim, 0, len(wins), c.roi, c.image, imp, dtype=np.float64)
        assert np.all(np.abs(want.astype(np.float64) - l64) <= R.gaussian_bound(sabs, c64, cover))
        assert np.all(np.abs(l.astype(np.float64) - l64) <= R.gaussian_bound(sabs, c64, cover))
        assert np.array_equal(l, want)       # torch's `w * pred` then `+=` is the product-rounded sequence too
    assert np.array_equal(lab, torch.argmax(ref, 1)[0].numpy())


def test_f32_blend_reference_meets_the_float64_gate_on_every_gaussian_case():
    """a condition on the inputs, independent of any kernel: the product-rounded f32 sequence itself lies inside
    (n_cover + 2) * 2^-24 * sum|w p| / count around the float64 twin (see BLEND_SEED in infer_ref)"""
    worst = 0.0
    for c in R.BLEND_CASES:
        if not c.gaussian:
            continue
        cache, per_dim, wins, imp = R.blend_inputs(c)
        l, _, _, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), c.roi, c.image, imp)
        l64, c64, _, sabs, cover = R.blend_ref(cache, per_dim, 0, len(wins), c.roi, c.image, imp, dtype=np.float64)
        bound = R.gaussian_bound(sabs, c64, cover)
        err = np.abs(l.astype(np.float64) - l64)
        assert not (err > bound).any(), c.name
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    assert 0.5 < worst < 1.0      # the gate is tight for the reference itself: it cannot hide more than a rounding or two


def test_argmax_reference_equals_torch():
    for k in (1, 2, 5, 64):
        lg = R.argmax_logits((3, 7, 11), k, 40 + k)
        assert np.array_equal(R.argmax_ref(lg), torch.argmax(torch.from_numpy(lg), -1).numpy())


@pytest.mark.parametrize("nearest", [False, True])
def test_resample_reference_equals_the_itk_oracle(nearest):
    rng = np.random.default_rng(7)
    arr = rng.standard_normal((9, 11, 13)).astype(np.float32)
    lab = rng.integers(0, 200, (9, 11, 13)).astype(np.uint8)
    sp_in, sp_out, size = (0.5, 0.6, 0.7), (0.3, 0.45, 0.4), (20, 15, 19)
    m = R.index_map(sp_in, (1, 2, 3), np.eye(3), sp_out, (1, 2, 3), np.eye(3))
    for a in (arr, lab):
        want = ref_resample_grid(a, sp_in, (1, 2, 3), np.eye(3), size, sp_out, (1, 2, 3), np.eye(3), nearest)
        got = R.resample_ref(a, m, size[::-1], nearest=nearest)
        real = R.resample_ref(a, m, size[::-1], nearest=nearest, return_real=True)
        assert not R.resample_violations(got, want, real, nearest)
    # oblique geometry handed to the oracle directly: the composed 3x4 map gives the same image
    d_in, d_out = R.rotation(0.21, -0.17, 0.33), R.rotation(-0.12, 0.27, 0.19)
    m = R.index_map(sp_in, (1, 2, 3), d_in, sp_out, (0.2, 1.1, 2.3), d_out)
    want = ref_resample_grid(arr, sp_in, (1, 2, 3), d_in, size, sp_out, (0.2, 1.1, 2.3), d_out, nearest, return_real=True)
    got = R.resample_ref(arr, m, size[::-1], nearest=nearest, return_real=True)
    assert (np.abs(got - want) > 1e-9).mean() < (0.01 if nearest else 1e-12)
    # the own float64 path (used for border / half_even) equals the oracle where neither option changes anything
    inner = np.array([[0.3, 0.02, 0.01, 3.0], [0.01, 0.3, 0.02, 3.0], [0.02, 0.01, 0.3, 2.0]])
    assert np.array_equal(R.resample_ref(arr, inner, (8, 9, 10), nearest=nearest, border=True),
                          R.resample_ref(arr, inner, (8, 9, 10), nearest=nearest))


def test_optimiser_restatements_equal_torch_in_float64():
    n = 1001
    p0, g = R.seeded((n,), 71).astype(np.float64), R.seeded((n,), 72, 0.1).astype(np.float64)
    for amsgrad in (False, True):
        for wd in (0.0, 1e-2):
            pt = torch.tensor(p0, requires_grad=True)
            opt = torch.optim.Adam([pt], lr=1e-3, amsgrad=amsgrad, weight_decay=wd)
            ref, pr = R.RefAdam(n, lr=1e-3, weight_decay=wd, amsgrad=amsgrad), p0
            for step in range(1, 4):
                pt.grad = torch.tensor(g * step)
                opt.step()
                pr = ref.step(pr, g * step)
            assert np.abs(pt.detach().numpy() - pr).max() < 1e-13
    for mu in (0.0, 0.9):
        for wd in (0.0, 1e-2):
            pt = torch.tensor(p0, requires_grad=True)
            opt = torch.optim.SGD([pt], lr=1e-2, momentum=mu, weight_decay=wd)
            ref, pr = R.RefSGD(n, lr=1e-2, momentum=mu, weight_decay=wd), p0
            for step in range(1, 4):
                pt.grad = torch.tensor(g * step)
                opt.step()
                pr = ref.step(pr, g * step)
            assert np.abs(pt.detach().numpy() - pr).max() < 1e-14


def test_normalize_and_ensemble_references_equal_the_existing_oracles():
    from oracle.metrics_ref import ref_normalize
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 17, 19, 23)) * 37 + 100).astype(np.float32)
    x[1] = 5.0
    assert np.abs(R.normalize_ref(x) - ref_normalize(x)).max() < 2e-6
    g = torch.Generator().manual_seed(21)
    labs = [torch.randint(0, 5, (4097,), generator=g, dtype=torch.int32) for _ in range(3)]
    oh = torch.stack([torch.nn.functional.one_hot(t.long(), 5).float() for t in labs]).mean(0)
    assert np.array_equal(R.ensemble_vote_ref([t.numpy() for t in labs]), oh.argmax(1).numpy())
    logits = [torch.randn((5, 4097), generator=g) for _ in range(3)]
    w = [0.81, 0.9, 0.42]
    wt = torch.tensor(w).view(3, 1, 1)
    ref = (torch.stack(logits) * wt / wt.mean(0, keepdim=True)).mean(0)
    assert np.abs(R.ensemble_mean_ref([t.numpy() for t in logits], w) - ref.numpy()).max() < 1e-5


# ------------------------------------------------------------------------------------------------ the gates bite
def test_blend_gate_accepts_the_reference():
    assert not blend_pair(case("two-0.5-gauss"), None, gate=True)


@pytest.mark.parametrize("name,fault", [("segments-two", "skip_second_pass"), ("segments-generic", "skip_second_pass"),
                                        ("two-0.5-gauss", "descending_windows"), ("clamped-0.5-gauss", "descending_windows"),
                                        ("two-0.5", "drop_second_x_at_start"), ("two-0.5-gauss", "drop_second_x_at_start"),
                                        ("64-origins", "drop_second_x_at_start"), ("two-0.5", "last_max"),
                                        ("K8-f32-two", "last_max")])
def test_blend_gate_rejects(name, fault):
    assert blend_pair(case(name), fault, gate=case(name).gaussian)


def test_scatter_gate_rejects_a_count_taken_from_another_channel():
    roi, vol, n = (8, 8, 8), (12, 19, 30), 33
    starts = [(i % 7 - 1, (3 * i) % 12 - 2, (5 * i) % 20 - 3) for i in range(n)]
    pred = R.seeded((n,) + roi + (4,), 1)
    a, c = R.scatter_ref(pred, starts, np.zeros(vol + (4,), np.float32), np.zeros(vol, np.float32))
    with R.fault("count_other_channel"):
        fa, fc = R.scatter_ref(pred, starts, np.zeros(vol + (4,), np.float32), np.zeros(vol, np.float32))
    assert np.array_equal(a, fa) and not np.array_equal(c, fc)


def test_gather_argmax_and_count_gates_reject_a_skipped_second_pass():
    img = R.seeded((60, 70, 100, 1), 21)
    starts = [(-5 + 4 * (i // 4), -7 + 9 * (i % 4), -9 + 13 * (i % 5)) for i in range(16)]
    good = R.gather_ref(img, starts, (48, 48, 63), "bf16")
    with R.fault("skip_second_pass"):
        assert not np.array_equal(R.gather_ref(img, starts, (48, 48, 63), "bf16"), good)
    lg = R.argmax_logits((1, 1, 140003), 64, 77)
    ref = R.argmax_ref(lg)
    cut = R.CAPS["grid_for"] // 16
    assert (ref[..., cut:] != 0).any()          # labels a skipped pass would leave unwritten
    with R.fault("last_max"):
        assert not np.array_equal(R.argmax_ref(lg), ref)
    rng = np.random.default_rng(5)
    pred = rng.integers(-1, 6, 300007).astype(np.int32)
    good = R.label_counts_ref(pred, pred, 5)
    with R.fault("skip_second_pass"):
        assert not np.array_equal(R.label_counts_ref(pred, pred, 5), good)


def test_resample_gate_rejects():
    rng = np.random.default_rng(3)
    arr = rng.standard_normal((9, 11, 13)).astype(np.float32)
    lab = rng.integers(0, 256, (9, 11, 13)).astype(np.uint8)
    m, size = R.RESAMPLE_OBLIQUE, R.RESAMPLE_OBLIQUE_SHAPES[1]
    assert np.all(np.abs(m[:, :3]) > 1e-2) and 0 < R.RESAMPLE_OBLIQUE_OUTSIDE < np.prod(size)
    for a, nearest in ((arr, False), (arr, True), (lab, False), (lab, True)):
        ref = R.resample_ref(a, m, size, nearest=nearest)
        real = R.resample_ref(a, m, size, nearest=nearest, return_real=True)
        assert not R.resample_violations(ref, ref, real, nearest)
        with R.fault("swap_m1_m4"):
            assert R.resample_violations(R.resample_ref(a, m, size, nearest=nearest), ref, real, nearest)
    ref, real = R.resample_ref(lab, m, size), R.resample_ref(lab, m, size, return_real=True)
    with R.fault("round_cast"):
        assert R.resample_violations(R.resample_ref(lab, m, size), ref, real, False)
    half = np.array([[0.5, 0, 0, 1.0], [0, 0.5, 0, 0.0], [0, 0, 0.5, 2.0]])
    a = rng.standard_normal((7, 9, 10)).astype(np.float32)
    ref = R.resample_ref(a, half, (8, 14, 15), nearest=True, half_even=True)
    with R.fault("half_up"):
        assert R.resample_violations(R.resample_ref(a, half, (8, 14, 15), nearest=True, half_even=True), ref, None, True)
    big = rng.standard_normal((4, 6, 7)).astype(np.float32)
    mb = np.array([[0.04, 0, 0, 0.0], [0, 0.03, 0, 0.0], [0, 0, 0.02, 0.0]])
    ref = R.resample_ref(big, mb, (130, 128, 128))
    with R.fault("skip_second_pass"):
        assert R.resample_violations(R.resample_ref(big, mb, (130, 128, 128)), ref, None, False)


def test_integer_resample_excuse_stays_under_its_cap_for_the_reference_alone():
    """the maps the GPU file resamples integer pixels linearly with, perturbed by one float64 ulp: the truncated results
    differ only where the real value is within 1e-9 of an integer, and on fewer than 2 % of the voxels -- so the excuse
    cannot hide a wrong kernel.  (A map that lands on exact halves, like the half-even case's, would not do: a fifth of
    its voxels sit on an integer, which is why that case is nearest-neighbour only.)"""
    rng = np.random.default_rng(3)
    for shape, m, size in (((9, 11, 13), R.RESAMPLE_OBLIQUE, (12, 14, 17)),
                           (R.RESAMPLE_LARGE_SHAPES[0], R.RESAMPLE_LARGE, (33, 32, 32))):
        for pixel, (lo, hi) in (("uint8", (0, 256)), ("int16", (-3000, 3000)), ("int32", (-10 ** 6, 10 ** 6))):
            lab = rng.integers(lo, hi, shape).astype(pixel)
            ref = R.resample_ref(lab, m, size)
            real = R.resample_ref(lab, m, size, return_real=True)
            for mp in (np.nextafter(m, np.inf), np.nextafter(m, -np.inf)):
                assert not R.resample_violations(R.resample_ref(lab, mp, size), ref, real, False)


def test_normalize_gate_rejects_the_sample_std_and_a_skipped_pass():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((1, 2 * 65536 + 777)) * 37 + 100).astype(np.float32)
    ref = R.normalize_ref(x)
    assert np.abs(R.normalize_one_pass(x) - ref).max() <= 2e-6
    with R.fault("sample_std"):
        assert np.abs(R.normalize_ref(x) - ref).max() > 2e-6
    x = (rng.standard_normal((1, 600001)) * 37 + 100).astype(np.float32)
    ref = R.normalize_ref(x)
    with R.fault("skip_second_pass"):
        assert np.abs(R.normalize_ref(x) - ref).max() > 2e-6
    # mean 3e4, std 1: the one-pass float64 variance is as good as the two-pass one; what is left is the float32 mean
    y = (rng.standard_normal((1, 2 * 65536 + 777)) + 3e4).astype(np.float32)
    y64 = y.astype(np.float64)
    one_pass_var = (y64 * y64).mean() - y64.mean() ** 2
    assert abs(one_pass_var - y64.var()) < 1e-6 * y64.var()


def test_ensemble_gates_reject():
    rng = np.random.default_rng(2)
    n, e = 1048576 + 4099, 2
    palette = np.array([0, 1, 2, 255, 256, 70000, 3], np.int32)
    labs = [palette[rng.integers(0, len(palette), n)] for _ in range(e)]
    vote = R.ensemble_vote_ref(labs)
    ties = labs[0] != labs[1]
    assert ties.sum() > 0 and np.array_equal(vote[ties], np.minimum(labs[0], labs[1])[ties])
    pairs = [(70000, e - 1), (1, 0), (256, e // 2), (2, e - 1), (255, 0), (3, e - 1)]
    sel = R.ensemble_select_ref(labs, pairs)
    assert (sel == 0).any()
    for f, fn in (("vote_largest", lambda: R.ensemble_vote_ref(labs)), ("select_reverse", lambda: R.ensemble_select_ref(labs, pairs)),
                  ("skip_second_pass", lambda: R.ensemble_vote_ref(labs)), ("skip_second_pass", lambda: R.ensemble_select_ref(labs, pairs))):
        with R.fault(f):
            got = fn()
        assert not np.array_equal(got, vote) and not np.array_equal(got, sel), f
    logits = [(rng.standard_normal(n) * 3).astype(np.float32) for _ in range(e)]
    ref = R.ensemble_mean_ref(logits, [0.3, 0.9])
    with R.fault("skip_second_pass"):
        bad = R.ensemble_mean_ref(logits, [0.3, 0.9])
    assert np.abs(bad - ref).max() > e * 2.0 ** -23 * max(np.abs(l).max() for l in logits)


def test_optimiser_gates_reject():
    n = 524288 + 12345
    p0, g = R.seeded((n,), 71), R.seeded((n,), 72, 0.1)
    for make, bound in ((lambda: R.RefAdam(n, lr=1e-3, weight_decay=1e-2), 2e-7),
                        (lambda: R.RefSGD(n, lr=1e-2, momentum=0.9, weight_decay=1e-2), 2e-7)):
        good, bad, pg, pb = make(), make(), p0, p0
        for step in range(1, 4):
            pg = good.step(pg, g * step)
            with R.fault("decay_after_moments"):
                pb = bad.step(pb, g * step)
        assert not R.optim_violations(pg.astype(np.float32), pg, bound)
        assert R.optim_violations(pb.astype(np.float32), pg, bound)
        assert R.optim_violations(R.skip_tail(pg, R.CAPS["optim"]).astype(np.float32), pg, bound)


# ------------------------------------------------------------------------------------------------ the tables
def test_blend_table_meets_its_conditions():
    kinds = {}
    for c in R.BLEND_CASES:
        per_dim, wins = R.schedule(c.image, c.roi, c.overlap)
        vec, g = R.lanes_per_voxel(c.k, c.dtype)
        two = R.is_two(per_dim, c.roi)
        assert c.kind == ("blend_scalar" if vec == "scalar" else "blend2" if two else "blend")
        assert all(len(s) <= R.MAX_STARTS for s in per_dim)
        kinds.setdefault(c.kind, set()).add(c.k // g)
        if "two" in c.name.split("-")[0] or c.name.endswith("-two"):
            assert two, c.name
        if "clamped" in c.name or "0.75" in c.name or "generic" in c.name:
            assert not two, c.name
    assert set(kinds) == {"blend2", "blend", "blend_scalar"}
    assert {1, 2, 4, 8, 16, 32, 64} <= kinds["blend2"] and {1, 2, 4, 8, 16, 32, 64} <= kinds["blend"]
    for nm in ("segments-two", "segments-generic"):
        c = case(nm)
        _, g = R.lanes_per_voxel(c.k, c.dtype)
        assert c.image[0] * c.image[1] * ((c.image[2] * (c.k // g) + 255) // 256) > R.CAPS["blend_segments"]
    for nm in ("wide-f32", "wide-bf16", "wide-f32-generic"):
        c = case(nm)
        _, g = R.lanes_per_voxel(c.k, c.dtype)
        lanes = c.image[2] * (c.k // g)
        assert lanes > 256 and lanes % 256 != 0
    assert len(R.schedule(case("64-origins").image, case("64-origins").roi, 0.5)[0][2]) == 64
    assert R.schedule((12, 16, 10), (16, 16, 16), 0.5)[0] == [[-2], [0], [-3]]
    assert len(R.schedule((16, 28, 40), (16, 16, 16), 0.25)[0][0]) == 1
    assert R.schedule((20, 27, 33), (16, 16, 16), 0.5)[0][1:] == [[0, 8, 11], [0, 8, 16, 17]]
    ks = {c.k for c in R.BLEND_CASES}
    assert {1, 3, 4, 8, 12, 16, 24, 32, 64, 256, 260, 512} <= ks
    assert {(c.dtype, c.gaussian) for c in R.BLEND_CASES} == {(d, g) for d in ("f32", "bf16", "f16") for g in (False, True)}
    assert {c.labels for c in R.BLEND_CASES} == {"uint8", "int16", "int32"}


def test_blend_inputs_hold_ties_and_nans():
    for nm in ("two-0.5", "clamped-0.5", "K8-f32-two", "K256-bf16-clamped"):
        c = case(nm)
        cache, per_dim, wins, imp = R.blend_inputs(c)
        l, _, lab, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), c.roi, c.image, imp)
        ties, nans, multi = R.tie_and_nan_counts(l)
        assert ties > 0 and nans > 0 and multi > 0, (nm, ties, nans, multi)
        with R.fault("last_max"):
            assert not np.array_equal(R.argmax_ref(l), lab)


def test_argmax_inputs_hold_ties_and_nans_and_sizes_cross_the_caps():
    for k in (2, 5, 8, 64, 128, 256, 300, 512):
        ties, nans, multi = R.tie_and_nan_counts(R.argmax_logits((3, 7, 11), k, 40 + k))
        assert ties > 0 and nans > 0 and multi > 0, k
    assert 140003 * 16 > R.CAPS["grid_for"] and (140003 * 16) % 256
    assert 16 * 96 * 96 * 64 // 4 > R.CAPS["grid_for"] and 16 * 48 * 48 * 63 > R.CAPS["grid_for"]
    assert 140 * 130 * 130 > R.CAPS["grid_for"]
    assert 130 * 128 * 128 > R.CAPS["resample"]
    assert 2 * 65536 + 777 > 2 * R.CAPS["norm_chunk"] and 600001 > R.CAPS["norm_apply"]
    assert 1048576 + 4099 > R.CAPS["ensemble"] and 524288 + 12345 > R.CAPS["optim"] and 300007 > R.CAPS["label_counts"]
