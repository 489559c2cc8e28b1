"""The inference data-path kernels (sliding.hip, image.hip, ensemble.hip, the flat optimiser updates of loss_optim.hip)
against the plain numpy references of tests/helpers/infer_ref.py: every storage type, sizes past each grid cap (so that
the strided loops run a second, ragged pass), negative and slab-shifted blend origins, rows wider than a workgroup,
non-diagonal index maps, saturating casts and the argument limits.  Caches and logits are seeded random data; no
network is involved.  The gates are the functions of infer_ref that tests/test_infer_sweep_host.py shows to bite."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.optim_ref import RefAdaBelief  # noqa: E402
from segmantic_amd import ops  # noqa: E402
from tests.helpers import infer_ref as R  # noqa: E402

DEV = "cuda:0"
LABEL_DT = {"uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32}


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ blend
def run_blend(case, cache, per_dim, lo, hi, shape, imp, normalize=True, want_count=True, labels=True):
    """one ops.sw_blend call for ``case``; returns (dict of numpy results, kernel name)"""
    D, H, W = shape
    cd = dev(cache[lo:hi], R.torch_dtype(case.dtype))
    impd = dev(imp.reshape(-1)) if imp is not None else None
    out = view = None
    if not case.labels_only or not normalize:
        ld = case.out_ld or case.k
        out = torch.full((1, D, H, W, ld), -77.0, device=DEV)
        view = out[..., :case.k]
    cnt = torch.empty((D, H, W), device=DEV) if want_count else None
    lab = torch.empty((D, H, W), dtype=LABEL_DT[case.labels], device=DEV) if (labels and normalize) else None
    args = (cd, per_dim, lo, hi, case.roi, D, H, W)
    kw = dict(importance=impd, out_logits=view, out_count=cnt, labels=lab, normalize=normalize)
    name = ops.sw_blend_kernel_name(*args, **kw)
    ops.sw_blend(*args, **kw)
    torch.cuda.synchronize()
    got = {"logits": None if view is None else view[0].cpu().numpy(),
           "count": None if cnt is None else cnt.cpu().numpy(),
           "labels": None if lab is None else lab.cpu().numpy()}
    if out is not None and out.shape[-1] > case.k:       # the padding columns of a wider logits row stay untouched
        assert bool((out[..., case.k:] == -77.0).all())
    return got, name


def kind_of(name):
    return name.split("_kernel")[0][3:]


@pytest.mark.parametrize("case", R.BLEND_CASES, ids=[c.name for c in R.BLEND_CASES])
def test_blend_is_the_ordered_f32_sum(case, record_property):
    cache, per_dim, wins, imp = R.blend_inputs(case)
    _, g = R.lanes_per_voxel(case.k, case.dtype)
    ref_l, ref_c, ref_lab, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), case.roi, case.image, imp)
    got, name = run_blend(case, cache, per_dim, 0, len(wins), case.image, imp)
    assert kind_of(name) == case.kind and f"G={g}>" in name and f"<{case.dtype}," in name, name
    ref = {"logits": None if case.labels_only else ref_l, "count": ref_c, "labels": ref_lab}
    gate = None
    if case.gaussian and not case.labels_only:
        l64, c64, _, sabs, cover = R.blend_ref(cache, per_dim, 0, len(wins), case.roi, case.image, imp, dtype=np.float64)
        gate = (l64, R.gaussian_bound(sabs, c64, cover))
        same = bool(np.array_equal(got["logits"], ref_l, equal_nan=True))
        record_property("gaussian_bit_identical_to_product_rounded_f32", same)
        print(f"{case.name}: {name}: gaussian blend bit-identical to the product-rounded f32 sequence: {same}")
    bad = R.blend_violations(got, ref, gate, exact=True)
    assert not bad, (case.name, name, bad)


def test_blend_table_reaches_every_variant():
    kinds = {c.kind for c in R.BLEND_CASES}
    assert kinds == {"blend2", "blend", "blend_scalar"}


@pytest.mark.parametrize("name", ["two-0.5-gauss", "clamped-0.5-gauss", "padded", "overlap-0.75"])
def test_blend_of_a_slab_equals_the_planes_of_the_whole(name):
    """origins shifted by -z_off with output depth = slab depth and the full window range (the pipelined blend), and
    the [lo, hi) restriction of ``z_slab``: both must give the same planes as the blend of the whole volume"""
    case = next(c for c in R.BLEND_CASES if c.name == name)
    cache, per_dim, wins, imp = R.blend_inputs(case)
    D, H, W = case.image
    ref_l, ref_c, ref_lab, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), case.roi, case.image, imp)
    nyx = len(per_dim[1]) * len(per_dim[2])
    for z0, z1 in ((0, max(1, D // 3)), (D // 3, D - 2), (D - 2, D)):
        if z1 <= z0:
            continue
        shifted = [[s - z0 for s in per_dim[0]], per_dim[1], per_dim[2]]
        ref = {"logits": ref_l[z0:z1], "count": ref_c[z0:z1], "labels": ref_lab[z0:z1]}
        got, kname = run_blend(case, cache, shifted, 0, len(wins), (z1 - z0, H, W), imp)
        assert kind_of(kname) == case.kind
        assert not R.blend_violations(got, ref), (name, "full range", z0, z1)
        ks = [k for k, s0 in enumerate(per_dim[0]) if s0 < z1 and s0 + case.roi[0] > z0]
        lo, hi = ks[0] * nyx, (ks[-1] + 1) * nyx
        got, _ = run_blend(case, cache, shifted, lo, hi, (z1 - z0, H, W), imp)
        assert not R.blend_violations(got, ref), (name, "window range", z0, z1, lo, hi)


@pytest.mark.parametrize("name", ["two-0.5", "two-0.5-gauss", "clamped-0.5-gauss", "K12-f32-two"])
def test_blend_shards_are_the_unnormalised_partial_sums(name):
    case = next(c for c in R.BLEND_CASES if c.name == name)
    cache, per_dim, wins, imp = R.blend_inputs(case)
    mid = len(wins) // 2
    ref_l, ref_c, _, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), case.roi, case.image, imp)
    tot, cs = 0, 0
    for lo, hi in ((0, mid), (mid, len(wins))):
        pl, pc, _, _, _ = R.blend_ref(cache[lo:hi], per_dim, lo, hi, case.roi, case.image, imp, normalize=False)
        got, kname = run_blend(case, cache, per_dim, lo, hi, case.image, imp, normalize=False)
        assert kind_of(kname) == case.kind
        assert not R.blend_violations(got, {"logits": pl, "count": pc, "labels": None}), (name, lo, hi)
        tot, cs = tot + got["logits"].astype(np.float64), cs + got["count"].astype(np.float64)
    # the shards' sum / count reproduces the blend up to the association of the f32 additions across the boundary
    assert np.array_equal(cs.astype(np.float32), ref_c) or np.allclose(cs, ref_c, rtol=1e-6)
    with np.errstate(invalid="ignore"):
        err = np.nanmax(np.abs(tot / cs[..., None] - ref_l))
    assert err <= 1e-5 * np.nanmax(np.abs(ref_l))


def test_blend_refuses_65_origins_and_bad_ranges():
    """host-side argument checks: nothing is launched"""
    roi = (2, 2, 4)
    cache = torch.zeros((65, 2, 2, 4, 4), device=DEV)
    out = torch.empty((1, 2, 2, 134, 4), device=DEV)
    starts = [[0], [0], [2 * i for i in range(65)]]
    with pytest.raises(RuntimeError, match="at most 64 window origins"):
        ops.sw_blend(cache, starts, 0, 65, roi, 2, 2, 134, out_logits=out)
    assert ops.sw_blend_kernel_name(cache, starts, 0, 65, roi, 2, 2, 134, out_logits=out) == "invalid"
    starts = [[0], [0], [2 * i for i in range(64)]]
    with pytest.raises(RuntimeError, match="outside the schedule"):
        ops.sw_blend(cache, starts, 0, 65, roi, 2, 2, 130, out_logits=out)
    with pytest.raises(RuntimeError, match="labels need the normalised blend"):
        ops.sw_blend(cache, starts, 0, 64, roi, 2, 2, 130, out_logits=out, normalize=False,
                     labels=torch.empty((2, 2, 130), dtype=torch.uint8, device=DEV))
    c260 = torch.zeros((1, 2, 2, 4, 260), device=DEV)
    with pytest.raises(RuntimeError, match="uint8 labels hold at most 256"):
        ops.sw_blend(c260, [[0], [0], [0]], 0, 1, roi, 2, 2, 4, out_logits=torch.empty((1, 2, 2, 4, 260), device=DEV),
                     labels=torch.empty((2, 2, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="scalar path labels from the written logits"):
        ops.sw_blend(c260, [[0], [0], [0]], 0, 1, roi, 2, 2, 4, labels=torch.empty((2, 2, 4), dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ gather / scatter / finalise
OUTSIDE = [(-3, -2, -5), (0, 0, 0), (4, 9, 14), (10, 17, 25), (-8, 0, 0), (12, 19, 30), (3, -8, 2), (0, 0, 40), (5, 5, 5)]


@pytest.mark.parametrize("c,roi,src,dst", [(1, (8, 8, 8), "f32", "f32"), (1, (8, 8, 8), "f32", "bf16"),
                                           (1, (8, 8, 8), "f32", "f16"), (1, (8, 8, 8), "bf16", "f32"),
                                           (1, (8, 8, 8), "f16", "f32"), (1, (8, 8, 8), "bf16", "bf16"),
                                           (1, (8, 8, 7), "f32", "bf16"), (1, (5, 6, 10), "f16", "f16"),
                                           (2, (8, 8, 8), "f32", "f16"), (3, (6, 7, 9), "bf16", "f32"),
                                           (3, (8, 8, 8), "f32", "f32")])
def test_gather_windows_inside_and_outside(c, roi, src, dst):
    """windows partly and wholly outside (zero fill), 1 .. 3 channels, roi width not a multiple of 4 (scalar gather),
    groups of 17 and 33 windows in launch order"""
    img = R.quantize(R.seeded((12, 19, 30, c), 11 + c), src)
    imd = dev(img[None], R.torch_dtype(src))
    for n in (len(OUTSIDE), 17, 33):
        starts = [OUTSIDE[i % len(OUTSIDE)] if i < len(OUTSIDE) else (i % 7 - 1, (3 * i) % 16 - 2, (5 * i) % 29 - 3)
                  for i in range(n)]
        wd = torch.full((n,) + roi + (c,), 9.0, dtype=R.torch_dtype(dst), device=DEV)
        ops.sw_gather(imd, 0, starts, wd)
        assert np.array_equal(host(wd.float()), R.gather_ref(img, starts, roi, dst)), (n,)


@pytest.mark.parametrize("k,dtype,gauss,ld", [(3, "f32", True, 3), (4, "f32", True, 4), (16, "bf16", True, 16),
                                              (4, "f16", False, 4), (3, "bf16", False, 16), (16, "f32", False, 16),
                                              (3, "f16", True, 16), (4, "bf16", True, 16)])
def test_scatter_add_and_finalize(k, dtype, gauss, ld):
    """streaming blend: windows partly / wholly outside, importance map, ld > c accumulators, 17 and 33 windows in launch
    order on top of a non-zero accumulator, untouched voxels unmodified; then the division + argmax, logits written or not"""
    roi, vol = (8, 8, 8), (12, 19, 30)
    imp = R.importance_map(roi, "gaussian").numpy() if gauss else None
    for n in (17, 33):
        starts = [OUTSIDE[i] if i < 7 else (i % 7 - 1, (3 * i) % 12 - 2, (5 * i) % 20 - 3) for i in range(n)]
        pred = R.quantize(R.seeded((n,) + roi + (k,), 100 + n + k), dtype)
        acc0, cnt0 = R.seeded(vol + (k,), 5), np.abs(R.seeded(vol, 6)) + 0.5
        buf = torch.full((1,) + vol + (ld,), -5.0, device=DEV)
        acc = buf[..., :k]
        acc.copy_(dev(acc0[None]))
        cnt = dev(cnt0)
        ops.sw_scatter_add(dev(pred, R.torch_dtype(dtype)), starts, acc, cnt, importance=None if imp is None else dev(imp.reshape(-1)))
        ra, rc = R.scatter_ref(pred, starts, acc0.copy(), cnt0.copy(), imp)
        assert np.array_equal(host(acc)[0], ra) and np.array_equal(host(cnt), rc), (n,)
        assert bool((rc == cnt0).any()), "the case must leave some voxels untouched"
        rl, rlab = R.finalize_ref(ra, rc)
        for write in (False, True):
            lab = torch.empty(vol, dtype=torch.int16 if write else torch.uint8, device=DEV)
            ops.sw_finalize(acc, cnt, lab, write_logits=write)
            assert np.array_equal(host(lab).astype(np.int64), rlab), (n, write)
            assert np.array_equal(host(acc)[0], rl if write else ra), (n, write)
        if ld > k:
            assert bool((buf[..., k:] == -5.0).all())


def test_gather_and_scatter_past_one_grid_pass():
    """16 windows of one channel: (48, 48, 64) as the 4-wide gather takes it, (96, 96, 64) whose 2 359 296 4-wide lanes
    exceed one pass of 8192 x 256, and (48, 48, 63) whose 2 322 432 scalar lanes do; then the K = 4 scatter"""
    vol = (100, 110, 100)
    img = R.seeded(vol + (1,), 21)
    imd = dev(img[None])
    for roi, per in (((48, 48, 64), 4), ((96, 96, 64), 4), ((48, 48, 63), 1)):
        assert per == 1 or roi[2] % 4 == 0
        if roi != (48, 48, 64):
            assert 16 * roi[0] * roi[1] * roi[2] // per > R.CAPS["grid_for"]
        starts = [(-5 + 4 * (i // 4), -7 + 9 * (i % 4), -9 + 13 * (i % 5)) for i in range(16)]
        wd = torch.empty((16,) + roi + (1,), dtype=torch.bfloat16, device=DEV)
        ops.sw_gather(imd, 0, starts, wd)
        assert np.array_equal(host(wd.float()), R.gather_ref(img, starts, roi, "bf16")), roi
    roi = (48, 48, 64)
    # the matching scatter: the windows' bounding box holds more than 2 097 152 voxels x (K / 4)
    vol = (140, 130, 130)
    starts = [(0, 0, 0), (92, 82, 66)] + [(7 * i, 5 * i, 4 * i) for i in range(1, 15)]
    assert vol[0] * vol[1] * vol[2] > R.CAPS["grid_for"]
    pred = R.quantize(R.seeded((16,) + roi + (4,), 22), "bf16")
    acc0, cnt0 = np.zeros(vol + (4,), np.float32), np.zeros(vol, np.float32)
    acc, cnt = dev(acc0[None]), dev(cnt0)
    ops.sw_scatter_add(dev(pred, torch.bfloat16), starts, acc, cnt)
    ra, rc = R.scatter_ref(pred, starts, acc0, cnt0)
    assert np.array_equal(host(acc)[0], ra) and np.array_equal(host(cnt), rc)


# ------------------------------------------------------------------------------------------------ argmax
@pytest.mark.parametrize("k", [1, 2, 5, 8, 64, 128, 256, 300, 512])
def test_argmax_first_max_first_nan(k):
    lg = R.argmax_logits((3, 7, 11), k, 40 + k)
    ref = R.argmax_ref(lg)
    for dt in ("f32", "bf16", "f16"):
        for ld in (k, k + 8 if k % 4 == 0 else k + 3):
            buf = torch.zeros((1, 3, 7, 11, ld), dtype=R.torch_dtype(dt), device=DEV)
            view = buf[..., :k]
            view.copy_(dev(lg[None], R.torch_dtype(dt)))
            for ldt in ((torch.uint8,) if k <= 256 else ()) + (torch.int16, torch.int32):
                lab = torch.empty((1, 3, 7, 11), dtype=ldt, device=DEV)
                ops.argmax(view, lab)
                assert np.array_equal(host(lab)[0].astype(np.int64), ref), (k, dt, ld, ldt)


def test_argmax_past_one_grid_pass_with_a_ragged_tail():
    k, nvox = 64, 140003
    assert nvox * (k // 4) > R.CAPS["grid_for"] and (nvox * (k // 4)) % 256 != 0
    lg = R.argmax_logits((1, 1, nvox), k, 77)
    lab = torch.empty((1, 1, 1, nvox), dtype=torch.uint8, device=DEV)
    ops.argmax(dev(lg[None], torch.bfloat16), lab)
    assert np.array_equal(host(lab)[0].astype(np.int64), R.argmax_ref(lg))


# ------------------------------------------------------------------------------------------------ label counts
@pytest.mark.parametrize("k", [1, 5, 4096])
def test_label_counts_strided_with_labels_outside(k):
    n = 300007
    assert n > R.CAPS["label_counts"]
    rng = np.random.default_rng(k)
    pred = rng.integers(-1, k + 1, n).astype(np.int32)
    truth = np.where(rng.uniform(size=n) < 0.5, pred, rng.integers(-1, k + 1, n)).astype(np.int32)
    assert (pred == -1).any() and (pred == k).any() and (truth == -1).any() and (truth == k).any()
    counts = torch.full((k, 3), -1, dtype=torch.int64, device=DEV)
    ops.label_counts(dev(pred), dev(truth), k, counts)
    assert np.array_equal(host(counts), R.label_counts_ref(pred, truth, k))


def test_label_counts_refuses_4097_classes():
    z = torch.zeros(16, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="label_counts"):
        ops.label_counts(z, z, 4097, torch.zeros((4097, 3), dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------ resample
PIXELS = ["float32", "uint8", "int16", "int32", "uint16"]


def pixels(shape, pixel, seed):
    rng = np.random.default_rng(seed)
    if pixel == "float32":
        return rng.standard_normal(shape).astype(np.float32)
    lo, hi = {"uint8": (0, 256), "int16": (-3000, 3000), "int32": (-10 ** 6, 10 ** 6), "uint16": (0, 65536)}[pixel]
    return rng.integers(lo, hi, shape).astype(pixel)


def torch_pixels(arr):
    if arr.dtype == np.uint16:
        if not hasattr(torch, "uint16"):
            pytest.skip("this torch has no uint16")
        return torch.from_numpy(arr.view(np.int16)).to(DEV).view(torch.uint16)
    return dev(arr)


def host_pixels(t):
    torch.cuda.synchronize()
    if hasattr(torch, "uint16") and t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def check_resample(arr, m, size, nearest=False, border=False, half_even=False, default=0.0):
    got = host_pixels(ops.resample3d(torch_pixels(arr), size, m, nearest=nearest, default=default, border=border,
                                     half_even=half_even))
    kw = dict(nearest=nearest, border=border, half_even=half_even, default=default)
    ref = R.resample_ref(arr, m, size, **kw)
    real = R.resample_ref(arr, m, size, return_real=True, **kw)
    bad = R.resample_violations(got, ref, real, nearest)
    assert not bad, bad
    return got


@pytest.mark.parametrize("pixel", PIXELS)
@pytest.mark.parametrize("nearest", [False, True])
def test_resample_oblique_maps(pixel, nearest):
    """direction cosines on both grids plus a rigid transform: all nine linear terms non-zero; every default, border"""
    arr = pixels((9, 11, 13), pixel, 3)
    m = R.RESAMPLE_OBLIQUE
    assert np.all(np.abs(m[:, :3]) > 1e-2)
    for default in (0.0, -7.5, 1e6):
        got = check_resample(arr, m, (12, 14, 17), nearest=nearest, default=default)
        if pixel != "float32":      # the default pixel saturates, and the case has voxels outside the source
            info = np.iinfo(arr.dtype)
            assert (got == int(np.trunc(np.clip(default, info.min, info.max)))).sum() >= R.RESAMPLE_OBLIQUE_OUTSIDE
    check_resample(arr, m, (12, 14, 17), nearest=nearest, border=True)


@pytest.mark.parametrize("pixel", ["float32", "uint8", "int16"])
def test_resample_half_even_on_exact_halves(pixel):
    """scale 0.5 with an integer offset: every second coordinate is exactly x.5, where ITK rounds up and torch to even"""
    arr = pixels((7, 9, 10), pixel, 4)
    m = np.array([[0.5, 0, 0, 1.0], [0, 0.5, 0, 0.0], [0, 0, 0.5, 2.0]])
    up = check_resample(arr, m, (8, 14, 15), nearest=True)
    even = check_resample(arr, m, (8, 14, 15), nearest=True, half_even=True)
    assert (up != even).mean() > 0.1
    check_resample(arr, m, (8, 14, 15), nearest=True, half_even=True, border=True, default=-7.5)


@pytest.mark.parametrize("pixel,nearest", [("float32", False), ("uint8", True), ("int16", False)])
def test_resample_past_one_grid_pass(pixel, nearest):
    arr = pixels(R.RESAMPLE_LARGE_SHAPES[0], pixel, 5)
    size, m = R.RESAMPLE_LARGE_SHAPES[1], R.RESAMPLE_LARGE
    assert size[0] * size[1] * size[2] > R.CAPS["resample"]
    check_resample(arr, m, size, nearest=nearest, default=-7.5)


@pytest.mark.parametrize("shape", [(1, 11, 13), (9, 1, 13), (9, 11, 1)])
def test_resample_extent_one(shape):
    arr = pixels(shape, "float32", 6)
    m = np.array([[0.7, 0.05, 0.0, 0.1], [0.0, 0.8, 0.05, -0.2], [0.05, 0.0, 0.9, 0.0]])
    out = tuple(max(1, int(s * 1.3)) for s in shape)
    for nearest in (False, True):
        check_resample(arr, m, out, nearest=nearest, default=1e6)
        check_resample(arr, m, out, nearest=nearest, border=True)


# ------------------------------------------------------------------------------------------------ normalise
@pytest.mark.parametrize("c,nvox", [(3, 2 * 65536 + 777), (2, 600001), (2, 1)])
def test_normalize_multi_chunk(c, nvox, record_property):
    rng = np.random.default_rng(nvox)
    x = (rng.standard_normal((c, nvox)) * 37 + 100).astype(np.float32)
    x[-1] = np.float32(1234.567)                       # constant channel at a non-trivial value
    if c == 3:
        x[1] = (rng.standard_normal(nvox) + 3e4).astype(np.float32)      # mean 3e4, std 1
    got = host(ops.normalize_intensity_(dev(x)))
    ref = R.normalize_ref(x)
    assert np.all(got[-1] == 0.0)
    err = np.abs(got - ref)
    assert err[0].max() <= 2e-6
    if c == 3:
        one = np.abs(R.normalize_one_pass(x)[1] - ref[1]).max()
        record_property("one_pass_numpy_error", float(one))
        record_property("kernel_error", float(err[1].max()))
        print(f"mean 3e4 / std 1: numpy one-pass error {one:.3e}, kernel error {err[1].max():.3e}")
        assert err[1].max() <= 4 * one


# ------------------------------------------------------------------------------------------------ ensemble
N_ENS = 1048576 + 4099


@pytest.mark.parametrize("e", [1, 2, 16])
def test_ensemble_mean_vote_select(e):
    assert N_ENS > R.CAPS["ensemble"]
    rng = np.random.default_rng(e)
    logits = [(rng.standard_normal(N_ENS) * 3).astype(np.float32) for _ in range(e)]
    ld = [dev(l) for l in logits]
    out = torch.empty(N_ENS, device=DEV)
    mx = max(float(np.abs(l).max()) for l in logits)
    for w in (None, list(rng.uniform(0.2, 1.0, e))):
        ops.ensemble_mean(ld, w, out)
        err = np.abs(host(out) - R.ensemble_mean_ref(logits, w)).max()
        assert err <= e * 2.0 ** -23 * mx, (w, err)
    # few distinct labels, large and small (ties between them), labels >= 256
    palette = np.array([0, 1, 2, 255, 256, 70000, 3], np.int32)
    labs = [palette[rng.integers(0, len(palette), N_ENS)] for _ in range(e)]
    lab_d = [dev(l) for l in labs]
    lo = torch.empty(N_ENS, dtype=torch.int32, device=DEV)
    ops.ensemble_vote(lab_d, lo)
    assert np.array_equal(host(lo), R.ensemble_vote_ref(labs))
    pairs = [(70000, e - 1), (1, 0), (256, e // 2), (2, e - 1), (255, 0), (3, e - 1)]
    ops.ensemble_select(lab_d, dict(pairs), lo)
    assert np.array_equal(host(lo), R.ensemble_select_ref(labs, pairs))


def test_ensemble_limits():
    n = 4099
    rng = np.random.default_rng(9)
    labs = [rng.integers(0, 300, n).astype(np.int32) for _ in range(3)]
    lab_d = [dev(l) for l in labs]
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    pairs = [(int(t), int(rng.integers(0, 3))) for t in rng.permutation(300)[:256]]
    ops.ensemble_select(lab_d, dict(pairs), out)
    assert np.array_equal(host(out), R.ensemble_select_ref(labs, pairs))
    with pytest.raises(RuntimeError, match="ensemble_select"):
        ops.ensemble_select(lab_d, {t: 0 for t in range(257)}, out)
    with pytest.raises(RuntimeError, match="ensemble_select"):
        ops.ensemble_select(lab_d, {1: 3}, out)
    z = [torch.zeros(8, dtype=torch.int32, device=DEV) for _ in range(17)]
    with pytest.raises(RuntimeError, match="ensemble_vote"):
        ops.ensemble_vote(z, out[:8].contiguous())
    zf = [torch.zeros(8, device=DEV) for _ in range(17)]
    with pytest.raises(RuntimeError, match="ensemble_mean"):
        ops.ensemble_mean(zf, None, torch.empty(8, device=DEV))


# ------------------------------------------------------------------------------------------------ optimisers
N_OPT = 524288 + 12345


def _pg():
    return R.seeded((N_OPT,), 71), R.seeded((N_OPT,), 72, 0.1)


@pytest.mark.parametrize("gs", [1.0, 1.0 / 128])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_strided(amsgrad, wd, gs):
    assert N_OPT > R.CAPS["optim"]
    p0, g = _pg()
    ref = R.RefAdam(N_OPT, lr=1e-3, weight_decay=wd, amsgrad=amsgrad, grad_scale=gs)
    pr, pd = p0, dev(p0)
    m, v = torch.zeros(N_OPT, device=DEV), torch.zeros(N_OPT, device=DEV)
    vm = torch.zeros(N_OPT, device=DEV) if amsgrad else None
    for step in range(1, 4):
        gg = (g * step / np.float32(gs)).astype(np.float32)
        pr = ref.step(pr, gg)
        ops.adam_step(pd, dev(gg), m, v, vm, 1e-3, 0.9, 0.999, 1e-8, wd, step, grad_scale=gs)
    assert not R.optim_violations(host(pd), pr, 2e-7)


@pytest.mark.parametrize("gs", [1.0, 1.0 / 128])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_strided(momentum, wd, gs):
    p0, g = _pg()
    ref = R.RefSGD(N_OPT, lr=1e-2, momentum=momentum, weight_decay=wd, grad_scale=gs)
    pr, pd, buf = p0, dev(p0), torch.zeros(N_OPT, device=DEV)
    for step in range(1, 4):
        gg = (g * step / np.float32(gs)).astype(np.float32)
        pr = ref.step(pr, gg)
        ops.sgd_step(pd, dev(gg), buf, 1e-2, momentum, wd, step == 1, grad_scale=gs)
    assert not R.optim_violations(host(pd), pr, 2e-7)


@pytest.mark.parametrize("gs", [1.0, 1.0 / 128])
@pytest.mark.parametrize("decouple,wd", [(False, 0.0), (False, 1e-2), (True, 1e-2)])
def test_adabelief_strided(decouple, wd, gs):
    p0, g = _pg()
    ref = RefAdaBelief(N_OPT, lr=1e-3, eps=1e-16, weight_decay=wd, weight_decouple=decouple)
    pr, pd = p0.copy(), dev(p0)
    m, s = torch.zeros(N_OPT, device=DEV), torch.zeros(N_OPT, device=DEV)
    for step in range(1, 4):
        gs_true = (g * step).astype(np.float32)
        pr = ref.step(pr, gs_true)
        ops.adabelief_step(pd, dev((gs_true / np.float32(gs)).astype(np.float32)), m, s, 1e-3, 0.9, 0.999, 1e-16, wd,
                           decouple, step, grad_scale=gs)
    assert not R.optim_violations(host(pd), pr, 3e-7)
