"""The training-batch augmentation kernels against the float64 references of
tests/helpers/augment_ref.py, at the shapes and edges the sampler reaches: crop_kernel,
warp_crop_kernel, the intensity kernels and the k-space DFT (augment.hip), and the whole
``trainer.make_batch`` chain against ``augment_ref.reference_chain`` for the same draws.

Every bound is written next to its check with what it is derived from.  MEASURED lines print the
observed error next to the bound (``pytest -s``)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.seg import augment as aug  # noqa: E402
from tests.helpers import augment_ref as ar  # noqa: E402

DEV = "cuda:0"
EPS32 = 2.0 ** -24          # f32 unit roundoff


def _measured(name, err, bound):
    print(f"MEASURED {name}: {err:.3e} (bound {bound:.3e})")


def _volume(shape, c, seed, b=1):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn((b,) + tuple(shape) + (c,), generator=g)
    lab = torch.randint(0, 4, (b,) + tuple(shape), generator=g).float()
    return img, lab


# ------------------------------------------------------------------------------------------ crop
def _cast_like_kernel(x64, dtype):
    """the kernel stores f32 values (or rounds them once, to nearest even, to bf16 / f16)"""
    return torch.from_numpy(np.ascontiguousarray(x64, dtype=np.float32)).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("c", [1, 3])
def test_crop_patches_is_bit_exact(dtype, c):
    """16 crops (the per-launch maximum) from source volume b = 1 of 2, all 8 flip codes, starts fully
    inside, partly outside and fully outside the volume (SpatialPad zeros)."""
    D, H, W = 23, 19, 28
    roi = (10, 12, 9)
    img, lab = _volume((D, H, W), c, 1, b=2)
    starts = [[1, 2, 3, 4], [1, 13, 7, 19], [1, -3, 5, 2], [1, 20, 15, 25], [1, -9, -11, -8],
              [1, 30, 0, 0], [1, 0, -12, 40], [1, 5, 4, -4], [0, 6, 2, 10], [1, -1, -1, -1],
              [1, 13, 7, 19], [1, 4, 8, 12], [0, -5, 10, 22], [1, 11, 0, 0], [1, 0, 11, 0], [1, 2, 2, 19]]
    flips = [i % 8 for i in range(16)]
    out = torch.full((16,) + roi + (c,), 7.0, device=DEV).to(dtype)
    olab = torch.full((16,) + roi, 7.0, device=DEV)
    ops.crop_patches(img.to(DEV), lab.to(DEV), starts, flips, out, olab)
    torch.cuda.synchronize()
    got, gl = out.cpu(), olab.cpu().numpy()
    for w, (st, fl) in enumerate(zip(starts, flips)):
        vol = img[st[0]].numpy().astype(np.float64).transpose(3, 0, 1, 2)
        ri, rl = ar.crop(vol, lab[st[0]].numpy().astype(np.float64), st[1:], roi)
        ri, rl = ar.flip(ri, fl), ar.flip(rl, fl)
        want = _cast_like_kernel(ri.transpose(1, 2, 3, 0), dtype)
        assert torch.equal(got[w], want), (w, st, fl)
        assert np.array_equal(gl[w], rl), (w, st, fl)
    assert float(out[5].float().abs().max()) == 0.0 and float(olab[5].abs().max()) == 0.0   # fully outside


def test_crop_patches_more_than_16_per_call():
    """make_batch passes num_samples crops per call and nothing caps num_samples: 37 crops = 3 launches"""
    img, lab = _volume((20, 18, 16), 2, 2)
    roi = (8, 6, 10)
    rng = np.random.RandomState(0)
    starts = [[0, int(rng.randint(-4, 16)), int(rng.randint(-4, 16)), int(rng.randint(-4, 10))] for _ in range(37)]
    flips = list(rng.randint(0, 8, 37))
    out = torch.empty((37,) + roi + (2,), device=DEV)
    olab = torch.empty((37,) + roi, device=DEV)
    ops.crop_patches(img.to(DEV), lab.to(DEV), starts, flips, out, olab)
    out2 = torch.empty_like(out)
    ops.warp_crop_patches(img.to(DEV), lab.to(DEV), starts, flips, np.eye(4)[:3], out2, None)
    torch.cuda.synchronize()
    vol = img[0].numpy().astype(np.float64).transpose(3, 0, 1, 2)
    for w, (st, fl) in enumerate(zip(starts, flips)):
        ri, rl = ar.crop(vol, lab[0].numpy().astype(np.float64), st[1:], roi)
        assert np.array_equal(out[w].cpu().numpy().transpose(3, 0, 1, 2), ar.flip(ri, fl)), w
        assert np.array_equal(olab[w].cpu().numpy(), ar.flip(rl, fl)), w
    assert torch.equal(out, out2)                                     # identity map = plain crop


# ------------------------------------------------------------------------------------------ warp
def _coord_error_bound(m, shape):
    """Largest error of the kernel's f32 source coordinate: the 12 map entries are rounded to f32
    (relative EPS32 each) and the three products plus three sums of a row each round once
    (6 roundings of at most |row| . (max extent, 1) each)."""
    row = np.abs(m[:3, :3]).sum(1) * (max(shape) + 32) + np.abs(m[:3, 3])
    return float(8 * EPS32 * row.max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_warp_crop_patches_matches_float64_trilinear(dtype):
    """Maps of ``augment.draw_spatial`` under fixed seeds (rotations and zoom together) on a
    96 x 80 x 72 two-channel volume with 48^3 patches, flips and SpatialPad included."""
    D, H, W = 96, 80, 72
    roi = (48, 48, 48)
    img, lab = _volume((D, H, W), 2, 3)
    vol = img[0].numpy().astype(np.float64).transpose(3, 0, 1, 2)
    lv = lab[0].numpy().astype(np.float64)
    imd, lad = img.to(DEV), lab.to(DEV)
    maps, seed = [], 0
    while len(maps) < 3:                         # seeds whose draw rotates about >= 2 axes and zooms
        m = aug.draw_spatial(np.random.RandomState(seed), (D, H, W))
        seed += 1
        if m is not None and abs(np.linalg.det(m[:3, :3]) - 1) > 1e-3 and np.count_nonzero(np.abs(m[:3, :3] - np.diag(np.diag(m[:3, :3]))) > 1e-6) >= 4:
            maps.append(m)
    starts = [[0, 10, 20, 8], [0, -6, 40, 30], [0, 60, -10, 40], [0, 24, 16, 12]]
    flips = [0, 7, 3, 4]
    vmax = float(np.abs(vol).max())
    # Lipschitz constant of the trilinear interpolant along one axis: the largest neighbour step
    lip = max(float(np.abs(np.diff(vol, axis=a)).max()) for a in (1, 2, 3))
    for m in maps:
        out = torch.empty((4,) + roi + (2,), device=DEV).to(dtype)
        olab = torch.empty((4,) + roi, device=DEV)
        ops.warp_crop_patches(imd, lad, starts, flips, aug.to_index_map_xyz(m), out, olab)
        torch.cuda.synchronize()
        got = out.float().cpu().numpy()
        gl = olab.cpu().numpy()
        delta = _coord_error_bound(m, (D, H, W))
        for w, (st, fl) in enumerate(zip(starts, flips)):
            ri, rl, src = ar.warp_crop(vol, lv, m, st[1:], roi)
            ri, rl, src = ar.flip(ri, fl), ar.flip(rl, fl), ar.flip(src, fl)
            ref = ri.transpose(1, 2, 3, 0)
            # coordinate error delta on each of 3 axes times the slope, + the f32 lerps (7 of them,
            # each rounding at most vmax * EPS32 twice), + the one output rounding of bf16 / f16
            tol = 3 * delta * lip + 16 * EPS32 * vmax
            ulp = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
            err = np.abs(got[w] - ref) - ulp * np.abs(ref)
            _measured(f"warp {dtype} map {len(maps)} patch {w}", float(err.max()), tol)
            assert float(err.max()) <= tol, (w, float(err.max()), tol)
            # nearest label: a pick may differ only where the float64 coordinate lies within the
            # coordinate error of a .5 boundary
            bad = gl[w] != rl
            assert not (bad & ~ar.near_half(src, (D, H, W), 2 * delta)).any(), w


# ------------------------------------------------------------------------------------- intensity
INT_RTOL = 2e-5    # f32 elementwise chain vs float64, relative to max(1, max |ref|): see below


def _int_draws(n, nctrl, seed, which):
    rng = np.random.RandomState(seed)
    on = lambda k: (rng.rand(n) < 0.6).astype(np.uint8) if k in which else np.zeros(n, np.uint8)  # noqa: E731
    gam = rng.uniform(0.5, 4.5, n).astype(np.float32)
    ctrl = np.tile(np.linspace(0.0, 1.0, nctrl), (n, 1))
    for i in range(n):
        for k in range(1, nctrl - 1):
            ctrl[i, k] = rng.uniform(ctrl[i, k - 1], ctrl[i, k + 1])
    coef = rng.uniform(0.0, 0.1, (n, 20)).astype(np.float32)
    con, hon, bon = on("c"), on("h"), on("b")
    for k, o in zip("chb", (con, hon, bon)):
        if k in which:
            o[0], o[-1] = 1, 0                   # at least one patch on and one off per transform
    return (con, gam), (hon, ctrl.astype(np.float32)), (bon, coef)


@pytest.mark.parametrize("shape,c,n,nctrl,which", [
    ((128, 128, 128), 1, 2, 10, "chb"),          # 2M voxels: 8192 per min / max chunk
    ((37, 41, 43), 2, 16, 16, "chb"),            # ragged, 16 patches, the largest nctrl
    ((37, 41, 43), 2, 5, 2, "c"),
    ((37, 41, 43), 1, 5, 10, "h"),
    ((37, 41, 43), 2, 5, 10, "b"),
    ((1, 7, 9), 1, 3, 10, "chb"),                # linspace(-1, 1, 1) == [-1]
    ((20, 12, 16), 3, 20, 10, "chb"),            # 20 patches: two launches
])
def test_intensity_augment_matches_float64(shape, c, n, nctrl, which):
    """Contrast, histogram shift and bias field alone and in sequence; patch minimum and maximum in
    the last min / max chunk; one constant patch."""
    g = torch.Generator().manual_seed(sum(shape) + n)
    x = torch.randn((n,) + shape + (c,), generator=g)
    per = int(np.prod(shape)) * c
    flat = x.reshape(n, per)
    flat[0, per - 3] = 9.0                       # the extremes of patch 0 sit in the last chunk
    flat[0, per - 1] = -8.5
    if n > 2:
        x[2] = 1.25                              # constant patch
    xd = x.to(DEV).contiguous()
    con, hist, bias = _int_draws(n, nctrl, n + c, which)
    ops.intensity_augment(xd, con, hist, bias)
    torch.cuda.synchronize()
    got = xd.cpu().numpy()
    worst = 0.0
    for i in range(n):
        v = x[i].numpy().astype(np.float64).transpose(3, 0, 1, 2)
        if con[0][i]:
            v = ar.adjust_contrast(v, con[1][i])
        if hist[0][i]:
            v = ar.histogram_shift(v, hist[1][i])
        if bias[0][i]:
            v = ar.bias_field(v, bias[1][i])
        ref = v.transpose(1, 2, 3, 0)
        # f32 arithmetic on f32 inputs: (x - min) / (range + 1e-7) rounds 3 times, powf is within 2 ulp and
        # scales the relative error by gamma <= 4.5; the histogram lerp and the Legendre sum (20 terms of
        # <= 0.1 * |L| <= 0.1) and expf add a few roundings each, times exp(2) at most: ~100 EPS32 = 6e-6
        err = float(np.abs(got[i] - ref).max()) / max(1.0, float(np.abs(ref).max()))
        worst = max(worst, err)
        assert err < INT_RTOL, (i, err)
        if not (con[0][i] or hist[0][i] or bias[0][i]):
            assert np.array_equal(got[i], x[i].numpy())
    _measured(f"intensity {shape} c{c} n{n} k{nctrl} {which}", worst, INT_RTOL)
    if n > 2 and not bias[0][2]:
        assert np.all(got[2] == 1.25)            # a constant patch stays constant


# --------------------------------------------------------------------------------------- k-space
def _check_radius_margin(shape, r):
    """the reference compares float64 distances with r, the kernel f32 ones (r and the distance each
    within ~4 EPS32 relative): keep every bin clear of the sphere by 1e-5 relative"""
    idx = [np.arange(n) - (n - 1) / 2.0 for n in shape]
    d = np.sqrt(idx[0][:, None, None] ** 2 + idx[1][None, :, None] ** 2 + idx[2][None, None, :] ** 2)
    assert np.abs(d - r).min() > 1e-5 * max(1.0, r), (shape, r)


def _ks_case(shape, c, gon, alpha, son, loc, u, flips, rtol, name):
    n = len(gon)
    g = torch.Generator().manual_seed(int(np.prod(shape)) % 9973 + n)
    x = torch.randn((n,) + tuple(shape) + (c,), generator=g)
    xd = x.to(DEV).contiguous()
    gon, son = np.asarray(gon, np.uint8), np.asarray(son, np.uint8)
    alpha, u = np.asarray(alpha, np.float32), np.asarray(u, np.float32)
    loc = np.asarray(loc, np.int32)
    for i in range(n):
        if gon[i]:
            _check_radius_margin(shape, ar.gibbs_radius(alpha[i], shape))
    ops.kspace_augment(xd, (gon, alpha), (son, loc, u), flips)
    torch.cuda.synchronize()
    got = xd.cpu().numpy()
    worst = 0.0
    for i in range(n):
        v = x[i].numpy().astype(np.float64).transpose(3, 0, 1, 2)
        fl = int(flips[i]) if flips is not None else 0
        if gon[i]:
            v = ar.gibbs(v, alpha[i], fl)
        if son[i]:
            v = ar.spike(v, loc[i], u[i])
        ref = v.transpose(1, 2, 3, 0)
        err = float(np.abs(got[i] - ref).max()) / max(1.0, float(np.abs(ref).max()))
        worst = max(worst, err)
        assert err < rtol, (name, i, err)
        if not (gon[i] or son[i]):
            assert np.array_equal(got[i], x[i].numpy())                # untouched patch
    _measured(f"kspace {name}", worst, rtol)


def _corner_locs(shape, n):
    """spike locations cycling through index 0 and N - 1 on every axis (and one interior bin)"""
    cs = [(0, 0, 0), tuple(s - 1 for s in shape), (0, shape[1] - 1, 0), (shape[0] - 1, 0, shape[2] - 1),
          tuple(s // 2 + 1 for s in shape)]
    return [cs[i % len(cs)] for i in range(n)]


# Bounds: a direct f32 DFT pass sums N products (error ~ sqrt(N) EPS32 of the line's norm in
# practice, N EPS32 at worst); 6 passes + the spike magnitude exp(2.5 mean log|K|) whose exponent
# carries the f32 mean's error.  Measured on an MI355X, relative to max(1, max |ref|): 4.0e-6 at
# 128^3, 3.2e-6 at 96^3, 1.4e-6 at 33x35x37, <= 2.5e-6 on the 480 / 481 / 512 lines.  KS_TIGHT
# keeps 5x over the largest (tests/test_ops_gpu.py's 6x9x10 case keeps its 5e-4).
KS_TIGHT = 2e-5


@pytest.mark.parametrize("shape", [(96, 96, 96), (128, 128, 128), (33, 35, 37)])
def test_kspace_augment_cubes(shape):
    """two channels, four patches in one call: Gibbs on 0 and 2, spike on 1 and 2 (slot -> patch
    mapping), patch 3 untouched; spike at corner bins; alpha near 0 and near 1."""
    n = 4
    near0, near1 = 0.0123, 0.9991          # radius below the first bin for near1
    _ks_case(shape, 2, [1, 0, 1, 0], [near0, 0.5, near1, 0.3], [0, 1, 1, 0], _corner_locs(shape, n),
             [0.2, 0.7, 0.95, 0.5], None, KS_TIGHT, f"{shape}")


def test_kspace_augment_gibbs_mid_alpha_and_flips():
    """the mask at the mirrored bin for every flip code, even and odd extents"""
    for shape in [(32, 24, 20), (21, 17, 25)]:
        n = 8
        alpha = np.linspace(0.15, 0.8, n) + 0.0137
        _ks_case(shape, 1, [1] * n, alpha, [0] * n, _corner_locs(shape, n), [0.5] * n, list(range(8)),
                 KS_TIGHT, f"flips {shape}")


@pytest.mark.parametrize("shape", [(4, 6, 512), (4, 6, 481), (5, 3, 480), (481, 4, 6), (512, 5, 3),
                                   (480, 3, 4), (5, 480, 3), (6, 481, 4), (3, 512, 5)])
def test_kspace_augment_long_lines(shape):
    """extents 480, 481 and 512 on each axis: the DFT of a 481..512 line takes more than 64 KiB
    of LDS ((N + 16 (N + 1)) * 8 bytes).  On an MI355X the launch runs correctly without
    hipFuncSetAttribute as well; the attribute is set as for every other kernel above 64 KiB, and
    this test guards the extents up to the documented cap of 512."""
    _ks_case(shape, 2, [1, 0, 1], [0.37, 0.0, 0.71], [0, 1, 0], _corner_locs(shape, 3), [0.1, 0.6, 0.9],
             None, KS_TIGHT, f"{shape}")


def test_kspace_augment_20_patches():
    """20 patches (two calls of <= 16), Gibbs on 7 of them and the spike on 7 others (a patch with
    both: see _spike_after_gibbs_ill_posed)"""
    shape = (12, 10, 14)
    n = 20
    rng = np.random.RandomState(5)
    gon = (np.arange(n) % 3 == 0).astype(np.uint8)
    son = (np.arange(n) % 3 == 1).astype(np.uint8)
    alpha = rng.uniform(0.2, 0.7, n)
    for i in range(n):                       # keep the radii clear of every bin distance
        while True:
            try:
                _check_radius_margin(shape, ar.gibbs_radius(np.float32(alpha[i]), shape))
                break
            except AssertionError:
                alpha[i] += 0.0031
    loc = np.stack([rng.randint(0, s, n) for s in shape], 1)
    _ks_case(shape, 2, gon, alpha, son, loc, rng.rand(n), None, KS_TIGHT, "20 patches")


# ----------------------------------------------------------------------------------------- chain
class _Net:
    device = torch.device(DEV)
    num_classes = 3


def _cache(shapes, c, seed):
    """a CachedVolumes of synthetic volumes, built the way bench.py's fit mode builds one"""
    from segmantic_amd.seg import streams, trainer
    cache = trainer.CachedVolumes.__new__(trainer.CachedVolumes)
    cache.items, cache.device = [], torch.device(DEV)
    cache._stream = streams.shared_stream(DEV, streams.AUX)
    cache._pinned = torch.empty(4096, dtype=torch.int64).pin_memory()
    g = torch.Generator().manual_seed(seed)
    host = []
    for shp in shapes:
        img = torch.randn((c,) + tuple(shp), generator=g)
        lab = torch.zeros(tuple(shp))
        lab[4:-6, 5:-4, 3:-5] = 1.0
        lab[shp[0] // 2:, :shp[1] // 2, 6:] = 2.0
        flat = lab.reshape(-1).long()
        idx = [torch.nonzero(flat == k).reshape(-1) for k in range(3)]
        counts = np.array([int(t.numel()) for t in idx], dtype=np.int64)
        cache.items.append({"image": img.to(DEV), "label": lab[None].to(DEV), "class_all": torch.cat(idx).to(DEV),
                            "class_counts": counts, "class_offsets": np.concatenate([[0], np.cumsum(counts)[:-1]]),
                            "image_ndhwc": img.permute(1, 2, 3, 0).contiguous()[None].to(DEV),
                            "label_dhw": lab.contiguous().to(DEV)})
        host.append((img.numpy().astype(np.float64), lab.numpy().astype(np.float64)))
    return cache, host


def _spike_after_gibbs_ill_posed(x, draws, i):
    """Gibbs and spike on one patch, and the mask zeroed some bin together with its conjugate: such a
    bin is 0 in exact arithmetic and round-off in any float arithmetic (1e-16 relative in float64,
    1e-7 in f32), and the spike's mean(log(|K| + 1e-10)) takes its log -- the reference itself is not
    determined to better than a few 1e-4 there (an f32 evaluation differs from a float64 one by that)."""
    if draws is None or not (draws[3][0][i] and draws[4][0][i]):
        return False
    shp = x.shape[1:]
    r = ar.gibbs_radius(draws[3][1][i], shp)
    idx = [np.arange(n) for n in shp]
    d = [(i_ - (n - 1) / 2.0) ** 2 for i_, n in zip(idx, shp)]
    dm = [(ar.mirror(i_, n) - (n - 1) / 2.0) ** 2 for i_, n in zip(idx, shp)]
    dist = np.sqrt(d[0][:, None, None] + d[1][None, :, None] + d[2][None, None, :])
    mdist = np.sqrt(dm[0][:, None, None] + dm[1][None, :, None] + dm[2][None, None, :])
    return bool(((dist > r) & (mdist > r)).any())


# (flip_prob, augment_spatial, num_samples, seed): the seeds give draws in which every intensity and
# k-space transform fires at least once (asserted below) and, with augment_spatial, a warp
CHAIN = [(0.0, False, 4, 0), (1.0, False, 4, 0), (0.5, False, 20, 1), (1.0, False, 20, 1),
         (0.5, True, 4, 1), (1.0, True, 20, 2)]


@pytest.mark.parametrize("flip_prob,spatial,num_samples,seed", CHAIN)
def test_make_batch_matches_the_reference_chain(flip_prob, spatial, num_samples, seed):
    """make_batch == reference order (crop -> contrast -> histogram shift -> bias field -> Gibbs ->
    spike -> flip) for the same draws, 2 volumes x num_samples patches, even roi extents (where the
    Gibbs mask is not mirror-symmetric)."""
    from segmantic_amd.seg import trainer
    roi = (24, 20, 16)
    shapes = [(40, 36, 30), (34, 28, 26)]
    cache, host = _cache(shapes, 2, 17)

    class N(_Net):
        spatial_size, augment_intensity, augment_spatial = list(roi), True, spatial
    N.num_samples, N.flip_prob = num_samples, flip_prob
    rng = np.random.RandomState(seed)
    records = trainer.draw_batch(N, cache, [0, 1], rng)
    batch = trainer.apply_batch(N, cache, records)
    torch.cuda.synchronize()
    got_i = batch["image"].cpu().numpy()
    got_l = batch["label"].cpu().numpy()[:, 0]
    assert got_i.shape == (2 * num_samples, 2) + roi
    fired = np.zeros(5, int)
    row, compared, skipped, worst = 0, 0, 0, 0.0
    for rec in records:
        image, label = host[rec["vid"]]
        ri, rl, src = ar.reference_chain(image, label, rec, roi)
        fired += [int(np.asarray(t[0]).sum()) for t in rec["intensity"]]
        shp = image.shape[1:]
        for i in range(len(rec["starts"])):
            g, want = got_i[row + i], ri[i]
            if src is None:
                assert np.array_equal(got_l[row + i], rl[i])
                # f32 chain on exact crops: INT_RTOL for the intensity part, KS_TIGHT for Gibbs / spike
                tol = (INT_RTOL + KS_TIGHT) * max(1.0, float(np.abs(want).max()))
            else:
                delta = _coord_error_bound(rec["spatial"], shp)
                bad = got_l[row + i] != rl[i]
                assert not (bad & ~ar.near_half(src[i], shp, 2 * delta)).any()
                # the warp's coordinate error (<= 3 delta * slope, ~1e-5 of the range) passes through
                # x ** gamma: with gamma = 0.5 next to the patch minimum an error e becomes sqrt(e) ~ 3e-3
                tol = 5e-3 * max(1.0, float(np.abs(want).max()))
            if _spike_after_gibbs_ill_posed(want, rec["intensity"], i):
                skipped += 1
                continue
            compared += 1
            err = float(np.abs(g - want).max())
            worst = max(worst, err / max(1.0, float(np.abs(want).max())))
            assert err <= tol, (rec["vid"], i, rec["flips"][i], err, tol)
        row += len(rec["starts"])
    assert row == 2 * num_samples and compared >= row - 2, (compared, skipped)
    print(f"MEASURED chain flip_prob {flip_prob} spatial {spatial} n {num_samples}: {worst:.3e} "
          f"(bounds per patch above)")
    assert fired.min() >= 1, fired                       # each of the five transforms was exercised
    if spatial:
        assert all(r["spatial"] is not None for r in records)
    if flip_prob == 1.0:
        assert all(f == 7 for r in records for f in r["flips"])
    if flip_prob == 0.0:
        assert all(f == 0 for r in records for f in r["flips"])
