"""Registration by mutual information on the GPU against the numpy restatement in
tests/helpers/registration_ref.py.  Every comparison is exact: the kernels' sums are integers and every
floating-point step is specified operation by operation."""
import functools
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import registration_ref as R  # noqa: E402

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.image import processing as P  # noqa: E402
from segmantic_amd.image import registration as reg  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
DTYPES = {"float32": np.float32, "uint8": np.uint8, "int16": np.int16, "uint16": np.uint16, "int32": np.int32}
FS, FP = (48, 44, 40), (1.0, 1.0, 1.1)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "float32":
        return (rng.normal(size=shape) * 40).astype(np.float32)
    info = np.iinfo(DTYPES[dtype])
    lo, hi = max(info.min, -(1 << 20)), min(info.max, 1 << 20)
    return rng.integers(lo, hi, shape, endpoint=True).astype(DTYPES[dtype])


# ---------------------------------------------------------------------------- pyramid level, fixed bins
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", [(17, 24, 33), (1, 40, 37)])
def test_bin_shrink_and_fixed_bins_equal_the_restatement(shape, dtype):
    vol = _volume(shape, dtype, 11)
    rng = np.random.default_rng(12)
    mask = (rng.random(shape) < 0.6).astype(np.uint8)
    for level in (2, 4):
        ff = R.shrink_factors(shape, level)
        assert ff == ops.shrink_factors(shape, level)
        want = R.bin_shrink(vol, ff)
        got = ops.bin_shrink(_dev(vol), ff)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
        mm = ops.bin_shrink(_dev(mask), ff)
        assert np.array_equal(mm.cpu().numpy(), R.bin_shrink(mask, ff))
        lo, hi = float(want.min()), float(want.max())
        assert (lo, hi) == (float(got.min()), float(got.max()))
        for bins in (16, 64):
            plain = R.fixed_bins(want, lo, hi, bins)
            assert np.array_equal(ops.fixed_bins(got, lo, hi, bins).cpu().numpy(), plain)
            assert plain.min() == 0 and plain.max() == bins - 1
            wb = R.fixed_bins(want, lo, hi, bins, R.bin_shrink(mask, ff))
            gb = ops.fixed_bins(got, lo, hi, bins, mm).cpu().numpy()
            assert np.array_equal(gb, wb) and (wb == 255).any() and (wb != 255).any()


def test_bin_shrink_beyond_one_pass_of_its_grid():
    """more output voxels than SEGMI_BIN_SHRINK_GRID_CAP * 256 lanes: the stride loop takes a second trip"""
    shape = (16, 260, 2 * 130)                              # 16 * 260 * 130 outputs = 540 800 > 524 288
    vol = _volume(shape, "int16", 13)
    got = ops.bin_shrink(_dev(vol), (1, 1, 2))
    assert got.numel() > 2048 * 256 and np.array_equal(got.cpu().numpy(), R.bin_shrink(vol, (1, 1, 2)))


# ---------------------------------------------------------------------------- joint histogram
F_SHAPE, M_SHAPE = (17, 24, 33), (19, 21, 35)


def _candidate_maps(n):
    """n index maps from near the identity, through half outside, to (the last) entirely outside"""
    maps = []
    for k in range(n):
        s = k / max(n - 1, 1)
        a = 0.02 + 0.1 * s
        rot = R.rot_z(a) @ R.rot_y(-0.5 * a) @ R.rot_x(0.3 * a)
        m = np.zeros((3, 4))
        m[:, :3] = rot * np.array([1.03, 0.9, 1.05])
        m[:, 3] = np.array([0.4 + 34.0 * s, 0.3 - 6.0 * s, 0.6 + 8.0 * s])
        maps.append(m)
    maps[-1][:, 3] = (80.0, 0.0, 0.0)
    return np.array(maps)


@functools.lru_cache(maxsize=None)
def _hist_case(bins, dtype="float32"):
    rng = np.random.default_rng(21)
    fbin = rng.integers(0, bins, F_SHAPE).astype(np.uint8)
    fbin[rng.random(F_SHAPE) < 0.1] = 255                    # ignored samples
    mov = _volume(M_SHAPE, dtype, 22)
    if dtype == "float32":                                   # smooth enough that neighbouring lanes share cells
        z, y, x = np.meshgrid(*[np.arange(n) for n in M_SHAPE], indexing="ij")
        mov = (mov * 0.05 + 20 * np.sin(x / 5.0) + 15 * np.cos(y / 4.0) + z).astype(np.float32)
    maps = np.concatenate([_candidate_maps(31), _candidate_maps(2)[1:]])      # 32, the last one entirely outside
    mlo, mhi = float(mov.min()), float(mov.max())
    mscale = (bins - 1) / (mhi - mlo)
    want, counted = R.joint_histogram(fbin, mov, maps, bins, mlo, mscale)
    return fbin, mov, maps, mlo, mscale, want, counted


def _candidate_counts(bins):
    g = ops.joint_histogram_group(bins)
    return sorted({t for t in (1, g, g + 1, 32) if t <= 32})


@pytest.mark.parametrize("bins", [16, 32, 64])
def test_joint_histogram_equals_the_restatement(bins):
    fbin, mov, maps, mlo, mscale, want, counted = _hist_case(bins)
    assert ops.joint_histogram_group(bins) == {16: 32, 32: 8, 64: 2}[bins]
    assert counted[0] > 0.8 * (fbin != 255).sum() and not want[-1].any() and counted[-1] == 0
    assert (0 < counted[12:20]).all() and (counted[12:20] < 0.6 * counted[0]).all()      # the half-outside ones
    fb, mv = _dev(fbin), _dev(mov)
    for T in _candidate_counts(bins):
        pick = list(range(T - 1)) + [31] if T > 1 else [0]                                # the last: all outside
        got = ops.joint_histogram(fb, mv, maps[pick], bins, mlo, mscale)
        assert got.dtype == torch.int64 and got.shape == (T, bins, bins) and got.is_cuda
        g = got.cpu().numpy()
        assert np.array_equal(g, want[pick]), f"bins {bins}, T {T}"
        assert np.array_equal(g.sum(axis=(1, 2)), counted[pick] * R.UNIT)
        again = ops.joint_histogram(fb, mv, maps[pick], bins, mlo, mscale)               # the same bits every time
        assert torch.equal(got, again)


@pytest.mark.parametrize("dtype", ["uint8", "int16", "uint16", "int32"])
def test_joint_histogram_reads_the_native_pixel_type(dtype):
    fbin, mov, maps, mlo, mscale, want, counted = _hist_case(32, dtype)
    pick = [0, 5, 14, 31]
    got = ops.joint_histogram(_dev(fbin), _dev(mov), maps[pick], 32, mlo, mscale).cpu().numpy()
    assert np.array_equal(got, want[pick]) and np.array_equal(got.sum(axis=(1, 2)), counted[pick] * R.UNIT)


def test_joint_histogram_past_the_counter_and_grid_limits():
    """SEGMI_JOINT_HIST_GRID_CAP * 65 536 voxels plus a ragged remainder, every sample in one cell: each workgroup adds
    more than 2^32 to one 32-bit LDS counter (only the flush interval keeps it exact) over more than one pass of the
    capped grid.  The expected table is analytic."""
    n = ops.JOINT_HIST_GRID_CAP * 65536 + 12345
    fbin = torch.full((1, 1, n), 5, dtype=torch.uint8, device=DEV)
    mov = torch.full((1, 1, n), 3, dtype=torch.uint8, device=DEV)
    ident = np.zeros((2, 3, 4))
    ident[:, 0, 0] = ident[:, 1, 1] = ident[:, 2, 2] = 1.0
    got = ops.joint_histogram(fbin, mov, ident, 16, 0.0, 1.0)
    want = torch.zeros((2, 16, 16), dtype=torch.int64)
    want[:, 5, 3] = n * R.UNIT
    assert n * R.UNIT > (1 << 32) * ops.JOINT_HIST_GRID_CAP and torch.equal(got.cpu(), want)


def test_joint_histogram_refusals():
    fb, mv = torch.zeros((4, 4, 4), dtype=torch.uint8, device=DEV), torch.zeros((4, 4, 4), device=DEV)
    ident = np.eye(4)[None, :3]
    with pytest.raises(ValueError, match="bins must be one of"):
        ops.joint_histogram(fb, mv, ident, 48, 0.0, 1.0)
    with pytest.raises(ValueError, match="1 <= T <= 32"):
        ops.joint_histogram(fb, mv, np.repeat(ident, 33, 0), 16, 0.0, 1.0)
    with pytest.raises(TypeError, match="fixed bins are uint8"):
        ops.joint_histogram(mv, mv, ident, 16, 0.0, 1.0)
    with pytest.raises(ValueError, match="constant"):
        ops.fixed_bins(mv, 1.0, 1.0, 16)
    with pytest.raises(ValueError, match="constant at pyramid level"):
        reg.register(P.Image(torch.zeros(16, 16, 16)), P.Image(torch.rand(16, 16, 16)), levels=(1,))


# ---------------------------------------------------------------------------- the whole registration
def _image(g: R.Grid) -> P.Image:
    return P.Image(torch.from_numpy(g.data), g.spacing, g.origin, g.direction.reshape(-1))


def _same(res: reg.RegistrationResult, ref: R.RefResult, what=""):
    assert np.array_equal(res.parameters, ref.parameters), f"{what}: parameters {res.parameters} / {ref.parameters}"
    assert np.array_equal(res.transform, ref.transform), what
    assert res.iterations == ref.iterations and res.evaluations == ref.evaluations, \
        f"{what}: {res.iterations} {res.evaluations} / {ref.iterations} {ref.evaluations}"
    assert res.final_step == ref.final_step and res.level_values == ref.level_values and res.value == ref.value, what
    assert res.converged == ref.converged


@functools.lru_cache(maxsize=None)
def _pair3d():
    truth = R.rigid_truth(FS, FP, (6, -4, 8), (3, -2, 4))
    return (truth,) + R.make_pair(truth)


@pytest.mark.parametrize("kind", ["translation", "rigid", "affine"])
def test_register_equals_the_restatement(kind):
    truth, fixed, moving = _pair3d()
    ref = R.register_ref(fixed, moving, kind, levels=(4, 2))
    res = reg.register(_image(fixed), _image(moving), transform=kind, levels=(4, 2))
    _same(res, ref, kind)
    assert res.kind == kind and res.metric == "nmi" and res.levels == [4, 2] and sum(res.iterations) > 10
    if kind != "translation":
        err = R.tre(fixed, truth, res.transform)
        assert err < 1.0, f"TRE {err:.3f} mm"


def test_register_at_full_resolution_from_a_native_int16_image_with_mi():
    truth, fixed, moving = _pair3d()
    moving16 = R.Grid(np.round(moving.data * 2000).astype(np.int16), moving.spacing, moving.origin, moving.direction)
    ref = R.register_ref(fixed, moving16, "rigid", metric="mi", bins=64, levels=(2, 1))
    res = reg.register(_image(fixed), _image(moving16), transform="rigid", metric="mi", bins=64, levels=(2, 1))
    _same(res, ref, "rigid (2, 1) int16 mi")
    err = R.tre(fixed, truth, res.transform)
    assert err < 1.0, f"TRE {err:.3f} mm"


def test_register_with_a_fixed_mask_and_a_matrix_start():
    truth, fixed, moving = _pair3d()
    mask = np.zeros(fixed.data.shape, np.uint8)
    mask[4:-3, 5:-4, 3:-6] = 1
    gmask = R.Grid(mask, fixed.spacing, fixed.origin, fixed.direction)
    start = R.rigid_truth(FS, FP, (4, -2, 5), (2, -1, 3))
    ref = R.register_ref(fixed, moving, "rigid", bins=16, levels=(4, 2), fixed_mask=gmask, initial=start)
    res = reg.register(_image(fixed), _image(moving), transform="rigid", bins=16, levels=(4, 2), fixed_mask=_image(gmask),
                       initial=start)
    _same(res, ref, "mask")
    unmasked = R.register_ref(fixed, moving, "rigid", bins=16, levels=(4, 2), initial=start)
    assert unmasked.level_values != ref.level_values                   # the mask took part


def test_register_from_the_geometry_start():
    """the moving grid sits 30 mm away: without the start no sample overlaps, with it the offset is absorbed"""
    truth, fixed, moving = _pair3d()
    far = R.Grid(moving.data, moving.spacing, moving.origin + np.array([30.0, -45.0, 20.0]), moving.direction)
    ref = R.register_ref(fixed, far, "rigid", levels=(4, 2), initial="geometry")
    res = reg.register(_image(fixed), _image(far), transform="rigid", levels=(4, 2), initial="geometry")
    _same(res, ref, "geometry")
    shift = np.eye(4)
    shift[:3, 3] = (30.0, -45.0, 20.0)
    err = R.tre(fixed, shift @ truth, res.transform)
    assert err < 1.0, f"TRE {err:.3f} mm"
    lost = reg.register(_image(fixed), _image(far), transform="rigid", levels=(4,), max_iterations=3)
    assert lost.value == -np.inf and not lost.converged and lost.iterations == [3]


@pytest.mark.parametrize("kind", ["translation", "rigid", "affine"])
def test_register_a_2d_pair(kind):
    truth = R.rigid_truth((48, 44), (1.0, 0.9), (7,), (3.0, -2.5))
    fixed, moving = R.make_pair(truth, (48, 44), (1.0, 0.9), (52, 50), (1.1, 0.8), seed=3)
    ref = R.register_ref(fixed, moving, kind, levels=(2, 1))
    res = reg.register(_image(fixed), _image(moving), transform=kind, levels=(2, 1))
    _same(res, ref, f"2-D {kind}")
    assert res.transform.shape == (3, 3) and res.parameters.shape == ({"translation": 2, "rigid": 3, "affine": 6}[kind],)
    if kind != "translation":
        err = R.tre(fixed, truth, res.transform)
        assert err < 0.9, f"TRE {err:.3f} mm"


# ---------------------------------------------------------------------------- files
def _script():
    spec = importlib.util.spec_from_file_location("register_images", ROOT / "scripts" / "register_images.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fit_then_apply_through_files(tmp_path):
    truth, fixed, moving = _pair3d()
    lo, hi = np.quantile(moving.data, (0.1, 0.8))            # label 1: the brightest fifth, 2: the darkest tenth
    labels = (moving.data > hi).astype(np.uint8) + 2 * (moving.data < lo).astype(np.uint8)
    P.write_image(_image(fixed), tmp_path / "fixed.nii.gz")
    P.write_image(_image(moving), tmp_path / "moving.nii.gz")
    P.write_image(P.Image(torch.from_numpy(labels), moving.spacing, moving.origin), tmp_path / "labels.nii.gz")
    S = _script()
    r = S.fit(tmp_path / "moving.nii.gz", tmp_path / "fixed.nii.gz", tmp_path / "t.json", "rigid", "nmi", S.parse_levels("4,2"))
    f, m, lab = (P.read_image(tmp_path / n) for n in ("fixed.nii.gz", "moving.nii.gz", "labels.nii.gz"))
    direct = reg.register(f, m, transform="rigid", levels=(4, 2))
    doc = reg.load_transform(tmp_path / "t.json")
    assert np.array_equal(doc["matrix"], r.transform) and np.array_equal(direct.transform, r.transform)
    assert doc["kind"] == "rigid" and doc["metric"] == "nmi" and doc["value"] == r.value and doc["fixed"]["size"] == list(FS)
    err = R.tre(fixed, truth, doc["matrix"])
    assert err < 1.0, f"TRE {err:.3f} mm"
    S.apply(tmp_path / "moving.nii.gz", tmp_path / "fixed.nii.gz", tmp_path / "out.nii.gz", tmp_path / "t.json")
    want = P.apply_transform(m, f, r.transform, False)
    out = P.read_image(tmp_path / "out.nii.gz")
    assert out.GetSize() == FS and np.array_equal(out.numpy(), want.numpy()) and out.numpy().std() > 0.1
    S.apply(tmp_path / "labels.nii.gz", tmp_path / "fixed.nii.gz", tmp_path / "lab_out.nii.gz", tmp_path / "t.json",
            interpolator="label-gaussian", sigma=0.8)
    want = P.apply_transform(lab, f, r.transform, False, interpolator=P.sitkLabelGaussian, sigma=0.8)
    out = P.read_image(tmp_path / "lab_out.nii.gz")
    assert out.GetPixelID() == P.sitkUInt8 and np.array_equal(out.numpy(), want.numpy()) and set(np.unique(out.numpy())) == {0, 1, 2}
