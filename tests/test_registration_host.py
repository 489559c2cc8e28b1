"""Registration by mutual information without a GPU: the numpy restatement against a
per-voxel brute force and against known values, the package's host code (matrices, metric, search, level geometry)
against the restatement, the recovery of known transforms, the seeded faults each gate must reject, and the
argument checks."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import registration_ref as R  # noqa: E402

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.image import registration as reg  # noqa: E402
from segmantic_amd.image.processing import Image  # noqa: E402

FS, FP = (48, 44, 40), (1.0, 1.0, 1.1)                   # the fixed grid of the phantom: size and spacing (x, y, z)
RIGID_TRUTHS = [((6, -4, 8), (3, -2, 4)), ((-8, 5, 3), (-4, 3, 2)), ((4, 8, -6), (2, 4, -3))]   # degrees, mm


# ---------------------------------------------------------------------------- matrices
@pytest.mark.parametrize("nd", [2, 3])
def test_rigid_matrices_are_orthonormal_and_carry_the_centre_to_c_plus_t(nd):
    rng = np.random.default_rng(1)
    c, r = rng.normal(size=nd) * 20, 31.0
    for _ in range(5):
        q = rng.normal(size=R.N_PARAMETERS[nd]["rigid"]) * 8
        m = reg.parameters_to_matrix("rigid", nd, q, c, r)
        a = m[:nd, :nd]
        assert np.allclose(a @ a.T, np.eye(nd), atol=1e-14) and abs(np.linalg.det(a) - 1) < 1e-14
        assert np.allclose(a @ c + m[:nd, nd], c + q[-nd:], atol=1e-12)
        assert np.array_equal(m, R.parameters_to_matrix("rigid", nd, q, c, r))
    # one unit of a rotation parameter moves a point at distance r by 1 mm (to first order)
    m = reg.parameters_to_matrix("rigid", 3, [0, 0, 1.0, 0, 0, 0], np.zeros(3), r)
    p = np.array([r, 0, 0])
    assert abs(np.linalg.norm(m[:3, :3] @ p - p) - 1.0) < 1e-3


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("kind", ["translation", "rigid", "affine"])
def test_package_matrices_equal_the_restatement(nd, kind):
    rng = np.random.default_rng(2)
    n = R.N_PARAMETERS[nd][kind]
    assert n == reg.N_PARAMETERS[nd][kind] == {2: (2, 3, 6), 3: (3, 6, 12)}[nd][("translation", "rigid", "affine").index(kind)]
    for _ in range(4):
        q, c = rng.normal(size=n) * 5, rng.normal(size=nd) * 10
        assert np.array_equal(reg.parameters_to_matrix(kind, nd, q, c, 27.5), R.parameters_to_matrix(kind, nd, q, c, 27.5))
    assert np.array_equal(reg.parameters_to_matrix(kind, nd, np.zeros(n), c, 27.5)[:nd, :nd], np.eye(nd))


def test_affine_factors():
    """A = R diag(exp(s/r)) U: with no rotation the matrix is upper triangular with the scales on its diagonal"""
    r = 10.0
    q = np.array([0, 0, 0, 1.0, -2.0, 0.5, 0.3, -0.4, 0.2, 0, 0, 0])
    a = reg.parameters_to_matrix("affine", 3, q, np.zeros(3), r)[:3, :3]
    s = np.exp(q[3:6] / r)
    want = np.diag(s) @ np.array([[1, 0.03, -0.04], [0, 1, 0.02], [0, 0, 1]])
    assert np.allclose(a, want, atol=1e-15)


# ---------------------------------------------------------------------------- metric
def test_metric_known_values():
    B = 16
    rng = np.random.default_rng(3)
    pf, pm = rng.integers(1, 50, B), rng.integers(1, 50, B)
    indep = np.outer(pf, pm).astype(np.int64) * R.UNIT
    assert abs(R.metric_value(indep, "mi", 0)) < 1e-14
    assert abs(R.metric_value(indep, "nmi", 0) - 1.0) < 1e-14
    diag = np.diag(rng.integers(1, 50, B)).astype(np.int64) * R.UNIT
    assert abs(R.metric_value(diag, "nmi", 0) - 2.0) < 1e-14
    p = np.diag(diag) / np.diag(diag).sum()
    assert abs(R.metric_value(diag, "mi", 0) + (p * np.log(p)).sum()) < 1e-14
    # too few samples, no samples, one occupied cell
    assert R.metric_value(diag, "nmi", diag.sum() / R.UNIT + 1) == -np.inf
    assert R.metric_value(np.zeros((B, B), np.int64), "mi", 0) == -np.inf
    one = np.zeros((B, B), np.int64)
    one[3, 4] = 7 * R.UNIT
    assert R.metric_value(one, "nmi", 0) == -np.inf and R.metric_value(one, "mi", 0) == 0.0


@pytest.mark.parametrize("metric", ["nmi", "mi"])
def test_package_metric_equals_the_restatement(metric):
    rng = np.random.default_rng(4)
    h = rng.integers(0, 1 << 22, (6, 32, 32)).astype(np.int64)
    h[h < (1 << 21)] = 0
    h[4] = 0
    h[5] = 0
    h[5, 2, 2] = 5 * R.UNIT
    got = reg.metric_values(h, metric, 10.0)
    want = np.array([R.metric_value(t, metric, 10.0) for t in h])
    assert np.array_equal(got, want) and np.isfinite(got[:4]).all() and got[4] == -np.inf


# ---------------------------------------------------------------------------- pyramid level
def test_shrink_factors():
    assert R.shrink_factors((40, 44, 48), 4) == (4, 4, 4) == ops.shrink_factors((40, 44, 48), 4)
    assert R.shrink_factors((17, 24, 33), 4) == (2, 2, 4) == ops.shrink_factors((17, 24, 33), 4)
    assert R.shrink_factors((1, 40, 37), 8) == (1, 4, 4) == ops.shrink_factors((1, 40, 37), 8)
    assert R.shrink_factors((1, 5, 15), 2) == (1, 1, 1) == ops.shrink_factors((1, 5, 15), 2)
    assert R.shrink_factors((64, 64, 63), 8) == (8, 8, 4) == ops.shrink_factors((64, 64, 63), 8)
    with pytest.raises(ValueError, match="pyramid level"):
        ops.shrink_factors((8, 8, 8), 3)


def test_bin_shrink_restatement_on_a_hand_case():
    v = np.arange(2 * 4 * 5, dtype=np.int16).reshape(2, 4, 5)
    out = R.bin_shrink(v, (2, 2, 2))
    assert out.shape == (1, 2, 2) and out.dtype == np.float32
    assert out[0, 0, 0] == np.float32(v[:2, :2, :2].mean()) and out[0, 1, 1] == np.float32(v[:2, 2:4, 2:4].mean())


def _physical(g, idx_xyz):
    return g.origin + g.direction @ (np.asarray(idx_xyz, np.float64) * g.spacing)


def test_level_geometry_keeps_physical_positions():
    """voxel i of a level sits at the mean position of the voxels of its block"""
    th = 0.3
    d = R.rot_z(th) @ R.rot_x(-0.2)
    g = R.Grid(np.zeros((17, 24, 33), np.float32), (0.8, 1.1, 1.3), (5.0, -7.0, 2.0), d)
    ff = R.shrink_factors(g.data.shape, 4)                       # (z, y, x) = (2, 2, 4)
    fx = tuple(reversed(ff))
    lv = R.level_grid(g, R.bin_shrink(g.data, ff), fx)
    for idx in [(0, 0, 0), (3, 5, 2), (7, 11, 7)]:
        block = [np.arange(i * f, i * f + f) for i, f in zip(idx, fx)]
        want = np.mean([_physical(g, (x, y, z)) for x in block[0] for y in block[1] for z in block[2]], axis=0)
        assert np.allclose(_physical(lv, idx), want, atol=1e-12)
        bad = R.level_grid(g, lv.data, fx, fault="no_origin_shift")         # the seeded fault moves every voxel
        assert np.linalg.norm(_physical(bad, idx) - want) > 0.5
    # the package's level geometry is the same
    pg = reg.level_geometry(reg._Geometry(g.size, g.spacing, g.origin, g.direction.reshape(-1)), fx)
    assert pg.size == lv.size and np.array_equal(pg.spacing, lv.spacing) and np.array_equal(pg.origin, lv.origin)
    im = Image(torch.zeros(17, 24, 33), (0.8, 1.1, 1.3), (5.0, -7.0, 2.0), d.reshape(-1))
    assert np.array_equal(reg.grid_centre(reg._Geometry.of(im)), g.centre())
    assert reg.grid_radius(reg._Geometry.of(im)) == g.radius()


# ---------------------------------------------------------------------------- histogram
def _brute_histogram(fbin, mov, m, bins, mlo, mscale):
    """one candidate, voxel by voxel, in Python floats (IEEE doubles)"""
    nz, ny, nx = mov.shape
    h = np.zeros((bins, bins), np.int64)
    count = 0
    for z in range(fbin.shape[0]):
        for y in range(fbin.shape[1]):
            for x in range(fbin.shape[2]):
                fb = int(fbin[z, y, x])
                if fb == 255:
                    continue
                c = [((float(m[r][0]) * x + float(m[r][1]) * y) + float(m[r][2]) * z) + float(m[r][3]) for r in range(3)]
                if not all(0.0 <= c[r] <= n - 1 for r, n in enumerate((nx, ny, nz))):
                    continue
                count += 1
                i0 = [int(math.floor(v)) for v in c]
                fr = [v - math.floor(v) for v in c]
                i1 = [min(i0[r] + 1, n - 1) for r, n in enumerate((nx, ny, nz))]
                val = 0.0
                for corner in range(8):
                    px, py, pz = (i1[0] if corner & 1 else i0[0], i1[1] if corner & 2 else i0[1],
                                  i1[2] if corner & 4 else i0[2])
                    w = fr[0] if corner & 1 else 1.0 - fr[0]
                    w = w * (fr[1] if corner & 2 else 1.0 - fr[1])
                    w = w * (fr[2] if corner & 4 else 1.0 - fr[2])
                    val = val + w * float(mov[pz, py, px])
                b = min(max((val - mlo) * mscale, 0.0), bins - 1.0)
                i = min(int(math.floor(b)), bins - 2)
                q = int(math.floor((b - i) * 65536.0 + 0.5))
                h[fb, i] += 65536 - q
                h[fb, i + 1] += q
    return h, count


def _tiny_case():
    rng = np.random.default_rng(5)
    fbin = rng.integers(0, 16, (4, 5, 6)).astype(np.uint8)
    fbin[rng.random(fbin.shape) < 0.15] = 255
    mov = rng.normal(size=(5, 4, 7)).astype(np.float32)
    maps = np.array([[[1.02, 0.05, -0.03, 0.3], [-0.04, 0.9, 0.02, 0.2], [0.03, -0.02, 1.1, 0.1]],
                     [[0.9, 0.2, 0.0, 2.6], [-0.2, 0.9, 0.1, -1.3], [0.0, 0.1, 1.0, 1.7]],       # half outside
                     [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]],       # integer positions
                     [[1.0, 0.0, 0.0, 40.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]])     # entirely outside
    mlo, mhi = float(mov.min()), float(mov.max())
    return fbin, mov, maps, mlo, 15 / (mhi - mlo)


def test_restated_histogram_equals_a_per_voxel_loop():
    fbin, mov, maps, mlo, mscale = _tiny_case()
    got, counted = R.joint_histogram(fbin, mov, maps, 16, mlo, mscale)
    for t, m in enumerate(maps):
        want, n = _brute_histogram(fbin, mov, m, 16, mlo, mscale)
        assert np.array_equal(got[t], want) and counted[t] == n and got[t].sum() == n * R.UNIT
    assert counted[0] > 40 and 0 < counted[1] < counted[0] and counted[3] == 0 and not got[3].any()
    assert counted[2] == int((fbin[:4, :4, :6] != 255).sum())           # the last moving row / plane counts too


@pytest.mark.parametrize("fault", ["truncate_q", "swap_axes", "border_clamp"])
def test_exact_histogram_comparison_rejects_seeded_faults(fault):
    fbin, mov, maps, mlo, mscale = _tiny_case()
    good, n_good = R.joint_histogram(fbin, mov, maps, 16, mlo, mscale)
    bad, n_bad = R.joint_histogram(fbin, mov, maps, 16, mlo, mscale, fault=fault)
    assert not np.array_equal(good, bad)
    if fault == "truncate_q":        # the sums cannot see it (each sample still weighs 2^16): only the cells do
        assert np.array_equal(good.sum(axis=(1, 2)), bad.sum(axis=(1, 2))) and np.array_equal(n_good, n_bad)
    if fault == "border_clamp":      # samples outside the moving image are counted at its border
        assert n_bad[1] > n_good[1] and n_bad[3] == int((fbin != 255).sum())


# ---------------------------------------------------------------------------- search
def _bump(cands):
    """two equal maxima at q0 = +1.5 and q0 = -1.5, and a ridge along q1"""
    return [-(abs(c[0]) - 1.5) ** 2 - 0.5 * (c[1] - 0.7) ** 2 for c in cands]


def test_pattern_search_by_hand_and_against_the_package():
    calls = []

    def ev(cands):
        calls.append(len(cands))
        return _bump(cands)
    q, value, its, evs, step = R.pattern_search(ev, np.zeros(2), 1.0, 1.0 / 32, 200)
    assert calls[0] == 1 and set(calls[1:]) == {4} and evs == 1 + 4 * its
    assert q[0] > 0                                        # the tie between +step and -step goes to +, tried first
    assert abs(q[0] - 1.5) < 1 / 32 and abs(q[1] - 0.7) < 1 / 32 and step == 1.0 / 64
    got = reg.pattern_search(_bump, np.zeros(2), 1.0, 1.0 / 32, 200)
    assert np.array_equal(got[0], q) and got[1:] == (value, its, evs, step)
    # an iteration limit stops it early, on a step that is still large
    q3, _, its3, evs3, step3 = R.pattern_search(_bump, np.zeros(2), 1.0, 1.0 / 32, 3)
    assert its3 == 3 and evs3 == 13 and step3 >= 1.0 / 32
    assert reg.pattern_search(_bump, np.zeros(2), 1.0, 1.0 / 32, 3)[2:] == (its3, evs3, step3)


def test_search_comparison_rejects_seeded_faults():
    good = R.pattern_search(_bump, np.zeros(2), 1.0, 1.0 / 32, 50)
    minus = R.pattern_search(_bump, np.zeros(2), 1.0, 1.0 / 32, 50, fault="minus_first")
    assert minus[0][0] < 0 < good[0][0]                    # the parameters differ: the other of the two maxima
    stuck = R.pattern_search(_bump, np.zeros(2), 1.0, 1.0 / 32, 50, fault="no_halving")
    assert stuck[2] == 50 and stuck[4] == 1.0 and (stuck[2], stuck[3], stuck[4]) != good[2:]
    assert abs(stuck[0][1] - 0.7) > 1 / 32                 # and it never gets closer than its first step allows


# ---------------------------------------------------------------------------- recovery
@pytest.mark.parametrize("case", range(len(RIGID_TRUTHS)))
def test_restatement_recovers_rigid_transforms(case):
    """Target registration error (largest displacement of the fixed box's corners between truth and result) below
    the smallest fixed spacing, 1.0 mm.  Measured: before 9.23 / 8.67 / 9.05 mm, after 0.10 / 0.10 / 0.06 mm with
    levels (4, 2, 1) and 519 / 567 / 531 evaluations."""
    ang, sh = RIGID_TRUTHS[case]
    truth = R.rigid_truth(FS, FP, ang, sh)
    fixed, moving = R.make_pair(truth)
    before = R.tre(fixed, truth, np.eye(4))
    r = R.register_ref(fixed, moving, "rigid", levels=(4, 2, 1))
    after = R.tre(fixed, truth, r.transform)
    assert before > 6.0 and after < min(FP), f"TRE before {before:.3f} mm, after {after:.3f} mm, {r.evaluations} evaluations"
    assert r.converged and r.evaluations[0] == 1 + 12 * r.iterations[0]


def test_restatement_recovers_an_affine_transform():
    """6 % scale, 3 % shear, a small rotation and shift; levels (4, 2) keep the test at a few seconds.  Measured:
    TRE before 5.88 mm, after 0.44 mm with 1009 + 553 evaluations (0.23 mm after a third level at full resolution)."""
    truth = R.rigid_truth(FS, FP, (3, -2, 4), (2, -1.5, 1))
    lin = np.diag([1.06, 0.97, 1.03]) @ np.array([[1, 0.03, 0.0], [0, 1, -0.02], [0, 0, 1]])
    truth[:3, :3] = truth[:3, :3] @ lin
    fixed, moving = R.make_pair(truth)
    before = R.tre(fixed, truth, np.eye(4))
    r = R.register_ref(fixed, moving, "affine", levels=(4, 2))
    after = R.tre(fixed, truth, r.transform)
    assert before > 3.0 and after < min(FP), f"TRE before {before:.3f} mm, after {after:.3f} mm, {r.evaluations} evaluations"


# ---------------------------------------------------------------------------- refusals
def _img(shape=(12, 12, 12), dtype=torch.float32):
    return Image(torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape).to(dtype))


def test_refusals_are_raised_by_name_before_any_launch():
    f, m = _img(), _img()
    with pytest.raises(ValueError, match="unknown transform 'similarity'"):
        reg.register(f, m, transform="similarity")
    with pytest.raises(ValueError, match="unknown metric 'ncc'"):
        reg.register(f, m, metric="ncc")
    with pytest.raises(ValueError, match="bins must be one of"):
        reg.register(f, m, bins=48)
    with pytest.raises(ValueError, match="levels"):
        reg.register(f, m, levels=(4, 3))
    with pytest.raises(ValueError, match="levels"):
        reg.register(f, m, levels=())
    with pytest.raises(ValueError, match="dimension mismatch"):
        reg.register(f, _img((12, 12)))
    with pytest.raises(TypeError, match="moving must be a processing.Image"):
        reg.register(f, torch.zeros(4, 4, 4))
    with pytest.raises(TypeError, match="fixed must be a processing.Image"):
        reg.register(np.zeros((4, 4, 4)), m)
    with pytest.raises(ValueError, match="fixed_mask has size"):
        reg.register(f, m, fixed_mask=_img((12, 12, 11)))
    with pytest.raises(ValueError, match="initial"):
        reg.register(f, m, initial="centre")
    with pytest.raises(ValueError, match="initial"):
        reg.register(f, m, initial=np.eye(3))
    with pytest.raises(ValueError, match="min_overlap"):
        reg.register(f, m, min_overlap=1.5)
    with pytest.raises(ValueError, match="max_iterations"):
        reg.register(f, m, max_iterations=0)
    with pytest.raises(TypeError, match="unsupported pixel type"):
        reg.register(f, _img(dtype=torch.float64))


def test_op_wrappers_refuse_bad_arguments_without_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bin_shrink(torch.zeros(4, 4, 4), (2, 2, 2))
    assert ops.joint_histogram_group(16) == 32 and ops.joint_histogram_group(32) == 8
    assert ops.joint_histogram_group(64) == 2 and ops.joint_histogram_group(48) == 0
    assert ops.JOINT_HIST_UNIT == R.UNIT == reg.UNIT and ops.FIXED_BIN_IGNORE == R.IGNORE == reg.IGNORE


def test_transform_file_round_trip(tmp_path):
    f = Image(torch.zeros(4, 5, 6), (1.0, 1.1, 1.2), (0.1, 0.2, 0.3))
    m = reg.parameters_to_matrix("rigid", 3, [0.3, -0.2, 0.1, 1.5, -2.5, 0.7], np.array([1.0, 2.0, 3.0]), 9.0)
    res = reg.RegistrationResult(m, np.array([0.3, -0.2, 0.1, 1.5, -2.5, 0.7]), "rigid", "nmi", 1.2345678901234567,
                                 levels=[4, 2], iterations=[10, 7], evaluations=[121, 85], final_step=[0.1, 0.05],
                                 level_values=[1.2, 1.2345678901234567], converged=True, initial=np.eye(4))
    reg.save_transform(tmp_path / "t.json", res, f)
    doc = reg.load_transform(tmp_path / "t.json")
    assert np.array_equal(doc["matrix"], m) and np.array_equal(doc["parameters"], res.parameters)
    assert doc["kind"] == "rigid" and doc["metric"] == "nmi" and doc["value"] == res.value
    assert doc["fixed"] == {"size": [6, 5, 4], "spacing": [1.0, 1.1, 1.2], "origin": [0.1, 0.2, 0.3],
                            "direction": [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]}
    (tmp_path / "bad.json").write_text('{"kind": "rigid"}')
    with pytest.raises(ValueError, match="not a transform file"):
        reg.load_transform(tmp_path / "bad.json")
