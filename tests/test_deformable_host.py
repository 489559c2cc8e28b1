"""B-spline deformable registration without a GPU: the numpy restatement in
tests/helpers/deformable_ref.py against finite differences, against a known field of the analytic phantom and against
seeded faults, and the host side of the package: subdivision, spans, the transform file, refusals, the scripts'
arguments."""
import functools
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import deformable_ref as D  # noqa: E402
import registration_ref as R  # noqa: E402

from segmantic_amd.image import processing as P  # noqa: E402
from segmantic_amd.image import registration as reg  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------- subdivision, spans
@pytest.mark.parametrize("full, n_zyx, flat", [((9, 10, 11), (4, 5, 6), (False, False, False)),
                                               ((1, 10, 11), (4, 5, 7), (False, False, True))])
def test_the_refined_grid_reproduces_the_coarse_field(full, n_zyx, flat):
    rng = np.random.default_rng(0)
    phi = rng.standard_normal((3,) + n_zyx)
    fine = reg.refine_grid(phi, flat)
    assert fine.tobytes() == D.refine_grid(phi, flat).tobytes()
    want_shape = tuple(n if fl else 2 * n - 3 for n, fl in zip(n_zyx, reversed(flat)))
    assert fine.shape == (3,) + want_shape
    coarse_u = D.displacement(phi, full, full, (1, 1, 1))
    fine_u = D.displacement(fine, full, full, (1, 1, 1))
    assert np.abs(coarse_u).max() > 0.1 and np.abs(fine_u - coarse_u).max() <= 1e-12
    if flat[2]:
        assert not coarse_u[2].any()                        # the component of the flat axis is 0


def test_spans_per_level_follow_grid_spacing():
    # extent 47 x 43 x 42.9 mm; three levels, 16 mm on the finest: 47 / 64 -> 1, doubled twice
    assert reg.control_spans((48, 44, 40), (1.0, 1.0, 1.1), 16.0, 3) == [(1, 1, 1), (2, 2, 2), (4, 4, 4)]
    assert reg.control_spans((48, 44, 40), (1.0, 1.0, 1.1), 8.0, 2) == [(3, 3, 3), (6, 6, 6)]
    assert reg.control_spans((256, 256, 100), (1.0, 1.0, 2.5), (16.0, 16.0, 20.0), 3) == [(4, 4, 3), (8, 8, 6), (16, 16, 12)]
    assert reg.control_spans((64, 48), (1.0, 1.0), 8.0, 2) == [(4, 3, 1), (8, 6, 1)]        # 2-D: z stays one span
    assert reg.control_spans((64, 48, 1), (1.0, 1.0, 3.0), 8.0, 2) == [(4, 3, 1), (8, 6, 1)]
    for args in (((48, 44, 40), (1.0, 1.0, 1.1), 16.0, 3), ((64, 48), (1.0, 1.0), 8.0, 2)):
        assert reg.control_spans(*args) == D.control_spans(*args)
    # 256^3 at 1 mm with 8 mm spacing: 32 spans -> 35^3 = 42 875 points
    with pytest.raises(ValueError, match="grid_spacing.*42875 control points"):
        reg.control_spans((256, 256, 256), (1.0, 1.0, 1.0), 8.0, 3)
    assert reg.control_spans((256, 256, 256), (1.0, 1.0, 1.0), 16.0, 3)[-1] == (16, 16, 16)
    for bad in (0.0, -4.0, float("nan"), (8.0, 8.0), "wide"):
        with pytest.raises((ValueError, TypeError), match="grid_spacing"):
            reg.control_spans((48, 44, 40), (1.0, 1.0, 1.1), bad, 2)


# ---------------------------------------------------------------------------- the gradient
@functools.lru_cache(maxsize=None)
def _small_pair():
    """12 x 11 x 10 fixed bins and a smooth 14 x 13 x 12 moving image under oblique geometry and a rigid matrix"""
    rng = np.random.default_rng(2)
    fsize, msize = (12, 11, 10), (14, 13, 12)
    fixed = R.Grid(np.zeros((10, 11, 12), np.float32), (1.0, 1.1, 1.2), (-5.0, -5.5, -5.0), R.rot_z(0.1) @ R.rot_x(0.05))
    origin = (-6.5, -6.0, -5.5)
    pm = R._points(msize, (1.0, 1.0, 1.0), origin)
    mov = (np.sin(0.45 * pm[..., 0] + 0.3) * np.cos(0.4 * pm[..., 1])
           + 0.6 * np.sin(0.5 * pm[..., 2] + 0.2 * pm[..., 0])).astype(np.float32)
    moving = R.Grid(mov, (1.0, 1.0, 1.0), origin, R.rot_y(-0.08))
    a = R.rigid_truth(fsize, None, (2.0, -3.0, 4.0), (0.3, -0.2, 0.4))
    bins = 16
    fbin = rng.integers(0, bins, (10, 11, 12)).astype(np.uint8)
    phi = rng.uniform(-0.6, 0.6, (3, 5, 5, 6))
    mlo, mhi = float(mov.min()), float(mov.max())
    return dict(fixed=fixed, moving=moving, a=a, fbin=fbin, mov=mov, phi=phi, full=(10, 11, 12), bins=bins, mlo=mlo,
                mscale=(bins - 1) / (mhi - mlo), mrange=mhi - mlo, m=R.index_map(moving, fixed, a),
                r=D.r_matrix(moving, fixed, a))


def _s_float(c, phi, metric):
    h = D.ffd_joint_histogram(c["fbin"], c["mov"], phi[None], c["full"], (1, 1, 1), c["m"], c["r"], c["bins"], c["mlo"],
                              c["mscale"], unquantised=True)[0]
    return D.metric_float(h, metric), h


@pytest.mark.parametrize("metric", ["nmi", "mi"])
def test_the_analytic_gradient_agrees_with_central_differences(metric):
    """Central differences (eps = 1e-4 mm) of the metric of the unquantised table are the reference.  Measured on
    the CPU: the largest difference over 16 entries is 6e-9 of the largest gradient entry (nmi and mi alike; 3e-9 at
    eps = 1e-3, 5e-8 at 1e-5, where the rounding of S takes over).  The bound 1e-6 leaves a factor of 170; a wrong sign, a
    transposed matrix in one of the two places or a missing factor is off by 1e-1 and more."""
    c = _small_pair()
    _, h = _s_float(c, c["phi"], metric)
    assert h.sum() > 0.8 * c["fbin"].size
    _, d, _, _ = D.derivative_table(h, metric)
    g = D.gradient_float(c["fbin"], c["mov"], c["phi"], c["full"], (1, 1, 1), c["m"], c["r"], c["bins"], c["mlo"],
                         c["mscale"], d, h.sum())
    rng = np.random.default_rng(5)
    eps, worst = 1e-4, 0.0
    for _ in range(16):
        ix = tuple(int(rng.integers(0, s)) for s in c["phi"].shape)
        up, down = c["phi"].copy(), c["phi"].copy()
        up[ix] += eps
        down[ix] -= eps
        fd = (_s_float(c, up, metric)[0] - _s_float(c, down, metric)[0]) / (2 * eps)
        worst = max(worst, abs(fd - g[ix]))
    print(f"{metric}: worst |fd - analytic| = {worst:.3e}, max |g| = {np.abs(g).max():.3e}")
    assert worst <= 1e-6 * np.abs(g).max()


def _integer_and_float_gradient(c, metric, phi=None, factors=(1, 1, 1), fbin=None, mov=None, m=None, r=None):
    phi = c["phi"] if phi is None else phi
    fbin, mov = c["fbin"] if fbin is None else fbin, c["mov"] if mov is None else mov
    m, r = c["m"] if m is None else m, c["r"] if r is None else r
    args = (fbin, mov, phi, c["full"], factors, m, r, c["bins"], c["mlo"], c["mscale"])
    h = D.ffd_joint_histogram(fbin, mov, phi[None], *args[3:])[0]
    counted = int(h.sum()) // D.UNIT
    _, d, dmax, qd = D.derivative_table(h, metric)
    assert np.abs(qd).max() == D.QD_UNIT
    gscale = 1.0 / (c["mrange"] * float(np.abs(r).sum(axis=1).max()))
    gi = D.descale(D.ffd_gradient(*args, gscale, qd), dmax, c["mscale"], gscale, counted)
    return gi, D.gradient_float(*args, d, counted)


def _cosine(a, b):
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("metric", ["nmi", "mi"])
def test_the_integer_gradient_points_where_the_float64_one_does(metric):
    """the condition of the issue: cosine >= 0.99.  Measured on this pair: 0.999999 for nmi and for mi."""
    gi, gf = _integer_and_float_gradient(_small_pair(), metric)
    cos = _cosine(gi, gf)
    print(f"{metric}: cosine {cos:.8f}, norm ratio {np.sqrt((gi * gi).sum() / (gf * gf).sum()):.6f}")
    assert cos >= 0.99


# ---------------------------------------------------------------------------- recovery
FIELD_AMPLITUDE, GRID_SPACING = 6.5, 8.0


@functools.lru_cache(maxsize=None)
def _recovery():
    (f, m), truth = D.make_deformed_pair(D.smooth_field((6, 6, 6), FIELD_AMPLITUDE, 1))
    return f, m, truth, D.register_deformable_ref(f, m, grid_spacing=GRID_SPACING, levels=(2, 1), max_iterations=10)


def test_a_known_field_of_the_phantom_is_recovered():
    """section 23's phantom (48 x 44 x 40 at (1, 1, 1.1) mm, 52 x 50 x 44 at (1.1, 0.9, 1) mm) under a seeded B-spline
    field of 6^3 control points, 2.0 mm mean displacement over the foreground; 10 iterations per level keep the test
    short (the full 60 reach 0.31 mm)."""
    f, m, truth, res = _recovery()
    before, after = D.residual(truth, res.control, f)
    print(f"mean foreground displacement error {before:.3f} -> {after:.3f} mm, iterations {res.iterations}, "
          f"J {[round(a[0], 4) for a in res.accepted]} -> {[round(v, 4) for v in res.level_values]}")
    assert 1.8 < before < 2.2                                # about 2 voxels
    assert after <= 0.5 * before and after < min(f.spacing)
    assert res.folded == 0 and res.min_jacobian > 0
    for level in res.accepted:                               # J rises with every accepted move of a level
        assert len(level) > 1 and all(b > a for a, b in zip(level, level[1:]))
    assert res.spans == [(3, 3, 3), (6, 6, 6)] and res.control.shape == (3, 9, 9, 9)


# ---------------------------------------------------------------------------- folds
def test_a_fold_is_counted_and_a_step_onto_it_is_skipped():
    full, n_xyz = (17, 19, 21), (7, 5, 6)
    h = D.control_spacing(tuple(reversed(full)), (1.0, 1.0, 1.0), n_xyz)
    inv_h = [1.0 / v for v in h]
    folding = np.zeros((3, 6, 5, 7))
    folding[0, :, :, 3] = 2.0 * h[0]                         # an adjacent control difference of twice the spacing
    gentle = folding * 0.1
    folded, lowest, dmap = D.jacobian(folding, full, full, (1, 1, 1), inv_h)
    assert folded > 0 and lowest < 0 and folded == int((dmap <= 0).sum())
    assert D.jacobian(gentle, full, full, (1, 1, 1), inv_h)[0] == 0
    assert D.jacobian(np.zeros_like(folding), full, full, (1, 1, 1), inv_h)[:2] == (0, 1.0)
    grids = [folding, gentle]
    folds_of = lambda i: D.jacobian(grids[i], full, full, (1, 1, 1), inv_h)[0]   # noqa: E731
    assert D.pick([2.0, 1.5], 1.0, folds_of) == (1, 1)       # the better candidate folds: refused, the next one taken
    assert D.pick([2.0, 0.5], 1.0, folds_of) == (None, 1)    # and nothing else is better: no move
    assert D.pick([0.9, 1.0], 1.0, folds_of) == (None, 0)    # "strictly better" is strict


# ---------------------------------------------------------------------------- seeded faults
def _gate_level_positions(fault):
    """the displacement of a level voxel is the full-resolution field at the middle of its block"""
    rng = np.random.default_rng(3)
    full, ff = (16, 18, 20), (2, 2, 2)
    phi = rng.standard_normal((3, 5, 6, 7))
    lvl = D.displacement(phi, (8, 9, 10), full, ff, fault)
    fine = D.displacement(phi, full, full, (1, 1, 1))
    # along an axis of even factor the block middle lies between two voxels: compare with the field there
    size = tuple(reversed(full))
    pts = np.stack(np.meshgrid(*[np.arange(n) * 2.0 + 0.5 for n in (10, 9, 8)], indexing="ij"), axis=-1)  # (x, y, z) order below
    pts = np.transpose(pts, (2, 1, 0, 3))
    want = D.field_at(phi, size, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), pts)
    assert np.abs(fine).max() > 0.1
    return bool(np.abs(np.stack([lvl[0], lvl[1], lvl[2]], axis=-1) - want).max() <= 1e-12)


def _gate_linear_precision(fault):
    """control values k along x give u_x = t + 1: the weights sit on the points k .. k + 3"""
    full = (5, 6, 23)
    phi = np.zeros((3, 4, 4, 8))
    phi[0] = np.arange(8.0)[None, None, :]
    u = D.displacement(phi, full, full, (1, 1, 1), fault)
    t = np.arange(23.0) * 5.0 / 22.0
    return bool(np.abs(u[0] - (t + 1.0)[None, None, :]).max() <= 1e-12)


def _gate_positions_are_physical(fault):
    """the sample position is the moving index of A (p + D_f u), formed from physical points"""
    c = _small_pair()
    f, mv = c["fixed"], c["moving"]
    u = D.displacement(c["phi"], c["full"], c["full"], (1, 1, 1))
    (zi, yi, xi), pos = D._positions(c["fbin"], u, c["m"], c["r"], fault)
    idx = np.stack([xi, yi, zi], axis=-1).astype(np.float64)
    uu = np.stack([u[k][zi, yi, xi] for k in range(3)], axis=-1)
    p = f.origin + (idx * f.spacing) @ f.direction.T
    q = (p + uu @ f.direction.T) @ c["a"][:3, :3].T + c["a"][:3, 3]
    want = ((q - mv.origin) @ np.linalg.inv(mv.direction).T) / mv.spacing
    return bool(np.abs(np.stack(pos, axis=-1) - want).max() <= 1e-9)


def _gate_empty_cells(fault):
    """Lt is 0 where the table is empty, so max|D| and with it the quantisation step belong to populated cells"""
    c = _small_pair()
    h = D.ffd_joint_histogram(c["fbin"], c["mov"], c["phi"][None], c["full"], (1, 1, 1), c["m"], c["r"], c["bins"],
                              c["mlo"], c["mscale"])[0]
    lt, d, dmax, _ = D.derivative_table(h, "nmi", fault)
    assert (h == 0).any() and (h > 0).any()
    return bool((lt[h == 0] == 0).all() and dmax == np.abs(d).max() and dmax < 1.0)


def _gate_ties(fault):
    return D.pick([1.0, 2.0, 2.0, 0.5], 0.0, lambda i: 0, fault) == (1, 0)


@pytest.mark.parametrize("fault, gate", [("no_level_offset", _gate_level_positions),
                                         ("weights_k_plus_1", _gate_linear_precision),
                                         ("r_transposed", _gate_positions_are_physical),
                                         ("empty_cells_kept", _gate_empty_cells), ("ties_last", _gate_ties)])
def test_each_seeded_fault_is_caught(fault, gate):
    assert fault in D.FAULTS
    assert gate(None) is True
    assert gate(fault) is False


# ---------------------------------------------------------------------------- the transform file
def _result(nd=3):
    rng = np.random.default_rng(9)
    data = np.zeros((10, 11, 12) if nd == 3 else (11, 12), np.float32)
    fixed = P.Image(data, (0.1 + 0.2,) * nd, tuple(1.0 / 3.0 for _ in range(nd)))
    a = np.eye(nd + 1)
    a[:nd, :] = rng.standard_normal((nd, nd + 1)) / 3.0
    control = rng.standard_normal((3, 4 if nd == 2 else 6, 5, 7)) * 1e-3 / 7.0
    return fixed, reg.DeformableResult(control, a, reg._Geometry.of(fixed), "nmi", 1.0 / 7.0, 0.01, [2, 1], [(2, 1, 1), (4, 2, 2)],
                                       [3, 4], [13, 17], [0.1, 0.3], [1.1, 1.2], True, 0, 2.0 / 3.0)


@pytest.mark.parametrize("nd", [2, 3])
def test_a_bspline_transform_reads_back_to_the_same_bits(tmp_path, nd):
    fixed, res = _result(nd)
    reg.save_transform(tmp_path / "t.json", res)
    doc = reg.load_transform(tmp_path / "t.json")
    back = doc["result"]
    assert doc["kind"] == "bspline" and isinstance(back, reg.DeformableResult)
    assert back.control.dtype == np.float64 and back.control.tobytes() == res.control.tobytes()
    assert back.affine.tobytes() == res.affine.tobytes() and back.control.shape == res.control.shape
    assert back.fixed.size == res.fixed.size and back.fixed.spacing == res.fixed.spacing
    assert back.fixed.origin == res.fixed.origin and back.fixed.direction == res.fixed.direction
    assert (back.metric, back.value, back.min_jacobian, back.folded) == ("nmi", 1.0 / 7.0, 2.0 / 3.0, 0)
    assert back.spans == res.spans and back.final_step == res.final_step and back.level_values == res.level_values
    # a matrix transform still needs its fixed image, and its file still loads
    rigid = reg.RegistrationResult(np.eye(nd + 1), np.zeros(3 if nd == 2 else 6), "rigid", "nmi", 1.5)
    with pytest.raises(ValueError, match="fixed image"):
        reg.save_transform(tmp_path / "r.json", rigid)
    reg.save_transform(tmp_path / "r.json", rigid, fixed)
    assert reg.load_transform(tmp_path / "r.json")["kind"] == "rigid"
    import json
    doc = json.loads((tmp_path / "t.json").read_text())
    doc["control"] = doc["control"][:-1]
    (tmp_path / "bad.json").write_text(json.dumps(doc))
    with pytest.raises(ValueError, match="control values"):
        reg.load_transform(tmp_path / "bad.json")


# ---------------------------------------------------------------------------- refusals
def test_arguments_are_refused_by_name_before_any_launch():
    """none of these touches the device: they raise their own error on a machine without one"""
    rng = np.random.default_rng(1)
    fixed = P.Image(rng.random((16, 16, 16)).astype(np.float32))
    moving = P.Image(rng.random((16, 16, 16)).astype(np.float32))
    for kwargs, name in ((dict(grid_spacing=0.0), "grid_spacing"), (dict(grid_spacing=(8.0, 8.0)), "grid_spacing"),
                         (dict(grid_spacing=0.3), "grid_spacing"), (dict(regularisation=-0.1), "regularisation"),
                         (dict(regularisation="much"), "regularisation"), (dict(metric="ssd"), "metric"),
                         (dict(bins=20), "bins"), (dict(levels=(3,)), "levels"), (dict(levels=()), "levels"),
                         (dict(min_overlap=1.5), "min_overlap"), (dict(max_iterations=0), "max_iterations"),
                         (dict(initial=np.eye(3)), "initial"), (dict(initial="centre"), "initial"),
                         (dict(fixed_mask=P.Image(np.zeros((8, 8, 8), np.uint8))), "fixed_mask")):
        with pytest.raises((ValueError, TypeError), match=name):
            reg.register_deformable(fixed, moving, **kwargs)
    with pytest.raises(ValueError, match="dimension mismatch"):
        reg.register_deformable(fixed, P.Image(np.zeros((16, 16), np.float32)))
    with pytest.raises(TypeError, match="moving must be a processing.Image"):
        reg.register_deformable(fixed, np.zeros((16, 16, 16), np.float32))
    _, res = _result()
    with pytest.raises(ValueError, match="geometry"):
        reg.warp(moving, fixed, res)                         # fitted on another grid
    with pytest.raises(TypeError, match="DeformableResult"):
        reg.warp(moving, fixed, np.eye(4))
    with pytest.raises(TypeError, match="DeformableResult"):
        reg.displacement_field(np.eye(4))
    with pytest.raises(TypeError, match="DeformableResult"):
        reg.jacobian_determinant(None)
    with pytest.raises(ValueError, match="at least 4 points"):
        reg.refine_grid(np.zeros((3, 3, 4, 4)))


# ---------------------------------------------------------------------------- the scripts' arguments
def test_register_images_takes_the_bspline_kind(tmp_path):
    from typer.testing import CliRunner
    cli = _load_script("register_images")
    env = {"COLUMNS": "200", "TERM": "dumb"}
    out = CliRunner().invoke(cli.app, ["fit", "--help"], env=env).output
    for opt in ("--grid-spacing", "--regularisation", "--initial", "bspline"):
        assert opt in out, opt
    assert "--save-jacobian" in CliRunner().invoke(cli.app, ["apply", "--help"], env=env).output
    for kwargs, name in ((dict(grid_spacing=8.0), "--grid-spacing"), (dict(regularisation=0.1), "--regularisation"),
                         (dict(initial=tmp_path / "a.json"), "--initial")):
        with pytest.raises(ValueError, match=name):          # before any file is read
            cli.fit(tmp_path / "m.nii.gz", tmp_path / "f.nii.gz", tmp_path / "t.json", "rigid", **kwargs)
    # apply reads the kind from the file: the two other interpolators are refused by name, a foreign grid too
    fixed, res = _result()
    reg.save_transform(tmp_path / "t.json", res)
    P.write_image(fixed, tmp_path / "f.nii.gz")
    P.write_image(P.Image(np.zeros((9, 9, 9), np.float32)), tmp_path / "other.nii.gz")
    for name in ("bspline", "label-gaussian"):
        with pytest.raises(ValueError, match=f"--interpolator {name}"):
            cli.apply(tmp_path / "f.nii.gz", tmp_path / "f.nii.gz", tmp_path / "o.nii.gz", tmp_path / "t.json", interpolator=name)
    with pytest.raises(ValueError, match="geometry"):
        cli.apply(tmp_path / "f.nii.gz", tmp_path / "other.nii.gz", tmp_path / "o.nii.gz", tmp_path / "t.json")
    r = CliRunner().invoke(cli.app, ["apply", str(tmp_path / "f.nii.gz"), str(tmp_path / "other.nii.gz"),
                                     str(tmp_path / "o.nii.gz"), "--transform", str(tmp_path / "t.json")], env=env)
    assert r.exit_code != 0 and "geometry" in r.output
    rigid = reg.RegistrationResult(np.eye(4), np.zeros(6), "rigid", "nmi", 1.5)
    reg.save_transform(tmp_path / "r.json", rigid, fixed)
    with pytest.raises(ValueError, match="--save-jacobian"):
        cli.apply(tmp_path / "f.nii.gz", tmp_path / "f.nii.gz", tmp_path / "o.nii.gz", tmp_path / "r.json",
                  save_jacobian=tmp_path / "j.nii.gz")


def test_multi_atlas_segment_arguments():
    from typer.testing import CliRunner
    cli = _load_script("multi_atlas_segment")
    out = CliRunner().invoke(cli.app, ["--help"], env={"COLUMNS": "200", "TERM": "dumb"}).output
    for opt in ("--atlas", "--tissue-list", "--grid-spacing", "TARGET", "OUTPUT"):
        assert opt in out, opt
    argv = ["t.nii", "o.nii", "--atlas", "a0.nii", "l0.nii", "--grid-spacing", "12", "--atlas", "a1.nii", "l1.nii"]
    assert cli.cli(argv) == ["t.nii", "o.nii", "--atlas", "a0.nii", "--atlas", "l0.nii", "--grid-spacing", "12",
                             "--atlas", "a1.nii", "--atlas", "l1.nii"]
    assert cli.pair_up([Path("a0"), Path("l0"), Path("a1"), Path("l1")]) == [(Path("a0"), Path("l0")), (Path("a1"), Path("l1"))]
    for bad in ([], [Path("a0")], [Path("a0"), Path("l0"), Path("a1")]):
        with pytest.raises(ValueError, match="--atlas"):
            cli.pair_up(bad)
    r = CliRunner().invoke(cli.app, cli.cli(["t.nii", "o.nii", "--atlas", "only-an-image.nii"]))
    assert r.exit_code != 0 and "--atlas" in r.output
    with pytest.raises(ValueError, match="atlases"):
        cli.segment(Path("t.nii"), Path("o.nii"), [(Path("a"), Path("l"))] * 17)
