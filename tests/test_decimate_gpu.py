"""Mesh decimation on the MI355X against the float64 Python oracle of tests/helpers/decimate_ref.py: the device
and the oracle produce the same integer mesh.  The volume-drift bounds are the oracle's own
figures times 1.5 (a constant of the algorithm once the hash is fixed), the measure bound is the existing F 2^-52."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.helpers import decimate_ref as dref
from tests.helpers import surface_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SEAM_SHAPES = [(1, 1, 1), (1, 37, 70), (33, 47, 65), (48, 48, 48), (5, 9, 200), (9, 1, 1)]   # test_surfaces_gpu.SHAPES


def _extract(*a, **k):
    from segmantic_amd.image.surfaces import extract_surfaces
    return extract_surfaces(*a, **k)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _diag():
    d = np.zeros((4, 4, 4), np.uint8)
    d[1, 1, 1] = d[2, 2, 1] = 1
    return d


def _one():
    d = np.zeros((3, 3, 3), np.uint8)
    d[1, 1, 1] = 1
    return d


NAMED = {"ball": ref.ball, "torus": ref.torus, "noise": lambda: ref.noise((12, 14, 16), 3, 0.5, 1), "diag": _diag,
         "one": _one, "box": lambda: np.ones((5, 6, 7), np.uint8)}


def _invariants(v_in, f_in, v_out, f_out):
    """computed from the device output alone (no oracle)"""
    assert dref.no_degenerate_or_repeated_face(f_out)
    assert ref.directed_edge_balance(f_out)
    assert ref.euler_characteristic(len(v_out), f_out) == ref.euler_characteristic(len(v_in), f_in)
    assert dref.n_components(len(v_out), f_out) == dref.n_components(len(v_in), f_in)
    # vertices are an order-preserving subset: match greedily on the bit patterns
    rows_in = [tuple(r) for r in _bits(v_in).tolist()]
    i = 0
    kept = []
    for r in (tuple(r) for r in _bits(v_out).tolist()):
        while rows_in[i] != r:
            i += 1
        kept.append(i)
        i += 1
    if len(set(rows_in)) == len(rows_in):              # clamped relaxation can put two vertices on one point
        assert dref.faces_are_ordered_subset(f_in, f_out, np.asarray(kept))


def _check_against_oracle(lab, r, rounds=128, classes=None, invariants=True, **kw):
    """decimated extraction == oracle on the undecimated extraction, for every label"""
    plain = _extract(lab, **kw)
    got = _extract(lab, decimate=r, decimate_max_rounds=rounds, **kw)
    assert sorted(got) == sorted(plain)
    for c in (classes or sorted(plain)):
        p, s = plain[c], got[c]
        want = dref.decimate(p.vertices, p.faces, r, rounds)
        assert s.faces.dtype == np.int32 and s.vertices.dtype == np.float32
        assert s.faces.shape == want["faces"].shape, (c, s.faces.shape, want["faces"].shape)
        assert np.array_equal(s.faces, want["faces"]), c
        assert np.array_equal(_bits(s.vertices), _bits(p.vertices[want["kept"]])), c
        area, vol, abs_area, abs_vol = ref.measures(s.vertices, s.faces)
        f = s.faces.shape[0]
        assert abs(s.area - area) <= f * 2.0 ** -52 * abs_area
        assert abs(s.volume - vol) <= f * 2.0 ** -52 * abs_vol
        if invariants:
            _invariants(p.vertices, p.faces, s.vertices, s.faces)
    return plain, got


@pytest.mark.parametrize("T", [0, 5])
@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_shapes_bit_equal_to_the_oracle(name, T):
    lab = NAMED[name]()
    plain, got = _check_against_oracle(lab, 0.8, smooth_iterations=T)
    for c in got:
        fin, fout = plain[c].faces.shape[0], got[c].faces.shape[0]
        print(f"{name} T={T} label {c}: F {fin} -> {fout}, volume {plain[c].volume!r} -> {got[c].volume!r}")
        if name in ("ball", "torus"):
            assert fout <= math.ceil(0.2 * fin)
        if name in ("ball", "torus", "box"):
            assert got[c].volume > 0
        if name in ("one",):
            assert got[c].vertices.shape[0] >= 4


def test_kept_vertex_numbers_and_batch_of_meshes():
    """the low-level batch entry point: kept numbers bit-equal to the oracle, one workspace for all meshes"""
    from segmantic_amd import ops
    meshes = []
    for lab, c in ((ref.ball(), 1), (_one(), 1), (ref.noise((12, 14, 16), 3, 0.5, 1), 2), (ref.torus(), 1)):
        m = ref.surface_nets(lab, c, 2, 0.5)
        meshes.append((np.asarray(m["index"], np.float32), np.ascontiguousarray(m["faces"], dtype=np.int32)))
    starts = np.zeros((len(meshes) + 2, 2), np.int32)
    for i, (v, f) in enumerate(meshes):
        starts[i + 1] = starts[i] + (len(v), len(f))
    v = torch.from_numpy(np.concatenate([m[0] for m in meshes])).cuda()
    f = torch.from_numpy(np.ascontiguousarray(np.concatenate([m[1] for m in meshes]))).cuda()
    v0, f0 = v.clone(), f.clone()
    stats = {}
    ov, of, kept, out_starts, out_host = ops.decimate_meshes(v, f, torch.from_numpy(starts).cuda(), starts, 0.8, 128, stats)
    assert torch.equal(v, v0) and torch.equal(f, f0)
    assert np.array_equal(out_starts.cpu().numpy(), out_host)
    rounds = 0
    for i, (mv, mf) in enumerate(meshes):
        want = dref.decimate(mv, mf, 0.8)
        rounds = max(rounds, len(want["history"]))
        a, b = out_host[i], out_host[i + 1]
        assert np.array_equal(kept[a[0]:b[0]].cpu().numpy(), want["kept"]), i
        assert np.array_equal(of[a[1]:b[1]].cpu().numpy(), want["faces"]), i
        assert np.array_equal(_bits(ov[a[0]:b[0]].cpu().numpy()), _bits(mv[want["kept"]])), i
    # one device-to-host copy per round and one for the output totals
    assert stats["rounds"] == rounds and stats["d2h_copies"] == rounds + 1


@pytest.mark.parametrize("shape", SEAM_SHAPES)
def test_seam_shapes_four_classes(shape):
    lab = ref.noise(shape, 4, 0.1, 2, np.uint8)
    before = lab.copy()
    _check_against_oracle(lab, 0.8)
    assert np.array_equal(lab, before)


def test_seam_shape_one_class_dense():
    _check_against_oracle(ref.noise((33, 47, 65), 1, 0.5, 1, np.uint8), 0.8, invariants=False)


def test_two_hundred_classes():
    lab = ref.noise((5, 9, 200), 200, 0.7, 7, np.uint8)
    _check_against_oracle(lab, 0.8)


@pytest.mark.parametrize("rounds", [1, 3, 128])
@pytest.mark.parametrize("r", [0.3, 0.8, 0.95])
def test_reductions_and_round_limits(r, rounds):
    for lab in (ref.ball(), ref.noise((17, 19, 70), 3, 0.5, 4)):
        plain, got = _check_against_oracle(lab, r, rounds, smooth_iterations=2)
        if rounds == 128 and r == 0.3:
            for c in got:
                assert got[c].faces.shape[0] <= math.ceil(0.7 * plain[c].faces.shape[0])


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
def test_label_dtypes_and_anisotropic_geometry(dtype):
    lab = ref.noise((20, 21, 70), 2, 0.5, 6, dtype)
    lab[4:16, 4:16, 10:60] = 1
    spacing, origin = (0.7, 1.3, 2.9), (-103.5, 40.25, 977.0)
    a, b = math.radians(25.0), math.radians(-40.0)
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    _check_against_oracle(lab, 0.8, spacing=spacing, origin=origin, direction=(rz @ rx).reshape(-1),
                          smooth_iterations=3)


def test_volume_drift_of_ball_and_torus():
    # oracle figures x 1.5
    bounds = {("ball", 0): 0.000989 * 1.5, ("ball", 5): 0.012328 * 1.5, ("torus", 0): 0.006590 * 1.5,
              ("torus", 5): 0.006386 * 1.5}
    for (name, T), bound in bounds.items():
        lab = NAMED[name]()
        v0 = _extract(lab, smooth_iterations=T)[1].volume
        v1 = _extract(lab, smooth_iterations=T, decimate=0.8)[1].volume
        print(f"{name} T={T}: volume drift {abs(v1 - v0) / v0:.6f} (bound {bound:.6f})")
        assert abs(v1 - v0) / v0 <= bound


def test_repeatable_inputs_untouched_and_device_tensors():
    lab = ref.noise((20, 30, 130), 5, 0.6, 10, np.int16)
    lab[3:17, 5:25, 20:110] = 2
    kw = dict(smooth_iterations=3, spacing=(0.9, 1.1, 1.7), decimate=0.8)
    a, b = _extract(lab, **kw), _extract(lab, **kw)
    assert sorted(a) == sorted(b)
    for c in a:
        assert a[c] == b[c] and np.array_equal(_bits(a[c].vertices), _bits(b[c].vertices))
    t = torch.from_numpy(lab).cuda()
    keep = t.clone()
    d = _extract(t, **kw)
    assert torch.equal(t, keep)
    for c in a:
        assert d[c].vertices.is_cuda and d[c].faces.is_cuda
        assert d[c].vertices.dtype == torch.float32 and d[c].faces.dtype == torch.int32
        assert np.array_equal(_bits(d[c].vertices.cpu().numpy()), _bits(a[c].vertices))
        assert np.array_equal(d[c].faces.cpu().numpy(), a[c].faces)
        assert d[c].area == a[c].area and d[c].volume == a[c].volume


def test_default_path_is_unchanged():
    lab = ref.noise((20, 30, 130), 5, 0.6, 10, np.int16)
    a = _extract(lab, smooth_iterations=2)
    b = _extract(lab, smooth_iterations=2, decimate=0.0)
    assert sorted(a) == sorted(b)
    for c in a:
        assert a[c] == b[c] and np.array_equal(_bits(a[c].vertices), _bits(b[c].vertices))


def test_decimate_surface_equals_the_pipeline(tmp_path):
    from segmantic_amd.image.surfaces import decimate_surface, read_ply, write_ply
    lab = ref.torus()
    plain = _extract(lab, smooth_iterations=2, spacing=(0.5, 1.25, 2.0))[1]
    want = _extract(lab, smooth_iterations=2, spacing=(0.5, 1.25, 2.0), decimate=0.8)[1]
    write_ply(tmp_path / "t.ply", plain)
    loaded = read_ply(tmp_path / "t.ply")
    v0, f0 = loaded.vertices.copy(), loaded.faces.copy()
    got = decimate_surface(loaded, 0.8)
    assert isinstance(got.vertices, np.ndarray) and isinstance(got.faces, np.ndarray)
    assert got == want and np.array_equal(_bits(got.vertices), _bits(want.vertices))
    assert np.array_equal(loaded.vertices, v0) and np.array_equal(loaded.faces, f0)
    assert decimate_surface(loaded, 0.0) is loaded
    from segmantic_amd.image.surfaces import Surface
    dev = Surface(torch.from_numpy(loaded.vertices).cuda(), torch.from_numpy(loaded.faces).cuda())
    on_dev = decimate_surface(dev, 0.8, max_rounds=128)
    assert on_dev.vertices.is_cuda and on_dev.faces.is_cuda and on_dev == want
    # a decimated surface survives the PLY round trip
    write_ply(tmp_path / "d.ply", got)
    assert read_ply(tmp_path / "d.ply") == got
    # a tetrahedron is irreducible
    tet = Surface(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32),
                  np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32))
    out = decimate_surface(tet, 0.9)
    assert np.array_equal(out.faces, tet.faces) and np.array_equal(out.vertices, tet.vertices)
    # an open border is pinned: a flat grid keeps its border vertices and every invariant but closedness
    n = 9
    gy, gx = np.mgrid[:n, :n]
    gv = np.stack([gx.ravel(), gy.ravel(), 0 * gx.ravel()], 1).astype(np.float32)
    quads = [(j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i) for j in range(n - 1) for i in range(n - 1)]
    gf = np.asarray([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    out = decimate_surface(Surface(gv, gf), 0.8)
    want = dref.decimate(gv, gf, 0.8)
    assert np.array_equal(out.faces, want["faces"]) and np.array_equal(_bits(out.vertices), _bits(gv[want["kept"]]))
    border = {tuple(p) for p in gv.tolist() if p[0] in (0, n - 1) or p[1] in (0, n - 1)}
    assert border <= {tuple(p) for p in out.vertices.tolist()}
    assert out.faces.shape[0] < gf.shape[0]


def test_script_end_to_end_with_decimation(tmp_path):
    from segmantic_amd.data.imageio import write_image
    from segmantic_amd.image.surfaces import read_ply
    lab = ref.ball()
    write_image(tmp_path / "seg.nii.gz", lab, np.diag([0.8, 1.5, 2.5, 1.0]))
    run = [sys.executable, str(ROOT / "scripts" / "visualize_label_surfaces.py"), str(tmp_path / "seg.nii.gz")]
    out = subprocess.run(run + [str(tmp_path / "plain"), str(tmp_path / "none.txt")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr
    out = subprocess.run(run + [str(tmp_path / "dec"), str(tmp_path / "none.txt"), "--decimate", "0.8"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    plain, dec = read_ply(tmp_path / "plain" / "label_001.ply"), read_ply(tmp_path / "dec" / "label_001.ply")
    assert dec.faces.shape[0] <= math.ceil(0.2 * plain.faces.shape[0])
    _invariants(plain.vertices, plain.faces, dec.vertices, dec.faces)
    assert dec.volume > 0
