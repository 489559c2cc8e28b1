"""Label surfaces without a GPU: the numpy oracle against independent counts and the consequences of the
surface-nets contract, the PLY reader / writer, file naming, and the validation that precedes any device work."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.helpers import surface_ref as ref

ROOT = Path(__file__).resolve().parent.parent


def _border_volume():
    lab = np.zeros((7, 8, 9), np.uint8)
    lab[0], lab[-1], lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1] = 1, 1, 1, 1, 1, 1
    return lab


def _two_diagonal():
    lab = np.zeros((4, 4, 4), np.uint8)
    lab[1, 1, 1] = lab[2, 2, 2] = 1
    return lab


def _single():
    lab = np.zeros((3, 3, 3), np.uint8)
    lab[1, 1, 1] = 1
    return lab


VOLUMES = {
    "ball": (ref.ball, [1]),
    "box": (lambda: np.ones((5, 6, 7), np.uint8), [1]),
    "torus": (ref.torus, [1]),
    "noise": (lambda: ref.noise((9, 10, 11), 3, 0.6, 5), [1, 2, 3]),
    "diagonal": (_two_diagonal, [1]),
    "single": (_single, [1]),
    "border": (_border_volume, [1]),
}


@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_oracle_counts_match_scipy_and_numpy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    make, labels = VOLUMES[name]
    lab = make()
    for c in labels:
        got = ref.surface_nets(lab, c)
        P = np.pad(lab == c, 1).astype(np.int32)
        win = ndi.correlate(P, np.ones((2, 2, 2), np.int32), mode="constant", origin=(-1, -1, -1))
        win = win[:-1, :-1, :-1]                       # one window per cell
        assert got["index"].shape[0] == int(((win >= 1) & (win <= 7)).sum())
        crossing = sum(int(np.abs(np.diff(P, axis=a)).sum()) for a in range(3))
        assert got["faces"].shape[0] == 2 * crossing


@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_oracle_consequences(name):
    make, labels = VOLUMES[name]
    lab = make()
    for c in labels:
        got = ref.surface_nets(lab, c)
        v, f = got["index"], got["faces"]
        assert ref.directed_edge_balance(f)
        area, vol, _, _ = ref.measures(v, f)
        assert vol > 0
        assert abs(vol - float((lab == c).sum())) <= v.shape[0]
        if name in ("ball", "box", "single"):
            assert ref.euler_characteristic(v.shape[0], f) == 2
        if name == "torus":
            assert ref.euler_characteristic(v.shape[0], f) == 0


def test_oracle_non_manifold_edge_is_kept():
    lab = np.zeros((4, 4, 4), np.uint8)
    lab[1, 1, 1] = lab[1, 2, 2] = 1                    # two voxels that share an edge
    f = ref.surface_nets(lab, 1)["faces"]
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert counts.max() == 2 and ref.directed_edge_balance(f)


@pytest.mark.parametrize("iterations", [0, 1, 7])
def test_oracle_vertices_stay_in_their_cells(iterations):
    lab = ref.noise((8, 9, 10), 3, 0.5, 11)
    for c in (1, 2, 3):
        got = ref.surface_nets(lab, c, iterations, 0.7)
        o = got["index"].astype(np.float64) - (got["cells"] - 1)
        assert (o >= 0).all() and (o <= 1).all()
        assert ref.directed_edge_balance(got["faces"])


def test_oracle_normals_point_outwards():
    got = ref.surface_nets(_single(), 1)
    v, f = got["index"].astype(np.float64), got["faces"]
    centre = np.ones(3)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (((v[f].mean(1) - centre) * n).sum(1) > 0).all()
    assert v.shape == (8, 3) and f.shape == (12, 3)


# ------------------------------------------------------------------ PLY and names
def test_ply_bytes_and_round_trip(tmp_path):
    from segmantic_amd.image.surfaces import Surface, ply_header, read_ply, write_ply

    got = ref.surface_nets(ref.ball(12, 4.2), 1)
    area, vol, _, _ = ref.measures(got["index"], got["faces"])
    s = Surface(got["index"].astype(np.float32), got["faces"], area, vol)
    p = tmp_path / "ball.ply"
    write_ply(p, s)
    raw = p.read_bytes()
    nv, nf = s.vertices.shape[0], s.faces.shape[0]
    head = (f"ply\nformat binary_little_endian 1.0\ncomment segmantic_amd label surface\ncomment area {area!r}\n"
            f"comment volume {vol!r}\nelement vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {nf}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    assert raw.startswith(head) and ply_header(s) == head
    assert len(raw) == len(head) + 12 * nv + 13 * nf
    assert raw[len(head):len(head) + 12] == s.vertices[0].astype("<f4").tobytes()
    first_face = raw[len(head) + 12 * nv:len(head) + 12 * nv + 13]
    assert first_face == b"\x03" + s.faces[0].astype("<i4").tobytes()
    back = read_ply(p)
    assert back == s and back.vertices.dtype == np.float32 and back.faces.dtype == np.int32
    # torch tensors are written alike
    write_ply(tmp_path / "t.ply", Surface(torch.from_numpy(s.vertices), torch.from_numpy(s.faces), area, vol))
    assert (tmp_path / "t.ply").read_bytes() == raw
    # an empty mesh
    e = Surface(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    write_ply(tmp_path / "e.ply", e)
    assert read_ply(tmp_path / "e.ply") == e
    with pytest.raises(ValueError):
        (tmp_path / "bad.ply").write_bytes(raw[:-1])
        read_ply(tmp_path / "bad.ply")


def test_file_names():
    from segmantic_amd.image.surfaces import surface_file_name

    assert surface_file_name(3) == "label_003.ply"
    assert surface_file_name(1234, {}) == "label_1234.ply"
    assert surface_file_name(2, {2: "Bone", 3: "Fat"}) == "Bone.ply"
    assert surface_file_name(4, {2: "Bone"}) == "label_004.ply"


# ------------------------------------------------------------------ validation needs no device
def test_value_errors_before_any_device_work():
    from segmantic_amd import image
    from segmantic_amd.image.processing import Image
    from segmantic_amd.image.surfaces import extract_surfaces

    assert image.surfaces.extract_surfaces is extract_surfaces
    with pytest.raises(ValueError, match="3-D"):
        extract_surfaces(np.zeros((5, 6), np.uint8))
    with pytest.raises(ValueError, match="integers"):
        extract_surfaces(np.zeros((4, 5, 6), np.float32))
    with pytest.raises(ValueError, match="integers"):
        extract_surfaces(torch.zeros((4, 5, 6)))
    big = np.zeros((4, 5, 6), np.int32)
    big[1, 2, 3] = 65536
    with pytest.raises(ValueError, match="65535"):
        extract_surfaces(big)
    with pytest.raises(ValueError, match="65535"):
        extract_surfaces(Image(torch.from_numpy(big)))
    # the unsigned wide tensor types are range-checked like any other integer type
    from segmantic_amd.image.surfaces import _value_range
    for dt in (np.uint32, np.uint64, np.int64):
        wide = np.zeros((4, 5, 6), dt)
        wide[1, 2, 3] = 65536
        with pytest.raises(ValueError, match="65535"):
            extract_surfaces(torch.from_numpy(wide))
    u16 = np.zeros((4, 5, 6), np.uint16)
    u16[1, 2, 3] = 65535                               # every uint16 value is a valid label
    assert _value_range(torch.from_numpy(u16)) == (0, 65535)
    assert _value_range(torch.from_numpy(u16.astype(np.int8))) == (-1, 0)
    neg = np.zeros((4, 5, 6), np.int16)
    neg[0, 0, 0] = -1
    with pytest.raises(ValueError, match="65535"):
        extract_surfaces(neg)
    ok = np.zeros((4, 5, 6), np.uint8)
    with pytest.raises(ValueError, match="selected"):
        extract_surfaces(ok, selected=[0, 1])
    with pytest.raises(ValueError, match="smooth_iterations"):
        extract_surfaces(ok, smooth_iterations=-1)
    with pytest.raises(ValueError, match="relaxation"):
        extract_surfaces(ok, relaxation=1.5)
    with pytest.raises(ValueError, match="2\\^31"):
        extract_surfaces(np.broadcast_to(np.zeros((1, 1, 1), np.uint8), (1290, 1290, 1290)))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the error raised without a GPU")
def test_no_gpu_is_a_runtime_error():
    from segmantic_amd.image.surfaces import extract_surfaces

    with pytest.raises(RuntimeError, match="MI355X"):
        extract_surfaces(np.ones((4, 5, 6), np.uint8))


@pytest.mark.parametrize("kind", ["2d", "float", "large"])
def test_script_value_errors(tmp_path, kind):
    from segmantic_amd.data.imageio import write_image

    if kind == "2d":
        arr = np.ones((5, 6), np.uint8)
    else:
        arr = np.zeros((4, 5, 6), np.float32 if kind == "float" else np.int32)
        arr[1, 2, 3] = 0.5 if kind == "float" else 70000
    write_image(tmp_path / "l.nii.gz", arr, np.eye(4))
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "visualize_label_surfaces.py"),
                          str(tmp_path / "l.nii.gz"), str(tmp_path / "out"), str(tmp_path / "none.txt")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "ValueError" in out.stderr and {"2d": "3-D", "float": "integers", "large": "65535"}[kind] in out.stderr
    assert not list((tmp_path / "out").glob("*.ply")) if (tmp_path / "out").exists() else True


def test_script_help():
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "visualize_label_surfaces.py"), "--help"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    for word in ("file_path", "output_dir", "tissuelist_path", "--selected-tissues", "--smooth", "--relaxation"):
        assert word in out.stdout.lower()
