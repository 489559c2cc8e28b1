"""Label clean-up (seg/transforms.py, csrc/components.hip) on the MI355X against the numpy oracle of
tests/helpers/components_ref.py.  Integer arithmetic with one canonical answer: every comparison is exact."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.helpers import components_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NP_DTYPES = {"uint8": np.uint8, "int16": np.int16, "int32": np.int32}
# none is a multiple of the 64 x 8 x 8 tile; 5x9x200 and 1x37x70 cross x seams, 33x47x65 all three kinds
SHAPES = [(1, 1, 1), (1, 37, 70), (33, 47, 65), (48, 48, 48), (5, 9, 200), (37, 70), (1, 130), (9, 1, 1)]


def T():
    from segmantic_amd.seg import transforms
    return transforms


def _random(rng, shape, classes, density, dtype=np.uint8):
    return (rng.integers(1, classes + 1, shape) * (rng.random(shape) < density)).astype(dtype)


def _check_cc(lab, connectivity=None, background=0):
    want, n_want = ref.connected_components(lab, connectivity, background)
    before = lab.copy()
    got, n = T().connected_components(lab, connectivity, background)
    assert n == n_want
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(lab, before)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_connected_components_shapes_and_connectivities(shape):
    rng = np.random.default_rng(sum(shape))
    for c in range(1, len(shape) + 1):
        _check_cc(_random(rng, shape, 1, 0.5), c)
        _check_cc(_random(rng, shape, 4, 0.7), c)
    _check_cc(_random(rng, shape, 3, 0.6), None)
    _check_cc(_random(rng, shape, 2, 0.6), None, background=None)


@pytest.mark.parametrize("dtype", sorted(NP_DTYPES))
@pytest.mark.parametrize("classes", [4, 200])
def test_connected_components_dtypes_classes_densities(dtype, classes):
    if dtype == "uint8" and classes > 255:
        pytest.skip("not representable")
    rng = np.random.default_rng(classes)
    for density in (0.1, 0.4, 0.8, 1.0):
        lab = _random(rng, (19, 30, 77), classes, density, NP_DTYPES[dtype])
        for c in (1, 2, 3):
            _check_cc(lab, c)
    if dtype != "uint8":
        # values are only compared: negative and large ones are components like any other
        lab = _random(rng, (6, 11, 70), 3, 0.7, NP_DTYPES[dtype])
        lab = np.where(lab == 2, -5, np.where(lab == 3, np.iinfo(NP_DTYPES[dtype]).max, lab)).astype(NP_DTYPES[dtype])
        _check_cc(lab, 2)


def test_empty_and_full_volumes():
    for shape in ((20, 21, 70), (30, 70)):
        empty = np.zeros(shape, np.uint8)
        comp, n = T().connected_components(empty)
        assert n == 0 and not comp.any()
        comp, n = T().connected_components(empty, background=None)
        assert n == 1 and (comp == 1).all()
        for c in range(1, len(shape) + 1):
            comp, n = T().connected_components(np.full(shape, 7, np.int16), c)
            assert n == 1 and (comp == 1).all()
        assert T().component_sizes(np.full(shape, 7, np.int16)).tolist() == [int(np.prod(shape))]
        assert T().component_sizes(empty).tolist() == []


def test_checkerboard():
    z, y, x = np.indices((18, 20, 70))
    board = ((z + y + x) % 2).astype(np.uint8)
    comp, n = T().connected_components(board, 1)      # every voxel a component: numbered in raster order
    assert n == int(board.sum())
    want = np.zeros(board.size, np.int32)
    want[board.ravel() != 0] = np.arange(1, n + 1)
    assert np.array_equal(comp.ravel(), want)
    # at full connectivity the set voxels form one component spanning every seam
    comp, n = T().connected_components(board, 3)
    assert n == 1 and np.array_equal(comp, board.astype(np.int32))
    _check_cc(board, 2)
    _check_cc(board, 3, background=None)


def test_serpentine_paths_through_every_seam():
    # a one-voxel-wide snake: every other row of every other plane, joined at alternating ends, so the path
    # crosses every tile seam many times (long parent chains before the flatten pass)
    d, h, w = 11, 13, 133
    base = np.zeros((d, h, w), np.uint8)
    for z in range(0, d, 2):
        for yi, y in enumerate(range(0, h, 2)):
            base[z, y, :] = 1
            if y + 2 < h:
                base[z, y + 1, w - 1 if yi % 2 == 0 else 0] = 1
        if z + 2 < d:
            base[z + 1, h - 1 if (z // 2) % 2 == 0 else 0, w - 1 if (z // 2) % 2 == 0 else 0] = 1
    # three orientations: the long runs lie along x, then along y, then along z
    for lab in (base, np.ascontiguousarray(base.transpose(2, 0, 1)), np.ascontiguousarray(base.transpose(1, 2, 0))):
        for c in (1, 2, 3):
            comp, n = T().connected_components(lab, c)
            assert n == 1 and np.array_equal(comp, lab.astype(np.int32))       # one component
    _check_cc(base, 1)
    _check_cc(base, 1, background=None)


def test_diagonal_line_and_interleaved_planes():
    n = 70
    line = np.zeros((n, n, n), np.uint8)
    i = np.arange(n)
    line[i, i, i] = 3
    for c, want in ((1, n), (2, n), (3, 1)):
        comp, count = T().connected_components(line, c)
        assert count == want
        assert np.array_equal(comp[i, i, i], np.arange(1, n + 1) if want == n else np.ones(n))
        assert int((comp != 0).sum()) == n
    sheet = np.zeros((n, n), np.int16)
    sheet[i, n - 1 - i] = 9
    assert T().connected_components(sheet, 1)[1] == n and T().connected_components(sheet, 2)[1] == 1
    planes = np.zeros((20, 19, 67), np.uint8)
    planes[0::2] = 1
    planes[1::2] = 2
    for c in (1, 3):
        comp, count = T().connected_components(planes, c)
        assert count == 20
        assert np.array_equal(comp, np.broadcast_to(np.arange(1, 21, dtype=np.int32)[:, None, None], planes.shape))
    for axis_planes in (np.ascontiguousarray(planes.transpose(1, 0, 2)), np.ascontiguousarray(planes.transpose(2, 1, 0))):
        _check_cc(axis_planes, 3)


def test_large_volume_from_known_pieces():
    n = 256
    lab = np.zeros((n, n, n), np.uint8)
    ids = np.zeros((n, n, n), np.int32)
    pieces = []                                   # (first voxel, size)
    zz, yy, xx = np.ogrid[:n, :n, :n]

    def add(mask_slices, mask, value):
        view = lab[mask_slices]
        assert not view[mask].any()
        view[mask] = value
        ids[mask_slices][mask] = len(pieces) + 1
        full = np.zeros((n, n, n), bool)
        full[mask_slices][mask] = True
        pieces.append((int(np.flatnonzero(full.ravel())[0]), int(mask.sum())))

    # boxes across tile seams (tiles are 64 x 8 x 8) and spheres, at least 2 voxels apart
    for k, (z0, y0, x0, dz, dy, dx) in enumerate([(3, 5, 10, 20, 30, 100), (60, 60, 60, 10, 10, 10),
                                                  (100, 3, 120, 9, 17, 130), (200, 200, 1, 50, 50, 254),
                                                  (130, 100, 7, 1, 1, 240), (140, 7, 63, 30, 1, 2)]):
        sl = (slice(z0, z0 + dz), slice(y0, y0 + dy), slice(x0, x0 + dx))
        add(sl, np.ones((dz, dy, dx), bool), 1 + k % 3)
    for k, (cz, cy, cx, r) in enumerate([(64, 128, 64, 30), (180, 64, 192, 40), (128, 200, 128, 17), (30, 200, 220, 9)]):
        sl = (slice(cz - r, cz + r + 1), slice(cy - r, cy + r + 1), slice(cx - r, cx + r + 1))
        ball = ((zz[sl[0]] - cz) ** 2 + (yy[:, sl[1]] - cy) ** 2 + (xx[:, :, sl[2]] - cx) ** 2) <= r * r
        add(sl, ball, 4)
    # single-voxel specks on a lattice of spacing 3 in a free slab
    assert not lab[232:250, 0:190, :].any() and not lab[230:252, 0:192, :].any()
    speck = np.zeros((n, n, n), bool)
    speck[233:249:3, 2:188:3, 1:255:3] = True
    n_specks = int(speck.sum())
    lab[speck] = 5

    comp, count = T().connected_components(lab, 3)
    assert count == len(pieces) + n_specks
    sizes = T().component_sizes(lab, 3)
    assert sorted(sizes.tolist()) == sorted([s for _, s in pieces] + [1] * n_specks)
    # canonical order: by first voxel
    firsts = sorted([f for f, _ in pieces] + np.flatnonzero(speck.ravel()).tolist())
    rank = {f: i + 1 for i, f in enumerate(firsts)}
    flat = comp.ravel()
    for k, (f, s) in enumerate(pieces):
        assert flat[f] == rank[f]
        assert int(sizes[rank[f] - 1]) == s
        assert np.array_equal(comp == rank[f], ids == k + 1)
    speck_idx = np.flatnonzero(speck.ravel())
    assert np.array_equal(flat[speck_idx], np.array([rank[f] for f in speck_idx.tolist()], np.int32))
    assert not comp[lab == 0].any()
    # the same through the clean-up transforms
    out = T().remove_small_objects(lab, 2, 3)
    assert np.array_equal(out, np.where(speck, 0, lab))
    kept = T().keep_largest_connected_component(lab, connectivity=3)
    by_class = {}
    for k, (f, s) in enumerate(pieces):
        by_class.setdefault(int(lab.ravel()[f]), []).append((-s, f, k + 1))
    want = np.zeros_like(lab)
    for cls, items in by_class.items():
        want[ids == sorted(items)[0][2]] = cls
    want.ravel()[speck_idx[0]] = 5
    assert np.array_equal(kept, want)


# ------------------------------------------------------------------ the transforms against the oracle
def _islands(rng, shape, classes, dtype=np.uint8):
    """blobby multi-class volume with small islands and cavities"""
    lab = _random(rng, shape, classes, 0.55, dtype)
    lab[rng.random(shape) < 0.2] = 0
    return lab


@pytest.mark.parametrize("dtype", sorted(NP_DTYPES))
def test_keep_largest(dtype):
    rng = np.random.default_rng(11)
    for shape in ((9, 14, 70), (23, 70)):
        lab = _islands(rng, shape, 3, NP_DTYPES[dtype])
        before = lab.copy()
        for c in range(1, len(shape) + 1):
            for k in (1, 2, 3):
                got = T().keep_largest_connected_component(lab, num_components=k, connectivity=c)
                assert got.dtype == lab.dtype
                assert np.array_equal(got, ref.keep_largest_connected_component(lab, None, True, c, k))
            got = T().keep_largest_connected_component(lab, applied_labels=[1, 3], connectivity=c)
            assert np.array_equal(got, ref.keep_largest_connected_component(lab, [1, 3], True, c))
            got = T().keep_largest_connected_component(lab, independent=False, connectivity=c, num_components=2)
            assert np.array_equal(got, ref.keep_largest_connected_component(lab, None, False, c, 2))
            got = T().keep_largest_connected_component(lab, [2, 3], False, c)
            assert np.array_equal(got, ref.keep_largest_connected_component(lab, [2, 3], False, c))
        assert np.array_equal(lab, before)


def test_keep_largest_ties_and_ranges():
    lab = np.zeros((3, 9, 140), np.int32)
    lab[0, 0, 0:5] = 7
    lab[1, 4, 60:65] = 7          # same size, later first voxel, across an x seam
    lab[2, 8, 130:135] = 7
    lab[2, 0, 0:4] = 65535
    got = T().keep_largest_connected_component(lab)
    want = np.zeros_like(lab)
    want[0, 0, 0:5] = 7
    want[2, 0, 0:4] = 65535
    assert np.array_equal(got, want)
    got = T().keep_largest_connected_component(lab, num_components=2)
    want[1, 4, 60:65] = 7
    assert np.array_equal(got, want)
    assert np.array_equal(T().keep_largest_connected_component(lab, num_components=3), lab)
    assert np.array_equal(T().keep_largest_connected_component(lab, applied_labels=[0]), lab)
    for bad in (65536, -1):
        broken = lab.copy()
        broken[1, 1, 1] = bad
        for fn in (T().keep_largest_connected_component, T().remove_small_objects, T().fill_holes):
            with pytest.raises(ValueError, match="65535"):
                fn(broken)
    wide = torch.from_numpy(lab).to(torch.int64)
    out = T().keep_largest_connected_component(wide)
    assert out.dtype == torch.int64 and out.device == wide.device
    assert np.array_equal(out.numpy(), T().keep_largest_connected_component(lab))


@pytest.mark.parametrize("dtype", sorted(NP_DTYPES))
def test_remove_small_objects(dtype):
    rng = np.random.default_rng(12)
    for shape in ((9, 14, 70), (23, 70)):
        lab = _islands(rng, shape, 3, NP_DTYPES[dtype])
        before = lab.copy()
        sizes = ref.component_sizes(lab, 1)
        threshold = int(np.sort(sizes)[len(sizes) // 2])     # an exact threshold: components of this size stay
        for c in range(1, len(shape) + 1):
            for m in (0, 1, 2, threshold, threshold + 1, 10 ** 9):
                got = T().remove_small_objects(lab, m, c)
                assert got.dtype == lab.dtype
                assert np.array_equal(got, ref.remove_small_objects(lab, m, c))
        assert np.array_equal(T().remove_small_objects(lab, 0), lab) and np.array_equal(T().remove_small_objects(lab, 1), lab)
        assert np.array_equal(T().remove_small_objects(lab), ref.remove_small_objects(lab, 64, 1))
        assert np.array_equal(lab, before)
        assert np.array_equal(T().component_sizes(lab, 1), sizes)


def _nested(n=21):
    """shell of 1, cavity, shell of 2 inside it, cavity inside that"""
    lab = np.zeros((n, n, 70), np.uint8)
    lab[1:-1, 1:-1, 1:-1] = 1
    lab[3:-3, 3:-3, 3:-3] = 0
    lab[5:-5, 5:-5, 5:-5] = 2
    lab[7:-7, 7:-7, 7:-7] = 0
    return lab


@pytest.mark.parametrize("dtype", sorted(NP_DTYPES))
def test_fill_holes(dtype):
    rng = np.random.default_rng(13)
    dt = NP_DTYPES[dtype]
    nested = _nested().astype(dt)
    two = np.zeros((9, 9, 70), dt)
    two[1:-1, 1:-1, 1:-1] = 1
    two[3:-3, 3:-3, 3:-3] = 0
    two[2, 4, 30] = 2
    corner = np.ones((6, 7, 66), dt)
    corner[1, 1, 1] = 0
    corner[0, 0, 0] = 0               # joins the cavity through a corner only
    corner[3, 3, 60:65] = 0           # a closed cavity across the x seam
    corner[4, 5, 65] = 0              # on the border
    cases = [nested, two, corner, _islands(rng, (9, 14, 70), 2, dt), (rng.random((8, 13, 66)) < 0.8).astype(dt),
             (rng.random((31, 70)) < 0.75).astype(dt) * 3, _islands(rng, (23, 70), 3, dt)]
    for lab in cases:
        before = lab.copy()
        for c in range(1, lab.ndim + 1):
            got = T().fill_holes(lab, connectivity=c)
            assert got.dtype == lab.dtype
            assert np.array_equal(got, ref.fill_holes(lab, None, c))
            assert np.array_equal(T().fill_holes(lab, [2], c), ref.fill_holes(lab, [2], c))
        assert np.array_equal(T().fill_holes(lab), ref.fill_holes(lab))
        assert np.array_equal(lab, before)
    # the statements of the definition, spelled out
    filled = T().fill_holes(nested)
    # the inner cavity is enclosed by 2 alone; the outer one lies between the 1-shell and the 2-shell: two classes
    assert filled[10, 10, 30] == 2 and filled[4, 4, 4] == 0
    assert (filled != 0).sum() == (nested != 0).sum() + 7 * 7 * 56
    assert np.array_equal(T().fill_holes(two), two)
    assert T().fill_holes(corner, connectivity=3)[1, 1, 1] == 0 and T().fill_holes(corner, connectivity=1)[1, 1, 1] == 1
    assert T().fill_holes(corner)[3, 3, 62] == 1 and T().fill_holes(corner)[4, 5, 65] == 0


TORCH_MAP = {"uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32, "int64": torch.int64}


@pytest.mark.parametrize("in_dtype", sorted(TORCH_MAP))
@pytest.mark.parametrize("out_dtype", sorted(TORCH_MAP))
def test_map_labels_dtype_pairs(in_dtype, out_dtype):
    rng = np.random.default_rng(14)
    mapping = {int(k): int(v) for k, v in zip(rng.permutation(120)[:90], rng.integers(0, 127, 90))}
    size = max(mapping) + 1
    img = torch.from_numpy(rng.integers(0, size, (3, 1, 17, 9, 5))).to(TORCH_MAP[in_dtype])
    before = img.clone()
    tf = T().MapLabels(mapping, out_dtype=TORCH_MAP[out_dtype])
    out = tf(img)
    assert out.dtype == TORCH_MAP[out_dtype] and out.shape == img.shape and out.device == img.device
    assert np.array_equal(out.numpy(), ref.map_labels(mapping, img.numpy(), out.numpy().dtype))
    assert torch.equal(img, before)
    assert torch.equal(tf(img.cuda()).cpu(), out) and tf(img.cuda()).is_cuda
    assert np.array_equal(tf(img.numpy()), out.numpy())


def test_map_labels_reference_answer_and_index_errors():
    tf = T().MapLabels({1: 3, 2: 1, 0: 0})
    img = torch.tensor([2, 1, 2, 0]).reshape(1, 4, 1, 1)
    out = tf(img)
    assert out.dtype == torch.int64 and out.shape == (1, 4, 1, 1) and out.reshape(-1).tolist() == [1, 3, 1, 0]
    out = T().MapLabelsd({1: 3, 2: 1, 0: 0}, keys=["label"])({"label": img, "image": 5})
    assert out["image"] == 5 and out["label"].reshape(-1).tolist() == [1, 3, 1, 0]
    # out of the table: caught on the host, as the reference's lookup[img] raises
    for bad, dt in ((3, torch.uint8), (3, torch.int32), (-1, torch.int16), (2 ** 40, torch.int64)):
        with pytest.raises(IndexError):
            tf(torch.tensor([0, 1, bad], dtype=dt))
    big = T().MapLabels({255: 9, 1: 2})
    assert big(np.array([[255, 1, 7]], np.uint8)).tolist() == [[9, 2, 0]]


def test_repeatable_streams_inputs_and_containers():
    rng = np.random.default_rng(15)
    lab_np = _islands(rng, (21, 30, 130), 3)
    lab = torch.from_numpy(lab_np).cuda()
    before = lab.clone()
    calls = {
        "cc": lambda x: T().connected_components(x, 2)[0],
        "cc_bg": lambda x: T().connected_components(x, 1, None)[0],
        "sizes": lambda x: T().component_sizes(x, 3),
        "keep": lambda x: T().keep_largest_connected_component(x, num_components=2),
        "small": lambda x: T().remove_small_objects(x, 5),
        "fill": lambda x: T().fill_holes(x),
        "map": lambda x: T().MapLabels({1: 2, 2: 3, 3: 1})(x),
    }
    side = torch.cuda.Stream()
    for name, fn in calls.items():
        a = fn(lab)
        b = fn(lab)
        assert a.is_cuda and torch.equal(a, b), name
        assert torch.equal(lab, before), name
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = fn(lab)
        side.synchronize()
        assert torch.equal(a, c), name
        # numpy in -> numpy out, cpu tensor in -> cpu tensor out, same values
        from_np = fn(lab_np)
        assert isinstance(from_np, np.ndarray) and np.array_equal(from_np, a.cpu().numpy()), name
        from_cpu = fn(torch.from_numpy(lab_np))
        assert not from_cpu.is_cuda and torch.equal(from_cpu, a.cpu()), name


def test_dictionary_transforms_channel_first_and_images():
    from segmantic_amd.image.processing import Image

    rng = np.random.default_rng(16)
    lab = _islands(rng, (9, 14, 70), 3)
    data = {"pred": torch.from_numpy(lab)[None], "image": "untouched"}
    out = T().KeepLargestConnectedComponentd(keys="pred", num_components=2, connectivity=1)(data)
    assert out["image"] == "untouched" and out["pred"].shape == (1, 9, 14, 70)
    assert np.array_equal(out["pred"][0].numpy(), ref.keep_largest_connected_component(lab, None, True, 1, 2))
    assert torch.equal(data["pred"], torch.from_numpy(lab)[None])
    out = T().RemoveSmallObjectsd(keys=["pred"], min_size=4)(data)
    assert np.array_equal(out["pred"][0].numpy(), ref.remove_small_objects(lab, 4, 1))
    out = T().FillHolesd(keys=["pred", "other"], allow_missing_keys=True)(data)
    assert np.array_equal(out["pred"][0].numpy(), ref.fill_holes(lab))
    with pytest.raises(KeyError):
        T().FillHolesd(keys=["pred", "other"])(data)
    # [1, h, w] is channel-first 2-D
    flat = lab[3]
    out = T().FillHoles(connectivity=1)(flat[None])
    assert out.shape == (1, 14, 70) and np.array_equal(out[0], ref.fill_holes(flat, None, 1))
    assert np.array_equal(T().RemoveSmallObjects(3)(flat), ref.remove_small_objects(flat, 3, 1))
    assert np.array_equal(T().KeepLargestConnectedComponent([1, 2])(lab),
                          ref.keep_largest_connected_component(lab, [1, 2]))
    # Image in -> Image out with the geometry copied
    img = Image(lab, spacing=(0.5, 0.7, 2.0), origin=(1.0, -2.0, 3.0),
                direction=(0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0))
    for res, want in ((T().fill_holes(img), ref.fill_holes(lab)),
                      (T().KeepLargestConnectedComponent()(img), ref.keep_largest_connected_component(lab)),
                      (T().connected_components(img)[0], ref.connected_components(lab)[0]),
                      (T().MapLabels({1: 4, 3: 1}, out_dtype=torch.uint8)(img), ref.map_labels({1: 4, 3: 1}, lab, np.uint8))):
        assert isinstance(res, Image)
        assert res.spacing == img.spacing and res.origin == img.origin and res.direction == img.direction
        assert np.array_equal(res.numpy(), want)
    assert np.array_equal(img.numpy(), lab)


def test_scripts_end_to_end(tmp_path):
    from segmantic_amd.data.imageio import read_image, write_image
    from segmantic_amd.image.labels import load_tissue_list, save_tissue_list

    rng = np.random.default_rng(17)
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    affine = np.diag([0.5, 0.75, 2.0, 1.0])
    affine[:3, 3] = (3.0, -4.0, 5.0)
    volumes = {"a.nii.gz": _islands(rng, (9, 14, 70), 3), "b.nii.gz": _islands(rng, (11, 9, 66), 3)}
    for name, lab in volumes.items():
        write_image(in_dir / name, lab, affine)

    script = str(ROOT / "scripts" / "postprocess_labels.py")
    r = subprocess.run([sys.executable, script, str(in_dir), str(tmp_path / "clean"), "--min-size", "3",
                        "--keep-largest", "2", "--fill-holes", "--connectivity", "1", "--labels", "1,2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for name, lab in volumes.items():
        want = ref.remove_small_objects(lab, 3, 1)
        want = ref.keep_largest_connected_component(want, [1, 2], True, 1, 2)
        want = ref.fill_holes(want, [1, 2], 1)
        got, got_affine = read_image(tmp_path / "clean" / name)
        assert got.dtype == lab.dtype and np.array_equal(got, want)
        assert np.allclose(got_affine, affine)
    r = subprocess.run([sys.executable, script, str(in_dir), str(tmp_path / "largest"), "--keep-largest"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got, _ = read_image(tmp_path / "largest" / "a.nii.gz")
    assert np.array_equal(got, ref.keep_largest_connected_component(volumes["a.nii.gz"]))

    tissues = tmp_path / "tissues.txt"
    save_tissue_list({"Background": 0, "Skull": 1, "Fat": 2, "Mandible": 3}, tissues)
    mapping = tmp_path / "map.json"
    mapping.write_text(json.dumps({"Background": "Background", "Skull": "Bone", "Mandible": "Bone", "Fat": "Fat"}))
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "map_labels.py"), str(in_dir), str(tmp_path / "mapped"),
                        str(tissues), str(mapping)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert load_tissue_list(tmp_path / "mapped" / "labels.txt") == {"Background": 0, "Bone": 1, "Fat": 2}
    for name, lab in volumes.items():
        got, got_affine = read_image(tmp_path / "mapped" / name)
        assert got.dtype == lab.dtype and np.array_equal(got, np.array([0, 1, 2, 1], lab.dtype)[lab])
        assert np.allclose(got_affine, affine)
