"""The label-volume kernels past the scan levels, grid caps and table chunks of csrc/labelvol.h, on the MI355X.
Inputs and the proof that each crosses its limit: tests/helpers/labelvol_limits.py and
tests/test_labelvol_limits_host.py.  Every comparison is exact (integers or float32 bit patterns) against the numpy
oracles; the one bound, on the float64 measures, is the derived one of test_surfaces_gpu.py::test_measures."""
import numpy as np
import pytest
import torch

from tests.helpers import components_ref as cref
from tests.helpers import labelvol_limits as lim
from tests.helpers import surface_ref as sref

pytestmark = pytest.mark.gpu


def _ops():
    from segmantic_amd import ops
    return ops


def _extract(*a, **k):
    from segmantic_amd.image.surfaces import extract_surfaces
    return extract_surfaces(*a, **k)


def T():
    from segmantic_amd.seg import transforms
    return transforms


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_mesh(s, want, what):
    assert s.faces.dtype == np.int32 and s.vertices.dtype == np.float32
    assert s.faces.shape == want["faces"].shape and s.vertices.shape == want["index"].shape, what
    assert np.array_equal(s.faces, want["faces"]), what
    assert np.array_equal(_bits(s.vertices), _bits(want["index"])), what


# ------------------------------------------------------------------ 1: lv_scan_partials_kernel<1> at nb = 1024, 1025, 2050
@pytest.mark.parametrize("n", lim.CC_SIZES)
def test_component_numbering_at_the_scan_boundaries(n):
    root, comp, n_comp, _ = lim.cc_roots(n)
    r = torch.from_numpy(root.copy()).cuda()
    before = r.clone()
    got, count = _ops().cc_compact(r)
    assert int(count.item()) == n_comp
    assert got.dtype == torch.int32 and got.shape == (1, n)
    assert np.array_equal(got.cpu().numpy(), comp)
    assert torch.equal(r, before)


# ------------------------------------------------------------------ 2: lv_scan_partials_kernel<2> with per = 3
@pytest.fixture(scope="module")
def surf_counts():
    return lim.surface_counts(lim.surf_volume(), lim.SURF_CLASSES)


def _check_surf(got, surf_counts, sampled):
    verts, faces = surf_counts
    assert sorted(got) == list(range(1, lim.SURF_CLASSES + 1))
    for c, s in got.items():
        assert (s.vertices.shape[0], s.faces.shape[0]) == (int(verts[c]), int(faces[c])), c
    for c in sampled:
        _same_mesh(got[c], lim.surf_oracle(c), c)


def test_surface_nets_with_three_scan_blocks_per_thread(surf_counts):
    lab = lim.surf_volume().copy()                     # the cached volume is read-only
    spacing = (0.5, 1.25, 2.0)
    got = _extract(lab)
    _check_surf(got, surf_counts, lim.SURF_SAMPLED)
    # the overflow word of the scan, and the starts it leaves, straight from the count
    ops = _ops()
    t = torch.from_numpy(lab).cuda()
    labels = list(range(1, lim.SURF_CLASSES + 1))
    boxes = ops.surface_boxes(t, labels).cpu().numpy()
    assert np.array_equal(boxes, lim.label_boxes(lab, labels))
    ws = torch.empty(ops.surface_workspace_bytes(t.shape, labels, boxes), dtype=torch.uint8, device=t.device)
    starts = ops.surface_count(t, labels, boxes, ws).cpu().numpy()
    verts, faces = surf_counts
    assert starts[-1].tolist() == [0, 0]
    assert np.array_equal(starts[:-1, 0], np.concatenate([[0], np.cumsum(verts[1:])]))
    assert np.array_equal(starts[:-1, 1], np.concatenate([[0], np.cumsum(faces[1:])]))
    # area and volume of the sampled labels, in physical units
    phys = _extract(lab, selected=lim.SURF_SAMPLED, spacing=spacing)
    voxel = spacing[0] * spacing[1] * spacing[2]
    for c in lim.SURF_SAMPLED:
        s = phys[c]
        assert np.array_equal(s.faces, got[c].faces)
        area, vol, abs_area, abs_vol = sref.measures(s.vertices, s.faces)
        f = s.faces.shape[0]
        print(f"label {c}: area {s.area!r} vs {area!r}, volume {s.volume!r} vs {vol!r}")
        assert abs(s.area - area) <= f * 2.0 ** -52 * abs_area
        assert abs(s.volume - vol) <= f * 2.0 ** -52 * abs_vol
        assert abs(s.volume - float((lab == c).sum()) * voxel) <= s.vertices.shape[0] * voxel


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_surface_nets_past_the_scan_in_wider_label_storage(dtype, surf_counts):
    _check_surf(_extract(lim.surf_volume().astype(dtype)), surf_counts, lim.SURF_SAMPLED)


# ------------------------------------------------------------------ 3: the overflow word
def test_two_to_the_31_faces_are_refused():
    n = lim.OVERFLOW_SIDE
    ops = _ops()
    dev = torch.device("cuda")
    i = (torch.arange(n, device=dev) & 1).to(torch.uint8)          # uint8 from here on: the volume is 0.36 GB
    board = (i[:, None, None] ^ i[None, :, None] ^ i[None, None, :]) & 1
    assert board.dtype == torch.uint8 and board.shape == (n, n, n) and board.is_contiguous()
    small = lim.checkerboard(6)
    assert np.array_equal(board[:6, :6, :6].cpu().numpy(), small) and int(board[-1, -1, -1]) == 1
    try:
        boxes = ops.surface_boxes(board, [1]).cpu().numpy()
        assert boxes.tolist() == [[0, n, 0, n, 0, n]]
        ws = torch.empty(ops.surface_workspace_bytes(board.shape, [1], boxes), dtype=torch.uint8, device=dev)
        starts = ops.surface_count(board, [1], boxes, ws).cpu().numpy()
        # the flag, and all totals 0 (labelvol.h: lv_scan_partials_kernel)
        assert starts[2].tolist() == [1, 0] and starts[1].tolist() == [0, 0] and starts[0].tolist() == [0, 0]
        del ws
        with pytest.raises(ValueError, match=r"2\^31"):
            _extract(board, selected=[1])
    finally:
        del board
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 4: dec_scan past one block per thread, > 254 meshes
def test_decimation_batch_past_the_scan_and_one_workgroup_of_meshes():
    ops = _ops()
    distinct = lim.dec_distinct()
    k, n = len(distinct), lim.DEC_MESHES
    cycles = n // k
    starts = lim.dec_batch_starts([(len(v), len(f)) for _, v, f, _ in distinct])
    v = torch.from_numpy(np.tile(np.concatenate([m[1] for m in distinct]), (cycles, 1))).cuda()
    f = torch.from_numpy(np.tile(np.concatenate([m[2] for m in distinct]), (cycles, 1))).cuda()
    v0, f0 = v.clone(), f.clone()
    stats = {}
    ov, of, kept, out_starts, out_host = ops.decimate_meshes(v, f, torch.from_numpy(starts).cuda(), starts,
                                                             lim.DEC_REDUCTION, 128, stats)
    assert torch.equal(v, v0) and torch.equal(f, f0)
    want_starts = lim.dec_batch_starts([(len(m[3]["kept"]), len(m[3]["faces"])) for m in distinct])
    assert np.array_equal(out_starts.cpu().numpy(), out_host)
    assert np.array_equal(out_host, want_starts)
    # every copy equals the oracle's mesh: meshes of a batch are independent
    want_kept = np.tile(np.concatenate([m[3]["kept"] for m in distinct]).astype(np.int32), cycles)
    want_faces = np.tile(np.concatenate([m[3]["faces"] for m in distinct]).astype(np.int32), (cycles, 1))
    want_verts = np.tile(np.concatenate([m[1][m[3]["kept"]] for m in distinct]), (cycles, 1))
    assert np.array_equal(kept.cpu().numpy(), want_kept)
    assert np.array_equal(of.cpu().numpy(), want_faces)
    assert np.array_equal(_bits(ov.cpu().numpy()), _bits(want_verts))
    rounds = max(len(m[3]["history"]) for m in distinct)
    assert stats["rounds"] == rounds and stats["d2h_copies"] == rounds + 1


# ------------------------------------------------------------------ 5: the stride loop of surf_boxes_kernel
@pytest.mark.parametrize("dtype", sorted(lim.BOX_VALUES))
@pytest.mark.parametrize("shape", lim.BOX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_surface_boxes_beyond_one_grid_pass(shape, dtype):
    lab, selected = lim.box_volume(shape, dtype)
    lab = lab.copy()
    t = torch.from_numpy(lab).cuda()
    got = _ops().surface_boxes(t, selected)
    assert got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), lim.label_boxes(lab, selected))
    if shape == lim.BOX_SHAPES[0]:
        present = sorted(set(np.unique(lab).tolist()) - {0})
        out = _extract(lab)
        assert sorted(out) == present and len(present) == 4
        for c in present:
            _same_mesh(out[c], sref.surface_nets(lab, c), c)
        out = _extract(lab, selected=selected)
        absent = lim.BOX_VALUES[dtype][4]
        assert out[absent].vertices.shape == (0, 3) and out[absent].faces.shape == (0, 3)
        for c in selected:
            if c != absent:
                _same_mesh(out[c], sref.surface_nets(lab, c), c)


# ------------------------------------------------------------------ 6: the stride loop of map_labels_kernel
@pytest.mark.parametrize("in_dtype, out_dtype", [("uint8", "uint8"), ("int32", "int64")])
def test_map_labels_beyond_the_grid_cap(in_dtype, out_dtype):
    x, table, want = lim.map_case(in_dtype, out_dtype)
    t = torch.from_numpy(x.copy()).cuda().view(2, 4, -1)      # a flat tensor viewed 3-D
    assert t.numel() == lim.MAP_N and t.is_contiguous()
    lut = torch.from_numpy(table.copy()).cuda()
    out = torch.full(t.shape, lim.MAP_FILL[out_dtype], dtype=getattr(torch, out_dtype), device=t.device)
    before = t.clone()
    got = _ops().map_labels(t, lut, out=out)
    assert got is out and torch.equal(t, before)
    host = got.cpu().numpy().reshape(-1)
    assert host.dtype == want.dtype and np.array_equal(host, want)
    # stated on its own: the tail is neither unwritten nor a copy of the elements one grid pass earlier
    tail = host[lim.MAP_STRIDE:]
    assert (tail != host[:tail.size]).any() and np.array_equal(tail, want[lim.MAP_STRIDE:])
    # the allocating form, through the transform
    if in_dtype == "uint8":
        tf = T().MapLabels(dict(enumerate(table.tolist())), out_dtype=torch.uint8)
        assert np.array_equal(tf(t).cpu().numpy().reshape(-1), want)


# ------------------------------------------------------------------ 7: table upload chunks
@pytest.fixture(scope="module")
def table_device():
    ops = _ops()
    t = torch.from_numpy(lim.table_volume().copy()).cuda()
    root = ops.cc_label(t, 3)
    return t, root, ops.cc_sizes(root), ops.cc_label(t, 3, with_background=True)


@pytest.mark.parametrize("count", lim.APPLIED_COUNTS)
def test_applied_label_tables_of_one_two_and_three_chunks(count, table_device):
    ops = _ops()
    lab = lim.table_volume().copy()
    applied = list(lim.applied_labels(count))
    t, root, size, root_bg = table_device
    # the kernels, with the list in its shuffled order
    want = cref.keep_largest_connected_component(lab, applied, True)
    assert np.array_equal(ops.cc_keep_largest(t, root, size, applied, True, 1).cpu().numpy(), want)
    want_fill = cref.fill_holes(lab, applied)
    assert np.array_equal(ops.cc_fill_holes(t, root_bg, applied, 3).cpu().numpy(), want_fill)
    # the transforms, both ways of taking the applied classes
    got = T().keep_largest_connected_component(lab, applied)
    assert got.dtype == lab.dtype and np.array_equal(got, want)
    got = T().keep_largest_connected_component(lab, applied, independent=False)
    assert np.array_equal(got, cref.keep_largest_connected_component(lab, applied, False))
    assert np.array_equal(T().fill_holes(lab, applied), want_fill)
    # two components per class, face connectivity
    got = T().keep_largest_connected_component(lab, applied, True, 1, 2)
    assert np.array_equal(got, cref.keep_largest_connected_component(lab, applied, True, 1, 2))
    assert np.array_equal(T().fill_holes(lab, applied, 1), cref.fill_holes(lab, applied, 1))


def test_applied_labels_that_the_storage_type_cannot_hold():
    """found by the case above: with independent=False a label above the storage type's range (65535 in an int16
    volume) used to raise RuntimeError while the union mask was built; such a label is simply absent"""
    lab = lim.table_volume().copy()
    small = (lab % 7).astype(np.uint8)
    for vol, applied in ((lab, [3, 40000, 17, 65535]), (small, [300, 2, 5]), (small, [256, 65535])):
        for independent in (True, False):
            got = T().keep_largest_connected_component(vol, applied, independent)
            assert got.dtype == vol.dtype
            assert np.array_equal(got, cref.keep_largest_connected_component(vol, applied, independent)), (applied, independent)
        assert np.array_equal(T().fill_holes(vol, applied), cref.fill_holes(vol, applied))


@pytest.mark.parametrize("count", lim.SELECTED_COUNTS)
def test_selected_label_tables_of_one_chunk_and_one_more(count):
    lab = lim.selected_volume()
    selected = list(lim.selected_labels(count))
    got = _extract(lab, selected=selected)
    assert sorted(got) == selected
    for c in selected:
        _same_mesh(got[c], sref.surface_nets(lab, c), c)
    assert [c for c in selected if got[c].faces.shape[0] == 0] == selected[-3:]
    big, selected = lim.selected_scaled(count)
    got = _extract(big, selected=selected)
    assert sorted(got) == list(selected)
    for c in selected:
        _same_mesh(got[c], sref.surface_nets(big, c), c)
    assert sum(got[c].faces.shape[0] == 0 for c in selected) == 3 and got[selected[-1]].faces.shape[0] > 0
