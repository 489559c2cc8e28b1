"""The generators of tests/helpers/labelvol_limits.py cross the limits their GPU tests are there for (no GPU needed).
The limits are read from the ``.hip`` sources; a changed constant or an edited literal fails here, with a message
that names the generator which no longer crosses its limit, instead of turning tests/test_labelvol_limits_gpu.py
into a test of the easy path."""
import math
import shutil

import numpy as np
import pytest

from tests.helpers import components_ref as cref
from tests.helpers import labelvol_limits as lim
from tests.helpers import surface_ref as sref


def test_every_generator_crosses_its_limit():
    L = lim.read_limits()
    bad = lim.crossings(L)
    assert not bad, "\n".join(bad)


def _doctored(tmp_path, file, old, new):
    """a copy of the three sources with one edit"""
    for f in {*lim.NAMED.values(), *(v[0] for v in lim.LITERALS.values())}:
        shutil.copy(lim.CSRC / f, tmp_path / f)
    text = (tmp_path / file).read_text()
    assert text.count(old) == 1, (file, old)
    (tmp_path / file).write_text(text.replace(old, new))
    return lim.read_limits(tmp_path)


@pytest.mark.parametrize("name, generator", [("kSurfScan", "surf_volume()"), ("kDecScan", "dec_batch_starts()"),
                                             ("kScanItems", "cc_roots("), ("kAppliedChunk", "applied_labels()"),
                                             ("kSurfTableChunk", "selected_labels()")])
def test_a_doubled_constant_is_reported_with_its_generator(tmp_path, name, generator):
    value = getattr(lim.read_limits(), name)
    L = _doctored(tmp_path, lim.NAMED[name], f"constexpr int {name} = {value};", f"constexpr int {name} = {2 * value};")
    assert getattr(L, name) == 2 * value
    bad = lim.crossings(L)
    assert bad and all(name in m for m in bad) and any(m.startswith(generator) for m in bad), bad


@pytest.mark.parametrize("key", sorted(lim.LITERALS))
def test_an_edited_literal_cap_is_reported(tmp_path, key):
    file, line, _ = lim.LITERALS[key]
    number = {"boxes_grid": "4096", "map_grid": "65536", "scan_threads": "1024"}[key]
    L = _doctored(tmp_path, file, line, line.replace(number, str(2 * int(number))))
    bad = lim.crossings(L)
    assert len(bad) == 1 and file in bad[0] and line in bad[0], bad


def test_component_roots_have_empty_full_and_mixed_blocks():
    L = lim.read_limits()
    assert lim.CC_BLOCK == L.kScanItems
    for n, want in zip(lim.CC_SIZES, lim.CC_WANT):
        assert lim.scan_blocks(n, L.kScanItems, L.scan_threads) == want
    n = lim.CC_SIZES[1]
    root, comp, n_comp, per_block = lim.cc_roots(n)
    root, comp = root.reshape(-1), comp.reshape(-1)
    assert per_block.size == 1025 and int(per_block.sum()) == n_comp
    assert (per_block == 0).sum() > 100 and (per_block == lim.CC_BLOCK).sum() > 100
    assert ((per_block > 0) & (per_block < lim.CC_BLOCK)).sum() > 100
    assert per_block[-1] == 1                          # the one-voxel block that only the per = 2 range reaches
    # a valid cc_label output: roots point to themselves, the others to an earlier root or to -1
    idx = np.arange(n)
    is_root = root == idx
    assert int(is_root.sum()) == n_comp and (root <= idx).all() and (root >= -1).all()
    assert is_root[root[root >= 0]].all()
    first = int(np.flatnonzero(is_root)[0])
    assert first >= 2 * lim.CC_BLOCK and (root[:first] == -1).all()
    assert 0.1 < (root == -1).mean() < 0.6
    # the numbering is canonical: the oracle's, on a prefix that holds every kind of block
    m = 6 * lim.CC_BLOCK
    want, n_want = cref.canonical(np.where(root[:m] >= 0, root[:m], m).astype(np.int64))
    assert np.array_equal(np.where(root[:m] >= 0, want, 0), comp[:m])
    assert comp.max() == n_comp and comp[n - 1] == n_comp


def test_surface_volume_and_the_vectorised_counts():
    L = lim.read_limits()
    lab = lim.surf_volume()
    labels = list(range(1, lim.SURF_CLASSES + 1))
    assert sorted(np.unique(lab).tolist()) == labels   # every label present, no background inside
    boxes = lim.label_boxes(lab, labels)
    chunks = lim.surf_chunks(boxes)
    assert chunks == 65 * 81 * 2 * 200
    nb, per = lim.scan_blocks(chunks, L.kSurfScan, L.scan_threads)
    assert (nb, per) == (2057, 3)
    assert lim.SURF_SAMPLED[0] == 1 and lim.SURF_SAMPLED[-1] == lim.SURF_CLASSES and len(set(lim.SURF_SAMPLED)) == 16
    verts, faces = lim.surface_counts(lab, lim.SURF_CLASSES)
    for c in (lim.SURF_SAMPLED[0], lim.SURF_SAMPLED[7], lim.SURF_SAMPLED[-1]):
        want = lim.surf_oracle(c)
        assert (int(verts[c]), int(faces[c])) == (want["index"].shape[0], want["faces"].shape[0]), c
    # every label's chunks span several thread ranges of the scan: a thread owns per * kSurfScan chunks
    assert 65 * 81 * 2 > 3 * per * L.kSurfScan
    assert int(verts[1:].sum()) < 2 ** 31 and int(faces[1:].sum()) < 2 ** 31
    # the small volumes the counts are also used on: several labels, background, labels touching the border
    small = sref.noise((5, 6, 7), 3, 0.6, 2)
    v, f = lim.surface_counts(small, 3)
    for c in (1, 2, 3):
        want = sref.surface_nets(small, c)
        assert (int(v[c]), int(f[c])) == (want["index"].shape[0], want["faces"].shape[0])


def test_checkerboard_face_and_vertex_counts():
    for n in (4, 6):
        want = sref.surface_nets(lim.checkerboard(n), 1)
        assert want["faces"].shape[0] == lim.checkerboard_faces(n) == 6 * n ** 3
        assert want["index"].shape[0] == lim.checkerboard_vertices(n)
    n = lim.OVERFLOW_SIDE
    assert n % 2 == 0 and lim.checkerboard_faces(n - 2) == 2147466000 <= 2 ** 31 - 1 < lim.checkerboard_faces(n) == 2165664768
    assert lim.checkerboard_faces(n) < 2 ** 32        # the flag, not a wrapped 64-bit sum, is what refuses the volume
    assert (n + 1) ** 3 < 2 ** 31 and lim.checkerboard_vertices(n) < 2 ** 31
    board = lim.checkerboard(6)
    z, y, x = np.indices(board.shape)
    assert np.array_equal(board, ((z + y + x) % 2).astype(np.uint8))


def test_decimation_batch_sizes_and_that_decimation_does_something():
    L = lim.read_limits()
    distinct = lim.dec_distinct()
    assert [(name, len(v), len(f)) for name, v, f, _ in distinct] == \
        [("ball", 1298, 2592), ("torus", 1960, 3920), ("noise", 2095, 4172)]
    starts = lim.dec_batch_starts([(len(v), len(f)) for _, v, f, _ in distinct])
    nv, nf = (int(x) for x in starts[lim.DEC_MESHES])
    assert nv > L.kDecScan * L.scan_threads + L.kDecScan and nf > L.kDecScan * L.scan_threads + L.kDecScan
    assert lim.scan_blocks(nv + 1, L.kDecScan, L.scan_threads)[1] == 2
    assert lim.scan_blocks(nf + 1, L.kDecScan, L.scan_threads)[1] == 3
    assert 254 < lim.DEC_MESHES <= 65535 and lim.DEC_MESHES % 3 == 0
    assert max(len(v) for _, v, _, _ in distinct) < 2 ** 23
    for name, v, f, want in distinct:
        if name in ("ball", "torus"):
            assert len(want["faces"]) <= math.ceil(0.2 * len(f)), name
        assert len(want["faces"]) < len(f) and len(want["kept"]) < len(v), name


def test_box_volumes_place_their_labels_in_the_passes():
    L = lim.read_limits()
    per_pass = L.boxes_rows_per_wg * L.boxes_grid_cap
    assert per_pass == lim.BOX_ROWS_PER_PASS == 16384
    for shape in lim.BOX_SHAPES:
        assert shape[0] * shape[1] > per_pass
        for dtype, (spread, late, both, other, absent) in lim.BOX_VALUES.items():
            lab, selected = lim.box_volume(shape, dtype)
            assert lab.dtype == np.dtype(dtype) and lab.shape == shape
            assert selected == sorted(selected) and absent in selected and other not in selected
            row = lambda c: np.nonzero(lab == c)[0] * shape[1] + np.nonzero(lab == c)[1]
            assert row(late).size >= 5 and row(late).min() >= per_pass
            if shape == lim.BOX_SHAPES[0]:
                assert np.nonzero(lab == late)[0].min() >= 127
            assert row(both).size == 2 and row(both).min() < per_pass <= row(both).max()
            assert row(spread).min() < 64 and row(spread).max() >= per_pass and row(spread).size > 0.2 * lab.size
            assert row(absent).size == 0 and row(other).size > 0
            boxes = lim.label_boxes(lab, selected)
            assert (boxes[selected.index(absent)] == 0).all()
            assert boxes[selected.index(both)].tolist()[4:] == [0, shape[2]]
    assert (np.arange(shape[0] * shape[1]) // per_pass).max() == 3       # the long volume takes four passes


def test_map_labels_inputs_reach_the_tail():
    L = lim.read_limits()
    assert lim.MAP_STRIDE == L.map_per_wg * L.map_grid_cap and lim.MAP_N == lim.MAP_STRIDE + 1000
    for in_dtype, out_dtype in (("uint8", "uint8"), ("int32", "int64")):
        x, table, want = lim.map_case(in_dtype, out_dtype)
        assert x.shape == want.shape == (lim.MAP_N,) and x.dtype == np.dtype(in_dtype) and want.dtype == np.dtype(out_dtype)
        assert 0 <= int(x.min()) and int(x.max()) == table.size - 1
        tail = want[lim.MAP_STRIDE:]
        # neither a tail that was never written nor one computed from the elements one pass earlier passes
        assert (tail != want[:1000]).any() and (tail != np.asarray(lim.MAP_FILL[out_dtype]).astype(out_dtype)).any()
        # no permutation of itself under the shift: the table is not constant either
        assert np.unique(table).size > 100


def test_table_chunk_lists_and_that_the_transforms_do_something():
    L = lim.read_limits()
    lab = lim.table_volume()
    assert lab.dtype == np.int16 and lab.shape == lim.TABLE_SHAPE and 150 < np.unique(lab).size <= 201
    present = set(np.unique(lab).tolist()) - {0}
    assert lim.APPLIED_COUNTS == (L.kAppliedChunk, L.kAppliedChunk + 1, 130) and 130 > 2 * L.kAppliedChunk
    everything = cref.fill_holes(lab)
    assert 20 < int((everything != lab).sum())
    for count in lim.APPLIED_COUNTS:
        applied = list(lim.applied_labels(count))
        assert len(applied) == len(set(applied)) == count and min(applied) >= 1 and max(applied) == 65535
        assert 3 <= len(set(applied) - present) < 20 and len(set(applied) & present) > 40
        assert applied != sorted(applied) and (np.diff(applied) < 0).sum() > count // 4       # early and late mixed
        # the applied labels matter: some of their components go and some of their cavities are filled, while
        # the other classes keep islands and cavities of their own
        kept = cref.keep_largest_connected_component(lab, applied, True)
        assert (kept != lab).any() and np.isin(lab[kept != lab], applied).all()
        assert not np.array_equal(kept, cref.keep_largest_connected_component(lab, None, True))
        filled = cref.fill_holes(lab, applied)
        assert (filled != lab).any() and not np.array_equal(filled, everything)
    assert lim.SELECTED_COUNTS == (L.kSurfTableChunk, L.kSurfTableChunk + 1)
    vol = lim.selected_volume()
    for count in lim.SELECTED_COUNTS:
        sel = list(lim.selected_labels(count))
        assert len(sel) == count and sel == sorted(set(sel)) and [c for c in sel if not (vol == c).any()] == sel[-3:]
        big, sel = lim.selected_scaled(count)
        absent = [c for c in sel if not (big == c).any()]
        assert len(sel) == count and list(sel) == sorted(set(sel)) and len(absent) == 3
        assert sel[-1] not in absent and sel[0] not in absent
