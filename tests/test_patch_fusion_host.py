"""Patch-based label fusion without a GPU: the numpy restatement of the definition on cases
worked by hand, the seeded faults that the exact comparison of the GPU tests must reject, the wiring of the new
names through the header, the binding, ops and the scripts, every argument refusal of the Python layer, and the
usefulness condition on the restatement alone."""
import importlib.util
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import patch_fusion_ref as R  # noqa: E402

RAMP = np.array([1024 - k for k in range(1024)])          # a table whose entry tells the bin: W[k] = 1024 - k


def vol(values, dtype=np.uint8, shape=None):
    a = np.asarray(values, dtype)
    return a.reshape(shape if shape is not None else (1, 1, a.size))


def same(a, b) -> bool:
    """the comparison of the GPU tests: exact equality of every returned quantity"""
    return (np.array_equal(a.labels, b.labels) and np.array_equal(a.best, b.best) and np.array_equal(a.total, b.total)
            and np.array_equal(a.scores, b.scores))


# ---------------------------------------------------------------------------- the restatement on hand-worked cases
def test_reference_on_a_hand_worked_row():
    """1 x 1 x 5, one atlas, rp = rs = 1 (0 on the two axes of extent 1), fixed h2 = 1: npatch = 3, den = 3.
    T = 1 3 0 2 5, I = 2 3 1 0 4, L = 0 1 1 0 1.  D(x, o) = sum over p = -1, 0, 1 of (T[c(x + p)] - I[c(x + o + p)])^2
    with c the clamp to 0 .. 4, e.g. D(0, 0) = (1-2)^2 + (1-2)^2 + (3-3)^2 = 2 and D(3, -1) = (0-3)^2 + (2-1)^2 +
    (5-0)^2 = 35.  k = floor(64 D / 3); the table RAMP gives w = 1024 - k; the candidate (x, o) votes for L[x + o]."""
    T, I, L = [1, 3, 0, 2, 5], [2, 3, 1, 0, 4], [0, 1, 1, 0, 1]
    D = {(0, 0): 2, (0, 1): 9, (1, -1): 11, (1, 0): 2, (1, 1): 8, (2, -1): 11, (2, 0): 5, (2, 1): 8, (3, -1): 35,
         (3, 0): 6, (3, 1): 5, (4, -1): 27, (4, 0): 6}                  # (0, -1) and (4, 1) leave the row: no candidate
    k = {2: 42, 5: 106, 6: 128, 8: 170, 9: 192, 11: 234, 27: 576, 35: 746}
    c = lambda v: min(max(v, 0), 4)  # noqa: E731
    want = np.zeros((2, 5), np.int64)
    for (x, o), dist in D.items():
        assert dist == sum((T[c(x + p)] - I[c(x + o + p)]) ** 2 for p in (-1, 0, 1))
        assert k[dist] == 64 * dist // 3
        want[L[x + o], x] += 1024 - k[dist]
    assert want.tolist() == [[982, 790, 854, 896, 448], [832, 1836, 1708, 1196, 896]]
    r = R.fuse(vol(T), [vol(I)], [vol(L)], 2, 1, 1, RAMP, h2=1)
    assert r.scores.reshape(2, 5).tolist() == want.tolist() and r.scores.dtype == np.uint32
    assert r.labels.ravel().tolist() == [0, 1, 1, 1, 1] and r.labels.dtype == np.uint8
    assert r.best.ravel().tolist() == [982, 1836, 1708, 1196, 896]
    assert r.total.ravel().tolist() == [1814, 2626, 2562, 2092, 1344]
    # adaptive with the floor 3 * 1: den = max(min D, 3) = 3 3 5 5 6
    a = R.fuse(vol(T), [vol(I)], [vol(L)], 2, 1, 1, RAMP, min_h2=1)
    assert a.den.ravel().tolist() == [3, 3, 5, 5, 6]
    assert a.scores.reshape(2, 5)[:, 4].tolist() == [1024 - 64 * 27 // 6, 1024 - 64]
    # the same through the tap-by-tap sums
    assert same(r, R.fuse(vol(T), [vol(I)], [vol(L)], 2, 1, 1, RAMP, h2=1, direct=True))


def test_the_best_candidate_of_the_adaptive_bandwidth_lands_on_bin_64():
    """one voxel, T = 0, I = 10: D = 100 = den, k = 64 exactly, the weight W[64] = round(65536 / e) for beta = 1"""
    r = R.fuse(vol([0]), [vol([10])], [vol([1])], 2, 0, 0, R.table(1.0))
    assert r.den.item() == 100 and r.scores.ravel().tolist() == [0, 24109]
    assert R.fuse(vol([0]), [vol([10])], [vol([1])], 2, 0, 0, RAMP).scores.ravel().tolist() == [0, 1024 - 64]


def test_bins_below_and_on_an_edge():
    """rp = 0, fixed: den = h2.  D = 1, den = 5: 64 / 5 = 12.8 = 13 - 1/5, one below the edge of bin 13: k = 12.
    D = 16, den = 4: 1024 / 4 = 256 on the edge: k = 256.  D = 255^2, den = 1: 4 161 600, capped at 1023."""
    one = lambda t, i, h2: R.fuse(vol([t]), [vol([i])], [vol([0])], 2, 0, 0, RAMP, h2=h2).scores.ravel()[0]  # noqa: E731
    assert one(0, 1, 5) == 1024 - 12 and one(0, 4, 4) == 1024 - 256 and one(0, 255, 1) == 1024 - 1023
    assert one(7, 7, 1) == 1024


# ---------------------------------------------------------------------------- seeded faults
def _random(shape, A, K, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, shape).astype(np.uint8), [rng.integers(0, 256, shape).astype(np.uint8) for _ in range(A)],
            [rng.integers(0, K, shape).astype(np.uint8) for _ in range(A)])


def _fault_case(fault):
    if fault in ("outside", "double_clamp"):              # borders: a volume that is all border
        T, I, L = _random((3, 4, 5), 2, 3, 1)
        return (T, I, L, 3, 1, 1, R.table()), {}
    if fault == "tie_largest":                            # two atlases with one image and different labels
        T, I, _ = _random((2, 3, 4), 1, 3, 2)
        return (T, [I[0], I[0]], [np.full(T.shape, 2, np.uint8), np.full(T.shape, 1, np.uint8)], 3, 1, 0, R.table()), {}
    if fault == "no_floor":                               # the first atlas is the target (min D = 0), the second near it
        T, I, L = _random((3, 4, 5), 2, 3, 3)
        near = np.clip(T.astype(np.int64) + (I[1] % 5).astype(np.int64) - 2, 0, 255).astype(np.uint8)
        return (T, [T.copy(), near], L, 3, 1, 0, RAMP), {}
    if fault == "round_k":                                # 64 D / den = 12.8
        return (vol([0]), [vol([1])], [vol([0])], 2, 0, 0, RAMP), dict(h2=5)
    if fault == "no_fallback":                            # no candidate within a 64th of the bandwidth
        T, I, L = _random((3, 4, 5), 3, 3, 4)
        table = np.zeros(1024, np.int64)
        table[0] = 1
        return (T, I, L, 3, 1, 1, table), dict(h2=1)
    raise AssertionError(fault)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_seeded_fault_is_rejected_by_the_exact_comparison(fault):
    args, kw = _fault_case(fault)
    good = R.fuse(*args, **kw)
    assert same(good, R.fuse(*args, **kw, direct=True))           # box sums and tap-by-tap sums agree on the input
    assert not same(good, R.fuse(*args, **kw, fault=fault)), fault


def test_clamping_the_offset_position_first_changes_nothing():
    """clamp(clamp(x + o) + p) equals clamp(x + o + p) at every candidate that exists, because x + o lies inside the
    volume there: the two-step clamp that is a fault is the one that clamps the patch position first"""
    args, kw = _fault_case("double_clamp")
    assert same(R.fuse(*args, **kw), R.fuse(*args, **kw, fault="double_clamp_offset_first"))
    T, I, L = _random((1, 5, 7), 3, 4, 9)
    assert same(R.fuse(T, I, L, 4, 3, 3, RAMP), R.fuse(T, I, L, 4, 3, 3, RAMP, fault="double_clamp_offset_first"))


def test_no_fallback_case_falls_back_to_the_vote_at_most_voxels():
    args, kw = _fault_case("no_fallback")
    good = R.fuse(*args, **kw)
    fell = good.total == 3                                 # three atlases, one vote each
    assert fell.mean() > 0.5
    assert np.array_equal(good.labels[fell], R.vote(args[2], 3)[fell])


FMA_WITNESS = dict(v=float.fromhex("0x1.91919p-3"), lo=0.0, hi=100.0)


def test_quantiser_rounds_the_product_before_the_half_is_added():
    """(v - lo) * scale rounds to 0.5 - 2^-25, and 0.5 - 2^-25 + 0.5 is a tie that rounds to 1.0: q = 1.  A fused
    multiply-add sees the exact product, which lies below 0.5 - 2^-25: the sum rounds to 1 - 2^-24 and q = 0."""
    w = FMA_WITNESS
    scale = np.float32(255.0 / (w["hi"] - w["lo"]))
    t = np.float32(w["v"]) * scale
    assert t == np.float32(0.5 - 2.0 ** -25) and np.float64(np.float32(w["v"])) * np.float64(scale) < np.float64(t)
    assert R.quantise([w["v"]], w["lo"], w["hi"]).tolist() == [1]
    assert R.quantise([w["v"]], w["lo"], w["hi"], fma=True).tolist() == [0]


def test_quantiser_edges():
    q = lambda v: R.quantise(np.asarray(v, np.float32), 0.0, 255.0).tolist()  # noqa: E731
    assert q([0.0, 0.49, 0.5, 1.5, 2.5, 254.49, 254.5, 255.0]) == [0, 0, 1, 2, 3, 254, 255, 255]
    assert q([float("nan"), float("inf"), -float("inf"), -3.0, 1e30, -1e30, 300.0]) == [0, 255, 0, 0, 255, 0, 255]
    assert R.quantise(np.float32([10.0, 15.0, 20.0]), 10.0, 20.0).tolist() == [0, 128, 255]
    assert R.default_range(np.arange(1001, dtype=np.float32)) == (5.0, 995.0)
    assert R.default_range(np.arange(10, dtype=np.float32)) == (0.0, 9.0)


# ---------------------------------------------------------------------------- wiring
def test_table_values():
    from segmantic_amd import ops
    t = ops.patch_fusion_table(1.0)
    assert t.shape == (1024,) and t.dtype == np.uint32
    assert int(t[0]) == 65536 and int(t[64]) == 24109 and int(t[1023]) == 0
    assert np.array_equal(t, R.table(1.0)) and np.array_equal(ops.patch_fusion_table(0.37), R.table(0.37))
    assert int(ops.patch_fusion_table(16.0)[1023]) == int(np.floor(65536.0 * np.exp(-1023 / 1024.0) + 0.5))
    for bad in (0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="beta"):
            ops.patch_fusion_table(bad)


def test_header_binding_and_ops_export_the_new_names():
    from segmantic_amd import _lib, ops
    header = (ROOT / "include" / "segmi.h").read_text()
    for name in ("segmi_quantise_u8", "segmi_patch_fusion_workspace_bytes", "segmi_patch_fusion_variant_name",
                 "segmi_patch_fusion"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    for name in ("quantise_u8", "patch_fusion_table", "patch_fusion_variant_name", "patch_fusion"):
        assert callable(getattr(ops, name)), name
    makefile = (ROOT / "segmantic_amd" / "csrc" / "Makefile").read_text()
    assert "patch_fusion.hip" in makefile and "build/patch_fusion.o: CXXFLAGS += -ffp-contract=off" in makefile


def test_native_argument_checks_and_variant_names():
    import ctypes as C

    from segmantic_amd import _lib, ops
    lib = _lib.lib
    assert lib.segmi_patch_fusion_workspace_bytes(0, 4) == 0 and lib.segmi_patch_fusion_workspace_bytes(17, 4) == 0
    assert lib.segmi_patch_fusion_workspace_bytes(3, 1) == 0 and lib.segmi_patch_fusion_workspace_bytes(3, 65) == 0
    assert lib.segmi_patch_fusion_workspace_bytes(16, 64) > 0 and lib.segmi_patch_fusion_workspace_bytes(1, 2) % 256 == 0
    small, large = ops.patch_fusion_variant_name(2), ops.patch_fusion_variant_name(64, 3, 3)
    assert small and large and small != large
    assert ops.patch_fusion_variant_name(17, 2, 2) == small and ops.patch_fusion_variant_name(65) == ""
    assert ops.patch_fusion_variant_name(1) == ""
    r = (C.c_int32 * 3)(1, 1, 1)
    four = (C.c_int32 * 3)(1, 4, 1)
    assert lib.segmi_patch_fusion_variant_name(4, r, four) == b"" and lib.segmi_patch_fusion_variant_name(4, None, r) == b""
    info = (C.c_int32 * 2)()
    one = C.c_void_p(256)                                   # never read: every call below is refused before a launch
    tab = (C.c_void_p * 1)(256)
    call = lambda **kw: lib.segmi_patch_fusion(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("tq", one), ("iq", tab), ("lab", tab), ("atlases", 1), ("lb", 1), ("d", 2), ("h", 3), ("w", 4), ("K", 3),
        ("rp", r), ("rs", r), ("adaptive", 1), ("h2", 4), ("table", one), ("out", one), ("best", None), ("total", None),
        ("scores", None), ("info", info), ("ws", one), ("ws_bytes", 0), ("stream", None))])
    assert call() != 0 and "workspace" in _lib.last_error()  # everything valid but the workspace size
    for kw in (dict(tq=None), dict(table=None), dict(out=None), dict(atlases=0), dict(atlases=17), dict(lb=3), dict(d=0),
               dict(K=1), dict(K=65), dict(rp=four), dict(rs=four), dict(adaptive=2), dict(h2=0), dict(h2=65026),
               dict(d=2048, h=2048, w=512)):
        assert call(ws_bytes=1 << 20, **kw) != 0, kw
        assert "patch_fusion" in _lib.last_error() and "workspace" not in _lib.last_error(), (kw, _lib.last_error())
    assert lib.segmi_quantise_u8(one, 10, 1.0, 1.0, one, None) != 0 and "quantise_u8" in _lib.last_error()
    assert lib.segmi_quantise_u8(one, 10, 0.0, float("inf"), one, None) != 0
    assert lib.segmi_quantise_u8(one, 10, float("nan"), 1.0, one, None) != 0
    assert lib.segmi_quantise_u8(one, 10, 0.0, 1e-44, one, None) != 0
    assert lib.segmi_quantise_u8(one, 0, 0.0, 1.0, one, None) != 0 and lib.segmi_quantise_u8(None, 1, 0.0, 1.0, one, None) != 0


def test_every_argument_error_of_the_python_layer_names_its_argument():
    from segmantic_amd.seg.patch_fusion import patch_fusion
    t = np.linspace(0, 1, 60, dtype=np.float32).reshape(3, 4, 5)
    lab = np.zeros((3, 4, 5), np.uint8)
    ok = dict(target=t, atlas_images=[t, t], atlas_labels=[lab, lab], num_classes=2)
    call = lambda **kw: patch_fusion(**{**ok, **kw})  # noqa: E731
    for kw, exc, match in (
            (dict(atlas_images=[], atlas_labels=[]), ValueError, "atlases"),
            (dict(atlas_images=[t] * 17, atlas_labels=[lab] * 17), ValueError, "atlases"),
            (dict(atlas_images=[t]), ValueError, "1 atlas images for 2 label maps"),
            (dict(atlas_images=t), TypeError, "atlas_images must be a sequence"),
            (dict(atlas_labels=lab), TypeError, "atlas_labels must be a sequence"),
            (dict(target="x"), TypeError, "expected an Image"),
            (dict(target=np.zeros(7, np.float32)), ValueError, "2-D or 3-D"),
            (dict(atlas_images=[t, t[:2]]), ValueError, r"atlas_images\[1\].*shape"),
            (dict(atlas_labels=[lab, np.zeros((3, 4, 6), np.uint8)]), ValueError, r"atlas_labels\[1\].*shape"),
            (dict(atlas_labels=[lab, lab.astype(np.float32)]), TypeError, r"atlas_labels\[1\].*float"),
            (dict(atlas_images=[t, t.astype(np.complex64)]), TypeError, r"atlas_images\[1\].*real"),
            (dict(num_classes=1), ValueError, "num_classes"), (dict(num_classes=65), ValueError, "num_classes"),
            (dict(num_classes=2.5), ValueError, "num_classes"),
            (dict(patch_radius=4), ValueError, "patch_radius"), (dict(patch_radius=-1), ValueError, "patch_radius"),
            (dict(patch_radius=(1, 1)), ValueError, "patch_radius"), (dict(patch_radius=1.5), ValueError, "patch_radius"),
            (dict(search_radius=(0, 0, 4)), ValueError, "search_radius"), (dict(search_radius="2"), ValueError, "search_radius"),
            (dict(beta=0.0), ValueError, "beta"), (dict(beta=float("nan")), ValueError, "beta"),
            (dict(bandwidth="fixed"), ValueError, "bandwidth"), (dict(bandwidth=0), ValueError, "bandwidth"),
            (dict(bandwidth=2.5), ValueError, "bandwidth"), (dict(bandwidth=65026), ValueError, "bandwidth"),
            (dict(min_h2=0), ValueError, "min_h2"), (dict(min_h2=1.5), ValueError, "min_h2"),
            (dict(intensity_ranges=[(0, 1)]), ValueError, "intensity_ranges"),
            (dict(intensity_ranges=[(0, 1), (1, 1), None]), ValueError, "lo < hi"),
            (dict(intensity_ranges=[(0, 1), (0, float("inf")), None]), ValueError, "lo < hi"),
            (dict(intensity_ranges=[(0, 1), 5, None]), ValueError, "intensity_ranges"),
            (dict(atlas_images=[t, np.full((3, 4, 5), 2.0, np.float32)]), ValueError, r"atlas_images\[1\] is constant"),
            (dict(target=np.zeros((3, 4, 5), np.float32)), ValueError, "target is constant"),
            (dict(atlas_labels=[lab, np.full((3, 4, 5), 2, np.int64)]), ValueError, "atlas 1 holds the label 2"),
            (dict(atlas_labels=[lab, np.full((3, 4, 5), 2 ** 32 + 1, np.int64)], num_classes=3), ValueError,
             "atlas 1 holds the label 4294967297")):
        with pytest.raises(exc, match=match):
            call(**kw)
    if not torch.cuda.is_available():                       # every check passed: only the device is missing
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


def test_ops_patch_fusion_checks_arguments_before_the_tensors():
    from segmantic_amd import ops
    q, lab = torch.zeros((2, 3, 4), dtype=torch.uint8), torch.zeros((2, 3, 4), dtype=torch.uint8)
    table = ops.patch_fusion_table(1.0)
    for kw, name in ((dict(num_classes=1), "num_classes"), (dict(num_classes=2, patch_radius=4), "patch_radius"),
                     (dict(num_classes=2, search_radius=(1, 2)), "search_radius"), (dict(num_classes=2, h2=0), "h2"),
                     (dict(num_classes=2, min_h2=-1), "min_h2"), (dict(num_classes=2, table=table[:5]), "table"),
                     (dict(num_classes=2, table=table.astype(np.int64) * 2), "table"),
                     (dict(num_classes=2, table=np.zeros(1024, np.int64)), "table")):
        kw = {"table": table, **kw}
        with pytest.raises(ValueError, match=name):
            ops.patch_fusion(q, [q], [lab], **kw)
    with pytest.raises(ValueError, match="label maps"):
        ops.patch_fusion(q, [q, q], [lab], 2, table=table)
    with pytest.raises(RuntimeError, match="MI355X"):       # host tensors are refused
        ops.patch_fusion(q, [q], [lab], 2, table=table)
    with pytest.raises(ValueError, match="lo < hi"):
        ops.quantise_u8(torch.zeros(4), 1.0, 1.0)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.quantise_u8(torch.zeros(4), 0.0, 1.0)


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script,options", [
    ("multi_atlas_segment.py", ("--fusion", "--patch-radius", "--search-radius", "--beta", "--atlas", "--grid-spacing")),
    ("patch_fuse_labels.py", ("--atlas", "--tissue-list", "--patch-radius", "--search-radius", "--beta", "TARGET", "OUTPUT"))])
def test_scripts_list_their_options(script, options):
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / script), "--help"], capture_output=True, text=True,
                         env={**os.environ, "COLUMNS": "200", "TERM": "dumb"})
    assert out.returncode == 0, out.stderr
    for opt in options:
        assert opt in out.stdout, opt


def test_fusion_staple_takes_the_code_path_of_before(monkeypatch, tmp_path):
    """with the registration, the warp, STAPLE and the file output replaced by recorders: ``fusion="staple"`` warps
    the label maps only, calls STAPLE, writes OUTPUT and staple_performance.csv and never reaches the patch fusion;
    ``fusion="patch"`` warps the images too, calls the patch fusion and writes no csv"""
    from types import SimpleNamespace

    from segmantic_amd.image import processing, registration
    from segmantic_amd.seg import patch_fusion as P
    from segmantic_amd.seg import staple as S
    mas = _load_script("multi_atlas_segment")
    calls = []
    image = processing.Image(np.zeros((2, 3, 4), np.float32))
    monkeypatch.setattr(processing, "read_image", lambda p: processing.Image(np.zeros((2, 3, 4), np.float32)))
    monkeypatch.setattr(processing, "write_image", lambda im, p: calls.append(("write", Path(p).name)))
    monkeypatch.setattr(registration, "register", lambda *a, **k: SimpleNamespace(transform=None))
    monkeypatch.setattr(registration, "register_deformable", lambda *a, **k: SimpleNamespace(folded=0))
    monkeypatch.setattr(registration, "warp", lambda m, f, r, nearest=False: calls.append(("warp", nearest)) or image)
    monkeypatch.setattr(S, "staple", lambda labels, k: calls.append(("staple", len(labels))) or SimpleNamespace(
        labels=image.data, sums=np.zeros((len(labels), 2, 2), np.int64), iterations=1))
    monkeypatch.setattr(S, "write_performance_csv", lambda rows, p: calls.append(("csv", Path(p).name)))
    monkeypatch.setattr(P, "patch_fusion", lambda *a, **k: calls.append(("patch", k)) or P.PatchFusionResult(
        image.data, image.data))
    atlases = [(tmp_path / "a.nii.gz", tmp_path / "la.nii.gz"), (tmp_path / "b.nii.gz", tmp_path / "lb.nii.gz")]
    r = mas.segment(tmp_path / "t.nii.gz", tmp_path / "out.nii.gz", atlases)
    assert calls == [("warp", True), ("warp", True), ("staple", 2), ("write", "out.nii.gz"), ("csv", "staple_performance.csv")]
    assert set(r) == {"labels", "staple", "results", "affine_labels"}
    del calls[:]
    r = mas.segment(tmp_path / "t.nii.gz", tmp_path / "out.nii.gz", atlases, fusion="patch", patch_radius=2,
                    search_radius=(0, 1, 1), beta=0.5)
    assert calls == [("warp", True), ("warp", False), ("warp", True), ("warp", False),
                     ("patch", dict(patch_radius=2, search_radius=(0, 1, 1), beta=0.5)), ("write", "out.nii.gz"),
                     ("write", "out_confidence.nii.gz")]
    assert r["confidence_path"] == tmp_path / "out_confidence.nii.gz" and "staple" not in r
    with pytest.raises(ValueError, match="fusion"):
        mas.segment(tmp_path / "t.nii.gz", tmp_path / "out.nii.gz", atlases, fusion="vote")


# ---------------------------------------------------------------------------- the usefulness condition
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_patch_fusion_repairs_what_the_vote_gets_wrong(seed):
    """12 x 20 x 28, 4 classes, 5 atlases shifted by up to 2 voxels in-plane and 1 in z, noise 8 on 0 .. 255, rp = 1,
    rs = 2, beta = 1, adaptive: the fused labels are wrong at no more than a tenth as many voxels as the majority vote"""
    ph = R.phantom((12, 20, 28), 4, 5, seed, max_shift=(1, 2, 2), noise=8.0)
    fused = R.fuse_images(ph, 1, 2, 1.0)
    wrong = int((fused.labels != ph.truth).sum())
    wrong_vote = int((R.vote(ph.labels, 4) != ph.truth).sum())
    print(f"seed {seed}: vote wrong at {wrong_vote} voxels, patch fusion at {wrong} of {ph.truth.size}")
    assert wrong_vote > 0 and 10 * wrong <= wrong_vote
