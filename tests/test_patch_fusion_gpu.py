"""Patch-based label fusion on the MI355X against the numpy restatement of its definition
(tests/helpers/patch_fusion_ref.py).  Everything after the quantiser is an integer, and the
quantiser rounds every float32 operation on its own on both sides, so every comparison is exact equality: labels,
best, total and the full score table."""
import functools
import importlib.util
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import patch_fusion_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (12, 20, 28)                                    # 2 x 3 x 4 tiles of 8^3, ragged along z, y and x
SMALL = (8, 14, 18)                                     # 2 016 voxels: K = 64 at radii (3, 3)
RAMP = np.array([1024 - k for k in range(1024)])
SOURCE = ROOT / "segmantic_amd" / "csrc" / "patch_fusion.hip"


def _ops():
    from segmantic_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def limits():
    """the tile extents and the class limit of the small-K form, read out of the source"""
    text = SOURCE.read_text()
    out = {}
    for name in ("kPfTileX", "kPfTileY", "kPfTileZSmall", "kPfTileZLarge", "kPfSmallMaxLabels", "kPfQuantGridCap",
                 "kPfCheckGridCap"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m is not None, f"patch_fusion.hip no longer defines `constexpr int {name} = <integer>;`"
        out[name] = int(m.group(1))
    assert "(unsigned)tiles, kPfThreads" in text, "the fusion grid is no longer one workgroup per tile: test its cap"
    return out


def inputs(shape, A, K, seed, dtype=np.uint8, sigma=12.0):
    """a smooth-ish random target, atlas images near it (so that the weights spread over the table), blocky labels"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, [-(-n // 3) for n in shape])
    base = coarse.repeat(3, 0).repeat(3, 1).repeat(3, 2)[:shape[0], :shape[1], :shape[2]].astype(np.float64)
    T = np.clip(base + rng.normal(0, sigma, shape), 0, 255).astype(np.uint8)
    I = [np.clip(rng.uniform(0.9, 1.1) * base + rng.normal(0, sigma, shape), 0, 255).astype(np.uint8) for _ in range(A)]
    blocks = rng.integers(0, K, [-(-n // 2) for n in shape])
    L = []
    for _ in range(A):
        lab = blocks.repeat(2, 0).repeat(2, 1).repeat(2, 2)[:shape[0], :shape[1], :shape[2]].copy()
        flip = rng.random(shape) < 0.3
        lab[flip] = rng.integers(0, K, int(flip.sum()))
        L.append(lab.astype(dtype))
    for a in [T] + I + L:
        a.setflags(write=False)
    return T, I, L


def run(T, I, L, K, rp, rs, table, **kw):
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
    out = _ops().patch_fusion(dev(T), [dev(a) for a in I], [dev(a) for a in L], K, patch_radius=rp, search_radius=rs,
                              table=np.asarray(table), return_scores=True, return_confidence=True, **kw)
    torch.cuda.synchronize()
    return out


def check(got, ref):
    labels, best, total, scores = (t.cpu().numpy() for t in got)
    assert labels.dtype == ref.labels.dtype and labels.shape == ref.labels.shape
    assert np.array_equal(scores.astype(np.uint32), ref.scores)
    assert np.array_equal(total.astype(np.uint32), ref.total) and np.array_equal(best.astype(np.uint32), ref.best)
    assert np.array_equal(labels, ref.labels)


def both(T, I, L, K, rp, rs, table, **kw):
    check(run(T, I, L, K, rp, rs, table, **kw), R.fuse(T, I, L, K, rp, rs, table, **kw))


# ---------------------------------------------------------------------------- 1. parity sweep
# (atlases, classes, patch radius, search radius, h2 (None: adaptive), label type, shape)
SWEEP = [
    (1, 2, 0, 0, None, np.uint8, SHAPE),
    (5, 17, 1, 0, 20, np.int16, SHAPE),
    (5, 17, 1, 2, None, np.uint8, SHAPE),
    (16, 17, 2, 1, 30, np.int32, SHAPE),
    (5, 64, 3, 3, None, np.uint8, SMALL),
    (5, 2, (0, 1, 3), (3, 0, 1), None, np.int16, SHAPE),
    (5, 17, (3, 1, 0), (1, 0, 3), 9, np.int32, SHAPE),
    (16, 64, 1, 1, None, np.int16, SHAPE),
    (1, 64, 2, 1, 50, np.int32, SHAPE),
    (5, 19, 1, 2, None, np.uint8, SHAPE),               # the first class count of the large-K form
    (5, 18, 1, 2, 15, np.uint8, SHAPE),                 # the last of the small-K form
]


@pytest.mark.parametrize("A,K,rp,rs,h2,dtype,shape", SWEEP)
def test_parity_sweep(A, K, rp, rs, h2, dtype, shape):
    T, I, L = inputs(shape, A, K, 7 * A + K, dtype)
    both(T, I, L, K, rp, rs, R.table(1.0), h2=h2)


def test_the_sweep_runs_both_score_variants():
    ops, lim = _ops(), limits()
    names = {ops.patch_fusion_variant_name(K, rp, rs) for _, K, rp, rs, _, _, _ in SWEEP}
    assert len(names) == 2 and "" not in names
    small, large = ops.patch_fusion_variant_name(lim["kPfSmallMaxLabels"]), ops.patch_fusion_variant_name(lim["kPfSmallMaxLabels"] + 1)
    assert {small, large} == names and small != large
    assert f"{lim['kPfTileZSmall']}x{lim['kPfTileY']}x{lim['kPfTileX']}" in small
    assert f"{lim['kPfTileZLarge']}x{lim['kPfTileY']}x{lim['kPfTileX']}" in large


# ---------------------------------------------------------------------------- 2. tile edges
def edge_shapes():
    lim = limits()
    out = []
    for tz in (lim["kPfTileZSmall"], lim["kPfTileZLarge"]):
        tile = (tz, lim["kPfTileY"], lim["kPfTileX"])
        out.append(tile)
        out += [tuple(n + (a == ax) for a, n in enumerate(tile)) for ax in range(3)]
    return out + [(1, 5, 7), (2, 3, 3), (1, 1, 1), (1, 40, 50), (1, 1, 300)]


@pytest.mark.parametrize("K", [3, 20])
def test_tile_edges(K):
    """one tile exactly, one voxel more along each axis in turn, volumes smaller than the halo, one voxel, a 2-D
    image and a row, all at the largest radii and through both tile shapes"""
    assert _ops().patch_fusion_variant_name(K, 3, 3) == _ops().patch_fusion_variant_name(2 if K == 3 else 64, 3, 3)
    for n, shape in enumerate(edge_shapes()):
        T, I, L = inputs(shape, 2, K, 100 + n)
        both(T, I, L, K, 3, 3, RAMP)
        both(T, I, L, K, 1, 2, RAMP, h2=40)


def test_two_dimensional_input_keeps_its_rank():
    T, I, L = inputs((1, 40, 50), 3, 5, 3)
    ref = R.fuse(T[0], [a[0] for a in I], [a[0] for a in L], 5, 2, 2, R.table())
    assert ref.labels.shape == (40, 50)
    check(run(T[0], [a[0] for a in I], [a[0] for a in L], 5, 2, 2, R.table()), ref)
    assert np.array_equal(ref.scores, R.fuse(T, I, L, 5, 2, 2, R.table()).scores[:, 0])


# ---------------------------------------------------------------------------- 3. division edges
def test_exact_multiples_of_the_denominator():
    """rp = 0 and h2 = 4: den = 4 and D = diff^2, so 64 D / den = 16 D is whole at every candidate; den = 3 * 5, where
    some candidates land on an edge and most do not; adaptive, where the best candidate of a voxel has D = den"""
    rng = np.random.default_rng(5)
    T = rng.integers(0, 200, SHAPE).astype(np.uint8)
    I = [(T + 2 * rng.integers(0, 9, SHAPE)).astype(np.uint8) for _ in range(3)]
    L = [rng.integers(0, 4, SHAPE).astype(np.uint8) for _ in range(3)]
    both(T, I, L, 4, 0, 1, RAMP, h2=4)
    both(T, I, L, 4, (0, 0, 1), 1, RAMP, h2=5)
    both(T, I, L, 4, 0, 1, RAMP)                          # adaptive: the best candidate has 64 D / den = 64


def test_the_largest_distance():
    """target 0, atlas 255, rp = 3: D = 343 * 65025 = 22 303 575 at every candidate, 64 D = 1 427 428 800 < 2^31"""
    shape = (8, 9, 10)
    T, I = np.zeros(shape, np.uint8), [np.full(shape, 255, np.uint8)] * 2
    L = [np.full(shape, 1, np.uint8), (np.arange(720).reshape(shape) % 3).astype(np.uint8)]
    for kw in (dict(h2=1), dict(h2=65025), dict(h2=65024), dict(min_h2=65025), dict(min_h2=1)):
        both(T, I, L, 3, 3, 1, RAMP, **kw)
    assert R.fuse(T, I, L, 3, 3, 1, RAMP, h2=65025).best.max() > 0


def test_the_denominator_at_its_floor():
    T, I, L = inputs(SHAPE, 3, 5, 11)
    I = [T.copy()] + I[1:]                                # min D = 0 everywhere: den = npatch * min_h2
    for min_h2 in (1, 4, 300):
        ref = R.fuse(T, I, L, 5, 1, 1, RAMP, min_h2=min_h2)
        assert (ref.den == 27 * min_h2).all()
        check(run(T, I, L, 5, 1, 1, RAMP, min_h2=min_h2), ref)


# ---------------------------------------------------------------------------- 4. fallback
def test_voxels_without_any_weight_take_the_vote():
    rng = np.random.default_rng(8)
    T = rng.integers(0, 256, SHAPE).astype(np.uint8)
    I = [rng.integers(0, 256, SHAPE).astype(np.uint8) for _ in range(4)]
    I[0] = np.where(rng.random(SHAPE) < 0.1, T, I[0])    # a tenth of the voxels keeps a candidate at D = 0 (rp = 0)
    L = [rng.integers(0, 6, SHAPE).astype(np.int16) for _ in range(4)]
    table = np.zeros(1024, np.int64)
    table[0] = 1
    for K in (6, 25):
        ref = R.fuse(T, I, L, K, 0, (0, 1, 1), table, h2=1)
        fell = ref.total == 4
        assert 0.5 < fell.mean() < 1.0 and np.array_equal(ref.labels[fell], R.vote(L, K)[fell])
        check(run(T, I, L, K, 0, (0, 1, 1), table, h2=1), ref)


def test_all_ones_without_a_search_window_is_the_ensemble_vote():
    ops = _ops()
    T, I, L = inputs(SHAPE, 5, 7, 21, np.int32)
    got = run(T, I, L, 7, 2, 0, np.ones(1024, np.int64), h2=3)
    labs = [torch.from_numpy(np.array(a)).to(DEV) for a in L]
    vote = torch.empty_like(labs[0])
    ops.ensemble_vote(labs, vote)
    assert torch.equal(got[0], vote)
    assert np.array_equal(got[0].cpu().numpy(), R.vote(L, 7))
    assert (got[2] == 5).all()


# ---------------------------------------------------------------------------- 5. quantiser
def quantise(v, lo, hi):
    out = _ops().quantise_u8(torch.from_numpy(np.asarray(v, np.float32)).to(DEV), lo, hi)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8
    return out.cpu().numpy()


def test_quantiser_boundaries_and_specials():
    v = np.float32([0.0, 0.49, 0.5, 1.5, 2.5, 254.49, 254.5, 255.0, np.nan, np.inf, -np.inf, -3.0, 1e30, -1e30, 300.0])
    assert quantise(v, 0.0, 255.0).tolist() == [0, 0, 1, 2, 3, 254, 255, 255, 0, 255, 0, 0, 255, 0, 255]
    assert np.array_equal(quantise(v, 0.0, 255.0), R.quantise(v, 0.0, 255.0))
    half = (np.arange(0, 256, dtype=np.float32) + np.float32(0.5)) * np.float32(100.0 / 255.0) + np.float32(-20.0)
    near = np.concatenate([half, np.nextafter(half, np.float32(-1e9)), np.nextafter(half, np.float32(1e9))])
    assert np.array_equal(quantise(near, -20.0, 80.0), R.quantise(near, -20.0, 80.0))


def test_quantiser_does_not_fuse_the_multiply_and_the_add():
    v, lo, hi = float.fromhex("0x1.91919p-3"), 0.0, 100.0  # the witness of tests/test_patch_fusion_host.py
    assert R.quantise([v], lo, hi).tolist() == [1] and R.quantise([v], lo, hi, fma=True).tolist() == [0]
    assert quantise([v], lo, hi).tolist() == [1]


@pytest.mark.parametrize("n", [1, 255, 257, "pass"])
def test_quantiser_sizes(n):
    if n == "pass":
        n = limits()["kPfQuantGridCap"] * 256 + 1         # one element beyond a pass of the capped grid
    v = (np.random.default_rng(n).random(n, dtype=np.float32) * np.float32(1.3) - np.float32(0.15))
    assert np.array_equal(quantise(v, 0.0, 1.0), R.quantise(v, 0.0, 1.0))


# ---------------------------------------------------------------------------- 6. other cases
@pytest.mark.parametrize("dtype,bad,where", [(np.uint8, 200, 17), (np.int16, -1, 6719), (np.int32, 70000, 0)])
def test_a_label_out_of_range_is_reported_and_nothing_is_written(dtype, bad, where):
    ops = _ops()
    T, I, L = inputs(SHAPE, 3, 5, 31, dtype)
    L = [a.copy() for a in L]
    L[2].reshape(-1)[where] = bad
    if where + 1 < T.size:
        L[1].reshape(-1)[where + 1] = 5                   # a later voxel of an earlier atlas is not the one reported
    with pytest.raises(ValueError, match=rf"atlas 2 holds the label {bad}, outside 0 \.\. 4"):
        R.fuse(T, I, L, 5, 1, 1, RAMP)
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
    lib, C = __import__("segmantic_amd._lib", fromlist=["lib"]), __import__("ctypes")
    tq, iq, ls = dev(T), [dev(a) for a in I], [dev(a) for a in L]
    fill = {np.uint8: 0xAA, np.int16: 0x5555, np.int32: 0x55555555}[dtype]
    out = torch.full(SHAPE, fill, dtype=ls[0].dtype, device=DEV)
    best, total = (torch.full(SHAPE, 0x55555555, dtype=torch.int32, device=DEV) for _ in range(2))
    scores = torch.full((5,) + SHAPE, 0x55555555, dtype=torch.int32, device=DEV)
    table = dev(RAMP.astype(np.int32))
    ws = torch.empty(int(lib.lib.segmi_patch_fusion_workspace_bytes(3, 5)), dtype=torch.uint8, device=DEV)
    info = (C.c_int32 * 2)()
    r3 = (C.c_int32 * 3)(1, 1, 1)
    rc = lib.lib.segmi_patch_fusion(tq.data_ptr(), (C.c_void_p * 3)(*[t.data_ptr() for t in iq]),
                                    (C.c_void_p * 3)(*[t.data_ptr() for t in ls]), 3, ls[0].element_size(), *SHAPE, 5, r3, r3,
                                    1, 4, table.data_ptr(), out.data_ptr(), best.data_ptr(), total.data_ptr(),
                                    scores.data_ptr(), info, ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0 and (info[0], info[1]) == (2, bad)
    assert (out == fill).all() and (best == 0x55555555).all() and (total == 0x55555555).all() and (scores == 0x55555555).all()
    with pytest.raises(ValueError, match=rf"atlas 2 holds the label {bad}, outside 0 \.\. 4"):
        ops.patch_fusion(tq, iq, ls, 5, patch_radius=1, search_radius=1, table=RAMP)


def test_a_label_out_of_range_beyond_one_pass_of_the_check():
    n = limits()["kPfCheckGridCap"] * 256 + 300
    ops = _ops()
    tq = torch.zeros((1, 1, n), dtype=torch.uint8, device=DEV)
    lab = torch.zeros((1, 1, n), dtype=torch.uint8, device=DEV)
    lab[0, 0, n - 2] = 9
    with pytest.raises(ValueError, match=r"atlas 0 holds the label 9, outside 0 \.\. 3"):
        ops.patch_fusion(tq, [tq], [lab], 4, patch_radius=0, search_radius=0, table=RAMP)
    lab[0, 0, n - 2] = 3
    out, best, total = ops.patch_fusion(tq, [tq], [lab], 4, patch_radius=0, search_radius=0, table=RAMP, return_confidence=True)
    assert torch.equal(out, lab) and (best == 1024).all() and (total == 1024).all()


def test_two_calls_on_one_workspace_are_bit_identical():
    """the allocator hands the second call the workspace and the outputs' memory of the first"""
    T, I, L = inputs(SHAPE, 5, 17, 41)
    first = [t.cpu().numpy() for t in run(T, I, L, 17, 1, 2, R.table())]
    second = [t.cpu().numpy() for t in run(T, I, L, 17, 1, 2, R.table())]
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    lib, C = __import__("segmantic_amd._lib", fromlist=["lib"]), __import__("ctypes")
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
    tq, iq, ls = dev(T), [dev(a) for a in I], [dev(a) for a in L]
    table = dev(R.table().astype(np.int32))
    ws = torch.empty(int(lib.lib.segmi_patch_fusion_workspace_bytes(5, 17)), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.empty(SHAPE, dtype=torch.uint8, device=DEV)
        scores = torch.empty((17,) + SHAPE, dtype=torch.int32, device=DEV)
        info = (C.c_int32 * 2)()
        r1, r2 = (C.c_int32 * 3)(1, 1, 1), (C.c_int32 * 3)(2, 2, 2)
        assert lib.lib.segmi_patch_fusion(tq.data_ptr(), (C.c_void_p * 5)(*[t.data_ptr() for t in iq]),
                                          (C.c_void_p * 5)(*[t.data_ptr() for t in ls]), 5, 1, *SHAPE, 17, r1, r2, 1, 4,
                                          table.data_ptr(), out.data_ptr(), None, None, scores.data_ptr(), info,
                                          ws.data_ptr(), ws.numel(), None) == 0
        torch.cuda.synchronize()
        outs.append((out.cpu().numpy(), scores.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][0], first[0]) and np.array_equal(outs[0][1], first[3])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_usefulness_phantom_through_the_python_layer(seed):
    """the phantom of tests/test_patch_fusion_host.py through seg.patch_fusion: the same bits as the restatement, and
    wrong at no more than a tenth as many voxels as ensemble_vote"""
    from segmantic_amd.seg.patch_fusion import patch_fusion
    ops = _ops()
    ph = R.phantom((12, 20, 28), 4, 5, seed, max_shift=(1, 2, 2), noise=8.0)
    res = patch_fusion(ph.target, ph.images, ph.labels, 4, patch_radius=1, search_radius=2, beta=1.0, return_scores=True)
    ref = R.fuse_images(ph, 1, 2, 1.0)
    assert isinstance(res.labels, np.ndarray) and res.labels.dtype == np.uint8
    assert np.array_equal(res.labels, ref.labels) and np.array_equal(res.scores.astype(np.uint32), ref.scores)
    assert res.confidence.dtype == np.float32
    assert np.allclose(res.confidence, ref.best.astype(np.float64) / ref.total.astype(np.float64), rtol=1e-6, atol=0)
    labs = [torch.from_numpy(np.array(a)).to(DEV).to(torch.int32) for a in ph.labels]
    vote = torch.empty_like(labs[0])
    ops.ensemble_vote(labs, vote)
    wrong = int((res.labels != ph.truth).sum())
    wrong_vote = int((vote.cpu().numpy() != ph.truth).sum())
    print(f"seed {seed}: ensemble_vote wrong at {wrong_vote} voxels, patch fusion at {wrong} of {ph.truth.size}")
    assert wrong_vote > 0 and 10 * wrong <= wrong_vote


def test_python_layer_forms_and_ranges():
    """tensors and Images come back in their own form; given ranges are used as they are; device images get their
    default range on the device, equal to the host's"""
    from segmantic_amd.image.processing import Image
    from segmantic_amd.seg.patch_fusion import patch_fusion
    ph = R.phantom((6, 10, 12), 3, 2, 5)
    ref = R.fuse_images(ph, 1, 1, 0.5)
    host = patch_fusion(ph.target, ph.images, ph.labels, patch_radius=1, search_radius=1, beta=0.5)
    assert np.array_equal(host.labels, ref.labels) and host.scores is None
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
    dev = patch_fusion(t(ph.target), [t(a) for a in ph.images], [t(a).to(torch.int64) for a in ph.labels], 3,
                       patch_radius=1, search_radius=1, beta=0.5)
    assert dev.labels.is_cuda and dev.labels.dtype == torch.int64 and np.array_equal(dev.labels.cpu().numpy(), ref.labels)
    im = patch_fusion(Image(np.array(ph.target), (2.0, 1.0, 1.0)), ph.images, ph.labels, 3, patch_radius=1,
                      search_radius=1, beta=0.5)
    assert isinstance(im.labels, Image) and im.labels.spacing == (2.0, 1.0, 1.0) and isinstance(im.confidence, Image)
    assert np.array_equal(im.labels.numpy(), ref.labels)
    ranges = [(0.0, 255.0), (10.0, 240.0), None]
    got = patch_fusion(ph.target, ph.images, ph.labels, 3, patch_radius=1, search_radius=1, bandwidth=30,
                       intensity_ranges=ranges)
    tq = R.quantise(ph.target, 0.0, 255.0)
    iq = [R.quantise(ph.images[0], 10.0, 240.0), R.quantise(ph.images[1], *R.default_range(ph.images[1]))]
    assert np.array_equal(got.labels, R.fuse(tq, iq, ph.labels, 3, 1, 1, R.table(1.0), h2=30).labels)


# ---------------------------------------------------------------------------- 7. multi-atlas segmentation
def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_multi_atlas_segment_with_patch_fusion(tmp_path):
    """the 24^3 registration phantom of tests/test_deformable_gpu.py with --fusion patch: OUTPUT and the confidence
    file are written, no staple_performance.csv, and the labels are those of patch_fusion on the same warped inputs"""
    import deformable_ref as D
    import registration_ref as RR
    from segmantic_amd.image import processing as P
    from segmantic_amd.seg.patch_fusion import patch_fusion
    mas = _load_script("multi_atlas_segment")
    size, spacing = (24, 24, 24), (2.0, 2.0, 2.0)
    origin = RR.centred_origin(size, spacing)
    pts = RR._points(size, spacing, origin)

    def anatomy(p):
        v = RR.phantom(p)
        return v, (v > 0.25).astype(np.uint8) + (v > 0.55).astype(np.uint8)

    rng = np.random.default_rng(4)
    tv, tl = anatomy(pts)
    write = lambda arr, name: P.write_image(P.Image(arr, spacing, tuple(origin)), tmp_path / name) or tmp_path / name  # noqa: E731
    target = write((tv + 0.01 * rng.standard_normal(tv.shape)).astype(np.float32), "target.nii.gz")
    atlases = []
    for k in range(2):
        u = D.field_at(D.smooth_field((5, 5, 5), 9.0, 20 + k), size, spacing, origin, pts)
        av, al = anatomy(pts + u)
        atlases.append((write(RR.remap(av + 0.01 * rng.standard_normal(av.shape)).astype(np.float32), f"atlas{k}.nii.gz"),
                        write(al, f"labels{k}.nii.gz")))
    out = tmp_path / "fused.nii.gz"
    report = mas.segment(target, out, atlases, grid_spacing=10.0, levels=(2, 1), max_iterations=8, fusion="patch",
                         patch_radius=1, search_radius=1)
    fused = P.read_image(out).numpy()
    conf = P.read_image(tmp_path / "fused_confidence.nii.gz").numpy()
    assert fused.shape == tl.shape and conf.shape == tl.shape and not (tmp_path / "staple_performance.csv").exists()
    assert report["confidence_path"] == tmp_path / "fused_confidence.nii.gz"
    assert conf.dtype == np.float32 and conf.min() > 0.0 and conf.max() <= 1.0
    again = patch_fusion(P.read_image(target).data, [w.data for w in report["warped_images"]],
                         [w.data for w in report["warped_labels"]], patch_radius=1, search_radius=1)
    assert np.array_equal(fused, again.labels.cpu().numpy())
    assert np.array_equal(conf, again.confidence.cpu().numpy())
