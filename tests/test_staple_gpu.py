"""STAPLE label fusion on the MI355X against the numpy restatement of its definition (tests/helpers/staple_ref.py,
DESIGN.md section 22).  Every sum is an integer and every float64 operation is rounded on its own on both sides,
so the comparison is exact equality of labels, sums, iterations, converged, prior and posterior * 2^24."""
import csv
import functools
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import staple_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = 1 << 24
SHAPE = (17, 24, 33)                                    # 13 464 voxels: 53 workgroups, the last one ragged
TORCH = {np.uint8: torch.uint8, np.int16: torch.int16, np.int32: torch.int32}


def _ops():
    from segmantic_amd import ops
    return ops


def run(raters, num_classes, **kw):
    ts = [torch.from_numpy(np.array(a)).to(DEV) for a in raters]
    out = _ops().staple(ts, num_classes, return_posterior=True, **kw)
    torch.cuda.synchronize()
    return out


def check(got, ref: R.RefResult, dtype=None):
    labels, sums, prior, it, converged, post = got
    assert (it, converged) == (ref.iterations, ref.converged), (it, converged, ref.iterations, ref.converged)
    assert np.array_equal(prior.cpu().numpy(), ref.prior)
    assert sums.dtype == torch.int64 and np.array_equal(sums.cpu().numpy(), ref.sums)
    want = ref.labels if dtype is None else ref.labels.astype(dtype)
    assert labels.cpu().numpy().dtype == want.dtype and np.array_equal(labels.cpu().numpy(), want)
    assert post.dtype == torch.float32 and tuple(post.shape) == (ref.sums.shape[1],) + tuple(want.shape)
    q = (post.cpu().numpy().astype(np.float64) * Q).reshape(post.shape[0], -1).T
    assert np.array_equal(q, ref.q)


# ---------------------------------------------------------------------------- 1. parity sweep
SWEEP = [(1, 16), (2, 2), (3, 3), (5, 5), (3, 16), (5, 32), (16, 64)]


@functools.lru_cache(maxsize=None)
def sweep_case(r, l):
    _, raters = R.make_raters(SHAPE, l, np.linspace(0.9, 0.5, r), 100 * r + l)
    for a in raters:
        a.setflags(write=False)
    ref = R.staple_ref(raters, l, max_iterations=6, tolerance=0.0)
    return raters, ref


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
@pytest.mark.parametrize("r,l", SWEEP)
def test_parity_sweep(r, l, dtype):
    raters, ref = sweep_case(r, l)
    if (r, l) == (16, 64):                              # R * L * L int64 = 512 KB: no workgroup table
        assert _ops().staple_table_name(r, l) == "global"
    if (r, l) in ((2, 2), (3, 3), (5, 5), (3, 16), (5, 32)):
        assert _ops().staple_table_name(r, l) == "lds"
    check(run([a.astype(dtype) for a in raters], l, max_iterations=6, tolerance=0.0), ref, dtype)


@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("r,l", [(3, 3), (7, 32)])     # the workgroup table and the global one
def test_tiny_volumes(n, r, l):
    _, raters = R.make_raters((1, n), l, np.linspace(0.9, 0.5, r), n)
    check(run(raters, l, max_iterations=6, tolerance=0.0), R.staple_ref(raters, l, max_iterations=6, tolerance=0.0))


# ---------------------------------------------------------------------------- 2. beyond one pass of the grid
def test_more_voxels_than_one_pass_of_the_capped_grid():
    """staple.hip caps its grids at kStapleGridCap = 4096 workgroups of 256 threads, one voxel per thread and
    pass: 1 048 576 voxels.  1 049 576 = that + 1000: the second pass is short and ends inside a wavefront."""
    n = 4096 * 256 + 1000
    _, raters = R.make_raters((8, n // 8), 4, [0.9, 0.8, 0.7], 11)
    assert raters[0].size == n and n % 256 != 0
    check(run(raters, 4, max_iterations=5, tolerance=0.0), R.staple_ref(raters, 4, max_iterations=5, tolerance=0.0))


# ---------------------------------------------------------------------------- 3. mostly agreed input
def test_raters_that_differ_on_a_thin_shell_only():
    """nested balls whose radii the raters draw a little differently: nearly every voxel is agreed and takes the
    count[l] * q_cons[l] shortcut, which must give the integers of the per-voxel sum"""
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in (28, 30, 31)], indexing="ij")
    d = np.sqrt((z - 13.5) ** 2 + (y - 14.2) ** 2 + (x - 15.1) ** 2)
    raters = []
    for k, grow in enumerate([0.0, 0.6, -0.5, 0.3, -0.2]):
        raters.append(((d < 12 + grow).astype(np.uint8) + (d < 8 + grow * (k % 2)) + (d < 4 - grow)).astype(np.uint8))
    D = np.stack(raters).reshape(5, -1)
    agreed = (D == D[0]).all(0).mean()
    assert 0.8 < agreed < 0.99
    ref = R.staple_ref(raters, 4, max_iterations=12, tolerance=0.0)
    check(run(raters, 4, max_iterations=12, tolerance=0.0), ref)
    # all agreed: the passes find nothing to do
    same = [raters[0]] * 3
    check(run(same, 4, max_iterations=3, tolerance=0.0), R.staple_ref(same, 4, max_iterations=3, tolerance=0.0))


# ---------------------------------------------------------------------------- 4. stopping
def test_stops_at_the_iteration_the_reference_stops_at():
    """The iteration count belongs to the drawn volumes.  The prototype that DESIGN.md section 22 grew from took 24
    on a draw that was not kept; seed 0 of make_raters is another draw of the same accuracies, on which the
    reference takes 23, and that is the figure asserted of the reference before the device is asked."""
    _, raters = R.make_raters(SHAPE, 3, [0.9, 0.8, 0.7], 0)
    ref = R.staple_ref(raters, 3)                       # tolerance 1e-5, at most 100 iterations
    assert ref.converged and ref.iterations == 23 and 5 < ref.iterations < 100
    got = run(raters, 3)
    assert got[3] == 23 and got[4] is True
    check(got, ref)
    short = R.staple_ref(raters, 3, max_iterations=5)
    assert (short.iterations, short.converged) == (5, False)
    got = run(raters, 3, max_iterations=5)
    assert got[3] == 5 and got[4] is False
    check(got, short)


# ---------------------------------------------------------------------------- 5. not the vote
def test_fusion_is_not_the_vote_and_is_nearer_the_truth():
    ops = _ops()
    truth, raters = R.make_raters(SHAPE, 2, [0.97, 0.6, 0.6, 0.6, 0.6], 1)
    ref = R.staple_ref(raters, 2, max_iterations=50, tolerance=0.0)
    vote = R.vote(np.stack(raters).reshape(5, -1).astype(np.int64), 2).reshape(SHAPE)
    differ, acc_fused, acc_vote = int((ref.labels != vote).sum()), float((ref.labels == truth).mean()), float((vote == truth).mean())
    print(f"reference: differs from the vote on {differ} voxels, agrees with the truth on {acc_fused:.4f} (vote {acc_vote:.4f})")
    assert differ > 1000 and acc_fused > acc_vote and (differ, round(acc_fused, 3), round(acc_vote, 3)) == (2546, 0.971, 0.81)
    got = run(raters, 2, max_iterations=50, tolerance=0.0)
    check(got, ref)
    ts = [torch.from_numpy(a.astype(np.int32)).to(DEV) for a in raters]
    dev_vote = torch.empty_like(ts[0])
    ops.ensemble_vote(ts, dev_vote)
    torch.cuda.synchronize()
    assert np.array_equal(dev_vote.cpu().numpy(), vote)
    fused = got[0].cpu().numpy()
    assert int((fused != dev_vote.cpu().numpy()).sum()) > 1000
    assert (fused == truth).sum() > (dev_vote.cpu().numpy() == truth).sum()


# ---------------------------------------------------------------------------- 6. prior, absent labels, posterior
def test_custom_prior_absent_labels_and_posterior():
    _, raters = R.make_raters(SHAPE, 16, [0.9, 0.7, 0.6], 7, truth_labels=range(0, 16, 2))
    raters = [np.where(a % 2 == 1, (a + 1) % 16, a).astype(np.uint8) for a in raters]      # even labels only
    prior = np.linspace(1.0, 2.5, 16)                   # not normalised: used as given
    for kw in (dict(prior=prior), dict()):
        ref = R.staple_ref(raters, 16, max_iterations=8, tolerance=0.0, **kw)
        got = run(raters, 16, max_iterations=8, tolerance=0.0, **kw)
        check(got, ref)
        labels, post = got[0].cpu().numpy(), got[5].cpu().numpy()
        assert not (labels % 2).any() and not post[1::2].any()
        assert np.array_equal(np.argmax(post, axis=0), labels)                              # first maximum
        assert not got[1].cpu().numpy()[:, 1::2, :].any() and not got[1].cpu().numpy()[:, :, 1::2].any()


def test_the_products_are_taken_in_ascending_rater_order():
    """a prior of subnormal size (used as given) makes every product round to a multiple of 2^-1074, so the
    order of the factors shows in q; the reference with descending order differs (tests/test_staple_host.py)"""
    _, raters = R.make_raters(SHAPE, 3, [0.8, 0.7, 0.6, 0.6], 3)
    prior = [3000000001 * 5e-324, 2000000003 * 5e-324, 4000000007 * 5e-324]
    ref = R.staple_ref(raters, 3, max_iterations=3, tolerance=0.0, prior=prior)
    assert not np.array_equal(ref.sums, R.staple_ref(raters, 3, max_iterations=3, tolerance=0.0, prior=prior,
                                                     fault="descending").sums)
    check(run(raters, 3, max_iterations=3, tolerance=0.0, prior=prior), ref)


def test_a_voxel_whose_products_all_underflow_is_dropped():
    """under a given prior of the smallest subnormal every product of a disputed voxel rounds to 0 (with two labels
    some rater's theta is below 1/2 for either): the passes, the table kernel and the final pass drop the voxel as
    the definition says (q = 0, nothing added to S, label 0) and the agreed voxels keep q = Q"""
    _, raters = R.make_raters(SHAPE, 2, [0.9, 0.8, 0.7], 5)
    prior = [5e-324, 5e-324]
    ref = R.staple_ref(raters, 2, max_iterations=4, tolerance=0.0, prior=prior)
    D = np.stack(raters).reshape(3, -1)
    disputed = ~(D == D[0]).all(0)
    assert 0.3 < disputed.mean() < 0.7 and not ref.q[disputed].any() and ref.q[~disputed].sum() == int((~disputed).sum()) * Q
    got = run(raters, 2, max_iterations=4, tolerance=0.0, prior=prior)
    check(got, ref)
    assert not got[5].cpu().numpy().reshape(2, -1)[:, disputed].any()


# ---------------------------------------------------------------------------- 7. labels outside the range
@pytest.mark.parametrize("dtype,bad", [(np.uint8, 5), (np.int16, 5), (np.int32, -1), (np.int16, -7), (np.int32, 1 << 20)])
def test_a_label_outside_the_range_raises_and_faults_nothing(dtype, bad):
    _, raters = R.make_raters(SHAPE, 5, [0.9, 0.8, 0.7, 0.6], 9, dtype=dtype)
    ref = R.staple_ref(raters, 5, max_iterations=4, tolerance=0.0)
    broken = [a.copy() for a in raters]
    broken[2].reshape(-1)[[77, 9001]] = bad
    with pytest.raises(ValueError, match=rf"rater 2 .*label {bad}\b"):
        run(broken, 5, max_iterations=4, tolerance=0.0)
    check(run(raters, 5, max_iterations=4, tolerance=0.0), ref, dtype)          # the next call on the stream is sound


# ---------------------------------------------------------------------------- 8. repeatability and validation
def test_repeated_calls_give_identical_bits_and_bad_tensors_are_refused():
    ops = _ops()
    raters, ref = sweep_case(5, 32)
    a, b = run(raters, 32, max_iterations=6, tolerance=0.0), run(raters, 32, max_iterations=6, tolerance=0.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
    check(a, ref)
    t = torch.zeros((6, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        ops.staple([t, t.t().contiguous().t()], 2)
    with pytest.raises(ValueError, match=r"labels\[1\]"):
        ops.staple([t, t.to(torch.int16)], 2)
    with pytest.raises(ValueError, match=r"labels\[1\]"):
        ops.staple([t, t[:5].contiguous()], 2)
    with pytest.raises(ValueError, match="uint8, int16 or int32"):
        ops.staple([t.long(), t.long()], 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.staple([t, t.cpu()], 2)
    out = ops.staple([t, t], 2)                          # without the posterior: five results
    assert len(out) == 5 and out[3] == 1 and out[4] is True and not out[0].any()


def test_staple_accepts_arrays_tensors_and_images():
    from segmantic_amd.image.processing import Image
    from segmantic_amd.seg.staple import staple
    _, raters = R.make_raters((9, 10, 11), 4, [0.9, 0.8, 0.7], 4, dtype=np.int16)
    ref = R.staple_ref(raters, 4, max_iterations=7)
    res = staple(raters, max_iterations=7, return_posterior=True)                          # num_classes from the data
    assert isinstance(res.labels, np.ndarray) and res.labels.dtype == np.int16 and np.array_equal(res.labels, ref.labels)
    assert np.array_equal(res.sums, ref.sums) and np.array_equal(res.confusion, ref.theta) and res.iterations == ref.iterations
    assert np.array_equal(res.posterior, ref.posterior) and res.converged == ref.converged
    img = staple([Image(a, [1, 2, 3]) for a in raters], 4, max_iterations=7)
    assert isinstance(img.labels, Image) and img.labels.spacing == (1.0, 2.0, 3.0)
    assert np.array_equal(img.labels.numpy(), ref.labels) and img.posterior is None
    two_d = staple([torch.from_numpy(a[0].astype(np.int64)) for a in raters], 4, max_iterations=7)   # int64 is narrowed
    assert two_d.labels.dtype == torch.int64 and not two_d.labels.is_cuda
    assert np.array_equal(two_d.labels.numpy(), R.staple_ref([a[0] for a in raters], 4, max_iterations=7).labels)


# ---------------------------------------------------------------------------- 9. ensemble_creator
def test_ensemble_creator_in_staple_mode(tmp_path):
    from segmantic_amd.data.nifti import read_nifti, write_nifti
    from segmantic_amd.seg import staple as S
    from segmantic_amd.seg.inferers import SlidingWindowInferer
    from segmantic_amd.seg.monai_unet import Net, _argmax_labels, ensemble_creator
    from segmantic_amd.seg.pipeline import PredictPipeline
    from segmantic_amd.utils import config
    ops = _ops()
    ckpts = []
    for seed in (4, 5, 6):
        torch.manual_seed(seed)
        net = Net(num_classes=3, spatial_dims=3, channels=(4, 8), strides=(2,), spatial_size=[16, 16, 16]).to(DEV).eval()
        ckpts.append(tmp_path / f"epoch={seed}-val_loss=0.5-val_dice=0.{seed}.ckpt")
        net.save_checkpoint(ckpts[-1], epoch=seed)
    g = torch.Generator().manual_seed(13)
    images = []
    for i, size in enumerate([(22, 20, 19), (20, 21, 18)]):
        vol = torch.randn(size, generator=g).numpy() * 50 + 100
        write_nifti(tmp_path / f"c{i}.nii.gz", vol.astype(np.float32).transpose(2, 1, 0), np.eye(4))
        images.append(tmp_path / f"c{i}.nii.gz")
    tissues = {"bg": 0, "a": 1, "b": 2}
    out = tmp_path / "fused"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        saved = ensemble_creator(model_files=ckpts, test_images=images, output_dir=out, tissue_dict=tissues,
                                 combination_mode="staple", staple_iterations=20, save_candidates=tmp_path / "cand.yml",
                                 gpu_ids=[0])
    assert [p.name for p in saved] == ["c0.nii.gz", "c1.nii.gz"]
    models = [Net.load_from_checkpoint(str(p)).to(DEV).eval() for p in ckpts]
    pipe = PredictPipeline(device=torch.device(DEV))
    inferer = SlidingWindowInferer(roi_size=(96, 96, 96), sw_batch_size=4, overlap=0.5)
    pooled = np.zeros((3, 3, 3), np.int64)
    with torch.no_grad():
        for i, img in enumerate(images):
            item = pipe.load(img)
            labs = [_argmax_labels(inferer(item["image"][None], m))[0, 0].contiguous() for m in models]
            fused, sums = ops.staple(labs, 3, max_iterations=20)[:2]
            pooled += sums.cpu().numpy()
            got, _ = read_nifti(out / f"c{i}.nii.gz")
            assert tuple(fused.shape) == tuple(item["shape0"])                             # no spacing, nothing cropped
            assert np.array_equal(got, fused.cpu().numpy().transpose(2, 1, 0).astype(got.dtype))
    rows = list(csv.DictReader(open(out / "staple_performance.csv")))
    want = S.performance_table(pooled, [p.name for p in ckpts], tissues)
    assert len(rows) == len(want) == 9
    for a, b in zip(rows, want):
        assert a["rater"] == b["rater"] and int(a["label"]) == b["label"] and a["tissue"] == b["tissue"]
        for k in ("sensitivity", "ppv", "voxels"):
            assert a[k] == repr(b[k])
    cand = config.load(tmp_path / "cand.yml")
    assert cand == S.best_candidates(pooled, tissues) and cand
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = ensemble_creator(model_files=ckpts, test_images=images[:1], output_dir=tmp_path / "best",
                                 tissue_dict=tissues, combination_mode="select_best",
                                 candidate_per_tissue_path=tmp_path / "cand.yml", gpu_ids=[0])
    assert len(again) == 1 and again[0].exists()


# ---------------------------------------------------------------------------- the file tool
def test_label_fusion_script_on_files(tmp_path):
    import importlib.util

    from segmantic_amd.image.processing import Image, read_image, write_image
    spec = importlib.util.spec_from_file_location("staple_labels", Path(__file__).resolve().parent.parent / "scripts" / "staple_labels.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, raters = R.make_raters((9, 10, 11), 3, [0.9, 0.8, 0.7], 21)
    paths = []
    for i, a in enumerate(raters):
        paths.append(tmp_path / f"rater{i}.nii.gz")
        write_image(Image(a, [0.5, 0.6, 0.7], [1.0, 2.0, 3.0]), paths[-1])
    (tmp_path / "tissues.txt").write_text("V7\nN2\nC0.0 0.0 1.0 0.5 A\nC0.0 1.0 0.0 0.5 B\n")
    tool.main(tmp_path / "out" / "fused.nii.gz", paths, tmp_path / "tissues.txt", 30, 1e-5, tmp_path / "perf.csv")
    ref = R.staple_ref(raters, 3, max_iterations=30)
    fused = read_image(tmp_path / "out" / "fused.nii.gz")
    assert np.array_equal(fused.numpy(), ref.labels) and fused.numpy().dtype == np.uint8
    assert np.allclose(fused.spacing, [0.5, 0.6, 0.7]) and np.allclose(fused.origin, [1.0, 2.0, 3.0])
    rows = list(csv.DictReader(open(tmp_path / "perf.csv")))
    assert len(rows) == 9 and rows[4]["rater"] == "rater1.nii.gz" and rows[4]["tissue"] == "A"
    write_image(Image(raters[1], [0.5, 0.6, 0.8], [1.0, 2.0, 3.0]), tmp_path / "other.nii.gz")
    with pytest.raises(ValueError, match=r"other\.nii\.gz: spacing"):
        tool.main(tmp_path / "o.nii.gz", [paths[0], tmp_path / "other.nii.gz"], None, 30, 1e-5, None)
    write_image(Image(raters[1][:, :, :10].copy(), [0.5, 0.6, 0.7], [1.0, 2.0, 3.0]), tmp_path / "small.nii.gz")
    with pytest.raises(ValueError, match=r"small\.nii\.gz: size"):
        tool.main(tmp_path / "o.nii.gz", [paths[0], tmp_path / "small.nii.gz"], None, 30, 1e-5, None)
