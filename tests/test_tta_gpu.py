"""Mirror test-time augmentation on the GPU: the three kernels against the float64 oracle of
tests/helpers/tta_ref.py (bounds derived there), repeatability, un-mirroring checked without the oracle, the
driver end to end (3-D and 2-D) and ``predict(tta=..., save_uncertainty=...)``."""
import csv
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import tta_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from segmantic_amd import ops
    return ops


def _view(arr: np.ndarray, pad: int) -> torch.Tensor:
    """[..., K] float32 -> NDHWC device tensor [1, d, h, w, K] that is a view into rows of K + pad floats"""
    a = torch.from_numpy(np.ascontiguousarray(arr, np.float32)).to(DEV)
    while a.dim() < 5:
        a = a[None]
    if pad == 0:
        return a
    big = torch.full(tuple(a.shape[:4]) + (a.shape[4] + pad,), float("nan"), dtype=torch.float32, device=DEV)
    big[..., :a.shape[4]] = a
    return big[..., :a.shape[4]]


def _accumulate(lg, masks, pad=0):
    ops = _ops()
    acc = torch.empty(lg[0].shape, dtype=torch.float32, device=DEV)
    for i, (l, m) in enumerate(zip(lg, masks)):
        ops.tta_accumulate(_view(l, pad), m, acc, first=(i == 0))
    return acc


def _finalize(scores: torch.Tensor, probs="new", label_dtype=torch.uint8, maps=True):
    """scores NDHWC -> (labels, confidence, entropy, probs) numpy"""
    ops = _ops()
    vox = tuple(scores.shape[:4])
    lab = torch.empty(vox, dtype=label_dtype, device=DEV)
    conf = torch.empty(vox, dtype=torch.float32, device=DEV) if maps else None
    ent = torch.empty(vox, dtype=torch.float32, device=DEV) if maps else None
    out = None
    if probs == "new":
        out = torch.empty(tuple(scores.shape), dtype=torch.float32, device=DEV)
    elif probs == "alias":
        out = scores
    ops.tta_finalize(scores, lab, conf, ent, probs_out=out)
    torch.cuda.synchronize()
    return (lab.cpu().numpy(), None if conf is None else conf.cpu().numpy(),
            None if ent is None else ent.cpu().numpy(), None if out is None else out.cpu().numpy())


# ---------------------------------------------------------------------------- kernels against the oracle
@pytest.mark.parametrize("K", R.CLASSES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_accumulate_and_finalize_against_the_oracle(shape, K):
    M = 8
    lg = R.make_logits(shape, K, R.case_seed(shape, K), M)
    acc64 = R.ref_accumulate(lg, R.ALL_MASKS)
    lab64, conf64, ent64, q64 = R.ref_finalize(acc64)
    pb = R.prob_bound(K, M)
    first = None
    for pad in (0, 4, 3):               # dense rows, wider aligned rows, rows off the 16-byte grid
        acc = _accumulate(lg, R.ALL_MASKS, pad)
        got = acc.cpu().numpy()
        R.check_close(got, acc64, R.acc_bound(K, M), f"accumulator (ld = K + {pad})")
        if first is None:
            first = got
        else:                           # every layout adds the same numbers in the same order
            assert np.array_equal(got, first)
    for probs in ("new", "alias"):
        lab, conf, ent, q = _finalize(acc.clone()[None], probs=probs, label_dtype=torch.uint8 if probs == "new" else torch.int32)
        R.check_close(q[0], q64, pb, "probabilities")
        assert np.abs(q[0].astype(np.float64).sum(-1) - 1).max() <= K * pb
        R.check_labels(lab[0], q64, pb)
        R.check_close(ent[0], ent64, R.entropy_bound(K, M), "entropy")
        R.check_close(conf[0], np.take_along_axis(q64, lab[0].astype(np.int64)[..., None], -1)[..., 0], pb, "confidence")
        assert ent.min() >= 0 and ent.max() <= 1


@pytest.mark.parametrize("K", R.CLASSES)
def test_each_mask_alone_lands_on_the_unmirrored_voxel(K):
    shape = (5, 6, 7)
    lg = R.make_logits(shape, K, 31 + K, 1)
    for m in R.ALL_MASKS:
        got = _accumulate(lg, [m]).cpu().numpy()
        R.check_close(got, R.ref_accumulate(lg, [m]), R.acc_bound(K, 1), f"mask {m}")


@pytest.mark.parametrize("K", R.CLASSES)
def test_finalize_special_scores(K):
    sc = R.special_scores(K)
    lab64, conf64, ent64, q64 = R.ref_finalize(sc)
    tie = (sc == sc.max(-1, keepdims=True)).sum(-1) > 1
    for pad, probs in ((0, "new"), (0, "alias"), (4, "alias"), (3, "new"), (0, None)):
        lab, conf, ent, q = _finalize(_view(sc, pad), probs=probs)
        lab, conf, ent = lab.reshape(-1), conf.reshape(-1), ent.reshape(-1)
        if q is not None:
            q = q.reshape(-1, K)
            R.check_close(q, q64, R.finalize_prob_bound(K), "probabilities")
            assert q[0, 0] == 1 and not q[0, 1:].any()
        R.check_close(ent, ent64, R.finalize_entropy_bound(K), "entropy")
        R.check_close(conf, conf64, R.finalize_prob_bound(K), "confidence")
        R.check_labels(lab[~tie], q64[~tie], R.finalize_prob_bound(K))
        assert np.array_equal(lab[tie], sc.argmax(-1)[tie])               # exact ties: the first class wins
        assert lab[0] == 0 and conf[0] == 1 and ent[0] == 0               # all-zero voxel
        assert list(lab[1:3]) == [0, K - 1] and np.all(conf[1:3] == 1) and np.all(ent[1:3] == 0)
        assert lab[3] == 0 and ent[3] <= 1 and 1 - float(ent[3]) <= R.finalize_entropy_bound(K)
        assert lab[4] == max(0, K - 2) and lab[5] == 0
    lab_only = _finalize(_view(sc, 0), probs=None, maps=False)[0].reshape(-1)
    assert np.array_equal(lab_only, lab)


def test_finalize_refuses_what_it_cannot_hold():
    ops = _ops()
    sc = torch.rand((1, 1, 2, 3, 300), device=DEV)
    with pytest.raises(RuntimeError):
        ops.tta_finalize(sc, torch.empty((1, 1, 2, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.tta_finalize(sc, torch.empty((1, 1, 2, 3), dtype=torch.int16, device=DEV))
    with pytest.raises(RuntimeError):
        ops.tta_accumulate(torch.rand((1, 2, 2, 2, 1), device=DEV), 0, torch.empty((2, 2, 2, 1), device=DEV), True)
    with pytest.raises(RuntimeError):
        ops.tta_accumulate(torch.rand((1, 2, 2, 2, 4), device=DEV), 8, torch.empty((2, 2, 2, 4), device=DEV), True)


@pytest.fixture(scope="module")
def ragged():
    """one volume past every capped grid (8192 workgroups of 256 lanes): 130 x 128 x 129 voxels, 2 classes"""
    shape, K = (130, 128, 129), 2
    lg = R.make_logits(shape, K, 9, 2)
    masks = [7, 0]
    acc = _accumulate(lg, masks)
    lab, conf, ent, q = _finalize(acc[None])
    return dict(K=K, lg=lg, masks=masks, acc=acc, lab=lab[0], conf=conf[0], ent=ent[0], q=q[0])


def test_ragged_volume_beyond_the_grid_caps(ragged):
    K, M = ragged["K"], 2
    acc64 = R.ref_accumulate(ragged["lg"], ragged["masks"])
    R.check_close(ragged["acc"].cpu().numpy(), acc64, R.acc_bound(K, M), "accumulator")
    lab64, conf64, ent64, q64 = R.ref_finalize(acc64)
    R.check_close(ragged["q"], q64, R.prob_bound(K, M), "probabilities")
    R.check_labels(ragged["lab"], q64, R.prob_bound(K, M))
    R.check_close(ragged["ent"], ent64, R.entropy_bound(K, M), "entropy")


# ---------------------------------------------------------------------------- repeatability, label means
def test_repeated_calls_are_bit_identical(ragged):
    ops = _ops()
    acc2 = _accumulate(ragged["lg"], ragged["masks"])
    assert torch.equal(acc2, ragged["acc"])
    lab, conf, ent, q = _finalize(acc2[None])
    for a, b in ((lab[0], ragged["lab"]), (conf[0], ragged["conf"]), (ent[0], ragged["ent"]), (q[0], ragged["q"])):
        assert np.array_equal(a, b)
    labels = torch.from_numpy(ragged["lab"]).to(DEV)
    ent_d = torch.from_numpy(ragged["ent"]).to(DEV)
    s1, c1 = ops.label_means(labels, ent_d, 2)
    s2, c2 = ops.label_means(labels, ent_d, 2)
    torch.cuda.synchronize()
    assert torch.equal(s1, s2) and torch.equal(c1, c2)


@pytest.mark.parametrize("k,dtype,n", [(2, torch.uint8, 130 * 128 * 129), (17, torch.int32, 40 * 33 * 35),
                                       (300, torch.int32, 70001), (512, torch.int32, 999), (5, torch.uint8, 63)])
def test_label_means_against_the_oracle(k, dtype, n):
    ops = _ops()
    rng = np.random.default_rng(k)
    runs = rng.integers(1, 200, size=n // 50 + 2)                       # label runs, as in a segmentation
    lab = np.repeat(rng.integers(0, k + (3 if k < 250 else 0), size=runs.size), runs)[:n]
    lab[rng.random(n) < 0.05] = rng.integers(0, k)                      # and isolated voxels
    if k > 3:
        lab[lab == 3] = 2                                               # an absent label
    val = rng.random(n).astype(np.float32)
    lab_np = lab.astype(np.uint8 if dtype == torch.uint8 else np.int32)
    sums, counts = ops.label_means(torch.from_numpy(lab_np).to(DEV), torch.from_numpy(val).to(DEV), k)
    s2, c2 = ops.label_means(torch.from_numpy(lab_np).to(DEV), torch.from_numpy(val).to(DEV), k)
    torch.cuda.synchronize()
    assert torch.equal(sums, s2) and torch.equal(counts, c2)
    rs, rc = R.ref_label_means(lab_np, val, k)
    assert np.array_equal(counts.cpu().numpy(), rc) and int(rc.sum()) == int((lab_np < k).sum())
    got = sums.cpu().numpy()
    assert np.all(np.abs(got - rs) <= 1e-12 * np.abs(rs))
    if k > 3:
        assert rc[3] == 0 and got[3] == 0


def test_uncertainty_summary_marks_absent_labels():
    from segmantic_amd.seg.tta import uncertainty_summary
    lab = torch.tensor([0, 0, 2, 2, 2], dtype=torch.uint8, device=DEV)
    ent = torch.tensor([0.5, 0.25, 1.0, 0.0, 0.5], device=DEV)
    conf = torch.tensor([1.0, 0.5, 0.25, 0.25, 0.25], device=DEV)
    s = uncertainty_summary(lab, ent, conf, 4)
    assert list(s["voxels"]) == [2, 0, 3, 0]
    assert s["mean_entropy"][0] == 0.375 and s["mean_entropy"][2] == 0.5 and s["mean_confidence"][2] == 0.25
    assert np.isnan(s["mean_entropy"][[1, 3]]).all() and np.isnan(s["mean_confidence"][[1, 3]]).all()


# ---------------------------------------------------------------------------- un-mirroring, without the oracle
def _voxel_map(x: torch.Tensor) -> torch.Tensor:
    """a foreign, position-independent predictor: [b, 1, *roi] -> [b, 3, *roi], a fixed map of the intensity"""
    return torch.cat([x * 1.5, x * -0.75 + 0.25, x * x * 0.5 - 1.0], dim=1)


def test_unmirroring_with_a_position_independent_predictor():
    """Whatever the mirroring, a per-voxel map gives every voxel the same logits in every pass (the constant
    blend of 1, 2, 4 or 8 equal values is exact), so the TTA probabilities must equal the softmax of the map at
    the voxel itself: an un-mirroring slip would pair a voxel with another voxel's intensity."""
    from segmantic_amd.seg.tta import mirror_tta_inference
    g = torch.Generator().manual_seed(11)
    x = (torch.randn((1, 1, 20, 18, 17), generator=g) * 2).to(DEV)
    res = mirror_tta_inference(x, (16, 16, 16), 2, _voxel_map)
    assert res.passes == 8 and tuple(res.probs.shape) == (1, 3, 20, 18, 17)
    want = torch.softmax(_voxel_map(x).double().cpu(), dim=1).numpy()
    R.check_close(res.probs.cpu().numpy(), want, R.prob_bound(3, 8), "probabilities")
    one = mirror_tta_inference(x, (16, 16, 16), 2, _voxel_map, flips=[()])
    assert one.passes == 1
    R.check_close(one.probs.cpu().numpy(), want, R.prob_bound(3, 1), "single pass")
    assert np.abs(res.probs.sum(1).cpu().numpy() - 1).max() <= 3 * R.prob_bound(3, 8)


# ---------------------------------------------------------------------------- end to end
def _tiny_net(spatial_dims=3):
    from segmantic_amd.seg.monai_unet import Net
    torch.manual_seed(4)
    roi = [16] * spatial_dims
    net = Net(num_classes=3, spatial_dims=spatial_dims, channels=(4, 8), strides=(2,), spatial_size=roi)
    return net.to(DEV).eval()


@pytest.mark.parametrize("spatial_dims,size", [(3, (20, 18, 17)), (2, (18, 17))])
def test_mirror_tta_inference_against_the_oracle(spatial_dims, size):
    from segmantic_amd.seg.inferers import sliding_window_inference
    from segmantic_amd.seg.tta import flip_sets, mirror_tta_inference
    net = _tiny_net(spatial_dims)
    g = torch.Generator().manual_seed(12)
    # The input scale makes the untrained network spread a voxel's logits over a unit or so, as a trained one does.
    # Far below it the three probabilities stay within 0.01 of 1/3 and near-ties abound; far above it every pass is
    # one-hot and the mean over M passes ties at multiples of 1 / M.  (The 3-D net answers a unit of input with
    # logits of the order of 0.01, the 2-D one with 1.)
    x = (torch.randn((1, 1) + size, generator=g) * {3: 100.0, 2: 3.0}[spatial_dims]).to(DEV)
    roi = (16,) * spatial_dims
    masks = flip_sets(spatial_dims)
    with torch.no_grad():
        res = mirror_tta_inference(x, roi, 4, net, overlap=0.25)
        passes = []
        for m in masks:
            dims = [2 + a for a in range(spatial_dims) if m & (1 << a)]
            lg = sliding_window_inference(torch.flip(x, dims) if dims else x, roi, 4, net, overlap=0.25)
            lg = lg[0].float().cpu().numpy()                              # [K, *size]
            if spatial_dims == 2:
                lg = lg[:, None]
            passes.append(np.moveaxis(lg, 0, -1))
    M = len(masks)
    assert res.passes == M == (1 << spatial_dims)
    shift = 3 - spatial_dims
    lab64, conf64, ent64, q64 = R.ref_mirror_tta(passes, [m << shift for m in masks])

    def nd(t):                                                            # [1, C, *size] -> [d, h, w, (C)]
        a = t[0].cpu().numpy()
        if spatial_dims == 2:
            a = a[:, None]
        return np.moveaxis(a, 0, -1)
    pb = R.prob_bound(3, M)
    assert tuple(res.probs.shape) == (1, 3) + size and tuple(res.labels.shape) == (1, 1) + size
    R.check_close(nd(res.probs), q64, pb, "probabilities")
    R.check_labels(nd(res.labels)[..., 0], q64, pb)
    R.check_close(nd(res.entropy)[..., 0], ent64, R.entropy_bound(3, M), "entropy")
    R.check_close(nd(res.confidence)[..., 0],
                  np.take_along_axis(q64, nd(res.labels).astype(np.int64), -1)[..., 0], pb, "confidence")


# ---------------------------------------------------------------------------- predict
def test_predict_with_tta_and_uncertainty(tmp_path):
    from segmantic_amd.data.nifti import read_nifti, write_nifti
    from segmantic_amd.seg.inferers import SlidingWindowInferer
    from segmantic_amd.seg.monai_unet import predict
    from segmantic_amd.seg.pipeline import PredictPipeline
    from segmantic_amd.seg.tta import mirror_tta_inference
    ops = _ops()
    net = _tiny_net()
    ckpt = tmp_path / "m.ckpt"
    net.save_checkpoint(ckpt, epoch=0)
    g = torch.Generator().manual_seed(13)
    images = []
    for i, size in enumerate([(22, 20, 19), (20, 21, 18)]):
        vol = torch.randn(size, generator=g).numpy() * 50 + 100
        vol[:2] = 0                                                       # a border the foreground crop removes
        vol[:, :, -1] = 0
        A = np.diag([-1.0, 1.0, 1.0, 1.0]) if i else np.eye(4)            # the second case needs re-orientation
        write_nifti(tmp_path / f"c{i}.nii.gz", vol.astype(np.float32).transpose(2, 1, 0), A)
        images.append(tmp_path / f"c{i}.nii.gz")
    kw = dict(model_file=ckpt, test_images=images, tissue_dict={"bg": 0, "a": 1, "b": 2})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        predict(output_dir=tmp_path / "plain", **kw)
        predict(output_dir=tmp_path / "tta", tta=True, save_uncertainty=True, **kw)
        predict(output_dir=tmp_path / "unc", save_uncertainty=True, **kw)
    pipe = PredictPipeline(device=torch.device(DEV))
    inferer = SlidingWindowInferer(roi_size=[16, 16, 16], sw_batch_size=4, device=torch.device(DEV))
    rows = list(csv.DictReader(open(tmp_path / "tta" / "uncertainty.csv")))
    assert list(rows[0].keys()) == ["case", "label", "name", "voxels", "mean_entropy", "mean_confidence"]
    assert len(rows) == 2 * 3 and [r["name"] for r in rows[:3]] == ["bg", "a", "b"]
    assert not (tmp_path / "plain" / "uncertainty.csv").exists()
    for i, img in enumerate(images):
        with torch.no_grad():
            item = pipe.load(img)
            # both options off: the file is the one today's code path writes
            want = pipe.invert_and_discretize(inferer(item["image"][None], net)[0], item).cpu().numpy().transpose(2, 1, 0)
            plain, _ = read_nifti(tmp_path / "plain" / f"c{i}.nii.gz")
            assert plain.dtype == want.dtype and np.array_equal(plain, want)
            assert not (tmp_path / "plain" / f"c{i}_entropy.nii.gz").exists()
            # tta: labels = first maximum of the returned probabilities carried through invert_scores
            res = mirror_tta_inference(item["image"][None], [16, 16, 16], 4, net)
            scores = pipe.invert_scores(res.probs[0], item)
            assert tuple(scores.shape) == (1,) + tuple(item["shape0"]) + (3,)
            lab = torch.empty(scores.shape[1:4], dtype=torch.int32, device=DEV)
            ops.argmax(scores, lab)
        saved, aff = read_nifti(tmp_path / "tta" / f"c{i}.nii.gz")
        assert np.array_equal(saved, lab.cpu().numpy().transpose(2, 1, 0)) and saved.dtype == np.uint8
        ent, aff_e = read_nifti(tmp_path / "tta" / f"c{i}_entropy.nii.gz")
        conf, _ = read_nifti(tmp_path / "tta" / f"c{i}_confidence.nii.gz")
        src, aff_s = read_nifti(img)
        assert ent.dtype == np.float32 and conf.dtype == np.float32 and ent.shape == conf.shape == src.shape
        assert np.allclose(aff_e, aff_s) and np.allclose(aff, aff_s)
        assert ent.min() >= 0 and ent.max() <= 1 and conf.min() >= 1 / 3 - 1e-6 and conf.max() <= 1
        # outside the crop: background, certain
        outside = (scores.sum(-1)[0] == 0).cpu().numpy().transpose(2, 1, 0)
        assert outside.any() and not saved[outside].any() and np.all(ent[outside] == 0) and np.all(conf[outside] == 1)
        case = [r for r in rows if r["case"] == img.name]
        assert [int(r["label"]) for r in case] == [0, 1, 2]
        assert sum(int(r["voxels"]) for r in case) == src.size
        for r in case:
            sel = saved == int(r["label"])
            assert int(r["voxels"]) == int(sel.sum())
            if sel.any():
                assert abs(float(r["mean_entropy"]) - float(ent[sel].astype(np.float64).mean())) < 1e-9
                assert abs(float(r["mean_confidence"]) - float(conf[sel].astype(np.float64).mean())) < 1e-9
            else:
                assert r["mean_entropy"] == "nan"
        # save_uncertainty alone: the identity pass
        one, _ = read_nifti(tmp_path / "unc" / f"c{i}.nii.gz")
        with torch.no_grad():
            r1 = mirror_tta_inference(item["image"][None], [16, 16, 16], 4, net, flips=[()])
            l1 = torch.empty(scores.shape[1:4], dtype=torch.int32, device=DEV)
            ops.argmax(pipe.invert_scores(r1.probs[0], item), l1)
        assert np.array_equal(one, l1.cpu().numpy().transpose(2, 1, 0))
        assert (tmp_path / "unc" / f"c{i}_entropy.nii.gz").exists()
