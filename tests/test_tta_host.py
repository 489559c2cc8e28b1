"""Host checks of the test-time-augmentation oracle, its error bounds and ``flip_sets`` (no GPU).

The float32 restatement of the kernels' operation order must stay inside the bounds of tests/helpers/tta_ref.py
on the very inputs tests/test_tta_gpu.py feeds the kernels, and each gate must reject a planted fault."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import tta_ref as R  # noqa: E402
from loss_ref import ref_dice_ce_loss  # noqa: E402

from segmantic_amd.seg.tta import flip_sets, parse_flips  # noqa: E402


def _exact_tie(scores):
    sc = np.asarray(scores)
    return (sc == sc.max(-1, keepdims=True)).sum(-1) > 1


def check_first_max(got, scores):
    """where several classes share the exact maximum of the scores the first of them is the label"""
    tie = _exact_tie(scores)
    assert tie.any()
    want = np.asarray(scores).argmax(-1)
    assert np.array_equal(np.asarray(got)[tie], want[tie]), "a tie of the maximum did not go to the first class"


# ---------------------------------------------------------------------------- the restatement inside the bounds
@pytest.mark.parametrize("K", R.CLASSES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_f32_restatement_inside_bounds(shape, K):
    M = 8
    lg = R.make_logits(shape, K, R.case_seed(shape, K), M)
    acc64 = R.ref_accumulate(lg, R.ALL_MASKS)
    acc32 = R.f32_accumulate(lg, R.ALL_MASKS)
    R.check_close(acc32, acc64, R.acc_bound(K, M), "accumulator")
    lab64, conf64, ent64, q64 = R.ref_finalize(acc64)
    lab32, conf32, ent32, q32 = R.f32_finalize(acc32)
    pb = R.prob_bound(K, M)
    R.check_close(q32, q64, pb, "probabilities")
    assert np.abs(q32.astype(np.float64).sum(-1) - 1).max() <= K * pb
    R.check_labels(lab32, q64, pb)
    R.check_close(ent32, ent64, R.entropy_bound(K, M), "entropy")
    R.check_close(conf32, np.take_along_axis(q64, lab32[..., None], -1)[..., 0], pb, "confidence")
    assert ent32.min() >= 0 and ent32.max() <= 1


@pytest.mark.parametrize("K", R.CLASSES)
def test_f32_finalize_special_scores(K):
    sc = R.special_scores(K)
    lab64, conf64, ent64, q64 = R.ref_finalize(sc)
    lab32, conf32, ent32, q32 = R.f32_finalize(sc)
    R.check_close(q32, q64, R.finalize_prob_bound(K), "probabilities")
    R.check_close(ent32, ent64, R.finalize_entropy_bound(K), "entropy")
    tie = _exact_tie(sc)
    R.check_labels(lab32[~tie], q64[~tie], R.finalize_prob_bound(K))
    check_first_max(lab32, sc)
    # all-zero voxel, single-class voxels, the uniform voxel
    assert lab32[0] == 0 and conf32[0] == 1 and ent32[0] == 0 and q32[0, 0] == 1 and not q32[0, 1:].any()
    assert list(lab32[1:3]) == [0, K - 1] and np.all(conf32[1:3] == 1) and np.all(ent32[1:3] == 0)
    assert lab32[3] == 0 and abs(float(ent32[3]) - 1) <= R.finalize_entropy_bound(K) and ent32[3] <= 1
    assert lab32[4] == max(0, K - 2) and lab32[5] == 0


# ---------------------------------------------------------------------------- flip_sets
def test_flip_sets_order_and_validation():
    assert flip_sets(3) == [0, 1, 2, 3, 4, 5, 6, 7]
    assert flip_sets(2, "all") == [0, 1, 2, 3]
    assert flip_sets(3, [(), (0,), (2, 1), (0, 1, 2)]) == [0, 1, 6, 7]
    assert flip_sets(3, [(2,)]) == [4]                    # the identity need not be listed
    assert flip_sets(2, [[1], []]) == [2, 0]              # the given order is kept
    for bad in ([(3,)], [(0, 0)], [(0,), (0,)], [], [(-1,)], ["01"], [(0.0,)], [1]):
        with pytest.raises(ValueError):
            flip_sets(3, bad)
    with pytest.raises(ValueError):
        flip_sets(2, [(2,)])
    with pytest.raises(ValueError):
        flip_sets(3, "some")
    with pytest.raises(ValueError):
        flip_sets(4)
    assert parse_flips("all") == "all"
    assert parse_flips("none, 0 ,1+2") == [(), (0,), (1, 2)]


# ---------------------------------------------------------------------------- planted faults
def _fault_case(K=16, shape=(5, 6, 7)):
    lg = R.make_logits(shape, K, R.case_seed(shape, K), 8)
    return lg, R.ref_accumulate(lg, R.ALL_MASKS)


def test_gate_rejects_mirror_off_by_one():
    lg, acc64 = _fault_case()

    def off_by_one(vol, mask):          # u = n - v instead of n - 1 - v on the last mirrored axis (wrapping)
        out = R.unmirror(vol, mask)
        return np.roll(out, 1, axis=2) if mask & 4 else out
    R.check_close(R.f32_accumulate(lg, R.ALL_MASKS), acc64, R.acc_bound(16, 8), "accumulator")
    with pytest.raises(AssertionError):
        R.check_close(R.f32_accumulate(lg, R.ALL_MASKS, mirror=off_by_one), acc64, R.acc_bound(16, 8), "accumulator")


def test_gate_rejects_swapped_axis_bit():
    lg, acc64 = _fault_case()

    def swapped(vol, mask):             # bits 0 and 2 exchanged
        return R.unmirror(vol, (mask & 2) | ((mask & 1) << 2) | ((mask & 4) >> 2))
    with pytest.raises(AssertionError):
        R.check_close(R.f32_accumulate(lg, R.ALL_MASKS, mirror=swapped), acc64, R.acc_bound(16, 8), "accumulator")


def test_gate_rejects_dropped_pass():
    lg, acc64 = _fault_case()
    _, _, _, q64 = R.ref_finalize(acc64)
    _, _, _, q32 = R.f32_finalize(R.f32_accumulate(lg[:7], R.ALL_MASKS[:7]))
    with pytest.raises(AssertionError):
        R.check_close(q32, q64, R.prob_bound(16, 8), "probabilities")


def test_gate_rejects_division_by_pass_count():
    sc = R.special_scores(16)
    _, _, _, q64 = R.ref_finalize(sc)
    _, _, _, q32 = R.f32_finalize(sc, divide_by=np.float32(8))
    with pytest.raises(AssertionError):
        R.check_close(q32, q64, R.finalize_prob_bound(16), "probabilities")


def test_gate_rejects_last_max():
    sc = R.special_scores(16)
    check_first_max(R.f32_finalize(sc)[0], sc)
    with pytest.raises(AssertionError):
        check_first_max(R.f32_finalize(sc, last_max=True)[0], sc)


def test_gate_rejects_unnormalised_entropy():
    sc = R.special_scores(16)
    ent64 = R.ref_finalize(sc)[2]
    with pytest.raises(AssertionError):
        R.check_close(R.f32_finalize(sc, normalise=False)[2], ent64, R.finalize_entropy_bound(16), "entropy")


def test_gate_rejects_wrong_label_away_from_ties():
    lg, acc64 = _fault_case()
    lab64, _, _, q64 = R.ref_finalize(acc64)
    R.check_labels(lab64, q64, R.prob_bound(16, 8))
    bad = lab64.copy()
    bad[2, 3, 4] = (bad[2, 3, 4] + 1) % 16
    with pytest.raises(AssertionError):
        R.check_labels(bad, q64, R.prob_bound(16, 8))


# ---------------------------------------------------------------------------- the oracle against loss_ref
def test_single_pass_softmax_agrees_with_loss_ref():
    K, shape = 3, (5, 6, 7)
    lg = R.make_logits(shape, K, 5, 1)[0].astype(np.float64)
    _, _, _, p = R.ref_mirror_tta([lg], [0])                       # identity flip, M = 1: the plain softmax
    rng = np.random.default_rng(6)
    y = rng.integers(0, K, size=shape)
    logits_t = torch.from_numpy(lg).permute(3, 0, 1, 2)[None]      # [1, K, d, h, w] float64
    labels_t = torch.from_numpy(y)[None, None]
    ce = -np.log(np.take_along_axis(p, y[..., None], -1)[..., 0]).mean()
    assert abs(ce - float(ref_dice_ce_loss(logits_t, labels_t, lambda_dice=0.0, lambda_ce=1.0))) < 1e-12
    t = np.eye(K)[y]
    inter, den = (p * t).sum((0, 1, 2)), t.sum((0, 1, 2)) + p.sum((0, 1, 2))
    dice = (1.0 - (2.0 * inter + 1e-5) / (den + 1e-5)).mean()
    assert abs(dice - float(ref_dice_ce_loss(logits_t, labels_t, lambda_dice=1.0, lambda_ce=0.0))) < 1e-12


def test_label_means_oracle():
    lab = np.array([0, 2, 2, 5, 1, 2], np.uint8)
    val = np.array([0.5, 1.0, 2.0, 9.0, 4.0, 3.0], np.float32)
    sums, counts = R.ref_label_means(lab, val, 4)
    assert list(counts) == [1, 1, 3, 0] and list(sums) == [0.5, 4.0, 6.0, 0.0]
