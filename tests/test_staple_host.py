"""STAPLE label fusion without a GPU: the numpy restatement of the definition on cases
worked by hand, the properties the definition implies, the seeded faults that the exact comparison of the GPU
tests must reject, the performance table / candidate list, and the argument checks."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import staple_ref as R  # noqa: E402

Q = 1 << 24
SHAPE = (17, 24, 33)


def same(a: R.RefResult, b: R.RefResult) -> bool:
    """the comparison of the GPU tests: exact equality of every returned quantity"""
    return (np.array_equal(a.labels, b.labels) and np.array_equal(a.sums, b.sums) and a.iterations == b.iterations
            and a.converged == b.converged and np.array_equal(a.prior, b.prior) and np.array_equal(a.q, b.q))


# ---------------------------------------------------------------------------- the reference itself
def test_reference_on_a_hand_worked_case():
    """R = 3, L = 2, four voxels.  Votes 0 1 1 1; the start M-step gives every rater S = [[Q, Q], [0, 2Q]], so
    T = [Q, 3Q] and theta_r = [[1, 1/3], [0, 2/3]]; prior = [1/2, 1/2].  Voxel 0 (0, 0, 0): p = [1/2, 1/2 * (1/3)^3]
    = [1/2, 1/54], W = [27/28, 1/28].  The other voxels have a rater that says 1, theta_r[1][0] = 0: W = [0, 1]."""
    D = [np.array([[0, 0], [1, 1]], np.uint8), np.array([[0, 1], [1, 0]], np.uint8), np.array([[0, 1], [0, 1]], np.uint8)]
    r = R.staple_ref(D, 2, max_iterations=1)
    assert np.array_equal(r.prior, [0.5, 0.5])
    q0 = [16178030, 599186]                              # round(27 Q / 28), round(Q / 28)
    assert q0 == [math.floor(27 * Q / 28 + 0.5), math.floor(Q / 28 + 0.5)] and sum(q0) == Q
    assert r.q.tolist() == [q0, [0, Q], [0, Q], [0, Q]]
    S = [[q0[0], q0[1] + Q], [0, 2 * Q]]                 # every rater says 0 at voxel 0 and at one other voxel
    assert r.sums.tolist() == [S, S, S]
    T = [q0[0], q0[1] + 3 * Q]
    want = [[1.0, S[0][1] / T[1]], [0.0, S[1][1] / T[1]]]
    assert r.theta.tolist() == [want, want, want]
    assert r.labels.tolist() == [[0, 1], [1, 1]] and r.labels.dtype == np.uint8
    assert r.iterations == 1 and not r.converged         # delta = |S01 / T1 - 1/3| = 0.0078
    assert r.posterior.shape == (2, 2, 2) and r.posterior.dtype == np.float32
    assert np.array_equal(r.posterior.reshape(2, 4).T.astype(np.float64) * Q, r.q)
    # the start M-step alone, and the vote with its tie rule
    Dm = np.stack([d.reshape(-1).astype(np.int64) for d in D])
    assert R.vote(Dm, 2).tolist() == [0, 1, 1, 1]
    assert R.vote(np.array([[1], [0]]), 2).tolist() == [0] and R.vote(np.array([[1], [0]]), 2, True).tolist() == [1]
    q = np.zeros((4, 2), np.int64)
    q[np.arange(4), [0, 1, 1, 1]] = Q
    assert R.m_step(Dm, q, 2).tolist() == [[[Q, Q], [0, 2 * Q]]] * 3
    assert R.theta_of(R.m_step(Dm, q, 2))[0].tolist() == [[1.0, 1 / 3], [0.0, 2 / 3]]


def test_m_step_is_exact_for_sums_beyond_2_to_the_53():
    n = 1 << 10
    D = np.zeros((1, n), np.int64)
    q = np.full((n, 2), 0, np.int64)
    q[:, 0] = (1 << 52) // n * 4 + 1                     # sum 2^54 + 1024: not a float64 if added as floats
    assert R.m_step(D, q, 2)[0, 0, 0] == int(q[:, 0].sum()) == (1 << 54) + n


def test_single_rater_returns_the_rater():
    _, (a,) = R.make_raters(SHAPE, 5, [1.0], 1, truth_labels=[0, 2, 3])
    r = R.staple_ref([a], 5)
    assert np.array_equal(r.labels, a) and r.iterations == 1 and r.converged
    assert np.array_equal(r.theta[0], np.diag([1.0, 0, 1.0, 1.0, 0]))


def test_identical_raters():
    _, (a,) = R.make_raters(SHAPE, 4, [1.0], 2)
    r = R.staple_ref([a, a.copy(), a.copy()], 4)
    assert np.array_equal(r.labels, a) and r.converged and r.iterations == 1
    assert np.array_equal(r.theta, np.stack([np.eye(4)] * 3))


def test_permuting_the_raters_permutes_the_sums():
    """the products of the E-step commute only up to rounding, so the definition fixes their order; on this case
    (and in general, short of a posterior within 2^-53 of a rounding boundary) the fused result is the same"""
    _, rs = R.make_raters(SHAPE, 3, [0.9, 0.8, 0.7, 0.6], 5)
    a = R.staple_ref(rs, 3, max_iterations=8, tolerance=0.0)
    perm = [2, 0, 3, 1]
    b = R.staple_ref([rs[p] for p in perm], 3, max_iterations=8, tolerance=0.0)
    assert np.array_equal(b.sums, a.sums[perm]) and np.array_equal(a.labels, b.labels)


def test_unused_labels_give_zero_columns_and_never_come_out():
    _, rs = R.make_raters(SHAPE, 16, [0.9, 0.7, 0.6], 7, truth_labels=range(0, 16, 2))
    rs = [np.where(a % 2 == 1, (a + 1) % 16, a).astype(np.uint8) for a in rs]      # raters use even labels only
    r = R.staple_ref(rs, 16, max_iterations=10)
    assert np.isfinite(r.theta).all() and not r.theta[:, :, 1::2].any() and not r.theta[:, 1::2, :].any()
    assert not (r.labels % 2).any() and not r.q[:, 1::2].any() and not r.prior[1::2].any()


# ---------------------------------------------------------------------------- seeded faults
def _case(fault):
    if fault == "stop_le":            # delta is exactly 0 for one rater: `<` never stops at tolerance 0, `<=` does
        _, rs = R.make_raters(SHAPE, 3, [1.0], 3)
        return dict(labels=rs, num_classes=3, max_iterations=4, tolerance=0.0)
    if fault == "descending":
        # Products in another order differ in the last bit only, far below the 2^-24 grid of q.  A prior is used as
        # given, so one of subnormal size makes every product round to a multiple of 2^-1074: there the order shows.
        _, rs = R.make_raters(SHAPE, 3, [0.8, 0.7, 0.6, 0.6], 3)
        return dict(labels=rs, num_classes=3, max_iterations=3, tolerance=0.0, prior=SUBNORMAL_PRIOR)
    _, rs = R.make_raters(SHAPE, 5, np.linspace(0.9, 0.5, 4), 3)                   # 4 raters: the vote has ties
    return dict(labels=rs, num_classes=5, max_iterations=6, tolerance=0.0)


SUBNORMAL_PRIOR = [3000000001 * 5e-324, 2000000003 * 5e-324, 4000000007 * 5e-324]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_seeded_fault_is_rejected_by_the_exact_comparison(fault):
    kw = _case(fault)
    good = R.staple_ref(**kw)
    assert same(good, R.staple_ref(**kw))
    assert not same(good, R.staple_ref(fault=fault, **kw))


# ---------------------------------------------------------------------------- tables for select_best
SUMS = np.array([[[6 * Q, 1 * Q, 0], [2 * Q, 5 * Q, 0], [0, 0, 0]],
                 [[4 * Q, 0, 0], [4 * Q, 6 * Q, 0], [0, 0, 0]],
                 [[6 * Q, 3 * Q, 0], [2 * Q, 3 * Q, 0], [0, 0, 0]]], dtype=np.int64)
TISSUES = {"Background": 0, "Fat": 1, "Bone": 2}


def test_performance_table_and_best_candidates(tmp_path):
    from segmantic_amd.seg import staple as S
    from segmantic_amd.utils import config
    rows = S.performance_table(SUMS, names=["a.ckpt", "b.ckpt", "c.ckpt"], tissues=TISSUES)
    assert len(rows) == 9 and list(rows[0]) == ["rater", "label", "tissue", "sensitivity", "ppv", "voxels"]
    assert rows[0] == {"rater": "a.ckpt", "label": 0, "tissue": "Background", "sensitivity": 6 / 8, "ppv": 6 / 7,
                       "voxels": 8.0}
    assert rows[4] == {"rater": "b.ckpt", "label": 1, "tissue": "Fat", "sensitivity": 1.0, "ppv": 6 / 10, "voxels": 6.0}
    bone = rows[8]
    assert bone["tissue"] == "Bone" and math.isnan(bone["sensitivity"]) and math.isnan(bone["ppv"]) and bone["voxels"] == 0
    assert S.performance_table(SUMS)[3]["rater"] == 1 and S.performance_table(SUMS)[3]["tissue"] == "0"
    assert np.array_equal(S.confusion_of(SUMS)[0], [[6 / 8, 1 / 6, 0], [2 / 8, 5 / 6, 0], [0, 0, 0]])
    # Background: raters 0 and 2 tie at 6/8 -> the lower index; Fat: rater 1; Bone has T = 0 and is left out
    best = S.best_candidates(SUMS, TISSUES)
    assert best == {"Background": 0, "Fat": 1}
    S.write_candidates(best, tmp_path / "cand.yml")
    loaded = config.load(tmp_path / "cand.yml")
    assert loaded == best and {int(TISSUES[n]): int(i) for n, i in loaded.items()} == {0: 0, 1: 1}
    S.write_performance_csv(rows, tmp_path / "perf.csv")
    import csv
    back = list(csv.DictReader(open(tmp_path / "perf.csv")))
    assert len(back) == 9 and back[4]["rater"] == "b.ckpt" and float(back[4]["ppv"]) == 0.6 and back[8]["ppv"] == "nan"
    # pooling over volumes = adding the sums
    assert S.best_candidates(SUMS + SUMS, TISSUES) == best
    with pytest.raises(ValueError, match="sums"):
        S.performance_table(np.zeros((2, 3, 4), np.int64))
    with pytest.raises(ValueError, match="names"):
        S.performance_table(SUMS, names=["a"])


# ---------------------------------------------------------------------------- argument errors, before any device
def test_every_argument_error_names_its_argument():
    from segmantic_amd.seg.staple import staple
    a = np.zeros((4, 5), np.uint8)
    with pytest.raises(ValueError, match="raters"):
        staple([], 2)
    with pytest.raises(ValueError, match="raters"):
        staple([a] * 17, 2)
    with pytest.raises(TypeError, match="sequence"):
        staple(a, 2)
    for bad in (1, 65, 2.5):
        with pytest.raises(ValueError, match="num_classes"):
            staple([a, a], bad)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="max_iterations"):
            staple([a, a], 2, max_iterations=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tolerance"):
            staple([a, a], 2, tolerance=bad)
    for bad in ([0.5], [0.5, float("nan")], [1.0, 0.0], [1.0, 1e-13], [-1.0, 2.0]):
        with pytest.raises(ValueError, match="prior"):
            staple([a, a], 2, prior=bad)
    with pytest.raises(TypeError, match=r"labels\[1\].*float"):
        staple([a, a.astype(np.float32)], 2)
    with pytest.raises(TypeError, match=r"labels\[0\].*float"):
        staple([torch.zeros(4, 5)], 2)
    with pytest.raises(ValueError, match=r"labels\[1\].*shape"):
        staple([a, np.zeros((5, 4), np.uint8)], 2)
    with pytest.raises(ValueError, match="2-D or 3-D"):
        staple([np.zeros(7, np.uint8)], 2)


def test_ops_staple_checks_arguments_before_the_tensors():
    from segmantic_amd import ops
    for kw, name in ((dict(num_classes=1), "num_classes"), (dict(num_classes=3, max_iterations=0), "max_iterations"),
                     (dict(num_classes=3, tolerance=-1.0), "tolerance"), (dict(num_classes=3, prior=[1, 1]), "prior")):
        with pytest.raises(ValueError, match=name):
            ops.staple([torch.zeros(4, dtype=torch.uint8)], **kw)
    with pytest.raises(RuntimeError, match="MI355X"):                               # host tensors are refused
        ops.staple([torch.zeros(4, dtype=torch.uint8)], 2)
    assert ops.staple_table_name(5, 5) == "lds" and ops.staple_table_name(16, 64) == "global"
    assert ops.staple_table_name(17, 4) == "" and ops.staple_table_name(4, 65) == ""


def test_native_argument_checks_and_workspace():
    from segmantic_amd import _lib
    assert _lib.lib.segmi_staple_workspace_bytes(0, 4) == 0 and _lib.lib.segmi_staple_workspace_bytes(3, 1) == 0
    small, large = _lib.lib.segmi_staple_workspace_bytes(3, 4), _lib.lib.segmi_staple_workspace_bytes(16, 64)
    assert 0 < small < large and large >= 3 * 16 * 64 * 64 * 8 and small % 256 == 0
    assert _lib.lib.segmi_staple(None, 3, 1, 100, 4, None, 10, 1e-5, None, None, None, None, None, None, 0, None) != 0
    assert "staple" in _lib.last_error()


def test_enum_and_cli_list_the_staple_mode():
    from typer.testing import CliRunner

    from segmantic_amd.commands.monai_unet_cli import app
    from segmantic_amd.seg.enum import EnsembleCombination
    assert EnsembleCombination("staple") is EnsembleCombination.staple
    assert [m.value for m in EnsembleCombination][:3] == ["mean", "vote", "select_best"]
    out = CliRunner().invoke(app, ["ensemble-predict", "--help"], env={"COLUMNS": "200", "TERM": "dumb"}).output
    for opt in ("--staple-iterations", "--staple-tolerance", "--save-candidates", "staple"):
        assert opt in out, opt


def test_label_fusion_script_lists_its_options():
    import subprocess
    script = Path(__file__).resolve().parent.parent / "scripts" / "staple_labels.py"
    out = subprocess.run([sys.executable, str(script), "--help"], capture_output=True, text=True,
                         env={**__import__("os").environ, "COLUMNS": "200", "TERM": "dumb"})
    assert out.returncode == 0, out.stderr
    for opt in ("--tissue-list", "--iterations", "--tolerance", "--performance", "OUTPUT", "INPUT"):
        assert opt in out.stdout, opt


def test_argument_errors_come_before_the_largest_label_is_read():
    """with num_classes left to the data the largest label has to be read (from a device tensor: a read-back);
    max_iterations, tolerance and prior are checked before that"""
    from segmantic_amd.seg.staple import staple

    class Unread(np.ndarray):
        def max(self, *args, **kwargs):
            raise AssertionError("the label values were read")

    a = np.zeros((4, 5), np.uint8).view(Unread)
    for kw, name in ((dict(max_iterations=0), "max_iterations"), (dict(tolerance=float("nan")), "tolerance"),
                     (dict(prior=[0.5]), "prior"), (dict(prior=[1.0, float("inf")]), "prior"),
                     (dict(prior=[1.0, 1e-13, 1.0]), "prior"), (dict(prior=[1.0] * 65), "prior")):
        with pytest.raises(ValueError, match=name):
            staple([a, a], **kw)
    with pytest.raises(AssertionError, match="were read"):
        staple([a, a], prior=[1.0, 1.0])
    with pytest.raises(ValueError, match="prior"):                                  # 2 classes in the data, 3 in the prior
        staple([np.zeros((4, 5), np.uint8)] * 2, prior=[1.0, 1.0, 1.0])


@pytest.mark.parametrize("dtype,bad", [(np.int64, (1 << 32) + 1), (np.int64, -(1 << 32) + 1), (np.int64, -1),
                                       (np.uint32, (1 << 32) - 3), (np.uint64, 1 << 40), (np.uint16, 65535)])
def test_a_wide_label_is_not_wrapped_into_the_range(dtype, bad):
    """types the kernels do not read are narrowed to int32; 2^32 + 1 would become the valid label 1"""
    from segmantic_amd.seg.staple import staple
    a = np.zeros((4, 5), dtype)
    b = a.copy()
    b[2, 3] = bad
    with pytest.raises(ValueError, match=rf"rater 1 .*label {bad}, outside 0 \.\. 2\b"):
        staple([a, b, a], 3)
    if dtype == np.int64:
        with pytest.raises(ValueError, match=rf"rater 2 .*label {bad}, outside 0 \.\. 2\b"):
            staple([torch.from_numpy(a), torch.from_numpy(a), torch.from_numpy(b)], 3)


TINY_PRIOR = [5e-324, 5e-324]         # times a theta above 1/2 it stays 2^-1074, times one below it becomes 0


def tiny_prior_case():
    _, rs = R.make_raters(SHAPE, 2, [0.9, 0.8, 0.7], 5)
    return rs, R.staple_ref(rs, 2, max_iterations=4, tolerance=0.0, prior=TINY_PRIOR)


def test_a_voxel_whose_products_all_underflow_is_dropped():
    """a given prior is used as given; under one of tiny size every product of a disputed voxel rounds to 0
    (some rater's theta is below 1/2 for either label): q = 0 there, nothing enters S, the label is 0.  Agreed
    voxels keep q = Q on their label."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                              # no 0 / 0 anywhere
        rs, r = tiny_prior_case()
    D = np.stack(rs).reshape(3, -1)
    agreed = (D == D[0]).all(0)
    assert 0.3 < agreed.mean() < 0.7
    assert not r.q[~agreed].any() and not r.labels.reshape(-1)[~agreed].any()
    assert np.array_equal(r.q[agreed, D[0][agreed]], np.full(agreed.sum(), Q)) and np.array_equal(r.labels.reshape(-1)[agreed], D[0][agreed])
    assert r.sums[0].sum() == int(agreed.sum()) * Q and np.isfinite(r.theta).all() and not r.posterior.reshape(2, -1)[:, ~agreed].any()
