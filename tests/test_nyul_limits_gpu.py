"""The Nyul kernels (csrc/nyul.hip) at 64 landmarks (128 ranks, 8 slot groups), with more slots per pass than one
workgroup holds, with many pass-C slots under one top digit, with the rank regime decided by the masked count, and
with more segments than workgroups per chip, on the MI355X.  Inputs and the proof that each crosses its limit:
tests/helpers/preproc_limits.py and tests/test_preproc_limits_host.py.  Landmarks are compared with the oracle of
tests/helpers/nyul_ref.py by the rules of tests/test_nyul_gpu.py (`_same_value`; within 1 ulp of torch.quantile), the
map bit for bit (`_same_bits`).  Every call is made twice and must give identical bits."""
import numpy as np
import pytest
import torch

from segmantic_amd import ops
from tests.helpers import nyul_ref as ref
from tests.helpers import preproc_limits as lim
from tests.helpers.preproc_limits import _same_bits, _same_value, _ulps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.view(torch.int32)


def _landmarks_twice(x_np, q, nonzero, segments=1):
    x = torch.from_numpy(np.array(x_np, np.float32)).to(DEV)
    lm, cnt = ops.nyul_landmarks(x, segments, nonzero, q)
    lm2, cnt2 = ops.nyul_landmarks(x, segments, nonzero, q)
    assert torch.equal(_bits(lm), _bits(lm2)) and torch.equal(cnt, cnt2)
    return lm.cpu().numpy(), cnt.cpu().numpy()


def _apply_twice(x_np, segments, nonzero, lm_np, counts, scale):
    lm = torch.from_numpy(np.array(lm_np, np.float32)).to(DEV)
    a = torch.from_numpy(np.array(x_np, np.float32)).to(DEV)
    b = a.clone()
    assert ops.nyul_apply_(a, segments, nonzero, lm, counts, scale) is a
    ops.nyul_apply_(b, segments, nonzero, lm, counts, scale)
    assert torch.equal(_bits(a), _bits(b))
    return a.cpu().numpy()


# ------------------------------------------------------------------ 64 landmarks: slot groups and the pass-C walk
@pytest.mark.parametrize("nonzero", [False, True])
@pytest.mark.parametrize("kind", ["wide", "narrow", "mixed"])
def test_64_landmarks_past_one_group_of_slots(kind, nonzero):
    """R = 128 ranks (the thread bound of nyul_dedup and the scans, the 64 threads of finalize, grid.z = 8).
    wide: 65 / 66 pass-B slots, work in five groups.  narrow: 77 / 87 pass-C slots under one top digit, the `++j`
    walk crosses groups and s_table names a slot of group 0 for matches in later groups.  mixed: top digits with
    one slot next to one with 43 / 47 that starts past group 0."""
    x = lim.nyul_input(kind)
    got, cnt = _landmarks_twice(x, lim.Q64, nonzero)
    m = lim.masked(x, nonzero)
    assert cnt.tolist() == [m.size]
    want = ref.landmarks(m, lim.Q64)
    assert _same_value(got[0], want), (kind, nonzero, np.flatnonzero(got[0] != want), got[0], want)
    # q = 0 and q = 1 are the extremes themselves
    assert _same_value(got[0, [0, -1]], [m.min(), m.max()])


@pytest.mark.parametrize("nonzero", [False, True])
def test_64_landmarks_of_three_segments_in_one_call(nonzero):
    """wide, narrow and all-zero segments side by side (the vectorised passes): each block reads its own segment's
    slots, the empty segment returns without touching the others"""
    x = lim.nyul_three_segments()
    got, cnt = _landmarks_twice(x, lim.Q64, nonzero, segments=3)
    want = ref.all_landmarks(x, lim.Q64, nonzero, True)
    assert cnt.tolist() == [lim.masked(s, nonzero).size for s in x]
    assert _same_value(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if nonzero:
        assert cnt[2] == 0 and np.isnan(got[2]).all()
    else:
        assert not got[2].any()


@pytest.mark.parametrize("kind", ["wide", "mixed"])
def test_repeated_quantiles_at_128_ranks(kind):
    """16 quantiles four times each: nyul_dedup sees runs of equal ranks at R = 128"""
    x = lim.nyul_input(kind)
    got, _ = _landmarks_twice(x, lim.Q64_REPEATED, True)
    want = ref.landmarks(lim.masked(x, True), lim.Q64_REPEATED)
    assert _same_value(got[0], want), (got[0], want)
    rep = got[0].reshape(16, 4)
    assert (rep.view(np.uint32) == rep.view(np.uint32)[:, :1]).all()


# ------------------------------------------------------------------ the rank regime follows the masked count
def test_rank_regime_follows_the_masked_count():
    """one segment of 2^24 + 3 values under nonzero.  With 8 zeros n = 2^24 - 5: torch's f32 rule, although the
    segment is longer than 2^24.  With 2 zeros n = 2^24 + 1: numpy's f64 rule."""
    q = lim.Q_BIG
    for form in ("below", "above"):
        x = lim.nyul_big(form)
        m = lim.masked(x, True)
        got, cnt = _landmarks_twice(x, q, True)
        assert cnt.tolist() == [m.size] == [lim.BIG_N - lim.BIG_ZEROS[form]]
        want = ref.landmarks(m, q)
        assert _same_value(got[0], want), (form, got[0], want)
        if form == "below":
            tq = torch.quantile(torch.from_numpy(m), torch.from_numpy(q.astype(np.float32))).numpy()
            assert _ulps(got[0], tq).max() <= 1, (got[0], tq)
        del x, m


# ------------------------------------------------------------------ more segments than workgroups per chip
@pytest.mark.parametrize("seg_len", lim.MANY_LENS)
def test_600_segments_then_an_ordinary_call(seg_len):
    """600 segments (grid.y = 600, one chunk each; 41: scalar loads, 40: float4), a workspace of about 90 MB; a
    small call afterwards still matches its reference"""
    x = lim.nyul_many(seg_len)
    for nonzero in (False, True):
        got, cnt = _landmarks_twice(x, lim.Q3, nonzero, segments=lim.MANY_SEGMENTS)
        want = ref.all_landmarks(x, lim.Q3, nonzero, True)
        assert cnt.tolist() == [lim.masked(s, nonzero).size for s in x]
        assert _same_value(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    small = lim.nyul_input("narrow")
    got, cnt = _landmarks_twice(small, lim.Q11, True)
    assert cnt.tolist() == [lim.masked(small, True).size]
    assert _same_value(got[0], ref.landmarks(lim.masked(small, True), lim.Q11))


def test_workspace_of_600_segments():
    need = ops.nyul_workspace_bytes(lim.MANY_SEGMENTS, lim.Q3.size)
    assert 80e6 < need < 110e6
    assert ops.nyul_workspace_bytes(1, 64) > 128 * 2048 * 8


# ------------------------------------------------------------------ the map
@pytest.mark.parametrize("nonzero", [False, True])
def test_map_of_2100_segments(nonzero):
    """nyul_apply_ alone, more segments than the map's 2048 workgroups per chip: each segment its own landmarks"""
    x, lm, scale = lim.nyul_map_many()
    got = _apply_twice(x, lim.MAP_SEGMENTS, nonzero, lm, None, scale)
    want = ref.apply_with(x, lm, scale, nonzero, True)
    assert _same_bits(got, want)
    if nonzero:
        assert np.array_equal(got[:, 3].view(np.uint32), x[:, 3].view(np.uint32))


def test_map_of_2100_segments_skips_the_empty_ones():
    x, lm, scale = lim.nyul_map_many()
    counts = np.full(lim.MAP_SEGMENTS, lim.MAP_LEN, np.int64)
    counts[[0, 777, 2048, 2099]] = 0
    got = _apply_twice(x, lim.MAP_SEGMENTS, False, lm, torch.from_numpy(counts).to(DEV), scale)
    want = ref.apply_with(x, lm, scale, False, True)
    want[counts == 0] = x[counts == 0]
    assert _same_bits(got, want)


@pytest.mark.parametrize("pad_to_four", [True, False])
@pytest.mark.parametrize("nonzero", [False, True])
def test_map_at_64_landmarks(nonzero, pad_to_four):
    """L = kNyulMaxLandmarks: the whole LDS tables and six steps of the search; values on every landmark, one ulp
    to either side, outside both ends, +-inf, NaN and +-0"""
    x, lm, scale = lim.nyul_map_64(pad_to_four)
    got = _apply_twice(x, 1, nonzero, lm[None], None, scale)
    want = ref.apply_with(x[None], lm[None], scale, nonzero)[0]
    assert _same_bits(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    z = x == 0
    if nonzero:
        assert np.array_equal(got[z].view(np.uint32), x[z].view(np.uint32))            # masked out: bit-untouched
    else:
        assert (got[z] != 0).all()
    assert np.isnan(got[np.isnan(x)]).all() and np.isinf(got[np.isinf(x)]).all()
