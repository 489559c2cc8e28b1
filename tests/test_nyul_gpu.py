"""Nyul standardisation (csrc/nyul.hip, seg/nyul_normalize.py) on the MI355X against the numpy oracle of
tests/helpers/nyul_ref.py and torch.quantile."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from segmantic_amd import ops
from segmantic_amd.seg.nyul_normalize import NyulNormalize, fit_standard_scale
from tests.helpers import nyul_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
Q11 = np.array([0.01] + [i / 10 for i in range(1, 10)] + [0.99])


def _same_value(a, b):
    """bit-equal, except that the sign of a zero may differ and NaN matches NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ok = (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))
    return bool(ok.all())


def _same_bits(a, b):
    """bit-equal, NaN payloads aside"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _ulps(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _data(kind, n, rng):
    if kind == "random":
        return rng.standard_normal(n).astype(np.float32) * 300
    if kind == "negative":
        return (-np.abs(rng.standard_normal(n)) * 1e3 + rng.uniform(-2, 0.1, n)).astype(np.float32)
    if kind == "ties":
        return rng.integers(-1024, 4, n).astype(np.float32)
    if kind == "special":
        pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.2e-38, -3e-39, 1.0, -1.0, 7.5],
                        np.float32)
        return rng.choice(pool, n)
    raise ValueError(kind)


def _device_landmarks(x_np, q, nonzero=False, segments=1):
    x = torch.from_numpy(np.ascontiguousarray(x_np, np.float32)).to(DEV)
    lm, cnt = ops.nyul_landmarks(x, segments, nonzero, q)
    return lm.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("kind", ["random", "negative", "ties", "special"])
@pytest.mark.parametrize("nonzero", [False, True])
def test_order_statistics_exact(kind, nonzero):
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 1000, 123_457):
        x = _data(kind, n, rng)
        m = x[x != 0] if nonzero else x
        if m.size < 1:
            continue
        # q = 0, 1 and (odd count) 0.5 have integer f32 ranks: the landmark is the order statistic itself
        q = [0.0, 0.5, 1.0]
        got, cnt = _device_landmarks(x, q, nonzero)
        assert cnt[0] == m.size
        ranks = [0, (m.size - 1) // 2, m.size - 1]
        part = np.partition(m, ranks)
        for j, r in enumerate(ranks):
            if np.isfinite(part[r]) and (j != 1 or m.size % 2):
                assert _same_value(got[0, j], part[r]), (kind, n, j, got[0, j], part[r])
        # every landmark (order statistics + lerp) against the oracle
        got2, _ = _device_landmarks(x, Q11, nonzero)
        assert _same_value(got2[0], ref.landmarks(m, Q11)), (kind, n, got2[0], ref.landmarks(m, Q11))


@pytest.mark.parametrize("n", [1 << 24, (1 << 24) + 3])
def test_both_rank_regimes(n):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(n) * 100).astype(np.float32)
    x[: n // 4] = -1024.0                             # heavy constant background
    got, cnt = _device_landmarks(x, Q11)
    assert cnt[0] == n
    want = ref.landmarks(x, Q11)
    assert _same_value(got[0], want), (got[0], want)
    xt = torch.from_numpy(x)
    if n <= 1 << 24:
        tq = torch.quantile(xt, torch.from_numpy(Q11.astype(np.float32))).numpy()
        assert _ulps(got[0], tq).max() <= 1, (got[0], tq)
    else:
        with pytest.raises(RuntimeError, match="too large"):
            torch.quantile(xt, torch.from_numpy(Q11.astype(np.float32)))


def test_ct_volume_512x512x80():
    rng = np.random.default_rng(7)
    x = np.full((1, 80, 512, 512), -1024.0, np.float32)
    x[:, :, 96:416, 96:416] = rng.normal(40, 300, (1, 80, 320, 320)).astype(np.float32)
    for nonzero in (False, True):
        got, _ = _device_landmarks(x, Q11, nonzero)
        m = x[x != 0] if nonzero else x.reshape(-1)
        assert _same_value(got[0], ref.landmarks(m, Q11))


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("channel_wise", [False, True])
@pytest.mark.parametrize("nonzero", [False, True])
def test_channels_and_masks_end_to_end(c, channel_wise, nonzero):
    rng = np.random.default_rng(c)
    img = (rng.standard_normal((c, 17, 33, 29)) * (50 * np.arange(1, c + 1))[:, None, None, None]).astype(np.float32)
    img[:, :5] = 0.0
    if c > 1:
        img[1] = 0.0                                   # an all-zero channel: empty under nonzero
    scale = np.linspace(-5.0, 95.0, Q11.size)
    t = torch.from_numpy(img).to(DEV)
    tr = NyulNormalize(Q11, scale, nonzero=nonzero, channel_wise=channel_wise)
    lms = tr.landmarks(t).cpu().numpy()
    assert _same_value(lms, ref.all_landmarks(img, Q11, nonzero, channel_wise))
    out = tr(t)
    assert out is t
    got = t.cpu().numpy()
    # the map is bit-equal to the f32 oracle given the device landmarks
    want = ref.apply_with(img, lms, scale, nonzero, channel_wise)
    assert _same_bits(got, want)
    if nonzero:
        z = img == 0
        assert np.array_equal(got[z].view(np.uint32), img[z].view(np.uint32))   # masked out: bit-untouched
    # end to end against the oracle within 1e-4 of the scale range
    e2e = ref.normalize(img, Q11, scale, nonzero, channel_wise)
    fin = np.isfinite(e2e)
    assert np.array_equal(np.isnan(got), np.isnan(e2e))
    assert np.abs(got[fin] - e2e[fin]).max() <= 1e-4 * (scale[-1] - scale[0])


def test_known_answers_through_hip_map(golden_dir):
    g = json.loads((golden_dir / "reference_nyul_interp1d.json").read_text())
    tr = NyulNormalize(np.array([0.1, 0.5, 0.9]), np.array([0, 0.5, 1.0]))
    xp, yp = torch.tensor(g["xp"], device=DEV), torch.tensor(g["yp"], device=DEV)
    for case in g["cases"]:
        x = torch.tensor(case["x"], device=DEV)
        y = tr.interp1d(x, xp, yp)
        assert y.shape == x.shape and y.device == x.device
        np.testing.assert_allclose(y.cpu().numpy(), case["expected"], rtol=g["rel_tol"], atol=1e-6)
        want = ref.interp(np.array(case["x"], np.float32), np.array(g["xp"]), np.array(g["yp"]))
        assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_empty_segment_untouched_and_nan_propagates():
    img = np.zeros((3, 8, 8, 8), np.float32)
    img[0] = np.arange(512, dtype=np.float32).reshape(8, 8, 8) - 100
    img[1, 0, 0, 0] = -0.0
    img[2] = np.arange(512, dtype=np.float32).reshape(8, 8, 8) + 1
    img[2, 3, 3, 3] = np.nan
    before = img.copy()
    t = torch.from_numpy(img).to(DEV)
    NyulNormalize(Q11, np.linspace(0, 100, 11), nonzero=True, channel_wise=True)(t)
    got = t.cpu().numpy()
    assert np.array_equal(got[1].view(np.uint32), before[1].view(np.uint32))   # empty mask: bit-untouched
    assert np.isnan(got[2][before[2] != 0]).all()                              # NaN in the mask: NaN out
    assert np.isfinite(got[0][before[0] != 0]).all()


def test_duplicate_landmarks_reproduce_reference_inf_nan():
    rng = np.random.default_rng(2)
    img = np.full((1, 40, 40, 40), -1024.0, np.float32)
    img[0, 20:] = rng.normal(50, 200, (20, 40, 40)).astype(np.float32)        # half air: low landmarks tie
    scale = np.linspace(0, 100, 11)
    t = torch.from_numpy(img).to(DEV)
    tr = NyulNormalize(Q11, scale)
    lms = tr.landmarks(t).cpu().numpy()
    assert lms[0, 0] == lms[0, 1] == -1024.0
    tr(t)
    got = t.cpu().numpy()
    want = ref.apply_with(img, lms, scale)
    assert _same_bits(got, want)
    assert not np.isfinite(got[0, 0]).any()


def test_repeat_calls_bit_identical_and_no_host_sync():
    rng = np.random.default_rng(9)
    img = (rng.standard_normal((2, 64, 64, 64)) * 100).astype(np.float32)
    tr = NyulNormalize(Q11, np.linspace(0, 100, 11), nonzero=True, channel_wise=True)
    a, b = torch.from_numpy(img).to(DEV), torch.from_numpy(img).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tr(a)
        tr(b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_host_and_other_dtype_inputs_in_place():
    rng = np.random.default_rng(4)
    img = (rng.standard_normal((2, 20, 21, 22)) * 100).astype(np.float32)
    scale = np.linspace(0, 100, 11)
    want = ref.normalize(img, Q11, scale, True, True)
    tr = NyulNormalize(Q11, scale, nonzero=True, channel_wise=True)
    a = img.copy()
    assert tr(a) is a and a.dtype == np.float32
    assert np.array_equal(a, want)
    c = torch.from_numpy(img.copy())
    assert tr(c) is c and c.device.type == "cpu"
    assert np.array_equal(c.numpy(), want)
    h = torch.from_numpy(img.copy()).to(DEV).half()
    h0 = h.clone()
    assert tr(h) is h and h.dtype == torch.float16
    want_h = ref.normalize(h0.float().cpu().numpy(), Q11, scale, True, True)
    np.testing.assert_allclose(h.float().cpu().numpy(), want_h, rtol=2e-3, atol=0.1)
    d = img.astype(np.float64)
    tr(d)
    assert d.dtype == np.float64 and np.array_equal(d.astype(np.float32), want)
    nc = torch.from_numpy(img.copy()).to(DEV).transpose(1, 3)           # non-contiguous
    tr(nc)
    np.testing.assert_array_equal(nc.transpose(1, 3).cpu().numpy(), want)


def test_fit_standard_scale_matches_oracle():
    rng = np.random.default_rng(8)
    imgs = [(rng.standard_normal((2, 24, 24, 24)) * s + s).astype(np.float32) for s in (10, 50, 200)]
    imgs.append(np.zeros((2, 8, 8, 8), np.float32))                   # skipped under nonzero: empty
    for nonzero in (False, True):
        want, skipped_want = ref.fit(imgs, Q11, nonzero, True, 0.0, 100.0)
        got, skipped = fit_standard_scale([torch.from_numpy(i).to(DEV) for i in imgs], Q11, nonzero=nonzero,
                                          channel_wise=True)
        again, _ = fit_standard_scale([torch.from_numpy(i).to(DEV) for i in imgs], Q11, nonzero=nonzero,
                                      channel_wise=True)
        assert skipped == skipped_want == 2
        assert np.array_equal(got, want) and np.array_equal(got.view(np.uint64), again.view(np.uint64))
    with pytest.raises(ValueError):
        fit_standard_scale([np.zeros((1, 4, 4, 4), np.float32)], Q11, nonzero=True)


def test_script_fit_and_apply(tmp_path):
    from segmantic_amd.data.imageio import read_image, write_image

    rng = np.random.default_rng(1)
    src, out = tmp_path / "img", tmp_path / "out"
    src.mkdir()
    vols = []
    for k in range(2):
        v = (rng.standard_normal((12, 14, 16)) * 100 + 20 * k).astype(np.float32)
        v[:2] = 0
        write_image(src / f"case{k}.nii.gz", v, np.eye(4))
        vols.append(read_image(src / f"case{k}.nii.gz")[0])
    scale_json = tmp_path / "scale.json"
    script = str(ROOT / "scripts" / "nyul_normalize.py")
    r = subprocess.run([sys.executable, script, "fit", str(src), str(scale_json), "--nonzero"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cfg = json.loads(scale_json.read_text())
    q = np.array(cfg["quantiles"])
    want_scale, _ = ref.fit([v[None] for v in vols], q, True, False)
    assert np.allclose(cfg["standard_scale"], want_scale, rtol=0, atol=1e-9) and cfg["nonzero"] is True
    r = subprocess.run([sys.executable, script, "apply", str(src), str(out), "--scale", str(scale_json)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for k, v in enumerate(vols):
        got = read_image(out / f"case{k}.nii.gz")[0]
        want = ref.normalize(v[None], q, np.array(cfg["standard_scale"]), True, False)[0]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-4 * 100)
