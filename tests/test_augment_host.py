"""Host checks of the float64 augmentation references (tests/helpers/augment_ref.py) against
independent formulations, and of the flip-order rewrite ``seg.augment.flip_params``: the reference
flips last (RandFlipd after the k-space transforms) while the crop kernels flip first, so
flip(T(x, p)) must equal T(flip(x), p') for every flip code and both parities of extent."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests.helpers import augment_ref as ar

_spec = importlib.util.spec_from_file_location(
    "segmi_augment", Path(__file__).resolve().parents[1] / "segmantic_amd" / "seg" / "augment.py")
aug = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(aug)

SHAPES = [(8, 6, 10), (7, 5, 9), (8, 5, 6), (6, 1, 7)]


def _noise(shape, seed, c=2):
    return np.random.RandomState(seed).randn(c, *shape)


def _all_on(n, roi, seed):
    """draws of ``draw_intensity`` with every transform switched on"""
    rng = np.random.RandomState(seed)
    con, hist, bias, gibbs, spike = aug.draw_intensity(rng, n, roi)
    on = np.ones(n, np.uint8)
    return ((on, con[1]), (on, hist[1]), (on, bias[1]), (on, gibbs[1]), (on, spike[1], spike[2]))


@pytest.mark.parametrize("shape", SHAPES + [(9, 16, 15)])
@pytest.mark.parametrize("code", [0, 1, 6, 7])
def test_gibbs_on_the_plain_spectrum_equals_the_centred_spectrum(shape, code):
    """The kernel masks fftn(x) with the centred index (j + n // 2) mod n: the circular shifts are
    phase ramps that commute with the mask (csrc/augment.hip, comment above dft_axis_kernel)."""
    x = _noise(shape, 1)
    for alpha in (0.05, 0.5, 0.8):
        a = ar.gibbs(x, alpha, code)
        b = ar.gibbs_unshifted(x, alpha, code)
        assert np.abs(a - b).max() < 1e-12 * np.abs(a).max()
    assert np.abs(a - x).max() > 1e-3                        # alpha 0.8: the mask removed something


@pytest.mark.parametrize("shape", SHAPES)
def test_spike_on_the_plain_spectrum_equals_the_centred_spectrum(shape):
    x = _noise(shape, 2)
    for loc in [(0, 0, 0), tuple(s - 1 for s in shape), tuple(s // 2 for s in shape), (1, 0, shape[2] - 2)]:
        a = ar.spike(x, loc, 0.3)
        b = ar.spike_unshifted(x, loc, 0.3)
        # exp(log(|K| + 1e-10)) moves every other bin by 1e-10: far below the bound
        assert np.abs(a - b).max() < 1e-9 * np.abs(a).max(), loc
        assert np.abs(a - x).max() > 1e-3


def _legendre(i, t):
    return [np.ones_like(t), t, 0.5 * (3 * t ** 2 - 1), 0.5 * (5 * t ** 3 - 3 * t)][i]


@pytest.mark.parametrize("shape", [(5, 6, 7), (1, 4, 3), (16, 2, 9)])
def test_bias_field_equals_a_direct_triple_sum(shape):
    x = _noise(shape, 3)
    coef = np.random.RandomState(4).uniform(-0.5, 0.5, 20)
    t = [np.linspace(-1, 1, n) for n in shape]
    s = np.zeros(shape)
    k = 0
    for a in range(4):
        for b in range(4 - a):
            for c in range(4 - a - b):
                s += coef[k] * (_legendre(a, t[0])[:, None, None] * _legendre(b, t[1])[None, :, None]
                                * _legendre(c, t[2])[None, None, :])
                k += 1
    assert k == 20
    ref = x * np.exp(s)[None]
    assert np.abs(ar.bias_field(x, coef) - ref).max() < 1e-13 * np.abs(ref).max()


def test_mirror_rule():
    for n in (1, 2, 7, 8, 15, 16):
        assert np.array_equal(aug.mirror_index(np.arange(n), n), ar.mirror(np.arange(n), n))
        # bin i holds frequency (i - n // 2); its mirror holds the negated frequency (mod n)
        f = np.arange(n) - n // 2
        fm = aug.mirror_index(np.arange(n), n) - n // 2
        assert np.array_equal((f + fm) % n, np.zeros(n, int))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("code", range(8))
def test_flip_last_equals_flip_first_with_mirrored_parameters(shape, code):
    """flip(T(x, p)) == T(flip(x), p'): T = contrast, histogram shift, bias field, Gibbs, spike;
    p' = flip_params(p) and the Gibbs mask at the mirrored bin (what ops.kspace_augment is told)."""
    n = 3
    draws = _all_on(n, shape, 10 + code)
    # patch 0: all five, the spike at the centre bin, inside the Gibbs radius.  Patches 1 and 2: the
    # spike at the corner bins, Gibbs off.  A spike on a bin the Gibbs mask zeroed (with its
    # conjugate) is left out: its phase is angle() of round-off, which no order of operations fixes.
    draws[3][1][0] = 0.5
    draws[4][1][0] = tuple(s // 2 for s in shape)
    draws[4][1][1] = (0, 0, 0)
    draws[4][1][2] = tuple(s - 1 for s in shape)
    draws[3][0][1:] = 0
    mirrored = aug.flip_params(draws, [code] * n, shape)
    worst_unfixed = 0.0
    for i in range(n):
        x = _noise(shape, 20 + i)
        want = ar.flip(ar.intensity_chain(x, draws, i), code)
        got = ar.intensity_chain(ar.flip(x, code), mirrored, i, code)
        assert np.abs(got - want).max() < 1e-9 * np.abs(want).max(), i
        naive = ar.intensity_chain(ar.flip(x, code), draws, i)        # flips before, parameters as drawn
        worst_unfixed = max(worst_unfixed, float(np.abs(naive - want).max() / np.abs(want).max()))
    flipped = [d for d in range(3) if code & (1 << d) and shape[d] > 1]
    if flipped:
        # the bias field's odd terms alone change sign: the unmirrored order is visibly different
        assert worst_unfixed > 1e-3
    else:
        assert worst_unfixed < 1e-12


def test_flip_params_leaves_unflipped_patches_and_draws_alone():
    roi = (8, 6, 10)
    draws = _all_on(4, roi, 3)
    before = [np.array(a, copy=True) for t in draws for a in t]
    out = aug.flip_params(draws, [0, 1, 2, 4], roi)
    after = [a for t in draws for a in t]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))    # inputs not modified
    assert np.array_equal(out[2][1][0], draws[2][1][0]) and np.array_equal(out[4][1][0], draws[4][1][0])
    # three-parameter form (no k-space draws)
    assert len(aug.flip_params(draws[:3], [7] * 4, roi)) == 3
