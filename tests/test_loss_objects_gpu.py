"""The loss objects of ``segmantic_amd.seg.losses`` against direct ``ops.softmax_*`` calls, bit for bit.

The kernels are held to their float64 references in tests/test_loss_gpu.py and tests/test_imbalance_loss_gpu.py; this
file pins the Python layer above them: an object's ``forward_ndhwc`` / ``backward_ndhwc`` must hand the kernels
exactly what a caller who allocates the buffers and calls the ops would, so loss, dlogits and bias gradient are
``torch.equal``.

Logits [2, 17, 24, 33, k]: 13 464 voxels per item = one full 8192-voxel chunk and a ragged one, and no multiple of
256, so the tail loop runs.  k = 16 dense (the full-width instantiation), k = 3 dense (scalar loads) and k = 3 as a
channel slice of rows of 8.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import ops  # noqa: E402
from segmantic_amd.seg import losses  # noqa: E402

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
N, SP = 2, (17, 24, 33)
LAYOUTS = {"k16": (16, None), "k3": (3, None), "k3-of-8": (3, 8)}      # classes, row length of a channel slice
AMP = [1024.0, 0.0, 0.0]


def weights_for(k):
    return [0.25 + 0.5 * (j % 4) for j in range(k)]                    # exact in f32


# configuration -> (the object, forward op, backward op, _amp backward op, (partial rows, coefficient rows),
#                   the forward op's arguments behind the smooths (class weights last, as a list), backward extras)
def config(name, k):
    w = weights_for(k)
    if name == "dice":
        return (losses.DiceLoss(), ops.softmax_dice_fwd, ops.softmax_dice_bwd, ops.softmax_dice_bwd_amp, (3, 2),
                (), None, ())
    if name == "dice-nobg":
        return (losses.DiceLoss(include_background=False), ops.softmax_dice_ce_fwd, ops.softmax_dice_ce_bwd,
                ops.softmax_dice_ce_bwd_amp, (4, 3), (1.0, 0.0, False), None, ())
    if name == "dice-ce-weights":
        return (losses.DiceCELoss(lambda_dice=0.5, lambda_ce=2.0, weight=w), ops.softmax_dice_ce_fwd,
                ops.softmax_dice_ce_bwd, ops.softmax_dice_ce_bwd_amp, (4, 3), (0.5, 2.0, True), w, ())
    if name == "tversky-focal-nobg":
        return (losses.TverskyLoss(include_background=False, exponent=0.75), ops.softmax_tversky_fwd,
                ops.softmax_tversky_bwd, ops.softmax_tversky_bwd_amp, (3, 2), (0.3, 0.7, 0.75, False), None, ())
    if name == "dice-focal-gamma2-weights":
        return (losses.DiceFocalLoss(gamma=2.0, weight=w), ops.softmax_dice_focal_fwd, ops.softmax_dice_focal_bwd,
                ops.softmax_dice_focal_bwd_amp, (4, 3), (1.0, 1.0, 2.0, True), w, (2.0,))
    assert name == "dice-focal-gamma0"
    return (losses.DiceFocalLoss(gamma=0.0), ops.softmax_dice_focal_fwd, ops.softmax_dice_focal_bwd,
            ops.softmax_dice_focal_bwd_amp, (4, 3), (1.0, 1.0, 0.0, True), None, (0.0,))


CONFIGS = ["dice", "dice-nobg", "dice-ce-weights", "tversky-focal-nobg", "dice-focal-gamma2-weights",
           "dice-focal-gamma0"]


def rows_of(shape, dtype, ld):
    """an NDHWC buffer of ``shape``; ``ld``: as a channel slice of rows of ``ld``"""
    if ld is None:
        return torch.zeros(shape, dtype=dtype, device=DEV)
    return torch.zeros(tuple(shape[:4]) + (ld,), dtype=dtype, device=DEV)[..., :shape[4]]


@functools.lru_cache(maxsize=None)
def inputs(layout, dt, n=N, sp=SP):
    k, ld = LAYOUTS[layout]
    g = torch.Generator().manual_seed(1000 * k + n)
    lg = rows_of((n,) + sp + (k,), DTYPES[dt], ld)
    lg.copy_(((torch.rand((n,) + sp + (k,), generator=g) * 2 - 1) * 3).to(DEV))
    lab = torch.randint(0, k, (n, 1) + sp, generator=g).float().to(DEV)
    return lg, lab


def scales():
    """the two ways a backward is scaled: (grad_scale, amp)"""
    return [(0.5, None), (1.0, torch.tensor(AMP, device=DEV))]


def through_ops(name, lg, lab, ld, grad_scale, amp):
    """the ops on buffers allocated here"""
    n, k = lg.shape[0], lg.shape[4]
    _, fwd, bwd, bwd_amp, (rows, crows), params, w, extra = config(name, k)
    chunks = ops.dice_chunks(lg) if fwd is ops.softmax_dice_fwd else ops.dice_ce_chunks(lg)
    part = torch.empty((chunks, n, rows, k), device=DEV)
    coef = torch.empty((n, crows, k), device=DEV)
    loss = torch.empty(1, device=DEV)
    if w is not None:
        params += (torch.tensor(w, dtype=torch.float32, device=DEV),)
    labf = lab.contiguous().view(-1)
    fwd(lg, labf, part, coef, loss, 1e-5, 1e-5, *params)
    dl, db = rows_of(lg.shape, lg.dtype, ld), torch.empty(k, device=DEV)
    if amp is not None:
        bwd_amp(lg, labf, coef, *extra, amp, dl, scratch=part, bias_grad=db)
    else:
        bwd(lg, labf, coef, *extra, grad_scale, dl, scratch=part, bias_grad=db)
    torch.cuda.synchronize()
    return loss.view(()), dl, db


def through_object(obj, lg, lab, ld, grad_scale, amp):
    db = torch.empty(lg.shape[4], device=DEV)
    loss = obj.forward_ndhwc(lg, lab)
    dl = obj.backward_ndhwc(lg, grad_scale, rows_of(lg.shape, lg.dtype, ld), bias_grad=db, amp=amp)
    torch.cuda.synchronize()
    return loss, dl, db


def same(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", CONFIGS)
def test_object_equals_direct_op_calls(name, layout, dt):
    k, ld = LAYOUTS[layout]
    lg, lab = inputs(layout, dt)
    obj = config(name, k)[0]
    for grad_scale, amp in scales():
        want = through_ops(name, lg, lab, ld, grad_scale, amp)
        got = through_object(obj, lg, lab, ld, grad_scale, amp)
        assert bool(torch.isfinite(want[0])) and bool(want[1].float().abs().max() > 0)
        assert torch.equal(got[0], want[0]), (float(got[0]), float(want[0]))
        assert torch.equal(got[1], want[1])
        assert torch.equal(got[2], want[2])
    # without a buffer the object allocates dlogits itself
    dl = obj.backward_ndhwc(lg, 0.5)
    assert dl.shape == lg.shape and dl.dtype == lg.dtype
    assert torch.equal(dl, through_ops(name, lg, lab, ld, 0.5, None)[1])


@pytest.mark.parametrize("name", ["dice", "dice-ce-weights", "dice-focal-gamma2-weights"])
def test_one_object_across_shapes_and_weight_edits(name):
    """scratch reuse: shape A, another batch size and extent, A again -- each as a fresh object computes it"""
    k = 3
    a = inputs("k3", "f32")
    b = inputs("k3", "f32", 3, (9, 10, 11))
    obj = config(name, k)[0]
    kept = []
    for lg, lab in (a, b, a):
        got = through_object(obj, lg, lab, None, 0.5, None)
        assert same(got, through_object(config(name, k)[0], lg, lab, None, 0.5, None))
        kept.append((got[0], got[0].clone()))
    assert not torch.equal(kept[0][0], kept[1][0])                     # the two shapes give different losses ...
    assert all(torch.equal(t, c) for t, c in kept)                     # ... and a returned loss keeps its value
    if not hasattr(obj, "weight"):
        return
    # the class weights may be edited between calls: in place, and by assignment
    lg, lab = a
    before = through_object(obj, lg, lab, None, 0.5, None)
    obj.weight[0] = 1.75
    edited = through_object(obj, lg, lab, None, 0.5, None)
    fresh = type(obj)(**{**_kwargs(name), "weight": [1.75] + weights_for(k)[1:]})
    assert same(edited, through_object(fresh, lg, lab, None, 0.5, None)) and not torch.equal(edited[0], before[0])
    obj.weight = [1.0, 0.5, 2.0]
    fresh = type(obj)(**{**_kwargs(name), "weight": [1.0, 0.5, 2.0]})
    assert same(through_object(obj, lg, lab, None, 0.5, None), through_object(fresh, lg, lab, None, 0.5, None))
    assert torch.equal(kept[0][0], kept[0][1])


def _kwargs(name):
    return dict(lambda_dice=0.5, lambda_ce=2.0) if name == "dice-ce-weights" else dict(gamma=2.0)
