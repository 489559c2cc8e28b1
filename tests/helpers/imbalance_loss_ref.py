"""Float64 references of the class-imbalance training losses (tests/test_imbalance_loss_host.py,
tests/test_imbalance_loss_gpu.py), written in torch so that autograd gives the gradients.

Logits ``[N, K, *spatial]``, integer-valued labels ``[N, 1, *spatial]``; softmax over all K classes.  A voxel whose
label lies outside ``[0, K)`` belongs to no class row: it is in no target sum, no cross-entropy sum and no normaliser.
``I``, ``P``, ``T`` are the per-(n, k) sums intersection, sum p, sum t.

* ``ref_tversky_loss``: ``TI = (I + smooth_nr) / (I + alpha (P - I) + beta (T - I) + smooth_dr)``,
  ``loss = mean over the included (n, k) of (1 - TI) ** exponent``; where ``1 - TI <= 0`` the term is 0.  The
  denominator is evaluated as ``(1 - alpha - beta) I + alpha P + beta T + smooth_dr``: the same number, and with
  ``alpha = beta = 0.5`` and both smooths ``s / 2`` every operation is the Dice term's scaled by exactly 1/2, so the
  value equals ``ref_dice_loss`` with smooth ``s`` to the last bit.
* ``ref_dice_focal_loss``: ``lambda_dice * Dice + lambda_focal * Focal`` with
  ``Focal = sum_v w[y_v] q_v ** gamma nll_v / W``, ``nll_v = -log p_{v,y_v}``, ``q_v = 1 - p_{v,y_v}`` formed as the
  sum of the other probabilities, ``W = sum_v w[y_v]`` batch-global.  ``gamma = 0`` leaves the factor out.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _probs_targets(logits, labels):
    k = logits.shape[1]
    y = labels[:, 0].long()
    valid = (y >= 0) & (y < k)
    yc = y.clamp(0, k - 1)
    p = torch.softmax(logits, 1)
    t = F.one_hot(yc, k).movedim(-1, 1).to(p.dtype) * valid[:, None].to(p.dtype)
    return p, t, yc, valid


def _sums(p, t, include_background):
    if not include_background:
        if p.shape[1] == 1:
            raise ValueError("include_background=False needs more than one class")
        p, t = p[:, 1:], t[:, 1:]
    axes = list(range(2, p.dim()))
    return (p * t).sum(axes), p.sum(axes), t.sum(axes)


def ref_dice_term(logits, labels, include_background=True, smooth_nr=1e-5, smooth_dr=1e-5):
    p, t, _, _ = _probs_targets(logits, labels)
    i, ps, ts = _sums(p, t, include_background)
    return (1.0 - (2.0 * i + smooth_nr) / (ts + ps + smooth_dr)).mean()


def ref_tversky_loss(logits, labels, include_background=True, alpha=0.3, beta=0.7, exponent=1.0, smooth_nr=1e-5,
                     smooth_dr=1e-5):
    p, t, _, _ = _probs_targets(logits, labels)
    i, ps, ts = _sums(p, t, include_background)
    ti = (i + smooth_nr) / ((1.0 - alpha - beta) * i + alpha * ps + beta * ts + smooth_dr)
    u = 1.0 - ti
    pos = u > 0
    term = torch.where(pos, u, torch.zeros_like(u))
    if exponent != 1.0:
        # the power only where the base is positive: no NaN gradient from 0 ** (exponent - 1)
        term = torch.where(pos, torch.where(pos, u, torch.ones_like(u)) ** exponent, torch.zeros_like(u))
    return term.mean()


def tversky_grad_abs(logits, labels, **params):
    """The ``A`` of tests/helpers/lowp_bounds.py for the Tversky gradient: with ``D = d loss / d p`` (per class, from
    autograd on the probabilities) the gradient is ``g_j = p_j (D_j - sum_i p_i D_i)``, and the same expression on the
    absolute values of its operands is ``A_j = p_j (|D_j| + sum_i p_i |D_i|)``.  ``D_j`` and the sum cancel (by factors
    of 10^5 and more where a voxel is classified well), so ``|g|`` itself is no bound on the rounding noise."""
    k = logits.shape[1]
    y = labels[:, 0].long()
    valid = (y >= 0) & (y < k)
    t = F.one_hot(y.clamp(0, k - 1), k).movedim(-1, 1).to(logits.dtype) * valid[:, None].to(logits.dtype)
    p = torch.softmax(logits.detach(), 1).requires_grad_(True)
    i, ps, ts = _sums(p, t, params.get("include_background", True))
    alpha, beta = params.get("alpha", 0.3), params.get("beta", 0.7)
    snr, sdr = params.get("smooth_nr", 1e-5), params.get("smooth_dr", 1e-5)
    u = 1.0 - (i + snr) / ((1.0 - alpha - beta) * i + alpha * ps + beta * ts + sdr)
    pos = u > 0
    (torch.where(pos, torch.where(pos, u, torch.ones_like(u)) ** params.get("exponent", 1.0),
                 torch.zeros_like(u)).mean()).backward()
    d, pd = p.grad.abs(), p.detach()
    return pd * (d + (pd * d).sum(1, keepdim=True))


def ref_nll(logits, labels):
    """per-voxel ``-log p_y`` [N, *spatial] (0 where the label is outside [0, K)) and the validity mask"""
    _, _, yc, valid = _probs_targets(logits, labels)
    nll = -torch.log_softmax(logits, 1).gather(1, yc[:, None])[:, 0]
    return torch.where(valid, nll, torch.zeros_like(nll)), valid


def ref_focal_term(logits, labels, gamma=2.0, weight=None):
    p, t, yc, valid = _probs_targets(logits, labels)
    nll, _ = ref_nll(logits, labels)
    w = torch.ones(logits.shape[1], dtype=logits.dtype) if weight is None else \
        torch.as_tensor(weight, dtype=logits.dtype)
    wv = w[yc] * valid.to(logits.dtype)
    f = nll
    if gamma != 0.0:
        q = (p * (1.0 - F.one_hot(yc, logits.shape[1]).movedim(-1, 1).to(p.dtype))).sum(1)
        f = q ** gamma * nll
    return (wv * f).sum() / wv.sum()


def ref_dice_focal_loss(logits, labels, include_background=True, lambda_dice=1.0, lambda_focal=1.0, gamma=2.0,
                        weight=None, smooth_nr=1e-5, smooth_dr=1e-5):
    loss = lambda_dice * ref_dice_term(logits, labels, include_background, smooth_nr, smooth_dr)
    if lambda_focal != 0.0:        # switched off altogether, as lambda_ce = 0: no NaN from W = 0
        loss = loss + lambda_focal * ref_focal_term(logits, labels, gamma, weight)
    return loss
