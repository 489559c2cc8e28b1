"""Reference of the Dice + cross-entropy training loss (tests/test_loss_host.py, tests/test_loss_gpu.py).

``loss = lambda_dice * Dice + lambda_ce * CE`` on logits ``[N, K, *spatial]`` and integer-valued labels
``[N, 1, *spatial]``:

* Dice: ``oracle.unet_ref.ref_dice_loss`` (softmax over all K classes, smooth 1e-5 / 1e-5, per (n, k), mean);
  with ``include_background=False`` class 0 is dropped after the softmax and the mean runs over N * (K - 1).
* CE: ``F.cross_entropy(logits, labels[:, 0].long(), weight=w, reduction="mean")`` over all voxels of the batch.

Built from ``torch.softmax`` and ``F.cross_entropy`` only; float64 when given float64 logits.  Labels must lie in
``[0, K)``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def ref_dice_ce_loss(logits, labels, include_background=True, lambda_dice=1.0, lambda_ce=1.0, weight=None,
                     smooth_nr=1e-5, smooth_dr=1e-5):
    k = logits.shape[1]
    if not include_background and k == 1:
        raise ValueError("include_background=False needs more than one class")
    y = labels[:, 0].long()
    p = torch.softmax(logits, 1)
    t = F.one_hot(y, k).movedim(-1, 1).to(p.dtype)
    if not include_background:
        p, t = p[:, 1:], t[:, 1:]
    axes = list(range(2, logits.dim()))
    inter = (p * t).sum(axes)
    den = t.sum(axes) + p.sum(axes)
    dice = (1.0 - (2.0 * inter + smooth_nr) / (den + smooth_dr)).mean()
    w = None if weight is None else torch.as_tensor(weight, dtype=logits.dtype)
    ce = F.cross_entropy(logits, y, weight=w, reduction="mean")
    return lambda_dice * dice + lambda_ce * ce
