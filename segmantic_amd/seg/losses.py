"""Loss / metric front-ends over the fused HIP kernels.

``DiceLoss`` replaces ``monai.losses.DiceLoss(to_onehot_y=True, softmax=True)`` as constructed at
reference ``src/segmantic/seg/monai_unet.py:128`` and called at ``:344`` / ``:357``;
``DiceMetric`` replaces ``monai.metrics.DiceMetric(include_background=False, reduction="mean")``
(``:136-138``, ``:642-644``).

``DiceCELoss`` (MONAI's ``DiceCELoss(to_onehot_y=True, softmax=True)``) adds a class-weighted cross-entropy
term computed by the same two kernels, and both losses take ``include_background``.  Every loss object offers
``forward_ndhwc`` / ``backward_ndhwc``, the explicit (no autograd graph) interface ``Net.training_step``
drives; ``loss_from_config`` builds the object an ``optimizer["loss"]`` dictionary names.

``TverskyLoss`` and ``DiceFocalLoss`` answer class imbalance on the same two passes.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from .. import ops


def as_ndhwc(t: torch.Tensor) -> torch.Tensor:
    """Logical [N,C,D,H,W] tensor -> dense NDHWC storage [N,D,H,W,C] (no copy if already so)."""
    if t.dim() != 5:
        raise ValueError("expected a 5-D [N,C,D,H,W] tensor")
    p = t.permute(0, 2, 3, 4, 1)
    return p if p.is_contiguous() else p.contiguous()


class _LossState:
    """Scratch owned by one loss instance (reused across calls).  ``rows`` / ``coef_rows``: the partial and
    coefficient rows per (n, k) of the kernels it serves -- (3, 2) for Dice and Tversky, (4, 3) with a
    cross-entropy or focal term."""

    def __init__(self, rows: int = 3, coef_rows: int = 2):
        self.rows, self.coef_rows = rows, coef_rows
        self.partials: Optional[torch.Tensor] = None     # f32 [chunks, n, rows, k], the kernel's layout
        self.coef: Optional[torch.Tensor] = None         # f32 [n, coef_rows, k]
        self.loss: Optional[torch.Tensor] = None
        self.labels: Optional[torch.Tensor] = None       # the flattened labels of the last forward
        self.gamma: Optional[float] = None               # DiceFocalLoss: the gamma of the last forward
        self.weight: Optional[torch.Tensor] = None       # device copy of the class weights
        self._weight_key = None

    def prepare(self, logits: torch.Tensor, labels: torch.Tensor, include_background: bool = True,
                weight: Optional[Sequence[float]] = None) -> torch.Tensor:
        """Checks and buffers of one forward on NDHWC ``logits``; returns the flattened f32 labels."""
        n, k, dev = logits.shape[0], logits.shape[4], logits.device
        if weight is not None and len(weight) != k:
            raise ValueError(f"'class_weights' has {len(weight)} entries, the logits have {k} classes")
        if not include_background and k == 1:
            raise ValueError("include_background=False needs more than one class")
        lab = labels.to(dev, torch.float32).contiguous().view(-1)
        if lab.numel() != logits.numel() // k:
            raise ValueError("label volume does not match logits")
        shape = (ops.dice_ce_chunks(logits), n, self.rows, k)
        if self.partials is None or self.partials.shape != shape or self.partials.device != dev:
            self.partials = torch.empty(shape, device=dev)
            self.coef = torch.empty((n, self.coef_rows, k), device=dev)
        # the device copy follows the values it was made from: a loss's ``weight`` may be edited between calls
        key = None if weight is None else (tuple(float(v) for v in weight), dev)
        if key != self._weight_key:
            if key is not None and any(not math.isfinite(v) or v < 0.0 for v in key[0]):
                raise ValueError(f"'class_weights' must be finite and >= 0 (got {list(key[0])})")
            self.weight = None if weight is None else torch.tensor(key[0], dtype=torch.float32, device=dev)
            self._weight_key = key
        # a fresh scalar per call: callers keep the returned loss tensor
        self.loss = torch.empty(1, device=dev)
        self.labels = lab
        return lab


def _backward(state: _LossState, bwd, bwd_amp, extra, logits_ndhwc: torch.Tensor, grad_scale: float,
              out: Optional[torch.Tensor], bias_grad: Optional[torch.Tensor],
              amp: Optional[torch.Tensor]) -> torch.Tensor:
    """dlogits of the last forward on ``state`` through ``bwd`` (``bwd_amp`` when ``amp`` is given);
    ``extra``: the backward op's own arguments in front of the scale."""
    if out is None or out.shape != logits_ndhwc.shape or out.dtype != logits_ndhwc.dtype:
        out = torch.empty_like(logits_ndhwc)
    scratch = state.partials if bias_grad is not None else None
    op, scale = (bwd, grad_scale) if amp is None else (bwd_amp, amp)
    op(logits_ndhwc, state.labels, state.coef, *extra, scale, out, scratch=scratch, bias_grad=bias_grad)
    return out


def dice_forward(state: _LossState, logits_ndhwc: torch.Tensor, labels: torch.Tensor,
                 smooth_nr: float, smooth_dr: float) -> torch.Tensor:
    lab = state.prepare(logits_ndhwc, labels)
    ops.softmax_dice_fwd(logits_ndhwc, lab, state.partials, state.coef, state.loss, smooth_nr, smooth_dr)
    return state.loss.view(())


def dice_backward(state: _LossState, logits_ndhwc: torch.Tensor, grad_scale: float = 1.0,
                  out: Optional[torch.Tensor] = None,
                  bias_grad: Optional[torch.Tensor] = None,
                  amp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``bias_grad`` (f32[K]): also receives sum_voxels dlogits, i.e. the bias gradient of the conv
    that produced the logits (saves that layer a pass over the gradient tensor).  ``amp`` (the f32[3]
    state of a ``GradScaler``): the gradient is scaled by the loss scale held there on the device
    (``grad_scale`` is then ignored)."""
    return _backward(state, ops.softmax_dice_bwd, ops.softmax_dice_bwd_amp, (), logits_ndhwc, grad_scale, out,
                     bias_grad, amp)


class _LossFn(torch.autograd.Function):
    """Bridges a loss object's explicit forward / backward into autograd for external training loops."""

    @staticmethod
    def forward(ctx, logits, labels, loss_mod):
        lg = as_ndhwc(logits)
        ctx.lg = lg
        ctx.mod = loss_mod
        return loss_mod.forward_ndhwc(lg, labels).clone()

    @staticmethod
    def backward(ctx, g):
        # g is the upstream scalar; fold it into the kernel on the host only when it is 1
        d = ctx.mod.backward_ndhwc(ctx.lg, 1.0)
        d = d.permute(0, 4, 1, 2, 3)
        gs = g.to(d.dtype)
        return (d if bool(gs == 1) else d * gs), None, None


# the kernel families: forward op, backward op, _amp backward op, (partial rows, coefficient rows)
_DICE = (ops.softmax_dice_fwd, ops.softmax_dice_bwd, ops.softmax_dice_bwd_amp, (3, 2))
_DICE_CE = (ops.softmax_dice_ce_fwd, ops.softmax_dice_ce_bwd, ops.softmax_dice_ce_bwd_amp, (4, 3))
_TVERSKY = (ops.softmax_tversky_fwd, ops.softmax_tversky_bwd, ops.softmax_tversky_bwd_amp, (3, 2))
_DICE_FOCAL = (ops.softmax_dice_focal_fwd, ops.softmax_dice_focal_bwd, ops.softmax_dice_focal_bwd_amp, (4, 3))


class _FusedLoss(torch.nn.Module):
    """What the losses share: ``forward`` on logical [N,K,D,H,W] logits (autograd bridge or plain value) over
    ``forward_ndhwc`` / ``backward_ndhwc``, the scratch, and the backward.  A subclass validates its parameters,
    binds its kernel family and writes ``forward_ndhwc``."""

    def _bind(self, family, what: str, to_onehot_y: bool, softmax: bool) -> None:
        """the subclass's kernel family and a scratch of its row counts"""
        if not (to_onehot_y and softmax):
            raise NotImplementedError(f"the HIP {what} kernels implement to_onehot_y=True, softmax=True")
        self._fwd, self._bwd, self._bwd_amp, rows = family
        self._state = _LossState(*rows)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """logits [N,K,D,H,W] (float32/bfloat16/float16), labels [N,1,D,H,W] integer-valued."""
        if logits.requires_grad and torch.is_grad_enabled():
            return _LossFn.apply(logits, labels, self)
        return self.forward_ndhwc(as_ndhwc(logits), labels).clone()

    def _run_forward(self, logits_ndhwc: torch.Tensor, labels: torch.Tensor, *params, weight=None) -> torch.Tensor:
        """the bound forward op on this loss's scratch; ``params``: the op's arguments behind ``loss`` (with
        ``weight`` the device copy of the class weights is appended)"""
        st = self._state
        lab = st.prepare(logits_ndhwc, labels, self.include_background, weight)
        if weight is not None:
            params += (st.weight,)
        self._fwd(logits_ndhwc, lab, st.partials, st.coef, st.loss, self.smooth_nr, self.smooth_dr, *params)
        return st.loss.view(())

    def _bwd_extra(self) -> tuple:
        """the backward op's own arguments (in front of the scale)"""
        return ()

    def backward_ndhwc(self, logits_ndhwc: torch.Tensor, grad_scale: float = 1.0,
                       out: Optional[torch.Tensor] = None, bias_grad: Optional[torch.Tensor] = None,
                       amp: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dlogits of the last ``forward_ndhwc`` (see ``dice_backward`` for ``bias_grad`` / ``amp``)"""
        return _backward(self._state, self._bwd, self._bwd_amp, self._bwd_extra(), logits_ndhwc, grad_scale, out,
                         bias_grad, amp)


def _check_lambda(name: str, v) -> float:
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"'{name}' must be finite and >= 0 (got {v})")
    return v


def _check_weight(weight) -> Optional[list]:
    if weight is None:
        return None
    w = [float(v) for v in (weight.tolist() if isinstance(weight, torch.Tensor) else weight)]
    if not w or any(not math.isfinite(v) or v < 0.0 for v in w):
        raise ValueError(f"'class_weights' must be finite and >= 0 (got {w})")
    return w


def _check_range(name: str, v, ok, what: str) -> float:
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"'{name}' must be a number (got {v!r})") from None
    if not (math.isfinite(v) and ok(v)):
        raise ValueError(f"'{name}' must {what} (got {v})")
    return v


class DiceLoss(_FusedLoss):
    """Fused softmax + one-hot + Dice (MONAI defaults: include_background, smooth 1e-5, mean).
    ``include_background=False`` drops class 0 after the softmax (mean over N * (K - 1)); it runs on the
    Dice + cross-entropy kernels with ``lambda_ce = 0``, the default on the Dice-only kernels."""

    def __init__(self, to_onehot_y: bool = True, softmax: bool = True, smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5, include_background: bool = True):
        super().__init__()
        self._bind(_DICE if include_background else _DICE_CE, "Dice", to_onehot_y, softmax)
        self.smooth_nr, self.smooth_dr = smooth_nr, smooth_dr
        self.include_background = bool(include_background)

    def forward_ndhwc(self, logits_ndhwc: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """NDHWC logits (K real classes; the row stride may be larger) -> 0-d loss on the device"""
        if self.include_background:
            return self._run_forward(logits_ndhwc, labels)
        return self._run_forward(logits_ndhwc, labels, 1.0, 0.0, False, None)


class DiceCELoss(_FusedLoss):
    """``lambda_dice * Dice + lambda_ce * CE`` in the two passes of the Dice kernels (MONAI's ``DiceCELoss``
    with ``to_onehot_y=True, softmax=True``).

    Dice is ``DiceLoss`` (``include_background`` applies to this term only).  CE is
    ``F.cross_entropy(logits, labels[:, 0].long(), weight=weight, reduction="mean")`` over every voxel of the
    batch and all K classes: ``sum_v w[y_v] * -log p_{v,y_v} / W`` with ``W = sum_v w[y_v]`` batch-global (NaN when
    ``W = 0``, as in torch).  A voxel whose label lies outside ``[0, K)`` contributes to neither CE nor ``W``
    (nor to the Dice target sums).  ``weight``: K finite values >= 0 (its length is checked against the logits
    at the first call).  Under data parallelism every rank normalises by its own ``W`` and the gradient
    all-reduce averages the ranks, as torch DDP does with this loss."""

    def __init__(self, include_background: bool = True, to_onehot_y: bool = True, softmax: bool = True,
                 lambda_dice: float = 1.0, lambda_ce: float = 1.0, weight=None, smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5):
        super().__init__()
        self._bind(_DICE_CE, "Dice + cross-entropy", to_onehot_y, softmax)
        self.include_background = bool(include_background)
        self.lambda_dice = _check_lambda("lambda_dice", lambda_dice)
        self.lambda_ce = _check_lambda("lambda_ce", lambda_ce)
        self.weight = _check_weight(weight)
        self.smooth_nr, self.smooth_dr = smooth_nr, smooth_dr

    def forward_ndhwc(self, logits_ndhwc: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self._run_forward(logits_ndhwc, labels, self.lambda_dice, self.lambda_ce, self.include_background,
                                 weight=self.weight)


class TverskyLoss(_FusedLoss):
    """Tversky / focal Tversky loss on the Dice kernels (MONAI's ``TverskyLoss(to_onehot_y=True, softmax=True)``
    raised to ``exponent``): per (n, k) ``TI = (I + smooth_nr) / (I + alpha (P - I) + beta (T - I) + smooth_dr)``,
    ``loss = mean (1 - TI) ** exponent``.  ``alpha`` weighs false positives, ``beta`` false negatives; the defaults
    0.3 / 0.7 are Salehi et al.'s, ``exponent = 0.75`` is Abraham and Khan's focal Tversky loss (gamma = 4/3).
    ``include_background=False`` drops class 0 after the softmax as ``DiceLoss`` does."""

    def __init__(self, include_background: bool = True, to_onehot_y: bool = True, softmax: bool = True,
                 alpha: float = 0.3, beta: float = 0.7, exponent: float = 1.0, smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5):
        super().__init__()
        self._bind(_TVERSKY, "Tversky", to_onehot_y, softmax)
        self.include_background = bool(include_background)
        self.alpha = _check_range("alpha", alpha, lambda v: v >= 0.0, "be finite and >= 0")
        self.beta = _check_range("beta", beta, lambda v: v >= 0.0, "be finite and >= 0")
        if not self.alpha + self.beta > 0.0:
            raise ValueError(f"'alpha' + 'beta' must be > 0 (got {self.alpha}, {self.beta})")
        self.exponent = _check_range("exponent", exponent, lambda v: 0.0 < v <= 3.0, "lie in (0, 3]")
        self.smooth_nr, self.smooth_dr = smooth_nr, smooth_dr

    def forward_ndhwc(self, logits_ndhwc: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self._run_forward(logits_ndhwc, labels, self.alpha, self.beta, self.exponent, self.include_background)


class DiceFocalLoss(_FusedLoss):
    """``lambda_dice * Dice + lambda_focal * Focal`` in the two passes of the Dice + cross-entropy kernels.

    ``Focal = sum_v w[y_v] * (1 - p_{v,y_v}) ** gamma * -log p_{v,y_v} / W`` with ``W = sum_v w[y_v]`` batch-global,
    the normaliser of ``DiceCELoss``'s cross-entropy term (Lin et al.'s focal loss on the softmax; MONAI's
    ``DiceFocalLoss`` averages over N * K * V elements instead, a constant factor).  ``gamma`` is 0 or in [1, 5];
    ``gamma = 0`` is ``DiceCELoss`` bit for bit.  ``weight``, ``include_background`` and the label rule as there."""

    def __init__(self, include_background: bool = True, to_onehot_y: bool = True, softmax: bool = True,
                 lambda_dice: float = 1.0, lambda_focal: float = 1.0, gamma: float = 2.0, weight=None,
                 smooth_nr: float = 1e-5, smooth_dr: float = 1e-5):
        super().__init__()
        self._bind(_DICE_FOCAL, "Dice + focal", to_onehot_y, softmax)
        self.include_background = bool(include_background)
        self.lambda_dice = _check_lambda("lambda_dice", lambda_dice)
        self.lambda_focal = _check_lambda("lambda_focal", lambda_focal)
        self.gamma = _check_range("gamma", gamma, lambda v: v == 0.0 or 1.0 <= v <= 5.0, "be 0 or lie in [1, 5]")
        self.weight = _check_weight(weight)
        self.smooth_nr, self.smooth_dr = smooth_nr, smooth_dr

    def forward_ndhwc(self, logits_ndhwc: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        loss = self._run_forward(logits_ndhwc, labels, self.lambda_dice, self.lambda_focal, self.gamma,
                                 self.include_background, weight=self.weight)
        self._state.gamma = self.gamma           # the backward differentiates the forward that ran
        return loss

    def _bwd_extra(self) -> tuple:
        return (self._state.gamma,)


# ------------------------------------------------------------------ configuration
LOSS_NAMES = ("Dice", "DiceCE", "CE", "Tversky", "DiceFocal")
_LOSS_KEYS = {"Dice": ("name", "include_background"),
              "DiceCE": ("name", "include_background", "lambda_dice", "lambda_ce", "class_weights"),
              "CE": ("name", "lambda_ce", "class_weights"),
              "Tversky": ("name", "include_background", "alpha", "beta", "exponent"),
              "DiceFocal": ("name", "include_background", "lambda_dice", "lambda_focal", "gamma", "class_weights")}


def loss_from_config(cfg, num_classes: Optional[int] = None) -> torch.nn.Module:
    """The loss object of ``optimizer["loss"]``: ``None`` -> ``DiceLoss()``; else a dictionary
    ``{name: Dice | DiceCE | CE, include_background, lambda_dice, lambda_ce, class_weights}`` (``CE`` is
    ``DiceCE`` with ``lambda_dice = 0``), ``{name: Tversky, include_background, alpha, beta, exponent}`` or
    ``{name: DiceFocal, include_background, lambda_dice, lambda_focal, gamma, class_weights}``.  Raises ``ValueError`` naming the offending key; touches no device.
    ``num_classes`` (when known) checks the length of ``class_weights``."""
    if cfg is None:
        return DiceLoss(to_onehot_y=True, softmax=True)
    if not isinstance(cfg, dict):
        raise ValueError(f"'loss' must be a dictionary with a 'name' in {LOSS_NAMES} (got {cfg!r})")
    name = cfg.get("name", "Dice")
    if name not in LOSS_NAMES:
        raise ValueError(f"'loss': unknown 'name' {name!r}; expected one of {LOSS_NAMES}")
    unknown = [k for k in cfg if k not in _LOSS_KEYS[name]]
    if unknown:
        raise ValueError(f"'loss': unknown key {unknown[0]!r} for name {name!r}; expected {_LOSS_KEYS[name]}")
    include_background = cfg.get("include_background", True)
    if not isinstance(include_background, bool):
        raise ValueError(f"'loss': 'include_background' must be true or false (got {include_background!r})")
    if not include_background and num_classes is not None and num_classes < 2:
        raise ValueError("'loss': 'include_background' = false needs more than one class")
    if name == "Dice":
        return DiceLoss(to_onehot_y=True, softmax=True, include_background=include_background)
    if name == "Tversky":
        try:
            return TverskyLoss(include_background=include_background, alpha=cfg.get("alpha", 0.3),
                               beta=cfg.get("beta", 0.7), exponent=cfg.get("exponent", 1.0))
        except ValueError as e:
            raise ValueError(f"'loss': {e}") from e
    weights = cfg.get("class_weights")
    if weights is not None:
        if not isinstance(weights, (list, tuple)):
            raise ValueError(f"'loss': 'class_weights' must be a list of numbers (got {weights!r})")
        if num_classes is not None and len(weights) != num_classes:
            raise ValueError(f"'loss': 'class_weights' has {len(weights)} entries, 'num_classes' is {num_classes}")
    try:
        if name == "DiceFocal":
            return DiceFocalLoss(include_background=include_background, lambda_dice=cfg.get("lambda_dice", 1.0),
                                 lambda_focal=cfg.get("lambda_focal", 1.0), gamma=cfg.get("gamma", 2.0),
                                 weight=weights)
        return DiceCELoss(include_background=include_background,
                          lambda_dice=0.0 if name == "CE" else cfg.get("lambda_dice", 1.0),
                          lambda_ce=cfg.get("lambda_ce", 1.0), weight=weights)
    except (TypeError, ValueError) as e:
        raise ValueError(f"'loss': {e}") from e


class DiceMetric:
    """Label-overlap Dice: per class 2|P&T| / (|P|+|T|), NaN when the class is absent in T,
    nan-mean over classes then over the accumulated batch items (reduction="mean")."""

    def __init__(self, num_classes: int, include_background: bool = False):
        self.k = num_classes
        self.include_background = include_background
        self._items = []

    def __call__(self, pred_labels: torch.Tensor, true_labels: torch.Tensor) -> torch.Tensor:
        """pred/true: integer label volumes with a leading batch dim [N, ...]. Returns [N, C']."""
        out = []
        for b in range(pred_labels.shape[0]):
            p = pred_labels[b].reshape(-1).to(torch.int32).contiguous()
            t = true_labels[b].reshape(-1).to(device=p.device, dtype=torch.int32).contiguous()
            counts = torch.empty((self.k, 3), dtype=torch.int64, device=p.device)
            ops.label_counts(p, t, self.k, counts)
            c = counts.double()
            d = torch.where(c[:, 2] > 0, 2.0 * c[:, 0] / (c[:, 1] + c[:, 2]),
                            torch.full((self.k,), float("nan"), dtype=torch.double, device=p.device))
            if not self.include_background:
                d = d[1:]
            out.append(d.float())
        res = torch.stack(out)
        self._items.append(res)
        return res

    def aggregate(self) -> torch.Tensor:
        if not self._items:
            return torch.tensor(float("nan"))
        d = torch.cat(self._items)
        nn_ = ~torch.isnan(d)
        per_b = torch.where(nn_, d, torch.zeros_like(d)).sum(1) / nn_.sum(1).clamp(min=1)
        valid = nn_.sum(1) > 0
        # MONAI do_metric_reduction("mean"): 0 (not NaN) when no item has a valid class
        return per_b[valid].mean() if bool(valid.any()) else torch.zeros((), device=d.device)

    def reset(self):
        self._items = []


class ConfusionMatrixMetric:
    """MONAI ``ConfusionMatrixMetric(metric_name=[...])`` as configured at reference
    ``monai_unet.py:645-646`` (include_background=True, compute_sample=False, reduction="mean"):
    tp / fp / tn / fn per (volume, class) from the same ``segmi_label_counts`` pass the Dice metric
    uses, averaged over all accumulated (volume, class) items, then the ratios."""

    NAMES = ("sensitivity", "specificity", "precision", "accuracy")

    def __init__(self, num_classes: int, metric_name=NAMES):
        unknown = [m for m in metric_name if m not in self.NAMES]
        if unknown:
            raise NotImplementedError(f"confusion metrics implemented: {self.NAMES}, not {unknown}")
        self.k, self.metric_name = num_classes, list(metric_name)
        self._items = []

    def __call__(self, pred_labels: torch.Tensor, true_labels: torch.Tensor) -> torch.Tensor:
        """integer label volumes [N, ...] -> [N, K, 4] (tp, fp, tn, fn) float64."""
        out = []
        for b in range(pred_labels.shape[0]):
            p = pred_labels[b].reshape(-1).to(torch.int32).contiguous()
            t = true_labels[b].reshape(-1).to(device=p.device, dtype=torch.int32).contiguous()
            counts = torch.empty((self.k, 3), dtype=torch.int64, device=p.device)
            ops.label_counts(p, t, self.k, counts)
            c = counts.double()
            tp, fp, fn = c[:, 0], c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
            tn = float(p.numel()) - tp - fp - fn
            out.append(torch.stack([tp, fp, tn, fn], 1))
        res = torch.stack(out)
        self._items.append(res)
        return res

    def aggregate(self):
        """-> one 0-d tensor per metric name (MONAI returns a list in ``metric_name`` order)."""
        if not self._items:
            return [torch.tensor(float("nan")) for _ in self.metric_name]
        tp, fp, tn, fn = torch.cat(self._items).mean((0, 1)).unbind()
        vals = {"sensitivity": tp / (tp + fn), "specificity": tn / (tn + fp),
                "precision": tp / (tp + fp), "accuracy": (tp + tn) / (tp + fp + tn + fn)}
        return [vals[m].float() for m in self.metric_name]

    def reset(self):
        self._items = []
