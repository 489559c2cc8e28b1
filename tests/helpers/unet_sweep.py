"""Shared pieces of the UNet shape / config sweep (tests/test_unet_sweep_host.py, tests/test_unet_sweep_gpu.py).

* ``SWEEP``: named network + batch configurations chosen so that every shape- and config-dependent decision of
  ``segmantic_amd/seg/unet.py`` goes both ways somewhere (see ``Census``).
* ``oracle_step`` / ``oracle_eval``: ``oracle.unet_ref.RefUNet`` in float64 (or float32 for the conditioning check):
  forward, Dice loss, backward, Adam(lr=1e-4) in the reference's step order.
* ``engine_step``: the same quantities from ``Net`` on the GPU in a given precision.
* ``f32_step_violations`` / ``f32_eval_violations``: the f32 gates of tests/test_unet_gpu.py as functions of
  (got, ref), so that the host test can show that they bite.
* ``emulate_lowp``: the oracle with every stored activation (and every MFMA weight operand) rounded to bf16 / fp16.
* ``Census``: observes which way each dispatch decision went and which convolution family ran.

Importable without a GPU (nothing below touches a device until ``engine_step`` is called).
"""
from __future__ import annotations

import re
from collections import OrderedDict, namedtuple
from contextlib import contextmanager

import numpy as np
import torch
import torch.nn as nn

from oracle.unet_ref import RefUNet, _ADN, _ResidualUnit, _hash_uniform, deterministic_fill_, ref_dice_loss

DEV = "cuda:0"
DEFAULT5 = (16, 32, 64, 128, 256)

Cfg = namedtuple("Cfg", "name K cin channels strides act dropout spatial batch dims seed")

# Strides: ``UNetEngine`` accepts stride values 1 and 2 in its argument check, but every level's up path is the
# stride-2 transposed convolution (``_make_level`` raises for any other stride), and every entry of ``strides`` up to
# ``len(channels) - 1`` belongs to a level.  So NO ladder with a stride-1 level is legal: the only legal kind is
# all-2, and ``STRIDE1_REFUSED`` is what tests/test_unet_sweep_gpu.py shows to be refused loudly.
# Dropout: the engine draws its own masks (counter hash), which no oracle can reproduce: the sweep keeps p = 0.
STRIDE1_REFUSED = Cfg("stride1-refused", 3, 1, (16, 32, 64), (2, 1), "PRELU", 0.0, (8, 16, 16), 1, 3, 1)

# Extents: d/h/w pairwise different except where a kernel's eligibility needs a particular product; total stride is
# 2^(levels); "min" = the smallest legal extent (one total stride) in that dimension.
SWEEP = [
    # default ladder, depth = ONE total stride (bottleneck depth 1), several in h / w; nothing is ring-sized: 16 -> 16 on the
    # tile kernel (CK=16 s1 in 16 bit), fused decoder top and apply+conv backward taken, class axis padded 3 -> 16
    Cfg("default5-K3-b1-16x32x48", 3, 1, DEFAULT5, (2, 2, 2, 2), "PRELU", 0.0, (16, 32, 48), 1, 3, 1),
    # default ladder, ring-sized top level with two z-segments, 32-channel class axis (K = 20 -> 32): ring2 NT=2, tensors
    # above the one-launch BatchNorm backward's 32 MB, two input channels
    Cfg("default5-K20-cin2-b3-32x64x96", 20, 2, DEFAULT5, (2, 2, 2, 2), "PRELU", 0.0, (32, 64, 96), 3, 3, 68),
    # three levels, batch 8, K = 16 (no class padding): ring3 single segment, in-kernel BatchNorm apply, backward sums
    Cfg("l16-32-64-K16-b8-16x64x80", 16, 1, (16, 32, 64), (2, 2), "PRELU", 0.0, (16, 64, 80), 8, 3, 22),
    # non-MFMA ladder (direct kernels), four input channels, ReLU, depth = one total stride
    Cfg("l8-16-32-K2-cin4-relu-b1-4x24x40", 2, 4, (8, 16, 32), (2, 2), "RELU", 0.0, (4, 24, 40), 1, 3, 4),
    # repeated 16 (a 16 -> 16 stride-2 unit, a 16-channel second level), LeakyReLU, K = 20, batch 3
    Cfg("l16-16-32-64-K20-leaky-b3-24x40x64", 20, 1, (16, 16, 32, 64), (2, 2, 2), "LEAKYRELU", 0.0, (24, 40, 64), 3, 3, 24),
    # h not a multiple of the fused decoder top's 16-voxel tile
    Cfg("l16-32-64-K3-b1-12x24x40", 3, 1, (16, 32, 64), (2, 2), "PRELU", 0.0, (12, 24, 40), 1, 3, 6),
    # 32-channel first level (small-Cin pair kernel with 32 outputs), K = 33 -> 48 padded classes (48 -> 48 top conv)
    Cfg("l32-64-128-K33-b1-20x28x36", 33, 1, (32, 64, 128), (2, 2), "PRELU", 0.0, (20, 28, 36), 1, 3, 7),
    # 2-D network (depth-1 volume: never ring-sized), batch 3
    Cfg("2d-l16-32-64-K3-b3-48x80", 3, 1, (16, 32, 64), (2, 2), "PRELU", 0.0, (48, 80), 3, 2, 8),
    # two levels, batch 8, the one case with 128 in a dimension: the half-resolution 16 -> 32 bottleneck convolution is
    # ring-sized, its input gradient is the 32 -> 16 layer that takes ring2 NT=1
    Cfg("l16-32-K2-b8-64x64x128", 2, 1, (16, 32), (2,), "PRELU", 0.0, (64, 64, 128), 8, 3, 9),
]
SWEEP_IDS = [c.name for c in SWEEP]


def total_stride(cfg: Cfg) -> int:
    return int(np.prod(cfg.strides[:len(cfg.channels) - 1]))


# ------------------------------------------------------------------------------------------------ inputs
def make_batch(cfg: Cfg):
    """(image [B, cin, *spatial] f32, label [B, 1, *spatial] f32): hash-uniform noise of unit variance per channel and
    nested ellipsoidal shells around a per-sample centre (``synthetic_batch`` for non-cubic extents): every class is
    present and the regions are blobs, not noise."""
    sp = tuple(cfg.spatial)
    shape = (cfg.batch, cfg.cin) + sp
    img = _hash_uniform(int(np.prod(shape)), 4321 + cfg.seed).reshape(shape) * np.float32(np.sqrt(3.0))
    grid = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in sp], indexing="ij")
    lab = np.zeros((cfg.batch, 1) + sp, np.float32)
    for b in range(cfg.batch):
        c = [s * (0.35 + 0.3 * ((b * 7 + i * 3 + cfg.seed) % 5) / 4.0) for i, s in enumerate(sp)]
        r = np.sqrt(sum(((g - ci) / (0.75 * s)) ** 2 for g, ci, s in zip(grid, c, sp)))
        lab[b, 0] = np.clip(np.floor(cfg.K * (1.0 - r)), 0, cfg.K - 1)
    return torch.from_numpy(img), torch.from_numpy(lab)


# ------------------------------------------------------------------------------------------------ oracle
def make_ref(cfg: Cfg, dtype=torch.float64, state=None) -> RefUNet:
    ref = RefUNet(cfg.dims, cfg.cin, cfg.K, cfg.channels, cfg.strides, dropout=cfg.dropout, act=cfg.act)
    if state is None:
        deterministic_fill_(ref, cfg.seed)
    else:
        ref.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
    return ref.to(dtype)


def initial_state(cfg: Cfg) -> "OrderedDict[str, torch.Tensor]":
    """the f32 weights every implementation starts from"""
    return OrderedDict((k, v.clone()) for k, v in make_ref(cfg, torch.float32).state_dict().items())


def oracle_step(cfg: Cfg, img, lab, dtype=torch.float64, ref=None, loss_fn=ref_dice_loss):
    """one training step in the reference's order (forward, zero_grad, Dice, backward, Adam lr=1e-4).  ``ref``: a
    prepared (possibly deliberately wrong) module; ``loss_fn``: likewise.  Returns the step's quantities on the CPU."""
    ref = make_ref(cfg, dtype) if ref is None else ref
    ref.train()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    out = ref(img.to(dtype))
    opt.zero_grad()
    loss = loss_fn(out, lab)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    opt.step()
    return {"logits": out.detach(), "loss": float(loss.detach()), "grads": grads,
            "state": OrderedDict((k, v.detach().clone()) for k, v in ref.state_dict().items()),
            "params": {n: p.detach().clone() for n, p in ref.named_parameters()}, "module": ref}


def wobbled_oracle_step(cfg: Cfg, img, lab, trial: int):
    """The float64 oracle step on an input moved by a relative 2^-24 (seeded by ``trial``), with every convolution,
    BatchNorm and activation output rounded to float32 on the way: what ANY f32 implementation may see.  An entry whose
    float64 gradients move by a good part of a gate under this is ill conditioned (several seeds of the ring-sized
    default ladder jump by 1-2x the gate: a discrete event in the graph, not rounding that averages out)."""
    g = torch.Generator().manual_seed(1000 + trial)
    x = img.double() * (1 + (torch.rand(img.shape, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** -23)
    ref = make_ref(cfg)
    kinds = (nn.Conv2d, nn.Conv3d, nn.ConvTranspose2d, nn.ConvTranspose3d, nn.BatchNorm2d, nn.BatchNorm3d, nn.PReLU,
             nn.ReLU, nn.LeakyReLU)
    for m in ref.modules():
        if isinstance(m, kinds):
            m.register_forward_hook(lambda _m, _i, o: o + (o.float().double() - o).detach())
    return oracle_step(cfg, x, lab, ref=ref)


def oracle_eval(cfg: Cfg, state, img, dtype=torch.float64):
    """folded-BN (eval mode) forward of the oracle holding ``state``"""
    ref = make_ref(cfg, dtype, state).eval()
    with torch.no_grad():
        return ref(img.to(dtype))


# ------------------------------------------------------------------------------------------------ gates
def rel(a, b) -> float:
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-20))


def biases_under_batchnorm(names):
    """convolution biases followed by a training-mode BatchNorm: their gradient is identically zero in exact
    arithmetic (the normalisation removes any per-channel constant), so whatever an implementation reports is its own
    summation noise (the engine writes an exact 0)"""
    names = set(names)
    return sorted(n for n in names
                  if n.endswith(".conv.bias") and n[:-len("conv.bias")] + "adn.N.weight" in names)


def f32_step_violations(got, ref, scale: float = 1.0, skip=()):
    """The f32 gates of ``test_train_step_parity_f32`` (tests/test_unet_gpu.py) with ``ref`` = the float64 oracle;
    every tolerance times ``scale`` (1 for the engine, 1/4 for the conditioning check).  Returns
    [(gate, name, value, limit)] of what is over."""
    bad = []

    def gate(name, what, value, limit):
        if not value <= limit:                      # NaN fails
            bad.append((name, what, value, limit))

    gate("logits", "", rel(got["logits"], ref["logits"]), 2e-4 * scale)
    gate("loss", "", abs(got["loss"] - ref["loss"]), 1e-4 * scale * abs(ref["loss"]))
    gr_all = ref["grads"]
    gmax = max(float(g.abs().max()) for g in gr_all.values())
    assert set(got["grads"]) == set(gr_all)
    for n, gr in gr_all.items():
        if n in skip:
            continue
        err = float((got["grads"][n].double() - gr.double()).abs().max())
        rtol = 2e-2 if (n.endswith(".A.weight") or n.endswith(".bias")) else 2e-3
        gate("grad", n, err, scale * (rtol * float(gr.abs().max()) + 2e-6 * gmax))
    for k, r in ref["state"].items():
        v = got["state"][k]
        if not r.dtype.is_floating_point:
            gate("num_batches_tracked", k, abs(int(v) - int(r)), 0)
        elif "running" in k:
            gate("running", k, rel(v, r), 1e-4 * scale)
    for n, gr in gr_all.items():
        mask = gr.abs() > 1e-3 * gmax               # Adam's first step is lr * sign(g): skip rounding-noise gradients
        if mask.any():
            d = float((ref["params"][n].double() - got["params"][n].double())[mask].abs().max())
            gate("adam", n, d, 5e-6 * scale)
    return bad


def f32_eval_violations(out, out_ref, scale: float = 1.0):
    """The gates of ``test_eval_forward_folded_bn_f32``: 2e-4 relative, arg-max flips only at exact near-ties."""
    bad = []
    if tuple(out.shape) != tuple(out_ref.shape):
        return [("shape", "", tuple(out.shape), tuple(out_ref.shape))]
    e = rel(out, out_ref)
    if not e <= 2e-4 * scale:
        bad.append(("logits", "", e, 2e-4 * scale))
    mism = torch.argmax(out.double(), 1) != torch.argmax(out_ref.double(), 1)
    if mism.any():
        top2 = torch.topk(out_ref, 2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1])[mism].max())
        if not gap < 1e-4 * scale * float(out_ref.abs().max()):
            bad.append(("argmax-gap", "", gap, 1e-4 * scale * float(out_ref.abs().max())))
    frac = float(mism.float().mean())
    if not frac < 1e-4 * scale:
        bad.append(("argmax-frac", "", frac, 1e-4 * scale))
    return bad


def argmax_agreement(out, out_ref) -> float:
    return float((torch.argmax(out.double(), 1) == torch.argmax(out_ref.double(), 1)).float().mean())


# ------------------------------------------------------------------------------------------------ 16-bit emulation
def emulate_lowp(cfg: Cfg, state, img, dtype, train: bool):
    """Float64 oracle holding ``state`` with every tensor the engine STORES rounded to ``dtype`` (bf16 / fp16): the
    input, each convolution's output, each BatchNorm + activation output, each residual sum; and the convolution
    weights, which are 16-bit MFMA operands.  Accumulation stays exact, as the kernels' is f32.  Returns logits."""
    def q(t):
        return t.to(dtype).double()

    ref = make_ref(cfg, torch.float64, state)
    convs = (nn.Conv2d, nn.Conv3d, nn.ConvTranspose2d, nn.ConvTranspose3d)
    hooks = []
    for m in ref.modules():
        if isinstance(m, convs):
            if m.weight.shape[0] % 16 == 0 and m.weight.shape[1] % 16 == 0:      # MFMA layers pack 16-bit operands
                m.weight.data = q(m.weight.data)
            hooks.append(m.register_forward_hook(lambda _m, _i, o: q(o)))
        elif isinstance(m, (_ADN, _ResidualUnit)):
            hooks.append(m.register_forward_hook(lambda _m, _i, o: q(o)))
    ref.train(train)
    with torch.no_grad():
        out = ref(q(img.double()))
    for h in hooks:
        h.remove()
    return out


# ------------------------------------------------------------------------------------------------ engine
def make_net(cfg: Cfg, state, precision):
    from segmantic_amd.seg.monai_unet import Net
    net = Net(num_classes=cfg.K, num_channels=cfg.cin, spatial_dims=cfg.dims, channels=cfg.channels,
              strides=cfg.strides, dropout=cfg.dropout, act=cfg.act)
    net.load_state_dict({"_model." + k: v.clone() for k, v in state.items()})
    net.mixed_precision = precision
    return net


def engine_step(cfg: Cfg, state, img, lab, precision, census: "Census" = None, with_eval: bool = True):
    """``Net`` on the GPU: one ``training_step`` from ``state`` in ``precision`` (False / True = bf16 / "fp16"), then
    an eval forward on the same images with the weights and running statistics the step left.  Reads what
    ``test_train_step_parity_f32`` reads: ``eng._bufs``, ``p.grad``, ``state_dict()``.  fp16 gradients are unscaled."""
    net = make_net(cfg, state, precision)
    net.to(DEV).train()
    eng = net._engine_for()
    if census is not None:
        census.note("kpad != K", eng.kpad != cfg.K)
        census.note("carry deeper than the net", len(eng._carry_lvls) < max(1, eng.carry_levels))
    x, y = img.to(DEV), lab.to(DEV)
    res = net.training_step({"image": x, "label": y})
    torch.cuda.synchronize()
    logits = eng._bufs["logits.t"][..., :cfg.K].float().cpu().permute(0, 4, 1, 2, 3)
    if cfg.dims == 2:
        logits = logits.squeeze(2)
    scale = net.grad_scaler().get_scale() if precision == "fp16" else 1.0
    out = {"logits": logits.contiguous(), "loss": float(res["loss"].cpu()), "grad_scale": scale,
           "grads": {n: p.grad.detach().cpu().clone() / scale for n, p in net._model.named_parameters()},
           "state": OrderedDict((k, v.detach().cpu().clone()) for k, v in net._model.state_dict().items()),
           "params": {n: p.detach().cpu().clone() for n, p in net._model.named_parameters()},
           "dtype": eng.dtype}
    if precision == "fp16":
        out["skipped_steps"] = net.grad_scaler().skipped_steps()
    if with_eval:
        net.eval()
        if census is not None:
            net.window_views_ok(eng.dtype)           # a host query of the plan (sliding windows are tested elsewhere)
        with torch.no_grad():
            ev = net(x)
        torch.cuda.synchronize()
        out["eval_logits"] = ev.float().cpu().contiguous()
        out["eval_top_fused"] = bool(net._engine.eval_top_fused)
    return out


def engine_forward(cfg: Cfg, state, img, precision, train: bool):
    """forward only (no step): logits [B, K, *spatial] f32 on the CPU"""
    net = make_net(cfg, state, precision)
    net.to(DEV).train(train)
    with torch.no_grad():
        out = net(img.to(DEV))
    torch.cuda.synchronize()
    return out.float().cpu().contiguous()


# ------------------------------------------------------------------------------------------------ census
# The k3 families ``segmi_conv3d_fwd_kernel_name`` can name (csrc/conv.hip), storage type dropped
FAMILIES = ("conv_ring3", "conv_ring2 NT=1", "conv_ring2 NT=2", "conv_fwd_ks", "conv_fwd_mfma CK=16 s1",
            "conv_fwd_mfma CK=16 s2", "conv_fwd_mfma CK=32 s1", "conv_fwd_mfma CK=32 s2", "conv_small_fwd", "conv_direct")

OPS_PREDICATES = ("conv3d_pair_ok", "conv3d_in_affine_ok", "conv3d_bn_bwd_sums_ok", "conv3d_split_act_ok",
                  "bn_act_bwd_fused_ok", "bn_act_bwd_apply_conv_ok", "dectop_ok")
ENGINE_PREDICATES = ("_pair_ok", "_tf_ok", "_bsum_ok", "window_views_ok")
NOTES = ("kpad != K",)

# Branches no legal network reaches (at most three; each a (name, outcome) the census test does not require)
UNREACHABLE = {
    "conv_fwd_mfma CK=32 s1":
        "CK=32 needs 16-bit storage and Cin % 32 == 0; every such k3 stride-1 layer satisfies conv_ks_ok (one k-step "
        "per tap) and is taken by conv_fwd_ks (or a ring kernel) first -- the name exists for the k1 residual "
        "convolutions only, which are not k3 layers",
    "conv3d_split_act_ok=False":
        "both call sites (_train_pair, _merged_eval) ask only for MFMA k3 stride-2 pairs, and for those the predicate "
        "is true by construction: the k-split and ring families (conv_plan.h), its two exclusions, are stride-1 "
        "only.  The engine's own guards in front of it (non-MFMA, carried, no residual convolution) do go both ways",
}


def family_of(kernel_name: str) -> str:
    """'conv_ring2_kernel<bf16, CK=32, NT=2>' -> 'conv_ring2 NT=2' etc.; k1 layers -> 'k1'"""
    m = re.match(r"(\w+?)_kernel<([^>]*)>", kernel_name)
    if not m:
        return kernel_name
    base, args = m.group(1), m.group(2)
    if base == "conv_ring2":
        return "conv_ring2 " + re.search(r"NT=\d", args).group(0)
    if base == "conv_fwd_mfma":
        k = re.search(r"k(\d) s(\d)", args)
        if k.group(1) != "3":
            return "k1"
        ck = re.search(r"CK=\d+", args).group(0)
        return f"conv_fwd_mfma {ck} s{k.group(2)}"
    if base == "conv_fwd_ks":
        return "conv_fwd_ks"
    return base


class Census:
    """Observes the dispatch decisions of one or more engine runs.  ``with census.watch(label):`` patches, by plain
    attribute assignment, the ``ops.*_ok`` predicates, ``ops.conv3d_fwd_kernel_name`` and the convolution entry points
    that stand for one launch each (which then ask ``conv3d_fwd_kernel_name`` what runs for their layer), and the
    engine's ``_pair_ok`` / ``_tf_ok`` / ``_bsum_ok`` / ``window_views_ok``.  Every wrapper returns what the wrapped
    function returns; nothing else is changed and no environment variable is read or set."""

    def __init__(self):
        self.rows = []          # (label, kind, name, outcome, layer)
        self._label = None

    def note(self, name, outcome):
        self.rows.append((self._label, "note", name, bool(outcome), ""))

    @staticmethod
    def _shape(t):
        return "x".join(str(int(s)) for s in t.shape)

    @contextmanager
    def watch(self, label):
        from segmantic_amd import ops
        from segmantic_amd.seg.unet import UNetEngine
        self._label = label
        saved = []

        def patch(obj, name, new):
            saved.append((obj, name, obj.__dict__[name] if isinstance(obj, type) else getattr(obj, name)))
            setattr(obj, name, new)

        def wrap_pred(obj, name, kind, layer_of):
            orig = obj.__dict__[name] if isinstance(obj, type) else getattr(obj, name)

            def w(*a, **k):
                r = orig(*a, **k)
                self.rows.append((label, kind, name, bool(r), layer_of(a)))
                return r
            patch(obj, name, w)

        for name in OPS_PREDICATES:
            wrap_pred(ops, name, "ops", lambda a: self._shape(a[0]) + "->" + self._shape(a[1]))
        wrap_pred(UNetEngine, "_pair_ok", "engine", lambda a: a[1]["prefix"])
        wrap_pred(UNetEngine, "_tf_ok", "engine", lambda a: a[3].prefix)
        wrap_pred(UNetEngine, "_bsum_ok", "engine", lambda a: a[1].prefix)
        wrap_pred(UNetEngine, "window_views_ok", "engine", lambda a: "")

        name_orig = ops.conv3d_fwd_kernel_name

        def kname(x, y, ksize, stride):
            r = name_orig(x, y, ksize, stride)
            self.rows.append((label, "family", family_of(r), True, self._shape(x) + "->" + self._shape(y)))
            return r
        patch(ops, "conv3d_fwd_kernel_name", kname)

        def wrap_launch(name, ks_of):
            orig = getattr(ops, name)

            def w(*a, **k):
                ksize, stride = ks_of(a, k)
                ops.conv3d_fwd_kernel_name(a[0], a[1], ksize, stride)
                return orig(*a, **k)
            patch(ops, name, w)

        wrap_launch("conv3d_fwd", lambda a, k: (a[6], a[7]))
        wrap_launch("conv3d_fwd_split_act", lambda a, k: (a[6], a[7]))
        wrap_launch("conv3d_fwd_pair", lambda a, k: (3, a[7]))       # runs conv_small_fwd for both halves

        back_orig = UNetEngine.__dict__["backward"]

        def backward(eng, *a, **k):
            r = back_orig(eng, *a, **k)
            self.rows.append((label, "note", "weight gradients carried", bool(r), ""))
            return r
        patch(UNetEngine, "backward", backward)
        try:
            yield self
        finally:
            for obj, name, orig in reversed(saved):
                setattr(obj, name, orig)
            self._label = None

    # -------------------------------------------------------------------------------- summaries
    def outcomes(self, name):
        return {r[3] for r in self.rows if r[2] == name and r[1] != "family"}

    def families(self):
        return {r[2] for r in self.rows if r[1] == "family"}

    def table(self) -> str:
        """per run: families taken and, per predicate, how often it said yes / no"""
        labels = list(OrderedDict.fromkeys(r[0] for r in self.rows))
        preds = list(OPS_PREDICATES) + list(ENGINE_PREDICATES) + ["kpad != K", "weight gradients carried",
                                                                  "carry deeper than the net"]
        lines = []
        for lb in labels:
            mine = [r for r in self.rows if r[0] == lb]
            fam = sorted({r[2] for r in mine if r[1] == "family"})
            lines.append(f"{lb}\n    families: {', '.join(fam)}")
            cells = []
            for p in preds:
                t = sum(1 for r in mine if r[2] == p and r[1] != "family" and r[3])
                f = sum(1 for r in mine if r[2] == p and r[1] != "family" and not r[3])
                if t or f:
                    cells.append(f"{p} {t}T/{f}F")
            lines.append("    " + "; ".join(cells))
        return "\n".join(lines)
