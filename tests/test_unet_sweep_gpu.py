"""The UNet training step and eval forward against a float64 oracle, over the configurations of
tests/helpers/unet_sweep.py: non-cubic extents, batch 1 / 3 / 8, several channel ladders, input-channel and class
counts, ReLU / LeakyReLU, a 2-D network -- chosen so that every dispatch decision of segmantic_amd/seg/unet.py is taken
both ways (``test_sweep_takes_every_dispatch_branch``).  The f32 gates are those of tests/test_unet_gpu.py, the 16-bit
ones those of tests/test_unet_gpu.py and tests/test_fp16_gpu.py; tests/test_unet_sweep_host.py shows that the entries are
well conditioned and that the gates notice six kinds of wrong implementation."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import unet_sweep as us  # noqa: E402

CFG = {c.name: c for c in us.SWEEP}
PRECISIONS = {"f32": False, "bf16": True, "fp16": "fp16"}
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16}
CASES = [(c.name, p) for c in us.SWEEP for p in PRECISIONS]
CASE_IDS = [f"{n}-{p}" for n, p in CASES]


@functools.lru_cache(maxsize=None)
def truth(name):
    """(image, label, initial weights, float64 oracle step) of a sweep entry, computed once per session"""
    cfg = CFG[name]
    img, lab = us.make_batch(cfg)
    r = us.oracle_step(cfg, img, lab)
    r.pop("module")
    return img, lab, us.initial_state(cfg), r


@functools.lru_cache(maxsize=None)
def engine(name, prec):
    img, lab, state0, _ = truth(name)
    return us.engine_step(CFG[name], state0, img, lab, PRECISIONS[prec])


@functools.lru_cache(maxsize=None)
def eval_truth(name, prec):
    """float64 eval forward of the oracle holding the weights and running statistics the ENGINE holds after its step"""
    return us.oracle_eval(CFG[name], engine(name, prec)["state"], truth(name)[0])


@functools.lru_cache(maxsize=None)
def emulation(name, prec, train):
    """(relative logit error, arg-max agreement) against the float64 oracle of the CPU emulation that rounds every stored
    tensor to the 16-bit type: measured on the reference, never on the engine"""
    img = truth(name)[0]
    if train:
        state, ref = truth(name)[2], truth(name)[3]["logits"]
    else:
        state, ref = engine(name, prec)["state"], eval_truth(name, prec)
    out = us.emulate_lowp(CFG[name], state, img, STORAGE[prec], train)
    return us.rel(out, ref), us.argmax_agreement(out, ref)


def lowp_forward_gate(err, agree, tol, min_agree, emu):
    """the stated tolerance of the default network, or -- where an entry needs more -- twice the emulation's error
    (a different accumulation order inside each layer, not a different rounding scheme)"""
    e_emu, a_emu = emu
    assert err < max(tol, 2.0 * e_emu), (err, tol, e_emu)
    if min_agree is not None:
        assert 1.0 - agree < max(1.0 - min_agree, 2.0 * (1.0 - a_emu)), (agree, min_agree, a_emu)


# ------------------------------------------------------------------------------------------------ training step
@pytest.mark.parametrize("name,prec", CASES, ids=CASE_IDS)
def test_train_step_matches_float64_oracle(name, prec, record_property):
    _, _, _, ref = truth(name)
    got = engine(name, prec)
    err = us.rel(got["logits"], ref["logits"])
    print(f"\n{name} {prec}: logits rel {err:.3e}, loss {got['loss']:.6f} (oracle {ref['loss']:.6f})")
    if prec == "f32":
        # the gates of test_train_step_parity_f32, unchanged, against float64
        bad = us.f32_step_violations(got, ref)
        assert not bad, bad[:8]
        return
    emu = emulation(name, prec, True)
    agree = us.argmax_agreement(got["logits"], ref["logits"])
    record_property(f"{prec}_train_emulation_rel_err", emu[0])
    record_property(f"{prec}_train_emulation_argmax_agreement", emu[1])
    record_property(f"{prec}_train_rel_err", err)
    print(f"    arg-max agreement {agree:.5f}; emulation: rel {emu[0]:.3e}, agreement {emu[1]:.5f}")
    if prec == "bf16":
        # test_bf16_path_close_to_f32_oracle (tests/test_unet_gpu.py): 2e-2 / 98.5 % / loss within 1e-4
        lowp_forward_gate(err, agree, 2e-2, 0.985, emu)
        assert abs(got["loss"] - ref["loss"]) < 1e-4
        return
    # fp16: test_fp16_network_is_closer_to_the_oracle_than_bf16 and test_fp16_training_step_matches_the_oracle_step
    # (tests/test_fp16_gpu.py)
    b = engine(name, "bf16")
    eb, ab = us.rel(b["logits"], ref["logits"]), us.argmax_agreement(b["logits"], ref["logits"])
    lowp_forward_gate(err, None, 0.25 * eb, None, emu)
    assert agree >= ab or 1.0 - agree <= 2.0 * (1.0 - emu[1]), (agree, ab, emu[1])
    assert got["skipped_steps"] == 0 and got["grad_scale"] == 2.0 ** 16
    assert abs(got["loss"] - ref["loss"]) < 1e-4 * abs(ref["loss"])
    gmax = max(float(g.abs().max()) for g in ref["grads"].values())
    bad, num, den = [], 0.0, 0.0
    for n, gr in ref["grads"].items():
        g, gr = got["grads"][n].double(), gr.double()
        num, den = num + float(((g - gr) ** 2).sum()), den + float((gr ** 2).sum())
        if n.endswith(".A.weight") or n.endswith(".bias"):
            continue
        e = float((g - gr).norm() / gr.norm().clamp(min=1e-30))
        if e > 0.1:
            bad.append((n, e))
    print(f"    arena gradient rel. error {math.sqrt(num / den):.3e}")
    record_property("fp16_arena_gradient_rel_err", math.sqrt(num / den))
    assert math.sqrt(num / den) < 3e-2
    assert not bad, bad[:8]
    for k, r in ref["state"].items():
        if "running" in k:
            assert us.rel(got["state"][k], r) < 2e-3, k
    for n, gr in ref["grads"].items():
        mask = gr.abs() > 1e-2 * gmax
        if mask.any():
            d = (ref["params"][n].double() - got["params"][n].double())[mask].abs().max()
            assert float(d) < 5e-6, (n, float(d))


# ------------------------------------------------------------------------------------------------ eval forward
@pytest.mark.parametrize("name,prec", CASES, ids=CASE_IDS)
def test_eval_forward_matches_float64_oracle(name, prec, record_property):
    """folded-BatchNorm forward AFTER the training step (the running statistics are not the initial ones), against the
    float64 oracle holding exactly what the engine holds"""
    got = engine(name, prec)
    out, out_ref = got["eval_logits"], eval_truth(name, prec)
    err = us.rel(out, out_ref)
    print(f"\n{name} {prec}: eval logits rel {err:.3e}, fused decoder top: {got['eval_top_fused']}")
    assert tuple(out.shape) == tuple(out_ref.shape)
    if prec == "f32":
        bad = us.f32_eval_violations(out, out_ref)          # test_eval_forward_folded_bn_f32
        assert not bad, bad
        return
    emu = emulation(name, prec, False)
    agree = us.argmax_agreement(out, out_ref)
    record_property(f"{prec}_eval_emulation_rel_err", emu[0])
    record_property(f"{prec}_eval_emulation_argmax_agreement", emu[1])
    record_property(f"{prec}_eval_rel_err", err)
    print(f"    arg-max agreement {agree:.5f}; emulation: rel {emu[0]:.3e}, agreement {emu[1]:.5f}")
    if prec == "bf16":
        lowp_forward_gate(err, agree, 2e-2, 0.985, emu)      # test_bf16_path_close_to_f32_oracle[False]
    else:
        lowp_forward_gate(err, None, 3e-3, None, emu)        # test_fp16_eval_forward_..._matches_the_oracle


# ------------------------------------------------------------------------------------------------ dispatch census
def test_sweep_takes_every_dispatch_branch():
    """Self-contained: every entry, one training step + one eval forward, in bf16 and in f32, under the census."""
    census = us.Census()
    for cfg in us.SWEEP:
        img, lab = us.make_batch(cfg)
        state0 = us.initial_state(cfg)
        for prec in ("bf16", "f32"):
            with census.watch(f"{cfg.name} [{prec}]"):
                us.engine_step(cfg, state0, img, lab, PRECISIONS[prec], census=census)
    print("\n" + census.table())
    fams = census.families()
    missing = [f for f in us.FAMILIES if f not in fams and f not in us.UNREACHABLE]
    assert not missing, f"convolution families no layer of the sweep took: {missing}"
    reached = [f for f in us.FAMILIES if f in fams and f in us.UNREACHABLE]
    assert not reached, f"listed as unreachable, but taken: {reached}"
    one_sided = []
    for name in us.OPS_PREDICATES + us.ENGINE_PREDICATES + us.NOTES:
        seen = census.outcomes(name)
        for want in (True, False):
            listed = f"{name}={want}" in us.UNREACHABLE
            if want not in seen and not listed:
                one_sided.append(f"{name} never {want}")
            if want in seen and listed:
                one_sided.append(f"{name}={want} is listed as unreachable, but occurred")
    assert not one_sided, one_sided
    assert len(us.UNREACHABLE) <= 3


def test_stride1_level_is_refused():
    """no ladder with a stride-1 level is legal: the engine says so instead of computing something else"""
    cfg = us.STRIDE1_REFUSED
    net = us.make_net(cfg, us.initial_state(cfg), False).to(us.DEV)
    with pytest.raises(NotImplementedError, match="stride-2"):
        net._engine_for()
