#!/usr/bin/env python3
"""Records tests/golden/engine_schedule_parent.json: the launch schedule of ``UNetEngine`` -- every ``ops.*`` call with
its operands (tensor identity, offset, shape, stride, dtype, scalars), the stream it is issued on and the event /
stream ordering edges between them (tests/helpers/engine_trace.py) -- for ten configurations, each through two
consecutive ``Net.training_step`` calls and one eval forward.  ``libsegmi.so`` computes a function of exactly these
calls, so an engine that reproduces the file computes what the recorded one computed, with the same kernels.

The file was recorded from the commit BEFORE the residual-unit paths of segmantic_amd/seg/unet.py were unified, and
tests/test_engine_schedule_gpu.py holds every later engine to it: it is regenerated only when the schedule is changed
on purpose.  Needs an MI355X.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_engine_schedule_goldens.py
"""
import inspect
import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from oracle.unet_ref import synthetic_batch  # noqa: E402
from segmantic_amd import ops  # noqa: E402
from segmantic_amd.seg.monai_unet import Net  # noqa: E402
from tests.helpers import engine_trace  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "engine_schedule_parent.json"
DEV = "cuda:0"
FUSION_FLAGS = ("fuse_bn_apply", "fuse_bn_bwd", "fuse_bn_bwd_small", "fuse_apply_conv", "merge_eval_pairs",
                "fuse_eval_top", "carry_top_wgrad")
DEEP = dict(channels=(16, 32, 64, 128), strides=(2, 2, 2))

# name -> network, precision (Net.mixed_precision), engine attributes, (batch, extent).  64^3 batch 4 is where the
# 16-channel layers take the ring kernels (BatchNorm apply in the consumer's staging, BatchNorm-backward sums in the
# input-gradient epilogue); the launch sequence of the other configurations does not depend on the extent, 32^3 keeps
# them short
CONFIGS = {
    "a bf16": dict(net=dict(num_classes=16, **DEEP), precision=True, size=(4, 64)),
    "b f32": dict(net=dict(num_classes=16, **DEEP), precision=False, size=(2, 32)),
    "c fp16": dict(net=dict(num_classes=16, **DEEP), precision="fp16", size=(2, 32)),
    "d kpad dropout": dict(net=dict(num_classes=3, channels=(16, 32, 64), strides=(2, 2), dropout=0.1), precision=True,
                           size=(2, 32)),
    "e fixed slope": dict(net=dict(num_classes=16, act="LEAKYRELU", **DEEP), precision=True, size=(2, 32)),
    "f one stream": dict(net=dict(num_classes=16, **DEEP), precision=True, size=(2, 32), flags=dict(overlap_wgrad=False)),
    "g grad hook": dict(net=dict(num_classes=16, **DEEP), precision=True, size=(2, 32), hook=True),
    "h unfused": dict(net=dict(num_classes=16, **DEEP), precision=True, size=(4, 64),
                      flags={f: False for f in FUSION_FLAGS}),
    # (equal channels at the bottom: its unit has an identity residual, whose input gradient is summed by `add`)
    "i 2-D": dict(net=dict(num_classes=16, spatial_dims=2, channels=(16, 32, 32), strides=(2, 2)), precision=True,
                  size=(2, 64)),
    "j windows": dict(net=dict(num_classes=16, **DEEP), precision=True, size=(2, 32), windows=True),
}


def run_config(cfg) -> list:
    """the events of one configuration"""
    torch.manual_seed(0)
    net = Net(**cfg["net"]).to(DEV)
    net.mixed_precision = cfg["precision"]
    eng = net._engine_for()
    for flag, value in cfg.get("flags", {}).items():
        assert hasattr(eng, flag), flag
        setattr(eng, flag, value)
    hooked = []
    if cfg.get("hook"):
        eng.grad_hook = lambda lo, events: hooked.append((lo, len(events)))
    batch, size = cfg["size"]
    dims = cfg["net"].get("spatial_dims", 3)
    img, lab = synthetic_batch(batch, size, cfg["net"]["num_classes"], seed=5, dims=dims)
    img, lab = img.to(DEV), lab.to(DEV)
    torch.cuda.synchronize()
    with engine_trace.record() as trace, torch.no_grad():
        if cfg.get("windows"):
            # eval only: windows read in place from a volume, into a caller's buffer, on the second lane
            net.eval()
            volume = img[0, 0].to(eng.dtype).contiguous()
            starts = [(0, 0, 0), (0, 0, size // 2), (size // 2, size // 2, 0)]
            roi = (size // 2,) * 3
            assert eng.window_views_ok(volume.dtype) and ops.WindowBatch.eligible(volume.shape, starts, roi)
            out = torch.empty((len(starts),) + roi + (eng.kpad,), dtype=eng.dtype, device=DEV)
            eng.forward(ops.WindowBatch(volume, starts, roi), train=False, out=out, lane=1)
            eng.forward(img, train=False, out=torch.empty((batch,) + (size,) * 3 + (eng.kpad,), dtype=eng.dtype,
                                                          device=DEV), lane=1)
        else:
            net.train()
            net.training_step({"image": img, "label": lab})
            net.training_step({"image": img, "label": lab})
            net.eval()
            net(img)
        torch.cuda.synchronize()
    assert bool(hooked) == bool(cfg.get("hook"))
    return trace.events


# ------------------------------------------------------------------------------------------------ census
def _arg(event, param):
    """the canonical value of parameter `param` of an op event"""
    names = list(inspect.signature(getattr(ops, event[1])).parameters)
    return event[3][1 + names.index(param)]


def _is(name, **given):
    """predicate: an event of op `name` whose named parameters are given (True) / None (False) / equal to a value"""
    def test(ev):
        if ev[1] != name:
            return False
        for param, want in given.items():
            v = _arg(ev, param)
            if isinstance(want, bool):
                if (v is not None) != want:
                    return False
            elif v != want:
                return False
        return True
    return test


def _reduce_then_apply(events):
    names = [e[1] for e in events]
    return any(a == "bn_act_bwd_reduce" and b == "bn_act_bwd_apply" for a, b in zip(names, names[1:]))


def _carried_wgrad(events):
    """a weight gradient issued on its stream after the main stream's ``wait_stream`` on that stream and before the
    step's optimiser launch: the step's own chain does not wait for it"""
    joined = set()
    for ev in events:
        if ev[1] == "Stream.wait_stream":
            joined.add(ev[3][2][1])
        elif ev[1].endswith(("_step", "_step_amp")):
            joined.clear()
        elif ev[1] == "conv3d_wgrad" and ev[2] in joined:
            return True
    return False


def _any(test):
    return lambda events: any(test(e) for e in events)


CENSUS = {
    "conv3d_fwd_pair with stats_a": _any(_is("conv3d_fwd_pair", stats_a=True)),
    "conv3d_fwd_pair without stats_a": _any(_is("conv3d_fwd_pair", stats_a=False)),
    "conv3d_fwd_split_act with stats": _any(_is("conv3d_fwd_split_act", stats=True)),
    "conv3d_fwd_split_act without stats": _any(_is("conv3d_fwd_split_act", stats=False)),
    "conv3d_fwd with in_tf": _any(_is("conv3d_fwd", in_tf=True)),
    "conv3d_fwd with bn_bwd": _any(_is("conv3d_fwd", bn_bwd=True)),
    # input gradients carry no bias; the stride-2 conv without one is the transposed convolution's
    "conv3d_fwd as a transposed conv's input gradient": _any(_is("conv3d_fwd", bias=False, stride=2)),
    "convT3d_fwd as a forward": _any(_is("convT3d_fwd", bias=True)),
    "convT3d_fwd as a stride-2 input gradient": _any(_is("convT3d_fwd", bias=False)),
    "bn_act_fwd with a residual": _any(_is("bn_act_fwd", residual=True)),
    "bn_act_fwd without a residual": _any(_is("bn_act_fwd", residual=False)),
    "bn_act_bwd_fused": _any(_is("bn_act_bwd_fused")),
    "bn_act_bwd_reduce followed by bn_act_bwd_apply": _reduce_then_apply,
    "bn_act_bwd_apply_conv": _any(_is("bn_act_bwd_apply_conv")),
    "dectop_fwd": _any(_is("dectop_fwd")),
    "add": _any(_is("add")),
    # the bias gradient of the convolution that produces the logits: filled by the loss backward that walks dlogits
    # anyway.  (``ops.bias_grad`` itself has no caller a network can reach: the engine issues it only for a transposed
    # convolution that does not feed a BatchNorm, and every transposed convolution of this UNet does.)
    "bias_grad": lambda evs: any(e[1] == "bias_grad" or (e[1].endswith("_bwd") or e[1].endswith("_bwd_amp"))
                                 and "bias_grad" in inspect.signature(getattr(ops, e[1])).parameters
                                 and _arg(e, "bias_grad") is not None for e in evs),
    "a carried conv3d_wgrad": _carried_wgrad,
    # (a trace starts on the caller's stream)
    "WpackBatch.run on a non-default stream": lambda evs: any(e[1] == "WpackBatch.run" and e[2] != evs[0][2] for e in evs),
}


def census_missing(traces: dict) -> list:
    """the census items no trace contains"""
    return [item for item, found in CENSUS.items() if not any(found(evs) for evs in traces.values())]


def main():
    traces = {}
    for name, cfg in CONFIGS.items():
        traces[name] = run_config(cfg)
        print(f"{name:16s} {len(traces[name]):5d} events")
    missing = census_missing(traces)
    if missing:
        sys.exit(f"not written: no configuration reaches {missing}")
    text = engine_trace.dumps(engine_trace.encode(traces))
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN
    out.write_text(text)
    print(f"{len(text)} bytes -> {out}")


if __name__ == "__main__":
    main()
