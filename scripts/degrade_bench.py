"""``augment_degrade`` benchmark: the sampler's ``make_batch`` for --patches patches of --roi^3 (two seeded
--size^3 volumes, plain crops, no intensity transforms) with the option off and with every transform forced on
(``prob: 1``), and ``ops.degrade_augment`` alone on the same patch buffer, one transform at a time and all four.

Device events around each call, the median of --repeats runs after one warm-up, one process.  Byte model per
patch element (f32): the in-place pointwise pass reads and writes it once, 8 bytes; a blur or a lowres is one
out-of-place pass, and a patch that takes only one of them is copied back from the workspace, 16 bytes; blur and
lowres together are the two out-of-place passes, 16 bytes.  Halo and tap re-reads are served by the caches and not
counted.

    python scripts/degrade_bench.py [--size 160] [--roi 128] [--patches 8] [--channels 1] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def _timed(fn, repeats: int):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(repeats + 1):                   # the first run is the warm-up
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms[1:])), "ms_all": [round(float(v), 3) for v in ms[1:]]}


def _cache(size: int, channels: int, classes: int, device, seed: int):
    """two synthetic cached volumes, built the way bench.py's fit mode builds them"""
    import torch
    from segmantic_amd.seg import streams, trainer
    cache = trainer.CachedVolumes.__new__(trainer.CachedVolumes)
    cache.items, cache.device = [], torch.device(device)
    cache._stream = streams.shared_stream(device, streams.AUX)
    cache._pinned = torch.empty(4096, dtype=torch.int64).pin_memory()
    g = torch.Generator(device=device).manual_seed(seed)
    for _ in range(2):
        img = torch.randn((channels, size, size, size), generator=g, device=device)
        lab = torch.randint(0, classes, (1, size, size, size), generator=g, device=device).float()
        flat = lab.reshape(-1).long()
        idx = [torch.nonzero(flat == c).reshape(-1) for c in range(classes)]
        counts = np.array([int(t.numel()) for t in idx], dtype=np.int64)
        cache.items.append({"image": img, "label": lab, "class_all": torch.cat(idx), "class_counts": counts,
                            "class_offsets": np.concatenate([[0], np.cumsum(counts)[:-1]]),
                            "image_ndhwc": img.permute(1, 2, 3, 0).contiguous()[None],
                            "label_dhw": lab[0].contiguous()})
    return cache


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=160)
    ap.add_argument("--roi", type=int, default=128)
    ap.add_argument("--patches", type=int, default=8)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 timed runs")
    if args.patches % 2 or not 2 <= args.patches <= 16:
        ap.error("--patches: an even number from 2 to 16 (two volumes, one launch)")
    import torch
    from segmantic_amd import ops
    from segmantic_amd.seg import augment as aug
    from segmantic_amd.seg import trainer
    assert torch.cuda.is_available(), "degrade_bench needs an MI355X"
    dev = torch.device("cuda:0")
    r, P, C = args.roi, args.patches, args.channels
    cache = _cache(args.size, C, 3, dev, args.seed)
    always = {k: {"prob": 1.0} for k in ("noise", "blur", "brightness", "lowres")}

    class Net:
        device = dev
        num_classes, spatial_size, num_samples, flip_prob = 3, [r, r, r], P // 2, 0.2
        augment_spatial, augment_intensity, augment_degrade = False, False, False
    out = trainer.batch_buffers(Net, cache, 2)
    res = {"size": args.size, "roi": r, "patches": P, "channels": C, "repeats": args.repeats}

    def step():
        trainer.make_batch(Net, cache, [0, 1], np.random.RandomState(args.seed), out=out)
    res["make_batch_off"] = _timed(step, args.repeats)
    Net.augment_degrade = always
    res["make_batch_all_on"] = _timed(step, args.repeats)
    res["make_batch_added_ms"] = res["make_batch_all_on"]["ms_median"] - res["make_batch_off"]["ms_median"]

    x = torch.randn((P, r, r, r, C), device=dev)
    elements = x.numel()
    d = aug.draw_degrade(np.random.RandomState(args.seed), P, (r, r, r), aug.degrade_config(always))
    low = (d["lowres"][0], d["lowres"][2])
    res["blur_radii"] = [int(np.floor(4.0 * float(s) + 0.5)) for s in d["blur"][1]]
    res["lowres_extents"] = d["lowres"][2].tolist()
    cases = {"noise": (dict(noise=d["noise"]), 8), "brightness": (dict(brightness=d["brightness"]), 8),
             "noise_brightness": (dict(noise=d["noise"], brightness=d["brightness"]), 8),
             "blur": (dict(blur=d["blur"]), 16), "lowres": (dict(lowres=low), 16),
             "all": (dict(noise=d["noise"], blur=d["blur"], brightness=d["brightness"], lowres=low), 16)}
    for name, (kw, bytes_per) in cases.items():
        t = _timed(lambda: ops.degrade_augment(x, **kw), args.repeats)
        t["model_bytes"] = elements * bytes_per
        t["model_GBps"] = t["model_bytes"] / (t["ms_median"] * 1e-3) / 1e9
        res[f"kernel_{name}"] = t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
