#!/usr/bin/env python3
"""Forward + backward of the low-rank language side branch (rsb.RepZeroLoRA) at 768 -> 192 -> 256, M = 2 x 41 and 2 x 195 rows,
x without a gradient (a frozen text encoder): the native node (csrc/lora.hip) against ``lora_reference`` on the same inputs,
through the module with ``Switches.native_lora`` on and off, and beside them the dense ``RepZeroLinear`` (768 -> 256) at the same
M.  The outputs are first held to the bar of tests/test_lora_gpu.py (error against float64 at most twice the fp32 reference's plus
one ulp); then 7 alternating regions of 10 calls each are event-timed, and the medians with their min and max and the launch
counts per call (kineto) go to profiles/lora.json.  No ratio is fixed in advance.

    python scripts/lora_time.py [--out profiles/lora.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import rsb  # noqa: E402
from ziragroundingdino_amd.transformer import Switches  # noqa: E402

REGIONS, CALLS = 7, 10
KINDS = ("native", "reference", "rep_zero_linear")


def step(mods, x, go, kind):
    mod = mods["dense" if kind == "rep_zero_linear" else "lora"]
    Switches.native_lora = kind == "native"
    for p in mod.parameters():
        p.grad = None
    out, loss = mod(x)
    ((out * go).sum() + loss).backward()
    return [out.detach(), loss.detach()] + [p.grad for p in mod.parameters()]


def held_to_the_bar(mods, x, go):
    twin = rsb.RepZeroLoRA(768, 256).to(x.device).double()
    twin.load_state_dict({k: v.double() for k, v in mods["lora"].state_dict().items()})
    out, loss = twin.train()(x.double())
    ((out * go.double()).sum() + loss).backward()
    ref = [out.detach(), loss.detach()] + [p.grad for p in twin.parameters()]
    native, chain = step(mods, x, go, "native"), step(mods, x, go, "reference")
    worst = 0.0
    for n, c, r in zip(native, chain, ref):
        err_n, err_c = float((n.double() - r).abs().max()), float((c.double() - r).abs().max())
        bar = 2.0 * err_c + float(np.spacing(np.float32(float(r.abs().max()))))
        assert err_n <= bar, (err_n, bar)
        worst = max(worst, err_n / bar)
    return worst


def region(mods, x, go, kind):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        step(mods, x, go, kind)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / CALLS


def launches(mods, x, go, kind):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(mods, x, go, kind)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)      # kernels, copies and memsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "unit": "us per call", "regions": REGIONS, "calls_per_region": CALLS,
              "geometry": "768 -> 192 -> 256 through RepZeroLoRA (rep_zero_linear: 768 -> 256 through RepZeroLinear), x without a "
                          "gradient, forward + backward", "sizes": {}}
    for rows in ((2, 41), (2, 195)):
        gen = torch.Generator().manual_seed(rows[1])
        mods = {"lora": rsb.RepZeroLoRA(768, 256), "dense": rsb.RepZeroLinear(768, 256)}
        with torch.no_grad():       # O(1) outputs: both arms of SmoothL1
            for mod in mods.values():
                for n, p in mod.named_parameters():
                    if n != "scaling":
                        p.copy_(torch.randn(p.shape, generator=gen) / p.shape[-1] ** 0.5)
        mods = {k: m.to(dev).train() for k, m in mods.items()}
        x, go = (torch.randn(*rows, d, generator=gen).to(dev) for d in (768, 256))
        worst = held_to_the_bar(mods, x, go)
        for kind in KINDS:       # warm-up: allocator, workspaces, library kernels
            for _ in range(5):
                step(mods, x, go, kind)
        times = {kind: [] for kind in KINDS}
        for _ in range(REGIONS):
            for kind in KINDS:
                times[kind].append(region(mods, x, go, kind))
        entry = {"rows": rows[0] * rows[1], "worst_error_over_bar": worst}
        for kind in KINDS:
            entry[kind] = {"median": statistics.median(times[kind]), "min": min(times[kind]), "max": max(times[kind]),
                           "launches": launches(mods, x, go, kind)}
        result["sizes"]["%dx%d" % rows] = entry
        print(json.dumps(entry))
    result["native_not_above_reference_at_both_sizes"] = all(e["native"]["median"] <= e["reference"]["median"]
                                                             for e in result["sizes"].values())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
