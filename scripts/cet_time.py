#!/usr/bin/env python3
"""Forward + backward of the CET text adapter (cet.py) at 768 -> 1024 -> 256 with five gate rows, M = 2 x 41 and 2 x 195 rows:
the native node (csrc/cet.hip) against ``cet_reference`` on the same inputs, through ``cet.cet_apply`` with
``Switches.native_cet`` on and off.  The outputs are first held to the bar of tests/test_cet_gpu.py (error against float64 at most
twice the fp32 reference's plus one ulp); then 7 alternating regions of 10 calls each are event-timed, and the medians with their
min and max and the launch counts per call (kineto) go to profiles/cet.json.  No ratio is fixed in advance.

    python scripts/cet_time.py [--out profiles/cet.json]
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
from ziragroundingdino_amd import cet  # noqa: E402
from ziragroundingdino_amd.transformer import Switches  # noqa: E402

REGIONS, CALLS = 7, 10


def step(mod, x, feat, go, native):
    Switches.native_cet = native
    for p in mod.parameters():
        p.grad = None
    enc, loss = cet.cet_apply(x, feat, mod, "L1", True)
    ((enc * go).sum() + loss.sum()).backward()
    return [enc.detach(), loss.detach()] + [p.grad for p in mod.parameters()]


def held_to_the_bar(mod, x, feat, go):
    twin = cet.CETAdapter(768, 1024, 256).to(x.device).double()
    twin.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
    enc, loss = cet.cet_reference(x.double(), feat.double(), twin, "L1", True)
    ((enc * go.double()).sum() + loss.sum()).backward()
    ref = [enc.detach(), loss.detach()] + [p.grad for p in twin.parameters()]
    native, chain = step(mod, x, feat, go, True), step(mod, x, feat, go, False)
    worst = 0.0
    for n, c, r in zip(native, chain, ref):
        err_n, err_c = float((n.double() - r).abs().max()), float((c.double() - r).abs().max())
        bar = 2.0 * err_c + float(np.spacing(np.float32(float(r.abs().max()))))
        assert err_n <= bar, (err_n, bar)
        worst = max(worst, err_n / bar)
    return worst


def region(mod, x, feat, go, native):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        step(mod, x, feat, go, native)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / CALLS


def launches(mod, x, feat, go, native):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(mod, x, feat, go, native)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)      # kernels, copies and memsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cet.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "geometry": "768 -> 1024 -> 256, 5 gate rows, L1, forward + backward",
              "regions": REGIONS, "calls_per_region": CALLS, "unit": "us per call", "sizes": {}}
    for rows in ((2, 41), (2, 195)):
        gen = torch.Generator().manual_seed(rows[1])
        mod = cet.CETAdapter(768, 1024, 256)
        with torch.no_grad():
            for n, p in mod.named_parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * (1.0 if n == "gate.weight" else 0.05))
        mod = mod.to(dev)
        x, feat, go = (torch.randn(*rows, d, generator=gen).to(dev) for d in (768, 256, 256))
        worst = held_to_the_bar(mod, x, feat, go)
        for native in (True, False):       # warm-up: allocator, workspaces, library kernels
            for _ in range(5):
                step(mod, x, feat, go, native)
        times = {True: [], False: []}
        for _ in range(REGIONS):
            for native in (True, False):
                times[native].append(region(mod, x, feat, go, native))
        entry = {"rows": rows[0] * rows[1], "worst_error_over_bar": worst}
        for native, name in ((True, "native"), (False, "reference")):
            entry[name] = {"median": statistics.median(times[native]), "min": min(times[native]), "max": max(times[native]),
                           "launches": launches(mod, x, feat, go, native)}
        result["sizes"]["%dx%d" % rows] = entry
        print(json.dumps(entry))
    Switches.native_cet = all(e["native"]["median"] <= e["reference"]["median"] for e in result["sizes"].values())
    result["native_not_above_reference_at_both_sizes"] = Switches.native_cet
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
