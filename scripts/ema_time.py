#!/usr/bin/env python3
"""Dev: the model EMA at the model's size -- every parameter and buffer of GroundingDINO-T (Swin-T, random weights) -- through
the Python calls a training run makes: ``EMAUpdater.update`` as the one native launch (csrc/ema.hip) and as the reference's op
chain (``ema.update_reference``: two ``_foreach`` passes) on the same device in the same process, and likewise
``apply_and_restore`` as two swap launches and as the reference's clone, apply and restore.

Warm-up, then the median of REGIONS event-timed regions of ITERS calls each; the kernel launches of one call of each kind are
counted with the profiler afterwards.  Writes profiles/ema.json (or the path given as the only argument) and prints it as one
JSON line."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import ema  # noqa: E402
from ziragroundingdino_amd.transformer import Switches  # noqa: E402

REGIONS, ITERS, WARMUP = 7, 10, 3
DECAY = 0.999


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return {"median_us": round(statistics.median(per_call), 1), "min_us": round(min(per_call), 1), "max_us": round(max(per_call), 1)}


def launches(fn):
    """Kernel launches of one call, from the profiler's device-side events (None where the profiler gives none)."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception as exc:   # noqa: BLE001  (a figure beside the timings, not worth losing them)
        print("profiler: %r" % (exc,), file=sys.stderr)
        return None


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    from ziragroundingdino_amd.config import zira_swint_config
    from ziragroundingdino_amd.groundingdino import build_model

    torch.manual_seed(0)
    model = build_model(zira_swint_config(device="cuda")).to("cuda").train()
    tensors = list(model.named_parameters()) + list(model.named_buffers())
    fp32 = [t for _, t in tensors if t.dtype == torch.float32]

    Switches.native_ema = True
    native = ema.EMAState()
    native_updater = ema.EMAUpdater(native, decay=DECAY)
    native_updater.init_state(model)
    Switches.native_ema = False
    reference = ema.EMAState.FromModel(model)
    Switches.native_ema = True
    served, rest = native._split(model)

    def reference_apply_and_restore():      # EMAState.apply_and_restore of the reference: clone, apply, restore
        old = ema.EMAState.FromModel(model, reference.device)
        reference.apply_to(model)
        old.apply_to(model)

    def native_apply_and_restore():
        with native.apply_and_restore(model):
            pass

    def chain():
        ema.update_reference(reference, model, DECAY)

    def kernel():
        native_updater.update(model)

    def off(fn):
        def run():
            Switches.native_ema = False
            try:
                fn()
            finally:
                Switches.native_ema = True
        return run

    n = sum(t.numel() for t in fp32)
    out = {"device": torch.cuda.get_device_name(0), "tensors": len(tensors), "fp32_tensors": len(fp32), "fp32_values": n,
           "served_by_the_kernel": len(served), "other_tensors": len(rest), "flat_values": native._flat.numel(),
           "regions": REGIONS, "calls_per_region": ITERS, "decay": DECAY,
           "update_kernel": timed(kernel), "update_reference": timed(chain),
           "swap_apply_and_restore": timed(native_apply_and_restore),
           "clone_apply_and_restore": timed(off(reference_apply_and_restore)),
           # what the launches must move: update reads average and model and writes the average; the chain reads and writes
           # the average, then reads both and writes it again; one swap reads and writes both
           "bytes": {"update_kernel": 12 * n, "update_reference": 20 * n, "swap_apply_and_restore": 32 * n,
                     "clone_apply_and_restore": 24 * n}}
    for key in ("update_kernel", "update_reference", "swap_apply_and_restore", "clone_apply_and_restore"):
        out[key]["GB_per_s"] = round(out["bytes"][key] / out[key]["median_us"] * 1e-3, 1)
    out["launches_per_call"] = {"update_kernel": launches(kernel), "update_reference": launches(chain),
                                "swap_apply_and_restore": launches(native_apply_and_restore),
                                "clone_apply_and_restore": launches(off(reference_apply_and_restore))}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ema.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
