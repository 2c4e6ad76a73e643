#!/usr/bin/env python3
"""Dev: the metrics log (metrics.py, csrc/metrics.hip) through the Python calls a training run makes, at the model's number of
scalars: 22 loss columns, the gradient norm, the found-inf flag and the loss scale by pointer, ``lr`` and ``data_time`` by value.

Three things on the same 0-dim device tensors in the same process:
  * ``record`` alone;
  * ``record`` with a ``flush`` on every 20th call (window 20);
  * the op chain it replaces: ``{k: v.item()}`` of every scalar in every call plus the reference's numpy bookkeeping
    (``metrics.record_reference`` on the values read, ``metrics.window_reference`` on every 20th call).

Nothing else runs on the device, so these are the costs of the calls on an idle queue -- the ``.item()`` chain's cost inside a
training step is the drain of the queued step, which this script does not see.  Warm-up, then the median of REGIONS
event-timed regions of ITERS calls; wall-clock time of the same regions beside it (the chains differ in host work, not in device
work).  Kernel launches of one call are counted with the profiler, host synchronisations by counting what each path calls.
Writes profiles/metrics.json (or the path given as the only argument) and prints it as one JSON line."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import metrics  # noqa: E402

REGIONS, ITERS, WARMUP = 7, 100, 20
N_LOSS, PERIOD, WINDOW = 22, 20, 20


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    event_us, wall_us = [], []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall_us.append((time.perf_counter() - t0) * 1e6 / ITERS)
        event_us.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return {"event_median_us": round(statistics.median(event_us), 2), "event_min_us": round(min(event_us), 2),
            "event_max_us": round(max(event_us), 2), "wall_median_us": round(statistics.median(wall_us), 2)}


def launches(fn):
    """Kernel launches and device copies of one call, from the profiler's device-side events (None where it gives none)."""
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
    torch.manual_seed(0)
    names = ["loss_%d" % i for i in range(N_LOSS)] + ["grad_norm", "found_inf", "loss_scale", "lr", "data_time"]
    values = torch.rand(len(names) - 2, device="cuda")
    tensors = [values[i] for i in range(values.numel())]
    host = [1e-3, 2e-3]
    log = metrics.DeviceMetrics(names, N_LOSS, window=WINDOW, rows=WINDOW, device="cuda", n_host=2)
    assert log.native
    calls = {"record_flush": 0, "chain": 0}

    def record():
        log.record(tensors, host)

    def record_flush():
        log.record(tensors, host)
        calls["record_flush"] += 1
        if calls["record_flush"] % PERIOD == 0:
            log.flush()

    reference = metrics.new_reference_log(WINDOW)

    def chain():
        read = [t.item() for t in tensors]                  # the reference's {k: v.detach().cpu().item()}
        metrics.record_reference(reference, read, host, N_LOSS)
        calls["chain"] += 1
        if calls["chain"] % PERIOD == 0:
            metrics.window_reference([reference], WINDOW, N_LOSS, len(names) - 1)

    def flush():
        log.flush()

    out = {"device": torch.cuda.get_device_name(0), "columns": len(names), "loss_columns": N_LOSS, "by_pointer": len(tensors),
           "by_value": len(host), "window": WINDOW, "flush_every": PERIOD, "regions": REGIONS, "calls_per_region": ITERS,
           "record": timed(record), "record_and_flush_every_20th": timed(record_flush),
           "item_chain_and_numpy_bookkeeping": timed(chain), "flush_alone": timed(flush),
           "launches_per_call": {"record": launches(record), "flush": launches(flush), "item_chain": launches(chain)},
           "host_syncs_per_step": {"record": 0, "record_and_flush_every_20th": 1.0 / PERIOD, "item_chain": len(tensors)},
           "not_measured": "the calls inside a training step: nothing else is queued here, so a .item() waits for nothing but "
                           "its own copy; no in-step gain is claimed"}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "metrics.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
