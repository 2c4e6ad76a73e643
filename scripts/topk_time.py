#!/usr/bin/env python3
"""Dev: the native row-wise top-k (csrc/topk.hip) beside ``torch.topk`` and the stable ``torch.sort`` path it replaces, and the
native evaluation tail beside ``dt_inference`` + ``detector_postprocess``, in one process on one stream.  Warm-up, then the
median of REGIONS event-timed regions of ITERS calls each; writes ``profiles/topk.json`` (``--out FILE``) with every median,
the spread (min, max) and the kernel launches each evaluation tail issues (the profiler's device activity list)."""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.profiler import ProfilerActivity, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import topk  # noqa: E402
from ziragroundingdino_amd.groundingdino import GroundingDINO  # noqa: E402
from ziragroundingdino_amd.transformer import Switches  # noqa: E402

REGIONS, ITERS, WARMUP = 7, 200, 20


def timed(fn):
    """-> {median_us, min_us, max_us} per call."""
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
    return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2), "max_us": round(max(per_call), 2)}


def launches(fn):
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


class _Tail:
    """What ``GroundingDINO.postprocess`` touches of a model (the tail has no parameters)."""
    postprocess = GroundingDINO.postprocess
    dt_inference = GroundingDINO.dt_inference
    _detection_sizes = GroundingDINO._detection_sizes

    def __init__(self, k):
        self.select_box_nums_for_evaluation, self._pixel_stats = k, {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "iters_per_region": ITERS, "topk": {}, "tail": {}}
    for rows, n, k in ((2, 22223, 900), (2, 900 * 7, 300), (2, 900 * 96, 300)):
        x = torch.randn(rows, n, device="cuda")
        assert topk.supported(x, k)
        r = {"torch_topk": timed(lambda: torch.topk(x, k, dim=1)),
             "torch_sort_stable": timed(lambda: torch.sort(x, dim=1, descending=True, stable=True)[1][:, :k]),
             "topk_rows": timed(lambda: topk.topk_rows(x, k))}
        out["topk"]["%dx%d_k%d" % (rows, n, k)] = r
        print(rows, n, k, json.dumps(r), flush=True)
    for C in (7, 96):
        B, Q, k = 2, 900, 300
        logits, boxes = torch.randn(B, Q, C, device="cuda") * 3, torch.rand(B, Q, 4, device="cuda") * 0.5 + 0.1
        tail = _Tail(k)
        batched, image_sizes = [{"height": 480, "width": 640}] * B, [(800, 1333)] * B

        def run(native):
            Switches.native_detections = native
            with torch.no_grad():
                return tail.postprocess(logits, boxes, batched, image_sizes)

        r = {"parent_chain": timed(lambda: run(False)), "native": timed(lambda: run(True)),
             "launches_parent_chain": launches(lambda: run(False)), "launches_native": launches(lambda: run(True))}
        out["tail"]["B%d_Q%d_C%d_k%d" % (B, Q, C, k)] = r
        print("tail C=%d" % C, json.dumps(r), flush=True)
    out["tail"]["note"] = ("host-inclusive: every call ends in the host read(s) of the kept counts; "
                           "the tail's share of a whole evaluation forward: not measured")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
