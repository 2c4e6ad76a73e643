#!/usr/bin/env python3
"""Dev: what the batched box NMS costs behind the two tails -- ``nms.nms_padded`` (one launch of csrc/nms.hip for the batch) on
the detections tail's shape (B = 2, K = 300, 80 labels) and the grounding tail's (B = 2, K = 900, class-agnostic), beside the
only alternative this stack has: the same batch copied to the host and run through ``nms.nms_reference`` there.  The outputs
are asserted equal before anything is timed.  Writes profiles/nms.json (or ``--out``) and prints it as one JSON line.

Per shape: ``nms_padded`` plus the one host read a tail makes behind it (the counts), ``nms_padded`` alone (back-to-back launches:
the larger of the Python around the entry and the kernel), and the captured launch replayed (the kernel and the graph launch
alone).  Beside them the kernel's two extremes at its limit, K = 1024 in one image, replayed: every candidate kept (boxes that do
not touch: the sweep ORs 1024 rows) and every candidate but one suppressed (one box 1024 times: it ORs one).

All sides: warm-up, then the median of REGIONS device-event-timed regions of ``iters`` calls each.  The numbers are written down
as found."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import nms  # noqa: E402

REGIONS, WARMUP = 7, 5
THR = 0.5


def inputs(B, K, n_labels, seed):
    """A box per eight candidates and copies of it moved by a few percent of its side -- what a DETR-style head hands over --
    in an image of 1333 x 800; the second image has three quarters of its rows live."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand(B, K, 2, generator=g) * torch.tensor([1333.0, 800.0])
    size = 40 + torch.rand(B, K, 2, generator=g) * 260
    src = torch.randint(0, K, (K,), generator=g) // 8 * 8 % K
    centre, size = centre[:, src], size[:, src]
    boxes = torch.cat([centre - size / 2, centre + size / 2], dim=2) + (torch.rand(B, K, 4, generator=g) - 0.5) * 0.1 * size.repeat(1, 1, 2)
    scores = torch.rand(B, K, generator=g)
    labels = None if n_labels is None else torch.randint(0, n_labels, (B, K), generator=g)
    n = torch.tensor([K] + [K * 3 // 4] * (B - 1), dtype=torch.int32)
    return boxes, scores, labels, n


def extremes(K):
    """(every candidate kept, all but one suppressed) for one image of K candidates."""
    i = torch.arange(K, dtype=torch.float32)
    apart = torch.stack([3 * i, 0 * i, 3 * i + 2, 0 * i + 2], dim=1)[None]
    same = torch.tensor([3.0, 2.0, 11.0, 7.0]).repeat(1, K, 1)
    scores = torch.rand(1, K, generator=torch.Generator().manual_seed(K))
    n = torch.tensor([K], dtype=torch.int32)
    return (apart, scores, None, n), (same, scores, None, n)


def cuda(case):
    return tuple(None if t is None else t.cuda() for t in case)


def replay_of(case):
    """The launch alone, captured: what a replay costs without the Python around the entry and without the host read."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nms.nms_padded(*case, THR)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nms.nms_padded(*case, THR)
    return graph.replay


def on_host(case):
    """The alternative: the batch to the host, the definition there."""
    return nms.nms_reference(*(None if t is None else t.cpu() for t in case), THR)


def timed(fn, iters):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / iters)
    return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2),
            "max_us": round(max(per_call), 2), "iters_per_region": iters}


def equal(case):
    keep, n_keep = nms.nms_padded(*case, THR)
    want_keep, want_n = on_host(case)
    return torch.equal(keep.cpu(), want_keep) and torch.equal(n_keep.cpu(), want_n), n_keep.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"device": torch.cuda.get_device_name(0), "iou_threshold": THR, "regions": REGIONS, "cases": {}, "limit_K_1024": {}}
    for name, (B, K, n_labels) in (("detections_B2_K300_80_labels", (2, 300, 80)), ("grounding_B2_K900_agnostic", (2, 900, None))):
        case = cuda(inputs(B, K, n_labels, K))
        same, counts = equal(case)
        assert same, "%s: the kernel's output is not the definition's" % name
        t_read = timed(lambda: nms.nms_padded(*case, THR)[1].tolist(), 50)
        t_enqueue = timed(lambda: nms.nms_padded(*case, THR), 50)
        t_replay = timed(replay_of(case), 50)
        t_host = timed(lambda: on_host(case), 5)
        out["cases"][name] = {"B": B, "K": K, "labels": n_labels, "n": case[3].tolist(), "n_keep": counts, "outputs_equal": same,
                              "nms_plus_host_read": dict(t_read, launches=1, host_syncs=1),
                              "nms_without_host_read": dict(t_enqueue, launches=1, host_syncs=0),
                              "nms_graph_replay": dict(t_replay, launches=1, host_syncs=0),
                              "copy_to_host_and_reference": t_host,
                              "ratio_host_over_nms": round(t_host["median_us"] / t_read["median_us"], 2)}
    for name, case in zip(("all_kept", "all_but_one_suppressed"), extremes(1024)):
        case = cuda(case)
        same, counts = equal(case)
        assert same, "%s: the kernel's output is not the definition's" % name
        out["limit_K_1024"][name] = {"B": 1, "K": 1024, "n_keep": counts, "outputs_equal": same,
                                     "nms_graph_replay": dict(timed(replay_of(case), 50), launches=1, host_syncs=0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
