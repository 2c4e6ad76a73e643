#!/usr/bin/env python3
"""Dev: what the merged detections tail of a chunked vocabulary costs -- ``vocab.merge_detections`` (one launch of
csrc/vocab.hip for the batch) at B = 2, Q = 900, k = 300 with J = 4 chunks and with J = 31 (an LVIS-sized list of 1203 names at
about 40 names per chunk), every chunk's slice k wide, beside ``vocab.detections_chunked_reference`` on the device for the same
inputs.  The outputs are asserted equal before anything is timed.  Writes profiles/vocab.json (or ``--out``) and prints it as
one JSON line.

Per shape: ``merge_detections`` through its Python call (back-to-back launches: the larger of the Python around the entry and
the kernel), the captured launch replayed (the kernel and the graph launch alone), and the definition's op chain on the device,
with the launches of one call (profiler) and its host synchronisations (counted by reading the code: one ``.tolist()`` of the
sizes, and per image the boolean-mask indexing of ``detector_postprocess`` on scores, classes and boxes, each a synchronising
``nonzero``).

All sides: warm-up, then the median of REGIONS device-event-timed regions of ``iters`` calls each.  The numbers are written
down as found.  Only the merge is timed: no chunked evaluation forward, so no end-to-end figure."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import vocab  # noqa: E402

REGIONS, WARMUP = 7, 5
B, Q, K = 2, 900, 300
SIZES = [[800.0, 1333.0, 800.0, 1333.0], [640.0, 1066.0, 480.0, 799.0]]


def inputs(J, n_names, seed):
    """What J per-chunk ``topk_rows`` calls leave: per chunk k sorted sigmoid-like scores and flat indices into its [Q, C_j],
    its own boxes (a few of them leaving the image or without width)."""
    g = torch.Generator().manual_seed(seed)
    classes = [n_names // J + (1 if j < n_names % J else 0) for j in range(J)]
    start = [K * j for j in range(J + 1)]
    offset = [sum(classes[:j]) for j in range(J)]
    scores = torch.cat([torch.rand(B, K, generator=g).pow(3).sort(dim=1, descending=True).values for _ in range(J)], dim=1)
    index = torch.cat([torch.randint(0, Q * C, (B, K), generator=g) for C in classes], dim=1)
    boxes = torch.rand(J, B, Q, 4, generator=g)
    boxes[..., 2:] = boxes[..., 2:] * 0.4 + 0.02
    boxes[:, :, ::9, 0] += 0.9
    boxes[:, :, 4::13, 2] = 0.0
    return scores.cuda(), index.cuda(), start, classes, offset, boxes.cuda(), K, torch.tensor(SIZES).cuda()


def replay_of(case):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vocab.merge_detections(*case)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vocab.merge_detections(*case)
    return graph.replay


def launches(fn):
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"device": torch.cuda.get_device_name(0), "B": B, "Q": Q, "k": K, "regions": REGIONS, "cases": {},
           "end_to_end": "not measured: only the merge is timed, no chunked evaluation forward"}
    for name, J, n_names in (("J4_160_names", 4, 160), ("J31_lvis_1203_names", 31, 1203)):
        case = inputs(J, n_names, J)
        assert vocab.supported(*case)
        got, want = vocab.merge_detections(*case), vocab.detections_chunked_reference(*case)
        same = all(torch.equal(a, b) for a, b in zip(got, want)) and all(
            torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in ((got[0], want[0]), (got[2], want[2])))
        assert same, "%s: the kernel's output is not the definition's" % name
        kernel = lambda: vocab.merge_detections(*case)
        chain = lambda: vocab.detections_chunked_reference(*case)
        t_kernel, t_replay, t_chain = timed(kernel, 50), timed(replay_of(case), 50), timed(chain, 10)
        out["cases"][name] = {"J": J, "names": n_names, "candidates": case[2][-1], "n_keep": got[3].tolist(), "outputs_equal": same,
                              "lds_bytes": int(vocab._lib.load().zira_det_merge_lds_bytes(case[2][-1])),
                              "merge_detections": dict(t_kernel, launches=launches(kernel), host_syncs=0),
                              "merge_graph_replay": dict(t_replay, launches=1, host_syncs=0),
                              "reference_on_device": dict(t_chain, launches=launches(chain), host_syncs=1 + 3 * B),
                              "ratio_reference_over_merge": round(t_chain["median_us"] / t_kernel["median_us"], 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
