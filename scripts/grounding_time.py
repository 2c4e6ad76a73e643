#!/usr/bin/env python3
"""Dev: what the free-text grounding tail costs at the model's size (B = 2, Q = 900, T = 256) -- ``grounding.ground`` (one
launch of csrc/grounding.hip) plus its one host read (the counts), beside the reference's op chain moved to the device, in the
same process and on the same tensors: per image ``max(dim)``, ``> box_threshold``, two boolean-mask indexings, and per kept row
``> text_threshold`` with ``nonzero`` -- every data-dependent size a host synchronisation, all of them counted.  Three keep
rates: none, ~5 % and all.  Writes profiles/grounding.json (or ``--out``) and prints it as one JSON line.

Beside them, for the design notes: ``ground`` without the host read (back-to-back launches: the larger of the Python around the
entry and the kernel) and the captured launch replayed (the kernel and the graph launch alone).

Both sides: warm-up, then the median of REGIONS device-event-timed regions of ``iters`` calls each (fewer where a call is long).
The numbers are written down as found, with their ratio; ``torch_ops`` / ``host_syncs`` of the chain are counts of the ATen
calls and of the reads that wait for the device (an op is one to a few kernels), not kernel counts."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import grounding  # noqa: E402

REGIONS, WARMUP = 7, 5
B, Q, T = 2, 900, 256
TEXT_THR = 0.25


def inputs(seed=0):
    """Scores below 0.3 except on ~5 % of the queries (0.5 .. 0.9), a second token above the text threshold on those."""
    g = torch.Generator().manual_seed(seed)
    prob = torch.rand(B, Q, T, generator=g) * 0.3
    for b in range(B):
        for q in torch.randperm(Q, generator=g)[:Q // 20].tolist():
            prob[b, q, int(torch.randint(0, T, (1,), generator=g))] = 0.3
            prob[b, q, int(torch.randint(0, T, (1,), generator=g))] = 0.5 + 0.4 * float(torch.rand(1, generator=g))
    return prob.cuda(), torch.rand(B, Q, 4, generator=g).cuda()


def native(prob, boxes, box_thr):
    g = grounding.ground(prob, boxes, box_thr, TEXT_THR)
    return g, g.n_keep.tolist()                                  # the one host read


def replay_of(prob, boxes, box_thr):
    """The launch alone, captured: what a replay costs without the Python around the entry and without the host read."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        grounding.ground(prob, boxes, box_thr, TEXT_THR)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grounding.ground(prob, boxes, box_thr, TEXT_THR)
    return graph.replay


def chain(prob, boxes, box_thr):
    """The reference's predict, its tensors left on the device; -> (per-image results, ATen calls, waits for the device)."""
    out, ops, syncs = [], 0, 0
    for b in range(B):
        p = prob[b]
        mask = p.max(dim=1)[0] > box_thr
        logits, bx = p[mask], boxes[b][mask]                     # each: nonzero (a wait for its size) + a gather
        ops, syncs = ops + 6, syncs + 2
        tokens = [(row > TEXT_THR).nonzero(as_tuple=True)[0] for row in logits]
        ops, syncs = ops + 3 * len(tokens), syncs + len(tokens)   # select, compare, nonzero (a wait) per kept row
        out.append((bx, logits.max(dim=1)[0] if len(tokens) else logits.new_zeros(0), tokens))
        ops += 1
    return out, ops, syncs


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


def same(g, counts, ref):
    """The chain's kept boxes, scores and token sets are the kernel's (order 0 is the boolean mask's order)."""
    for b, (bx, sc, tokens) in enumerate(ref):
        n = counts[b]
        if n != len(tokens) or not torch.equal(g.box[b, :n], bx) or not torch.equal(g.score[b, :n], sc):
            return False
        for row, tok in zip(g.token_bits[b, :n].tolist(), tokens):
            if grounding._set_bits(row) != tok.tolist():
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grounding.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    prob, boxes = inputs()
    out = {"device": torch.cuda.get_device_name(0), "B": B, "Q": Q, "T": T, "text_threshold": TEXT_THR, "regions": REGIONS,
           "cases": {}}
    for name, box_thr in (("keep_none", 1.0), ("keep_5_percent", 0.35), ("keep_all", 0.0)):
        g, counts = native(prob, boxes, box_thr)
        ref, ops, syncs = chain(prob, boxes, box_thr)
        kept = sum(counts)
        t_native = timed(lambda: native(prob, boxes, box_thr), 50)
        t_enqueue = timed(lambda: grounding.ground(prob, boxes, box_thr, TEXT_THR), 50)
        t_replay = timed(replay_of(prob, boxes, box_thr), 50)
        t_chain = timed(lambda: chain(prob, boxes, box_thr), 20 if kept < 200 else 2)
        out["cases"][name] = {"box_threshold": box_thr, "n_keep": counts, "outputs_equal": same(g, counts, ref),
                              "ground_plus_host_read": dict(t_native, launches=1, host_syncs=1),
                              "ground_without_host_read": dict(t_enqueue, launches=1, host_syncs=0),
                              "ground_graph_replay": dict(t_replay, launches=1, host_syncs=0),
                              "op_chain_on_device": dict(t_chain, torch_ops=ops, host_syncs=syncs),
                              "ratio_chain_over_ground": round(t_chain["median_us"] / t_native["median_us"], 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
