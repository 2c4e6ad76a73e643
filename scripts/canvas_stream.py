#!/usr/bin/env python3
"""Canvas batching against a stream of ODinW-sized minibatches: the full-size GroundingDINO-T training step over minibatches of
two images drawn independently from ``ResizeShortestEdge(480 ... 800 step 32, max 1333)`` plus the mapper's crop branch.

    python scripts/canvas_stream.py [--out FILE] [--batches N] [--timeout S]     the A/B (needs a GPU)
    python scripts/canvas_stream.py --pick                                        how DEFAULT_CANVASES was chosen (no GPU)
    python scripts/canvas_stream.py --placement kernel|chain [--iters N]          the placement alone (for rocprofv3 --stats)
    python scripts/canvas_stream.py --placement-report STATS_KERNEL.csv STATS_CHAIN.csv [--out FILE]

The A/B starts two FRESH child processes on the same stream, one after the other, each under its own time limit, the second
only if the first exited 0: (a) ``canvas_sizes = None`` (every batch padded to its own maximum: today's behaviour) and (b)
``canvas_sizes = canvas.DEFAULT_CANVASES``.  A child warms up with one pass over the stream (graphs are captured there), times
three more passes and reports the median pass: ms per step, real (unpadded) pixels per second, the share of steps whose
transformer / front end replayed from graphs, the mean canvas / batch-max pixel ratio and the peak allocated memory.  The parent
writes both and their ratio as one JSON document (default: profiles/canvas_stream.json; the ``placement`` block of an existing
file is kept).

``--placement`` runs only the batch assembly of a full-size pair (800 x 1333 beside 640 x 1066 into the 800 x 1344 canvas) N
times, for a ``rocprofv3 --kernel-trace --stats`` run of its own; ``--placement-report`` reads the two kernel-stats tables of
such runs and sets the kernel against its byte bound at 8 TB/s and at the box's measured copy speed (bench.copy_ceiling)."""
import csv
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHORT_EDGES = tuple(range(480, 801, 32))
MAX_SIZE = 1333
# (width / height of the original, share): landscape, portrait and square photographs
ASPECTS = ((4 / 3, 0.35), (3 / 2, 0.20), (16 / 9, 0.10), (1.0, 0.10), (3 / 4, 0.15), (2 / 3, 0.10))
PLACEMENT_SIZES, PLACEMENT_CANVAS = ((800, 1333), (640, 1066)), (800, 1344)


def _resize_shortest_edge(h, w, short, max_size=None):
    scale = short / min(h, w)
    nh, nw = h * scale, w * scale
    if max_size is not None and max(nh, nw) > max_size:
        scale = max_size / max(nh, nw)
        nh, nw = nh * scale, nw * scale
    return int(nh + 0.5), int(nw + 0.5)


def sample_size(rng):
    """(h, w) of one training image: the reference mapper's two branches with equal odds -- ResizeShortestEdge alone, or
    ResizeShortestEdge(400 / 500 / 600) -> RandomCrop(absolute_range 384 ... 600) -> ResizeShortestEdge."""
    aspect = ASPECTS[rng.choice(len(ASPECTS), p=[p for _, p in ASPECTS])][0]
    h, w = (480, int(480 * aspect + 0.5)) if aspect >= 1 else (int(480 / aspect + 0.5), 480)
    if rng.random() < 0.5:
        h, w = _resize_shortest_edge(h, w, int(rng.choice((400, 500, 600))))
        h = min(h, int(rng.integers(384, min(600, h) + 1))) if h >= 384 else h
        w = min(w, int(rng.integers(384, min(600, w) + 1))) if w >= 384 else w
    return _resize_shortest_edge(h, w, int(rng.choice(SHORT_EDGES)), MAX_SIZE)


def stream_sizes(n_batches, seed=0):
    rng = np.random.default_rng(seed)
    return [(sample_size(rng), sample_size(rng)) for _ in range(n_batches)]


def pick(n_canvases=12, n_batches=20000):
    """Greedy: start from (1344, 1344), add the canvas that lowers the mean canvas / batch-max pixel ratio most."""
    sizes = np.array([np.max(np.array(pair), 0) for pair in stream_sizes(n_batches)])
    area = sizes[:, 0] * sizes[:, 1]
    sides = range(480, 1345, 32)
    cands = [(H, W) for H in sides for W in sides]
    fits = {c: (sizes[:, 0] <= c[0]) & (sizes[:, 1] <= c[1]) for c in cands}
    chosen, cur = [(1344, 1344)], np.full(len(sizes), 1344 * 1344.0)
    while len(chosen) < n_canvases:
        best = None
        for c in cands:
            if c not in chosen:
                new = np.where(fits[c] & (c[0] * c[1] < cur), c[0] * c[1], cur)
                ratio = float((new / area).mean())
                if best is None or ratio < best[0]:
                    best = (ratio, c, new)
        chosen.append(best[1])
        cur = best[2]
        print("%2d canvases: + %s -> mean canvas / batch-max pixels %.4f" % (len(chosen), best[1], best[0]))
    print(sorted(chosen))


# ---- the A/B --------------------------------------------------------------------------------------------------------------------

def child(variant, n_batches):
    import torch

    from ziragroundingdino_amd import canvas
    from ziragroundingdino_amd.config import zira_swint_config
    from ziragroundingdino_amd.groundingdino import build_model
    from ziragroundingdino_amd.train import ZiraTrainer, synthetic_batch

    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = build_model(zira_swint_config(device="cuda")).to(dev).train()
    model.canvas_sizes = canvas.DEFAULT_CANVASES if variant == "b" else None
    trainer = ZiraTrainer(model)
    sizes = stream_sizes(n_batches)
    batches = [[synthetic_batch(1, h, w, n_categories=15, seed=2 * i + j, device=dev)[0] for j, (h, w) in enumerate(pair)]
               for i, pair in enumerate(sizes)]
    real_pixels = sum(h * w for pair in sizes for h, w in pair)
    maxima = [(max(p[0][0], p[1][0]), max(p[0][1], p[1][1])) for p in sizes]
    if variant == "b":
        padded = [canvas.choose(h, w) for h, w in maxima]
        ratio = statistics.mean(c[0] * c[1] / (h * w) for c, (h, w) in zip(padded, maxima))
    else:
        padded, ratio = maxima, 1.0

    eager = {"transformer": 0}
    real_forward = model.transformer.forward
    model.transformer.forward = lambda *a, **k: (eager.__setitem__("transformer", eager["transformer"] + 1), real_forward(*a, **k))[1]

    def one_pass():
        replayed_t = replayed_f = 0
        t0 = time.perf_counter()
        for i, data in enumerate(batches):
            before = eager["transformer"]
            trainer.run_step(data, next_data=batches[(i + 1) % len(batches)])
            replayed_t += eager["transformer"] == before
            sig = ((2, 3) + tuple(padded[i]), torch.float32, dev.index or 0)
            replayed_f += any(key[0][0] == sig for key in model._graphed_backbone._cache)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(batches) * 1e3, replayed_t / len(batches), replayed_f / len(batches)

    one_pass()                                    # warm-up: captures
    torch.cuda.reset_peak_memory_stats()
    passes = sorted(one_pass() for _ in range(3))
    ms, share_t, share_f = passes[1]
    print(json.dumps({
        "variant": variant, "canvas_sizes": None if variant == "a" else [list(c) for c in canvas.DEFAULT_CANVASES],
        "batches": n_batches, "distinct_shapes": len(set(padded)), "ms_per_step": round(ms, 3),
        "ms_per_step_passes": [round(p[0], 3) for p in passes],
        "real_pixels_per_s": round(real_pixels / n_batches / (ms * 1e-3)),
        "transformer_replayed_share": share_t, "frontend_replayed_share": share_f,
        "canvas_over_batch_max_pixels": round(ratio, 4),
        "peak_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2),
        "transformer_graph_sets": len(model._graphed_transformer._cache),
        "frontend_graphs": len(model._graphed_backbone._cache)}), flush=True)


def parent(out_path, n_batches, timeout):
    results = {}
    for variant in ("a", "b"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--batches", str(n_batches)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("variant %s failed (exit %d); nothing further is started" % (variant, p.returncode))
        results[variant] = json.loads(lines[-1])
    doc = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc.update({
        "workload": "GroundingDINO-T + ZiRa training step, fp32 interfaces, 2 images per step, %d minibatches drawn from "
                    "scripts/canvas_stream.py sample_size (seed 0), one warm-up pass, median of three timed passes" % n_batches,
        "a_batch_maximum": results["a"], "b_default_canvases": results["b"],
        "b_over_a_ms_per_step": round(results["b"]["ms_per_step"] / results["a"]["ms_per_step"], 4),
        "fixed_shape_ms_per_step": 24.1,
        "b_over_fixed_shape": round(results["b"]["ms_per_step"] / 24.1, 4)})
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


# ---- the placement alone --------------------------------------------------------------------------------------------------------

def placement(kind, iters):
    import torch

    from ziragroundingdino_amd import canvas
    from ziragroundingdino_amd.structures import ImageList
    from ziragroundingdino_amd.utils import nested_tensor_from_tensor_list

    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8).float().to(dev) for h, w in PLACEMENT_SIZES]
    mean, std = [123.675, 116.280, 103.530], [58.395, 57.12, 57.375]
    m, s = (torch.tensor(v, device=dev).view(3, 1, 1) for v in (mean, std))
    for _ in range(iters):
        if kind == "kernel":
            canvas.place(images, PLACEMENT_CANVAS, mean, std)
        else:    # preprocess_image -> ImageList.from_tensors -> nested_tensor_from_tensor_list, as GroundingDINO.forward runs them
            nested_tensor_from_tensor_list(ImageList.from_tensors([(x.to(dev) - m) / s for x in images]))
    torch.cuda.synchronize()
    print("placement %s: %d iterations" % (kind, iters))


def _stats_rows(path):
    with open(path) as f:
        return [r for r in csv.DictReader(f)]


def placement_report(kernel_csv, chain_csv, out_path, iters):
    import torch

    from bench import copy_ceiling

    def total_us(rows, keep):
        return sum(float(r["TotalDurationNs"]) for r in rows if keep(r["Name"])) / 1e3 / iters

    def launches(rows, keep):
        return sum(int(r["Calls"]) for r in rows if keep(r["Name"])) / iters

    krows, crows = _stats_rows(kernel_csv), _stats_rows(chain_csv)
    is_place = lambda n: "place_kernel" in n
    bytes_read = sum(3 * h * w * 4 for h, w in PLACEMENT_SIZES)
    bytes_written = len(PLACEMENT_SIZES) * PLACEMENT_CANVAS[0] * PLACEMENT_CANVAS[1] * 13
    nbytes = bytes_read + bytes_written
    ceiling = copy_ceiling(torch.device("cuda"))
    k_us = total_us(krows, is_place)
    block = {
        "shape": "fp32 sources %s into canvas %s" % (list(PLACEMENT_SIZES), list(PLACEMENT_CANVAS)),
        "bytes": nbytes, "kernel_us": round(k_us, 2), "kernel_launches": launches(krows, is_place),
        "bound_us_at_8TBs": round(nbytes / 8e12 * 1e6, 2),
        "copy_ceiling_GBs": round(ceiling["copy_GBs"], 1),
        "bound_us_at_copy_ceiling": round(nbytes / (ceiling["copy_GBs"] * 1e9) * 1e6, 2),
        "kernel_GBs": round(nbytes / (k_us * 1e-6) / 1e9, 1),
        "frac_of_8TBs": round(nbytes / 8e12 * 1e6 / k_us, 3),
        "frac_of_copy_ceiling": round(nbytes / (ceiling["copy_GBs"] * 1e9) * 1e6 / k_us, 3),
        "op_chain_us": round(total_us(crows, lambda n: True), 2), "op_chain_launches": launches(crows, lambda n: True),
        "source": "rocprofv3 --kernel-trace --stats, one run per kind, %d iterations each, kernel time only" % iters}
    doc = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc["placement"] = block
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(block))


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


if __name__ == "__main__":
    out = _arg("--out", os.path.join(ROOT, "profiles", "canvas_stream.json"))
    n = int(_arg("--batches", "16"))
    if "--pick" in sys.argv:
        pick()
    elif "--child" in sys.argv:
        child(_arg("--child"), n)
    elif "--placement" in sys.argv:
        placement(_arg("--placement"), int(_arg("--iters", "50")))
    elif "--placement-report" in sys.argv:
        i = sys.argv.index("--placement-report")
        placement_report(sys.argv[i + 1], sys.argv[i + 2], out, int(_arg("--iters", "50")))
    else:
        assert n >= 16, "the stream is at least 16 minibatches"
        parent(out, n, int(_arg("--timeout", "420")))
