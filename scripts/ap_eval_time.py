#!/usr/bin/env python3
"""Dev: what one batch of COCO box AP matching costs -- ``evaluation.match`` (one launch of csrc/apmatch.hip, where the
detections are) beside the host-side alternative, per batch: the nine tensors copied to the host (the copy included) and
``evaluation.match_reference`` on them.  Two batches: B = 2, K = 300 detections, ~20 GTs per image over 7 labels (an ODinW
task) and B = 2, K = 300, 80 labels (COCO-like).  Writes profiles/ap_eval.json (or ``--out``) and prints it as one JSON line.

``match``: warm-up, then the median of REGIONS device-event-timed regions of ITERS launches each.  The host path is timed with a
host clock around copy + compute (it ends on the host, nothing is left in flight), median of HOST_REPS runs after one warm-up run.
Both numbers are written down as found; no ratio is claimed.

Then ``CocoBoxEvaluator.evaluate()`` on a whole data set's kept state, both ways on the same synthetic state: accumulated
where it is (``evaluation.accumulate_device``: torch orders the state, ONE launch of csrc/apaccum.hip, the two tables copied to
the host) and, with ``FORCE_REFERENCE``, the state copied to the host and ``evaluation.accumulate`` there (the path of the
parent commit).  Two shapes, batches of 2 images as the evaluation loop feeds them: 7 classes, 500 images x 300 detections
(ODinW-like) and 80 classes, 5000 images x 300 detections (COCO-like).  The device way is timed with device events around
``evaluate()`` (median of EVAL_REGIONS regions of EVAL_ITERS calls after a warm-up call; the copy back is inside), the host way
with a host clock (median of EVAL_HOST_REPS runs after one warm-up run); the kernel launches of one device-way call (the
profiler's device activity list), the bytes each way copies to the host and whether the tables are equal are recorded beside
them, and the ratio of the two medians."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch.profiler import ProfilerActivity, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import evaluation as ev  # noqa: E402

REGIONS, ITERS, WARMUP, HOST_REPS = 7, 50, 20, 5
EVAL_REGIONS, EVAL_ITERS, EVAL_HOST_REPS = 7, 3, 3


def batch(B, K, gts_per_image, n_labels, seed):
    """Detections in score order over an 800 x 1333 image, GTs of mixed sizes, a few crowds; a third of the detections sit on a GT."""
    rng = np.random.default_rng(seed)
    G = gts_per_image + 4
    n_gt = rng.integers(gts_per_image - 4, gts_per_image + 5, B).astype(np.int32)
    gwh = rng.uniform(8, 400, (B, G, 2))
    gxy = rng.uniform(0, 1, (B, G, 2)) * (np.array([1333, 800]) - gwh)
    glab = rng.integers(0, n_labels, (B, G))
    dwh = rng.uniform(8, 400, (B, K, 2))
    dxy = rng.uniform(0, 1, (B, K, 2)) * (np.array([1333, 800]) - dwh)
    dlab = rng.integers(0, n_labels, (B, K))
    for b in range(B):
        for k in range(0, K, 3):
            g = int(rng.integers(0, n_gt[b]))
            dxy[b, k], dwh[b, k], dlab[b, k] = gxy[b, g] + rng.normal(0, 4, 2), gwh[b, g] * rng.uniform(0.8, 1.2, 2), glab[b, g]
    scores = -np.sort(-rng.uniform(0.05, 1, (B, K)).astype(np.float32), axis=1)
    arrs = [scores, dlab.astype(np.int64), np.concatenate([dxy, dxy + dwh], -1).astype(np.float32), np.full(B, K, np.int32),
            np.concatenate([gxy, gwh], -1), gwh[..., 0] * gwh[..., 1], glab.astype(np.int64),
            (rng.random((B, G)) < 0.05).astype(np.uint8), n_gt]
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def device_time(t):
    fn = lambda: ev.match(*t, with_gt_of=False)
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


def host_time(t):
    def fn():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        on_host = [x.cpu() for x in t]
        t1 = time.perf_counter()
        out = ev.match_reference(*on_host, with_gt_of=False)
        return out, (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6

    fn()
    runs = [fn() for _ in range(HOST_REPS)]
    same = all(bool(torch.equal(a.cpu(), b)) for a, b in zip(ev.match(*t, with_gt_of=False)[:4], runs[0][0][:4]))
    total = [r[2] for r in runs]
    return {"median_us": round(statistics.median(total), 1), "min_us": round(min(total), 1), "max_us": round(max(total), 1),
            "copy_median_us": round(statistics.median(r[1] for r in runs), 1)}, same


def dataset_state(images, K, n_labels, gts_per_image, seed, per_batch=2):
    """What ``CocoBoxEvaluator`` holds after ``images`` images: rows in score order, ranks counted per row, a hit at a threshold
    is a hit at every lower one and hits are fewer than GTs, a tenth of the ignore bits set, the last tenth of every row padding; drawn on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *shape: torch.rand(shape, generator=g, device="cuda")
    T, A = len(ev.DEFAULT_IOU_THRS), len(ev.DEFAULT_AREA_RNGS)
    scores = torch.sort(rand(images, K) * 0.95 + 0.05, dim=1, descending=True)[0]
    labels = torch.randint(0, n_labels, (images, K), generator=g, device="cuda")
    rank = torch.empty((images, K), dtype=torch.int32, device="cuda")
    for lo in range(0, images, 250):
        l = labels[lo:lo + 250]
        rank[lo:lo + 250] = (l[:, :, None] == l[:, None, :]).tril(-1).sum(2).to(torch.int32)
    rank[:, K - K // 10:] = -1
    # hits at thresholds 0 .. best - 1, for about one detection in twenty (the better-scored ones more often): recall stays under 1
    best = (torch.floor(rand(images, K) * (T + 1)).clamp(max=T) * (rand(images, K) < 0.1 * scores)).to(torch.int64)
    matched = torch.zeros((images, K), dtype=torch.int64, device="cuda")
    ignored = torch.zeros((images, K), dtype=torch.int64, device="cuda")
    for a in range(A):
        matched |= ((1 << best) - 1) << (a * T)
        ignored |= torch.where(rand(images, K) < 0.1, (1 << T) - 1, 0) << (a * T)
    G = gts_per_image + 4
    gt_label = torch.randint(0, n_labels, (images, G), generator=g, device="cuda")
    gt_label[:, gts_per_image:] = -1
    gt_ignored = torch.randint(0, 1 << A, (images, G), generator=g, device="cuda").to(torch.uint8) & 0x0E     # never for "all"
    state = dict(scores=scores.float(), labels=labels, rank=rank, matched=matched, ignored=ignored, gt_label=gt_label,
                 gt_ignored=gt_ignored)
    return [{k: v[lo:lo + per_batch] for k, v in state.items()} for lo in range(0, images, per_batch)]


def evaluate_times(images, K, n_labels, gts_per_image, seed):
    names = ["c%d" % i for i in range(n_labels)]

    def evaluator():
        e = ev.CocoBoxEvaluator(names)
        e._batches = dataset_state(images, K, n_labels, gts_per_image, seed)
        return e

    e = evaluator()
    assert ev.accumulate_supported(e._batches, n_labels, e.iou_thrs, e.area_rngs, e.max_dets)
    result = e.evaluate()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(EVAL_REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(EVAL_ITERS):
            e.evaluate()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / EVAL_ITERS)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ev.accumulate_device(e._batches, n_labels, e.iou_thrs, e.area_rngs, e.max_dets)
        torch.cuda.synchronize()
    kernels = [x.name for x in prof.events() if x.device_type == torch.autograd.DeviceType.CUDA]
    device = {"median_ms": round(statistics.median(per_call), 3), "min_ms": round(min(per_call), 3), "max_ms": round(max(per_call), 3),
              "accumulate_device_launches": len(kernels), "of_them_ap_accumulate_kernel": sum("ap_accumulate" in k for k in kernels),
              "bytes_to_host": (e.precision.size + e.recall.size) * 8}

    ev.FORCE_REFERENCE = True
    try:
        h = evaluator()

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h._gather()
            t1 = time.perf_counter()
            out = h.evaluate()
            return out, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        run()
        runs = [run() for _ in range(EVAL_HOST_REPS)]
    finally:
        ev.FORCE_REFERENCE = False
    total = [r[2] for r in runs]
    host = {"median_ms": round(statistics.median(total), 1), "min_ms": round(min(total), 1), "max_ms": round(max(total), 1),
            "gather_alone_median_ms": round(statistics.median(r[1] for r in runs), 1),
            "bytes_to_host": sum(t.numel() * t.element_size() for b in h._batches for t in b.values())}
    same = bool(np.array_equal(e.precision, h.precision) and np.array_equal(e.recall, h.recall) and runs[0][0] == result)
    assert same, "the device tables differ from the host's"
    return {"classes": n_labels, "images": images, "K": K, "batches": len(e._batches), "detection_slots": images * K,
            "evaluate_device_accumulate": device, "evaluate_force_reference": host, "outputs_equal": same,
            "host_over_device": round(host["median_ms"] / device["median_ms"], 1), "AP": result["bbox"]["AP"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ap_eval.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "iters_per_region": ITERS, "host_reps": HOST_REPS,
           "iou_thrs": len(ev.DEFAULT_IOU_THRS), "area_rngs": len(ev.DEFAULT_AREA_RNGS), "max_det": 100, "cases": {},
           "eval_regions": EVAL_REGIONS, "eval_iters_per_region": EVAL_ITERS, "eval_host_reps": EVAL_HOST_REPS, "evaluate": {}}
    for name, (B, K, gts, labels) in {"odinw_like_B2_K300_G20_L7": (2, 300, 20, 7), "coco_like_B2_K300_G20_L80": (2, 300, 20, 80)}.items():
        t = batch(B, K, gts, labels, seed=len(name))
        host, same = host_time(t)
        out["cases"][name] = {"B": B, "K": K, "G": int(t[6].shape[1]), "labels": labels, "match_device": device_time(t),
                              "host_copy_plus_match_reference": host, "outputs_equal": same}
    for name, shape in {"odinw_like_C7_500x300": (500, 300, 7, 20), "coco_like_C80_5000x300": (5000, 300, 80, 20)}.items():
        out["evaluate"][name] = evaluate_times(*shape, seed=len(name))
        print(name, json.dumps(out["evaluate"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
