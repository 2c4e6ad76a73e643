#!/usr/bin/env python3
"""Dev: what one batch of Pascal VOC box AP matching costs -- ``voc_evaluation.match`` (one launch of csrc/vocmatch.hip, where
the detections are) beside the host-side alternative on the same batch: the eight tensors copied to the host (the copy
included) and ``voc_evaluation.match_reference`` on them.  One batch: B = 2, K = 300 detections, G = 20 GTs per image over VOC's
20 labels, ten thresholds.  Writes profiles/voc_eval.json (or ``--out``) and prints it as one JSON line.

``match``: warm-up, then the median of REGIONS device-event-timed regions of ITERS launches each.  The host path is timed with a
host clock around copy + compute (it ends on the host, nothing is left in flight), median of HOST_REPS runs after one warm-up run.
Both numbers are written down as found; no ratio is claimed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import voc_evaluation as voc  # noqa: E402

REGIONS, ITERS, WARMUP, HOST_REPS = 7, 50, 20, 5
B, K, G, LABELS = 2, 300, 20, 20


def batch(seed):
    """Detections in the model's order (unsorted) over a 375 x 500 image, integer GT corners, a tenth of the GTs difficult; a
    third of the detections sit on a GT."""
    rng = np.random.default_rng(seed)
    gwh = rng.integers(8, 200, (B, G, 2))
    gxy = 1 + (rng.uniform(0, 1, (B, G, 2)) * (np.array([500, 375]) - gwh)).astype(np.int64)
    glab = rng.integers(0, LABELS, (B, G))
    dwh = rng.uniform(8, 200, (B, K, 2))
    dxy = rng.uniform(0, 1, (B, K, 2)) * (np.array([500, 375]) - dwh)
    dlab = rng.integers(0, LABELS, (B, K))
    for b in range(B):
        for k in range(0, K, 3):
            g = int(rng.integers(0, G))
            dxy[b, k], dwh[b, k], dlab[b, k] = gxy[b, g] - 1 + rng.normal(0, 3, 2), gwh[b, g] * rng.uniform(0.8, 1.2, 2), glab[b, g]
    arrs = [rng.uniform(0.05, 1, (B, K)).astype(np.float32), dlab.astype(np.int64),
            np.concatenate([dxy, dxy + dwh], -1).astype(np.float32), np.full(B, K, np.int32),
            np.concatenate([gxy, gxy + gwh], -1).astype(np.float64), glab.astype(np.int64),
            (rng.random((B, G)) < 0.1).astype(np.uint8), np.full(B, G, np.int32)]
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def device_time(t):
    fn = lambda: voc.match(*t, LABELS, with_gt_of=False)
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
        out = voc.match_reference(*on_host, LABELS, with_gt_of=False)
        return out, (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6

    fn()
    runs = [fn() for _ in range(HOST_REPS)]
    same = all(bool(torch.equal(a.cpu(), b)) for a, b in zip(voc.match(*t, LABELS, with_gt_of=False)[:3], runs[0][0][:3]))
    total = [r[2] for r in runs]
    return {"median_us": round(statistics.median(total), 1), "min_us": round(min(total), 1), "max_us": round(max(total), 1),
            "copy_median_us": round(statistics.median(r[1] for r in runs), 1)}, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voc_eval.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    t = batch(seed=2007)
    host, same = host_time(t)
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "iters_per_region": ITERS, "host_reps": HOST_REPS,
           "iou_thrs": len(voc.DEFAULT_IOU_THRS),
           "cases": {"voc_B2_K300_G20_L20": {"B": B, "K": K, "G": G, "labels": LABELS, "match_device": device_time(t),
                                             "host_copy_plus_match_reference": host, "outputs_equal": same}}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
