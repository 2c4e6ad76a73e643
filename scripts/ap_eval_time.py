#!/usr/bin/env python3
"""Dev: what one batch of COCO box AP matching costs -- ``evaluation.match`` (one launch of csrc/apmatch.hip, where the
detections are) beside the host-side alternative, per batch: the nine tensors copied to the host (the copy included) and
``evaluation.match_reference`` on them.  Two batches: B = 2, K = 300 detections, ~20 GTs per image over 7 labels (an ODinW
task) and B = 2, K = 300, 80 labels (COCO-like).  Writes profiles/ap_eval.json (or ``--out``) and prints it as one JSON line.

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
from ziragroundingdino_amd import evaluation as ev  # noqa: E402

REGIONS, ITERS, WARMUP, HOST_REPS = 7, 50, 20, 5


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ap_eval.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "iters_per_region": ITERS, "host_reps": HOST_REPS,
           "iou_thrs": len(ev.DEFAULT_IOU_THRS), "area_rngs": len(ev.DEFAULT_AREA_RNGS), "max_det": 100, "cases": {}}
    for name, (B, K, gts, labels) in {"odinw_like_B2_K300_G20_L7": (2, 300, 20, 7), "coco_like_B2_K300_G20_L80": (2, 300, 20, 80)}.items():
        t = batch(B, K, gts, labels, seed=len(name))
        host, same = host_time(t)
        out["cases"][name] = {"B": B, "K": K, "G": int(t[6].shape[1]), "labels": labels, "match_device": device_time(t),
                              "host_copy_plus_match_reference": host, "outputs_equal": same}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
