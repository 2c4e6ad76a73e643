#!/usr/bin/env python3
"""Dev: what one batch of LVIS box AP matching costs -- ``lvis_evaluation.match`` (one launch of csrc/lvismatch.hip, where the
detections are) beside the host-side alternative on the same batch: the eleven tensors copied to the host (the copy included)
and ``lvis_evaluation.match_reference`` on them.  One batch: B = 2, K = 300 detections, G = 40 GTs per image over LVIS v0.5's
1230 classes, ten thresholds, four area ranges.  The outputs of the two are asserted equal first; the launches of one ``match``
call are counted with the profiler.  Writes profiles/lvis_eval.json (or ``--out``) and prints it as one JSON line.

``match``: warm-up, then the median of REGIONS device-event-timed regions of ITERS launches each.  The host path is timed with a
host clock around copy + compute (it ends on the host, nothing is left in flight), median of HOST_REPS runs after one warm-up run.
Both numbers are written down as found; no ratio and no end-to-end gain is claimed."""
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
from ziragroundingdino_amd import lvis_evaluation as lv  # noqa: E402

REGIONS, ITERS, WARMUP, HOST_REPS = 7, 50, 20, 5
B, K, G, C = 2, 300, 40, 1230


def batch(seed):
    """Detections in score order over a 480 x 640 image; the GTs of an image come from 12 of the 1230 categories, 15 more are
    its negative set, 4 are not exhaustive; a third of the detections sit on a GT, a third carry a category that was never
    checked on the image; a twentieth of the GTs carry the ignore flag."""
    rng = np.random.default_rng(seed)
    gwh = rng.integers(8, 200, (B, G, 2)).astype(np.float64)
    gxy = (rng.uniform(0, 1, (B, G, 2)) * (np.array([640, 480]) - gwh)).astype(np.int64).astype(np.float64)
    dwh = rng.uniform(8, 200, (B, K, 2))
    dxy = rng.uniform(0, 1, (B, K, 2)) * (np.array([640, 480]) - dwh)
    glab = np.zeros((B, G), np.int64)
    dlab = rng.integers(0, C, (B, K))
    neg, nel = [], []
    for b in range(B):
        cats = rng.permutation(C)
        pos, negative = cats[:12], cats[12:27]
        glab[b] = pos[rng.integers(0, 12, G)]
        neg.append(negative.tolist())
        nel.append(pos[:2].tolist() + negative[:2].tolist())
        for k in range(0, K, 3):
            g = int(rng.integers(0, G))
            dxy[b, k], dwh[b, k], dlab[b, k] = gxy[b, g] + rng.normal(0, 3, 2), gwh[b, g] * rng.uniform(0.8, 1.2, 2), glab[b, g]
        for k in range(1, K, 3):
            dlab[b, k] = negative[int(rng.integers(0, 15))]
    arrs = [-np.sort(-rng.uniform(0.05, 1, (B, K)).astype(np.float32), axis=1), dlab.astype(np.int64),
            np.concatenate([dxy, dxy + dwh], -1).astype(np.float32), np.full(B, K, np.int32),
            np.concatenate([gxy, gwh], -1), gwh[..., 0] * gwh[..., 1], glab, (rng.random((B, G)) < 0.05).astype(np.uint8),
            np.full(B, G, np.int32)]
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]
    return t + [lv.category_bitsets(neg, C, "cuda"), lv.category_bitsets(nel, C, "cuda")]


def device_time(t):
    fn = lambda: lv.match(*t, C, with_gt_of=False)
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
        out = lv.match_reference(*on_host, C, with_gt_of=False)
        return out, (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6

    fn()
    runs = [fn() for _ in range(HOST_REPS)]
    total = [r[2] for r in runs]
    return {"median_us": round(statistics.median(total), 1), "min_us": round(min(total), 1), "max_us": round(max(total), 1),
            "copy_median_us": round(statistics.median(r[1] for r in runs), 1)}


def launches(t):
    """Device kernels of ONE ``match`` call, by the profiler (the output tensors are ``torch.empty``: no fill kernels)."""
    lv.match(*t, C, with_gt_of=False)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        lv.match(*t, C, with_gt_of=False)
        torch.cuda.synchronize()
    on_device = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
    return {"count": sum(e.count for e in on_device), "names": sorted(e.key for e in on_device)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lvis_eval.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    t = batch(seed=2019)
    got = lv.match(*t, C)
    want = lv.match_reference(*[x.cpu() for x in t], C)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want)), "match and match_reference differ"
    taking_part = int((got[0] >= 0).sum())
    assert 0 < taking_part < B * K and bool((got[1] != 0).any())
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "iters_per_region": ITERS, "host_reps": HOST_REPS,
           "iou_thrs": len(lv.DEFAULT_IOU_THRS), "area_rngs": len(lv.DEFAULT_AREA_RNGS),
           "cases": {"lvis_B2_K300_G40_C1230": {"B": B, "K": K, "G": G, "C": C, "detections_taking_part": taking_part,
                                                "outputs_equal": True, "match_device": device_time(t),
                                                "host_copy_plus_match_reference": host_time(t), "match_launches": launches(t)}}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
