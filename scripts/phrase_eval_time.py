#!/usr/bin/env python3
"""Dev: what one batch of phrase-grounding matching costs -- ``phrase_evaluation.match`` (one launch of csrc/phrasematch.hip,
where ``forward_grounding``'s outputs are) beside the same function as torch ops, ``phrase_evaluation.match_reference``, on the
device, and beside the batch copied to the host (the copy included) and ``match_reference`` there.  One batch: B = 2, Q = 900,
T = 256, P = 32 phrases of one to four tokens per image, G = 4 boxes per phrase, k_max = 10, one threshold.  The outputs of the
three are asserted equal first.  Launches are counted with the profiler, synchronising torch calls with torch's sync debug mode
(the warnings of one call).  Writes profiles/phrase_eval.json (or ``--out``) and prints it as one JSON line.

Device paths: warm-up, then the median of REGIONS device-event-timed regions of ITERS calls each.  The host path is timed with a
host clock around copy + compute (it ends on the host, nothing is left in flight), median of HOST_REPS runs after one warm-up
run.  A first measurement: the numbers are written down as found; no end-to-end gain is claimed."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import phrase_evaluation as pe  # noqa: E402

REGIONS, ITERS, REF_ITERS, WARMUP, HOST_REPS = 7, 50, 3, 20, 5
B, Q, T, P, G, K = 2, 900, 256, 32, 4, 10
THRS = (0.5,)


def batch(seed):
    """Token probabilities as a sigmoid of normal logits, a caption of 40 tokens (the rest of the 256 is padding: probability
    0); boxes over a 480 x 640 frame; every phrase one to four neighbouring tokens; its GT boxes sit on four of the queries,
    moved by a few per cent, so that some phrases hit at rank 0, some later and some never."""
    rng = np.random.default_rng(seed)
    prob = np.zeros((B, Q, T), np.float32)
    prob[:, :, :40] = 1 / (1 + np.exp(-rng.normal(-2, 1.5, (B, Q, 40))))
    boxes = np.concatenate([rng.uniform(0.1, 0.9, (B, Q, 2)), rng.uniform(0.05, 0.5, (B, Q, 2))], -1).astype(np.float32)
    sizes = np.array([[480.0, 640.0]] * B, np.float32)
    bits = np.zeros((B, P, T // 32), np.uint32)
    gt = np.zeros((B, P, G, 4), np.float32)
    for b in range(B):
        for p in range(P):
            first, n = int(rng.integers(1, 36)), int(rng.integers(1, 5))
            for t in range(first, first + n):
                bits[b, p, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
            for g in range(G):
                cx, cy, w, h = boxes[b, rng.integers(0, Q)] * rng.uniform(0.9, 1.1, 4)
                gt[b, p, g] = ((cx - w / 2) * 640, (cy - h / 2) * 480, (cx + w / 2) * 640, (cy + h / 2) * 480)
    arrs = (prob, boxes, sizes, bits.view(np.int32), gt, np.full((B, P), G, np.int32))
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


def device_time(fn, iters):
    for _ in range(min(WARMUP, 2 * iters)):
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
    return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2), "max_us": round(max(per_call), 2),
            "calls_per_region": iters}


def host_time(t):
    def fn():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        on_host = [x.cpu() for x in t]
        t1 = time.perf_counter()
        out = pe.match_reference(*on_host, K, THRS)
        return out, (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6

    fn()
    runs = [fn() for _ in range(HOST_REPS)]
    total = [r[2] for r in runs]
    return {"median_us": round(statistics.median(total), 1), "min_us": round(min(total), 1), "max_us": round(max(total), 1),
            "copy_median_us": round(statistics.median(r[1] for r in runs), 1), "launches": 0,
            "host_syncs": "%d device -> host copies, each waits for the device" % len(t)}


def counted(fn):
    """Device kernels (the profiler) and synchronising torch calls (sync debug mode's warnings) of ONE call."""
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    on_device = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return {"launches": sum(e.count for e in on_device), "kernels": len(on_device),
            "host_syncs": sum("synchroniz" in str(w.message) for w in seen)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phrase_eval.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    t = batch(seed=2024)
    assert pe.match_supported(*t, K, THRS)
    got = pe.match(*t, K, THRS)
    on_device = pe.match_reference(*t, K, THRS)
    on_host = pe.match_reference(*[x.cpu() for x in t], K, THRS)
    bits = lambda x: x.cpu().view(torch.int32 if x.dtype == torch.float32 else torch.int64) if x.is_floating_point() else x.cpu()
    for a, b, c in zip(got, on_device, on_host):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c)), "match and match_reference differ"
    first = got.first_hit[..., 0]
    assert bool((first == 0).any()) and bool((first == K).any()) and bool(((first > 0) & (first < K)).any())
    kernel = lambda: pe.match(*t, K, THRS)
    chain = lambda: pe.match_reference(*t, K, THRS)
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "host_reps": HOST_REPS, "first_measurement": True,
           "cases": {"B2_Q900_T256_P32_G4_k10": {
               "B": B, "Q": Q, "T": T, "P": P, "G": G, "k_max": K, "iou_thrs": len(THRS), "outputs_equal": True,
               "phrases_hit_at_rank_0": int((first == 0).sum()), "phrases_without_hit": int((first == K).sum()),
               "match": dict(device_time(kernel, ITERS), **counted(kernel)),
               "match_reference_on_device": dict(device_time(chain, REF_ITERS), **counted(chain)),
               "host_copy_plus_match_reference": host_time(t)}}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
