#!/usr/bin/env python3
"""Dev: what the device augmentation costs per minibatch of two 1024 x 1024 decoded images at ODinW sizes, both branches:
``augment.apply_image`` (csrc/resample.hip: per stage one coefficient launch and one resample launch) beside the same chain on
the host -- through Pillow where it is importable, otherwise through ``augment.resample_reference`` on CPU tensors.  Writes
profiles/augment.json (or ``--out``) and prints it as one JSON line.

Device: warm-up, then the median of REGIONS device-event-timed regions of ITERS minibatches each.  Host: a host clock around the
chain of both images, median of HOST_REPS runs after one warm-up run.  ``bytes``: what the streaming bound counts (every source
byte read once, every output byte written once, per stage) and the rate that bound would mean at the measured time.  Both
numbers are written down as found; no ratio is claimed."""
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
from ziragroundingdino_amd import augment  # noqa: E402
from ziragroundingdino_amd.augment import AugmentParams  # noqa: E402

REGIONS, ITERS, WARMUP, HOST_REPS = 7, 20, 10, 5
SIDE = 1024

# a minibatch of two per branch, sizes the ODinW configuration draws for a 1024 x 1024 original
CASES = {
    "plain_800_and_640": [AugmentParams(True, None, None, (800, 800)), AugmentParams(False, None, None, (640, 640))],
    "crop_600_then_800_and_500_then_704": [
        AugmentParams(True, (600, 600), (37, 101, 480, 384), augment.output_shape(480, 384, 800, 1333)),
        AugmentParams(False, (500, 500), (0, 16, 500, 450), augment.output_shape(500, 450, 704, 1333))],
}


def streaming_bytes(params):
    total = 0
    for p in params:
        h = w = SIDE
        if p.first is not None:
            total += 3 * (h * w + p.first[0] * p.first[1])
            h, w = p.crop[2], p.crop[3]
        total += 3 * (h * w + p.final[0] * p.final[1])
    return total


def device_time(images, params):
    fn = lambda: augment.apply_image(images, params)
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


def host_chain(arrays, params):
    try:
        from PIL import Image
    except ImportError:
        Image = None
    out = []
    for a, p in zip(arrays, params):
        if Image is None:
            out.append(augment.apply_image([torch.from_numpy(a)], [p])[0].permute(1, 2, 0).numpy())
            continue
        img = Image.fromarray(a[:, ::-1] if p.flip else a)
        if p.first is not None:
            img = img.resize((p.first[1], p.first[0]), Image.BILINEAR)
            y0, x0, ch, cw = p.crop
            img = img.crop((x0, y0, x0 + cw, y0 + ch))
        out.append(np.asarray(img.resize((p.final[1], p.final[0]), Image.BILINEAR)))
    return out, ("pillow" if Image is not None else "resample_reference_cpu")


def host_time(arrays, params):
    host_chain(arrays, params)
    runs = []
    for _ in range(HOST_REPS):
        t0 = time.perf_counter()
        out, how = host_chain(arrays, params)
        runs.append((time.perf_counter() - t0) * 1e6)
    return {"through": how, "median_us": round(statistics.median(runs), 1), "min_us": round(min(runs), 1),
            "max_us": round(max(runs), 1)}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(0)
    arrays = [rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8) for _ in range(2)]
    images = [torch.from_numpy(a).cuda() for a in arrays]
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "iters_per_region": ITERS, "host_reps": HOST_REPS,
           "source": "2 x [%d, %d, 3] uint8 (HWC) on the device" % (SIDE, SIDE), "cases": {}}
    for name, params in CASES.items():
        assert all(augment.supported([i], [p.first or p.final]) for i, p in zip(images, params))
        host, want = host_time(arrays, params)
        got = augment.apply_image(images, params)
        same = all(np.array_equal(g.permute(1, 2, 0).cpu().numpy(), w) for g, w in zip(got, want))
        dev = device_time(images, params)
        n = streaming_bytes(params)
        out["cases"][name] = {"params": [[p.flip, p.first, p.crop, p.final] for p in params], "device": dev, "host": host,
                              "outputs_equal": same, "streaming_bound_bytes": n,
                              "bound_bytes_per_us_at_device_median": round(n / dev["median_us"], 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
