#!/usr/bin/env python3
"""Dev: the trained class head of the linear-probing baseline (utils.ContrastiveEmbedwithLinear.category_logits) at the model's
size, forward + backward through the module, with the native node (csrc/clslinear.hip), with ``cls_linear_logits_reference``
(the definition in torch ops) and with the two-step composition the model would otherwise run (the module's token logits, then
``recover_to_cls_logits`` through csrc/catlogits.hip), in the same process.

R = 7 * 2 * 900 rows (six decoder layers and the encoder's set, two images, 900 queries) with 32 and with 194 text tokens;
categories of two tokens and a separator, as the mask generator makes them.  x carries no gradient: pure linear probing.

Before anything is timed the native output is compared with the definition in float64: max|native - fp64| <= 2 * max|reference
fp32 - fp64| + one fp32 ulp of the largest magnitude, asserted (the bar of tests/test_cls_linear_gpu.py), the same ratios
recorded for the two gradients (not asserted here: at 12 600 x 64 maxima a few sit closer together than two fp32 arithmetics
resolve, and the category's gradient then lands on the neighbouring token; the tests draw their inputs away from that).  Then
warm-up and REGIONS event-timed regions of ITERS calls for each setting, alternating; the kernel launches of one call are
counted with the profiler.  Writes profiles/cls_linear.json (or the path given as the only argument) and prints it as one JSON line."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import utils as zutils  # noqa: E402

REGIONS, ITERS, WARMUP = 7, 10, 3
S, B, Q, MAX_TEXT_LEN, FILL = 7, 2, 900, 256, -100.0
NAMES = ["out", "grad_cls_linear.weight", "grad_cls_linear.bias"]


def step(mod, x, td, masks, go, how):
    """forward + backward of one head call; returns the output and the two gradients"""
    for p in mod.parameters():
        p.grad = None
    if how == "composed":
        out = zutils.recover_to_cls_logits(mod(x, td), masks, FILL)
    else:
        zutils.FORCE_REFERENCE = how == "reference"
        try:
            out = mod.category_logits(x, td, masks, FILL)
        finally:
            zutils.FORCE_REFERENCE = False
    out.backward(go.to(out.dtype))
    return [out.detach(), mod.cls_linear.weight.grad, mod.cls_linear.bias.grad]


def agreement(mod, x, td, masks, go):
    import copy
    ref = step(copy.deepcopy(mod).double(), x.double(), dict(td, encoded_text=td["encoded_text"].double()), masks, go, "reference")
    chain, native = step(mod, x, td, masks, go, "reference"), step(mod, x, td, masks, go, "native")
    assert torch.equal(native[0] == FILL, ref[0] == FILL)
    over = {}
    for name, r, c, k in zip(NAMES, ref, chain, native):
        err_c, err_k = float((c.double() - r).abs().max()), float((k.double() - r).abs().max())
        bar = 2.0 * err_c + float(np.spacing(np.float32(float(r.abs().max()))))
        print("  %-26s native %.3e  reference fp32 %.3e  bar %.3e" % (name, err_k, err_c, bar), file=sys.stderr)
        if name == "out":
            assert err_k <= bar, "%s: native %.3e above the bar %.3e (reference fp32 %.3e)" % (name, err_k, bar, err_c)
        over[name] = round(err_k / bar, 3)
    return over


def timed(fns):
    """REGIONS regions of ITERS calls for each function, the functions alternating region by region"""
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    per_call = {k: [] for k in fns}
    for _ in range(REGIONS):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per_call[k].append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
            for k, v in per_call.items()}


def launches(fn):
    """Kernel launches of one call, from the profiler's device-side events (None where the profiler gives none)."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception as exc:   # noqa: BLE001  (a figure beside the timings, not worth losing them)
        print("profiler: %r" % (exc,), file=sys.stderr)
        return None


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda")
    mod = zutils.ContrastiveEmbedwithLinear(max_text_len=MAX_TEXT_LEN, hidden_dim=256).to(dev)
    with torch.no_grad():
        mod.cls_linear.weight.copy_(torch.randn(256, 256, device=dev) / 16)
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "calls_per_region": ITERS, "rows": S * B * Q,
           "what": "forward + backward of one class-head call through the module, x without a gradient; reference = "
                   "cls_linear_logits_reference (torch ops) in fp32; composed = module forward + recover_to_cls_logits (csrc/catlogits.hip)"}
    for T in (32, 194):
        print("T = %d" % T, file=sys.stderr)
        spans = [[t, t + 1] for t in range(1, T - 2, 3)]             # [CLS] a a . b b . ... [SEP]
        mask = torch.zeros(len(spans), T, dtype=torch.bool)
        for c, toks in enumerate(spans):
            mask[c, toks] = True
        masks = [mask.to(dev) for _ in range(B)]
        x, go = torch.randn(S, B, Q, 256, device=dev), torch.randn(S, B, Q, MAX_TEXT_LEN, device=dev)
        td = {"encoded_text": torch.randn(B, T, 256, device=dev), "text_token_mask": torch.ones(B, T, dtype=torch.bool, device=dev)}
        res = {"tokens": T, "categories": len(spans), "native_error_over_bar": agreement(mod, x, td, masks, go)}
        fns = {k: (lambda k=k: step(mod, x, td, masks, go, k)) for k in ("reference", "composed", "native")}
        for k, v in timed(fns).items():
            res[k] = v
            res[k]["launches"] = launches(fns[k])
        out["tokens_%d" % T] = res
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cls_linear.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
