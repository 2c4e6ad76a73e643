#!/usr/bin/env python3
"""Dev: one call of the gated adapter (adapter.py) at the model's two sizes, forward + backward through the Python module, with the
native node (csrc/adapter.hip) and with ``adapter_reference`` (the torch op chain) in the same process.

M = 44 446 rows (the encoder at two 800 x 1333 images, [2, 22223, 256]) and M = 1800 (the decoder's [900, 2, 256]); five gate
rows, gate and self-KD on, every parameter seeded noise.

Before anything is timed both are compared with ``adapter_reference`` in float64 at each size: max|native - fp64| <= 2 *
max|reference fp32 - fp64| + one fp32 ulp of the tensor's largest magnitude, asserted for the output, the loss and the six
gradients (the bar of tests/test_adapter_gpu.py), the ratios recorded.  Then warm-up and REGIONS event-timed regions of ITERS
calls for each setting, the two alternating; the kernel launches of one call are counted with the profiler.  Writes
profiles/adapter.json (or the path given as the only argument) and prints it as one JSON line."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import adapter as zadapter  # noqa: E402

REGIONS, ITERS, WARMUP = 7, 10, 3
SIZES = [("encoder_2x22223", (2, 22223)), ("decoder_900x2", (900, 2))]
NAMES = ["out", "loss", "grad_x", "grad_adapter_down.weight", "grad_adapter_down.bias", "grad_adapter_up.weight",
         "grad_adapter_up.bias", "grad_gate.weight"]


def step(mod, x, go, native):
    """forward + backward of one module call; returns the outputs and the gradients"""
    zadapter.FORCE_REFERENCE = not native
    try:
        x = x.detach().requires_grad_(True)
        for p in mod.parameters():
            p.grad = None
        out, loss = mod(x)
        torch.autograd.backward([out, loss], [go.to(out.dtype), torch.full_like(loss, 0.37)])
    finally:
        zadapter.FORCE_REFERENCE = False
    return [out.detach(), loss.detach(), x.grad] + [p.grad for p in mod.parameters()]


def agreement(mod, x, go):
    import copy
    ref = step(copy.deepcopy(mod).double(), x.double(), go, False)
    chain, native = step(mod, x, go, False), step(mod, x, go, True)
    over = {}
    for name, r, c, k in zip(NAMES, ref, chain, native):
        err_c, err_k = float((c.double() - r).abs().max()), float((k.double() - r).abs().max())
        bar = 2.0 * err_c + float(np.spacing(np.float32(float(r.abs().max()))))
        print("  %-26s native %.3e  reference fp32 %.3e  bar %.3e" % (name, err_k, err_c, bar), file=sys.stderr)
        assert err_k <= bar, "%s: native %.3e above the bar %.3e (reference fp32 %.3e)" % (name, err_k, bar, err_c)
        over[name] = round(err_k / bar, 3)
    return over


def timed_pair(fns):
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
    mod = zadapter.Adapter(num_gate_embed=5, gate_base_scale=0.1, use_gate=True, use_self_kd=True).to(dev)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            p.copy_(torch.randn_like(p) * (1.0 if n == "gate.weight" else 0.1))
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "calls_per_region": ITERS,
           "what": "forward + backward of one Adapter call through the module; reference = adapter_reference (torch ops) in fp32"}
    for name, lead in SIZES:
        print(name, file=sys.stderr)
        x, go = torch.randn(*lead, 256, device=dev), torch.randn(*lead, 256, device=dev)
        res = {"input": list(x.shape), "rows": x.numel() // 256, "native_error_over_bar": agreement(mod, x, go)}
        fns = {"reference": lambda: step(mod, x, go, False), "native": lambda: step(mod, x, go, True)}
        for k, v in timed_pair(fns).items():
            res[k] = v
            res[k]["launches"] = launches(fns[k])
        out[name] = res
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adapter.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
