#!/usr/bin/env python3
"""Dev: the side branches of the multilayer-branch variant (rsb_multilayer.py) at the model's sizes, forward + backward through
the Python modules, with ``NATIVE_EPILOGUE`` on (csrc/rsb_ml.hip behind two GEMMs) and off (the op chain: two convolutions,
scale, add, ATen's GroupNorm, two abs().mean() and autograd's backward) in the same process.

B = 2, 256 output channels, the four ``input_proj`` levels of an 800 x 1333 image behind Swin-T (1x1 convolutions from 192 / 384 /
768 channels at 100x167, 50x84, 25x42 and the 3x3 stride-2 one to 13x21) and the language branch (768 -> 256 on 195 tokens);
the branch parameters as ZiRa starts them (1e-8), the twin a random projection.

Before anything is timed the two epilogues are compared on the same contraction results at each size, against the op chain's
expressions in float64: max|native - fp64| <= 2 * max|op chain - fp64| + one fp32 ulp of the tensor's largest magnitude,
asserted for the outputs (output and loss) and recorded for the five gradients.  (Through the whole module the two paths also
hand the contractions to different libraries -- batched GEMMs / the convolution library -- whose own rounding differs.)
Then warm-up and
REGIONS event-timed regions of ITERS calls for each setting, the two alternating; the kernel launches of one call are counted
with the profiler.  Writes profiles/rsb_multilayer.json (or the path given as the only argument) and prints it as one JSON line."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch.nn.functional as F  # noqa: E402
from ziragroundingdino_amd import rsb_multilayer as ml  # noqa: E402
from ziragroundingdino_amd.dense import conv2d_pair_as_gemm  # noqa: E402

REGIONS, ITERS, WARMUP = 7, 10, 3
B, C_OUT = 2, 256
LEVELS = [("level0_100x167", 192, (100, 167), dict(kernel_size=1)), ("level1_50x84", 384, (50, 84), dict(kernel_size=1)),
          ("level2_25x42", 768, (25, 42), dict(kernel_size=1)),
          ("level3_13x21", 768, (25, 42), dict(kernel_size=3, stride=2, padding=1))]
TOKENS, TEXT_DIM = 195, 768
GROUPS, EPS = 32, 1e-5


def step(mod, x, go, native):
    """forward + backward of one module call; returns the outputs and the parameter gradients"""
    ml.NATIVE_EPILOGUE = native
    try:
        for p in mod.parameters():
            p.grad = None
        out, zl = mod(x)
        torch.autograd.backward([out, zl], [go.to(out.dtype), torch.ones_like(zl)])
    finally:
        ml.NATIVE_EPILOGUE = False
    return [out.detach(), zl.detach()] + [p.grad for p in mod.parameters()]


def epilogue_inputs(mod, x):
    """what the two contractions hand to the epilogue, computed once for both paths"""
    with torch.no_grad():
        if isinstance(mod, ml.RepZeroConv2dGN):
            twin = mod.freeze_conv
            yb, yt = conv2d_pair_as_gemm(x, mod.weight, mod.bias, twin.weight, twin.bias, mod.stride, mod.padding)
            return [yb, yt, mod.scaling.detach(), mod.freeze_gn.weight.detach(), mod.freeze_gn.bias.detach()]
        return [F.linear(x, mod.weight, mod.bias), mod.freeze_linear(x), mod.scaling.detach()]


def op_chain(yb, yt, s, gamma=None, beta=None):
    """rsb_multilayer's expressions behind the contractions"""
    if gamma is None:
        branch = s * yb
        out = branch + yt
    else:
        branch = yb * s
        out = F.group_norm(branch + yt, GROUPS, gamma, beta, EPS)
    return out, branch.abs().mean() + out.abs().mean()


def native_epilogue(yb, yt, s, gamma=None, beta=None):
    if gamma is None:
        return ml._L1Epilogue.apply(yb, yt, s)
    return ml._GNEpilogue.apply(yb, yt, s, gamma, beta, GROUPS, EPS)


def epilogue_run(fn, leaves, go):
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves]
    out, zl = fn(*leaves)
    grads = torch.autograd.grad([out, zl], leaves, [go.to(out.dtype), torch.ones_like(zl)])
    return [out.detach(), zl.detach()] + list(grads)


def agreement(mod, x, go):
    """the native epilogue's error over the bar of the docstring, on the inputs the contractions give it at this size:
    asserted <= 1 for the outputs, recorded for the gradients"""
    leaves = epilogue_inputs(mod, x)
    names = ["out", "loss", "g_branch", "g_twin", "g_scaling", "g_gamma", "g_beta"]
    ref = epilogue_run(op_chain, [t.double() for t in leaves], go)
    chain = epilogue_run(op_chain, leaves, go)
    native = epilogue_run(native_epilogue, leaves, go)
    over = {}
    for name, r, c, k in zip(names, ref, chain, native):
        err_c, err_k = float((c.double() - r).abs().max()), float((k.double() - r).abs().max())
        bar = 2.0 * err_c + float(np.spacing(np.float32(float(r.abs().max()))))
        print("  %-10s native %.3e  chain %.3e  bar %.3e" % (name, err_k, err_c, bar), file=sys.stderr)
        assert err_k <= bar or name not in ("out", "loss"), "%s: native %.3e above the bar %.3e (op chain %.3e)" % (name, err_k, bar, err_c)
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


def measure(name, mod, x, go):
    print(name, file=sys.stderr)
    ml.NATIVE_EPILOGUE = True
    try:
        assert "Epilogue" in type(mod(x)[0].grad_fn).__name__, "the native path declined this shape"
    finally:
        ml.NATIVE_EPILOGUE = False
    res = {"input": list(x.shape), "native_error_over_bar": agreement(mod, x, go)}
    fns = {"op_chain": lambda: step(mod, x, go, False), "native": lambda: step(mod, x, go, True)}
    for k, v in timed_pair(fns).items():
        res[k] = v
        res[k]["launches"] = launches(fns[k])
    return res


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "channels": C_OUT, "regions": REGIONS, "calls_per_region": ITERS,
           "what": "forward + backward of one module call, both contractions included; op_chain = NATIVE_EPILOGUE off"}
    for name, c_in, (h, w), kw in LEVELS:
        mod = ml.RepZeroConv2dGN(c_in, C_OUT, **kw).to(dev).train()
        with torch.no_grad():
            mod.freeze_conv.weight.normal_(0.0, (c_in * kw["kernel_size"] ** 2) ** -0.5)
            mod.freeze_conv.bias.normal_(0.0, 0.1)
        x = torch.randn(B, c_in, h, w, device=dev)
        y = mod.freeze_conv(x)
        out[name] = measure(name, mod, x, torch.randn_like(y))
    lin = ml.RepZeroLinear(TEXT_DIM, C_OUT).to(dev).train()
    with torch.no_grad():
        lin.freeze_linear.weight.normal_(0.0, TEXT_DIM ** -0.5)
    x = torch.randn(B, TOKENS, TEXT_DIM, device=dev)
    out["language_195x768"] = measure("language", lin, x, torch.randn(B, TOKENS, C_OUT, device=dev))
    keys = [k for k in out if isinstance(out[k], dict)]
    out["sum_over_branches_us"] = {s: round(sum(out[k][s]["median_us"] for k in keys), 1) for s in ("op_chain", "native")}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rsb_multilayer.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
