#!/usr/bin/env python3
"""Dev: the prompt-tuning substitution (prompt.py), forward + backward through the Python calls, with the native node
(csrc/prompt.hip) over a cached table and with ``substitute_reference`` built the naive way -- from the masks, one boolean-mask
write per image and category, which is what the baseline costs without the table -- in the same process.

B = 2 images that share a caption of 13 names and one of 64 names (two tokens and a separator each: 41 and 194 tokens with
[CLS] and [SEP]), D = 256, every name with an entry in the pool; the pool entries are leaves that accumulate into ``.grad``
tensors which already exist (the trainer's flat bucket), x carries no gradient (the plain baseline).  Values on the 1/256
grid, so the outputs and gradients are compared for EQUALITY before anything is timed.  Then warm-up and REGIONS event-timed
regions of ITERS calls for each setting, alternating; the kernel launches of one call and its synchronising calls (device-to-
host copies, ``nonzero`` / ``item`` reads) are counted with the profiler.  Writes profiles/prompt.json (or the path given as
the only argument) and prints it as one JSON line."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd import prompt  # noqa: E402

REGIONS, ITERS, WARMUP = 7, 10, 3
B, D = 2, 256


def grid(shape, gen):
    return torch.round(torch.randn(*shape, generator=gen).clamp(-2, 2) * 256) / 256


def step(how, x, g, pool, names_list, masks, table, collect=False):
    """forward + backward of one substitution; the gradients accumulate into the entries' existing .grad (cleared first, by one
    multi-tensor call on both sides)"""
    torch._foreach_zero_([p.grad for p in pool.values()])
    if how == "native":
        out = prompt.substitute(x, table, pool)
    else:
        out = prompt.substitute_reference(x, (names_list, masks), pool)
    out.backward(g)
    return (out.detach(), [p.grad.clone() for p in pool.values()]) if collect else None


def timed(fns):
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


def counts(fn):
    """(kernel launches, synchronising calls) of one call, from the profiler (None where it gives none)."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
        events = list(prof.events())
        kernels = sum(1 for e in events if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                      and "memset" not in e.name.lower())
        # every aten::nonzero and aten::_local_scalar_dense (item) waits for the device; so does a device-to-host copy
        syncs = sum(1 for e in events if e.name in ("aten::nonzero", "aten::_local_scalar_dense")
                    or (str(e.device_type).endswith("CUDA") and "dtoh" in e.name.lower()))
        return kernels or None, syncs
    except Exception as exc:   # noqa: BLE001  (figures beside the timings, not worth losing them)
        print("profiler: %r" % (exc,), file=sys.stderr)
        return None, None


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "calls_per_region": ITERS, "B": B, "D": D,
           "what": "forward + backward of one substitution, x without a gradient, pool gradients accumulated into existing .grad; "
                   "native = prompt.substitute over a cached table; reference = prompt.substitute_reference from the masks "
                   "(one boolean-mask index_put per image and category); launches of native include autograd's per-leaf "
                   "accumulation (one per entry)"}
    for n_names in (13, 64):
        T = 3 * n_names + 2                                           # [CLS] a a . b b . ... [SEP]
        names = ["c%d" % i for i in range(n_names)]
        mask = torch.zeros(n_names, T, dtype=torch.bool)
        for c in range(n_names):
            mask[c, [1 + 3 * c, 2 + 3 * c]] = True
        names_list, masks = [names] * B, [mask.to(dev) for _ in range(B)]
        x, g = grid((B, T, D), gen).to(dev), grid((B, T, D), gen).to(dev)
        pool = {prompt.pool_key(n): grid((2, D), gen).to(dev).requires_grad_(True) for n in names}
        for p in pool.values():
            p.grad = torch.zeros_like(p)
        keys = list(pool)
        table = prompt.build_table(names_list, masks, keys, [2] * n_names, T)
        ref = step("reference", x, g, pool, names_list, masks, table, collect=True)
        nat = step("native", x, g, pool, names_list, masks, table, collect=True)
        assert torch.equal(ref[0], nat[0]) and all(torch.equal(a, b) for a, b in zip(ref[1], nat[1])), "native != reference"
        assert not torch.equal(nat[0], x)
        fns = {k: (lambda k=k: step(k, x, g, pool, names_list, masks, table)) for k in ("reference", "native")}
        res = {"names": n_names, "tokens": T, "pool_rows": 2 * n_names, "outputs_equal": True}
        for k, v in timed(fns).items():
            res[k] = v
            res[k]["launches"], res[k]["synchronising_calls"] = counts(fns[k])
        out["names_%d" % n_names] = res
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prompt.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
