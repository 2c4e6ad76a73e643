#!/usr/bin/env python3
"""Dev: the training tail alone at the model's size -- the 25 trainable side-branch tensors (4 622 853 values, two
learning-rate groups, the packed bucket of train.py) -- as the op chain of ``ZiraTrainer.run_step`` (``vector_norm``, add,
divide, ``clamp``, ``mul_``, fused AdamW per group, ``zero_``) and as the two native launches (csrc/optim_tail.hip).

``--mode both`` (default): warm-up, then the median of REGIONS event-timed regions of ITERS tails each, one JSON line; every
tail is preceded by a refill of the bucket (a 18.5 MB device copy, timed alone as ``refill``).  ``--mode torch|native
--iters N``: N tails of one kind and nothing else, for a ``rocprofv3 --kernel-trace --stats -- python scripts/optim_tail_time.py
--mode ...`` run of its own (the per-kernel times of ``profiles/optim_tail.json``).

``--amp``: the fp16 tail instead (``profiles/optim_tail_amp.json``): the bucket holds gradients times the loss scale, the op
chain is the one ``run_step`` issues with a ``GradScaler`` -- ``unscale_``, ``vector_norm``, add, divide, ``clamp``, ``mul_``,
``scaler.step`` (fused AdamW per group), ``scaler.update``, ``zero_`` -- and the native pair is ``NativeOptimTail.step_amp`` on
a scale and a growth tracker of its own.  Beside the medians, the kernels of one tail of each kind are counted with
``torch.profiler``."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ziragroundingdino_amd.optim_tail import NativeOptimTail  # noqa: E402

# (numel, learning-rate group) of the model's trainable tensors in named_parameters() order (zira_swint_config)
_BRANCH = lambda w: [(w, 0), (256, 0), (1, 0), (w, 1), (256, 1)]
SEGMENTS = _BRANCH(196608) + _BRANCH(49152) + _BRANCH(98304) + _BRANCH(196608) + _BRANCH(1769472)
LRS, WD, BETAS, MAX_NORM = [1e-3, 2e-4], 1e-4, (0.9, 0.999), 0.1
REGIONS, ITERS, WARMUP = 7, 100, 20


class Setup:
    def __init__(self, amp=False):
        g = torch.Generator().manual_seed(0)
        self.params = [torch.nn.Parameter((0.05 * torch.randn(x, generator=g)).cuda()) for x, _ in SEGMENTS]
        n = sum(x for x, _ in SEGMENTS)
        self.flat = torch.zeros(n, device="cuda")
        self.src = torch.randn(n, generator=g).cuda()
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        groups = [{"params": [p for p, (_, gi) in zip(self.params, SEGMENTS) if gi == k], "lr": lr} for k, lr in enumerate(LRS)]
        self.optimizer = torch.optim.AdamW(groups, lr=LRS[0], betas=BETAS, weight_decay=WD, fused=True)
        self.tail = NativeOptimTail(self.params, self.flat, [gi for _, gi in SEGMENTS], betas=BETAS, eps=1e-8, weight_decay=WD,
                                    amp=amp)
        self.n = n
        if amp:
            self.scaler = torch.amp.GradScaler("cuda")      # 65536, x2 every 2000 steps, x0.5 on inf: the reference's
            self.scaler.scale(torch.zeros((), device="cuda"))
            self.src.mul_(self.scaler.get_scale())
            self.scale, self.tracker = self.scaler._scale.clone(), self.scaler._growth_tracker.clone()

    def refill(self):
        self.flat.copy_(self.src)

    def torch_tail(self):
        total_norm = torch.linalg.vector_norm(self.flat, 2.0)
        self.flat.mul_(torch.clamp(MAX_NORM / (total_norm + 1e-6), max=1.0))
        self.optimizer.step()
        self.flat.zero_()

    def native_tail(self):
        self.tail.step(LRS, do_step=True, max_norm=MAX_NORM)

    def torch_amp_tail(self):
        sc = self.scaler
        sc.unscale_(self.optimizer)
        total_norm = torch.linalg.vector_norm(self.flat, 2.0)
        self.flat.mul_(torch.clamp(MAX_NORM / (total_norm + 1e-6), max=1.0))
        sc.step(self.optimizer)
        sc.update()
        self.flat.zero_()

    def native_amp_tail(self):
        sc = self.scaler
        self.tail.step_amp(LRS, self.scale, self.tracker, sc.get_growth_factor(), sc.get_backoff_factor(),
                           sc.get_growth_interval(), max_norm=MAX_NORM)


def launches(fn, refill):
    """The kernels of one tail (the refill's copy not counted), by name, as torch.profiler sees them."""
    from torch.profiler import ProfilerActivity, profile

    refill()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if getattr(e, "device_type", None) is not None and "CUDA" in str(e.device_type)
             and not e.name.lower().startswith(("memcpy", "memset"))]
    by_name = {}
    for x in names:
        by_name[x[:96]] = by_name.get(x[:96], 0) + 1
    return {"launches": len(names), "kernels": by_name}


def timed(fn, refill):
    for _ in range(WARMUP):
        refill()
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            refill()
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2), "max_us": round(max(per_call), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("both", "torch", "native"), default="both")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--amp", action="store_true", help="the fp16 tail: GradScaler chain against step_amp")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    s = Setup(amp=args.amp)
    torch_tail, native_tail = (s.torch_amp_tail, s.native_amp_tail) if args.amp else (s.torch_tail, s.native_tail)
    if args.mode != "both":
        fn = torch_tail if args.mode == "torch" else native_tail
        for _ in range(args.iters):
            s.refill()
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"mode": args.mode, "tails": args.iters}))
        return
    out = {"device": torch.cuda.get_device_name(0), "values": s.n, "tensors": len(SEGMENTS), "regions": REGIONS,
           "iters_per_region": ITERS,
           "refill": timed(lambda: None, s.refill),
           "torch_chain_with_refill": timed(torch_tail, s.refill),
           "native_with_refill": timed(native_tail, s.refill),
           # what the native launches must move: the norm pass reads the bucket; the update reads gradient, parameter and
           # two moments and writes all four
           "native_bytes": {"grad_sqnorm_kernel": 4 * s.n, "clip_adamw_kernel": 32 * s.n}}
    if args.amp:
        out["amp"] = True
        out["torch_chain_launches"] = launches(torch_tail, s.refill)
        out["native_launches"] = launches(native_tail, s.refill)
        out["found_inf"] = float(s.tail.found_inf)       # 0: the timed tails were steps, not skips
        out["steps_taken"] = s.tail.sync_step_count()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
