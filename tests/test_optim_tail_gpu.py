"""The native training tail (csrc/optim_tail.hip, ziragroundingdino_amd/optim_tail.py) on the GPU.

Yardstick: ``torch.optim.AdamW(foreach=False)`` with ``clip_grad_norm_(..., 0.1)`` on float64 CPU copies.  The bar is
measured in the test: torch's own fp32 path (``fused=False``) runs on the same inputs, ``e_torch`` is its largest error
against fp64, and the native error must be at most ``2 * e_torch + 1 ulp`` of the largest parameter magnitude -- for the
parameters and for each of the two moments.  (The factor 2: the operation order inside the update may differ, and the norm
is summed in double.)  Every figure is printed before it is asserted (``pytest -s``)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NUMELS = [1, 3, 5, 255, 4103, 65536]      # starts 0, 1, 4, 9, 264, 4367 in the packed bucket: 17 blocks of 4096
GROUPS = [0, 1, 0, 1, 0, 1]
LRS = [1e-3, 2e-4]
WD, BETAS, EPS, MAX_NORM = 1e-4, (0.9, 0.999), 1e-8, 0.1
STEPS = 5
SENTINEL = 12345.0
CASES = ("above", "below", "some_zeros", "all_zero")


def _ulp(x):
    return float(np.spacing(np.float32(x)))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Initial parameters, an AdamW state to import (step 1000) and STEPS fresh gradients per tensor, as fp32 CPU tensors."""
    g = torch.Generator().manual_seed(CASES.index(case) + 1)
    params = [0.5 * torch.randn(x, generator=g) for x in NUMELS]
    mask = [torch.rand(x, generator=g) < 0.3 for x in NUMELS]      # some_zeros: the same elements every step, so v stays 0
    exp_avg = [0.01 * torch.randn(x, generator=g) for x in NUMELS]
    exp_avg_sq = [1e-4 * torch.rand(x, generator=g) for x in NUMELS]
    grads = []
    for _ in range(STEPS):
        gs = [torch.randn(x, generator=g) for x in NUMELS]
        if case == "below":         # norm ~ 2.6e-3 < 0.1: the scale is exactly 1
            gs = [1e-5 * t for t in gs]
        elif case == "all_zero":
            gs = [torch.zeros_like(t) for t in gs]
        elif case == "some_zeros":
            gs = [t.masked_fill(m, 0.0) for t, m in zip(gs, mask)]
        grads.append(gs)
    if case == "some_zeros":
        exp_avg = [t.masked_fill(m, 0.0) for t, m in zip(exp_avg, mask)]
        exp_avg_sq = [t.masked_fill(m, 0.0) for t, m in zip(exp_avg_sq, mask)]
    return params, (exp_avg, exp_avg_sq), grads


def _adamw(ps, **kw):
    groups = [{"params": [p for p, g in zip(ps, GROUPS) if g == gi], "lr": lr} for gi, lr in enumerate(LRS)]
    return torch.optim.AdamW(groups, lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD, **kw)


def _set_state(opt, ps, state, step, on_device=False):
    for p, m, v in zip(ps, state[0], state[1]):
        opt.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32, device=p.device if on_device else "cpu"),
                        "exp_avg": m.to(p).clone(), "exp_avg_sq": v.to(p).clone()}


def _state_of(opt, ps):
    zeros = lambda p: torch.zeros_like(p)
    return ([opt.state[p]["exp_avg"] if p in opt.state else zeros(p) for p in ps],
            [opt.state[p]["exp_avg_sq"] if p in opt.state else zeros(p) for p in ps])


@functools.lru_cache(maxsize=None)
def _torch_cpu(case, dtype, start_step):
    """The yardstick (float64) or torch's own fp32 path, on the CPU: (params, exp_avg, exp_avg_sq, norms)."""
    params, state, grads = _inputs(case)
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params]
    opt = _adamw(ps, foreach=False, fused=False)
    if start_step:
        _set_state(opt, ps, state, start_step)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(dtype).clone()
        norms.append(torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False).detach().clone())
        opt.step()
    m, v = _state_of(opt, ps)
    return [p.detach() for p in ps], m, v, norms


class _Device:
    """Parameters and the bucket on the GPU, each inside a larger buffer of sentinels: ``guard`` elements on either side
    (4 keeps the 16-byte alignment real tensors have, odd ones shift every pointer off it)."""

    def __init__(self, params, bucket_guard=4, param_guards=(4, 4)):
        self.bufs, self.ps, self.guards = [], [], []
        for i, p in enumerate(params):
            gd = param_guards[i % 2]
            buf = torch.full((p.numel() + 2 * gd,), SENTINEL, device="cuda")
            buf[gd:gd + p.numel()] = p.cuda()
            self.bufs.append(buf)
            self.guards.append(gd)
            self.ps.append(buf[gd:gd + p.numel()])
        n = sum(NUMELS)
        self.gbuf = torch.full((n + 2 * bucket_guard,), SENTINEL, device="cuda")
        self.flat = self.gbuf[bucket_guard:bucket_guard + n]
        self.flat.zero_()
        self.bg = bucket_guard
        off = 0
        for p in self.ps:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    def load(self, gs):
        self.flat.copy_(torch.cat([g.reshape(-1) for g in gs]))

    def guards_untouched(self):
        ok = bool((self.gbuf[:self.bg] == SENTINEL).all()) and bool((self.gbuf[-self.bg:] == SENTINEL).all())
        for buf, gd in zip(self.bufs, self.guards):
            ok = ok and bool((buf[:gd] == SENTINEL).all()) and bool((buf[-gd:] == SENTINEL).all())
        return ok


def _tail(dev):
    from ziragroundingdino_amd.optim_tail import NativeOptimTail

    return NativeOptimTail(dev.ps, dev.flat, GROUPS, betas=BETAS, eps=EPS, weight_decay=WD)


def _split(flat):
    return [t.clone() for t in flat.split(NUMELS)]


def _native(case, start_step, **layout):
    params, state, grads = _inputs(case)
    dev = _Device(params, **layout)
    tail = _tail(dev)
    if start_step:
        opt = _adamw(dev.ps, foreach=False, fused=False)
        _set_state(opt, dev.ps, state, start_step)
        tail.import_from(opt)
        assert tail.step_count == start_step
    norms = []
    for gs in grads:
        dev.load(gs)
        tail.step(LRS, do_step=True, max_norm=MAX_NORM)
        norms.append(tail.norm.clone())
        assert int(torch.count_nonzero(dev.flat)) == 0, "the bucket is cleared by the step"
    assert tail.step_count == start_step + STEPS
    assert dev.guards_untouched()
    return [p.clone() for p in dev.ps], _split(tail.exp_avg), _split(tail.exp_avg_sq), norms


def _max_err(got, want):
    return max(float((a.detach().cpu().double() - b.double()).abs().max()) for a, b in zip(got, want))


def _check_bar(got, case, start_step, what):
    """got = (params, exp_avg, exp_avg_sq) against the fp64 yardstick, the bar from torch's fp32 path; returns the ratios."""
    want, base = _torch_cpu(case, torch.float64, start_step), _torch_cpu(case, torch.float32, start_step)
    ulp = _ulp(max(float(p.abs().max()) for p in want[0]))
    ratios = {}
    for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
        e_nat, e_torch = _max_err(got[k], want[k]), _max_err(base[k], want[k])
        ratios[name] = e_nat / e_torch if e_torch > 0 else (0.0 if e_nat == 0 else float("inf"))
        print("%s %s start %d %-10s e_native %.3e  e_torch %.3e  ratio %.3f  (bar %.3e)"
              % (what, case, start_step, name, e_nat, e_torch, ratios[name], 2 * e_torch + ulp))
        assert e_nat <= 2 * e_torch + ulp, (what, case, start_step, name, e_nat, e_torch, ulp)
    return ratios


def _check_norms(norms, case, start_step):
    want = _torch_cpu(case, torch.float64, start_step)[3]
    for got, ref in zip(norms, want):
        got, ref = float(got), float(ref)
        print("norm %s: native %.9e fp64 %.9e" % (case, got, ref))
        assert abs(got - ref) <= 1e-6 * ref, (case, got, ref)


@pytest.mark.parametrize("start_step", [0, 1000], ids=["from_step_1", "imported_at_1000"])
@pytest.mark.parametrize("case", CASES)
def test_five_steps_against_fp64(case, start_step):
    """Segments of 1, 3, 5, 255, 4103 and 65536 values in two learning-rate groups, 5 steps with fresh gradients: norm above
    the clip, below it (scale exactly 1), gradients with exact zeros (v = 0: the denominator is eps), all-zero gradients.
    Measured on an MI355X, e_native / e_torch: parameters 1.000 in all eight cases (e_torch 4.3e-7 .. 5.5e-7), exp_avg
    0.25 .. 1.00, exp_avg_sq 0.20 .. 1.00; the norm slot within 3e-8 relative of the fp64 norm."""
    params, m, v, norms = _native(case, start_step)
    _check_bar((params, m, v), case, start_step, "kernel")
    _check_norms(norms, case, start_step)
    if case == "below":
        assert all(float(x) < MAX_NORM for x in norms)
    if case == "above":
        assert all(float(x) > MAX_NORM for x in norms)
    if case == "some_zeros" and start_step == 0:
        assert any(bool((t == 0).any()) for t in v)


def test_pointers_off_the_16_byte_grid():
    """The same five steps with every parameter pointer and the bucket shifted off 16-byte alignment (odd guards): the
    16-byte accesses need dword alignment only.  Bit-identical to the aligned layout, guards intact."""
    a = _native("above", 0)
    b = _native("above", 0, bucket_guard=1, param_guards=(3, 1))
    _check_bar(b[:3], "above", 0, "misaligned")
    # (the bucket's blocks and the 16-byte groups are laid on the flat index, not on addresses: the same sums, the same bits)
    for x, y in zip(a[0] + a[1] + a[2] + a[3], b[0] + b[1] + b[2] + b[3]):
        assert torch.equal(x, y)


def test_two_runs_are_bit_identical():
    a, b = _native("above", 1000), _native("above", 1000)
    for x, y in zip(a[0] + a[1] + a[2] + a[3], b[0] + b[1] + b[2] + b[3]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case", ["above", "below"])
def test_clip_only_mode(case):
    """do_step = 0: the bucket becomes grad * scale (same bar: torch's fp32 ``mul_(clamp(...))`` against fp64, one ulp of the
    largest scaled gradient), the norm is written, parameters, moments and the step counter are bit-unchanged."""
    params, state, grads = _inputs(case)
    dev = _Device(params, bucket_guard=1, param_guards=(4, 3))
    tail = _tail(dev)
    opt = _adamw(dev.ps, foreach=False, fused=False)
    _set_state(opt, dev.ps, state, 7)
    tail.import_from(opt)
    before = [p.clone() for p in dev.ps], tail.exp_avg.clone(), tail.exp_avg_sq.clone()
    dev.load(grads[0])
    g32 = torch.cat(grads[0])
    tail.step(LRS, do_step=False, max_norm=MAX_NORM)
    g64 = g32.double()
    n64 = torch.linalg.vector_norm(g64)
    want = g64 * torch.clamp(MAX_NORM / (n64 + 1e-6), max=1.0)
    n32 = torch.linalg.vector_norm(g32)
    base = g32 * torch.clamp(MAX_NORM / (n32 + 1e-6), max=1.0)
    e_nat, e_torch = _max_err([dev.flat], [want]), _max_err([base], [want])
    print("clip only %s: e_native %.3e e_torch %.3e" % (case, e_nat, e_torch))
    assert e_nat <= 2 * e_torch + _ulp(float(want.abs().max()))
    if case == "below":
        assert torch.equal(dev.flat.cpu(), g32)     # scale exactly 1: the gradients pass as they are
    assert abs(float(tail.norm) - float(n64)) <= 1e-6 * float(n64)
    assert tail.step_count == 7
    assert all(torch.equal(p, q) for p, q in zip(dev.ps, before[0]))
    assert torch.equal(tail.exp_avg, before[1]) and torch.equal(tail.exp_avg_sq, before[2])
    assert dev.guards_untouched()


def _torch_gpu_step(dev, opt, gs):
    """One step of the trainer's torch tail on the GPU."""
    dev.load(gs)
    total_norm = torch.linalg.vector_norm(dev.flat, 2.0)
    dev.flat.mul_(torch.clamp(MAX_NORM / (total_norm + 1e-6), max=1.0))
    opt.step()
    dev.flat.zero_()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "single_tensor"])
def test_round_trip_through_a_torch_optimizer(fused):
    """3 native steps, export_to, 2 torch steps -- and 2 torch steps, import_from, 3 native steps -- against 5 torch-only
    steps (the fp64 yardstick and the bar of the first test)."""
    params, _, grads = _inputs("above")
    kw = dict(fused=True) if fused else dict(foreach=False, fused=False)
    # native, then torch
    dev = _Device(params)
    tail, opt = _tail(dev), _adamw(dev.ps, **kw)
    for gs in grads[:3]:
        dev.load(gs)
        tail.step(LRS, do_step=True, max_norm=MAX_NORM)
    tail.export_to(opt)
    for gs in grads[3:]:
        _torch_gpu_step(dev, opt, gs)
    assert all(float(opt.state[p]["step"]) == 5.0 for p in dev.ps)
    m, v = _state_of(opt, dev.ps)
    _check_bar((dev.ps, m, v), "above", 0, "native->torch")
    # torch, then native
    dev = _Device(params)
    tail, opt = _tail(dev), _adamw(dev.ps, **kw)
    for gs in grads[:2]:
        _torch_gpu_step(dev, opt, gs)
    tail.import_from(opt)
    assert tail.step_count == 2
    for gs in grads[2:]:
        dev.load(gs)
        tail.step(LRS, do_step=True, max_norm=MAX_NORM)
    _check_bar((dev.ps, _split(tail.exp_avg), _split(tail.exp_avg_sq)), "above", 0, "torch->native")
    assert dev.guards_untouched()


# ---------------------------------------------------------------------------------------------------------------------------
# trainer level: the smallest model the trainer tests build (tests/test_train_step.py: the shrunken ZiRa slice)

def _trainer_run(native, monkeypatch, batch_size_scale=1, rebind_after=None, amp_dtype=None, inject=None, steps=3):
    """``steps`` run_steps from the seeded slice model.  The gradients that reach the tail are recorded through
    ``on_reduced_grad``; with ``inject`` (another run's record) they are REPLACED by that run's, so both tails see the same
    bits whatever the model's own run-to-run differences (atomics in the backward kernels) are."""
    from conftest import GOLDEN
    from test_train_step import _SliceWrapper, build_slice_model, slice_inputs
    from ziragroundingdino_amd.train import ZiraTrainer

    monkeypatch.setattr(ZiraTrainer, "native_tail", native)
    g = torch.load(os.path.join(GOLDEN, "step_zira_slice.pt"), weights_only=False)
    model = build_slice_model(g, "cuda")
    trainer = ZiraTrainer(model, batch_size_scale=batch_size_scale, amp_dtype=amp_dtype)
    data = slice_inputs(g, model, "cuda")
    trainer.model = _SliceWrapper(model)
    rec = dict(piles=[], losses=[], norms=[], after=[], stepping=[], trainer=trainer)

    def hook(flat):
        if inject is not None:
            flat.copy_(inject["piles"][len(rec["piles"])])
        rec["piles"].append(flat.detach().clone())

    trainer.on_reduced_grad = hook
    rec["names"], rec["init"] = list(trainer.names), [p.detach().clone() for p in trainer.params]
    rec["first"] = 0
    for it in range(steps):
        if rebind_after is not None and it == rebind_after:
            trainer.after_train(["fish"])       # __rep__: new `scaling` parameters, a new bucket, a fresh optimizer state
            rec["names"], rec["init"], rec["first"] = list(trainer.names), [p.detach().clone() for p in trainer.params], it
        rec["stepping"].append(trainer.iter % trainer.batch_size_scale == 0)
        out = trainer.run_step(data)
        rec["losses"].append({k: float(v) for k, v in out.items()})
        rec["norms"].append(float(trainer.last_grad_norm))
        rec["after"].append(trainer.flat_grad.detach().clone())
    rec["final"] = [p.detach().clone() for p in trainer.params]
    return rec


def _replay_fp64(rec):
    """The tail in float64 on the CPU over the recorded gradients, from the parameters at the (latest) binding."""
    from ziragroundingdino_amd.train import lr_factor

    ps = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in rec["init"]]
    groups = [{"params": [p], "lr": 1e-3 * lr_factor(n)} for n, p in zip(rec["names"], ps)]
    opt = torch.optim.AdamW(groups, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-4, foreach=False, fused=False)
    sizes = [p.numel() for p in ps]
    for it in range(rec["first"], len(rec["piles"])):
        for p, gflat in zip(ps, rec["piles"][it].cpu().double().split(sizes)):
            p.grad = gflat.view_as(p).clone()
        torch.nn.utils.clip_grad_norm_(ps, 0.1, foreach=False)
        if rec["stepping"][it]:
            opt.step()
    return [p.detach() for p in ps]


@pytest.mark.parametrize("variant", ["plain", "accumulate_2", "across_after_train"])
def test_trainer_steps_with_and_without_the_native_tail(variant, monkeypatch):
    """3 run_steps with ``native_tail = True`` against ``False`` from the same seed (the second run is fed the first one's
    gradients, see ``_trainer_run``): trainable parameters to the bar of the kernel test -- each run against the float64
    replay of the tail over the same gradients --, every loss entry and ``last_grad_norm`` to 1e-6 relative; with
    ``batch_size_scale = 2`` iteration 1 clips without stepping; ``after_train()`` rebinds between the first and second step."""
    kw = {"plain": {}, "accumulate_2": {"batch_size_scale": 2}, "across_after_train": {"rebind_after": 1}}[variant]
    a = _trainer_run(True, monkeypatch, **kw)
    assert a["trainer"]._tail is not None and a["trainer"]._tail.step_count == (2 if variant != "plain" else 3)
    assert not a["trainer"].optimizer.state, "the torch optimizer took no step on the native path"
    b = _trainer_run(False, monkeypatch, inject=a, **kw)
    assert b["trainer"]._tail is None
    assert a["names"] == b["names"]
    want_a, want_b = _replay_fp64(a), _replay_fp64(b)
    e_nat, e_torch = _max_err(a["final"], want_a), _max_err(b["final"], want_b)
    ulp = _ulp(max(float(p.abs().max()) for p in want_a))
    direct = _max_err(a["final"], [p.cpu() for p in b["final"]])
    print("trainer %s: e_native %.3e e_torch %.3e ratio %.3f (bar %.3e); native - torch %.3e"
          % (variant, e_nat, e_torch, e_nat / e_torch if e_torch else 0.0, 2 * e_torch + ulp, direct))
    assert e_nat <= 2 * e_torch + ulp
    moved = _max_err(a["final"], [p.cpu() for p in a["init"]])
    assert moved > 100 * ulp, "the steps moved the parameters"
    for it, (la, lb) in enumerate(zip(a["losses"], b["losses"])):
        assert set(la) == set(lb)
        for k in la:
            print("loss it %d %-24s native %.9e torch %.9e" % (it, k, la[k], lb[k]))
            assert abs(la[k] - lb[k]) <= 1e-6 * max(abs(la[k]), abs(lb[k])), (it, k, la[k], lb[k])
    for na, nb in zip(a["norms"], b["norms"]):
        print("last_grad_norm native %.9e torch %.9e" % (na, nb))
        assert abs(na - nb) <= 1e-6 * max(na, nb)
    for it, (fa, fb) in enumerate(zip(a["after"], b["after"])):
        if a["stepping"][it]:
            assert int(torch.count_nonzero(fa)) == 0 and int(torch.count_nonzero(fb)) == 0
        else:       # the clipped pile stays in the bucket: the same in both, to an ulp of its largest entry
            assert float(fa.abs().max()) > 0
            assert float((fa.double() - fb.double()).abs().max()) <= 2 * _ulp(float(fb.abs().max()))


def test_fp16_with_a_grad_scaler_stays_on_the_torch_path(monkeypatch):
    """amp_dtype = float16: ``unscale_`` and the inf-skip belong to the GradScaler, the native tail declines and the steps are
    the ones the switch-off trainer takes (same gradients in: the same bits out)."""
    a = _trainer_run(True, monkeypatch, amp_dtype=torch.float16)
    assert a["trainer"]._tail is not None and a["trainer"]._tail.step_count == 0
    assert not bool(a["trainer"]._tail.exp_avg.any())
    b = _trainer_run(False, monkeypatch, amp_dtype=torch.float16, inject=a)
    for p, q in zip(a["final"], b["final"]):
        assert torch.equal(p, q)
    assert a["norms"] == b["norms"] or all(not np.isfinite(x) or x == y for x, y in zip(a["norms"], b["norms"]))
    assert a["trainer"].grad_scaler.get_scale() == b["trainer"].grad_scaler.get_scale()
