"""The fp16 training tail (zira_grad_sqnorm_amp_f32 + zira_clip_adamw_amp_f32, ``NativeOptimTail.step_amp``) on the GPU:
``GradScaler.unscale_``, the clip, ``scaler.step`` (skip on inf / NaN), ``scaler.update`` and the gradient clear as two launches.

Layout, inputs and the bar are those of tests/test_optim_tail_gpu.py: segments of 1, 3, 5, 255, 4103 and 65536 values in two
learning-rate groups (18 blocks, the last one partial) and a bucket of one value (one block).  Yardstick for the arithmetic:
``torch.optim.AdamW(foreach=False)`` in float64 on the CPU over the scaled fp32 gradients divided by the scale in double;
``e_torch`` is measured here from torch's own fp32 chain on the device (``_amp_foreach_non_finite_check_and_unscale_``, the
trainer's clip, ``AdamW(foreach=False, fused=False)``) and the native error must be at most ``2 * e_torch + 1 ulp`` of the
largest parameter, for parameters and each moment.  The loss scale and the growth tracker are compared bit for bit with
``torch._amp_update_scale_`` on device copies.  Every figure is printed before it is asserted (``pytest -s``)."""
import pytest
import torch

import test_optim_tail_gpu as T
from test_optim_tail_gpu import BETAS, EPS, GROUPS, LRS, MAX_NORM, NUMELS, WD

pytestmark = pytest.mark.gpu

GROWTH, BACKOFF = 2.0, 0.5
ODD = dict(bucket_guard=1, param_guards=(3, 1))      # every pointer off the 16-byte grid
N = sum(NUMELS)
# where a non-finite value is placed: the first bucket element (the size-1 segment), the last element of the last, partial
# block, and the second lane of a 16-byte body group (flat 5000 .. 5003, inside the segment that starts at 4367)
POSITIONS = {"first": 0, "last": N - 1, "in_a_body_group": 5001}


class _Dev(T._Device):
    """``_Device`` for any list of sizes (that one is fixed to NUMELS)."""

    def __init__(self, params, bucket_guard=4, param_guards=(4, 4)):
        self.bufs, self.ps, self.guards = [], [], []
        for i, p in enumerate(params):
            gd = param_guards[i % 2]
            buf = torch.full((p.numel() + 2 * gd,), T.SENTINEL, device="cuda")
            buf[gd:gd + p.numel()] = p.cuda()
            self.bufs.append(buf)
            self.guards.append(gd)
            self.ps.append(buf[gd:gd + p.numel()])
        n = sum(p.numel() for p in params)
        self.gbuf = torch.full((n + 2 * bucket_guard,), T.SENTINEL, device="cuda")
        self.flat = self.gbuf[bucket_guard:bucket_guard + n]
        self.flat.zero_()
        self.bg = bucket_guard
        off = 0
        for p in self.ps:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()


def _amp_tail(dev, groups=GROUPS):
    from ziragroundingdino_amd.optim_tail import NativeOptimTail

    return NativeOptimTail(dev.ps, dev.flat, groups, betas=BETAS, eps=EPS, weight_decay=WD, amp=True)


def _dev_scalar(x, dtype):
    return torch.full((), x, dtype=dtype, device="cuda")


def _amp_run(params, state, grads, start_step, scale0, tracker0, interval, inject=None, layout=None, groups=GROUPS, lrs=LRS):
    """``len(grads)`` amp steps.  Step k's bucket is ``grads[k]`` times the scale of that moment, in fp32, with
    ``inject[k] = (flat index, value)`` written over one element.  After every step the bucket must be all zeros, ``found_inf``
    what the injection says, and scale and tracker bit-equal to ``torch._amp_update_scale_`` on device copies driven with the
    same flags.  Returns everything the tests compare, the scaled buckets and the scales among it (for the replays)."""
    inject = inject or {}
    numels = [p.numel() for p in params]
    dev = _Dev(params, **(layout or {}))
    tail = _amp_tail(dev, groups)
    if start_step:
        opt = T._adamw(dev.ps, foreach=False, fused=False) if groups is GROUPS else torch.optim.AdamW(dev.ps, lr=lrs[0])
        T._set_state(opt, dev.ps, state, start_step)
        tail.import_from(opt)
        assert tail.step_count == start_step and tail.sync_step_count() == start_step
    scale, tracker = _dev_scalar(scale0, torch.float32), _dev_scalar(tracker0, torch.int32)
    ref_scale, ref_tracker = scale.clone(), tracker.clone()
    out = dict(norms=[], flags=[], scales=[], scaled=[], after=[], dev=dev, tail=tail, scale=scale, tracker=tracker)
    for k, gs in enumerate(grads):
        cur = float(scale)
        bucket = torch.cat([g.reshape(-1) for g in gs]) * cur          # fp32, on the CPU
        if k in inject:
            bucket[inject[k][0]] = inject[k][1]
        out["scales"].append(cur)
        out["scaled"].append(bucket)
        dev.flat.copy_(bucket)
        tail.step_amp(lrs, scale, tracker, GROWTH, BACKOFF, interval, max_norm=MAX_NORM)
        flag = 1.0 if k in inject else 0.0
        torch._amp_update_scale_(ref_scale, ref_tracker, _dev_scalar(flag, torch.float32), GROWTH, BACKOFF, interval)
        out["norms"].append(tail.norm.clone())
        out["flags"].append(float(tail.found_inf))
        out["after"].append((scale.clone(), tracker.clone()))
        print("step %d scale in %.9g flag %.0f -> scale %.9g tracker %d (torch: %.9g, %d) norm %.9e"
              % (k, cur, out["flags"][-1], float(scale), int(tracker), float(ref_scale), int(ref_tracker), float(tail.norm)))
        assert int(torch.count_nonzero(dev.flat)) == 0, "the bucket is cleared by the step, skipped or not"
        assert out["flags"][-1] == flag
        assert torch.equal(scale, ref_scale) and torch.equal(tracker, ref_tracker), (k, float(scale), float(ref_scale))
        assert scale.dtype == torch.float32 and tracker.dtype == torch.int32
    assert dev.guards_untouched()
    out["params"] = [p.clone() for p in dev.ps]
    out["m"] = [t.clone() for t in tail.exp_avg.split(numels)]
    out["v"] = [t.clone() for t in tail.exp_avg_sq.split(numels)]
    out["steps"] = tail.sync_step_count()
    return out


def _replay(params, state, start_step, scaled, scales, skips, on_gpu):
    """The steps the scaler lets through, over ``scaled[k] / scales[k]``: float64 on the CPU (the yardstick), or torch's own
    fp32 chain on the device (what e_torch is measured from).  (params, exp_avg, exp_avg_sq)."""
    if on_gpu:
        dev = T._Device(params)
        ps = dev.ps
    else:
        ps = [torch.nn.Parameter(p.double().clone()) for p in params]
    opt = T._adamw(ps, foreach=False, fused=False)
    if start_step:
        T._set_state(opt, ps, state, start_step)
    for k, (bucket, s) in enumerate(zip(scaled, scales)):
        if k in skips:
            continue
        if on_gpu:
            dev.flat.copy_(bucket)
            inv = _dev_scalar(s, torch.float32).double().reciprocal().float()      # GradScaler.unscale_
            torch._amp_foreach_non_finite_check_and_unscale_([p.grad for p in ps], _dev_scalar(0.0, torch.float32), inv)
            total_norm = torch.linalg.vector_norm(dev.flat, 2.0)                   # ZiraTrainer.run_step
            dev.flat.mul_(torch.clamp(MAX_NORM / (total_norm + 1e-6), max=1.0))
            opt.step()
            dev.flat.zero_()
        else:
            for p, g in zip(ps, (bucket.double() / s).split(NUMELS)):
                p.grad = g.view_as(p).clone()
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False)
            opt.step()
    m, v = T._state_of(opt, ps)
    return [p.detach() for p in ps], m, v


def _check_bar(got, run, params, state, start_step, skips, what):
    want = _replay(params, state, start_step, run["scaled"], run["scales"], skips, on_gpu=False)
    base = _replay(params, state, start_step, run["scaled"], run["scales"], skips, on_gpu=True)
    ulp = T._ulp(max(float(p.abs().max()) for p in want[0]))
    for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
        e_nat, e_torch = T._max_err(got[k], want[k]), T._max_err(base[k], want[k])
        print("%s start %d %-10s e_native %.3e  e_torch %.3e  ratio %.3f  (bar %.3e)"
              % (what, start_step, name, e_nat, e_torch, e_nat / e_torch if e_torch else 0.0, 2 * e_torch + ulp))
        assert e_nat <= 2 * e_torch + ulp, (what, start_step, name, e_nat, e_torch, ulp)


@pytest.mark.parametrize("layout", [{}, ODD], ids=["aligned", "odd_guards"])
@pytest.mark.parametrize("start_step", [0, 1000], ids=["from_step_1", "imported_at_1000"])
@pytest.mark.parametrize("case", ["above", "below"])
def test_power_of_two_scale_is_exact(case, start_step, layout):
    """Gradients times 65536 through 5 amp steps (growth_interval 2000: the scale holds): 1 / 65536 and every product with it
    are exact, so parameters, both moments and the norm are bit-identical to the plain tail fed the unscaled gradients -- which
    also pins the bias corrections formed on the device (double pow and sqrt) to the ones the plain tail's caller forms on
    the host, at steps 1 .. 5 and 1001 .. 1005."""
    params, state, grads = T._inputs(case)
    want = T._native(case, start_step, **layout)
    got = _amp_run(params, state, grads, start_step, 65536.0, 0, 2000, layout=layout)
    assert got["steps"] == start_step + T.STEPS
    assert float(got["scale"]) == 65536.0 and int(got["tracker"]) == T.STEPS
    for name, a, b in (("param", got["params"], want[0]), ("exp_avg", got["m"], want[1]), ("exp_avg_sq", got["v"], want[2]),
                       ("norm", got["norms"], want[3])):
        diff = max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))
        print("pow2 %s start %d %-10s largest difference %.3e" % (case, start_step, name, diff))
        assert all(torch.equal(x, y) for x, y in zip(a, b)), name


@pytest.mark.parametrize("start_step", [0, 1000], ids=["from_step_1", "imported_at_1000"])
@pytest.mark.parametrize("case", ["above", "below"])
def test_scale_1000_against_fp64(case, start_step):
    """A scale that is no power of two: 1 / 1000 rounds, and so does every product with it.  Measured on an MI355X, e_native /
    e_torch: parameters 1.000 in all four cases (e_torch 4.9e-7 .. 5.5e-7), exp_avg 0.85 .. 1.50, exp_avg_sq 1.00 .. 1.12."""
    params, state, grads = T._inputs(case)
    got = _amp_run(params, state, grads, start_step, 1000.0, 0, 2000, layout=ODD)
    assert got["steps"] == start_step + T.STEPS and float(got["scale"]) == 1000.0
    _check_bar((got["params"], got["m"], got["v"]), got, params, state, start_step, (), "scale 1000 " + case)
    for k, nrm in enumerate(got["norms"]):
        ref = float(torch.linalg.vector_norm(got["scaled"][k].double() / got["scales"][k]))
        print("norm %s step %d: native %.9e fp64 %.9e" % (case, k, float(nrm), ref))
        assert abs(float(nrm) - ref) <= 1e-6 * ref


def _one_value_inputs():
    g = torch.Generator().manual_seed(11)
    return ([0.5 * torch.randn(1, generator=g)], ([0.01 * torch.randn(1, generator=g)], [1e-4 * torch.rand(1, generator=g)]),
            [[torch.randn(1, generator=g)]])


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("where", list(POSITIONS) + ["bucket_of_one"])
def test_a_non_finite_gradient_skips_the_step(where, value):
    """One inf or NaN in the bucket: parameters and moments bit-unchanged with the sentinels around them intact, the device
    step counter unchanged, the bucket all zeros, found_inf 1, a non-finite norm, scale and tracker as
    ``torch._amp_update_scale_`` leaves them (``_amp_run`` checks the last three)."""
    if where == "bucket_of_one":
        params, state, grads = _one_value_inputs()
        kw, at = dict(groups=[0], lrs=LRS[:1]), 0
    else:
        params, state, grads = T._inputs("above")
        kw, at = dict(layout=ODD), POSITIONS[where]
    run = _amp_run(params, state, grads[:1], 7, 65536.0, 1, 2, inject={0: (at, value)}, **kw)
    assert run["flags"] == [1.0]
    assert not bool(torch.isfinite(run["norms"][0])), float(run["norms"][0])
    assert run["steps"] == 7 and int(run["tail"]._step_dev) == 7
    assert float(run["scale"]) == 32768.0 and int(run["tracker"]) == 0
    for p, q in zip(run["params"], params):
        assert torch.equal(p.cpu(), q)
    for got, was in ((run["m"], state[0]), (run["v"], state[1])):
        for a, b in zip(got, was):
            assert torch.equal(a.cpu(), b)
    # and the step after it is taken: the skip left nothing behind
    dev, tail = run["dev"], run["tail"]
    dev.flat.copy_(torch.cat([g.reshape(-1) for g in grads[0]]) * 32768.0)
    tail.step_amp(kw.get("lrs", LRS), run["scale"], run["tracker"], GROWTH, BACKOFF, 2, max_norm=MAX_NORM)
    assert float(tail.found_inf) == 0.0 and tail.sync_step_count() == 8 and bool(torch.isfinite(tail.norm))
    assert all(bool(torch.isfinite(p).all()) for p in dev.ps) and not torch.equal(dev.ps[-1].cpu(), params[-1])
    assert int(run["tracker"]) == 1 and dev.guards_untouched()


def _schedule(start_step=0):
    params, state, grads = T._inputs("above")
    grads = list(grads) + [grads[0]]
    return params, state, _amp_run(params, state, grads, start_step, 1000.0, 0, 2, inject={3: (4367 + 70, float("inf"))}, layout=ODD)


def test_scale_schedule_with_a_skipped_step():
    """6 steps, growth_interval 2, an inf in step 3: the scale goes 1000, 1000, 2000, 2000 (skip), 1000, 1000 -> 2000, bit-equal
    to ``torch._amp_update_scale_`` after every step; 5 steps are counted; the parameters meet the bar against the float64
    replay that skips the same step.  Measured on an MI355X, e_native / e_torch: parameters 1.000 (4.8e-7), exp_avg 1.19,
    exp_avg_sq 1.00."""
    params, state, run = _schedule()
    assert run["flags"] == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert run["scales"] == [1000.0, 1000.0, 2000.0, 2000.0, 1000.0, 1000.0] and float(run["scale"]) == 2000.0
    assert run["steps"] == 5
    _check_bar((run["params"], run["m"], run["v"]), run, params, state, 0, (3,), "schedule")


def test_growth_that_would_overflow_keeps_the_scale():
    """From 2**127 the grown scale is inf in fp32: it is not stored, and the tracker resets all the same."""
    params, state, grads = T._inputs("below")        # 1e-5 * randn: times 2**127 stays finite
    run = _amp_run(params, state, grads[:1], 0, 2.0 ** 127, 1, 2)
    assert run["flags"] == [0.0] and run["steps"] == 1
    assert float(run["scale"]) == 2.0 ** 127 and int(run["tracker"]) == 0
    want = T._native("below", 0)                      # (the first of its five steps is this one; a power of two: exact)
    assert torch.equal(run["norms"][0], want[3][0])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "single_tensor"])
def test_two_runs_are_bit_identical_and_export_the_true_step(fused):
    a, b = _schedule()[2], _schedule()[2]
    for x, y in zip(a["params"] + a["m"] + a["v"] + a["norms"], b["params"] + b["m"] + b["v"] + b["norms"]):
        assert torch.equal(x, y)        # (the skipped step's norm is inf in both)
    assert [float(s) for s, _ in a["after"]] == [float(s) for s, _ in b["after"]]
    # 6 calls, one skipped: the optimizer gets step 5 and the moments
    dev, tail = a["dev"], a["tail"]
    tail.step_count = -1                              # (stale on the host: export_to reads the device counter)
    opt = T._adamw(dev.ps, **(dict(fused=True) if fused else dict(foreach=False, fused=False)))
    tail.export_to(opt)
    assert tail.step_count == 5
    for p, m, v in zip(dev.ps, a["m"], a["v"]):
        st = opt.state[p]
        assert float(st["step"]) == 5.0 and st["step"].is_cuda == fused
        assert torch.equal(st["exp_avg"].reshape(-1), m) and torch.equal(st["exp_avg_sq"].reshape(-1), v)
    # and back: import_from writes the device counter
    tail.import_from(opt)
    assert int(tail._step_dev) == 5


def test_step_amp_reads_nothing_back():
    """``step_amp`` under ``torch.cuda.set_sync_debug_mode("error")``: no synchronising torch call on the way.  This covers
    the torch-side code only -- the mode does not see what the library's launchers do (they enqueue two kernels and return)."""
    params, state, grads = T._inputs("above")
    dev = _Dev(params)
    tail = _amp_tail(dev)
    scale, tracker = _dev_scalar(65536.0, torch.float32), _dev_scalar(0, torch.int32)
    dev.load([g * 65536.0 for g in grads[0]])
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tail.step_amp(LRS, scale, tracker, GROWTH, BACKOFF, 2000, max_norm=MAX_NORM)
        with pytest.raises(RuntimeError):
            tail.sync_step_count()                   # (the one host read, and the mode does catch such a thing)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert tail.sync_step_count() == 1 and float(tail.found_inf) == 0.0 and int(tracker) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# trainer level

def test_trainer_fp16_steps_with_and_without_the_native_amp_tail(monkeypatch):
    """3 fp16 run_steps of the slice model with ``native_tail`` and ``native_amp_tail`` on, against the torch path, both fed the
    (scaled) gradients of a recorded run with one element of the second step's set to inf: the same scale, tracker and found_inf
    (0, 1, 0), two steps counted, nothing in ``optimizer.state``, final parameters to the bar against the float64 replay of
    steps 0 and 2, losses and norms to 1e-6 relative, and the scaler's state dict round-trips.  Measured on an MI355X: e_native
    3.0e-8, e_torch 2.0e-8 (ratio 1.54, bar 6.9e-8)."""
    from ziragroundingdino_amd.train import ZiraTrainer

    monkeypatch.setattr(ZiraTrainer, "native_amp_tail", True)
    seen = {}
    plain_run_step = ZiraTrainer.run_step

    def run_step(self, *a, **kw):
        out = plain_run_step(self, *a, **kw)
        if self.last_found_inf is not None:      # (None: no scaler in use, the fp32 recording run)
            seen.setdefault(id(self), []).append(float(self.last_found_inf))
        return out

    monkeypatch.setattr(ZiraTrainer, "run_step", run_step)
    # the recorded run is the fp32 one: its gradients are finite (the slice model's own fp16 backward overflows at the initial
    # scale, which would add skips of its own), and times the loss scale in force at each step -- 65536 until the skip halves
    # it, powers of two: exact -- they are what a GradScaler run would have left in the bucket
    rec = T._trainer_run(False, monkeypatch)
    scales = [65536.0, 65536.0, 32768.0]
    assert all(bool(torch.isfinite(p).all()) for p in rec["piles"])
    piles = [p * s for p, s in zip(rec["piles"], scales)]
    assert all(bool(torch.isfinite(p).all()) for p in piles)
    piles[1][piles[1].numel() // 2] = float("inf")
    feed = dict(piles=piles)
    a = T._trainer_run(True, monkeypatch, amp_dtype=torch.float16, inject=feed)
    b = T._trainer_run(False, monkeypatch, amp_dtype=torch.float16, inject=feed)
    ta, tb = a["trainer"], b["trainer"]
    assert tb._tail is None and ta._tail is not None
    assert ta._tail.sync_step_count() == 2
    assert not ta.optimizer.state, "the torch optimizer took no step on the native path"
    assert seen[id(ta)] == [0.0, 1.0, 0.0] and seen[id(tb)] == [0.0, 1.0, 0.0]
    assert ta.last_found_inf.dim() == 0 and tb.last_found_inf.dim() == 0 and tb.last_found_inf.is_cuda
    sa, sb = ta.grad_scaler, tb.grad_scaler
    print("scale native %r torch %r; tracker native %d torch %d" % (sa.get_scale(), sb.get_scale(), int(sa._growth_tracker),
                                                                   int(sb._growth_tracker)))
    assert sa.get_scale() == sb.get_scale() == 32768.0
    assert int(sa._growth_tracker) == int(sb._growth_tracker) == 1
    sd = sa.state_dict()
    assert sd == sb.state_dict() and sd["scale"] == 32768.0 and sd["_growth_tracker"] == 1
    fresh = torch.amp.GradScaler("cuda")
    fresh.load_state_dict(sd)
    assert fresh.state_dict() == sd and fresh.get_scale() == 32768.0
    # the float64 replay of steps 0 and 2 over the unscaled gradients
    replay = dict(a, piles=[p.cpu().double() / s for p, s in zip(piles, scales)], stepping=[True, False, True])
    want = T._replay_fp64(replay)
    e_nat, e_torch = T._max_err(a["final"], want), T._max_err(b["final"], want)
    ulp = T._ulp(max(float(p.abs().max()) for p in want))
    print("trainer fp16: e_native %.3e e_torch %.3e ratio %.3f (bar %.3e); native - torch %.3e"
          % (e_nat, e_torch, e_nat / e_torch if e_torch else 0.0, 2 * e_torch + ulp,
             T._max_err(a["final"], [p.cpu() for p in b["final"]])))
    assert e_nat <= 2 * e_torch + ulp
    assert T._max_err(a["final"], [p.cpu() for p in a["init"]]) > 100 * ulp, "the steps moved the parameters"
    for it, (la, lb) in enumerate(zip(a["losses"], b["losses"])):
        assert set(la) == set(lb)
        for k in la:
            print("loss it %d %-24s native %.9e torch %.9e" % (it, k, la[k], lb[k]))
            assert abs(la[k] - lb[k]) <= 1e-6 * max(abs(la[k]), abs(lb[k])), (it, k, la[k], lb[k])
    for it, (na, nb) in enumerate(zip(a["norms"], b["norms"])):
        print("last_grad_norm it %d native %.9e torch %.9e" % (it, na, nb))
        if it == 1:
            assert not (na < float("inf")) and not (nb < float("inf"))      # inf or NaN on both
        else:
            assert abs(na - nb) <= 1e-6 * max(na, nb)
    for fa, fb in zip(a["after"], b["after"]):
        assert int(torch.count_nonzero(fa)) == 0 and int(torch.count_nonzero(fb)) == 0
