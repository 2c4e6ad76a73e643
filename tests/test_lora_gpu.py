"""The low-rank language side branch's kernels (csrc/lora.hip, include/zira_lora.h) through ``rsb._LoRANative`` on the MI355X.

Oracle: ``lora_reference`` in float64 on the same device.  Yardstick: ``lora_reference`` in float32 on the same inputs -- what
``lora_apply`` runs with the switch off.  For the output, the loss and every gradient

    max|native - fp64|  <=  2 * max|reference fp32 - fp64|  +  one fp32 ulp of the tensor's largest magnitude

both errors measured here (the bar of tests/test_adapter_gpu.py and tests/test_cet_gpu.py).  Every figure is printed before it is
asserted (``pytest -s``).

Shapes: a wave owns 32 rows, so M = 1, 33 (a second tile with one row) and 390 (13 tiles: every folded sum has more than one
term); ``down_dim`` 32 (a single hidden panel) and 192; ``in_features`` 64 (two panels, two waves a tile) and 768 (24 panels:
24 waves a tile at M = 1 and 33, 12 waves with two panels each at M = 390).  Weights are O(1), so both SmoothL1 arms occur
(asserted where the case is made).
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_modules_golden import TOL, close

from ziragroundingdino_amd import _lib, rsb, transformer

pytestmark = pytest.mark.gpu

NAMES = ["x", "down.weight", "up.weight", "freeze_linear.weight", "scaling"]
GRAD_LOSS = 0.37
CASES = [(M, E, R) for M in (1, 33, 390) for E in (64, 768) for R in (32, 192)]


def dev():
    return torch.device("cuda:0")


def ulp(t):
    return float(np.spacing(np.float32(float(t.detach().abs().max()))))


def within_bar(what, native, chain, ref):
    native, chain, ref = (t.detach().double().reshape(-1) for t in (native, chain, ref))
    assert torch.isfinite(native).all(), what
    err_c, err_n = float((chain - ref).abs().max()), float((native - ref).abs().max())
    bar = 2.0 * err_c + ulp(ref)
    print("%-44s native %.3e  reference fp32 %.3e  bar %.3e  (max|ref| %.3e)" % (what, err_n, err_c, bar, float(ref.abs().max())))
    assert err_n <= bar, "%s: native %.3e > bar %.3e (reference fp32 %.3e)" % (what, err_n, bar, err_c)


def run(weights, x, go, dtype, native, x_grad=True):
    """(out, loss) and the gradients of sum(out * go) + GRAD_LOSS * loss for x (None without x_grad) and the four parameters"""
    leaves = [x.detach().to(dtype).requires_grad_(x_grad)] + [w.detach().to(dtype).requires_grad_(True) for w in weights]
    if native:
        out, loss = rsb._LoRANative.apply(leaves[0].reshape(-1, x.shape[-1]), *leaves[1:])
        out = out.view(go.shape)
    else:
        out, loss = rsb.lora_reference(*leaves)
    grads = list(torch.autograd.grad((out * go.to(dtype)).sum() + GRAD_LOSS * loss.sum(), leaves[0 if x_grad else 1:]))
    return [out.detach(), loss.detach().reshape(())] + ([] if x_grad else [None]) + grads


def compare(tag, got, chain, ref):
    for name, n, c, r in zip(["out", "loss"] + ["grad " + k for k in NAMES], got, chain, ref):
        within_bar("%s %s" % (tag, name), n, c, r)


@functools.lru_cache(maxsize=None)
def case(M, E, R, knee=False):
    """weights (down, up, twin, scaling), x, go, the fp64 oracle and the fp32 reference: made once, read by every test of the case"""
    gen = torch.Generator().manual_seed(3000 + M + E + R)
    wd = torch.randn(R, E, generator=gen) / E ** 0.5
    wu = torch.randn(256, R, generator=gen) / R ** 0.5
    wt = torch.randn(256, E, generator=gen) / E ** 0.5
    s = torch.tensor([0.8])
    x = torch.randn(M, E, generator=gen)
    if knee:        # row 0 is a unit vector and column 0 of W_down another: h[0] = e_0 and branch[0, n] = s * W_up[n, 0], exactly
        x[0], wd[:, 0], s = 0.0, 0.0, torch.tensor([0.5])
        x[0, 0] = wd[0, 0] = 1.0
        wu[5, 0], wu[9, 0] = 2.0, -2.0
    go = torch.randn(M, 256, generator=gen)
    weights = tuple(t.to(dev()) for t in (wd, wu, wt, s))
    x, go = x.to(dev()), go.to(dev())
    branch = weights[3] * ((x @ weights[0].T) @ weights[1].T)
    out = branch + x @ weights[2].T
    for t in (branch, out):       # both arms of SmoothL1
        assert bool((t.abs() > 1).any()) and bool((t.abs() < 1).any())
    if knee:
        assert float(branch[0, 5]) == 1.0 and float(branch[0, 9]) == -1.0
    return weights, x, go, run(weights, x, go, torch.float64, False), run(weights, x, go, torch.float32, False)


@pytest.mark.parametrize("M, E, R", CASES)
def test_native_against_fp64(M, E, R):
    weights, x, go, ref, chain = case(M, E, R)
    compare("M=%d %d->%d" % (M, E, R), run(weights, x, go, torch.float32, True), chain, ref)


def test_an_element_of_branch_exactly_at_the_knee():
    weights, x, go, ref, chain = case(33, 64, 32, True)
    compare("knee", run(weights, x, go, torch.float32, True), chain, ref)


def test_the_construction_state():
    """``down`` and ``up`` at 1e-8, a zero twin: h is 1e-7, branch 1e-16, the loss 1e-34 -- all normal numbers, none flushed."""
    mod = rsb.RepZeroLoRA(768, 256).to(dev())
    weights = (mod.down.weight, mod.up.weight, mod.freeze_linear.weight, mod.scaling)
    gen = torch.Generator().manual_seed(77)
    x, go = torch.randn(2, 195, 768, generator=gen).to(dev()), torch.randn(2, 195, 256, generator=gen).to(dev())
    ref, chain = run(weights, x, go, torch.float64, False), run(weights, x, go, torch.float32, False)
    got = run(weights, x, go, torch.float32, True)
    compare("1e-8", got, chain, ref)
    for name, g in zip(NAMES, got[2:]):
        assert torch.isfinite(g).all(), name
    for name in ("down.weight", "up.weight"):
        g = got[2 + NAMES.index(name)]
        assert float((g != 0).float().mean()) > 0.99 and float(g.abs().max()) > 1e-12, name
    assert float(got[1]) > 0.0


def test_two_runs_give_the_same_bits():
    for key in ((390, 768, 192), (33, 768, 32)):
        weights, x, go, _, _ = case(*key)
        a, b = run(weights, x, go, torch.float32, True), run(weights, x, go, torch.float32, True)
        for name, u, v in zip(["out", "loss"] + NAMES, a, b):
            assert torch.equal(u, v), name


def test_graph_replays_on_fresh_inputs_give_the_eager_bits():
    weights, x, go, _, _ = case(390, 768, 192)
    gen = torch.Generator().manual_seed(91)
    fresh = [torch.randn(x.shape, generator=gen).to(dev()) for _ in range(3)]
    eager = [run(weights, xi, go, torch.float32, True) for xi in fresh]
    static = x.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(weights, static, go, torch.float32, True)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(weights, static, go, torch.float32, True)
    for xi, want in zip(fresh, eager):       # no memset between the replays: the tickets wrap
        static.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        for name, u, v in zip(["out", "loss"] + NAMES, want, captured):
            assert torch.equal(u, v), name


def test_gx_only_when_x_takes_a_gradient(monkeypatch):
    weights, x, go, ref, chain = case(33, 768, 192)
    lib, seen = _lib.load(), []
    monkeypatch.setattr(lib, "zira_lora_bwd_f32", lambda *a, _f=lib.zira_lora_bwd_f32: (seen.append(a[15]), _f(*a))[1])
    with_x, without = run(weights, x, go, torch.float32, True), run(weights, x, go, torch.float32, True, x_grad=False)
    assert seen[0] is not None and seen[1] is None and without[2] is None
    within_bar("gx", with_x[2], chain[2], ref[2])
    for name, u, v in zip(["out", "loss"] + NAMES[1:], with_x[:2] + with_x[3:], without[:2] + without[3:]):
        assert torch.equal(u, v), name
    # through the module, as under a frozen text encoder
    mod = rsb.RepZeroLoRA(768, 256).to(dev()).train()
    out, loss = mod(x)
    (out.sum() + loss).backward()
    assert seen[2] is None and mod.down.weight.grad is not None


def test_lora_apply_dispatches_to_the_node_and_equals_it(monkeypatch):
    weights, x, go, _, _ = case(390, 768, 192)
    ran = []
    monkeypatch.setattr(rsb._LoRANative, "apply", lambda *a, _f=rsb._LoRANative.apply: (ran.append(a[0].shape), _f(*a))[1])
    monkeypatch.setattr(transformer.Switches, "native_lora", True)
    out, loss = rsb.lora_apply(x.view(2, 195, 768), *weights)
    assert ran == [(390, 768)] and out.shape == (2, 195, 256) and loss.dim() == 0
    got = run(weights, x, go, torch.float32, True)
    assert torch.equal(out.detach().view(390, 256), got[0]) and torch.equal(loss.detach(), got[1])


@pytest.mark.parametrize("how", ["switch", "force", "half", "autocast", "narrow"])
def test_the_fallbacks_are_the_reference(monkeypatch, how):
    def never(*a, **k):
        raise AssertionError("the native node was entered")

    weights, x, _, _, chain = case(33, 768, 192)
    monkeypatch.setattr(rsb._LoRANative, "apply", never)
    monkeypatch.setattr(transformer.Switches, "native_lora", how != "switch")
    if how == "force":
        monkeypatch.setattr(rsb, "FORCE_LORA_REFERENCE", True)
    if how in ("switch", "force"):
        out, loss = rsb.lora_apply(x, *weights)
        assert torch.equal(out, chain[0]) and torch.equal(loss, chain[1])
    elif how == "half":
        args = [t.half() for t in (x,) + weights]
        for u, v in zip(rsb.lora_apply(*args), rsb.lora_reference(*args)):
            assert u.dtype == torch.float16 and torch.equal(u, v)
    elif how == "autocast":
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got, want = rsb.lora_apply(x, *weights), rsb.lora_reference(x, *weights)
        assert got[0].shape == (33, 256) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    else:       # out_features = 128: a shape the header declines
        mod = rsb.RepZeroLoRA(768, 128).to(dev()).train()
        with torch.no_grad():
            mod.down.weight.copy_(weights[0])
            mod.up.weight.copy_(weights[1][:128])
            mod.freeze_linear.weight.copy_(weights[2][:128])
        out, loss = mod(x)
        want = rsb.lora_reference(x, mod.down.weight, mod.up.weight, mod.freeze_linear.weight, mod.scaling)
        assert out.shape == (33, 128) and torch.equal(out, want[0]) and torch.equal(loss, want[1])


def test_the_fixture_through_the_module(monkeypatch):
    g = torch.load(os.path.join(GOLDEN, "mod_rep_zero_lora.pt"), weights_only=True)
    g = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in g.items()}
    ran = []
    monkeypatch.setattr(rsb._LoRANative, "apply", lambda *a, _f=rsb._LoRANative.apply: (ran.append(1), _f(*a))[1])
    monkeypatch.setattr(transformer.Switches, "native_lora", True)
    mod = rsb.RepZeroLoRA(g["dims"][0], g["dims"][2], down_dim=g["dims"][1])
    mod.load_state_dict(g["state"])
    mod.to(dev()).train()
    x = g["x"].clone().requires_grad_(True)
    out, zl = mod(x)
    assert ran == [1] and zl.dim() == 0
    close(out, g["out"], TOL, "out")
    close(zl, g["zl"], TOL, "zero-interference loss")
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad((out * g["grad_out"]).sum() + g["zl_weight"] * zl, [x] + list(params.values()))
    close(grads[0], g["grad_x"], TOL, "grad_x")
    for k, gr in zip(params, grads[1:]):
        close(gr, g["grad_params"][k].to(dev()), TOL, "grad " + k)
    out_e, zl_e = mod.eval()(x)
    close(out_e, g["out_eval"], TOL, "eval out")
    assert ran == [1] and zl_e.shape == (1,) and float(zl_e) == 0.0
    mod.__rep__()
    for k, v in mod.state_dict().items():
        close(v, g["state_after_rep"][k].to(dev()), 1e-6, "after __rep__ " + k)
