"""The CET text adapter's kernels (csrc/cet.hip, include/zira_cet.h) through ``cet._CETNative`` on the MI355X.

Oracle: ``cet_reference`` in float64 on the same device.  Yardstick: ``cet_reference`` in float32 on the same inputs -- what
``cet_apply`` runs with the switch off.  For the output, the loss and every gradient

    max|native - fp64|  <=  2 * max|reference fp32 - fp64|  +  one fp32 ulp of the tensor's largest magnitude

both errors measured here (the bar of tests/test_adapter_gpu.py).  Every figure is printed before it is asserted (``pytest -s``).

Row counts at 768 -> 1024 -> 256: a wave owns 32 rows, so M = 1, 31, 32, 33 (a second tile with one row), 2 x 41 and 2 x 195
(13 tiles: every folded sum has more than one term); 32 hidden panels are dealt to 32 waves per tile at all of them.  The
smallest geometry, 32 -> 32 -> 256, has one slice, one panel and no split.
"""
import functools

import numpy as np
import pytest
import torch

from ziragroundingdino_amd import cet as zcet
from ziragroundingdino_amd import transformer

pytestmark = pytest.mark.gpu

FULL = (768, 1024)
ROWS = [(1,), (31,), (32,), (33,), (2, 41), (2, 195)]
NAMES = ["x", "feat", "adapter_down.weight", "adapter_down.bias", "adapter_up.weight", "adapter_up.bias", "gate.weight"]
GRAD_LOSS = 0.37


def dev():
    return torch.device("cuda:0")


def ulp(t):
    return float(np.spacing(np.float32(float(t.detach().abs().max()))))


def within_bar(what, native, chain, ref):
    native, chain, ref = (t.detach().double().reshape(-1) for t in (native, chain, ref))
    assert torch.isfinite(native).all(), what
    err_c, err_n = float((chain - ref).abs().max()), float((native - ref).abs().max())
    bar = 2.0 * err_c + ulp(ref)
    print("%-48s native %.3e  reference fp32 %.3e  bar %.3e  (max|ref| %.3e)" % (what, err_n, err_c, bar, float(ref.abs().max())))
    assert err_n <= bar, "%s: native %.3e > bar %.3e (reference fp32 %.3e)" % (what, err_n, bar, err_c)


def make_module(E, H, G, use_gate, seed):
    gen = torch.Generator().manual_seed(seed)
    mod = zcet.CETAdapter(E, H, 256, num_gate_embed=G, use_gate=use_gate, gate_base_scale=1.0)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (1.0 if n == "gate.weight" else 0.05))
    return mod.to(dev())


def run(mod, x, feat, go, dtype, native, loss_type="L1", use_loss=True, x_grad=True):
    """(encoded_text, loss) and the gradients of sum(enc * go) + GRAD_LOSS * loss for x, feat and the parameters in use"""
    twin = make_twin(mod, dtype)
    leaves = [x.detach().to(dtype).requires_grad_(x_grad), feat.detach().to(dtype).requires_grad_(True)]
    params = [p for n, p in twin.named_parameters() if twin.use_gate or n != "gate.weight"]
    if native:
        enc, loss = zcet._CETNative.apply(leaves[0].reshape(-1, x.shape[-1]), leaves[1].reshape(-1, 256), *params[:4],
                                          params[4] if twin.use_gate else None, twin.gate_T, twin.gate_base_scale,
                                          zcet.LOSS_CODES[loss_type] if use_loss else zcet.LOSS_NONE)
        enc = enc.view(feat.shape)
    else:
        enc, loss = zcet.cet_reference(leaves[0], leaves[1], twin, loss_type, use_loss)
    wanted = [t for t in leaves + params if t.requires_grad]
    grads = list(torch.autograd.grad((enc * go.to(dtype)).sum() + GRAD_LOSS * loss.sum(), wanted, allow_unused=True))
    if not x_grad:
        grads.insert(0, None)
    if not twin.use_gate:
        grads.append(None)
    return [enc.detach(), loss.detach()] + grads


@functools.lru_cache(maxsize=None)
def make_twin(mod, dtype):
    """``mod``'s values in ``dtype`` (made once per module: nothing is allocated from the host inside a graph capture)"""
    twin = zcet.CETAdapter(mod.adapter_down.in_features, mod.adapter_down.out_features, 256, num_gate_embed=mod.gate.weight.shape[0],
                           gate_T=mod.gate_T, gate_base_scale=mod.gate_base_scale, use_gate=mod.use_gate).to(dev()).to(dtype)
    twin.load_state_dict({k: v.to(dtype) for k, v in mod.state_dict().items()})
    return twin


@functools.lru_cache(maxsize=None)
def case(rows, dims, G, use_gate, loss_type, use_loss):
    """module, inputs, the fp64 oracle and the fp32 reference: computed once, read by every test of the case"""
    seed = 2000 + 16 * ROWS.index(rows) + G + dims[0]
    mod = make_module(dims[0], dims[1], G, use_gate, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(*rows, dims[0], generator=gen).to(dev())
    feat = torch.randn(*rows, 256, generator=gen).to(dev())
    go = torch.randn(*rows, 256, generator=gen).to(dev())
    return (mod, x, feat, go, run(mod, x, feat, go, torch.float64, False, loss_type, use_loss),
            run(mod, x, feat, go, torch.float32, False, loss_type, use_loss))


CASES = ([(rows, FULL, 5, True, "L1", True) for rows in ROWS]
         + [((2, 41), FULL, G, True, "L1", True) for G in (1, 8)]
         + [((2, 41), FULL, 5, True, lt, True) for lt in ("L2", "Smooth_L1")]
         + [((2, 41), FULL, 5, False, "L1", True), ((2, 41), FULL, 5, True, "L1", False), ((33,), FULL, 5, False, "L1", False)]
         + [(rows, (32, 32), 5, True, "Smooth_L1", True) for rows in ((1,), (33,), (2, 195))])


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("rows, dims, G, use_gate, loss_type, use_loss", CASES, ids=case_id)
def test_native_against_fp64(rows, dims, G, use_gate, loss_type, use_loss):
    mod, x, feat, go, ref, chain = case(rows, dims, G, use_gate, loss_type, use_loss)
    got = run(mod, x, feat, go, torch.float32, True, loss_type, use_loss)
    tag = "%s %s G=%d gate=%d %s=%d" % (case_id(rows), case_id(dims), G, use_gate, loss_type, use_loss)
    for name, n, c, r in zip(["enc", "loss"] + ["grad " + k for k in NAMES], got, chain, ref):
        if r is None:       # a gate not in use has no gradient
            assert n is None and c is None
            continue
        within_bar("%s %s" % (tag, name), n, c, r)
    assert torch.equal(got[3], go)       # g_feat is the incoming gradient as it stands
    if not use_loss:
        assert float(got[1]) == 0.0


def test_x_without_a_gradient_changes_nothing_else():
    mod, x, feat, go, _, _ = case((2, 41), FULL, 5, True, "L1", True)
    a, b = run(mod, x, feat, go, torch.float32, True), run(mod, x, feat, go, torch.float32, True, x_grad=False)
    assert b[2] is None and a[2] is not None
    for name, u, v in zip(["enc", "loss"] + NAMES[1:], a[:2] + a[3:], b[:2] + b[3:]):
        assert torch.equal(u, v), name


def test_two_runs_give_the_same_bits():
    for key in (((2, 195), FULL, 5, True, "L1", True), ((33,), FULL, 5, True, "L1", True)):
        mod, x, feat, go, _, _ = case(*key)
        a, b = run(mod, x, feat, go, torch.float32, True), run(mod, x, feat, go, torch.float32, True)
        for name, u, v in zip(["enc", "loss"] + NAMES, a, b):
            assert torch.equal(u, v), name


def test_graph_replay_gives_the_eager_bits():
    mod, x, feat, go, _, _ = case((2, 195), FULL, 5, True, "L1", True)
    eager = run(mod, x, feat, go, torch.float32, True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(mod, x, feat, go, torch.float32, True)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(mod, x, feat, go, torch.float32, True)
    graph.replay()
    torch.cuda.synchronize()
    for name, u, v in zip(["enc", "loss"] + NAMES, eager, captured):
        assert torch.equal(u, v), name


def test_cet_apply_dispatches_to_the_node_and_equals_it(monkeypatch):
    mod, x, feat, go, _, _ = case((2, 41), FULL, 5, True, "L1", True)
    ran = []
    monkeypatch.setattr(zcet._CETNative, "apply", lambda *a, _f=zcet._CETNative.apply: (ran.append(a[0].shape[0]), _f(*a))[1])
    monkeypatch.setattr(transformer.Switches, "native_cet", True)
    enc, loss = zcet.cet_apply(x, feat, mod, "L1", True)
    assert ran == [82] and enc.shape == feat.shape and loss.shape == (1,)
    got = run(mod, x, feat, go, torch.float32, True)
    assert torch.equal(enc.detach(), got[0]) and torch.equal(loss.detach(), got[1])


@pytest.mark.parametrize("how", ["switch", "force", "autocast", "double", "linear", "wide"])
def test_the_node_is_not_entered(monkeypatch, how):
    def never(*a, **k):
        raise AssertionError("the native node was entered")

    mod, x, feat, _, _, chain = case((2, 41), FULL, 5, True, "L1", True)
    monkeypatch.setattr(zcet._CETNative, "apply", never)
    monkeypatch.setattr(transformer.Switches, "native_cet", how != "switch")
    if how == "force":
        monkeypatch.setattr(zcet, "FORCE_REFERENCE", True)
    if how in ("switch", "force"):
        enc, loss = zcet.cet_apply(x, feat, mod, "L1", True)
        assert torch.equal(enc.detach(), chain[0]) and torch.equal(loss.detach(), chain[1])
    elif how == "autocast":
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert zcet.cet_apply(x, feat, mod, "L1", True)[0].shape == feat.shape
    elif how == "double":
        assert zcet.cet_apply(x.double(), feat.double(), make_twin(mod, torch.float64), "L1", True)[0].dtype == torch.float64
    elif how == "linear":
        lin = zcet.LinearCETAdapter(768, 256).to(dev())
        assert zcet.cet_apply(x, feat, lin, "L1", True)[0].shape == feat.shape
    else:
        wide = zcet.CETAdapter(768, 1056, 256).to(dev())      # down_dim above the header's limit
        assert zcet.cet_apply(x, feat, wide, "L1", True)[0].shape == feat.shape
