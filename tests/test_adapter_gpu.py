"""The gated adapter's kernels (csrc/adapter.hip, include/zira_adapter.h) through ``adapter.Adapter`` on the MI355X.

Oracle: ``adapter_reference`` in float64 on the same device.  Yardstick: ``adapter_reference`` in float32 on the same inputs --
what the module runs with the switch off.  For the output, the loss and each of the six gradients

    max|native - fp64|  <=  2 * max|reference fp32 - fp64|  +  one fp32 ulp of the tensor's largest magnitude

both errors measured here (the bar of tests/test_rsb_ml_gpu.py).  Every figure is printed before it is asserted (``pytest -s``).

Row counts: a block owns a panel of 128 rows (four waves of 32), so M = 1, 127, 128, 129, three panels plus five rows (more than
one block in every folded sum, a partial wave and idle waves in the last block) and the decoder's 1800 as [900, 2, 256].
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adapter_cases as cases

from ziragroundingdino_amd import adapter as zadapter
from ziragroundingdino_amd import transformer

pytestmark = pytest.mark.gpu

PANEL = 128
ROWS = [(1,), (PANEL - 1,), (PANEL,), (PANEL + 1,), (3 * PANEL + 5,), (900, 2)]
NAMES = ["x", "adapter_down.weight", "adapter_down.bias", "adapter_up.weight", "adapter_up.bias", "gate.weight"]
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
    print("%-40s native %.3e  reference fp32 %.3e  bar %.3e  (max|ref| %.3e)" % (what, err_n, err_c, bar, float(ref.abs().max())))
    assert err_n <= bar, "%s: native %.3e > bar %.3e (reference fp32 %.3e)" % (what, err_n, bar, err_c)


def make_module(G, use_gate, use_self_kd, seed):
    gen = torch.Generator().manual_seed(seed)
    mod = zadapter.Adapter(num_gate_embed=G, use_gate=use_gate, use_self_kd=use_self_kd, gate_base_scale=0.5)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (1.0 if n == "gate.weight" else 0.1))
    return mod.to(dev())


def run(mod, x, go, dtype, native):
    """(out, loss) and the gradients of sum(out * go) + GRAD_LOSS * loss for x and the parameters in use, in NAMES' order"""
    params = [p for n, p in mod.named_parameters() if mod.use_gate or n != "gate.weight"]
    leaves = [x.detach().to(dtype).requires_grad_(True)] + [p.detach().to(dtype).requires_grad_(True) for p in params]
    if native:
        out, loss = zadapter._AdapterNative.apply(leaves[0].reshape(-1, 256), *leaves[1:5], leaves[5] if mod.use_gate else None,
                                                  mod.gate_T, mod.gate_base_scale, mod.use_self_kd)
        out = out.view(x.shape)
    else:
        out, loss = zadapter.adapter_reference(leaves[0], tuple(leaves[1:5]) + (leaves[5] if mod.use_gate else None,), F.relu, None,
                                               mod.gate_T, mod.gate_base_scale, mod.use_gate, mod.use_self_kd)
    grads = torch.autograd.grad((out * go.to(dtype)).sum() + GRAD_LOSS * loss.sum(), leaves, allow_unused=True)
    return [out.detach(), loss.detach()] + [g for g in grads]


@functools.lru_cache(maxsize=None)
def case(rows, G, use_gate, use_self_kd):
    """module, inputs, the fp64 oracle and the fp32 reference: computed once, read by every test of the case"""
    seed = 1000 + 16 * ROWS.index(rows) + G
    mod = make_module(G, use_gate, use_self_kd, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(*rows, 256, generator=gen).to(dev())
    go = torch.randn(*rows, 256, generator=gen).to(dev())
    return mod, x, go, run(mod, x, go, torch.float64, False), run(mod, x, go, torch.float32, False)


CASES = [(rows, G, True, True) for rows in ROWS for G in (5, 8)] + [((3 * PANEL + 5,), 5, False, True), ((3 * PANEL + 5,), 5, True, False),
                                                                     ((900, 2), 5, False, False), ((1,), 5, False, True)]


@pytest.mark.parametrize("rows, G, use_gate, use_self_kd", CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(int(v)))
def test_native_against_fp64(rows, G, use_gate, use_self_kd):
    mod, x, go, ref, chain = case(rows, G, use_gate, use_self_kd)
    got = run(mod, x, go, torch.float32, True)
    for name, n, c, r in zip(["out", "loss"] + ["grad " + k for k in NAMES], got, chain, ref):
        if r is None:       # the loss term without use_self_kd carries no gradient of its own; a gate not in use has none
            assert n is None and c is None
            continue
        within_bar("%s G=%d gate=%d kd=%d %s" % ("x".join(map(str, rows)), G, use_gate, use_self_kd, name), n, c, r)
    if not use_self_kd:
        assert float(got[1]) == 0.0


def recorded(monkeypatch):
    """the row counts of the calls that enter the native node from here on"""
    ran = []
    monkeypatch.setattr(zadapter._AdapterNative, "apply",
                        lambda *a, _f=zadapter._AdapterNative.apply: (ran.append(a[0].shape[0]), _f(*a))[1])
    return ran


def test_module_dispatches_to_the_node_and_equals_it(monkeypatch):
    mod, x, go, _, _ = case((900, 2), 5, True, True)
    ran = recorded(monkeypatch)
    out, loss = mod(x)
    assert ran == [1800] and out.shape == x.shape and loss.shape == (1,)
    got = run(mod, x, go, torch.float32, True)
    assert torch.equal(out, got[0]) and torch.equal(loss, got[1])


def test_two_runs_give_the_same_bits():
    for key in (((3 * PANEL + 5,), 8, True, True), ((900, 2), 5, True, True)):
        mod, x, go, _, _ = case(*key)
        a, b = run(mod, x, go, torch.float32, True), run(mod, x, go, torch.float32, True)
        for name, u, v in zip(["out", "loss"] + NAMES, a, b):
            assert torch.equal(u, v), name


def test_tie_goes_to_the_first_gate_row():
    mod = make_module(5, True, True, 77)
    with torch.no_grad():
        mod.gate.weight[3].copy_(mod.gate.weight[1])
        gen = torch.Generator().manual_seed(78)
        x = (torch.randn(3 * PANEL + 5, 256, generator=gen).to(dev()) + 0.5 * mod.gate.weight[torch.arange(3 * PANEL + 5) % 5])
        go = torch.randn(3 * PANEL + 5, 256, generator=gen).to(dev())
        xd, gd = x.double(), mod.gate.weight.double()
        cos = (xd / xd.norm(dim=-1, keepdim=True)) @ (gd / gd.norm(dim=-1, keepdim=True)).t()
        want = torch.max(cos, dim=-1)[1]
    assert int((want == 1).sum()) > 50 and int((want == 3).sum()) == 0        # torch.max: the first of the two equal rows
    got = run(mod, x, go, torch.float32, True)
    ref, chain = run(mod, x, go, torch.float64, False), run(mod, x, go, torch.float32, False)
    g_gate = got[7]
    assert float(g_gate[3].abs().max()) == 0.0 and float(g_gate[1].abs().max()) > 0.0
    assert float(ref[7][3].abs().max()) == 0.0
    within_bar("tie grad gate", g_gate, chain[7], ref[7])
    within_bar("tie out", got[0], chain[0], ref[0])


def test_graph_replay_gives_the_eager_bits():
    mod, x, go, _, _ = case((3 * PANEL + 5,), 5, True, True)
    eager = run(mod, x, go, torch.float32, True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(mod, x, go, torch.float32, True)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(mod, x, go, torch.float32, True)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for name, u, v in zip(["out", "loss"] + NAMES, eager, captured):
        assert torch.equal(u, v), name


@pytest.mark.parametrize("how", ["switch", "force", "autocast", "double", "dropout", "gelu"])
def test_the_node_is_not_entered(monkeypatch, how):
    def never(*a, **k):
        raise AssertionError("the native node was entered")

    mod, x, _, _, chain = case((PANEL + 1,), 5, True, True)
    monkeypatch.setattr(zadapter._AdapterNative, "apply", never)
    if how == "switch":
        monkeypatch.setattr(transformer.Switches, "native_adapter", False)
    elif how == "force":
        monkeypatch.setattr(zadapter, "FORCE_REFERENCE", True)
    if how in ("switch", "force"):
        out, loss = mod(x)
        assert torch.equal(out, chain[0]) and torch.equal(loss, chain[1])
    elif how == "autocast":
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert mod(x)[0].shape == x.shape
    elif how == "double":
        twin = make_module(5, True, True, 5).double()
        assert twin(x.double())[0].dtype == torch.float64
    elif how == "dropout":
        twin = zadapter.Adapter(ffn_drop=0.1).to(dev()).train()
        assert twin(x)[0].shape == x.shape
        monkeypatch.undo()
        ran = recorded(monkeypatch)
        twin.eval()(x)
        assert ran == [PANEL + 1]        # eval mode: the dropout is the identity
    else:
        twin = zadapter.Adapter(activation=F.gelu).to(dev())
        assert twin(x)[0].shape == x.shape


@pytest.mark.parametrize("trainable_adapter_only", [False, True], ids=["all_trainable", "frozen_layer"])
def test_layers_against_the_reference_fixture(monkeypatch, trainable_adapter_only):
    ran = recorded(monkeypatch)
    enc = cases.check_encoder_layer("cuda", trainable_adapter_only)
    dec = cases.check_decoder_layer("cuda", trainable_adapter_only)
    assert ran == [2 * 32, 12 * 2] and enc.use_adapter and dec.use_adapter


def test_model_with_adapters_trains_one_step(monkeypatch):
    """A small model built with ``use_adapter`` and ``use_self_kd``: one step through the trainer has finite losses, ``loss_adapter``
    among them, every adapter call of the four layers goes through the native node, and every adapter parameter (started from
    seeded noise: the reference's zero ``adapter_up`` would leave the other four without a gradient) receives one and moves."""
    from ziragroundingdino_amd import backbone as zb
    from ziragroundingdino_amd import bert as zbert
    from ziragroundingdino_amd.config import zira_swint_config
    from ziragroundingdino_amd.criterion import build_criterion
    from ziragroundingdino_amd.groundingdino import GroundingDINO
    from ziragroundingdino_amd.train import ZiraTrainer, synthetic_batch
    from ziragroundingdino_amd.transformer import build_transformer

    torch.manual_seed(0)       # (tests/test_model_gpu.py's small model, with the two switches)
    args = zira_swint_config(num_queries=50, enc_layers=2, dec_layers=2, dim_feedforward=128, fusion_droppath=0.0, max_text_len=32,
                             use_adapter=True, use_self_kd=True)
    swin = zb.SwinTransformer(embed_dim=24, depths=(1, 1, 2, 1), num_heads=(1, 2, 4, 8), window_size=7, drop_path_rate=0.0,
                              out_indices=(1, 2, 3))
    bb = zb.Joiner(swin, zb.PositionEmbeddingSineHW(128, 20, 20, normalize=True))
    bb.num_channels = swin.num_features[1:]
    tiny_bert = zbert.BertModel(zbert.BertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                                                 hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
    model = GroundingDINO(bb, build_transformer(args), num_queries=50, aux_loss=True, iter_update=True, query_dim=4,
                          num_feature_levels=4, nheads=8, two_stage_type="standard", two_stage_bbox_embed_share=False,
                          two_stage_class_embed_share=False, max_text_len=32, criterion=build_criterion(args), freeze_all=True,
                          use_cet=True, use_project_adapter=True, device="cuda", bert=tiny_bert, select_box_nums_for_evaluation=20,
                          use_adapter=True, use_self_kd=True).to("cuda")
    adapters = {n: p for n, p in model.named_parameters() if ".adapter." in n}
    assert len(adapters) == 4 * 5
    with torch.no_grad():
        for p in adapters.values():
            p.copy_(torch.randn_like(p) * 0.05)
    model.train()
    model.before_train()
    assert all(p.requires_grad for p in adapters.values())
    ran = recorded(monkeypatch)
    data = synthetic_batch(2, 224, 320, n_categories=4, boxes_per_image=3, device="cuda")
    losses = model(data)
    assert len(ran) == 4 and "loss_adapter" in losses and all(torch.isfinite(v).all() for v in losses.values())
    sum(v.sum() for v in losses.values()).backward()
    for n, p in adapters.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0, n
    before = {n: p.detach().clone() for n, p in adapters.items()}
    trainer = ZiraTrainer(model)
    assert set(adapters) <= set(trainer.names)
    out = trainer.run_step(data)
    assert all(torch.isfinite(v).all() for v in out.values())
    assert all(not torch.equal(p.detach(), before[n]) for n, p in adapters.items())
