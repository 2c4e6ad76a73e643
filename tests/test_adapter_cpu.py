"""The gated adapter baseline (``use_adapter``) without a GPU: the module and the two layers against the reference's own
(tests/golden/mod_adapter.pt, mod_adapter_layers.pt), the state-dict and freeze / unfreeze contracts of a model built with the
switch, and the C ABI as declared in include/zira_adapter.h."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import ROOT

import adapter_cases as cases
from test_modules_golden import load, msda_backend  # noqa: F401  (the fixture: the MSDA entry points served by the oracle)

from ziragroundingdino_amd import _lib
from ziragroundingdino_amd import adapter as zadapter
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd import transformer
from ziragroundingdino_amd.config import zira_swint_config
from ziragroundingdino_amd.groundingdino import build_model

ENTRIES = ["zira_adapter_workspace_floats", "zira_adapter_fwd_f32", "zira_adapter_bwd_f32"]


@pytest.mark.parametrize("name", ["gate1_kd1", "gate1_kd0", "gate0_kd1", "gate0_kd0"])
def test_adapter_against_the_reference(name):
    out = cases.check_adapter_entry(load("adapter"), name, "cpu")
    assert "AdapterNative" not in type(out.grad_fn).__name__


def test_adapter_takes_any_leading_shape():
    torch.manual_seed(2)
    mod = zadapter.Adapter()
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn_like(p) * 0.1)
    x = torch.randn(7, 3, 256)
    out, loss = mod(x)
    flat, loss_flat = mod(x.reshape(-1, 256))
    four, _ = mod(x.reshape(7, 3, 1, 256))
    assert torch.equal(out.reshape(-1, 256), flat) and torch.equal(four.reshape(-1, 256), flat) and torch.equal(loss, loss_flat)
    assert loss.shape == (1,) and float(loss) == float(x.abs().mean())
    mod.use_self_kd = False
    assert float(mod(x)[1]) == 0.0


@pytest.mark.parametrize("msda_backend", ["cpu"], indirect=True)
def test_encoder_layer_with_adapter(msda_backend):
    cases.check_encoder_layer("cpu")


@pytest.mark.parametrize("msda_backend", ["cpu"], indirect=True)
def test_decoder_layer_with_adapter(msda_backend):
    cases.check_decoder_layer("cpu")


def test_layers_without_the_switch_are_the_parent_s():
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as fh:
        want = json.load(fh)["transformer"]
    enc, dec = transformer.DeformableTransformerEncoderLayer(), transformer.DeformableTransformerDecoderLayer(use_text_cross_attention=True)
    assert not hasattr(enc, "adapter") and not hasattr(dec, "adapter")
    assert sorted(enc.state_dict()) == sorted(k[len("encoder.layers.0."):] for k in want if k.startswith("encoder.layers.0."))
    assert sorted(dec.state_dict()) == sorted(k[len("decoder.layers.0."):] for k in want if k.startswith("decoder.layers.0."))
    model = build_model(zira_swint_config(device="cpu"))
    assert not any(".adapter." in k for k in model.state_dict())
    mine = sorted(k[len("transformer."):] for k in model.state_dict() if k.startswith("transformer."))
    assert mine == sorted(want)


def test_model_with_adapter_trains_the_side_branches_and_the_adapters():
    model = build_model(zira_swint_config(device="cpu", use_adapter=True, use_self_kd=True))
    plain = build_model(zira_swint_config(device="cpu"))
    plain.before_train()
    model.before_train()
    side = {n for n, p in plain.named_parameters() if p.requires_grad}
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    adapters = {n for n in trainable if ".adapter." in n}
    assert trainable - adapters == side
    names = ["adapter_down.weight", "adapter_down.bias", "adapter_up.weight", "adapter_up.bias", "gate.weight"]
    assert adapters == {"transformer.%s.layers.%d.adapter.%s" % (part, i, n) for part in ("encoder", "decoder") for i in range(6)
                        for n in names}
    assert {n for n, _ in model.named_parameters() if ".adapter." in n} == adapters
    assert set(model.side_branch_parameters()) == {p for n, p in model.named_parameters() if n in trainable}
    layer = model.transformer.encoder.layers[0]
    assert (layer.adapter.gate_base_scale, layer.adapter.use_gate, layer.adapter.use_self_kd) == (0.1, True, True)
    assert model.transformer.decoder.layers[5].adapter.adapter_down.weight.shape == (64, 256)
    model = build_model(zira_swint_config(device="cpu", use_adapter=True, use_self_kd=True, decoder_gate_base_scale=0.3))
    assert model.transformer.decoder.layers[0].adapter.gate_base_scale == 0.3
    assert model.transformer.encoder.layers[0].adapter.gate_base_scale == 0.1


@pytest.mark.parametrize("use_adapter, use_self_kd", [(True, True), (True, False), (False, True), (False, False)])
def test_loss_adapter_only_with_both_switches(monkeypatch, use_adapter, use_self_kd):
    """forward_features behind a stubbed transformer and criterion: the loss dict has ``loss_adapter`` = the transformer's adapter
    loss times ``loss_adapter_weight`` exactly when both switches are on, and is otherwise what it was."""
    from ziragroundingdino_amd import groundingdino as gd

    model = build_model(zira_swint_config(device="cpu", use_adapter=use_adapter, use_self_kd=use_self_kd, enc_layers=1, dec_layers=1))
    model.train()
    B, Q, d = 1, model.num_queries, model.hidden_dim
    adapter_loss = torch.tensor([0.25])

    def fake_transformer(srcs, masks, *a, **k):
        hs = [torch.zeros(B, Q, d)]
        ref = [torch.full((B, Q, 4), 0.5)] * 2
        return hs, ref, torch.zeros(1, B, Q, d), torch.full((1, B, Q, 4), 0.5), None, adapter_loss

    class Losses(dict):
        pass

    monkeypatch.setattr(model.transformer, "forward", fake_transformer)
    class Criterion(torch.nn.Module):
        weight_dict = {"loss_class": 2.0}

        def forward(self, out, targets):
            return Losses(loss_class=torch.ones(()))

    model.criterion = Criterion()
    monkeypatch.setattr(gd, "recover_to_cls_logits", lambda logits, *a, **k: logits)
    feats = [gd.NestedTensor(torch.zeros(B, c, 4, 4), torch.zeros(B, 4, 4, dtype=torch.bool)) for c in (192, 384, 768)]
    text_dict = {"encoded_text": torch.zeros(B, 3, d), "text_token_mask": torch.ones(B, 3, dtype=torch.bool)}
    losses = model.forward_features(feats, [torch.zeros(B, d, 4, 4)] * 3, torch.zeros(B, 16, 16, dtype=torch.bool), text_dict, None,
                                    loss_linear_adapter=torch.zeros(1), targets=[{}])
    assert ("loss_adapter" in losses) == (use_adapter and use_self_kd)
    if use_adapter and use_self_kd:
        assert torch.equal(losses["loss_adapter"], adapter_loss * model.loss_adapter_weight)
    assert set(losses) - {"loss_adapter"} == {"loss_class", "loss_conv_adapter", "loss_linear_adapter"}


def test_entry_points_are_declared_typed_and_exported():
    text = open(os.path.join(ROOT, "include", "zira_adapter.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(zira_[a-z0-9_]+)\s*\(", text)
    assert declared == ENTRIES == list(_lib.ADAPTER_SYMBOLS) == list(_lib.ADAPTER_PROTOTYPES)
    assert os.path.join(ROOT, "include", "zira_adapter.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "adapter.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    zbuild.build_extension()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ENTRIES:
        assert hasattr(raw, sym), "libzira_msda.so does not export %s" % sym
    vp, i, f32, sz, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_longlong
    P = _lib.ADAPTER_PROTOTYPES
    assert P["zira_adapter_workspace_floats"] == (sz, [ll, i, i])
    assert P["zira_adapter_fwd_f32"] == (i, [vp] * 6 + [ll, i, f32, f32, i] + [vp] * 9 + [vp])
    assert P["zira_adapter_bwd_f32"] == (i, [vp] * 12 + [ll, i, f32, f32, i] + [vp] * 7 + [vp])
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert not set(ENTRIES) & set(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 100        # zira_msda.h's own surface is what it was


def test_host_side_answers():
    lib = _lib.load()
    for M in (1, 128, 1800, 44446, 1 << 22):
        assert lib.zira_adapter_workspace_floats(M, 256, 64) > 2 * 64 * M
    for bad in ((1800, 128, 64), (1800, 255, 64), (1800, 256, 32), (0, 256, 64), (-3, 256, 64), ((1 << 22) + 1, 256, 64)):
        assert lib.zira_adapter_workspace_floats(*bad) == 0, bad
    # declined arguments are reported and nothing is launched
    assert lib.zira_adapter_fwd_f32(*([None] * 6 + [4, 5, 2.0, 0.5, 1] + [None] * 10)) == -1
    assert lib.zira_adapter_bwd_f32(*([None] * 12 + [4, 9, 2.0, 0.5, 1] + [None] * 8)) == -1


def test_cpu_tensors_and_declined_shapes_take_the_reference(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the native node was entered")

    monkeypatch.setattr(zadapter._AdapterNative, "apply", never)
    assert transformer.Switches.native_adapter is True and zadapter.FORCE_REFERENCE is False
    for kw, x in ((dict(), torch.randn(3, 256)), (dict(embed_dim=128), torch.randn(3, 128)), (dict(down_dim=32), torch.randn(3, 256)),
                  (dict(num_gate_embed=9), torch.randn(3, 256))):
        out, loss = zadapter.Adapter(**kw)(x)
        assert out.shape == x.shape and loss.shape == (1,)
    assert not zadapter.native_supported(torch.randn(3, 256), torch.zeros(64, 256), torch.zeros(256, 64), None)
