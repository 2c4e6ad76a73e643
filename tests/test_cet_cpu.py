"""The CET text-adapter baseline (``dtgroundingdino``, ``text_branch="cet"``) without a GPU: the registry builds it, the module's
keys and initialisation are the reference's, ``cet_reference`` and the model's ``project_text`` equal the reference's sibling
class (tests/golden/mod_cet.pt, both ``cet_type``s: the encoded text bit for bit; the loss and the gradients, sums whose order is
the machine's, to the project's bar against float64), the loss types, ``use_gate=False`` and the eval skip, the loss
dict's and the replay's ``loss_adapter_text``, what ``before_train`` leaves trainable, a default-built model without a trace of
it, and the header, the build and the binding."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import prompt_cases as cases
import prompt_memory_cases as mcases

from ziragroundingdino_amd import _lib, cet, transformer
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd.config import zira_swint_config
from ziragroundingdino_amd.groundingdino import MODULE_BUILD_FUNCS, build_model

TYPES = ["Adapter", "Linear"]


def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "mod_cet.pt"), weights_only=True)


def golden_model(g, cet_type, **kw):
    """the small model with the fixture's text side: the grid-valued encoder stand-in, the fixture's feat_map and adapter"""
    kw.setdefault("use_prompt_memory", False)
    model = mcases.small_model("cpu", text_branch="cet", cet_type=cet_type, cet_middle_dim=g["cet_middle_dim"], **kw)
    model.bert = cases.GridBert()
    model.feat_map.load_state_dict(g[cet_type]["feat_map"])
    model.cet_adapter.load_state_dict(g[cet_type]["state"])
    return model


def bar_holds(got, fixture, exact):
    """The project's bar for a value whose sum order differs between machines: the error of ``got`` against the float64
    evaluation is at most twice the fixture's, plus one fp32 ulp of the largest magnitude.  -> (holds, error, bound)"""
    got, fixture, exact = (t.detach().double().reshape(-1) for t in (got, fixture, exact))
    top = float(exact.abs().max())
    ulp = float(np.spacing(np.float32(top))) if top != 0.0 else float(np.finfo(np.float32).tiny)
    err, bound = float((got - exact).abs().max()), 2.0 * float((fixture - exact).abs().max()) + ulp
    return err <= bound, err, bound


def fp64_oracle(model, hidden, feat, upstream, loss_type="L1"):
    """(loss, gradients by parameter name) of the definition in float64 on the same fp32 values"""
    twin = cet.build_cet_adapter(model.cet_type, hidden.shape[-1], 32, 256).double()
    twin.load_state_dict({k: v.double() for k, v in model.cet_adapter.state_dict().items()})
    enc, loss = cet.cet_reference(hidden.double(), feat.double(), twin, loss_type, True)
    params = dict(twin.named_parameters())
    grads = torch.autograd.grad((enc * upstream.double()).sum() + loss.sum(), list(params.values()))
    return loss.detach(), dict(zip(params, grads))


def text_side(model, g, names=False):
    captions = list(g["captions"])
    kw = {"names_list": [c[:-1].split(".") for c in captions]} if names else {}
    text_dict, _, loss = model.encode_text(captions, "cpu", **kw)
    return text_dict, loss


def test_the_registry_builds_dtgroundingdino():
    assert "dtgroundingdino" in MODULE_BUILD_FUNCS
    model = build_model(zira_swint_config(device="cpu", modelname="dtgroundingdino", enc_layers=1, dec_layers=1))
    assert model.text_branch == "cet" and isinstance(model.cet_adapter, cet.CETAdapter)
    assert model.cet_adapter.adapter_down.weight.shape == (1024, 768) and model.cet_adapter.adapter_up.weight.shape == (256, 1024)
    assert model.cet_adapter.gate.weight.shape == (5, 768) and model.cet_adapter.gate_base_scale == 1.0
    keys = list(model.state_dict())
    assert not any(k.startswith(("rep_linear_adapter.", "input_proj_conv_adapter.")) for k in keys)
    assert [k for k in keys if k.startswith("cet_adapter.")] == ["cet_adapter." + k for k in (
        "adapter_down.weight", "adapter_down.bias", "adapter_up.weight", "adapter_up.bias", "gate.weight")]
    assert model.replay_parameter_prefixes()[0] == "cet_adapter."
    linear = build_model(zira_swint_config(device="cpu", modelname="dtgroundingdino", enc_layers=1, dec_layers=1, cet_type="Linear"))
    assert isinstance(linear.cet_adapter, cet.LinearCETAdapter)
    with pytest.raises(NotImplementedError, match="Transformer"):
        build_model(zira_swint_config(device="cpu", modelname="dtgroundingdino", enc_layers=1, dec_layers=1, cet_type="Transformer"))
    with pytest.raises(NotImplementedError, match="Huber"):
        mcases.small_model("cpu", text_branch="cet", zero_loss_type="Huber")


@pytest.mark.parametrize("cet_type", TYPES)
def test_keys_and_initialisation_match_the_fixture(cet_type):
    g = golden()[cet_type]
    torch.manual_seed(3)
    mod = cet.build_cet_adapter(cet_type, 64, 32, 256)
    state = mod.state_dict()
    assert list(state) == list(g["init_state"]) and all(state[k].shape == v.shape for k, v in g["init_state"].items())
    for k, v in g["init_state"].items():
        if k.startswith(("adapter_up.", "linear.")) or k == "adapter_down.bias":
            assert not bool(v.any()) and not bool(state[k].any()), k
    if cet_type == "Adapter":       # kaiming-uniform with a = sqrt(5): bound 1 / sqrt(fan_in), and both fill it
        bound = 1.0 / math.sqrt(64)
        for w in (state["adapter_down.weight"], g["init_state"]["adapter_down.weight"]):
            assert 0.9 * bound < float(w.abs().max()) <= bound
    for w in (state["gate.weight"], g["init_state"]["gate.weight"]):        # nn.Embedding: standard normal
        assert 0.8 < float(w.std()) < 1.2
    fresh = cet.build_cet_adapter(cet_type, 64, 32, 256)
    fresh.load_state_dict(g["state"])       # strict


@pytest.mark.parametrize("cet_type", TYPES)
def test_reference_and_project_text_equal_the_fixture(cet_type):
    full, g = golden(), golden()[cet_type]
    model = golden_model(full, cet_type).train()
    assert transformer.Switches.native_cet in (True, False) and cet.FORCE_REFERENCE is False
    text_dict, model_loss = text_side(model, full)
    assert torch.equal(text_dict["encoded_text"], g["encoded_text"])
    # the definition itself, on the encoder's states
    hidden = model.bert(input_ids=model._encoder_inputs(list(full["captions"]), "cpu")[0]["input_ids"])["last_hidden_state"]
    feat = model.feat_map(hidden).detach()
    enc, loss = cet.cet_reference(hidden, feat, model.cet_adapter, "L1", True)
    assert torch.equal(enc.detach(), g["encoded_text"]) and torch.equal(loss.detach(), model_loss.detach())
    assert torch.equal((enc.detach() - feat), (feat + g["adapter_output"]) - feat)
    # the loss and the gradients are sums of rounded numbers, whose order is the machine's: the project's bar against float64
    exact_loss, exact_grads = fp64_oracle(model, hidden, feat, g["upstream"])
    ok, err, bound = bar_holds(loss, g["losses"]["L1"], exact_loss)
    print("%s loss %.9g fixture %.9g error %.3g bound %.3g" % (cet_type, float(loss), float(g["losses"]["L1"]), err, bound))
    assert ok
    params = dict(model.cet_adapter.named_parameters())
    grads = torch.autograd.grad((enc * g["upstream"]).sum() + loss.sum(), list(params.values()))
    for (k, _), got in zip(params.items(), grads):
        ok, err, bound = bar_holds(got, g["grads"][k], exact_grads[k])
        print("%s grad %s error %.3g bound %.3g" % (cet_type, k, err, bound))
        assert ok, k
    # cet_apply on CPU tensors is the definition
    again, _ = cet.cet_apply(hidden, feat, model.cet_adapter, "L1", True)
    assert torch.equal(again.detach(), enc.detach())


def test_loss_types_no_gate_and_no_zero_loss():
    full, g = golden(), golden()["Adapter"]
    model = golden_model(full, "Adapter").train()
    hidden = model.bert(input_ids=model._encoder_inputs(list(full["captions"]), "cpu")[0]["input_ids"])["last_hidden_state"]
    feat = model.feat_map(hidden).detach()
    for name in ("L1", "L2", "Smooth_L1"):
        enc, loss = cet.cet_reference(hidden, feat, model.cet_adapter, name, True)
        ok, err, bound = bar_holds(loss, g["losses"][name], fp64_oracle(model, hidden, feat, g["upstream"], name)[0])
        print("%s %.9g fixture %.9g error %.3g bound %.3g" % (name, float(loss), float(g["losses"][name]), err, bound))
        assert ok and tuple(loss.shape) == (1,), name
        assert torch.equal(enc.detach(), g["encoded_text"])
        typed = golden_model(full, "Adapter", zero_loss_type=name).train()
        assert torch.equal(text_side(typed, full)[1].detach(), loss.detach()), name
    enc, loss = cet.cet_reference(hidden, feat, model.cet_adapter, "L1", False)
    assert float(loss) == 0.0 and tuple(loss.shape) == (1,) and torch.equal(enc.detach(), g["encoded_text"])
    with pytest.raises(NotImplementedError, match="Huber"):
        cet.cet_reference(hidden, feat, model.cet_adapter, "Huber", True)
    # use_gate = False: the constant scale (1.0 here), so the output is the bare bottleneck
    mod = model.cet_adapter
    mod.use_gate = False
    enc, _ = cet.cet_reference(hidden, feat, mod, "L1", True)
    bare = mod.adapter_up(torch.relu(mod.adapter_down(hidden)))
    assert torch.equal(enc.detach(), (feat + bare * 1.0).detach()) and not torch.equal(enc.detach(), g["encoded_text"])
    # an all-zero row: NaN, as the reference's x / x.norm gives it
    mod.use_gate = True
    zeroed = hidden.clone()
    zeroed[0, 3] = 0.0
    enc, loss = cet.cet_reference(zeroed, feat, mod, "L1", True)
    assert bool(torch.isnan(enc[0, 3]).all()) and not bool(torch.isnan(enc[0, 2]).any()) and bool(torch.isnan(loss).all())


@pytest.mark.parametrize("cet_type", TYPES)
def test_eval_skips_the_adapter_under_use_prompt_memory_output(cet_type):
    full, g = golden(), golden()[cet_type]
    model = golden_model(full, cet_type, use_prompt_memory_output=True).eval()
    ran = []
    model.cet_adapter.register_forward_hook(lambda *a: ran.append(1))
    with torch.no_grad():
        text_dict, loss = text_side(model, full)
    assert not ran and loss is None and torch.equal(text_dict["encoded_text"], g["eval_memory_output"])
    model.use_prompt_memory_output = False
    with torch.no_grad():
        text_dict, loss = text_side(model, full)
    assert ran == [1] and torch.equal(text_dict["encoded_text"], g["eval_no_memory_output"])
    model.train()
    assert torch.equal(text_side(model, full)[0]["encoded_text"].detach(), g["encoded_text"])


def test_loss_adapter_text_in_the_loss_dict_and_in_the_replay():
    full = golden()
    model = golden_model(full, "Adapter", use_prompt_memory=True).train()
    _, zero = text_side(model, full, names=True)
    loss_dict = model(cases.batch([["cat", "owl"], ["polar bear", "cat"]]))
    assert "loss_adapter_text" in loss_dict and "loss_linear_adapter" not in loss_dict and "loss_prompt_memory" in loss_dict
    data = cases.batch([["cat", "owl"], ["polar bear", "cat"]])
    captions, names_list = model._captions(data)
    _, _, zero = model.encode_text(captions, "cpu", names_list=names_list)
    assert model.loss_adapter_weight == 0.1 and float(zero.detach()) > 0
    assert torch.equal(loss_dict["loss_adapter_text"].detach(), (zero * model.loss_adapter_weight).detach())
    torch.testing.assert_close(loss_dict.total.reshape(()), sum(v.reshape(()) for v in loss_dict.values()), rtol=1e-5, atol=1e-6)
    # the replay: the pool entries are taken with the adapter as it stands, then moved
    model.add_cls_prompt(["cat", "polar bear"])
    with torch.no_grad():
        for p in model.prompt_memory_pool.values():
            p.add_(0.25)
    losses = model.replay_memory()
    assert list(losses) == ["loss_prompt_memory", "loss_adapter_text"] and float(losses["loss_prompt_memory"].detach()) > 0
    _, _, zero = model.encode_text(["cat.polar bear."], "cpu")
    assert torch.equal(losses["loss_adapter_text"].detach(), (zero.reshape(()) * 0.1).detach())
    losses["loss_prompt_memory"].backward()
    assert model.cet_adapter.adapter_up.weight.grad is not None and float(model.cet_adapter.adapter_up.weight.grad.abs().max()) > 0
    with pytest.raises(NotImplementedError, match="L1"):
        golden_model(full, "Adapter", use_prompt_memory=True, zero_loss_type="L2")


def test_before_train_leaves_the_adapter_trainable_and_after_train_keeps_it():
    from ziragroundingdino_amd.train import MemoryReplayer

    full = golden()
    model = golden_model(full, "Adapter", use_project_adapter=False, use_prompt_memory=True)
    model.before_train()
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert trainable == [n for n, _ in model.named_parameters() if n.startswith("cet_adapter.")] and len(trainable) == 5
    before = {k: v.clone() for k, v in model.state_dict().items() if k.startswith("cet_adapter.")}
    model.after_train()
    after = model.state_dict()
    assert before and all(torch.equal(after[k], v) for k, v in before.items())
    model.train()
    model.add_cls_prompt(["cat"])
    assert all(n.startswith("cet_adapter.") for n in MemoryReplayer(model).names)


def test_a_default_model_has_no_trace_of_it():
    from test_model_gpu import small_model

    present = small_model(dev="cpu")
    assert present.text_branch == "rep" and not hasattr(present, "cet_adapter")
    assert not any("cet_adapter" in k for k in present.state_dict())
    assert any(k.startswith("rep_linear_adapter.") for k in present.state_dict())
    assert present.replay_parameter_prefixes()[0] == "rep_linear_adapter." and present._text_loss_name() == "loss_linear_adapter"
    model = build_model(zira_swint_config(device="cpu", enc_layers=1, dec_layers=1))
    assert not any("cet_adapter" in k for k in model.state_dict())


def test_header_build_and_binding_agree_and_the_limits_are_declined():
    text = open(os.path.join(ROOT, "include", "zira_cet.h")).read()
    declared = re.findall(r"\b(zira_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert declared == list(_lib.CET_SYMBOLS) == ["zira_cet_supported", "zira_cet_splits", "zira_cet_ticket_words",
                                                  "zira_cet_fwd_workspace_floats", "zira_cet_bwd_workspace_floats",
                                                  "zira_cet_fwd_f32", "zira_cet_bwd_f32"]
    assert os.path.join(ROOT, "include", "zira_cet.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "cet.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    vp, i, ll, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    assert _lib.CET_PROTOTYPES["zira_cet_fwd_f32"] == (i, [vp] * 7 + [ll, i, i, i, f, f, i] + [vp] * 10)
    assert _lib.CET_PROTOTYPES["zira_cet_bwd_f32"] == (i, [vp] * 12 + [ll, i, i, i, f, f, i] + [vp] * 11)
    assert (cet.MAX_E, cet.MAX_H, cet.OUT_DIM, cet.MAX_GATES, cet.MAX_ROWS) == (768, 1024, 256, 8, 64 * 256)
    lib = _lib.load()
    for ok in ((1, 32, 32, 0), (390, 768, 1024, 5), (64 * 256, 768, 1024, 8), (82, 64, 32, 1)):
        assert lib.zira_cet_supported(*ok) == 1, ok
    for bad in ((0, 768, 1024, 5), (64 * 256 + 1, 768, 1024, 5), (390, 800, 1024, 5), (390, 760, 1024, 5), (390, 768, 1056, 5),
                (390, 768, 1000, 5), (390, 768, 1024, 9), (390, 768, 1024, -1), (390, 0, 1024, 5), (390, 768, 0, 5)):
        assert lib.zira_cet_supported(*bad) == 0, bad
        assert lib.zira_cet_bwd_workspace_floats(*bad) == 0, bad
    # the split is a function of the shape alone: the row tiles times the split aim at 512 waves, a panel of 32 units at least
    assert [lib.zira_cet_splits(m, 1024) for m in (1, 33, 82, 390, 544, 64 * 256)] == [32, 32, 32, 32, 30, 1]
    assert lib.zira_cet_splits(390, 32) == 1 and lib.zira_cet_splits(390, 1056) == 0
    assert lib.zira_cet_ticket_words(390) == 16 and lib.zira_cet_ticket_words(0) == 0
    assert lib.zira_cet_fwd_workspace_floats(64 * 256, 1024) == 2 * 512
    assert lib.zira_cet_fwd_workspace_floats(390, 1024) == 28 + 32 * 13 * 32 * 256
    # null pointers: -1, and nothing is launched (no GPU here)
    assert lib.zira_cet_fwd_f32(*([None] * 7), 390, 768, 1024, 5, 2.0, 1.0, 1, *([None] * 10)) == -1
    assert lib.zira_cet_bwd_f32(*([None] * 12), 390, 768, 1024, 5, 2.0, 1.0, 1, *([None] * 11)) == -1
    # the Python side declines what the header declines, and everything that is not the gated bottleneck on the device
    mod = cet.build_cet_adapter("Adapter", 64, 32, 256)
    x, feat = torch.zeros(2, 3, 64), torch.zeros(2, 3, 256)
    assert not cet.native_supported(x, feat, mod)                                       # CPU tensors
    assert not cet.native_supported(x, feat, cet.build_cet_adapter("Linear", 64, 32, 256))
