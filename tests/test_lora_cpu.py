"""The low-rank language side branch (``rsb.RepZeroLoRA``, ``text_branch="lora"``) without a GPU: the module against the
reference's own class (tests/golden/mod_rep_zero_lora.pt, at the bar of ``mod_rep_zero_linear.pt``'s test: 1e-4 of the tensor
scale, 1e-6 for the merged state), its keys and shapes, the merge identity at an O(1) state against float64, the model switch
(keys, the loss dict, ``after_train``, a checkpoint round trip, the combinations that raise), a default-built model without a
trace of it, and the header, the build and the binding."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import prompt_cases as cases
import prompt_memory_cases as mcases
from test_modules_golden import TOL, close

from ziragroundingdino_amd import _lib, rsb, transformer
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd.config import zira_swint_config
from ziragroundingdino_amd.groundingdino import build_model

LORA_KEYS = ["scaling", "freeze_linear.weight", "down.weight", "up.weight"]


def golden():
    return torch.load(os.path.join(GOLDEN, "mod_rep_zero_lora.pt"), weights_only=True)


def fixture_module(g, state="state"):
    mod = rsb.RepZeroLoRA(g["dims"][0], g["dims"][2], down_dim=g["dims"][1])
    mod.load_state_dict(g[state])       # strict
    return mod


def test_construction_state_keys_and_shapes():
    g = golden()
    mod = rsb.RepZeroLoRA(*[g["dims"][i] for i in (0, 2)], down_dim=g["dims"][1])
    state = mod.state_dict()
    assert [[k, list(v.shape)] for k, v in state.items()] == g["keys"] and list(state) == LORA_KEYS
    for k, v in g["init_state"].items():
        assert torch.equal(state[k], v), k
    assert float(mod.scaling.detach()) == pytest.approx(0.1) and bool((mod.down.weight == 1e-8).all()) and bool((mod.up.weight == 1e-8).all())
    assert not bool(mod.freeze_linear.weight.any())
    assert rsb.RepZeroLoRA(768, 256).down.weight.shape == (192, 768)       # down_dim defaults to in_features // 4
    with pytest.raises(ValueError, match="no biases"):
        rsb.RepZeroLoRA(64, 256, bias=True)


def test_train_eval_gradients_and_merge_match_the_fixture():
    g = golden()
    mod = fixture_module(g).train()
    x = g["x"].clone().requires_grad_(True)
    out, zl = mod(x)
    close(out, g["out"], TOL, "out")
    close(zl, g["zl"], TOL, "zero-interference loss")
    assert zl.dim() == 0
    params = dict(mod.named_parameters())
    assert list(params) == LORA_KEYS
    grads = torch.autograd.grad((out * g["grad_out"]).sum() + g["zl_weight"] * zl, [x] + list(params.values()))
    close(grads[0], g["grad_x"], TOL, "grad_x")
    for k, gr in zip(params, grads[1:]):
        close(gr, g["grad_params"][k], TOL, "grad " + k)
    # the definition and the entry point on CPU tensors are the module's forward
    again, zl2 = rsb.lora_reference(x, mod.down.weight, mod.up.weight, mod.freeze_linear.weight, mod.scaling)
    assert torch.equal(again, out) and torch.equal(zl2, zl)
    again, zl2 = rsb.lora_apply(x, mod.down.weight, mod.up.weight, mod.freeze_linear.weight, mod.scaling)
    assert torch.equal(again, out) and torch.equal(zl2, zl)
    mod.eval()
    out_e, zl_e = mod(x)
    close(out_e, g["out_eval"], TOL, "eval out")
    assert zl_e.shape == (1,) and float(zl_e) == 0.0
    mod.__rep__()
    assert list(mod.state_dict()) == LORA_KEYS and mod.scaling.requires_grad
    for k, v in mod.state_dict().items():
        close(v, g["state_after_rep"][k], 1e-6, "after __rep__ " + k)
    assert float(mod.scaling.detach()) == pytest.approx(0.1) and bool((mod.down.weight == 1e-8).all()) and bool((mod.up.weight == 1e-8).all())


def test_the_merge_keeps_the_output_at_an_o1_state():
    """``eval()(x)`` after ``__rep__`` is the train-mode ``out`` before it.  Expected value: the train-mode expression in float64
    on the fp32 values.  Bound: both fp32 evaluations are sums of at most n = E + R + 4 rounded terms a element (the merged
    weight adds R products and two operations, the products with x another E), so each is within gamma_n * (|x| (|W_t| + |s|
    |W_u| |W_d|)^T) of it, gamma_n = n eps / (1 - n eps): the standard forward bound of an inner product, taken at its largest
    element."""
    g = golden()
    mod = fixture_module(g).train()
    x = g["x"]
    wd, wu, wt, s = (t.detach().double() for t in (mod.down.weight, mod.up.weight, mod.freeze_linear.weight, mod.scaling))
    exact = s * (x.double() @ wd.T @ wu.T) + x.double() @ wt.T
    n, eps = g["dims"][0] + g["dims"][1] + 4, float(np.finfo(np.float32).eps)
    bound = n * eps / (1 - n * eps) * float((x.double().abs() @ (wt.abs() + s.abs() * (wu.abs() @ wd.abs())).T).max())
    before = mod(x)[0].detach()
    mod.__rep__()
    after = mod.eval()(x)[0].detach()
    err_b, err_a = float((before.double() - exact).abs().max()), float((after.double() - exact).abs().max())
    print("train before the merge %.3e, eval after it %.3e, bound %.3e (max|out| %.3e)" % (err_b, err_a, bound, float(exact.abs().max())))
    assert float(exact.abs().max()) > 1.0 and err_b <= bound and err_a <= bound
    # and the train-mode forward after the merge adds a branch at the 1e-8 initialisation: nothing a float sees here
    assert float((mod.train()(x)[0].detach() - after).abs().max()) <= bound


def lora_model(**kw):
    return mcases.small_model("cpu", use_prompt_memory=False, text_branch="lora", **kw)


def test_the_model_switch_builds_the_module_and_its_loss_enters_the_dict():
    model = lora_model()
    assert model.text_branch == "lora" and isinstance(model.rep_linear_adapter, rsb.RepZeroLoRA)
    assert model.rep_linear_adapter.down.weight.shape == (16, 64) and model.rep_linear_adapter.up.weight.shape == (256, 16)
    assert [k for k in model.state_dict() if k.startswith("rep_linear_adapter.")] == ["rep_linear_adapter." + k for k in LORA_KEYS]
    assert lora_model(lora_down_dim=32).rep_linear_adapter.down.weight.shape == (32, 64)
    assert model.replay_parameter_prefixes()[0] == "rep_linear_adapter." and model._text_loss_name() == "loss_linear_adapter"
    model.before_train()
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert all("rep_linear_adapter." + k in trainable for k in LORA_KEYS)
    with torch.no_grad():       # an O(1) branch, so the term is far from the 1e-32 of the initialisation
        model.rep_linear_adapter.down.weight.normal_(0, 0.2, generator=torch.Generator().manual_seed(5))
        model.rep_linear_adapter.up.weight.normal_(0, 0.2, generator=torch.Generator().manual_seed(6))
    model.train()
    data = cases.batch([["cat", "owl"], ["polar bear", "cat"]])
    loss_dict = model(data)
    assert "loss_linear_adapter" in loss_dict and "loss_adapter_text" not in loss_dict
    captions, names_list = model._captions(data)
    _, _, zero = model.encode_text(captions, "cpu", names_list=names_list)
    assert float(zero.detach()) > 1e-4
    assert torch.equal(loss_dict["loss_linear_adapter"].detach(), (zero * model.loss_adapter_weight).detach())
    torch.testing.assert_close(loss_dict.total.reshape(()), sum(v.reshape(()) for v in loss_dict.values()), rtol=1e-5, atol=1e-6)


def test_after_train_merges_and_the_checkpoint_loads_again():
    model = lora_model()
    branch = model.rep_linear_adapter
    with torch.no_grad():
        branch.down.weight.normal_(0, 0.2, generator=torch.Generator().manual_seed(7))
        branch.up.weight.normal_(0, 0.2, generator=torch.Generator().manual_seed(8))
        branch.freeze_linear.weight.normal_(0, 0.05, generator=torch.Generator().manual_seed(9))
        branch.scaling.fill_(0.3)
    merged = (branch.up.weight @ branch.down.weight) * branch.scaling + branch.freeze_linear.weight
    model.after_train()
    assert model.rep_linear_adapter is branch and torch.equal(branch.freeze_linear.weight, merged.detach())
    assert float(branch.scaling.detach()) == pytest.approx(0.1) and bool((branch.down.weight == 1e-8).all()) and bool((branch.up.weight == 1e-8).all())
    state = model.state_dict()
    fresh = lora_model()
    assert not bool(fresh.rep_linear_adapter.freeze_linear.weight.any())
    fresh.load_state_dict(state)       # strict
    assert torch.equal(fresh.rep_linear_adapter.freeze_linear.weight, merged.detach())
    with pytest.raises(RuntimeError, match="rep_linear_adapter"):       # and the dense branch's model refuses it
        mcases.small_model("cpu", use_prompt_memory=False).load_state_dict(state)


def test_the_combinations_that_raise():
    with pytest.raises(ValueError, match="multilayer"):
        mcases.small_model("cpu", use_prompt_memory=False, text_branch="lora", side_branch="multilayer")
    with pytest.raises(ValueError, match="multilayer"):
        build_model(zira_swint_config(device="cpu", modelname="dualzerorepmultilayerbranchgroundingdino", enc_layers=1, dec_layers=1,
                                      text_branch="lora"))


def test_the_builder_passes_the_switch_and_a_default_model_has_no_trace_of_it():
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as fh:
        ref = json.load(fh)
    model = build_model(zira_swint_config(device="cpu", enc_layers=1, dec_layers=1))
    under = {k[len("rep_linear_adapter."):]: list(v.shape) for k, v in model.state_dict().items() if k.startswith("rep_linear_adapter.")}
    assert model.text_branch == "rep" and under == ref["rep_zero_linear_768_256"] and type(model.rep_linear_adapter) is rsb.RepZeroLinear
    assert not any(k.endswith(("down.weight", "up.weight")) and "rep_linear" in k for k in model.state_dict())
    lora = build_model(zira_swint_config(device="cpu", enc_layers=1, dec_layers=1, text_branch="lora", lora_down_dim=64))
    assert isinstance(lora.rep_linear_adapter, rsb.RepZeroLoRA) and lora.rep_linear_adapter.down.weight.shape == (64, 768)
    assert build_model(zira_swint_config(device="cpu", enc_layers=1, dec_layers=1,
                                         text_branch="lora")).rep_linear_adapter.down.weight.shape == (192, 768)
    assert [k for k in lora.state_dict() if k not in model.state_dict()] == ["rep_linear_adapter.down.weight", "rep_linear_adapter.up.weight"]


def test_header_build_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "zira_lora.h")).read()
    declared = re.findall(r"\b(zira_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert declared == list(_lib.LORA_SYMBOLS) == ["zira_lora_supported", "zira_lora_splits", "zira_lora_ticket_words",
                                                   "zira_lora_fwd_workspace_floats", "zira_lora_bwd_workspace_floats",
                                                   "zira_lora_fwd_f32", "zira_lora_bwd_f32"]
    assert os.path.join(ROOT, "include", "zira_lora.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert any(os.path.basename(s) == "lora.hip" for s in zbuild.SOURCES)
    vp, i, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    assert _lib.LORA_PROTOTYPES["zira_lora_fwd_f32"] == (i, [vp] * 5 + [ll, i, i] + [vp] * 6)
    assert _lib.LORA_PROTOTYPES["zira_lora_bwd_f32"] == (i, [vp] * 9 + [ll, i, i] + [vp] * 10)
    assert _lib.LORA_PROTOTYPES["zira_lora_fwd_workspace_floats"] == (sz, [ll, i, i])
    assert _lib.LORA_CONSTANTS == {"ZIRA_LORA_MAX_E": 1024, "ZIRA_LORA_MAX_R": 256, "ZIRA_LORA_OUT": 256, "ZIRA_LORA_MAX_ROWS": 16384}
    assert transformer.Switches.native_lora in (True, False) and rsb.FORCE_LORA_REFERENCE is False
    zbuild.build_extension()
    exported = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(exported, s) for s in _lib.LORA_SYMBOLS)
    lib = _lib.load()
    for ok in ((1, 32, 32), (390, 768, 192), (64 * 256, 1024, 256)):
        assert lib.zira_lora_supported(*ok) == 1, ok
    for bad in ((0, 768, 192), (64 * 256 + 1, 768, 192), (390, 48, 32), (390, 1056, 192), (390, 768, 16), (390, 768, 288)):
        assert lib.zira_lora_supported(*bad) == 0, bad
        assert lib.zira_lora_fwd_workspace_floats(*bad) == 0 and lib.zira_lora_bwd_workspace_floats(*bad) == 0, bad
    # the deal, as the header states it: 24 panels at 768; the row tiles of M = 390 leave room for 19 waves each, so a wave
    # takes two panels and twelve waves share a tile
    assert [lib.zira_lora_splits(m, 768) for m in (1, 33, 82, 390, 4096, 64 * 256)] == [24, 24, 24, 12, 2, 1]
    assert lib.zira_lora_splits(390, 64) == 2 and lib.zira_lora_splits(390, 32) == 1 and lib.zira_lora_splits(390, 1056) == 0
    assert lib.zira_lora_ticket_words(390) == 16 and lib.zira_lora_ticket_words(0) == 0
    assert lib.zira_lora_fwd_workspace_floats(64 * 256, 768, 192) == 4 * 512
    assert lib.zira_lora_fwd_workspace_floats(390, 768, 192) == 52 + 12 * 13 * 32 * (192 + 256)
    # argument errors are reported, never thrown, and nothing is launched
    assert lib.zira_lora_fwd_f32(*([None] * 5), 390, 768, 192, *([None] * 6)) == -1
    assert lib.zira_lora_bwd_f32(*([None] * 9), 390, 768, 192, *([None] * 10)) == -1
