"""The linear-probing baseline (``use_cls_linear``) without a GPU: the model builds with the switch and keeps the reference's
state-dict and freeze / unfreeze contracts (tests/golden/cls_linear_state_dict_keys.json), ``ContrastiveEmbedwithLinear`` equals
the reference's module bit for bit (tests/golden/mod_contrastive_linear.pt), ``cls_linear_logits_reference`` is the two-step
composition and has the right gradients, the switch off changes nothing, and the C ABI is as include/zira_clslinear.h declares."""
import ctypes
import json
import os
import re

import torch

from conftest import ROOT

import cls_linear_cases as cases

from ziragroundingdino_amd import _lib
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd import utils as zutils

ENTRIES = ["zira_cls_linear_workspace_floats", "zira_cls_linear_logits_fwd_f32", "zira_cls_linear_logits_bwd_f32"]


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "cls_linear_state_dict_keys.json")) as fh:
        return json.load(fh)


def outside(name):
    return name.startswith(("bert.", "backbone."))      # (the generator's stand-ins: not part of the fixture)


def test_model_builds_with_the_switch_and_keeps_the_reference_s_keys():
    ref = fixture()
    model = cases.small_model("cpu", use_cls_linear=True)
    assert isinstance(model.class_embed[0], zutils.ContrastiveEmbedwithLinear) and model.use_cls_linear
    mine = {k: list(v.shape) for k, v in model.state_dict().items() if not outside(k)}
    assert sorted(mine) == sorted(ref["state_dict"]), (sorted(set(ref["state_dict"]) - set(mine))[:10],
                                                       sorted(set(mine) - set(ref["state_dict"]))[:10])
    assert mine == ref["state_dict"]
    # the decoder layers share one module; the encoder's is a copy with weights of its own (two_stage_class_embed_share = False)
    assert all(m is model.class_embed[0] for m in model.class_embed)
    assert model.transformer.decoder.class_embed is model.class_embed
    enc = model.transformer.enc_out_class_embed
    assert isinstance(enc, zutils.ContrastiveEmbedwithLinear) and enc is not model.class_embed[0]
    assert enc.cls_linear.weight.data_ptr() != model.class_embed[0].cls_linear.weight.data_ptr()
    assert torch.equal(enc.cls_linear.weight, model.class_embed[0].cls_linear.weight)
    shared = cases.small_model("cpu", use_cls_linear=True, two_stage_class_embed_share=True, two_stage_bbox_embed_share=True)
    assert shared.transformer.enc_out_class_embed is shared.class_embed[0]


def test_before_train_leaves_what_the_reference_leaves_trainable():
    ref = fixture()
    model = cases.small_model("cpu", use_cls_linear=True)
    model.before_train()
    trainable = [n for n, p in model.named_parameters() if p.requires_grad and not outside(n)]
    assert trainable == ref["trainable"]
    assert sum("cls_linear" in n for n in trainable) == 4 and sum("bbox_embed" in n for n in trainable) == 12
    assert not any(p.requires_grad for n, p in model.named_parameters() if outside(n))
    off = cases.small_model("cpu", use_cls_linear=False)
    off.before_train()
    assert all("adapter" in n for n, p in off.named_parameters() if p.requires_grad)


def test_module_equals_the_reference_s_bit_for_bit():
    g = torch.load(os.path.join(ROOT, "tests", "golden", "mod_contrastive_linear.pt"), weights_only=True)
    mod = zutils.ContrastiveEmbedwithLinear(max_text_len=g["max_text_len"], hidden_dim=256)
    assert list(mod.state_dict()) == list(g["state"]) == ["cls_linear.weight", "cls_linear.bias"]
    bound = 1.0 / 256 ** 0.5                    # nn.Linear's default: kaiming_uniform_(a = sqrt(5)) on fan_in 256, bias in the same range
    assert 0.9 * bound < float(mod.cls_linear.weight.detach().abs().max()) <= bound
    assert 0.0 < float(mod.cls_linear.bias.detach().abs().max()) <= bound
    assert float(g["state"]["cls_linear.weight"].abs().max()) <= bound
    # the fixture's values sit on binary grids coarse enough that both products are exact in fp32 in any order of addition
    # (gen_cls_linear_golden.py asserts it), so the bits below do not depend on the CPU's GEMM kernels
    assert all(torch.equal(v * 256, torch.round(v * 256)) for v in g["state"].values())
    assert torch.equal(g["x"] * 4, torch.round(g["x"] * 4)) and torch.equal(g["encoded_text"] * 2, torch.round(g["encoded_text"] * 2))
    mod.load_state_dict(g["state"])
    td = {"encoded_text": g["encoded_text"], "text_token_mask": g["text_token_mask"]}
    assert g["encoded_text"].shape[1] < g["max_text_len"] and not bool(g["text_token_mask"].all())        # ragged, and T < max_text_len
    with torch.no_grad():
        out = mod(g["x"], td)
    assert out.shape == g["out"].shape and torch.equal(out, g["out"])
    assert bool(torch.isneginf(out[0, :, 5:]).all()) and bool(torch.isfinite(out[1, :, :9]).all())


def head_case(dtype=torch.float32, R_shape=(2, 3), T=5, C=3, seed=3):
    """x [.., B = 2, Q, 256], text padded to T with ragged token counts, C categories in image 0 and one in image 1, one of
    image 0's without tokens"""
    gen = torch.Generator().manual_seed(seed)
    B = 2
    x = torch.randn(*R_shape[:-1], B, R_shape[-1], 256, generator=gen).to(dtype)
    w = (torch.randn(256, 256, generator=gen) / 16).to(dtype)
    b = (torch.randn(256, generator=gen) * 0.1).to(dtype)
    text = torch.randn(B, T, 256, generator=gen).to(dtype)
    td = cases.text_dict(text, (T - 1, T))
    masks = cases.category_masks([[[1], [2, 3], []][:C], [[0, 1, 2, 3, 4][:T]]], (T - 1, T), "cpu")
    return x, w, b, td, masks


def test_reference_is_the_two_step_composition_bit_for_bit():
    x, w, b, td, masks = head_case()
    mod = zutils.ContrastiveEmbedwithLinear(max_text_len=16, hidden_dim=256)
    with torch.no_grad():
        mod.cls_linear.weight.copy_(w)
        mod.cls_linear.bias.copy_(b)
        for fill in (-100.0, float("-inf")):
            want = zutils.recover_to_cls_logits(mod(x, td), masks, for_fill=fill)
            got = zutils.cls_linear_logits_reference(x, w, b, td, masks, fill, 16)
            assert got.shape == x.shape[:-1] + (16,) and torch.equal(got, want)
            assert torch.equal(mod.category_logits(x, td, masks, fill), want)          # CPU tensors: the module takes the reference
        assert bool((got[..., 0, :, 2] == fill).all())                                 # the category without tokens
        assert bool((got[..., 1, :, 1:] == fill).all()) and bool(torch.isfinite(got[..., 1, :, 0]).all())


def test_reference_gradients_pass_gradcheck():
    # R = 6 rows (B = 2, Q = 3), T = 5, C = 3
    x, w, b, td, masks = head_case(torch.float64, R_shape=(3,), T=5, C=3, seed=4)
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    assert x.numel() // 256 == 6
    torch.autograd.gradcheck(lambda x_, w_, b_: zutils.cls_linear_logits_reference(x_, w_, b_, td, masks, -100.0, 8), (x, w, b),
                             eps=1e-6, atol=1e-6)
    # and for a text that requires grad
    td2 = dict(td, encoded_text=td["encoded_text"].clone().requires_grad_(True))
    out = zutils.cls_linear_logits_reference(x, w, b, td2, masks, -100.0, 8)
    (g_text,) = torch.autograd.grad(out[out > -100.0].sum(), [td2["encoded_text"]])
    assert float(g_text.abs().max()) > 0.0 and float(g_text[0, 4].abs().max()) == 0.0       # image 0's padded token


def test_the_switch_off_changes_nothing():
    from test_model_gpu import small_model
    from ziragroundingdino_amd.train import synthetic_batch

    ref = fixture()
    present, off = small_model(dev="cpu").eval(), cases.small_model("cpu", use_cls_linear=False).eval()
    assert isinstance(off.class_embed[0], zutils.ContrastiveEmbed) and not any("cls_linear" in k for k in off.state_dict())
    assert list(off.state_dict()) == list(present.state_dict())
    assert all(torch.equal(v, present.state_dict()[k]) for k, v in off.state_dict().items())
    assert sorted(k for k in off.state_dict() if not outside(k)) == sorted(k for k in ref["state_dict"] if "cls_linear" not in k)
    data = [synthetic_batch(1, 64, 96, n_categories=3, boxes_per_image=2, seed=1)[0],
            synthetic_batch(1, 80, 72, n_categories=3, boxes_per_image=2, seed=2)[0]]
    with torch.no_grad():
        a, b = present(data), off(data)
    for u, v in zip(a, b):
        u, v = u["instances"], v["instances"]
        assert torch.equal(u.scores, v.scores) and torch.equal(u.pred_boxes.tensor, v.pred_boxes.tensor)
        assert torch.equal(u.pred_classes, v.pred_classes)


def test_model_with_the_switch_runs_on_the_cpu():
    """training-mode losses through the reference path: finite, and the trained heads -- only they and the side branches --
    receive gradients"""
    from ziragroundingdino_amd.train import synthetic_batch

    model = cases.small_model("cpu", use_cls_linear=True).train()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "bbox_embed" in n and "layers.2" in n:
                p.copy_(torch.randn_like(p) * 0.05)          # (the zero-initialised last layer would starve the two before it)
    model.before_train()
    data = synthetic_batch(2, 64, 96, n_categories=3, boxes_per_image=2, seed=1)
    losses = model(data)
    assert {"loss_class", "loss_class_0", "loss_class_enc", "loss_bbox_enc"} <= set(losses)
    assert all(torch.isfinite(v).all() for v in losses.values())
    sum(v.sum() for v in losses.values()).backward()
    for n, p in model.named_parameters():
        if "cls_linear" in n or "bbox_embed" in n:
            assert p.grad is not None and float(p.grad.abs().max()) > 0.0, n
        elif "adapter" not in n:
            assert p.grad is None, n


def test_header_build_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "zira_clslinear.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(zira_\w+)\s*\(", code)
    assert declared == ENTRIES == list(_lib.CLSLINEAR_SYMBOLS) == list(_lib.CLSLINEAR_PROTOTYPES)
    assert os.path.join(ROOT, "include", "zira_clslinear.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "clslinear.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    vp, i, ll, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t
    P = _lib.CLSLINEAR_PROTOTYPES
    assert P["zira_cls_linear_workspace_floats"] == (sz, [ll, i, i, i])
    assert P["zira_cls_linear_logits_fwd_f32"] == (i, [vp] * 9 + [ll] + [i] * 6 + [f32] + [vp] * 3)
    assert P["zira_cls_linear_logits_bwd_f32"] == (i, [vp] * 7 + [ll] + [i] * 5 + [vp] * 6)


def test_entry_points_decline_on_the_host():
    lib = _lib.load()
    for sym in ENTRIES:
        getattr(lib, sym)
    assert lib.zira_cls_linear_workspace_floats(12600, 256, 194, 80) > 12600 * 256
    for bad in ((0, 256, 5, 3), (6, 128, 5, 3), (6, 256, 257, 3), (6, 256, 5, 257), (6, 256, 0, 3), (6, 256, 5, 0), ((1 << 22) + 1, 256, 5, 3)):
        assert lib.zira_cls_linear_workspace_floats(*bad) == 0, bad
    # null pointers: -1, and nothing is launched (no GPU here)
    assert lib.zira_cls_linear_logits_fwd_f32(*([None] * 9 + [6, 2, 3, 5, 16, 3, 5, -100.0] + [None] * 3)) == -1
    assert lib.zira_cls_linear_logits_bwd_f32(*([None] * 7 + [6, 2, 3, 5, 16, 3] + [None] * 6)) == -1
