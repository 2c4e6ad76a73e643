#!/usr/bin/env python3
"""Reference fixtures of the linear-probing baseline (``use_cls_linear``), from the REFERENCE's own classes on the CPU.

* ``mod_contrastive_linear.pt``: ``ContrastiveEmbedwithLinear`` (models/GroundingDINO/utils.py:272-310) -- inputs, the
  two parameters (its default initialisation, rounded to 1/256) and the output; a ragged token mask and fewer text tokens than
  ``max_text_len``; values on binary grids coarse enough that fp32 adds them exactly in any order.
* ``cls_linear_state_dict_keys.json``: names and shapes only.  The reference's ``GroundingDINO`` class
  (groundingdino_dual_zero_rep_branch.py:137-745) INSTANTIATED with ``use_cls_linear=True`` over a small transformer: every
  state-dict key outside ``bert.`` / ``backbone.`` with its shape, and the parameters ``before_train()`` leaves trainable
  (``freeze_all=True``).  The class fetches its text encoder by name; the two fetching functions are replaced here by a small
  locally built ``transformers.BertModel`` and a tokenizer stand-in, the backbone by a module that only names its channels --
  which is why their keys are left out.

    python tests/golden/gen_cls_linear_golden.py      (needs /root/reference; never runs on the GPU box)
"""
import contextlib
import io
import json
import os
import sys

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
from gen_fullsize_golden import full_args  # noqa: E402

MAX_TEXT_LEN, B, Q, T = 16, 2, 7, 9
N_TOK = (5, 9)
# the small model of tests/test_model_gpu.py: 2 + 2 layers, FFN 128, 50 queries, text length 32, a Swin of width 24
SMALL = dict(num_queries=50, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=128, fusion_droppath=0.0)
CHANNELS = [48, 96, 192]
BERT_HIDDEN = 64
MODEL_KW = dict(num_queries=50, aux_loss=True, iter_update=True, query_dim=4, num_feature_levels=4, nheads=8,
                two_stage_type="standard", two_stage_bbox_embed_share=False, two_stage_class_embed_share=False,
                dec_pred_bbox_embed_share=True, max_text_len=32, freeze_all=True, use_cet=True, use_project_adapter=True,
                use_cls_linear=True)


class _Backbone(nn.Module):
    num_channels = CHANNELS


class _Tokenizer:
    def convert_tokens_to_ids(self, tokens):
        return [{"[CLS]": 101, "[SEP]": 102, ".": 1012, "?": 1029}[t] for t in tokens]


def exact_in_fp32(a, b, quantum):
    """every sum of products a[.., k] * b[.., k] over k, in ANY order and with or without fused multiply-adds, is exact in fp32:
    all terms are multiples of ``quantum`` and the sum of their magnitudes stays below 2^24 quanta"""
    return float((a.abs().double() @ b.abs().double().transpose(-1, -2)).max()) / quantum < 2 ** 24


def module_fixture(ref):
    """The values sit on coarse binary grids (x: 1/4, weights and bias: 1/256 -- the default initialisation rounded to it --,
    text: 1/2), so that both products are exact in fp32 whatever order a CPU's GEMM kernels add in: the stored output is then
    the same bits on every machine, which is what lets the test ask for equality."""
    torch.manual_seed(20)
    mod = ref["utils"].ContrastiveEmbedwithLinear(max_text_len=MAX_TEXT_LEN, hidden_dim=256)
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.round(p * 256) / 256)
    x = torch.round(torch.randn(B, Q, 256, generator=g).clamp(-2, 2) * 4) / 4
    text = torch.round(torch.randn(B, T, 256, generator=g).clamp(-1, 1) * 2) / 2
    mask = torch.zeros(B, T, dtype=torch.bool)
    for b, n in enumerate(N_TOK):
        mask[b, :n] = True
    with torch.no_grad():
        z = mod.cls_linear(x)
        out = mod(x, {"encoded_text": text, "text_token_mask": mask})
    w, bias = mod.cls_linear.weight.detach(), mod.cls_linear.bias.detach()
    assert float(w.abs().max()) > 0 and exact_in_fp32(torch.cat([x, torch.ones(B, Q, 1)], -1), torch.cat([w, bias[:, None]], -1), 2.0 ** -10)
    assert exact_in_fp32(z, text, 2.0 ** -11)
    return dict(max_text_len=MAX_TEXT_LEN, x=x, encoded_text=text, text_token_mask=mask, out=out,
                state={k: v.clone() for k, v in mod.state_dict().items()})


def keys_fixture(ref):
    import transformers

    zr = ref["groundingdino_dual_zero_rep_branch"]
    cfg = transformers.BertConfig(hidden_size=BERT_HIDDEN, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128)
    zr.get_tokenlizer.get_tokenlizer = lambda name: _Tokenizer()

    def local_bert(name):
        bert = transformers.BertModel(cfg)
        for method in ("get_extended_attention_mask", "invert_attention_mask", "get_head_mask"):
            if not hasattr(bert, method):       # the warper only keeps handles to them (bertwarper.py:27-29); nothing here calls them
                setattr(bert, method, None)
        return bert

    zr.get_tokenlizer.get_pretrained_language_model = local_bert
    tr = ref["transformer_for_adapter"].Transformer(**dict(full_args(), **SMALL))
    model = zr.GroundingDINO(_Backbone(), tr, **MODEL_KW)
    with contextlib.redirect_stdout(io.StringIO()):       # (the reference prints every name it unfreezes)
        model.before_train()
    outside = ("bert.", "backbone.")
    return {"model_kwargs": MODEL_KW, "transformer_kwargs": SMALL, "channels": CHANNELS, "bert_hidden": BERT_HIDDEN,
            "state_dict": {k: list(v.shape) for k, v in model.state_dict().items() if not k.startswith(outside)},
            "trainable": [n for n, p in model.named_parameters() if p.requires_grad and not n.startswith(outside)]}


def main():
    ref = ref_import.load()
    path = os.path.join(HERE, "mod_contrastive_linear.pt")
    torch.save(module_fixture(ref), path)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1e3))
    path = os.path.join(HERE, "cls_linear_state_dict_keys.json")
    out = keys_fixture(ref)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print("wrote", path, len(out["state_dict"]), "keys,", len(out["trainable"]), "trainable, %.1f KB" % (os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
