#!/usr/bin/env python3
"""Reference fixture of the prompt-tuning baseline (``use_prompt_tuning``), from the REFERENCE's own sibling class on the CPU:
``GroundingDINO`` of models/GroundingDINO/groundingdino_dt.py (registry name ``dtgroundingdino``), INSTANTIATED over a small
transformer with the stand-ins of gen_cls_linear_golden.py (a small locally built ``transformers.BertModel``, a tokenizer
stand-in -- here this package's ``SimpleTokenizer``, which is callable --, a backbone that only names its channels).

``mod_prompt_tuning.pt`` records

* what its ``add_cls_prompt`` (:379-437) puts into the pool for ``GOLDEN_CLASSES``;
* the substituted ``encoded_text`` of its ``forward`` (:521-531) for two images with different captions.  ``forward`` calls
  ``self.backbone(samples)`` directly after it has built ``text_dict``: the backbone stand-in raises there and ``text_dict`` is
  read from the raising frame's locals, so nothing behind the text side runs.  ``preprocess_image`` is replaced on the instance
  and ``nested_tensor_from_tensor_list`` on the module (they only have to name a device);
* the pool's gradients for a seeded upstream gradient through that captured tensor.

Bit equality on any machine: after construction the instance's text encoder is replaced by ``prompt_cases.GridBert`` (a lookup
whose values are multiples of 1/4) and ``feat_map``'s weights are rounded to 1/256, so the encoded text is a sum of exact
products, exact in fp32 in any order; the upstream gradient sits on the 1/256 grid as well.

    python tests/golden/gen_prompt_tuning_golden.py      (needs the reference checkout ref_import.py names; CPU only)
"""
import importlib
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
from gen_cls_linear_golden import BERT_HIDDEN, SMALL, _Backbone, exact_in_fp32  # noqa: E402
from gen_fullsize_golden import full_args  # noqa: E402

MODEL_KW = dict(num_queries=50, aux_loss=True, iter_update=True, query_dim=4, num_feature_levels=4, nheads=8,
                two_stage_type="standard", two_stage_bbox_embed_share=False, two_stage_class_embed_share=False,
                dec_pred_bbox_embed_share=True, max_text_len=32, freeze_all=True, use_cet=False, use_zero_inter_loss=False,
                use_add_names=False, use_project_adapter=True, use_prompt_tuning=True, device="cpu")


class _Captured(Exception):
    pass


class _RaisingBackbone(torch.nn.Module):
    num_channels = _Backbone.num_channels

    def forward(self, samples):
        raise _Captured()


def build(ref, dt):
    import transformers

    from ziragroundingdino_amd.bert import SimpleTokenizer

    cfg = transformers.BertConfig(hidden_size=BERT_HIDDEN, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128)
    dt.get_tokenlizer.get_tokenlizer = lambda name: SimpleTokenizer()

    def local_bert(name):
        bert = transformers.BertModel(cfg)
        for method in ("get_extended_attention_mask", "invert_attention_mask", "get_head_mask"):
            if not hasattr(bert, method):
                setattr(bert, method, None)
        return bert

    dt.get_tokenlizer.get_pretrained_language_model = local_bert
    tr = ref["transformer_for_adapter"].Transformer(**dict(full_args(), **SMALL))
    torch.manual_seed(30)
    return dt.GroundingDINO(_RaisingBackbone(), tr, **MODEL_KW)


def main():
    import prompt_cases as cases

    ref = ref_import.load()
    dt = importlib.import_module("groundingdino.models.GroundingDINO.groundingdino_dt")
    model = build(ref, dt).eval()
    model.bert = cases.GridBert()
    with torch.no_grad():
        model.feat_map.weight.copy_(torch.round(model.feat_map.weight * 256) / 256)
        model.feat_map.bias.copy_(cases.grid((256,), torch.Generator().manual_seed(31), bound=0.5))
    w = torch.cat([model.feat_map.weight.detach(), model.feat_map.bias.detach()[:, None]], -1)
    assert exact_in_fp32(torch.cat([model.bert.table, torch.ones(len(model.bert.table), 1)], -1), w, 2.0 ** -10)

    model.add_cls_prompt(list(cases.GOLDEN_CLASSES))
    pool = {k: v.detach().clone() for k, v in model.prompt_memory_pool.items()}
    assert list(pool) == ["-%s-" % c for c in cases.GOLDEN_CLASSES] and [len(v) for v in pool.values()] == [1, 3, 2, 2]
    # move the entries off their initial values (the text the frozen model sees), so that a substitution shows
    gen = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for p in model.prompt_memory_pool.values():
            p.copy_(cases.grid(tuple(p.shape), gen))
    trained = {k: v.detach().clone() for k, v in model.prompt_memory_pool.items()}

    model.preprocess_image = lambda batched_inputs: object()
    dt.nested_tensor_from_tensor_list = lambda images: types.SimpleNamespace(device="cpu")
    try:
        model([{"captions": c} for c in cases.GOLDEN_CAPTIONS])
        raise AssertionError("the backbone stand-in was not reached")
    except _Captured as stop:
        tb = stop.__traceback__
        frames = []
        while tb is not None:
            frames.append(tb.tb_frame)
            tb = tb.tb_next
        frame = next(f for f in frames if f.f_code.co_name == "forward" and "text_dict" in f.f_locals)
        text_dict = frame.f_locals["text_dict"]
        plain = frame.f_locals["bert_output"]["last_hidden_state"]
    encoded = text_dict["encoded_text"]
    with torch.no_grad():
        unsubstituted = model.feat_map(plain)
    assert encoded.requires_grad and not torch.equal(encoded.detach(), unsubstituted)
    upstream = cases.grid(tuple(encoded.shape), torch.Generator().manual_seed(33))
    encoded.backward(upstream)
    grads = {k: (v.grad.clone() if v.grad is not None else None) for k, v in model.prompt_memory_pool.items()}
    assert grads["-sea otter-"] is None and float(grads["-cat-"].abs().max()) > 0

    out = dict(classes=list(cases.GOLDEN_CLASSES), captions=list(cases.GOLDEN_CAPTIONS), max_text_len=MODEL_KW["max_text_len"],
               feat_map={k: v.detach().clone() for k, v in model.feat_map.state_dict().items()},
               pool_initial=pool, pool_trained=trained, encoded_text=encoded.detach().clone(), unsubstituted=unsubstituted,
               text_token_mask=text_dict["text_token_mask"].clone(), upstream=upstream,
               pool_grads={k: v for k, v in grads.items() if v is not None})
    path = os.path.join(HERE, "mod_prompt_tuning.pt")
    torch.save(out, path)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1e3), tuple(encoded.shape))


if __name__ == "__main__":
    main()
