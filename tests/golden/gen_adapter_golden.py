#!/usr/bin/env python3
"""Golden vectors for the gated adapter baseline (``use_adapter``), generated FROM THE REFERENCE (its pure-PyTorch CPU path,
imported with stubs -- see ref_import.py).  Build container only.

    python tests/golden/gen_adapter_golden.py

Writes tests/golden/mod_adapter.pt -- the reference's ``Adapter`` (models/GroundingDINO/adapter.py:124-179) with its inits
replaced by name-seeded noise (seeded.py: the state dict is its keys, shapes and the salt; both sides rebuild the values), one
entry per (use_gate, use_self_kd): a seeded input [2, 37, 256], output, loss and the gradients of the input and the parameters.
All four entries share the weights, the input and the output gradient, and ``use_self_kd`` changes nothing but the loss and
the input's gradient (asserted here), so the tensors that are equal are stored once: the file stays under the size limit for a
committed file.  And tests/golden/mod_adapter_layers.pt: one reference encoder layer and one reference decoder layer with
``use_adapter=True`` at the tiny model sizes gen_modules_golden.py uses for the transformer (weights by name, not stored; the
decoder's memory is the encoder's input), with outputs, ``adapter_loss`` and gradients.
"""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
from gen_modules_golden import randomize_, save, sd, shapes_meta  # noqa: E402
from seeded import fill_by_name_, layernorm_weights_plus_one_  # noqa: E402

LAYER_SALT = "adapter_layers/"
LAYER_KW = dict(d_model=256, d_ffn=64, dropout=0.0, activation="relu", n_levels=3, n_heads=8, n_points=2, use_adapter=True,
                use_self_kd=True)
LOSS_WEIGHT = 0.7


ADAPTER_SALT = "adapter/"
ADAPTER_SCALE = 0.1


def gen_adapter(A):
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(2, 37, 256, generator=g)
    go = torch.randn(2, 37, 256, generator=g)
    entries = dict(salt=ADAPTER_SALT, scale=ADAPTER_SCALE, x=x0, grad_out=go, loss_weight=LOSS_WEIGHT)
    for use_gate in (True, False):
        first = None
        for use_self_kd in (False, True):
            mod = A.Adapter(embed_dim=256, down_dim=64, activation=torch.nn.functional.relu, ffn_drop=0, num_gate_embed=5,
                            gate_T=2.0, gate_base_scale=0.5, use_gate=use_gate, use_self_kd=use_self_kd)
            init = {k: (tuple(v.shape), float(v.abs().max())) for k, v in mod.state_dict().items()}
            fill_by_name_(mod, ADAPTER_SALT, ADAPTER_SCALE)
            x = x0.clone().requires_grad_(True)
            out, loss = mod(x)
            params = dict(mod.named_parameters())
            grads = torch.autograd.grad((out * go).sum() + LOSS_WEIGHT * loss.sum(), [x] + list(params.values()), allow_unused=True)
            e = dict(use_gate=use_gate, use_self_kd=use_self_kd, state_keys=list(mod.state_dict()), init=init, out=out.detach(),
                     loss=loss.detach(), grad_x=grads[0], grad_params=dict(zip(params, grads[1:])))      # (None: a gate not in use)
            if first is None:
                first = e
            else:       # what use_self_kd leaves alone is stored once (torch.save keeps shared tensors shared)
                assert torch.equal(e["out"], first["out"])
                e["out"] = first["out"]
                for k, v in e["grad_params"].items():
                    assert (v is None and first["grad_params"][k] is None) or torch.equal(v, first["grad_params"][k])
                e["grad_params"] = first["grad_params"]
            entries["gate%d_kd%d" % (use_gate, use_self_kd)] = e
    save("adapter", entries)


def gen_layers(T_):
    g = torch.Generator().manual_seed(32)
    shapes = [(4, 6), (2, 3), (1, 2)]
    sh, start = shapes_meta(shapes)
    S, B, d = int((sh[:, 0] * sh[:, 1]).sum()), 2, 256

    def prepare(layer, prefix):
        fill_by_name_(layer, LAYER_SALT, 0.05, {"sampling_offsets.bias": 0.6, "adapter": 0.1}, prefix=prefix)
        layernorm_weights_plus_one_(layer)
        return layer.eval()      # (dropout 0)

    enc = prepare(T_.DeformableTransformerEncoderLayer(encoder_gate_base_scale=0.1, **LAYER_KW), "encoder.")
    src = torch.randn(B, S, d, generator=g).requires_grad_(True)
    pos = torch.randn(B, S, d, generator=g)
    ref = torch.rand(B, S, 3, 2, generator=g)
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[1, -3:] = True
    out, aloss = enc(src=src, pos=pos, reference_points=ref, spatial_shapes=sh, level_start_index=start, key_padding_mask=mask)
    go = torch.randn(out.shape, generator=g)
    params = dict(enc.named_parameters())
    grads = torch.autograd.grad((out * go).sum() + LOSS_WEIGHT * aloss.sum(), [src] + list(params.values()))
    encoder = dict(param_names=list(params), src=src.detach(), pos=pos, reference_points=ref, key_padding_mask=mask,
                   out=out.detach(), adapter_loss=aloss.detach(), grad_out=go, grad_src=grads[0],
                   grad_params={k: gr for k, gr in zip(params, grads[1:]) if "adapter" in k})

    dec = prepare(T_.DeformableTransformerDecoderLayer(use_text_cross_attention=True, decoder_gate_base_scale=0.1, **LAYER_KW),
                  "decoder.")
    Q, T = 12, 6
    tgt = torch.randn(Q, B, d, generator=g).requires_grad_(True)
    qpos = torch.randn(Q, B, d, generator=g)
    refp = torch.cat([torch.rand(Q, B, 3, 2, generator=g), 0.1 + 0.3 * torch.rand(Q, B, 3, 2, generator=g)], -1)
    memory = src.detach().transpose(0, 1).requires_grad_(True)      # (stored once, as the encoder's input)
    text = torch.randn(B, T, d, generator=g).requires_grad_(True)
    tpad = torch.zeros(B, T, dtype=torch.bool)
    tpad[1, -1] = True
    out, aloss = dec(tgt=tgt, tgt_query_pos=qpos, tgt_reference_points=refp, memory_text=text, text_attention_mask=tpad,
                     memory=memory, memory_key_padding_mask=mask, memory_level_start_index=start, memory_spatial_shapes=sh)
    go = torch.randn(out.shape, generator=g)
    params = dict(dec.named_parameters())
    grads = torch.autograd.grad((out * go).sum() + LOSS_WEIGHT * aloss.sum(), [tgt, memory, text] + list(params.values()))
    decoder = dict(param_names=list(params), tgt=tgt.detach(), query_pos=qpos, reference_points=refp,
                   text=text.detach(), text_padding_mask=tpad, memory_padding_mask=mask, out=out.detach(),
                   adapter_loss=aloss.detach(), grad_out=go, grad_tgt=grads[0], grad_memory=grads[1], grad_text=grads[2],
                   grad_params={k: gr for k, gr in zip(params, grads[3:]) if "adapter" in k})
    save("adapter_layers", dict(kwargs=LAYER_KW, salt=LAYER_SALT, scale=0.05, scales={"sampling_offsets.bias": 0.6, "adapter": 0.1},
                                shapes=shapes, loss_weight=LOSS_WEIGHT, encoder=encoder, decoder=decoder))


def main():
    torch.set_num_threads(1)
    ref = ref_import.load()
    gen_adapter(importlib.import_module("groundingdino.models.GroundingDINO.adapter"))
    gen_layers(ref["transformer_for_adapter"])


if __name__ == "__main__":
    main()
