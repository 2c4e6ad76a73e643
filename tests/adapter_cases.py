"""Shared by tests/test_adapter_cpu.py and tests/test_adapter_gpu.py: the reference fixtures of the gated adapter
(tests/golden/gen_adapter_golden.py) and the checks of the module and of the two layers against them, on a device."""
import os
import sys

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
from seeded import fill_by_name_, layernorm_weights_plus_one_  # noqa: E402

from test_modules_golden import close, load, to  # noqa: E402

from ziragroundingdino_amd import adapter as zadapter  # noqa: E402
from ziragroundingdino_amd import transformer  # noqa: E402

TOL, GRAD_TOL = 1e-4, 2e-4         # test_modules_golden.py's: outputs, gradients (scaled by the tensor's largest magnitude)
REF_KEYS = ["adapter_down.weight", "adapter_down.bias", "adapter_up.weight", "adapter_up.bias", "gate.weight"]


def check_adapter_entry(g, name, dev):
    """One (use_gate, use_self_kd) entry of mod_adapter.pt: keys, init, output, loss and every gradient."""
    e = g[name]
    mod = zadapter.Adapter(embed_dim=256, down_dim=64, activation=F.relu, ffn_drop=0, num_gate_embed=5, gate_T=2.0,
                           gate_base_scale=0.5, use_gate=e["use_gate"], use_self_kd=e["use_self_kd"])
    assert list(mod.state_dict()) == e["state_keys"] == REF_KEYS
    for k, v in mod.state_dict().items():       # shapes, and which tensors start at zero
        shape, largest = e["init"][k]
        assert tuple(v.shape) == shape and (float(v.abs().max()) == 0.0) == (largest == 0.0), k
    bound = 1.0 / 256 ** 0.5                    # kaiming_uniform_(a = sqrt(5)) on fan_in 256
    assert 0.9 * bound < float(mod.adapter_down.weight.detach().abs().max()) <= bound
    fill_by_name_(mod, g["salt"], g["scale"])
    mod.to(dev)
    e, x0, go = to(e, dev), g["x"].to(dev), g["grad_out"].to(dev)
    x = x0.clone().requires_grad_(True)
    out, loss = mod(x)
    assert loss.shape == (1,) and out.shape == x.shape
    close(out, e["out"], TOL, name + " out")
    close(loss, e["loss"], TOL, name + " loss")
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad((out * go).sum() + g["loss_weight"] * loss.sum(), [x] + list(params.values()), allow_unused=True)
    close(grads[0], e["grad_x"], GRAD_TOL, name + " grad_x")
    for k, got in zip(params, grads[1:]):
        want = e["grad_params"][k]
        assert (got is None) == (want is None), k
        if want is not None:
            close(got, want, GRAD_TOL, name + " grad " + k)
    return out


def _prepared(layer, g, prefix, dev):
    fill_by_name_(layer, g["salt"], g["scale"], g["scales"], prefix=prefix)
    layernorm_weights_plus_one_(layer)
    return layer.to(dev).eval()


def shapes_meta(shapes, dev):
    sh = torch.tensor(shapes, dtype=torch.long, device=dev)
    start = torch.cat([sh.new_zeros(1), (sh[:, 0] * sh[:, 1]).cumsum(0)[:-1]])
    return sh, start


def check_encoder_layer(dev, trainable_adapter_only=False):
    g = load("adapter_layers")
    e = g["encoder"]
    layer = transformer.DeformableTransformerEncoderLayer(encoder_gate_base_scale=0.1, **g["kwargs"])
    assert [n for n, _ in layer.named_parameters()] == e["param_names"]
    _prepared(layer, g, "encoder.", dev)
    if trainable_adapter_only:      # the baseline's regime: a frozen layer (its fast paths) with a trained adapter
        for n, p in layer.named_parameters():
            p.requires_grad_("adapter" in n)
    e = to(e, dev)
    sh, start = shapes_meta(g["shapes"], dev)
    src = e["src"].clone().requires_grad_(True)
    out, aloss = layer(src, e["pos"], e["reference_points"], sh, start, key_padding_mask=e["key_padding_mask"])
    close(out, e["out"], TOL, "encoder out")
    close(aloss, e["adapter_loss"], TOL, "encoder adapter_loss")
    wanted = [(n, p) for n, p in layer.named_parameters() if "adapter" in n]
    grads = torch.autograd.grad((out * e["grad_out"]).sum() + g["loss_weight"] * aloss.sum(), [src] + [p for _, p in wanted])
    close(grads[0], e["grad_src"], GRAD_TOL, "encoder grad_src")
    for (n, _), got in zip(wanted, grads[1:]):
        close(got, e["grad_params"][n], GRAD_TOL, "encoder grad " + n)
    return layer


def check_decoder_layer(dev, trainable_adapter_only=False):
    g = load("adapter_layers")
    e = g["decoder"]
    layer = transformer.DeformableTransformerDecoderLayer(use_text_cross_attention=True, decoder_gate_base_scale=0.1, **g["kwargs"])
    assert [n for n, _ in layer.named_parameters()] == e["param_names"]
    _prepared(layer, g, "decoder.", dev)
    if trainable_adapter_only:
        for n, p in layer.named_parameters():
            p.requires_grad_("adapter" in n)
    e = to(e, dev)
    sh, start = shapes_meta(g["shapes"], dev)
    tgt = e["tgt"].clone().requires_grad_(True)
    memory = to(g["encoder"]["src"], dev).transpose(0, 1).clone().requires_grad_(True)
    text = e["text"].clone().requires_grad_(True)
    out, aloss = layer(tgt=tgt, tgt_query_pos=e["query_pos"], tgt_reference_points=e["reference_points"], memory_text=text,
                       text_attention_mask=e["text_padding_mask"], memory=memory, memory_key_padding_mask=e["memory_padding_mask"],
                       memory_level_start_index=start, memory_spatial_shapes=sh)
    close(out, e["out"], TOL, "decoder out")
    close(aloss, e["adapter_loss"], TOL, "decoder adapter_loss")
    wanted = [(n, p) for n, p in layer.named_parameters() if "adapter" in n]
    grads = torch.autograd.grad((out * e["grad_out"]).sum() + g["loss_weight"] * aloss.sum(),
                                [tgt, memory, text] + [p for _, p in wanted])
    for got, key in zip(grads[:3], ("grad_tgt", "grad_memory", "grad_text")):
        close(got, e[key], GRAD_TOL, "decoder " + key)
    for (n, _), got in zip(wanted, grads[3:]):
        close(got, e["grad_params"][n], GRAD_TOL, "decoder grad " + n)
    return layer
