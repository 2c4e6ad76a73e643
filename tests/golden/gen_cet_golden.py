#!/usr/bin/env python3
"""Reference fixture of the CET text-adapter baseline, from the REFERENCE's own sibling class on the CPU: ``GroundingDINO`` of
models/GroundingDINO/groundingdino_dt.py with ``use_cet=True, use_zero_inter_loss=True`` and ``cet_type="Adapter"``, then
``"Linear"``, built over the stand-ins of gen_prompt_tuning_golden.py by the capture route of gen_prompt_memory_golden.py (the
backbone stand-in raises behind the text side and the text side's tensors are read from the raising frame's locals).

Reduced geometry: the encoder stand-in's 64 states, ``cet_middle_dim = 32``, ``hidden_dim = 256``, two captions of 10 tokens.
``mod_cet.pt`` records, per ``cet_type``:

* the adapter's state dict as the reference initialises it (keys, shapes, the zero up-projection) and the non-zero values that
  are then loaded (on the 1/64 grid);
* in training mode: ``encoded_text``, ``adapter_output`` and the text loss (``adapter_loss_text``, L1) of its ``forward``
  (:499-507), torch's own MSE and smooth-L1 means of the same ``adapter_output`` (what :208-215 would select), and the gradients
  of ``sum(encoded_text * upstream) + loss`` for every adapter parameter;
* in eval mode: ``encoded_text`` with ``use_prompt_memory_output`` True (the adapter is skipped) and False.

The text encoder is ``prompt_cases.GridBert`` (values multiples of 1/4) and ``feat_map``'s weights are rounded to 1/256, so the
projected text and the adapter's products are sums of exact terms; the loaded gate rows have one non-zero element each, so the
cosines are exact too and ``encoded_text`` is the same bits on any machine.  The loss (a mean of 5120 rounded numbers) and the
weight gradients (sums of rounded products over the rows) depend on the order a machine adds in: the test holds those to the
project's bar against a float64 evaluation instead.

    python tests/golden/gen_cet_golden.py      (needs the reference checkout ref_import.py names; CPU only)
"""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import gen_prompt_tuning_golden as tuning  # noqa: E402
from gen_prompt_memory_golden import MEMORY_CAPTIONS, capture  # noqa: E402

CET_MIDDLE_DIM = 32


def model_kw(cet_type):
    return dict(tuning.MODEL_KW, use_cet=True, cet_type=cet_type, cet_middle_dim=CET_MIDDLE_DIM, use_zero_inter_loss=True,
                use_prompt_tuning=False, use_prompt_memory=False, zero_loss_type="L1", loss_adapter_weight=0.1)


def one(ref, dt, cet_type):
    import prompt_cases as cases

    saved_kw, tuning.MODEL_KW = tuning.MODEL_KW, model_kw(cet_type)
    try:
        model = tuning.build(ref, dt)
    finally:
        tuning.MODEL_KW = saved_kw
    model.bert = cases.GridBert()
    with torch.no_grad():
        model.feat_map.weight.copy_(torch.round(model.feat_map.weight * 256) / 256)
        model.feat_map.bias.copy_(cases.grid((256,), torch.Generator().manual_seed(51), bound=0.5))
    init_state = {k: v.detach().clone() for k, v in model.cet_adapter.state_dict().items()}
    gen = torch.Generator().manual_seed(52)
    state = {k: cases.grid(tuple(v.shape), gen, bound=(1.0 if k == "gate.weight" else 0.25), quantum=64) for k, v in init_state.items()}
    # a gate row with ONE non-zero element: its normalised row is exactly +-1 there, so a row's cosine is one element of
    # x / |x| whatever order a CPU's GEMM adds in, and the encoded text is the same bits on every machine
    hot = torch.zeros_like(state["gate.weight"])
    for row in range(hot.shape[0]):
        at = (7 * row + 3) % hot.shape[1]
        hot[row, at] = state["gate.weight"][row, at] if float(state["gate.weight"][row, at]) != 0.0 else 0.5
    state["gate.weight"] = hot
    model.cet_adapter.load_state_dict(state)
    params = dict(model.cet_adapter.named_parameters())
    for p in params.values():
        p.requires_grad_(True)

    model.train()
    local = capture(model, dt, MEMORY_CAPTIONS)
    encoded, out, loss = local["encoded_text"], local["adapter_output"], local["adapter_loss_text"]
    assert float(out.detach().abs().max()) > 0 and float(loss.detach()) > 0 and tuple(loss.shape) == (1,)
    upstream = cases.grid(tuple(encoded.shape), torch.Generator().manual_seed(53))
    grads = torch.autograd.grad((encoded * upstream).sum() + loss.sum(), list(params.values()))
    zeros = torch.zeros_like(out)
    losses = {"L1": loss.detach().clone(), "L2": torch.nn.MSELoss()(out, zeros).detach().reshape(1).clone(),
              "Smooth_L1": torch.nn.SmoothL1Loss()(out, zeros).detach().reshape(1).clone()}
    model.eval()
    evals = {}
    for flag in (True, False):
        model.use_prompt_memory_output = flag
        with torch.no_grad():
            evals[flag] = capture(model, dt, MEMORY_CAPTIONS)["encoded_text"].detach().clone()
    with torch.no_grad():
        plain = model.feat_map(model.bert(input_ids=local["tokenized"]["input_ids"])["last_hidden_state"])
    assert torch.equal(evals[True], plain) and torch.equal(evals[False], encoded.detach())
    return dict(init_state=init_state, state=state, feat_map={k: v.detach().clone() for k, v in model.feat_map.state_dict().items()},
                encoded_text=encoded.detach().clone(), adapter_output=out.detach().clone(), losses=losses, upstream=upstream,
                grads={k: g.clone() for k, g in zip(params, grads)}, eval_memory_output=evals[True], eval_no_memory_output=evals[False])


def main():
    ref = ref_import.load()
    dt = importlib.import_module("groundingdino.models.GroundingDINO.groundingdino_dt")
    out = dict(captions=list(MEMORY_CAPTIONS), max_text_len=tuning.MODEL_KW["max_text_len"], cet_middle_dim=CET_MIDDLE_DIM,
               loss_adapter_weight=0.1, Adapter=one(ref, dt, "Adapter"), Linear=one(ref, dt, "Linear"))
    path = os.path.join(HERE, "mod_cet.pt")
    torch.save(out, path)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1e3), {k: float(v) for k, v in out["Adapter"]["losses"].items()})


if __name__ == "__main__":
    main()
