#!/usr/bin/env python3
"""Reference fixture of the text-memory replay (``use_prompt_memory``), from the REFERENCE's own sibling class on the CPU:
``GroundingDINO`` of models/GroundingDINO/groundingdino_dt.py with ``use_cet=True, cet_type="Adapter", use_prompt_memory=True,
use_zero_inter_loss=True``, built over the stand-ins of gen_prompt_tuning_golden.py (the capture route: the backbone stand-in
raises behind the text side and the text side's tensors are read from the raising frame's locals).

``mod_prompt_memory.pt`` records

* what its ``add_cls_prompt`` (:379-437) puts into the pool for ``MEMORY_CLASSES`` and the values the entries are moved to;
* in training mode, with ``learned_classes`` set: ``encoded_text`` and ``loss_prompt_memory`` of its ``forward`` (:509-519) for
  two images whose captions share a class (so one pool row has two occurrences -- a sum of two fp32 numbers is order-free) and
  hold one class that is not learned;
* ``autograd.grad`` of that loss with respect to the encoded text and, with the entries set to require grad, to the pool;
* the dict its ``replay_memory()`` (:786-838) returns.

Bit equality on any machine: the text encoder is ``prompt_cases.GridBert`` (values multiples of 1/4), ``feat_map``'s weights are
rounded to 1/256, the entries sit on the 1/256 grid, and the reference's ``Adapter`` starts with a zero up-projection, so its
output is exactly zero and the encoded text is a sum of exact products.  The gradients are +-1/N or sums of two of them.

    python tests/golden/gen_prompt_memory_golden.py      (needs the reference checkout ref_import.py names; CPU only)
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
import gen_prompt_tuning_golden as tuning  # noqa: E402
from gen_cls_linear_golden import exact_in_fp32  # noqa: E402

MODEL_KW = dict(tuning.MODEL_KW, use_cet=True, cet_type="Adapter", use_prompt_memory=True, use_zero_inter_loss=True,
                use_prompt_tuning=False)
# "walrus" is in a caption and not learned; "sea otter" is learned and in no caption; "cat" is in both captions
MEMORY_CLASSES = ["cat", "polar bear cub", "sea otter", "red fox"]
MEMORY_CAPTIONS = ["cat.polar bear cub.walrus.", "red fox.cat.gray seal."]


def capture(model, dt, captions):
    """locals of the reference's ``forward`` at the point where the backbone stand-in raises"""
    model.preprocess_image = lambda batched_inputs: object()
    dt.nested_tensor_from_tensor_list = lambda images: types.SimpleNamespace(device="cpu")
    model.prepare_targets = lambda *a, **k: None
    try:
        model([{"captions": c, "instances": types.SimpleNamespace(to=lambda d: None)} for c in captions])
        raise AssertionError("the backbone stand-in was not reached")
    except tuning._Captured as stop:
        tb = stop.__traceback__
        frames = []
        while tb is not None:
            frames.append(tb.tb_frame)
            tb = tb.tb_next
        return next(f for f in frames if f.f_code.co_name == "forward" and "text_dict" in f.f_locals).f_locals


def main():
    import prompt_cases as cases

    ref = ref_import.load()
    dt = importlib.import_module("groundingdino.models.GroundingDINO.groundingdino_dt")
    saved_kw, tuning.MODEL_KW = tuning.MODEL_KW, MODEL_KW
    try:
        model = tuning.build(ref, dt)
    finally:
        tuning.MODEL_KW = saved_kw
    model.bert = cases.GridBert()
    with torch.no_grad():
        model.feat_map.weight.copy_(torch.round(model.feat_map.weight * 256) / 256)
        model.feat_map.bias.copy_(cases.grid((256,), torch.Generator().manual_seed(41), bound=0.5))
    w = torch.cat([model.feat_map.weight.detach(), model.feat_map.bias.detach()[:, None]], -1)
    assert exact_in_fp32(torch.cat([model.bert.table, torch.ones(len(model.bert.table), 1)], -1), w, 2.0 ** -10)

    model.eval()
    model.add_cls_prompt(list(MEMORY_CLASSES))
    pool_initial = {k: v.detach().clone() for k, v in model.prompt_memory_pool.items()}
    assert list(pool_initial) == ["-%s-" % c for c in MEMORY_CLASSES] and [len(v) for v in pool_initial.values()] == [1, 3, 2, 2]
    gen = torch.Generator().manual_seed(42)
    with torch.no_grad():       # off their initial values: the loss and its gradients are not zero
        for p in model.prompt_memory_pool.values():
            p.copy_(cases.grid(tuple(p.shape), gen))
    pool = {k: v.detach().clone() for k, v in model.prompt_memory_pool.items()}
    model.learned_classes = list(MEMORY_CLASSES)
    for p in model.prompt_memory_pool.values():
        p.requires_grad_(True)

    model.train()
    local = capture(model, dt, MEMORY_CAPTIONS)
    encoded, loss = local["encoded_text"], local["loss_prompt_memory"]
    adapter_output = local["adapter_output"]
    assert not bool(adapter_output.detach().any()), "the zero-initialised adapter is expected to add exactly nothing"
    assert float(loss.detach()) > 0 and encoded.requires_grad
    params = list(model.prompt_memory_pool.values())
    grads = torch.autograd.grad(loss, [encoded] + params, allow_unused=True)
    g_text, g_pool = grads[0], dict(zip(model.prompt_memory_pool.keys(), grads[1:]))
    assert g_pool["-sea otter-"] is None and float(g_pool["-cat-"].abs().max()) > 0
    replay = {k: v.detach().clone() for k, v in model.replay_memory().items()}
    assert set(replay) == {"loss_prompt_memory", "loss_adapter_text"}

    out = dict(classes=list(MEMORY_CLASSES), captions=list(MEMORY_CAPTIONS), max_text_len=MODEL_KW["max_text_len"],
               feat_map={k: v.detach().clone() for k, v in model.feat_map.state_dict().items()},
               pool_initial=pool_initial, pool=pool, encoded_text=encoded.detach().clone(), loss_prompt_memory=loss.detach().clone(),
               grad_encoded_text=g_text.clone(), grad_pool={k: v.clone() for k, v in g_pool.items() if v is not None},
               replay=replay)
    path = os.path.join(HERE, "mod_prompt_memory.pt")
    torch.save(out, path)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1e3), tuple(encoded.shape), float(loss), {k: float(v) for k, v in replay.items()})


if __name__ == "__main__":
    main()
