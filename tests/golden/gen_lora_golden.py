#!/usr/bin/env python3
"""Reference fixture of the low-rank language side branch, from the REFERENCE's own ``RepZeroLoRA`` class
(models/GroundingDINO/adapter.py:227-259) on the CPU, imported by the ref_import.py route like gen_modules_golden.py.

``mod_rep_zero_lora.pt`` records, at 64 -> 32 -> 256 (the smallest geometry the native node takes: two panels of features, one
hidden panel) and x ``[2, 7, 64]``:

* ``init_state``: the state dict at construction (``scaling`` 0.1, ``down`` / ``up`` 1e-8, a zero twin) and ``keys``, the
  module's ``[name, shape]`` list in state-dict order;
* ``state``: a seeded O(1) state in which ``|branch|`` and ``|out|`` lie on BOTH sides of 1 (asserted here), so both arms of
  SmoothL1 and of its derivative are exercised -- at the 1e-8 initialisation nothing crosses the knee;
* in that state: ``x``, train-mode ``out`` and ``zl``, the gradients of ``sum(out * grad_out) + zl_weight * zl`` for x and the
  four parameters, the eval output, and the state after ``__rep__``.

    python tests/golden/gen_lora_golden.py      (needs the reference checkout ref_import.py names; CPU only)
"""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

IN, DOWN, OUT = 64, 32, 256
SCALES = {"scaling": None, "freeze_linear.weight": 0.05, "down.weight": 0.2, "up.weight": 0.2}


def sd(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def main():
    ref_import.load()
    A = importlib.import_module("groundingdino.models.GroundingDINO.adapter")
    g = torch.Generator().manual_seed(61)
    mod = A.RepZeroLoRA(IN, OUT, down_dim=DOWN)
    init_state = sd(mod)
    keys = [[k, list(v.shape)] for k, v in init_state.items()]
    with torch.no_grad():
        for k, p in mod.named_parameters():
            p.copy_(torch.full((1,), 0.3) if k == "scaling" else torch.randn(p.shape, generator=g) * SCALES[k])
    x = torch.randn(2, 7, IN, generator=g, requires_grad=True)
    mod.train()
    out, zl = mod(x)
    branch = (mod.scaling * mod.up(mod.down(x))).detach()
    for name, t in (("branch", branch), ("out", out.detach())):
        above = float((t.abs() > 1).float().mean())
        assert 0.02 < above < 0.98, (name, above)
        print("%-6s |.| > 1 on %.1f %% of the elements, max %.2f" % (name, 100 * above, float(t.abs().max())))
    go = torch.randn(out.shape, generator=g)
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad((out * go).sum() + 0.7 * zl, [x] + list(params.values()))
    mod.eval()
    out_eval, zl_eval = mod(x)
    state = sd(mod)
    mod.__rep__()
    path = os.path.join(HERE, "mod_rep_zero_lora.pt")
    torch.save(dict(dims=[IN, DOWN, OUT], keys=keys, init_state=init_state, state=state, x=x.detach(), out=out.detach(),
                    zl=zl.detach(), grad_out=go, zl_weight=0.7, grad_x=grads[0],
                    grad_params={k: gr for k, gr in zip(params, grads[1:])}, out_eval=out_eval.detach(),
                    zl_eval=zl_eval.detach(), state_after_rep=sd(mod)), path)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
