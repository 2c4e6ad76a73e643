"""Golden vectors for the model EMA (ziragroundingdino_amd/ema.py): the reference's own ``EMAState`` / ``EMAUpdater``
(groundingdino/util/ema.py) driven on the CPU over a tiny module for 8 steps of parameter changes -> ema_zira_slice.pt.

The module, its initial values and the change of every step are plain IEEE arithmetic on index ramps (``tiny_module``,
``set_step`` below), so the tests rebuild them bit for bit and the fixture holds only what the reference computed: the
averaged state after each step, and the buffers of the model inside / after ``apply_and_restore`` (the generator asserts that
the fp32 tensors inside the context are the state of step 8 and afterwards the parameters of step 8, so they are not stored
twice).  The tests import ``tiny_module`` / ``set_step`` / ``model_state`` from this file; the reference is touched in
``main`` only.

    python tests/golden/gen_ema_golden.py
"""
import os
import sys
import types

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))

# fp32 parameters, in this order (tests/test_ema_gpu.py lays them out as separate allocations and as offset views)
SIZES = [1, 3, 4095, 1, 4097, 4096] + [5] * 17 + [8192 + 7]
STEPS = 8
DECAY = 0.999


def _initial(i, n):
    """Values of parameter i: multiples of 1/64 stretched by a 13-periodic factor, both signs, zeros among them."""
    j = torch.arange(n, dtype=torch.float32)
    v = ((j * 37 + i * 11) % 101 - 50) / 64
    v = v * (1 + (j % 13) / 16)
    if n >= 4097:      # signed zeros and the far ends of the normal range
        v[:4] = torch.tensor([0.0, -0.0, 1e30, -3e-30])
    return v


class Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        for i, n in enumerate(SIZES):
            self.register_parameter("p%02d" % i, nn.Parameter(_initial(i, n)))
        self.register_buffer("ratio16", torch.tensor([0.5, -1.25, 3.0, 0.0, 100.0, -0.001], dtype=torch.float16))
        self.register_buffer("count", torch.tensor([0, 5, 1000], dtype=torch.int64))
        self.register_buffer("flag", torch.tensor([True, False, True, False]))


def tiny_module():
    return Tiny()


def set_step(model, k):
    """The model's tensors after training step k (1-based), in place, from those of step k - 1."""
    with torch.no_grad():
        for i, n in enumerate(SIZES):
            p = getattr(model, "p%02d" % i)
            p.add_(_initial(i, n).to(p.device) * (0.03125 * k))
        model.ratio16.add_(0.25)
        model.count.add_(3 * k)
        if k % 2 == 1:
            model.flag.logical_not_()


def model_state(model):
    """name -> clone, parameters then buffers."""
    return {k: v.detach().clone() for k, v in list(model.named_parameters()) + list(model.named_buffers())}


def main():
    sys.path.insert(0, HERE)
    import ref_import

    ref_import.load()
    for name in ("detectron2.engine", "detectron2.engine.train_loop"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["detectron2.engine.train_loop"].HookBase = object
    from groundingdino.util import ema as ref

    model = tiny_module()
    state = ref.EMAState()
    updater = ref.EMAUpdater(state, decay=DECAY, device="")
    updater.init_state(model)
    steps = []
    for k in range(1, STEPS + 1):
        set_step(model, k)
        updater.update(model)
        steps.append({name: val.clone() for name, val in state.state_dict().items()})
    before = model_state(model)
    with state.apply_and_restore(model):
        applied = model_state(model)
    restored = model_state(model)
    params = [name for name, _ in model.named_parameters()]
    buffers = [name for name, _ in model.named_buffers()]
    assert all(torch.equal(applied[k].view(torch.int32), steps[-1][k].view(torch.int32)) for k in params)
    assert all(torch.equal(restored[k].view(torch.int32), before[k].view(torch.int32)) for k in params)
    out = {"decay": DECAY, "sizes": SIZES, "keys": list(state.state_dict().keys()), "steps": steps,
           "applied_buffers": {k: applied[k] for k in buffers}, "restored_buffers": {k: restored[k] for k in buffers}}
    path = os.path.join(HERE, "ema_zira_slice.pt")
    torch.save(out, path)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
