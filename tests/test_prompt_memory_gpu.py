"""The memory loss on the GPU: the autograd node over csrc/prompt_memory.hip against ``memory_loss_reference`` on the device --
``gx`` and ``g_pool`` bit for bit (the cases' values sit on binary grids and a pool row has at most two occurrences, or
s = g / N is a power of two, so the sums are exact in any order), the loss to the project's bar --, twice over, under graph
capture replayed three times (the ticket is left at zero), the switches and the declined shapes take the definition, and the
small model hands the same loss over on the direct and on the prefetched route."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import prompt_cases as cases  # noqa: E402
import prompt_memory_cases as mcases  # noqa: E402

from ziragroundingdino_amd import prompt  # noqa: E402
from ziragroundingdino_amd.transformer import Switches  # noqa: E402

CASES = mcases.memory_cases()
DEV = "cuda"
NATIVE = "_MemoryLossNativeBackward"
_TABLES = {}


def table_of(case):
    if case.name not in _TABLES:
        keys = list(case.pool)
        _TABLES[case.name] = prompt.build_table(case.names_list, case.masks(), keys, [case.pool[k].shape[0] for k in keys], case.T)
    return _TABLES[case.name]


def run(fn, case, weight, x_grad=True, pool_grad=True):
    table = table_of(case)
    x = case.x.to(DEV).requires_grad_(x_grad)
    pool = [v.to(DEV).requires_grad_(pool_grad) for v in case.pool.values()]
    loss = fn(x, table, pool)
    (loss * weight).backward()
    return loss.detach(), x.grad, [p.grad if p.grad is not None else torch.zeros_like(p) for p in pool], loss.grad_fn


@pytest.mark.parametrize("case,weight", CASES, ids=[c.name for c, _ in CASES])
def test_native_equals_the_reference(case, weight):
    want = run(prompt.memory_loss_reference, case, weight)
    got = run(prompt.memory_loss, case, weight)
    again = run(prompt.memory_loss, case, weight)
    assert (type(got[3]).__name__ == NATIVE) == case.native          # a declined shape takes the definition
    assert torch.equal(got[1], want[1]) and all(torch.equal(u, v) for u, v in zip(got[2], want[2]))
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and all(torch.equal(u, v) for u, v in zip(again[2], got[2]))
    x = case.x.to(DEV)
    target = prompt.substitute_reference(x, table_of(case), [v.to(DEV) for v in case.pool.values()])
    ok, err, bound = mcases.loss_bar_holds(got[0], want[0], x, target)
    print("%s: native %.9g reference %.9g error %.3g bound %.3g" % (case.name, float(got[0]), float(want[0]), err, bound))
    assert ok
    # the loop itself, from the masks
    loop = prompt.memory_loss_reference(x, (case.names_list, case.masks(DEV)), {k: v.to(DEV) for k, v in case.pool.items()})
    assert torch.equal(loop, want[0])
    if case.name == "empty_table":
        assert float(got[0]) == 0.0 and not bool(got[1].any())
    if case.name == "every_row":
        assert bool((got[1] != 0).any(-1).all())


@pytest.mark.parametrize("x_grad,pool_grad", [(True, False), (False, True), (True, True)])
def test_the_requires_grad_combinations(x_grad, pool_grad):
    case, weight = next(cw for cw in CASES if cw[0].name == "b2_t7_d12")
    want = run(prompt.memory_loss_reference, case, weight, x_grad, pool_grad)
    got = run(prompt.memory_loss, case, weight, x_grad, pool_grad)
    assert type(got[3]).__name__ == NATIVE and torch.equal(got[0], run(prompt.memory_loss, case, weight)[0])
    assert (got[1] is None and want[1] is None) if not x_grad else torch.equal(got[1], want[1])
    assert all(torch.equal(u, v) for u, v in zip(got[2], want[2]))
    assert pool_grad or not any(bool(g.any()) for g in got[2])


def test_the_switches_take_the_definition():
    case, weight = next(cw for cw in CASES if cw[0].name == "b2_t7_d12")
    assert type(run(prompt.memory_loss, case, weight)[3]).__name__ == NATIVE
    try:
        prompt.FORCE_REFERENCE = True
        assert type(run(prompt.memory_loss, case, weight)[3]).__name__ != NATIVE
        prompt.FORCE_REFERENCE = False
        Switches.native_prompt_memory = False
        assert type(run(prompt.memory_loss, case, weight)[3]).__name__ != NATIVE
    finally:
        prompt.FORCE_REFERENCE, Switches.native_prompt_memory = False, True
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert type(run(prompt.memory_loss, case, weight)[3]).__name__ != NATIVE


@pytest.mark.parametrize("name", ["b2_t7_d12", "b64_t256_d4"])
def test_graph_capture_replays_the_eager_bits(name):
    """forward + backward captured once and replayed three times: every replay gives the eager call's bits, so the last block
    has left the ticket at zero (no memset node clears it: the workspace is the table's, allocated before the capture)"""
    case, weight = next(cw for cw in CASES if cw[0].name == name)
    table = table_of(case)
    eager = run(prompt.memory_loss, case, 1.0)
    x = case.x.to(DEV).requires_grad_(True)
    pool = [v.to(DEV).requires_grad_(True) for v in case.pool.values()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up: tables and workspace exist before the capture
        torch.autograd.grad(prompt.memory_loss(x, table, pool), [x] + pool)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = prompt.memory_loss(x, table, pool)
        grads = torch.autograd.grad(loss, [x] + pool)
    for _ in range(3):
        loss.fill_(-1.0)
        for g in grads:
            g.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager[0]) and torch.equal(grads[0], eager[1])
        assert all(torch.equal(u, v) for u, v in zip(grads[1:], eager[2]))
    assert torch.equal(run(prompt.memory_loss, case, 1.0)[0], eager[0])          # and an eager call behind the replays


def test_the_model_hands_the_loss_over_on_both_routes():
    model = mcases.small_model(DEV).train()
    model.add_cls_prompt(["cat", "polar bear"])
    model.before_train()           # backbone and BERT frozen: the front end can be prefetched
    assert all(p.is_cuda and not p.requires_grad for p in model.prompt_memory_pool.values())
    with torch.no_grad():
        for p in model.prompt_memory_pool.values():
            p.add_(0.25)
    data = cases.batch([["cat", "owl"], ["polar bear", "cat"]], 224, 320, device=DEV, boxes_per_image=3)
    direct = model(data)
    assert float(direct["loss_prompt_memory"].detach()) > 0
    assert model.can_prefetch_frontend()
    handle = model.prefetch_frontend(data)
    routed = model(data, frontend=handle)
    assert torch.equal(routed["loss_prompt_memory"], direct["loss_prompt_memory"])
    captions, names_list = model._captions(data)
    try:
        prompt.FORCE_REFERENCE = True
        text_dict, cate_list, _ = model.encode_text(captions, DEV, names_list=names_list)
    finally:
        prompt.FORCE_REFERENCE = False
    x, keys = text_dict["encoded_text"].detach(), list(model.prompt_memory_pool.keys())
    table = prompt.build_table(names_list, cate_list, keys, [model.prompt_memory_pool[k].shape[0] for k in keys], x.shape[1])
    target = prompt.substitute_reference(x, table, [model.prompt_memory_pool[k].detach() for k in keys])
    ok, err, bound = mcases.loss_bar_holds(direct["loss_prompt_memory"].detach(), text_dict["loss_prompt_memory"].detach(), x, target)
    print("model: native %.9g reference %.9g error %.3g bound %.3g"
          % (float(direct["loss_prompt_memory"].detach()), float(text_dict["loss_prompt_memory"].detach()), err, bound))
    assert ok
    # one replay iteration through the trainer moves the side branch and leaves the memory alone
    from ziragroundingdino_amd.train import MemoryReplayer

    stored = {k: v.detach().clone() for k, v in model.prompt_memory_pool.items()}
    trainer = MemoryReplayer(model)
    before = model.rep_linear_adapter.bias.detach().clone()
    first = trainer.run_step()
    second = trainer.run_step()
    trainer._check_bucket()
    assert float(second["loss_prompt_memory"]) < float(first["loss_prompt_memory"])
    assert not torch.equal(model.rep_linear_adapter.bias.detach(), before)
    assert all(torch.equal(model.prompt_memory_pool[k].detach(), v) for k, v in stored.items())
