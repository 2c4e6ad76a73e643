"""The prompt-tuning substitution on the GPU: the autograd node over csrc/prompt.hip equals ``substitute_reference`` bit for bit
(the cases' values sit on binary grids, so fp32 sums are exact in any order), twice over, under graph capture and replay with
new values, the switches take the op chain, and the small model trains its pool through ``ZiraTrainer``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import prompt_cases as cases  # noqa: E402

from ziragroundingdino_amd import prompt  # noqa: E402
from ziragroundingdino_amd.transformer import Switches  # noqa: E402

CASES = cases.cases()
DEV = "cuda"


def table_of(case):
    keys = list(case.pool)
    return prompt.build_table(case.names_list, case.masks(), keys, [case.pool[k].shape[0] for k in keys], case.T)


def run(fn, case, table, x_grad, values=None):
    x = (values or case).x.to(DEV).requires_grad_(x_grad)
    pool = [v.to(DEV).requires_grad_(True) for v in case.pool.values()]
    out = fn(x, table, pool)
    out.backward(case.grad.to(DEV))
    return out.detach(), x.grad, [p.grad if p.grad is not None else torch.zeros_like(p) for p in pool], out.grad_fn


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
@pytest.mark.parametrize("x_grad", [False, True])
def test_native_equals_the_reference_bit_for_bit(case, x_grad):
    table = table_of(case)
    want = run(prompt.substitute_reference, case, table, x_grad)
    got = run(prompt.substitute, case, table, x_grad)
    again = run(prompt.substitute, case, table, x_grad)
    assert (type(got[3]).__name__ == "_SubstituteNativeBackward") == case.native      # a declined shape falls back
    for a, b in ((got, want), (again, got)):
        assert torch.equal(a[0], b[0]) and all(torch.equal(u, v) for u, v in zip(a[2], b[2]))
        assert (a[1] is None and b[1] is None) if not x_grad else torch.equal(a[1], b[1])
    # and against the loop itself, from the masks
    x = case.x.to(DEV)
    loop = prompt.substitute_reference(x, (case.names_list, case.masks(DEV)), {k: v.to(DEV) for k, v in case.pool.items()})
    assert torch.equal(loop, got[0])


def test_the_switches_take_the_op_chain():
    case = next(c for c in CASES if c.name == "ragged")
    table = table_of(case)
    assert type(run(prompt.substitute, case, table, True)[3]).__name__ == "_SubstituteNativeBackward"
    try:
        prompt.FORCE_REFERENCE = True
        assert type(run(prompt.substitute, case, table, True)[3]).__name__ != "_SubstituteNativeBackward"
        prompt.FORCE_REFERENCE = False
        Switches.native_prompt = False
        assert type(run(prompt.substitute, case, table, True)[3]).__name__ != "_SubstituteNativeBackward"
    finally:
        prompt.FORCE_REFERENCE, Switches.native_prompt = False, True
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert type(run(prompt.substitute, case, table, True)[3]).__name__ != "_SubstituteNativeBackward"


@pytest.mark.parametrize("name", ["ragged", "three_images"])
@pytest.mark.parametrize("backward", [False, True])
def test_graph_capture_and_replay_on_new_values(name, backward):
    """the cached table needs no host read: forward (+ backward) is captured, the inputs are overwritten in place, and the
    replay equals the reference on the new values"""
    case = next(c for c in CASES if c.name == name)
    table = table_of(case)
    x = case.x.to(DEV).requires_grad_(backward)
    pool = [v.to(DEV).requires_grad_(backward) for v in case.pool.values()]
    g = case.grad.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up: the tables are uploaded outside the capture
        out = prompt.substitute(x, table, pool)
        if backward:
            torch.autograd.grad(out, [x] + pool, g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = prompt.substitute(x, table, pool)
        grads = torch.autograd.grad(out, [x] + pool, g) if backward else ()
    with torch.no_grad():
        x.copy_(case.x2.to(DEV))
        g.copy_(case.grad2.to(DEV))
        for p, v in zip(pool, case.pool2.values()):
            p.copy_(v.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    x_ref = case.x2.to(DEV).requires_grad_(True)
    pool_ref = [v.to(DEV).requires_grad_(True) for v in case.pool2.values()]
    want = prompt.substitute_reference(x_ref, table, pool_ref)
    assert torch.equal(out, want.detach())
    if backward:
        want_grads = torch.autograd.grad(want, [x_ref] + pool_ref, case.grad2.to(DEV), allow_unused=True)
        for a, b, ref in zip(grads, want_grads, [x_ref] + pool_ref):
            assert torch.equal(a, b if b is not None else torch.zeros_like(ref))


def test_small_model_trains_its_pool_through_the_trainer():
    from ziragroundingdino_amd.train import ZiraTrainer

    model = cases.small_model(DEV, use_cet=False, use_zero_inter_loss=False).train()
    model.add_cls_prompt(["cat", "polar bear", "owl"])
    assert all(p.is_cuda for p in model.prompt_memory_pool.values())
    trainer = ZiraTrainer(model)
    seen = {}
    trainer.on_reduced_grad = lambda flat: seen.update({n: p.grad.clone() for n, p in zip(trainer.names, trainer.params)})
    before = {k: v.detach().clone() for k, v in model.prompt_memory_pool.items()}
    data = cases.batch([["cat", "polar bear"], ["cat", "polar bear"]], 224, 320, device=DEV, boxes_per_image=3)
    trainer.run_step(data)
    trainer._check_bucket()
    assert all(bool(torch.isfinite(g).all()) for g in seen.values())
    assert float(seen["prompt_memory_pool.-cat-"].abs().max()) > 0 and float(seen["prompt_memory_pool.-polar bear-"].abs().max()) > 0
    assert not bool(seen["prompt_memory_pool.-owl-"].any())
    assert not torch.equal(model.prompt_memory_pool["-cat-"].detach(), before["-cat-"])
    trainer.run_step(data)               # the second step takes whatever graph the first one captured
    trainer._check_bucket()
    # eval mode with use_add_names: the appended names get their prompts -- change one entry, the logits of its column move
    model.eval()
    model.use_add_names = True
    one = cases.batch([["cat"], ["cat"]], 224, 320, device=DEV)
    first = cases.pred_logits(model, one)
    with torch.no_grad():
        model.prompt_memory_pool["-polar bear-"][0].add_(0.5)
    second = cases.pred_logits(model, one)
    assert not torch.equal(first[..., 1], second[..., 1])
