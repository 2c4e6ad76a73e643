"""The trained class head's kernels (csrc/clslinear.hip, include/zira_clslinear.h) through ``utils._ClsLinearLogits`` on the MI355X.

Oracle: ``cls_linear_logits_reference`` in float64 on the same device.  Yardstick: the same definition in float32 on the same
inputs -- what the module runs with the switch off.  For the output and each of the three gradients

    max|native - fp64|  <=  2 * max|reference fp32 - fp64|  +  one fp32 ulp of the tensor's largest magnitude

both errors measured here (the bar of tests/test_adapter_gpu.py), and the ``for_fill`` positions are the same.  Every figure is
printed before it is asserted (``pytest -s``).

The inputs are drawn so that in the float64 run every category's best and second-best token logit are more than 1e-3 of the
logits' largest magnitude apart (rows are drawn in excess and those that keep the gap are used; asserted on the float64 values
of the inputs in use): an arg-max that flips between arithmetics would put a category's gradient on another token.  A condition
on the data, not a tolerance.

Shapes: a wave owns 32 rows of one image, so R = 37 (a partly filled second block), two images with ragged token and category
counts, an empty category, a category over every token, 256 tokens (eight panels of 32) with one category and with 128, Q = 1 (a
row per block), seven stacked sets, a non-contiguous x.
"""
import functools

import numpy as np
import pytest
import torch

import cls_linear_cases as cases

from ziragroundingdino_amd import transformer
from ziragroundingdino_amd import utils as zutils

pytestmark = pytest.mark.gpu

FILL = -100.0
GAP = 1e-3
NAMES = ["out", "grad x", "grad cls_linear.weight", "grad cls_linear.bias"]

# name: (leading dims, B, Q, T of the text, tokens that are real, max_text_len, category token lists per image)
SHAPES = {
    "rows37": ((), 1, 37, 5, (5,), 16, [[[1], [2, 3], [4]]]),
    "two_images": ((), 2, 5, 9, (5, 9), 16, [[[1], [2, 3], [4]], [[1, 2, 3, 4, 5, 6, 7, 8]]]),
    "empty_category": ((), 2, 5, 9, (5, 9), 16, [[[1], [], [3, 4]], [[2, 5]]]),
    "every_token": ((), 1, 33, 9, (9,), 16, [[list(range(9)), [3]]]),
    "t256_c1": ((), 1, 64, 256, (256,), 256, [[list(range(1, 255))]]),
    "t256_c128": ((), 1, 64, 256, (256,), 256, [[[2 * c, 2 * c + 1] for c in range(128)]]),
    "q1": ((), 2, 1, 9, (5, 9), 16, [[[1], [2, 3], [4]], [[1, 2, 3]]]),
    "stacked7": ((7,), 2, 5, 9, (5, 9), 16, [[[1], [2, 3], [4]], [[1, 2, 3]]]),
    "padded_token_in_mask": ((), 2, 5, 9, (4, 9), 16, [[[1], [2, 3], [4]], [[1, 2, 3]]]),      # image 0's category 2: a padded token only
}


def dev():
    return torch.device("cuda:0")


def ulp(t):
    return float(np.spacing(np.float32(float(t.detach().abs().max()))))


def within_bar(what, native, chain, ref):
    native, chain, ref = (t.detach().double().reshape(-1) for t in (native, chain, ref))
    assert torch.isfinite(native).all(), what
    err_c, err_n = float((chain - ref).abs().max()), float((native - ref).abs().max())
    bar = 2.0 * err_c + ulp(ref)
    print("%-44s native %.3e  reference fp32 %.3e  bar %.3e  (max|ref| %.3e)" % (what, err_n, err_c, bar, float(ref.abs().max())))
    assert err_n <= bar, "%s: native %.3e > bar %.3e (reference fp32 %.3e)" % (what, err_n, bar, err_c)
    return bar


def rows_with_gaps(x, w, b, td, masks):
    """[..., B, Q] bool, in float64: the rows whose every category has its best and second-best token logit more than GAP of
    the logits' largest magnitude apart"""
    z = torch.nn.functional.linear(x.double(), w.double(), b.double()) @ td["encoded_text"].double().transpose(-1, -2)
    scale = float(z.abs().max())
    ok = torch.ones(x.shape[:-1], dtype=torch.bool, device=x.device)
    for bid, m in enumerate(masks):
        valid = m & td["text_token_mask"][bid, :m.shape[1]]
        for c in range(m.shape[0]):
            if int(valid[c].sum()) < 2:
                continue
            top = z[..., bid, :, :m.shape[1]][..., valid[c]].topk(2, dim=-1)[0]
            ok[..., bid, :] &= (top[..., 0] - top[..., 1]) > GAP * scale
    return ok


def run(x, w, b, td, masks, go, T_out, dtype, native, x_grad=True):
    """the head's output and the gradients of sum(out * go) for x, W, b"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (x, w, b)]
    leaves[0].requires_grad_(x_grad)
    tdd = dict(td, encoded_text=td["encoded_text"].to(dtype))
    if native:
        out = zutils._ClsLinearLogits.apply(leaves[0], leaves[1], leaves[2], tdd["encoded_text"], tdd["text_token_mask"], masks, FILL, T_out)
    else:
        out = zutils.cls_linear_logits_reference(leaves[0], leaves[1], leaves[2], tdd, masks, FILL, T_out)
    grads = torch.autograd.grad((out * go.to(dtype)).sum(), leaves if x_grad else leaves[1:])
    return [out.detach()] + ([] if x_grad else [None]) + list(grads)


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs, the fp64 oracle and the fp32 reference: computed once, read by every test of the case.  Four times the rows are
    drawn and, per image and set, the first Q that keep the gap are taken (a row's logits do not depend on the other rows)."""
    lead, B, Q, T, n_valid, T_out, spans = SHAPES[name]
    n_tok = [max([t for s in sp for t in s] + [0]) + 1 for sp in spans]
    masks = cases.category_masks(spans, n_tok, dev())
    gen = torch.Generator().manual_seed(100 + list(SHAPES).index(name))
    drawn = torch.randn(*lead, B, 4 * Q, 256, generator=gen).to(dev())
    w = (torch.randn(256, 256, generator=gen) / 16).to(dev())
    b = (torch.randn(256, generator=gen) * 0.1).to(dev())
    td = cases.text_dict(torch.randn(B, T, 256, generator=gen).to(dev()), n_valid)
    go = torch.randn(*lead, B, Q, T_out, generator=gen).to(dev())
    ok = rows_with_gaps(drawn, w, b, td, masks).reshape(-1, 4 * Q)
    picked = [rows[keep][:Q] for rows, keep in zip(drawn.reshape(-1, 4 * Q, 256), ok)]
    assert all(p.shape[0] == Q for p in picked), name
    x = torch.stack(picked).reshape(*lead, B, Q, 256)
    # the condition, on the inputs the tests use (the scale is the kept rows' own: not larger than the drawn rows')
    assert bool(rows_with_gaps(x, w, b, td, masks).all()), name
    args = (x, w, b, td, masks, go, T_out)
    return args, run(*args, torch.float64, False), run(*args, torch.float32, False)


def check(name, got, chain, ref):
    assert got[0].shape == ref[0].shape and got[0].dtype == torch.float32
    assert torch.equal(got[0] == FILL, ref[0] == FILL), name + ": for_fill positions"
    assert not bool(torch.isinf(got[0]).any())
    for what, n, c, r in zip(NAMES, got, chain, ref):
        within_bar("%s %s" % (name, what), n, c, r)


@pytest.mark.parametrize("name", list(SHAPES))
def test_native_against_fp64(name):
    args, ref, chain = case(name)
    check(name, run(*args, torch.float32, True), chain, ref)
    lead, B, Q, T, n_valid, T_out, spans = SHAPES[name]
    for bid, sp in enumerate(spans):          # what lies beyond an image's categories, and its token-less ones
        assert bool((ref[0][..., bid, :, len(sp):] == FILL).all())
        for c, toks in enumerate(sp):
            assert bool((ref[0][..., bid, :, c] == FILL).all()) == (not [t for t in toks if t < n_valid[bid]]), (bid, c)


def test_minus_infinity_fill_sits_where_the_reference_puts_it():
    (x, w, b, td, masks, go, T_out), _, _ = case("empty_category")
    with torch.no_grad():
        got = zutils._ClsLinearLogits.apply(x, w, b, td["encoded_text"], td["text_token_mask"], masks, float("-inf"), T_out)
        want = zutils.cls_linear_logits_reference(x, w, b, td, masks, float("-inf"), T_out)
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)) and bool(torch.isneginf(got[0, :, 1]).all())


def test_non_contiguous_x():
    (x, w, b, td, masks, go, T_out), ref, chain = case("two_images")
    wide = torch.zeros(x.shape[:-1] + (512,), device=x.device)
    wide[..., ::2] = x
    xs = wide[..., ::2]
    assert not xs.is_contiguous() and torch.equal(xs, x)
    check("non-contiguous", run(xs, w, b, td, masks, go, T_out, torch.float32, True), chain, ref)


def test_exact_ties_go_to_the_lower_token():
    """two equal text rows inside one category: the arg table names the first, as zira_cat_logits_fwd_f32 does"""
    (x, w, b, td, masks, go, T_out), _, _ = case("two_images")
    text = td["encoded_text"].clone()
    text[1, 6] = text[1, 2]                                   # image 1's category covers tokens 1..8
    td = dict(td, encoded_text=text)
    xg = x.clone().requires_grad_(True)
    out = zutils._ClsLinearLogits.apply(xg, w, b, text, td["text_token_mask"], masks, FILL, T_out)
    arg = out.grad_fn.saved_tensors[3].view(2, 5, -1)
    z = torch.nn.functional.linear(x.double(), w.double(), b.double()) @ text.double().transpose(-1, -2)
    want = z[1, :, 1:9].max(dim=-1)[1] + 1                    # torch.max: the first of equal values
    tied = (want == 2)
    assert int(tied.sum()) >= 1, "no row of the case has its maximum on the duplicated token"
    assert int((arg[1, :, 0] == 6).sum()) == 0 and bool((arg[1, :, 0][tied] == 2).all())
    # the same rule through the existing kernel, on the token logits of the op chain
    mod_logits = (torch.nn.functional.linear(x, w, b) @ text.transpose(-1, -2))
    mod_logits = torch.nn.functional.pad(mod_logits.masked_fill(~td["text_token_mask"][:, None, :], float("-inf")), (0, T_out - 9),
                                         value=float("-inf")).requires_grad_(True)
    chain = zutils.recover_to_cls_logits(mod_logits, masks, FILL)
    chain_arg = chain.grad_fn.saved_tensors[0].view(2, 5, -1)
    assert torch.equal(chain_arg[1, :, 0][tied], arg[1, :, 0][tied])
    assert bool((arg[0, :, 1:3] >= 0).all()) and bool((arg[1, :, 1:] == -1).all())


def test_two_runs_give_the_same_bits():
    for name in ("stacked7", "t256_c128"):
        args, _, _ = case(name)
        a, b = run(*args, torch.float32, True), run(*args, torch.float32, True)
        for what, u, v in zip(NAMES, a, b):
            assert torch.equal(u, v), (name, what)


def test_graph_replay_gives_the_eager_bits():
    (x, w, b, td, masks, go, T_out), _, _ = case("stacked7")

    def fwd():
        with torch.no_grad():
            return zutils._ClsLinearLogits.apply(x, w, b, td["encoded_text"], td["text_token_mask"], masks, FILL, T_out)

    eager = fwd()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fwd()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = fwd()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager, captured)


def test_without_a_gradient_for_x_the_backward_skips_it():
    args, _, _ = case("two_images")
    full, lean = run(*args, torch.float32, True), run(*args, torch.float32, True, x_grad=False)
    assert lean[1] is None and torch.equal(full[0], lean[0])
    assert torch.equal(full[2], lean[2]) and torch.equal(full[3], lean[3])
    # and autograd hands the node's None on: a frozen x under the module
    (x, w, b, td, masks, go, T_out) = args
    mod = zutils.ContrastiveEmbedwithLinear(max_text_len=T_out).to(dev())
    out = mod.category_logits(x, td, masks, FILL)
    assert type(out.grad_fn).__name__.startswith("_ClsLinearLogits")
    (out * go).sum().backward()
    assert x.grad is None and mod.cls_linear.weight.grad is not None and mod.cls_linear.bias.grad is not None


@pytest.mark.parametrize("how", ["force", "switch", "half", "text_grad", "autocast", "cpu"])
def test_the_node_is_not_entered(monkeypatch, how):
    def never(*a, **k):
        raise AssertionError("the native node was entered")

    (x, w, b, td, masks, go, T_out), _, chain = case("two_images")
    mod = zutils.ContrastiveEmbedwithLinear(max_text_len=T_out).to(dev())
    with torch.no_grad():
        mod.cls_linear.weight.copy_(w)
        mod.cls_linear.bias.copy_(b)
    monkeypatch.setattr(zutils._ClsLinearLogits, "apply", never)
    if how == "force":
        monkeypatch.setattr(zutils, "FORCE_REFERENCE", True)
    elif how == "switch":
        monkeypatch.setattr(transformer.Switches, "native_cls_linear", False)
    if how in ("force", "switch"):
        assert torch.equal(mod.category_logits(x, td, masks, FILL), chain[0])
    elif how == "half":
        out = mod.half().category_logits(x.half(), dict(td, encoded_text=td["encoded_text"].half()), masks, FILL)
        assert out.dtype == torch.float16 and out.shape == chain[0].shape
    elif how == "text_grad":
        text = td["encoded_text"].clone().requires_grad_(True)
        out = mod.category_logits(x, dict(td, encoded_text=text), masks, FILL)
        (g,) = torch.autograd.grad((out * go).sum(), [text])
        assert float(g.abs().max()) > 0.0
    elif how == "autocast":
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert mod.category_logits(x, td, masks, FILL).shape == chain[0].shape
    else:
        cpu = mod.cpu().category_logits(x.cpu(), {k: v.cpu() for k, v in td.items()}, [m.cpu() for m in masks], FILL)
        assert cpu.shape == chain[0].shape
    if how in ("force", "switch"):
        monkeypatch.undo()
        ran = []
        monkeypatch.setattr(zutils._ClsLinearLogits, "apply",
                            lambda *a, _f=zutils._ClsLinearLogits.apply: (ran.append(tuple(a[0].shape)), _f(*a))[1])
        mod.category_logits(x, td, masks, FILL)
        assert ran == [tuple(x.shape)]


def test_model_with_the_switch_trains_one_step(monkeypatch):
    """The small model of tests/test_model_gpu.py as the reference's linear-probing config builds it (``use_cls_linear``, no side
    branches), two images: both heads' calls go through the native node -- the decoder's two layers stacked, the encoder's set
    through its own module -- the losses are finite, every ``cls_linear`` and ``bbox_embed`` parameter (the box MLP's zero last
    layer started from seeded noise: it would starve the two before it) receives a gradient and nothing else does, and the
    losses agree with ``FORCE_REFERENCE``'s.

    Bound on a loss's difference: the head's outputs differ by at most the forward bar `e` (checked here on the very tensors
    the model's calls received, against float64); the focal class loss is a sum over B * Q * max_text_len logits of terms whose
    slope is below 1, divided by a box count >= 1, so it moves by at most weight * B * Q * max_text_len * e; the box losses see
    the logits only through the matching and get the same allowance."""
    from ziragroundingdino_amd.train import synthetic_batch

    model = cases.small_model("cuda", use_cls_linear=True, use_cet=False, use_project_adapter=False).train()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "bbox_embed" in n and "layers.2" in n:
                p.copy_(torch.randn_like(p) * 0.05)
            if "cls_linear.weight" in n:
                p.add_(torch.eye(256, device=p.device))
    model.before_train()
    heads = {n: p for n, p in model.named_parameters() if "cls_linear" in n or "bbox_embed" in n}
    assert len(heads) == 4 + 12 and all(p.requires_grad for p in heads.values())
    assert [n for n, p in model.named_parameters() if p.requires_grad] == list(heads)
    data = synthetic_batch(2, 224, 320, n_categories=4, boxes_per_image=3, device="cuda")
    seen = []
    real = zutils._ClsLinearLogits.apply
    monkeypatch.setattr(zutils._ClsLinearLogits, "apply", lambda *a: (seen.append(a), real(*a))[1])
    losses = model(data)
    assert [tuple(a[0].shape) for a in seen] == [(2, 2, 50, 256), (2, 50, 256)]
    assert all(not a[0].requires_grad for a in seen)          # pure linear probing: no gradient for x, the launch skips it
    assert all(torch.isfinite(v).all() for v in losses.values())
    sum(v.sum() for v in losses.values()).backward()
    for n, p in model.named_parameters():
        if n in heads:
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0, n
        else:
            assert p.grad is None, n
    monkeypatch.undo()
    e = 0.0
    for a in seen:
        x, w, b, text, tmask, masks, fill, T_out = a
        td = {"encoded_text": text, "text_token_mask": tmask}
        with torch.no_grad():
            ref = zutils.cls_linear_logits_reference(x.double(), w.double(), b.double(), dict(td, encoded_text=text.double()), masks, fill, T_out)
            chain = zutils.cls_linear_logits_reference(x, w, b, td, masks, fill, T_out)
            got = real(x, w, b, text, tmask, masks, fill, T_out)
        assert torch.equal(got == fill, ref == fill)
        e = max(e, within_bar("model head %s" % (tuple(x.shape),), got, chain, ref))
    monkeypatch.setattr(zutils, "FORCE_REFERENCE", True)
    forced = model(data)
    weights = model.criterion.weight_dict
    assert set(forced) == set(losses)
    for k in losses:
        allow = weights.get(k, 1.0) * 2 * 50 * 32 * e
        diff = abs(float(losses[k].detach()) - float(forced[k].detach()))
        print("%-16s native %.6f  FORCE_REFERENCE %.6f  diff %.3e  allowance %.3e" % (k, float(losses[k].detach()), float(forced[k].detach()), diff, allow))
        assert diff <= allow, k
