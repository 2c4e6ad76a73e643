"""The text-memory replay (``use_prompt_memory``) without a GPU: ``memory_loss_reference`` equals the reference's sibling class
(tests/golden/mod_prompt_memory.pt: gradients bit for bit, the loss to the project's bar), the model carries the loss with the
switch on and nothing with it off, the entries are frozen memory, eval substitutes under both switches only, ``replay_memory``
and a ``TaskSpec(replay=True)`` run, and the header, the build and the binding agree."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

import prompt_cases as cases
import prompt_memory_cases as mcases

from ziragroundingdino_amd import _lib, prompt, vocab
from ziragroundingdino_amd import build as zbuild

CASES = mcases.memory_cases()


def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "mod_prompt_memory.pt"), weights_only=True)


def golden_model(g, **kw):
    """the small model with the fixture's text side: the grid-valued encoder stand-in, the fixture's feat_map and pool, and a
    language side branch that adds exactly nothing (as the reference's zero-initialised ``Adapter`` does)"""
    model = mcases.small_model("cpu", **kw)
    model.bert = cases.GridBert()
    model.feat_map.load_state_dict(g["feat_map"])
    with torch.no_grad():
        model.rep_linear_adapter.weight.zero_()
        model.rep_linear_adapter.bias.zero_()
    model.load_state_dict({"prompt_memory_pool." + k: v for k, v in g["pool"].items()}, strict=False)
    return model


def table_of(case):
    keys = list(case.pool)
    return prompt.build_table(case.names_list, case.masks(), keys, [case.pool[k].shape[0] for k in keys], case.T)


def golden_masks(g):
    model = golden_model(g)
    _, cate_list, _ = model.encode_text(list(g["captions"]), "cpu")
    return [c[:-1].split(".") for c in g["captions"]], cate_list


@pytest.mark.parametrize("how", ["masks", "table"])
def test_reference_equals_the_fixture(how):
    g = golden()
    names_list, cate_list = golden_masks(g)
    x = g["encoded_text"].clone().requires_grad_(True)
    pool = {k: v.clone().requires_grad_(True) for k, v in g["pool"].items()}
    if how == "masks":
        loss = prompt.memory_loss_reference(x, (names_list, cate_list), pool)
    else:
        keys = list(pool)
        table = prompt.build_table(names_list, cate_list, keys, [pool[k].shape[0] for k in keys], x.shape[1])
        assert int(table.occ_start[1]) - int(table.occ_start[0]) == 2       # "cat": one pool row, two occurrences
        loss = prompt.memory_loss(x, table, pool)                            # (CPU tensors: the definition)
    loss.backward()
    assert torch.equal(x.grad, g["grad_encoded_text"])
    for k, p in pool.items():
        if k in g["grad_pool"]:
            assert torch.equal(p.grad, g["grad_pool"][k]), k
        else:
            assert k == "-sea otter-" and (p.grad is None or not bool(p.grad.any()))
    target = prompt.substitute_reference(g["encoded_text"], (names_list, cate_list), g["pool"])
    ok, err, bound = mcases.loss_bar_holds(loss.detach(), g["loss_prompt_memory"], g["encoded_text"], target)
    print("loss %.9g fixture %.9g error %.3g bound %.3g" % (float(loss.detach()), float(g["loss_prompt_memory"]), err, bound))
    assert ok


@pytest.mark.parametrize("case,weight", CASES, ids=[c.name for c, _ in CASES])
def test_reference_from_the_table_equals_the_loop(case, weight):
    outs = []
    for how in ("loop", "table"):
        x = case.x.clone().requires_grad_(True)
        pool = {k: v.clone().requires_grad_(True) for k, v in case.pool.items()}
        loss = prompt.memory_loss_reference(x, (case.names_list, case.masks()) if how == "loop" else table_of(case), pool)
        (loss * weight).backward()
        outs.append((loss.detach(), x.grad, [p.grad if p.grad is not None else torch.zeros_like(p) for p in pool.values()]))
    (la, ga, pa), (lb, gb, pb) = outs
    assert torch.equal(la, lb) and torch.equal(ga, gb) and all(torch.equal(u, v) for u, v in zip(pa, pb))
    where = case.brute_force()
    keep = torch.ones(case.B, case.T, dtype=torch.bool)
    for b, t in where:
        keep[b, t] = False
    assert not bool(ga[keep].any())
    if case.name == "empty_table":
        assert float(la) == 0.0 and not bool(ga.any())


def train_losses(model, names_per_image):
    model.train()
    return model(cases.batch(names_per_image))


def test_the_training_loss_dict_carries_the_memory_loss():
    model = mcases.small_model("cpu")
    model.add_cls_prompt(["cat", "polar bear"])
    with torch.no_grad():
        for p in model.prompt_memory_pool.values():
            p.add_(0.25)
    loss_dict = train_losses(model, [["cat", "owl"], ["polar bear", "cat"]])
    assert "loss_prompt_memory" in loss_dict and float(loss_dict["loss_prompt_memory"].detach()) > 0
    total = getattr(loss_dict, "total", None)
    assert total is not None
    torch.testing.assert_close(total.reshape(()), sum(v.reshape(()) for v in loss_dict.values()), rtol=1e-5, atol=1e-6)
    without = sum(v.reshape(()) for k, v in loss_dict.items() if k != "loss_prompt_memory")
    assert float(total.detach()) > float(without.detach())
    # the definition on the text the model encodes
    model.train()
    data = cases.batch([["cat", "owl"], ["polar bear", "cat"]])
    captions, names_list = model._captions(data)
    text_dict, cate_list, _ = model.encode_text(captions, "cpu", names_list=names_list)
    got = text_dict.pop("loss_prompt_memory")
    want = prompt.memory_loss_reference(text_dict["encoded_text"], (names_list, cate_list), dict(model.prompt_memory_pool.items()))
    assert torch.equal(got.detach(), want.detach()) and torch.equal(got.detach(), loss_dict["loss_prompt_memory"].detach())
    # the text side of the prefetched route (encode_text deferred, finished later) hands over the same loss
    finish, _ = model.encode_text(captions, "cpu", defer=True, hidden_only=True, **model._prompt_names(names_list))
    assert torch.equal(finish()[0]["loss_prompt_memory"].detach(), got.detach())
    # nothing learned yet: the key is there and zero
    fresh = mcases.small_model("cpu")
    first = train_losses(fresh, [["cat"], ["cat"]])
    assert float(first["loss_prompt_memory"].detach()) == 0.0
    # a learned class without an entry raises
    fresh.learned_classes.append("cat")
    with pytest.raises(KeyError, match="-cat-"):
        train_losses(fresh, [["cat"], ["cat"]])


def test_the_switch_off_changes_nothing():
    from test_model_gpu import small_model

    present, off = small_model(dev="cpu"), mcases.small_model("cpu", use_prompt_memory=False)
    assert list(off.state_dict()) == list(present.state_dict())
    off.add_cls_prompt(["cat", "dog"])
    assert [tuple(p.shape) for p in off.prompt_memory_pool.values()] == [(256,), (256,)]
    assert all(p.requires_grad for p in off.prompt_memory_pool.values())
    data = [["cat", "dog"], ["cat", "dog"]]
    a, b = train_losses(present, data), train_losses(off, data)
    assert list(a) == list(b) and "loss_prompt_memory" not in b
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert off._prompt_names([["cat"]]) == {} and not off._prompt_tables
    with pytest.raises(RuntimeError, match="use_prompt_memory"):
        off.replay_memory()


def test_add_cls_prompt_gives_frozen_rows_that_stay_out_of_the_bucket():
    from ziragroundingdino_amd.train import ZiraTrainer

    model = mcases.small_model("cpu", freeze_all=False).train()
    model.add_cls_prompt(["cat", "polar bear"])
    assert [tuple(p.shape) for p in model.prompt_memory_pool.values()] == [(1, 256), (2, 256)]
    assert not any(p.requires_grad for p in model.prompt_memory_pool.values())
    trainer = ZiraTrainer(model)
    assert not [n for n in trainer.names if "prompt_memory_pool" in n]
    groups = [p for grp in trainer.optimizer.param_groups for p in grp["params"]]
    assert not any(p is q for p in model.prompt_memory_pool.values() for q in groups)
    # loaded entries are memory as well, and a checkpoint written without the switch is refused with both switches named
    fresh = mcases.small_model("cpu")
    fresh.load_state_dict(model.state_dict())
    assert fresh.learned_classes == ["cat", "polar bear"] and not any(p.requires_grad for p in fresh.prompt_memory_pool.values())
    plain = mcases.small_model("cpu", use_prompt_memory=False)
    plain.add_cls_prompt(["cat"])
    fresh = mcases.small_model("cpu")
    fresh.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="prompt-memory"):
        train_losses(fresh, [["cat"], ["cat"]])


def test_eval_substitution_needs_both_switches():
    data = cases.batch([["cat", "polar bear"], ["cat", "polar bear"]])

    def moved(**kw):
        model = mcases.small_model("cpu", **kw).eval()
        model.use_prompt_tuning = False
        if not model.use_prompt_memory:        # row entries, made as the switch makes them
            model.use_prompt_memory = True
            model.add_cls_prompt(["cat", "polar bear"])
            model.use_prompt_memory = False
        else:
            model.add_cls_prompt(["cat", "polar bear"])
        before = cases.pred_logits(model, data)
        with torch.no_grad():
            model.prompt_memory_pool["-polar bear-"][1].add_(0.5)
        return not torch.equal(before, cases.pred_logits(model, data))

    assert moved(use_prompt_memory=True, use_prompt_memory_output=True)
    assert not moved(use_prompt_memory=True, use_prompt_memory_output=False)
    assert not moved(use_prompt_memory=False, use_prompt_memory_output=True)


def test_replay_memory_equals_the_fixture_and_the_definition():
    g = golden()
    model = golden_model(g).train()
    assert model.learned_classes == list(g["classes"])
    losses = model.replay_memory()
    assert list(losses) == ["loss_prompt_memory", "loss_linear_adapter"]
    names_list = [list(g["classes"])]
    text_dict, cate_list, _ = model.encode_text([vocab.caption_of(g["classes"])], "cpu")
    target = prompt.substitute_reference(text_dict["encoded_text"], (names_list, cate_list), g["pool"])
    ok, err, bound = mcases.loss_bar_holds(losses["loss_prompt_memory"].detach() * 2, g["replay"]["loss_prompt_memory"] * 2,
                                           text_dict["encoded_text"], target)
    print("replay %.9g fixture %.9g error %.3g bound %.3g"
          % (float(losses["loss_prompt_memory"].detach()), float(g["replay"]["loss_prompt_memory"]), err, bound))
    assert ok and float(losses["loss_linear_adapter"].detach()) == float(g["replay"]["loss_adapter_text"]) == 0.0
    # the frozen text encoder's states are kept: the second iteration does not run it
    calls = []
    model.bert.register_forward_hook(lambda *a: calls.append(1))
    again = model.replay_memory()
    assert not calls and torch.equal(again["loss_prompt_memory"].detach(), losses["loss_prompt_memory"].detach())
    # J = 2: a class list longer than max_text_len is replayed as a batch of two captions
    model = mcases.small_model("cpu").train()
    names = ["w%d" % i for i in range(20)]                      # 1 + 20 * 2 = 41 tokens > max_text_len = 32
    chunks = vocab.split_categories(names, model.tokenizer, model.max_text_len)
    assert len(chunks) == 2
    for chunk in chunks:                                         # (entries are taken caption by caption)
        model.add_cls_prompt(list(chunk))
    with torch.no_grad():
        for p in model.prompt_memory_pool.values():
            p.add_(0.125)
    losses = model.replay_memory()
    captions = [vocab.caption_of(c) for c in chunks]
    text_dict, cate_list, _ = model.encode_text(captions, "cpu")
    assert text_dict["encoded_text"].shape[0] == 2
    want = prompt.memory_loss_reference(text_dict["encoded_text"], ([list(c) for c in chunks], cate_list),
                                        dict(model.prompt_memory_pool.items()))
    assert torch.equal(losses["loss_prompt_memory"].detach(), want.detach() * 0.5) and float(want.detach()) > 0
    # the zero-interference term: the side branch's own (not zero here), times loss_adapter_weight
    _, _, zero_loss = model.encode_text(captions, "cpu")
    assert float(zero_loss.detach()) > 0 and model.loss_adapter_weight == 0.1
    assert torch.equal(losses["loss_linear_adapter"].detach(), (zero_loss.reshape(()) * model.loss_adapter_weight).detach())
    # a trainable text encoder's states are not kept; a frozen one's are, until weights are loaded
    assert model._replay_cache is not None and model._replay_cache[3] is None
    model.before_train()
    frozen = model.replay_memory()
    assert model._replay_cache[3] is not None and torch.equal(frozen["loss_prompt_memory"].detach(), losses["loss_prompt_memory"].detach())
    model.load_state_dict(model.state_dict())
    assert model._replay_cache is None
    # errors
    empty = mcases.small_model("cpu").train()
    with pytest.raises(RuntimeError, match="empty"):
        empty.replay_memory()
    empty.learned_classes.append("cat")
    with pytest.raises(KeyError, match="cat"):
        empty.replay_memory()


def test_the_replayer_trains_the_text_side_only():
    from ziragroundingdino_amd.train import MemoryReplayer, ZiraTrainer

    model = mcases.small_model("cpu").train()
    model.add_cls_prompt(["cat", "polar bear"])
    with torch.no_grad():
        for p in model.prompt_memory_pool.values():
            p.add_(0.25)
    everything = ZiraTrainer(model).names
    trainer = MemoryReplayer(model, weight_decay=0.1)
    assert trainer.names and all(n.startswith("rep_linear_adapter.") for n in trainer.names)
    assert [n for n in everything if n.startswith("rep_linear_adapter.")] == trainer.names and len(everything) > len(trainer.names)
    others = {n: p.detach().clone() for n, p in model.named_parameters() if n not in trainer.names}
    before = {n: p.detach().clone() for n, p in zip(trainer.names, trainer.params)}
    trainer.run_step()
    trainer._check_bucket()
    assert all(torch.equal(p.detach(), others[n]) for n, p in model.named_parameters() if n in others)      # no decay, no step
    assert any(not torch.equal(p.detach(), before[n]) for n, p in zip(trainer.names, trainer.params))


def test_a_replay_task_lowers_the_loss_and_leaves_merged_branches(tmp_path):
    from ziragroundingdino_amd import rsb, tasks

    def build():
        return mcases.small_model("cpu")

    model = build()
    model.add_cls_prompt(["cat", "polar bear", "owl"])
    with torch.no_grad():
        for p in model.prompt_memory_pool.values():
            p.add_(0.25)
    stored = {k: v.detach().clone() for k, v in model.prompt_memory_pool.items()}
    init = str(tmp_path / "init.pth")
    torch.save({"model": model.state_dict()}, init)
    seen = []

    def data(start):
        raise AssertionError("a replay task builds no loader")

    spec = tasks.TaskSpec("replay", [], data, 3, str(tmp_path / "replay"), replay=True, weight_decay=0.0)
    final = tasks.run_task(spec, build, init, device="cpu", on_step=lambda s, it, losses: seen.append(float(losses["loss_prompt_memory"])))
    print("loss_prompt_memory per iteration:", seen)
    assert len(seen) == 3 and seen[-1] < seen[0]
    saved = torch.load(final, weights_only=False)["model"]
    assert all(torch.equal(saved["prompt_memory_pool." + k], v) for k, v in stored.items())       # memory is not trained
    # merged: the branch is back at its initialisation and its twin holds what was learned
    assert bool((saved["rep_linear_adapter.weight"] == rsb.zero_value).all())
    assert not torch.equal(saved["rep_linear_adapter.freeze_linear.weight"], model.state_dict()["rep_linear_adapter.freeze_linear.weight"])


def test_header_build_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "zira_prompt_memory.h")).read()
    declared = re.findall(r"\b(zira_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert declared == list(_lib.PMEM_SYMBOLS) == ["zira_pmem_supported", "zira_pmem_workspace_bytes", "zira_pmem_loss_fwd_f32",
                                                   "zira_pmem_loss_bwd_f32"]
    assert os.path.join(ROOT, "include", "zira_prompt_memory.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "prompt_memory.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.PMEM_PROTOTYPES["zira_pmem_workspace_bytes"] == (ctypes.c_size_t, [i, i])
    assert _lib.PMEM_PROTOTYPES["zira_pmem_loss_fwd_f32"] == (i, [vp] * 3 + [i] * 4 + [vp] * 3)
    assert _lib.PMEM_PROTOTYPES["zira_pmem_loss_bwd_f32"] == (i, [vp] * 6 + [i] * 4 + [ll, i] + [vp] * 3)
    lib = _lib.load()
    for case, _ in CASES:
        assert bool(lib.zira_pmem_supported(case.B, case.T, case.D, len(case.pool), 8)) == case.native, case.name
    for bad in ((0, 9, 256, 1, 1), (65, 9, 256, 1, 1), (2, 9, 256, 0, 1), (2, 9, 256, 1, 65537), (2, 9, 4100, 1, 1), (2, 257, 8, 1, 1)):
        assert lib.zira_pmem_supported(*bad) == 0, bad
    assert lib.zira_pmem_workspace_bytes(2, 9) == 16 + 8 * 5 and lib.zira_pmem_workspace_bytes(64, 256) == 16 + 8 * 4096
    assert lib.zira_pmem_workspace_bytes(65, 9) == 0 and lib.zira_pmem_workspace_bytes(2, 257) == 0
    # null pointers: -1, and nothing is launched (no GPU here)
    assert lib.zira_pmem_loss_fwd_f32(None, None, None, 2, 9, 256, 1, None, None, None) == -1
    assert lib.zira_pmem_loss_bwd_f32(None, None, None, None, None, None, 2, 9, 256, 1, 8, 3, None, None, None) == -1
