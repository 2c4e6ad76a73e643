"""The prompt-tuning baseline (``use_prompt_tuning``) without a GPU: ``add_cls_prompt`` and the substitution equal the
reference's sibling class bit for bit (tests/golden/mod_prompt_tuning.pt), ``build_table`` is a brute-force walk of the masks,
the switch off changes nothing, and with the switch on the pool is created, trained, saved and loaded through the model, the
trainer and the task chain."""
import os

import pytest
import torch

from conftest import ROOT

import prompt_cases as cases

from ziragroundingdino_amd import _lib, prompt
from ziragroundingdino_amd import build as zbuild

CASES = cases.cases()


def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "mod_prompt_tuning.pt"), weights_only=True)


def golden_model(g):
    """the small model with the fixture's text side: the grid-valued encoder stand-in and the fixture's feat_map"""
    model = cases.small_model("cpu", use_cet=False, use_zero_inter_loss=False).eval()
    model.bert = cases.GridBert()
    model.feat_map.load_state_dict(g["feat_map"])
    return model


def test_add_cls_prompt_equals_the_reference_s_bit_for_bit():
    g = golden()
    model = golden_model(g)
    model.add_cls_prompt(list(g["classes"]))
    assert list(model.prompt_memory_pool.keys()) == list(g["pool_initial"]) == ["-%s-" % c for c in cases.GOLDEN_CLASSES]
    for k, want in g["pool_initial"].items():
        got = model.prompt_memory_pool[k]
        assert got.shape == want.shape and got.dim() == 2 and got.shape[1] == 256 and torch.equal(got.detach(), want), k
    assert [len(v) for v in g["pool_initial"].values()] == [1, 3, 2, 2]
    assert model.learned_classes == list(g["classes"])
    # entries that exist are kept
    with torch.no_grad():
        model.prompt_memory_pool["-cat-"].add_(1.0)
    model.add_cls_prompt(["cat", "owl"])
    assert torch.equal(model.prompt_memory_pool["-cat-"].detach(), g["pool_initial"]["-cat-"] + 1.0)
    assert "-owl-" in model.prompt_memory_pool and model.learned_classes[-2:] == ["cat", "owl"]


def test_substitution_equals_the_reference_s_forward_bit_for_bit():
    g = golden()
    assert all(torch.equal(v * 256, torch.round(v * 256)) for v in list(g["pool_trained"].values()) + [g["upstream"]])
    assert torch.equal(g["encoded_text"] * 1024, torch.round(g["encoded_text"] * 1024))       # (products of 1/4 and 1/256)
    model = golden_model(g)
    model.load_state_dict({"prompt_memory_pool." + k: v for k, v in g["pool_trained"].items()}, strict=False)
    names_list = [c[:-1].split(".") for c in g["captions"]]
    text_dict, cate_list, _ = model.encode_text(list(g["captions"]), "cpu", names_list=names_list)
    assert torch.equal(text_dict["encoded_text"].detach(), g["encoded_text"]) and torch.equal(text_dict["text_token_mask"], g["text_token_mask"])
    assert not torch.equal(g["encoded_text"], g["unsubstituted"])
    # no category list (free text): nothing is substituted
    plain, _, _ = model.encode_text(list(g["captions"]), "cpu")
    assert torch.equal(plain["encoded_text"].detach(), g["unsubstituted"])
    # the pool's gradients, through the model's path and through the loop
    text_dict["encoded_text"].backward(g["upstream"])
    for k, p in model.prompt_memory_pool.items():
        if k in g["pool_grads"]:
            assert torch.equal(p.grad, g["pool_grads"][k]), k
        else:
            assert p.grad is None and k == "-sea otter-"
    pool = {k: v.clone().requires_grad_(True) for k, v in g["pool_trained"].items()}
    out = prompt.substitute_reference(g["unsubstituted"], (names_list, cate_list), pool)
    assert torch.equal(out.detach(), g["encoded_text"])
    out.backward(g["upstream"])
    assert all(torch.equal(pool[k].grad, v) for k, v in g["pool_grads"].items())


def table_of(case):
    keys = list(case.pool)
    return prompt.build_table(case.names_list, case.masks(), keys, [case.pool[k].shape[0] for k in keys], case.T)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_build_table_is_the_brute_force_walk(case):
    table, keys, where = table_of(case), list(case.pool), case.brute_force()
    assert table.seg_row.shape == (case.B, case.T, 2) and table.seg_row.dtype == torch.int32
    for b in range(case.B):
        for t in range(case.T):
            seg, row = table.seg_row[b, t].tolist()
            assert ((keys[seg], row) if seg >= 0 else None) == where.get((b, t)), (b, t)
            assert seg >= 0 or row == -1
    # the occurrence lists: per pool row the positions that hold it, ascending
    r = 0
    for s, k in enumerate(keys):
        for i in range(case.pool[k].shape[0]):
            want = sorted(b * case.T + t for (b, t), v in where.items() if v == (k, i))
            assert table.occ[table.occ_start[r]:table.occ_start[r + 1]].tolist() == want, (k, i)
            r += 1
    assert r == table.n_rows and int(table.occ_start[-1]) == table.n_occ == len(where)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
@pytest.mark.parametrize("x_grad", [False, True])
def test_reference_from_the_table_equals_the_loop(case, x_grad):
    outs = []
    for how in ("loop", "table"):
        x = case.x.clone().requires_grad_(x_grad)
        pool = {k: v.clone().requires_grad_(True) for k, v in case.pool.items()}
        arg = (case.names_list, case.masks()) if how == "loop" else table_of(case)
        out = prompt.substitute(x, arg, pool) if how == "table" else prompt.substitute_reference(x, arg, pool)
        out.backward(case.grad)
        outs.append((out.detach(), x.grad, {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in pool.items()}))
    (a, ga, pa), (b, gb, pb) = outs
    assert torch.equal(a, b) and all(torch.equal(pa[k], pb[k]) for k in pa)
    assert (ga is None and gb is None) if not x_grad else torch.equal(ga, gb)
    where = case.brute_force()
    for (bi, t), (k, i) in where.items():
        assert torch.equal(a[bi, t], case.pool[k][i])
    keep = torch.ones(case.B, case.T, dtype=torch.bool)
    for bi, t in where:
        keep[bi, t] = False
    assert torch.equal(a[keep], case.x[keep])
    if x_grad:
        assert torch.equal(ga[keep], case.grad[keep]) and not bool(ga[~keep].any())


def test_overlap_the_later_category_wins_and_both_raises():
    case = next(c for c in CASES if c.name == "overlap")
    table = table_of(case)
    assert table.seg_row[0].tolist() == [[-1, -1], [0, 0], [1, 0], [1, 1], [-1, -1]]
    pool = {k: v.clone().requires_grad_(True) for k, v in case.pool.items()}
    prompt.substitute_reference(case.x, table, pool).backward(case.grad)
    assert not bool(pool["-a-"].grad[1].any()) and torch.equal(pool["-a-"].grad[0], case.grad[0, 1])
    keys = list(case.pool)
    with pytest.raises(ValueError, match="tokens"):          # a class's token count differs from its entry's row count
        prompt.build_table(case.names_list, case.masks(), keys, [3, 2], case.T)
    with pytest.raises(ValueError, match="wide"):            # a mask wider than the encoded text
        prompt.build_table(case.names_list, case.masks(), keys, [2, 2], case.T - 1)


def test_an_over_long_class_raises():
    model = cases.small_model("cpu")
    names = ["w%d" % i for i in range(14)] + ["a b c d e"]      # 1 + 14 * 2 = 29 tokens, then 5 more: cut at max_text_len = 32
    with pytest.raises(ValueError, match="'a b c d e'"):
        model.add_cls_prompt(names)
    with pytest.raises(ValueError, match="'behind'"):
        model.add_cls_prompt(["w%d" % i for i in range(15)] + ["edge", "behind"])     # "edge" is token 31, "behind" token 33
    assert len(model.prompt_memory_pool) == 0                                         # nothing is created where a class raises
    model.add_cls_prompt(["w%d" % i for i in range(15)] + ["edge"])
    assert tuple(model.prompt_memory_pool["-edge-"].shape) == (1, 256)


def test_the_switch_off_changes_nothing():
    from test_model_gpu import small_model

    present, off = small_model(dev="cpu").eval(), cases.small_model("cpu", use_prompt_tuning=False).eval()
    assert list(off.state_dict()) == list(present.state_dict())
    off.add_cls_prompt(["cat", "dog"])
    assert [tuple(p.shape) for p in off.prompt_memory_pool.values()] == [(256,), (256,)]
    assert all(p.device.type == "cpu" for p in off.prompt_memory_pool.values()) and off.learned_classes == ["cat", "dog"]
    captions, names_list = ["cat.dog."] * 2, [["cat", "dog"]] * 2
    with torch.no_grad():
        a, _, _ = present.encode_text(captions, "cpu")
        b, _, _ = off.encode_text(captions, "cpu", names_list=names_list)
    assert torch.equal(a["encoded_text"], b["encoded_text"]) and not off._prompt_tables
    data = cases.batch([["cat", "dog"], ["cat", "dog"]])
    assert torch.equal(cases.pred_logits(present, data), cases.pred_logits(off, data))


def test_before_train_leaves_the_pool_and_the_adapters_trainable():
    model = cases.small_model("cpu")
    model.add_cls_prompt(["cat", "polar bear"])
    model.before_train()
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    pool = [n for n in trainable if "prompt_memory_pool" in n]
    assert pool == ["prompt_memory_pool.-cat-", "prompt_memory_pool.-polar bear-"]
    assert all("adapter" in n for n in trainable if n not in pool) and len(trainable) > len(pool)


def test_changing_one_entry_changes_the_logits_and_the_state_dict_round_trips():
    model = cases.small_model("cpu").eval()
    model.add_cls_prompt(["cat", "polar bear"])
    assert [tuple(p.shape) for p in model.prompt_memory_pool.values()] == [(1, 256), (2, 256)]
    data = cases.batch([["cat", "polar bear"], ["cat", "polar bear"]])
    before = cases.pred_logits(model, data)
    assert len(model._prompt_tables) == 1
    with torch.no_grad():
        model.prompt_memory_pool["-polar bear-"][1].add_(0.5)
    after = cases.pred_logits(model, data)
    assert len(model._prompt_tables) == 1                      # the cached table serves the changed values
    assert not torch.equal(before[..., 1], after[..., 1])
    # the free-text surface has no category list and does not substitute
    with torch.no_grad():
        g1 = model.forward_grounding(data)["pred_logits"]
        model.prompt_memory_pool["-polar bear-"][1].add_(0.5)
        g2 = model.forward_grounding(data)["pred_logits"]
    assert torch.equal(g1, g2)
    # the learned names that use_add_names appends at eval time get their prompts too
    model.use_add_names = True
    one = cases.batch([["cat"], ["cat"]])
    c1 = cases.pred_logits(model, one)
    with torch.no_grad():
        model.prompt_memory_pool["-polar bear-"][0].add_(0.5)
    assert not torch.equal(c1[..., 1], cases.pred_logits(model, one)[..., 1])
    # round trip
    fresh = cases.small_model("cpu").eval()
    fresh.load_state_dict(model.state_dict())
    assert all(torch.equal(fresh.prompt_memory_pool[k], v) and fresh.prompt_memory_pool[k].shape == v.shape
               for k, v in model.prompt_memory_pool.items())
    assert fresh.learned_classes == ["cat", "polar bear"]
    fresh.use_add_names = True
    assert torch.equal(cases.pred_logits(fresh, one), cases.pred_logits(model, one))
    # the chunked-vocabulary eval path substitutes as well
    model.use_add_names = False
    model.category_chunk_size = 1
    model._prompt_tables.clear()
    with torch.no_grad():
        model(data)
    assert sorted(key[1] for key in model._prompt_tables) == [(("cat",),) * 2, (("polar bear",),) * 2]     # one table per chunk


def test_run_tasks_trains_the_named_entries_and_the_next_task_loads_them(tmp_path):
    from ziragroundingdino_amd import tasks

    seen = {}

    def build():
        return cases.small_model("cpu", use_cet=False, use_zero_inter_loss=False)

    def on_step(spec, it, loss_dict):
        seen.setdefault(spec.name, []).append(it)

    names_a, names_b = ["cat", "polar bear", "owl"], ["red fox"]
    data_a = cases.batch([["cat", "polar bear"], ["cat", "polar bear"]])      # "owl" is a class of the task in no caption
    data_b = cases.batch([["red fox"], ["red fox"]])
    specs = [tasks.TaskSpec("a", names_a, lambda start: iter([data_a] * 4), 1, str(tmp_path / "a"), weight_decay=0.0,
                            model_ema=dict(decay=0.5)),
             tasks.TaskSpec("b", names_b, lambda start: iter([data_b] * 4), 1, str(tmp_path / "b"), weight_decay=0.0)]
    # the entries as they are created: one text pass of a fresh model
    fresh = build()
    fresh.add_cls_prompt(names_a)
    initial = {k: v.detach().clone() for k, v in fresh.prompt_memory_pool.items()}
    finals = tasks.run_tasks(specs, build, device="cpu", on_step=on_step)
    assert seen == {"a": [0], "b": [0]}
    ckpt = torch.load(finals[0], weights_only=False)
    saved = {k.split(".", 1)[1]: v for k, v in ckpt["model"].items() if k.startswith("prompt_memory_pool.")}
    assert list(saved) == ["-cat-", "-polar bear-", "-owl-"] and [tuple(v.shape) for v in saved.values()] == [(1, 256), (2, 256), (1, 256)]
    assert not torch.equal(saved["-cat-"], initial["-cat-"]) and not torch.equal(saved["-polar bear-"], initial["-polar bear-"])
    assert torch.equal(saved["-owl-"], initial["-owl-"])      # no gradient, and no weight decay in these specs: it stays
    # the model EMA holds the entries that existed before the first step
    assert all("prompt_memory_pool." + k in ckpt["ema_state"] for k in saved)
    second = torch.load(finals[1], weights_only=False)["model"]
    assert all(torch.equal(second["prompt_memory_pool." + k], v) for k, v in saved.items())       # loaded, and not in task b's captions
    assert tuple(second["prompt_memory_pool.-red fox-"].shape) == (2, 256)


def test_trainer_sees_the_entries_and_keeps_them_in_the_bucket():
    from ziragroundingdino_amd.train import ZiraTrainer

    model = cases.small_model("cpu", use_cet=False, use_zero_inter_loss=False).train()
    model.add_cls_prompt(["cat", "polar bear", "owl"])
    trainer = ZiraTrainer(model)
    assert [n for n in trainer.names if "prompt_memory_pool" in n] == ["prompt_memory_pool.-cat-", "prompt_memory_pool.-polar bear-",
                                                                       "prompt_memory_pool.-owl-"]
    seen = {}
    trainer.on_reduced_grad = lambda flat: seen.update({n: p.grad.clone() for n, p in zip(trainer.names, trainer.params)})
    trainer.run_step(cases.batch([["cat", "polar bear"], ["cat", "polar bear"]]))
    trainer._check_bucket()
    assert float(seen["prompt_memory_pool.-cat-"].abs().max()) > 0 and float(seen["prompt_memory_pool.-polar bear-"].abs().max()) > 0
    assert not bool(seen["prompt_memory_pool.-owl-"].any())
    assert all(bool(torch.isfinite(g).all()) for g in seen.values())


def test_header_build_and_binding_agree():
    import ctypes
    import re

    text = open(os.path.join(ROOT, "include", "zira_prompt.h")).read()
    declared = re.findall(r"\b(zira_prompt_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert declared == list(_lib.PROMPT_SYMBOLS) == ["zira_prompt_supported", "zira_prompt_substitute_fwd_f32", "zira_prompt_substitute_bwd_f32"]
    assert os.path.join(ROOT, "include", "zira_prompt.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "prompt.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.PROMPT_PROTOTYPES["zira_prompt_substitute_fwd_f32"] == (i, [vp] * 3 + [i] * 4 + [vp] * 2)
    assert _lib.PROMPT_PROTOTYPES["zira_prompt_substitute_bwd_f32"] == (i, [vp] * 4 + [i] * 3 + [ll, i] + [vp] * 3)
    lib = _lib.load()
    for case in CASES:
        assert bool(lib.zira_prompt_supported(case.B, case.T, case.D, len(case.pool), 8)) == case.native, case.name
    for bad in ((0, 9, 256, 1, 1), (65, 9, 256, 1, 1), (2, 9, 256, 0, 1), (2, 9, 256, 4097, 1), (2, 9, 256, 1, 65537), (2, 9, 4100, 1, 1)):
        assert lib.zira_prompt_supported(*bad) == 0, bad
    # null pointers: -1, and nothing is launched (no GPU here)
    assert lib.zira_prompt_substitute_fwd_f32(None, None, None, 2, 9, 256, 1, None, None) == -1
    assert lib.zira_prompt_substitute_bwd_f32(None, None, None, None, 2, 9, 256, 8, 3, None, None, None) == -1
