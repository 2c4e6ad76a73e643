"""The grounding tail without a GPU (ziragroundingdino_amd/grounding.py): the op-chain twin ``ground_reference`` byte for byte
against a numpy restatement of the contract in include/zira_msda.h (loops, no torch), the phrase decoding against the
reference's own strings (tests/golden/grounding_phrases.json, written by gen_grounding_golden.py), the limits of the C entry,
and the model surface ``forward_features(token_logits=True)`` / ``forward_grounding`` on the CPU slice model."""
import json
import os

import numpy as np
import pytest
import torch

import grounding_cases as gc
from conftest import GOLDEN
from test_modules_golden import msda_backend  # noqa: F401
from test_train_step import build_slice_model, slice_inputs

from ziragroundingdino_amd import _lib, grounding
from ziragroundingdino_amd import transformer as zt
from ziragroundingdino_amd.utils import recover_to_cls_logits


# ---- the contract, restated ------------------------------------------------------------------------------------------------
def _rows(prob, text_thr):
    """Per (b, q): (score or None for a row with a NaN, first index of the maximum, mask words) -- plain Python on the fp32
    values (a float32 is exact as a Python float, so ``>`` on them is the fp32 comparison)."""
    B, Q, T = prob.shape
    W = (T + 31) // 32
    out = []
    for b in range(B):
        img = []
        for q in range(Q):
            best, arg, nan, words = None, 0, False, [0] * W
            for t, x in enumerate(prob[b, q].tolist()):
                if x != x:
                    nan = True
                    continue
                if best is None or x > best:
                    best, arg = x, t
                if x > text_thr:
                    words[t >> 5] |= 1 << (t & 31)
            img.append((None if nan else best, arg, words))
        out.append(img)
    return out


def numpy_ground(prob, boxes, box_threshold, text_threshold, order, rows=None):
    prob, boxes = np.asarray(prob, dtype=np.float32), np.asarray(boxes, dtype=np.float32)
    B, Q, T = prob.shape
    W = (T + 31) // 32
    box_thr, text_thr = float(np.float32(box_threshold)), float(np.float32(text_threshold))
    rows = rows if rows is not None else _rows(prob, text_thr)
    query, score = np.zeros((B, Q), np.int32), np.zeros((B, Q), np.float32)
    box, arg = np.zeros((B, Q, 4), np.float32), np.zeros((B, Q), np.int32)
    bits, n_keep = np.zeros((B, Q, W), np.uint32), np.zeros((B,), np.int32)
    for b in range(B):
        kept = [q for q in range(Q) if rows[b][q][0] is not None and rows[b][q][0] > box_thr]
        if order == 1:
            kept = sorted(kept, key=lambda q: -rows[b][q][0])      # stable: equal scores stay in ascending q
        for p, q in enumerate(kept):
            query[b, p] = q
            score[b, p] = prob[b, q, rows[b][q][1]]                # the element itself: its bit pattern
            box[b, p] = boxes[b, q]
            arg[b, p] = rows[b][q][1]
            bits[b, p] = rows[b][q][2]
        n_keep[b] = len(kept)
    return query, score, box, arg, bits, n_keep


def assert_bytes_equal(got, want, what):
    """got: a ``Grounded`` of CPU tensors; want: the numpy tuple or another ``Grounded``."""
    for name, a, b in zip(grounding.Grounded._fields, got, want):
        a = a.numpy() if torch.is_tensor(a) else a
        b = b.numpy() if torch.is_tensor(b) else b
        assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("case", gc.all_cases(), ids=gc.case_id)
def test_reference_twin_equals_the_numpy_restatement(case):
    prob, boxes, box_thr, text_thr = gc.make(*case)
    rows = _rows(prob.numpy(), float(np.float32(text_thr)))
    for order in (0, 1):
        got = grounding.ground_reference(prob, boxes, box_thr, text_thr, order)
        want = numpy_ground(prob.numpy(), boxes.numpy(), box_thr, text_thr, order, rows)
        assert_bytes_equal(got, want, "order %d" % order)
        assert got.query.dtype == torch.int32 and got.argmax_token.dtype == torch.int32 and got.n_keep.dtype == torch.int32
        assert got.score.dtype == torch.float32 and got.box.dtype == torch.float32 and got.token_bits.dtype == torch.int32
    kind, B, Q, _ = case
    n = want[5]
    if kind == "none":
        assert not n.any() and not any(np.asarray(w).any() for w in want)
    elif kind == "all":
        assert (n == Q).all()
    elif kind in ("sparse", "at_threshold", "nan", "ties8") and Q >= 63:
        assert (n > 0).all() and (n < Q).all()                    # some kept, some dropped


def test_cases_cover_what_they_are_for():
    """The inputs hold the situations their names promise (a case that lost its edge would pass for nothing)."""
    for B, Q, T in gc.VALUE_SHAPES:
        prob, _, box_thr, text_thr = gc.make("at_threshold", B, Q, T)
        assert (prob.max(dim=2).values == np.float32(box_thr)).any() and (prob == np.float32(text_thr)).any()
        prob, _, box_thr, _ = gc.make("ties8", B, Q, T)
        s = prob.max(dim=2).values
        assert prob.unique().numel() <= 8 and all(int((s[b] > box_thr).sum()) > s[b][s[b] > box_thr].unique().numel() for b in range(B))
        prob, _, _, _ = gc.make("double_max", B, Q, T)
        assert ((prob == prob.max(dim=2, keepdim=True).values).sum(dim=2) >= 2).any()
        prob, _, _, _ = gc.make("nan", B, Q, T)
        assert prob[:, :, 0].isnan().any() and prob[:, :, T // 2].isnan().any() and prob[:, :, T - 1].isnan().any()
        prob, _, _, _ = gc.make("denormal", B, Q, T)
        assert ((prob > 0) & (prob < 1.1754944e-38)).any()
    got = grounding.ground_reference(*gc.make("ties8", 3, 65, 33), order=1)
    for b in range(3):                                            # descending scores, ascending q inside a tie
        n = int(got.n_keep[b])
        s, q = got.score[b, :n], got.query[b, :n]
        assert bool((s[:-1] >= s[1:]).all()) and bool((q[:-1] < q[1:])[s[:-1] == s[1:]].all()) and bool((s[:-1] == s[1:]).any())
    sparse = grounding.ground_reference(*gc.make("sparse", 1, 900, 256), order=0)
    n = int(sparse.n_keep[0])
    assert int(sparse.query[0, 0]) == 0 and int(sparse.query[0, n - 1]) == 899 and 0.03 < n / 900 < 0.08


def test_twin_rejects_what_is_not_a_grounding_input():
    prob, boxes = torch.rand(2, 5, 9), torch.rand(2, 5, 4)
    with pytest.raises(ValueError):
        grounding.ground_reference(prob, boxes[:, :4], 0.3, 0.2)
    with pytest.raises(ValueError):
        grounding.ground_reference(prob.double(), boxes, 0.3, 0.2)
    with pytest.raises(ValueError):
        grounding.ground(prob, boxes, 0.3, 0.2, order=2)
    assert_bytes_equal(grounding.ground(prob, boxes, 0.3, 0.2), grounding.ground_reference(prob, boxes, 0.3, 0.2), "CPU tensors")


# ---- strings -----------------------------------------------------------------------------------------------------------------
def _fixture():
    with open(os.path.join(GOLDEN, "grounding_phrases.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", _fixture()["phrases"], ids=lambda c: c["name"].replace(" ", "_"))
def test_phrases_from_bits_gives_the_reference_string(case):
    tokenized = grounding.WordTable(case["token_to_word"])
    assert grounding.phrases_from_bits(case["token_bits"], tokenized, case["caption"]) == case["phrase"]
    # the same words as the int32 tensor ``ground`` returns (bit 31 set = a negative word)
    words = torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in case["token_bits"]], dtype=torch.int32)
    assert grounding.phrases_from_bits(words, tokenized, case["caption"]) == case["phrase"]
    # ... and from the twin's own mask of a row that holds exactly these tokens
    row = torch.zeros(1, 1, 256)
    row[0, 0, case["tokens"]] = 0.9
    if case["tokens"]:
        g = grounding.ground_reference(row, torch.zeros(1, 1, 4), 0.5, 0.5)
        assert int(g.n_keep[0]) == 1
        assert grounding.phrases_from_bits(g.token_bits[0, 0], tokenized, case["caption"]) == case["phrase"]


def test_fixture_holds_the_cases_it_is_for():
    cases = {c["name"]: c for c in _fixture()["phrases"]}
    assert cases["special tokens only"]["phrase"] == "" and cases["special tokens only"]["tokens"]
    assert cases["one word"]["phrase"].strip() == "cat"
    assert len(cases["words of two categories"]["phrase"].split()) >= 2
    assert len(set(cases["a word in several tokens, all set"]["token_to_word"][1:4])) == 1
    assert 255 in cases["token 255"]["tokens"] and cases["token 255"]["phrase"]


def test_preprocess_caption_gives_the_reference_string():
    for c in _fixture()["captions"]:
        assert grounding.preprocess_caption(c["raw"]) == c["preprocessed"]


def test_simple_tokenizer_gets_a_word_table():
    """bert.SimpleTokenizer returns ids only: one token per word between [CLS] and [SEP], "." a word of its own."""
    from ziragroundingdino_amd.bert import SimpleTokenizer

    tok = grounding.tokenize_caption(SimpleTokenizer(), "red fish . crab.")
    assert tok.table == [None, 0, 1, 2, 3, 4, None]
    assert tok.token_to_word(6) is None and tok.token_to_word(255) is None
    before = SimpleTokenizer()(["red fish . crab."])
    assert before["input_ids"].shape == (1, 7) and not hasattr(before, "token_to_word")   # bert.py itself is as it was


# ---- limits ------------------------------------------------------------------------------------------------------------------
def test_workspace_query_and_supported_agree_on_the_limits():
    lib = _lib.load()
    inside = [(1, 1, 1), (65535, 1024, 256), (2, 900, 256)]
    outside = [(0, 900, 256), (65536, 900, 256), (2, 0, 256), (2, 1025, 256), (2, 900, 0), (2, 900, 257), (-1, 900, 256)]
    for B, Q, T in inside:
        assert lib.zira_ground_workspace_bytes(B, Q, T) > 0 and grounding._limits(B, Q, T)
    for B, Q, T in outside:
        assert lib.zira_ground_workspace_bytes(B, Q, T) == 0 and not grounding._limits(B, Q, T)
    assert (grounding.MAX_B, grounding.MAX_Q, grounding.MAX_T) == (65535, 1024, 256)
    # supported() is the limits plus device, dtype and layout: CPU tensors are declined whatever their shape
    assert not grounding.supported(torch.rand(2, 9, 5), torch.rand(2, 9, 4))
    assert not grounding.supported(torch.rand(2, 9, 5, device="meta"), torch.rand(2, 9, 4, device="meta"))
    # the entry refuses before it launches: host pointers are never looked at
    for B, Q, T in outside:
        assert lib.zira_ground_f32(16, 16, B, Q, T, 0.3, 0.2, 0, 16, 16, 16, 16, 16, 16, 16, 256, None) == 1   # ZIRA_MSDA_EINVAL
    assert lib.zira_ground_f32(16, 16, 2, 900, 256, 0.3, 0.2, 2, 16, 16, 16, 16, 16, 16, 16, 256, None) == 1   # order


# ---- the model surface ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msda_backend", ["cpu"], indirect=True)
def test_token_logits_are_class_embed_of_the_last_decoder_layer(msda_backend):
    g = torch.load(os.path.join(GOLDEN, "eval_zira_slice.pt"), weights_only=False)
    model = build_slice_model(g, "cpu").eval()
    inp, feats, poss, am, pid, c2t = slice_inputs(g, model, "cpu")
    seen = {}
    hook = model.transformer.register_forward_hook(lambda mod, args, out: seen.update(hs=out[0], ref=out[1]))
    with torch.no_grad():
        text_dict, loss_lin = model.project_text(inp["bert_hidden"], torch.ones_like(inp["input_ids"]).bool(), pid, am)
        before = model.forward_features(feats, poss, inp["img_mask"], text_dict, c2t, loss_lin, None)      # keyword absent
        # (a text_dict serves one pass: the transformer leaves the fused text features in it)
        text_dict, loss_lin = model.project_text(inp["bert_hidden"], torch.ones_like(inp["input_ids"]).bool(), pid, am)
        tok = model.forward_features(feats, poss, inp["img_mask"], text_dict, c2t, loss_lin, None, token_logits=True)
        by_hand = model.class_embed[-1](seen["hs"][-1], text_dict)
    hook.remove()
    assert set(tok) == {"pred_logits", "pred_boxes"}
    B, Q = before["pred_boxes"].shape[:2]
    assert tuple(tok["pred_logits"].shape) == (B, Q, model.max_text_len)
    assert torch.equal(tok["pred_logits"], by_hand)
    n_tok = inp["input_ids"].shape[1]
    assert torch.isinf(tok["pred_logits"][..., n_tok:]).all() and (tok["pred_logits"][..., n_tok:] < 0).all()
    assert torch.isfinite(tok["pred_logits"][..., :n_tok]).all()
    assert torch.equal(tok["pred_boxes"], before["pred_boxes"])
    # the default path is what it was: the golden values of the unchanged eval test, and the fold of these very token logits
    from test_modules_golden import close

    close(before["pred_logits"], g["pred_logits"], 1e-4, "pred_logits")
    close(before["pred_boxes"], g["pred_boxes"], 1e-4, "pred_boxes")
    assert torch.equal(before["pred_logits"], recover_to_cls_logits(by_hand, c2t, for_fill=-100.0))
    assert "cate_to_token_mask_list" in before and "cate_to_token_mask_list" not in tok


def test_forward_grounding_is_forward_with_the_keyword(monkeypatch):
    """``forward_grounding`` shares ``forward``: the same front end, ``forward_features(token_logits=True)``, no postprocess;
    ``forward`` without the keyword still ends in ``postprocess``.  Eval mode only."""
    g = torch.load(os.path.join(GOLDEN, "eval_zira_slice.pt"), weights_only=False)
    model = build_slice_model(g, "cpu").eval()
    calls = []

    def fake_features(*a, **kw):
        calls.append(kw.get("token_logits", False))
        return {"pred_logits": torch.zeros(1, 2, 3), "pred_boxes": torch.zeros(1, 2, 4)}

    class _Samples:
        mask, device, no_padding = torch.zeros(1, 4, 4, dtype=torch.bool), torch.device("cpu"), False

    class _Images:
        image_sizes = [(4, 4)]

    monkeypatch.setattr(model, "forward_features", fake_features)
    monkeypatch.setattr(model, "_canvas_batch", lambda inputs: (_Images(), _Samples()))
    monkeypatch.setattr(model, "_canvas_sizes", ((4, 4),), raising=False)
    monkeypatch.setattr(model, "encode_text", lambda captions, device, defer=False: ((lambda: ({}, [], None)), []))
    monkeypatch.setattr(model, "run_backbone", lambda samples: ([], []))
    monkeypatch.setattr(model, "postprocess", lambda *a: "postprocessed")
    inputs = [{"captions": "cat . dog ."}]
    out = model.forward_grounding(inputs)
    assert calls == [True] and set(out) == {"pred_logits", "pred_boxes"}
    assert model.forward(inputs) == "postprocessed" and calls == [True, False]
    with pytest.raises(AssertionError):
        model.train().forward_grounding(inputs)
    assert zt.Switches.native_grounding is True
