"""Phrase grounding without a GPU: the C ABI of the matching is declared in include/zira_phrase.h, typed from that header into
tables of its own and exported by the built library; argument errors are answered on the host; ``match_reference`` against
phrase_oracle (plain loops, written independently) bit for bit; hand-worked cases; ``phrase_bits_from_spans`` around the word
size; ``PhraseGroundingEvaluator`` and ``inference_on_grounding_dataset`` on CPU state end to end."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import phrase_cases as cases
import phrase_oracle as oracle
from conftest import ROOT

from ziragroundingdino_amd import _lib
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd import phrase_evaluation as pe
from ziragroundingdino_amd.bert import SimpleTokenizer

ENTRIES = ["zira_phrase_match_lds_bytes", "zira_phrase_match_f32"]
EINVAL = 1


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_typed_and_exported():
    text = open(os.path.join(ROOT, "include", "zira_phrase.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(zira_[a-z0-9_]+)\s*\(", text)
    assert declared == ENTRIES == list(_lib.PHRASE_SYMBOLS) == list(_lib.PHRASE_PROTOTYPES)
    zbuild.build_extension()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ENTRIES:
        assert hasattr(raw, sym), "libzira_msda.so does not export %s" % sym
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    P = _lib.PHRASE_PROTOTYPES
    assert P["zira_phrase_match_lds_bytes"] == (sz, [i, i, i, i, i])
    assert P["zira_phrase_match_f32"] == (i, [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp, i, i, vp, vp, vp, vp, vp, vp])
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert _lib.PHRASE_CONSTANTS == {"ZIRA_PHRASE_MAX_B": 65535, "ZIRA_PHRASE_MAX_Q": 1024, "ZIRA_PHRASE_MAX_T": 256,
                                     "ZIRA_PHRASE_MAX_P": 256, "ZIRA_PHRASE_MAX_G": 64, "ZIRA_PHRASE_MAX_K": 32,
                                     "ZIRA_PHRASE_MAX_THRS": 10}
    assert (pe.MAX_B, pe.MAX_Q, pe.MAX_T, pe.MAX_P, pe.MAX_G, pe.MAX_K, pe.MAX_THRS) == (65535, 1024, 256, 256, 64, 32, 10)


def test_the_other_headers_surfaces_are_what_they_were():
    assert len(_lib.SYMBOLS) == 100 and not set(ENTRIES) & set(_lib.SYMBOLS)
    assert not any("PHRASE" in name or "LVIS" in name for name in _lib.CONSTANTS)
    assert len(_lib.NMS_SYMBOLS) == 2 and len(_lib.VOCAB_SYMBOLS) == 2
    assert list(_lib.LVIS_SYMBOLS) == ["zira_lvis_match_lds_bytes", "zira_lvis_match"]
    assert os.path.join(ROOT, "include", "zira_phrase.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "phrasematch.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    assert "-ffp-contract=off" in zbuild.EXTRA_FLAGS["phrasematch.hip"] and "topk.hip" not in zbuild.EXTRA_FLAGS


def _call(lib, B=2, Q=900, T=256, P=32, G=4, k_max=10, n_thr=1, merged=0, **ptr):
    """The entry on made-up addresses: an argument error is answered before any of them is looked at."""
    p = dict(prob=64, boxes=64, sizes=64, phrase_bits=64, gt_boxes=64, gt_count=64, top_query=64, top_score=64, top_iou=64,
             first_hit=64, valid=64)
    p.update(ptr)
    thrs = (ctypes.c_double * max(n_thr, 1))(*([0.5] * max(n_thr, 1)))
    return lib.zira_phrase_match_f32(p["prob"], p["boxes"], p["sizes"], p["phrase_bits"], p["gt_boxes"], p["gt_count"], B, Q, T, P,
                                     G, k_max, p.get("thrs", thrs), n_thr, merged, p["top_query"], p["top_score"], p["top_iou"],
                                     p["first_hit"], p["valid"], None)


def test_argument_errors_are_answered_on_the_host():
    """Nothing is launched: there is no device here, and the host pointers are never looked at."""
    lib = _lib.load()
    for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(Q=0), dict(Q=1025), dict(T=0), dict(T=257), dict(P=0), dict(P=257),
                dict(G=0), dict(G=65), dict(k_max=0), dict(k_max=33), dict(n_thr=0), dict(n_thr=11), dict(n_thr=-1)):
        assert _call(lib, **bad) == EINVAL, bad
    for null in ("prob", "boxes", "sizes", "phrase_bits", "gt_boxes", "gt_count", "thrs", "top_query", "top_score", "top_iou",
                 "first_hit", "valid"):
        assert _call(lib, **{null: None}) == EINVAL, null
    # the LDS the launch takes (host arithmetic): 16 G + 8 (the power of two at or above Q) + 4 Q + 4 k_max + 4 ceil(T / 32)
    assert lib.zira_phrase_match_lds_bytes(900, 256, 4, 10, 1) == 64 + 8192 + 3600 + 40 + 32
    assert lib.zira_phrase_match_lds_bytes(1024, 256, 64, 32, 10) == 1024 + 8192 + 4096 + 128 + 32 <= 48 * 1024
    assert lib.zira_phrase_match_lds_bytes(1, 1, 1, 1, 1) == 16 + 8 + 4 + 4 + 4
    for Q, T, G, K, N in ((0, 1, 1, 1, 1), (1025, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 257, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 65, 1, 1),
                          (1, 1, 1, 0, 1), (1, 1, 1, 33, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 11)):
        assert lib.zira_phrase_match_lds_bytes(Q, T, G, K, N) == 0, (Q, T, G, K, N)


# ---- the definition against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", (False, True))
@pytest.mark.parametrize("name", cases.names())
def test_match_reference_equals_the_oracle(name, merged):
    case = cases.get(name)
    got = cases.as_numpy(pe.match_reference(*cases.tensors(case), case["k_max"], case["iou_thrs"], merged))
    cases.assert_equal(got, cases.expected(name, merged), (name, merged))


def test_match_takes_the_reference_for_cpu_tensors():
    case = cases.get("q63_t31")
    args = cases.tensors(case)
    assert not pe.match_supported(*args, case["k_max"], case["iou_thrs"])
    got = cases.as_numpy(pe.match(*args, case["k_max"], case["iou_thrs"], False))
    cases.assert_equal(got, cases.expected("q63_t31", False), "match on CPU tensors")
    with pytest.raises(ValueError):
        pe.match_reference(args[0], args[1][:, :-1], *args[2:])


def test_the_cases_hold_what_they_are_for():
    """By the ORACLE's verdict on the inputs, never by the code under test."""
    assert {c[2] for c in cases.SHAPES} >= {1, 63, 64, 65, 257, 900, 1024} and {c[3] for c in cases.SHAPES} >= {1, 31, 32, 33, 195, 256}
    assert {c[4] for c in cases.SHAPES} >= {1, 3, 32} and {c[5] for c in cases.SHAPES} >= {1, 5, 64}
    assert {c[6] for c in cases.SHAPES} >= {1, 10, 32} and {len(c[7]) for c in cases.SHAPES} == {1, 10}
    assert any(c[6] > c[2] for c in cases.SHAPES)                                   # k_max > Q
    case, want = cases.get("q900_t256"), cases.expected("q900_t256", False)
    merged = cases.expected("q900_t256", True)
    assert np.isnan(want["top_score"][0, 0, 0]) and want["top_query"][0, 0, 0] == 1                     # the NaN inside the mask
    assert not np.isnan(want["top_score"][0, 1:]).any() and np.isnan(case["prob"][0, 2]).any()         # ... and the one outside
    assert want["valid"][0, 2] == 0 and (want["top_query"][0, 2] == -1).all() and (want["first_hit"][0, 2] == 10).all()
    assert want["valid"][1, 0] == 0 and want["valid"][1, 2] == 0 and want["valid"].sum() == 2 * 32 - 3
    live = want["valid"] != 0
    assert (np.diff(want["top_score"][live][:, 1:], axis=1) == 0).any(), "no tie among the candidates"
    assert 0 < (want["first_hit"][live] < 10).sum() < want["first_hit"][live].size                     # hits and misses
    assert (want["first_hit"][live][:, 0] > 0).any() and (want["first_hit"][live][:, 0] == 0).any()
    assert (want["first_hit"] != merged["first_hit"]).any() and (want["top_iou"] != merged["top_iou"]).any()
    assert (np.diff(want["first_hit"][live], axis=1) >= 0).all()                                       # a harder threshold hits later
    assert cases.expected("q1", False)["top_query"][0, 0].tolist() == [0] + [-1] * 9
    assert (cases.expected("q20_k32", False)["top_query"][0, 0, 20:] == -1).all()
    assert sorted(cases.expected("q20_k32", False)["top_query"][0, 0, :20].tolist()) == list(range(20))
    zero = cases.get("q63_t31")["gt_boxes"][0, 0, 0]
    assert zero[0] == zero[2]                                                                          # the zero-area GT box
    assert (cases.get("q63_t31")["prob"] == 0).any() and np.signbit(cases.get("q63_t31")["prob"]).any()   # -0.0 among the zeros


# ---- hand-worked cases: a 128 x 128 frame, one token, dyadic boxes, so every number below is exact --------------------------------
def _hand(scores, boxes, gts, k_max=10, iou_thrs=(0.5,), merged=False):
    prob = torch.tensor(scores, dtype=torch.float32).reshape(1, -1, 1)
    boxes = torch.tensor(boxes, dtype=torch.float32).reshape(1, -1, 4)
    gt = torch.tensor(gts, dtype=torch.float32).reshape(1, 1, -1, 4)
    args = (prob, boxes, torch.tensor([[128.0, 128.0]]), torch.tensor([[[1]]], dtype=torch.int32), gt,
            torch.tensor([[gt.shape[2]]], dtype=torch.int32))
    got = pe.match_reference(*args, k_max, iou_thrs, merged)
    want = oracle.match(*(a.numpy() for a in args), k_max, iou_thrs, merged)
    cases.assert_equal(cases.as_numpy(got), want, "hand-worked")
    return got


def test_hand_worked_a_hit_only_at_rank_3():
    small, big = [0.125, 0.125, 0.125, 0.125], [0.5, 0.5, 0.25, 0.25]           # [8, 8, 24, 24] and [48, 48, 80, 80]
    got = _hand([0.6, 0.9, 0.8, 0.7, 0.5], [big, small, small, small, small], [[200, 200, 210, 210], [48, 48, 80, 80]], k_max=5)
    assert got.top_query[0, 0].tolist() == [1, 2, 3, 0, 4]
    assert np.array_equal(got.top_score[0, 0].numpy(), np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32))
    assert got.top_iou[0, 0].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0]
    assert got.first_hit[0, 0].tolist() == [3] and got.valid[0, 0] == 1
    cut = _hand([0.6, 0.9, 0.8, 0.7, 0.5], [big, small, small, small, small], [[48, 48, 80, 80]], k_max=3)
    assert cut.first_hit[0, 0].tolist() == [3] and cut.top_iou[0, 0].tolist() == [0.0, 0.0, 0.0]   # three candidates: no hit is k_max


def test_hand_worked_merged_turns_a_hit_into_a_miss():
    corner = [0.125, 0.125, 0.25, 0.25]                                         # [0, 0, 32, 32]
    gts = [[0, 0, 32, 32], [96, 96, 128, 128]]
    any_box = _hand([0.5], [corner], gts)
    assert any_box.top_iou[0, 0, 0] == 1.0 and any_box.first_hit[0, 0].tolist() == [0]
    union = _hand([0.5], [corner], gts, merged=True)                            # the union is the frame: 1024 / 16384
    assert union.top_iou[0, 0, 0] == 0.0625 and union.first_hit[0, 0].tolist() == [10]


def test_hand_worked_an_iou_equal_to_the_threshold_is_a_hit():
    got = _hand([0.5], [[0.25, 0.25, 0.5, 0.5]], [[0, 0, 64, 128]], iou_thrs=(0.5, 0.5000000000000001))   # 4096 / 8192
    assert got.top_iou[0, 0, 0] == 0.5 and got.first_hit[0, 0].tolist() == [0, 10]


# ---- spans -> mask words -------------------------------------------------------------------------------------------------------
def test_phrase_bits_from_spans_around_the_word_size():
    tok = SimpleTokenizer()
    words = ["w%02d" % i for i in range(40)]                                    # token i + 1 is word i ([CLS] is token 0)
    caption = " ".join(words) + " ."
    tokenized = pe.tokenize_with_offsets(tok, caption)
    assert tokenized.offsets[0] is None and tokenized.offsets[-1] is None and len(tokenized.offsets) == 43
    assert [caption[b:e] for b, e in tokenized.offsets[1:-1]] == words + ["."]
    assert [tokenized.token_to_word(i) for i in (0, 1, 41, 42)] == [None, 0, 40, None]
    at = lambda i: (4 * i, 4 * i + 3)                                           # the characters of word i
    spans = [[at(30)], [at(31)], [at(32)], [at(30), at(32)], [(4 * 30 + 2, 4 * 31 + 1)], [(4 * 30 + 3, 4 * 30 + 4)], []]
    bits = pe.phrase_bits_from_spans(tokenized, spans)
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (7, 2)
    assert bits.tolist() == [[-2 ** 31, 0], [0, 1], [0, 2], [-2 ** 31, 2], [-2 ** 31, 1], [0, 0], [0, 0]]   # tokens 31 / 32 / 33; a cut token; a blank
    # the model's T: tokens at and behind it are dropped, and the word count follows it
    assert pe.phrase_bits_from_spans(tokenized, spans[:3], 32).tolist() == [[-2 ** 31], [0], [0]]
    assert tuple(pe.phrase_bits_from_spans(tokenized, spans[:3], 256).shape) == (3, 8)
    assert pe.phrase_bits_from_spans([None, (0, 3), (4, 5)], [[(2, 5)]]).tolist() == [[6]]               # plain ranges
    # the bits select the same tokens as the oracle reads
    assert oracle.phrase_tokens(bits[3].numpy(), 43) == [31, 33]


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------
class StubModel:
    """``forward_grounding`` from fixed tensors; the logits are the inverse sigmoid of the case's probabilities."""

    def __init__(self, case, tokenizer=None):
        self.training = True
        self.case = case
        self.calls = []
        self.tokenizer = tokenizer

    def eval(self):
        return self.train(False)

    def train(self, mode=True):
        self.training = mode
        return self

    def forward_grounding(self, inputs):
        assert not self.training and not torch.is_grad_enabled()
        idx = [x["index"] for x in inputs]
        self.calls.append(idx)
        return {"pred_logits": torch.from_numpy(self.case["logits"][idx]), "pred_boxes": torch.from_numpy(self.case["boxes"][idx])}


def _dataset(name):
    """The case as a grounding dataset: probabilities that survive logit -> sigmoid exactly are not needed -- the oracle is
    given the sigmoid of the logits the model returns."""
    case = dict(cases.get(name))
    with np.errstate(all="ignore"):
        logits = np.log(case["prob"].astype(np.float64) / (1 - case["prob"].astype(np.float64))).astype(np.float32)
    case["logits"] = np.nan_to_num(logits, nan=0.0, posinf=30.0, neginf=-30.0)
    case["prob"] = torch.from_numpy(case["logits"]).sigmoid().numpy()
    B, P, G = case["gt_count"].shape + (case["gt_boxes"].shape[2],)
    inputs = [dict(index=b, height=float(case["sizes"][b, 0]), width=float(case["sizes"][b, 1]),
                   phrases=torch.from_numpy(case["phrase_bits"][b]),
                   phrase_boxes=[case["gt_boxes"][b, p, :min(max(int(case["gt_count"][b, p]), 0), G)] for p in range(P)])
              for b in range(B)]
    return case, inputs


def _counts(case, ks, thrs, merged, k_max):
    want = oracle.match(*(case[k] for k in cases.INPUTS), k_max, thrs, merged)
    live = want["valid"] != 0
    return [[int((want["first_hit"][live][:, j] < k).sum()) for j in range(len(thrs))] for k in ks], int(live.sum())


def test_evaluator_end_to_end_on_cpu_state():
    case, inputs = _dataset("q63_t31")
    model = StubModel(case)
    ev = pe.PhraseGroundingEvaluator()
    result = pe.inference_on_grounding_dataset(model, [inputs[:1], inputs[1:]], ev)
    assert model.training and model.calls == [[0], [1]]                          # the mode is put back
    hits, n = _counts(case, (1, 5, 10), (0.5,), False, 10)
    assert n == 3 and ev.num_valid == n and ev.hits == hits
    assert result == {"grounding": {"R@1": 100.0 * hits[0][0] / n, "R@5": 100.0 * hits[1][0] / n, "R@10": 100.0 * hits[2][0] / n}}
    assert all(t.device.type == "cpu" and t.dtype == torch.int64 for state in ev._state.values() for t in state)
    model.training = False
    pe.inference_on_grounding_dataset(model, [inputs], ev)
    assert not model.training and ev.hits == hits                                # reset, one batch of two: the same counts

    # RefCOCO-style precision: top-1 at several thresholds, merged boxes, other names
    thrs = (0.5, 0.6, 0.7, 0.8, 0.9)
    prec = pe.PhraseGroundingEvaluator(ks=(1,), iou_thrs=thrs, merged=True)
    result = pe.inference_on_grounding_dataset(model, [inputs], prec)
    hits, n = _counts(case, (1,), thrs, True, 1)
    assert list(result["grounding"]) == ["R@1/IoU=0.50", "R@1/IoU=0.60", "R@1/IoU=0.70", "R@1/IoU=0.80", "R@1/IoU=0.90"]
    assert list(result["grounding"].values()) == [100.0 * h / n for h in hits[0]]


def test_evaluator_merge_empty_state_and_refusals():
    case, inputs = _dataset("q65_t33")
    model = StubModel(case).eval()
    whole, first, second = (pe.PhraseGroundingEvaluator(ks=(1, 10, 32), k_max=32) for _ in range(3))
    with torch.no_grad():
        whole.process(inputs, model.forward_grounding(inputs))
        first.process(inputs[:1], model.forward_grounding(inputs[:1]))
        second.process(inputs[1:], model.forward_grounding(inputs[1:]))
    assert first.merge(second) is first and first.evaluate() == whole.evaluate() and first.num_valid == whole.num_valid == 3
    assert whole.hits == _counts(case, (1, 10, 32), (0.5,), False, 32)[0]
    empty = pe.PhraseGroundingEvaluator()
    assert empty.evaluate() == {"grounding": {"R@1": -1.0, "R@5": -1.0, "R@10": -1.0}}
    assert empty.merge(pe.PhraseGroundingEvaluator()).evaluate()["grounding"]["R@5"] == -1.0
    whole.reset()
    assert whole.evaluate()["grounding"] == {"R@1": -1.0, "R@10": -1.0, "R@32": -1.0}
    with pytest.raises(ValueError):
        pe.PhraseGroundingEvaluator(ks=(1, 20), k_max=10)                        # k beyond the candidates that are matched
    with pytest.raises(ValueError):
        pe.PhraseGroundingEvaluator(ks=(0,))
    with pytest.raises(ValueError):
        first.merge(pe.PhraseGroundingEvaluator(ks=(1, 10, 32), k_max=32, merged=True))


def test_evaluator_takes_phrases_as_character_spans():
    """Spans into the caption, tokenized by the evaluator's tokenizer, select the tokens the ready bits would."""
    tok = SimpleTokenizer()
    caption = "a red car . the tall man ."                                        # tokens: [CLS] a red car . the tall man . [SEP]
    T, Q = 12, 6
    rng = np.random.default_rng(5)
    logits = rng.normal(size=(1, Q, T)).astype(np.float32)
    boxes = np.concatenate([rng.uniform(0.2, 0.8, (1, Q, 2)), rng.uniform(0.1, 0.5, (1, Q, 2))], -1).astype(np.float32)
    gts = [np.array([[10.0, 10.0, 60.0, 50.0]], np.float32), np.array([[30.0, 5.0, 90.0, 70.0], [0.0, 0.0, 20.0, 20.0]], np.float32)]
    x = dict(captions=caption, height=80.0, width=100.0, phrases=[[(2, 9)], [(16, 24)]], phrase_boxes=gts)
    ev = pe.PhraseGroundingEvaluator(ks=(1, 5), tokenizer=tok)
    ev.process([x], {"pred_logits": torch.from_numpy(logits), "pred_boxes": torch.from_numpy(boxes)})
    ready = pe.PhraseGroundingEvaluator(ks=(1, 5))
    bits = torch.tensor([[0b1100], [0b11000000]], dtype=torch.int32)            # "red car", "tall man"
    assert pe.phrase_bits_from_spans(pe.tokenize_with_offsets(tok, caption), x["phrases"], T).tolist() == bits.tolist()
    ready.process([dict(x, phrases=bits)], {"pred_logits": torch.from_numpy(logits), "pred_boxes": torch.from_numpy(boxes)})
    assert ev.evaluate() == ready.evaluate() and ev.num_valid == 2
    with pytest.raises(ValueError):
        ready.process([x], {"pred_logits": torch.from_numpy(logits), "pred_boxes": torch.from_numpy(boxes)})   # spans, no tokenizer
