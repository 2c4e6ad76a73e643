"""LVIS box AP without a GPU: the C ABI of the matching is declared in include/zira_lvis.h, typed from that header into tables
of its own and exported by the built library; argument errors are answered on the host; ``match_reference`` against lvis_oracle
(the loop-for-loop LVISEval, written independently) bit for bit; ``summarize`` on a hand-worked table; ``category_bitsets`` around
the word size; ``LVISBoxEvaluator`` on CPU state end to end; the category fixture."""
import collections
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import lvis_cases as cases
import lvis_oracle as oracle
from conftest import GOLDEN, ROOT

from ziragroundingdino_amd import _lib
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd import evaluation as ev
from ziragroundingdino_amd import lvis_evaluation as lv

ENTRIES = ["zira_lvis_match_lds_bytes", "zira_lvis_match"]
EINVAL = 1
FIXTURE = os.path.join(GOLDEN, "lvis_v0_5_categories.json")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_typed_and_exported():
    text = open(os.path.join(ROOT, "include", "zira_lvis.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(zira_[a-z0-9_]+)\s*\(", text)
    assert declared == ENTRIES == list(_lib.LVIS_SYMBOLS) == list(_lib.LVIS_PROTOTYPES)
    zbuild.build_extension()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ENTRIES:
        assert hasattr(raw, sym), "libzira_msda.so does not export %s" % sym
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    P = _lib.LVIS_PROTOTYPES
    assert P["zira_lvis_match_lds_bytes"] == (sz, [i, i, i, i, i])
    assert P["zira_lvis_match"] == (i, [vp, vp, vp, vp, i, i, vp, vp, vp, vp, vp, i, vp, vp, i, vp, i, vp, i, i, vp, vp, vp, vp, vp, vp])
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert _lib.LVIS_CONSTANTS == {"ZIRA_LVIS_MAX_B": 65535, "ZIRA_LVIS_MAX_K": 1024, "ZIRA_LVIS_MAX_G": 1024,
                                   "ZIRA_LVIS_MAX_CLASSES": 65535}
    assert (lv.MAX_B, lv.MAX_K, lv.MAX_G, lv.MAX_CLASSES) == (65535, 1024, 1024, 65535)


def test_the_other_headers_surfaces_are_what_they_were():
    assert len(_lib.SYMBOLS) == 100 and not set(ENTRIES) & set(_lib.SYMBOLS)
    assert not any("LVIS" in name for name in _lib.CONSTANTS) and len(_lib.NMS_SYMBOLS) == 2 and len(_lib.VOCAB_SYMBOLS) == 2
    assert os.path.join(ROOT, "include", "zira_lvis.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "lvismatch.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    assert "-ffp-contract=off" in zbuild.EXTRA_FLAGS["lvismatch.hip"] and "topk.hip" not in zbuild.EXTRA_FLAGS


def _call(lib, B=2, K=300, G=40, C=1230, T=10, A=4, max_det=300, **ptr):
    """The entry on made-up addresses: an argument error is answered before any of them is looked at."""
    p = dict(scores=64, labels=64, xyxy=64, n_keep=64, gt_xywh=64, gt_area=64, gt_label=64, gt_ignore=64, n_gt=64, neg_set=64,
             nel_set=64, rank=64, matched=64, ignored=64, gt_ignored=64, gt_of=64)
    p.update(ptr)
    thrs = (ctypes.c_double * max(T, 1))(*([0.5] * max(T, 1)))
    rngs = (ctypes.c_double * (2 * max(A, 1)))(*([0.0, 1e10] * max(A, 1)))
    return lib.zira_lvis_match(p["scores"], p["labels"], p["xyxy"], p["n_keep"], B, K, p["gt_xywh"], p["gt_area"], p["gt_label"],
                               p["gt_ignore"], p["n_gt"], G, p["neg_set"], p["nel_set"], C, p.get("thrs", thrs), T,
                               p.get("rngs", rngs), A, max_det, p["rank"], p["matched"], p["ignored"], p["gt_ignored"],
                               p["gt_of"], None)


def test_argument_errors_are_answered_on_the_host():
    """Nothing is launched: there is no device here, and the host pointers are never looked at."""
    lib = _lib.load()
    for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(K=0), dict(K=1025, max_det=300), dict(G=-1), dict(G=1025), dict(C=0),
                dict(C=65536), dict(T=0), dict(T=17, A=1), dict(A=0), dict(A=5, T=1), dict(T=13, A=5), dict(T=9, A=8), dict(max_det=0), dict(max_det=301), dict(max_det=-1)):
        assert _call(lib, **bad) == EINVAL, bad
    for null in ("scores", "labels", "xyxy", "n_keep", "neg_set", "nel_set", "thrs", "rngs", "rank", "matched", "ignored",
                 "gt_xywh", "gt_area", "gt_label", "gt_ignore", "n_gt", "gt_ignored"):
        assert _call(lib, **{null: None}) == EINVAL, null
    # the LDS the launch takes (host arithmetic): K (16 + 4 + 4 + 1) + G (40 + 4 + 1) + A T 2 ceil(K / 32) 4 + ceil(C / 32) 4
    assert lib.zira_lvis_match_lds_bytes(300, 40, 10, 4, 1230) == 300 * 25 + 40 * 45 + 40 * 2 * 10 * 4 + 39 * 4 == 12656
    assert lib.zira_lvis_match_lds_bytes(1024, 1024, 10, 4, 65535) == 1024 * 25 + 1024 * 45 + 40 * 2 * 32 * 4 + 2048 * 4 == 90112
    assert lib.zira_lvis_match_lds_bytes(1024, 1024, 16, 4, 65535) <= 160 * 1024
    for K, G, T, A, C in ((0, 1, 1, 1, 1), (1025, 1, 1, 1, 1), (1, 1025, 1, 1, 1), (1, -1, 1, 1, 1), (1, 1, 17, 1, 1), (1, 1, 1, 5, 1),
                          (1, 1, 13, 5, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 65536)):
        assert lib.zira_lvis_match_lds_bytes(K, G, T, A, C) == 0, (K, G, T, A, C)


# ---- the definition against the oracle -------------------------------------------------------------------------------------------
def assert_equal(got, want, what):
    for k in cases.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %s" % (what, k, np.argwhere(got[k] != want[k])[:5].tolist())


@pytest.mark.parametrize("name", cases.names())
def test_match_reference_equals_the_oracle(name):
    case = cases.get(name)
    got = cases.as_numpy(lv.match_reference(*cases.tensors(case), case["C"], cases.IOU_THRS, cases.AREA_RNGS, case["max_det"]))
    assert_equal(got, cases.expected(case), name)


def test_the_cases_hold_what_they_are_for():
    """By the ORACLE's verdict on the inputs, never by the code under test."""
    mixed, want = cases.get("mixed"), cases.expected(cases.get("mixed"))
    assert mixed["scores"].shape == (3, 40) and mixed["gt_label"].shape == (3, 12) and mixed["C"] == 70
    assert len(cases.IOU_THRS) == 10 and len(cases.AREA_RNGS) == 4
    seen = collections.defaultdict(set)                       # label -> the ranks' signs the oracle gave it
    for b in range(3):
        gts = set(mixed["gt_label"][b, :mixed["n_gt"][b]].tolist())
        for k in range(int(mixed["n_keep"][b])):
            c = int(mixed["labels"][b, k])
            kind = ("pos" if c in gts else "") + ("neg" if c in cases.NEG else "") + ("nel" if c in cases.NEL else "")
            seen[kind or ("out" if not 0 <= c < 70 else "none")].add(bool(want["rank"][b, k] >= 0))
    assert {k: v for k, v in seen.items() if k in ("pos", "neg", "nel", "posnel", "posneg", "negnel", "none", "out")} == {
        "pos": {True}, "neg": {True}, "nel": {False}, "posnel": {True}, "posneg": {True}, "negnel": {True}, "none": {False},
        "out": {False}}
    ties = sum(len(set(r)) < len(r) for r in mixed["scores"])
    assert ties == 3 and (want["matched"] != 0).any() and ((want["ignored"] != 0) & (want["matched"] == 0)).any()
    empty = cases.expected(cases.get("empty_image"))
    assert (empty["rank"][0] == -1).all() and (empty["rank"][1] >= 0).any() and not empty["matched"][0].any()
    none = cases.expected(cases.get("no_gt_arrays"))
    assert none["gt_ignored"].shape == (2, 0) and (none["rank"] >= 0).any() and not none["matched"].any() and none["ignored"].any()
    # hand-worked (the rules of include/zira_lvis.h by hand, not a run of either implementation)
    bits = lambda a, ts=range(10): sum(1 << (a * 10 + t) for t in ts)
    full = bits(0) | bits(1) | bits(2) | bits(3)
    ign = cases.expected(cases.get("ignored_gt"))
    # GT 0 flagged (IoU 1 with the three detections), GT 1 plain (IoU 100 / 120: thresholds 0.5 .. 0.8), both small
    assert ign["gt_ignored"][0].tolist() == [15, 4 | 8, 15]
    assert ign["gt_of"][0, 0].tolist() == ([1] * 7 + [0] * 3) * 2 + [0] * 20      # all, small: the plain GT first; medium, large: both are out
    assert ign["matched"][0].tolist() == [full, bits(0, range(7)) | bits(1, range(7)) | bits(2, range(7)) | bits(3, range(7)), 0, full]
    assert ign["ignored"][0].tolist() == [bits(0, range(7, 10)) | bits(1, range(7, 10)) | bits(2) | bits(3),
                                          bits(0, range(7)) | bits(1, range(7)) | bits(2) | bits(3), bits(2) | bits(3), full]
    area = cases.expected(cases.get("area_ignore"))
    assert area["gt_ignored"][0].tolist() == [2 | 8]                                                    # 34 x 34 is medium
    assert area["matched"][0].tolist() == [sum(bits(a, range(6)) for a in range(4)), 0]                 # IoU 900 / 1156: six thresholds
    assert area["ignored"][0].tolist() == [bits(1, range(6)) | bits(2, range(6, 10)) | bits(3), bits(2) | bits(3)]
    cut, cut_k = cases.get("image_cut"), cases.expected(cases.get("image_cut_max_det_K"))
    want = cases.expected(cut)
    assert cut["scores"][0, 299] == cut["scores"][0, 300] and cut["max_det"] == 300 and cut["n_keep"][0] == 700
    assert (want["rank"][0, 300:] == -1).all() and (want["rank"][0, :300] >= 0).any() and (cut_k["rank"][0, 300:700] >= 0).any()
    assert (cut_k["rank"][0, 700:] == -1).all() and np.array_equal(cut_k["matched"][0, :300], want["matched"][0, :300])
    assert cut_k["matched"][0, 300:700].any() and not want["matched"][0, 300:].any()
    clamp = cases.expected(cases.get("clamping"))
    assert (clamp["rank"][0] == -1).all() and (clamp["rank"][1] >= 0).any() and (clamp["gt_ignored"][1] == 0).all()


def test_cpu_tensors_never_reach_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a CPU tensor reached the library"))
    case = cases.get("ignored_gt")
    t = cases.tensors(case)
    assert not lv.match_supported(*t, case["C"])
    with pytest.raises(RuntimeError, match="does not serve"):
        lv.match(*t, case["C"])
    with pytest.raises(ValueError):
        lv.match_reference(*t[:9], t[9][:, :2], t[10], case["C"])                       # a bitset of the wrong width


# ---- summarize, category_bitsets, the fixture --------------------------------------------------------------------------------------
def test_summarize_on_a_hand_worked_table():
    T, R, C, A = 10, 2, 4, 4
    p = -np.ones((T, R, C, A, 1))
    r = -np.ones((T, C, A, 1))
    p[:, :, 0, 0], p[:, :, 1, 0], p[:, :, 2, 0] = 0.5, 0.25, 1.0          # class 3 is unpopulated
    p[0, :, 0, 0], p[5, :, 1, 0] = 1.0, 0.75                                  # IoU 0.5 of class 0, IoU 0.75 of class 1
    p[:, :, 0, 1], p[:, :, 1, 3] = 0.125, 0.375                               # small: class 0; large: class 1; medium: nothing
    r[:, 0, 0], r[:, 1, 0], r[:, 2, 0], r[:, 0, 1], r[:, 1, 3] = 0.5, 0.25, 1.0, 0.75, 0.125
    got = lv.summarize(p, r, ["f", "c", "f", "c"], ev.DEFAULT_IOU_THRS)
    want = {"AP": 100 * (0.55 + 0.3 + 1.0) / 3, "AP50": 100 * (1.0 + 0.25 + 1.0) / 3, "AP75": 100 * (0.5 + 0.75 + 1.0) / 3,
            "APs": 12.5, "APm": -1.0, "APl": 37.5, "APr": -1.0, "APc": 30.0, "APf": 100 * (0.55 + 1.0) / 2,
            "AR@300": 100 * (0.5 + 0.25 + 1.0) / 3, "ARs@300": 75.0, "ARm@300": -1.0, "ARl@300": 12.5}
    assert list(got) == list(want) and list(got)[:9] == list(lv.METRICS)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    assert got["APr"] == -1.0 and got["APm"] == -1.0                          # an empty frequency group, an empty area range
    assert all(v == -1.0 for v in lv.summarize(-np.ones_like(p), -np.ones_like(r), ["r", "c", "f", "f"], ev.DEFAULT_IOU_THRS).values())
    with pytest.raises(ValueError):
        lv.summarize(p, r, ["f", "c"], ev.DEFAULT_IOU_THRS)


@pytest.mark.parametrize("C,W", [(31, 1), (32, 1), (33, 2), (70, 3)])
def test_category_bitsets(C, W):
    lists = [[0, C - 1], [], [c for c in (30, 31, 32, 63, 64, 69) if c < C], [5, 5, 0]]
    got = lv.category_bitsets(lists, C)
    assert got.dtype == torch.int32 and tuple(got.shape) == (4, W) and got.is_contiguous()
    words = got.numpy().view(np.uint32)
    for b, ids in enumerate(lists):
        assert [c for c in range(W * 32) if (int(words[b, c // 32]) >> (c % 32)) & 1] == sorted(set(ids))
    if C >= 32:
        assert int(got[2, 0]) < 0                                             # bit 31: the int32 holds the u32's bits
    for bad in ([[C]], [[-1]]):
        with pytest.raises(ValueError):
            lv.category_bitsets(bad, C)
    assert tuple(lv.category_bitsets([], C).shape) == (0, W)


def test_load_frequencies_reads_the_fixture():
    raw = json.load(open(FIXTURE))
    freq = lv.load_frequencies(FIXTURE)
    names, again = lv.load_categories(FIXTURE)
    assert len(freq) == len(names) == 1230 and again == freq and os.path.getsize(FIXTURE) < 1 << 20
    assert dict(collections.Counter(freq)) == raw["counts"] == {"r": 454, "c": 461, "f": 315}
    assert [r["index"] for r in raw["categories"]] == list(range(1230)) and set(raw) == {"dataset", "counts", "categories"}
    assert all(set(r) == {"index", "name", "frequency"} for r in raw["categories"])
    assert (names[0], freq[0]) == (raw["categories"][0]["name"], raw["categories"][0]["frequency"])
    lv.LVISBoxEvaluator(names, freq)                                           # the evaluator takes them as they are


# ---- the evaluator on CPU state ------------------------------------------------------------------------------------------------
class _Inst:
    def __init__(self, scores, classes, boxes):
        self.scores, self.pred_classes, self.pred_boxes = scores, classes, types.SimpleNamespace(tensor=boxes)

    def __len__(self):
        return len(self.scores)


def batch_of(case):
    """A case as ``process`` takes it: batched_inputs with annotations and the two id lists, outputs with Instances."""
    inputs, outputs = [], []
    K, G = case["scores"].shape[1], case["gt_label"].shape[1]
    for b in range(case["scores"].shape[0]):
        nk, ng = min(max(int(case["n_keep"][b]), 0), K), min(max(int(case["n_gt"][b]), 0), G) if G else 0
        anns = [{"bbox": case["gt_xywh"][b, g].tolist(), "category_id": int(case["gt_label"][b, g]),
                 "area": float(case["gt_area"][b, g]), "ignore": int(case["gt_ignore"][b, g])} for g in range(ng)]
        inputs.append({"annotations": anns, "neg_category_ids": case["neg"][b], "not_exhaustive_category_ids": case["nel"][b]})
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a[b, :nk]))
        outputs.append({"instances": _Inst(t(case["scores"]), t(case["labels"]), t(case["xyxy"]))})
    return inputs, outputs


def oracle_tables(names, C, max_dets=300):
    """lvis_oracle's matching of the cases, flattened, through ``evaluation.accumulate``."""
    flat = collections.defaultdict(list)
    for name in names:
        case = cases.get(name)
        K = case["scores"].shape[1]
        out = oracle.match_outputs(cases.images(case), K, case["gt_label"].shape[1], C, cases.IOU_THRS, cases.AREA_RNGS,
                                   min(max_dets, K))
        det = out[0] >= 0
        ng = np.clip(case["n_gt"], 0, case["gt_label"].shape[1])
        gt = np.arange(case["gt_label"].shape[1])[None, :] < ng[:, None]
        for k, v in (("scores", case["scores"][det].astype(np.float64)), ("labels", case["labels"][det]), ("rank", out[0][det]),
                     ("matched", out[1][det]), ("ignored", out[2][det]), ("gt_label", case["gt_label"][gt]), ("gt_ignored", out[3][gt])):
            flat[k].append(v)
    cat = {k: np.concatenate(v) for k, v in flat.items()}
    return ev.accumulate(cat["scores"], cat["labels"], cat["rank"], cat["matched"], cat["ignored"], cat["gt_label"],
                         cat["gt_ignored"], C, cases.IOU_THRS, cases.AREA_RNGS, (max_dets,))


EVAL_CASES = ("mixed", "empty_image", "no_gt_arrays", "wide", "ignored_gt")
FREQ70 = [("r", "c", "f")[c % 3] for c in range(70)]


def test_evaluator_on_cpu_state_end_to_end(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("CPU state reached the library"))
    names = ["c%d" % c for c in range(70)]
    e = lv.LVISBoxEvaluator(names, FREQ70)
    for name in EVAL_CASES:
        e.process(*batch_of(cases.get(name)))
    got = e.evaluate()
    precision, recall = oracle_tables(EVAL_CASES, 70)
    assert np.array_equal(e.precision, precision) and np.array_equal(e.recall, recall)
    want = lv.summarize(precision, recall, FREQ70, cases.IOU_THRS)
    assert got == {"bbox": want} and list(want)[:9] == list(lv.METRICS)
    assert 0 < want["AP"] < 100 and want["APr"] > -1 and want["APc"] > -1 and want["APf"] > -1 and want["AR@300"] > 0
    # merge: two halves are the whole
    a, b = lv.LVISBoxEvaluator(names, FREQ70), lv.LVISBoxEvaluator(names, FREQ70)
    for name in EVAL_CASES[:2]:
        a.process(*batch_of(cases.get(name)))
    for name in EVAL_CASES[2:]:
        b.process(*batch_of(cases.get(name)))
    assert a.merge(b).evaluate() == got
    with pytest.raises(ValueError):
        a.merge(lv.LVISBoxEvaluator(names, FREQ70, max_dets=100))
    # COCO's rules on the same state give another number: the federated rules are in force
    coco = ev.CocoBoxEvaluator(names, max_dets=(300,))
    for name in EVAL_CASES:
        inputs, outputs = batch_of(cases.get(name))
        coco.process(inputs, outputs)
    assert coco.evaluate()["bbox"]["AP"] != want["AP"]


def test_evaluator_cuts_to_max_dets_per_image_and_without_predictions_reports_minus_one():
    names = ["c%d" % c for c in range(70)]
    cut = cases.get("image_cut")
    e = lv.LVISBoxEvaluator(names, FREQ70)
    e.process(*batch_of(cut))
    got = e.evaluate()["bbox"]
    precision, recall = oracle_tables(("image_cut",), 70)
    assert np.array_equal(e.precision, precision) and got == lv.summarize(precision, recall, FREQ70, cases.IOU_THRS)
    assert int((e._batches[0]["rank"] >= 0).sum()) < 300 and e._batches[0]["scores"].shape == (1, 700)
    wide = lv.LVISBoxEvaluator(names, FREQ70, max_dets=700)
    wide.process(*batch_of(cut))
    assert wide.evaluate()["bbox"] != got and "AR@700" in wide.evaluate()["bbox"]
    # no predictions at all: the reference sets every metric to -1
    none = lv.LVISBoxEvaluator(names, FREQ70)
    inputs, outputs = batch_of(cases.get("mixed"))
    empty = [{"instances": _Inst(torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.zeros(0, 4))} for _ in outputs]
    none.process(inputs, empty)
    assert none.evaluate() == {"bbox": {k: -1.0 for k in got}} and len(got) == 13
    assert lv.LVISBoxEvaluator(names, FREQ70).evaluate() == {"bbox": {k: -1.0 for k in got}}
    with pytest.raises(ValueError):
        lv.LVISBoxEvaluator(names, FREQ70[:3])
