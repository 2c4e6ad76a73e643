"""``box_eval`` without a GPU: what the four evaluators share, at the smallest shapes at which it can go wrong -- the padding of
detections and annotations, the stable score order, the one-copy read-back of the kept state, the greedy walk under COCO's and
under LVIS's rules against answers worked out by hand, and ``process`` -> ``evaluate`` of the three box evaluators on a batch
with an image without detections and an image without annotations, against the oracles."""
import numpy as np
import pytest
import torch

import cocoeval_oracle
import lvis_oracle
import voc_oracle

from ziragroundingdino_amd import box_eval
from ziragroundingdino_amd import evaluation as ev
from ziragroundingdino_amd import lvis_evaluation as lv
from ziragroundingdino_amd import voc_evaluation as voc
from ziragroundingdino_amd.structures import Boxes, Instances


def instances(dets):
    """(score, label, x0, y0, x1, y1) per detection -> one output dict."""
    a = np.asarray(dets, np.float64).reshape(len(dets), 6)
    return {"instances": Instances((200, 200), pred_boxes=Boxes(torch.from_numpy(a[:, 2:].astype(np.float32))),
                                   scores=torch.from_numpy(a[:, 0].astype(np.float32)),
                                   pred_classes=torch.from_numpy(a[:, 1].astype(np.int64)))}


# ---- padding
def test_pad_instances_counts_and_zero_rows():
    outputs = [instances([]), instances([(0.5, 3, 1, 2, 3, 4)]),
               instances([(0.9, 1, 0, 0, 5, 5), (0.2, 2, 1, 1, 6, 6), (0.7, 0, 2, 2, 7, 7)])]
    scores, labels, xyxy, n_keep = box_eval.pad_instances(outputs)
    assert (scores.dtype, labels.dtype, xyxy.dtype, n_keep.dtype) == (torch.float32, torch.int64, torch.float32, torch.int32)
    assert tuple(scores.shape) == (3, 3) and tuple(labels.shape) == (3, 3) and tuple(xyxy.shape) == (3, 3, 4)
    assert n_keep.tolist() == [0, 1, 3]
    assert scores.tolist() == [[0, 0, 0], [0.5, 0, 0], [torch.tensor(v, dtype=torch.float32).item() for v in (0.9, 0.2, 0.7)]]
    assert labels.tolist() == [[0, 0, 0], [3, 0, 0], [1, 2, 0]]
    assert xyxy[1].tolist() == [[1, 2, 3, 4], [0, 0, 0, 0], [0, 0, 0, 0]] and not xyxy[0].any() and xyxy[2, 2].tolist() == [2, 2, 7, 7]
    scores, labels, xyxy, n_keep = box_eval.pad_instances([instances([]), instances([])])
    assert tuple(scores.shape) == (2, 1) and tuple(xyxy.shape) == (2, 1, 4) and n_keep.tolist() == [0, 0]
    assert not scores.any() and not labels.any() and not xyxy.any()


def test_pad_annotations_without_any_annotation():
    for inputs in ([{}, {"annotations": []}], [{"annotations": ()}]):
        box, area, label, flag, n_gt = box_eval.pad_annotations(inputs, "cpu", "iscrowd", with_area=True)
        B = len(inputs)
        assert tuple(box.shape) == (B, 0, 4) and all(tuple(t.shape) == (B, 0) for t in (area, label, flag))
        assert (box.dtype, area.dtype, label.dtype, flag.dtype, n_gt.dtype) == (torch.float64, torch.float64, torch.int64,
                                                                               torch.uint8, torch.int32)
        assert n_gt.tolist() == [0] * B
    box, area, label, flag, n_gt = box_eval.pad_annotations([{}], "cpu", "difficult", with_area=False)
    assert tuple(box.shape) == (1, 0, 4) and area is None and tuple(flag.shape) == (1, 0)


@pytest.mark.parametrize("key", ["iscrowd", "ignore", "difficult"])
def test_pad_annotations_area_default_and_flag_key(key):
    others = {"iscrowd", "ignore", "difficult"} - {key}
    inputs = [{"annotations": [{"bbox": [1.5, 2.0, 0.1, 3.0], "category_id": 4, key: 1},
                               {"bbox": [0, 0, 7, 9], "category_id": 2, "area": 11.0, **{k: 1 for k in others}}]},
              {"annotations": [{"bbox": [3, 4, 5, 6], "category_id": 9, key: 0}]}]
    box, area, label, flag, n_gt = box_eval.pad_annotations(inputs, "cpu", key, with_area=True)
    assert n_gt.tolist() == [2, 1] and label.tolist() == [[4, 2], [9, 0]]
    assert flag.tolist() == [[1, 0], [0, 0]]                                  # this key only; a missing key is 0
    assert area.tolist() == [[0.1 * 3.0, 11.0], [30.0, 0.0]]                  # w * h in doubles where ``area`` is absent
    assert box.tolist() == [[[1.5, 2.0, 0.1, 3.0], [0, 0, 7, 9]], [[3, 4, 5, 6], [0, 0, 0, 0]]]


def test_pad_annotations_voc_form_passes_the_corners_through():
    corners = [1.0, 2.5, 0.1 + 0.2, 1e6 + 0.25]
    inputs = [{"annotations": [{"bbox": corners, "category_id": 1, "difficult": 1, "area": 5.0}]}, {}]
    box, area, label, flag, n_gt = box_eval.pad_annotations(inputs, "cpu", "difficult", with_area=False)
    assert area is None and box.dtype == torch.float64 and box[0, 0].tolist() == corners and not box[1].any()
    assert flag.tolist() == [[1], [0]] and label.tolist() == [[1], [0]] and n_gt.tolist() == [1, 0]


# ---- the score order
def test_sort_by_score_is_stable_and_puts_invalid_rows_last():
    scores = torch.tensor([[0.5, 0.9, 0.5, 0.9, 99.0], [0.3, 0.8, 0.3, 9.0, 0.8]])
    n_keep = torch.tensor([4, 3], dtype=torch.int32)
    labels = torch.arange(10).reshape(2, 5)
    xyxy = torch.arange(40, dtype=torch.float32).reshape(2, 5, 4)
    want = torch.tensor([[1, 3, 0, 2, 4], [1, 0, 2, 3, 4]])      # ties in input order; the 99.0 and the 9.0 lie behind n_keep
    s, l, x = box_eval.sort_by_score(scores, labels, xyxy, n_keep)
    assert torch.equal(s, torch.gather(scores, 1, want)) and torch.equal(l, torch.gather(labels, 1, want))
    assert torch.equal(x, torch.stack([xyxy[b][want[b]] for b in range(2)]))
    assert s.is_contiguous() and l.is_contiguous() and x.is_contiguous()
    assert s[0].tolist() == [pytest.approx(0.9), pytest.approx(0.9), 0.5, 0.5, 99.0] and l[0].tolist() == [1, 3, 0, 2, 4]


def test_mask_behind():
    t = torch.tensor([[5, 6, 7], [8, 9, 10]])
    assert box_eval.mask_behind(t, torch.tensor([0, 2], dtype=torch.int32)).tolist() == [[-1, -1, -1], [8, 9, -1]]


# ---- the kept state
def test_gather_state_rereads_the_words_as_unsigned():
    batches = [dict(scores=torch.tensor([[0.25, 0.5]]), matched=torch.tensor([[-1, -2 ** 63]]), extra=torch.zeros(3)),
               dict(scores=torch.zeros((2, 0)), matched=torch.zeros((2, 0), dtype=torch.int64)),
               dict(scores=torch.tensor([[1.0]]), matched=torch.tensor([[5]]))]
    host = box_eval.gather_state(batches, ("scores", "matched"), ("matched",), np.uint64)
    assert [set(h) for h in host] == [{"scores", "matched"}] * 3
    assert host[0]["matched"].dtype == np.uint64 and host[0]["matched"].tolist() == [2 ** 64 - 1, 2 ** 63]
    assert host[0]["scores"].dtype == np.float32 and host[0]["scores"].tolist() == [0.25, 0.5]
    assert host[1]["matched"].shape == (0,) and host[2]["matched"].tolist() == [5] and host[2]["scores"].tolist() == [1.0]
    words = box_eval.gather_state([dict(qscore=torch.tensor([[0.5]], dtype=torch.float64), tp=torch.tensor([[-1]], dtype=torch.int32),
                                        fp=torch.tensor([[-2 ** 31]], dtype=torch.int32))], ("qscore", "tp", "fp"), ("tp", "fp"), np.uint32)
    assert words[0]["tp"].dtype == np.uint32 and words[0]["tp"].tolist() == [2 ** 32 - 1] and words[0]["fp"].tolist() == [2 ** 31]
    assert words[0]["qscore"].dtype == np.float64
    assert box_eval.gather_state([], ("scores", "matched"), ("matched",), np.uint64) == []
    for e in (ev.CocoBoxEvaluator(["a"]), lv.LVISBoxEvaluator(["a"], ["f"]), voc.PascalVOCBoxEvaluator(["a"])):
        assert e._gather() == []
    assert "_gather" not in vars(lv.LVISBoxEvaluator)           # taken from the base class, not from another evaluator


# ---- the walk, by hand
# One image, one label, 4 detections x 3 GTs, T = 2 (IoU >= 0.5, >= 0.75), A = 2: problem p = a T + t.
# g0 is flagged (ignored in both ranges; under COCO's rules a crowd), g2 lies outside range 1, d2 does not take part.
WALK_IOU = np.array([[0.9, 0.6, 0.6], [0.8, 0.0, 0.55], [0.9, 0.9, 0.9], [0.0, 0.7, 0.7]])
WALK_IGN = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 1], [1, 0, 1]], bool)
WALK_FLOOR = np.array([[0.5], [0.75], [0.5], [0.75]])
WALK_TAKES = np.array([True, True, False, True])
WALK_OUT = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]], bool)         # [p, k]: d1 is outside range 1
# d0: p0 -- g0 has the best IoU but the not-ignored g1, g2 shut it out, and they tie at 0.6: the LAST, g2;  p1 -- only g0 reaches
#     0.75: taken, ignored;  p2 -- g2 is ignored here, so g1;  p3 -- g0.
# d1: p0 -- g2 is taken, g0 is left: ignored;  p1 / p3 -- g0 was taken by d0: a crowd is taken AGAIN (COCO), else nothing is left
#     and the detection's own flag decides (LVIS: 0 in range 0, 1 in range 1);  p2 -- g0 (0.8) before g2 (0.55), both ignored.
# d3: p0 -- g2 and g0 are taken: g1;  p2 -- g1 and g0 are taken: g2, ignored;  p1 / p3 -- 0.7 < 0.75: unmatched, its own flag
#     (LVIS: its category is not exhaustively annotated, every bit).
WALK_WANT = {
    "coco": dict(matched=[15, 15, 0, 5], ignored=[0b1010, 15, 0, 0b0100],
                 gt_of=[[2, 0, 1, 0], [0, 0, 0, 0], [-1, -1, -1, -1], [1, -1, 2, -1]]),
    "lvis": dict(matched=[15, 5, 0, 5], ignored=[0b1010, 0b1101, 0, 0b1110],
                 gt_of=[[2, 0, 1, 0], [0, -1, 0, -1], [-1, -1, -1, -1], [1, -1, 2, -1]]),
}


@pytest.mark.parametrize("rules", ["coco", "lvis"])
def test_greedy_walk_by_hand(rules):
    same = np.ones((4, 3), bool)
    if rules == "coco":
        retake, det_out = np.array([True, False, False]), WALK_OUT
    else:
        retake, det_out = None, WALK_OUT | np.array([False, False, False, True])[None, :]
    matched, ignored, gt_of = box_eval.greedy_walk(WALK_IOU, same, WALK_TAKES, WALK_IGN, det_out, WALK_FLOOR, retake)
    want = WALK_WANT[rules]
    assert (matched.dtype, ignored.dtype, gt_of.dtype) == (np.uint64, np.uint64, np.int32)
    assert matched.tolist() == want["matched"] and ignored.tolist() == want["ignored"] and gt_of.tolist() == want["gt_of"]
    taken_g0_in_p1 = sum(row[1] == 0 for row in want["gt_of"])
    assert taken_g0_in_p1 == (2 if rules == "coco" else 1)


def test_crowd_mask_switches_the_union():
    box = np.array([[0, 0, 10, 10]], np.float32)
    gbox = np.array([[0.0, 0.0, 20.0, 20.0], [0.0, 0.0, 20.0, 20.0], [50.0, 50.0, 5.0, 5.0]])
    iou, da = box_eval.xywh_iou(box, gbox, np.array([True, False, False]))
    assert da.tolist() == [100.0] and iou.tolist() == [[1.0, 0.25, 0.0]]
    assert box_eval.xywh_iou(box, gbox)[0].tolist() == [[0.25, 0.25, 0.0]]


# ---- process -> evaluate against the oracles: image 0 has no detection, image 1 no annotations, image 2 both
DETS = ([], [(0.9, 0, 0, 0, 10, 10), (0.8, 1, 5, 5, 40, 40)],
        [(0.95, 0, 0, 0, 10, 12), (0.6, 1, 21, 20, 50, 50), (0.6, 0, 100, 100, 120, 120)])
GTS = ([(0, 0, 0, 10, 10, 0), (1, 20, 20, 30, 30, 0)], None, [(0, 0, 0, 10, 10, 0), (1, 20, 20, 30, 30, 1), (1, 20, 20, 30, 30, 0)])
NAMES = ["c0", "c1"]


def dataset(flag_key, voc_corners=False):
    inputs = []
    for gts in GTS:
        if gts is None:
            inputs.append({})
            continue
        corners = lambda x, y, w, h: [x + 1.0, y + 1.0, float(x + w), float(y + h)]     # VOC: 1-based, inclusive
        inputs.append({"annotations": [{"bbox": corners(*g[1:5]) if voc_corners else [float(v) for v in g[1:5]],
                                        "category_id": g[0], flag_key: g[5]} for g in gts]})
    return inputs, [instances(d) for d in DETS]


def oracle_dts(dets):
    f = np.float32
    return [{"category_id": d[1], "score": float(f(d[0])), "pos": k,
             "bbox": [float(d[2]), float(d[3]), float(f(f(d[4]) - f(d[2]))), float(f(f(d[5]) - f(d[3])))]} for k, d in enumerate(dets)]


def oracle_gts(gts, flag_key):
    return [{"category_id": g[0], "bbox": [float(v) for v in g[1:5]], "area": float(g[3] * g[4]), flag_key: g[5], "idx": i}
            for i, g in enumerate(gts or ())]


def test_coco_evaluator_with_an_empty_image_on_either_side():
    e = ev.CocoBoxEvaluator(NAMES)
    e.process(*dataset("iscrowd"))
    got = e.evaluate()["bbox"]
    assert [tuple(v.shape) for v in (e._batches[0]["scores"], e._batches[0]["gt_label"])] == [(3, 3), (3, 3)]
    want = cocoeval_oracle.coco_summary([{"dts": oracle_dts(d), "gts": oracle_gts(g, "iscrowd")} for d, g in zip(DETS, GTS)], NAMES)
    assert set(got) == set(want) and 0 < want["AP"] < 100
    for k in want:          # two summations of the same fp64 table entries: a few ulp of 100, as test_evaluation_cpu.py allows
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])


def test_lvis_evaluator_with_an_empty_image_on_either_side():
    inputs, outputs = dataset("ignore")
    for x in inputs:
        x["neg_category_ids"] = [0, 1]              # image 1's detections are false positives, not filtered
    inputs[2]["not_exhaustive_category_ids"] = [0]
    e = lv.LVISBoxEvaluator(NAMES, ["r", "f"])
    e.process(inputs, outputs)
    got = e.evaluate()
    images = [{"dts": oracle_dts(d), "gts": oracle_gts(g, "ignore"), "neg": {0, 1}, "nel": {0} if b == 2 else set()}
              for b, (d, g) in enumerate(zip(DETS, GTS))]
    rank, matched, ignored, gt_ignored, _ = lvis_oracle.match_outputs(images, 3, 3, 2, ev.DEFAULT_IOU_THRS, ev.DEFAULT_AREA_RNGS, 3)
    state = e._batches[0]
    assert np.array_equal(state["rank"].numpy(), rank) and np.array_equal(state["matched"].numpy().view(np.uint64), matched)
    assert np.array_equal(state["ignored"].numpy().view(np.uint64), ignored) and np.array_equal(state["gt_ignored"].numpy(), gt_ignored)
    assert state["gt_label"].tolist() == [[0, 1, -1], [-1, -1, -1], [0, 1, 1]] and int(state["n_pred"]) == 5
    det, gt = rank >= 0, state["gt_label"].numpy() >= 0
    precision, recall = ev.accumulate(state["scores"].numpy()[det].astype(np.float64), state["labels"].numpy()[det], rank[det],
                                      matched[det], ignored[det], state["gt_label"].numpy()[gt], gt_ignored[gt], 2,
                                      ev.DEFAULT_IOU_THRS, ev.DEFAULT_AREA_RNGS, (300,))
    assert np.array_equal(e.precision, precision) and np.array_equal(e.recall, recall)
    assert got == {"bbox": lv.summarize(precision, recall, ["r", "f"], ev.DEFAULT_IOU_THRS)} and 0 < got["bbox"]["AP"] < 100


@pytest.mark.parametrize("year", [2007, 2012])
def test_voc_evaluator_with_an_empty_image_on_either_side(year):
    e = voc.PascalVOCBoxEvaluator(NAMES, year=year)
    e.process(*dataset("difficult", voc_corners=True))
    got = e.evaluate()["bbox"]
    f = np.float32
    images = [{"dts": [(f(d[0]), d[1], tuple(f(v) for v in d[2:])) for d in dets],
               "gts": [(g[0], (g[1] + 1.0, g[2] + 1.0, float(g[1] + g[3]), float(g[2] + g[4])), bool(g[5])) for g in gts or ()]}
              for dets, gts in zip(DETS, GTS)]
    want = voc_oracle.voc_summary(images, NAMES, year)
    assert set(got) == set(want) and 0 < want["AP"] < 100
    for k in want:          # means of the same fp64 APs taken twice: a few ulp of 100, as test_voc_evaluation.py allows
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
