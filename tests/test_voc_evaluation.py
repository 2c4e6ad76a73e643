"""Pascal VOC box AP without a GPU: ``voc_evaluation.match_reference`` + ``accumulate`` against the reference's own ``voc_eval``
(tests/golden/voc_eval.pt, written by gen_voc_golden.py) and against the loop-for-loop restatement in voc_oracle.py (two
independent statements of the rules); hand-built cases with known answers; the evaluator's surface, ``merge`` and the
``evaluate=`` keyword of the task chain.  The same cases are what test_voc_match_gpu.py holds the kernel to."""
import itertools
import os

import numpy as np
import pytest
import torch

import voc_cases as cases
import voc_oracle as oracle
from conftest import GOLDEN

from ziragroundingdino_amd import voc_evaluation as voc

T = len(cases.IOU_THRS)
ALL = np.uint32((1 << T) - 1)


def reference(case, thrs=cases.IOU_THRS):
    return cases.as_numpy(voc.match_reference(*cases.tensors(case), case["n_classes"], thrs))


def evaluator_of(case, chunks=1, **kw):
    e = voc.PascalVOCBoxEvaluator(["c%d" % i for i in range(case["n_classes"])], **kw)
    t = cases.tensors(case)
    B = t[0].shape[0]
    step = -(-B // chunks)
    for lo in range(0, B, step):
        e.process_padded(*(x[lo:lo + step].contiguous() for x in t))
    return e


def bits(*ts):
    return np.uint32(sum(1 << t for t in ts))


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLDEN, "voc_eval.pt"), weights_only=False)


# ---- the reference's own numbers

def flat_state(g, num_classes):
    inp = g["inputs"]
    t = [torch.from_numpy(np.ascontiguousarray(inp[k])) for k in cases.INPUTS]
    qscore, tp, fp, _ = cases.as_numpy(voc.match_reference(*t, num_classes, [x / 100.0 for x in g["thresholds"]])).values()
    K, G = inp["scores"].shape[1], inp["gt_label"].shape[1]
    det = (np.arange(K)[None, :] < inp["n_keep"][:, None]).reshape(-1)
    gt = (np.arange(G)[None, :] < inp["n_gt"][:, None]).reshape(-1)
    return (qscore.reshape(-1)[det], inp["labels"].reshape(-1)[det], tp.reshape(-1)[det], fp.reshape(-1)[det],
            inp["gt_label"].reshape(-1)[gt], inp["gt_difficult"].reshape(-1)[gt])


@pytest.mark.parametrize("use07", [True, False])
def test_curves_and_ap_equal_the_references_voc_eval(golden, use07):
    names = golden["names"]
    thrs = [x / 100.0 for x in golden["thresholds"]]
    ap, curves = voc.accumulate(*flat_state(golden, len(names)), len(names), thrs, use07, with_curves=True)
    ghost = names.index("ghost")
    for c in range(len(names)):
        for t, thresh in enumerate(golden["thresholds"]):
            rec, prec, want = golden["curves"][(use07, c, thresh)]
            got_rec, got_prec = curves[c][t]
            assert got_rec.shape == rec.shape and np.array_equal(got_rec, rec, equal_nan=True), (c, thresh)
            assert np.array_equal(got_prec, prec), (c, thresh)
            print(names[c], thresh, ap[c, t], want)
            if np.isnan(want):
                assert c == ghost and not use07 and np.isnan(ap[c, t])
            else:
                assert abs(ap[c, t] - want) <= 1e-12, (c, thresh, ap[c, t], want)
    assert sum(len(golden["curves"][(use07, c, 50)][0]) for c in range(len(names))) == int(golden["inputs"]["n_keep"].sum())


def test_class_without_a_countable_gt_does_what_the_reference_does(golden):
    """npos == 0 (difficult GTs only) with detections: rec is 0 / 0 = NaN, so the 11-point rule gives 0.0 and the envelope area
    NaN; that is the reference's arithmetic (the golden's ghost class), and ours."""
    ghost = golden["names"].index("ghost")
    assert golden["curves"][(True, ghost, 50)][2] == 0.0 and np.isnan(golden["curves"][(False, ghost, 50)][2])
    assert len(golden["curves"][(True, ghost, 50)][0]) > 0
    case = cases.get("difficult")
    a = {k: case[k].copy() for k in cases.INPUTS}
    a["gt_difficult"][:] = 1
    args = [torch.from_numpy(a[k]) for k in cases.INPUTS]
    for year, check in ((2007, lambda v: v == 0.0), (2012, np.isnan)):
        e = voc.PascalVOCBoxEvaluator(["c0"], year=year)
        e.process_padded(*args)
        res = e.evaluate()["bbox"]
        assert check(res["AP"]) and check(res["AP50"]) and check(e.per_class_ap50["c0"]), (year, res)
    # ... and without detections it is 0 under both metrics
    assert voc.accumulate(np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.int64),
                          np.ones(1, np.uint8), 1, cases.IOU_THRS, False).tolist() == [[0.0] * T]


def test_voc_ap_equals_the_references(golden):
    for rec, prec, use07, want in golden["ap_checks"]:
        assert abs(voc.voc_ap(rec, prec, use07) - want) <= 1e-12, (rec, prec, use07)
    assert voc.voc_ap([], [], True) == 0.0 and voc.voc_ap([], [], False) == 0.0          # a class without detections


@pytest.mark.parametrize("year", [2007, 2012])
def test_evaluator_equals_the_references_result_dict(golden, year):
    inp = golden["inputs"]
    args = [torch.from_numpy(np.ascontiguousarray(inp[k])) for k in cases.INPUTS]
    for key, kw in ((year, dict(base_classes=golden["base"], novel_classes=golden["novel"])), ((year, "plain"), {})):
        e = voc.PascalVOCBoxEvaluator(golden["classes"], year=year, **kw)
        e.process_padded(*(x[:2].contiguous() for x in args))
        e.process_padded(*(x[2:].contiguous() for x in args))
        got, want = e.evaluate(), golden["results"][key]
        assert set(got) == {"bbox"} and set(got["bbox"]) == set(want)
        for k in want:
            print(year, k, got["bbox"][k], want[k])
            assert abs(got["bbox"][k] - want[k]) <= 1e-12, k
    assert set(golden["results"][year]) == {"AP", "AP50", "AP75", "bAP", "bAP50", "bAP75", "nAP", "nAP50", "nAP75"}
    assert set(golden["results"][(year, "plain")]) == {"AP", "AP50", "AP75"}
    assert list(e.per_class_ap50) == golden["classes"]


# ---- the two statements of the rules against each other

@pytest.mark.parametrize("name", cases.names())
def test_match_reference_equals_oracle(name):
    case = cases.get(name)
    got, want = reference(case), cases.expected(case)
    for k in cases.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %s" % (name, k, np.argwhere(got[k] != want[k])[:5].tolist())


def test_single_threshold_equals_oracle():
    case = cases.get("random_B2_K65_G70_L3_v0")
    got, want = reference(case, (0.6,)), cases.expected(case, (0.6,))
    for k in cases.OUTPUTS:
        assert np.array_equal(got[k], want[k]), k
    ten = reference(case)
    assert np.array_equal(got["tp"], (ten["tp"] >> np.uint32(2)) & np.uint32(1))


def test_random_cases_contain_what_they_are_for():
    """Over the random cases: detections on a difficult GT, duplicates on a taken GT, equal quantised scores inside one image
    and label, and corners that are ties of the "%.1f" round trip."""
    seen = dict(tp=0, duplicate=0, swallowed=0, score_tie=0, corner_tie=0)
    for case in cases.random_cases().values():
        out = cases.expected(case)
        qs = out["qscore"]
        for b in range(qs.shape[0]):
            nk, ng = min(max(int(case["n_keep"][b]), 0), qs.shape[1]), int(case["n_gt"][b])
            seen["tp"] += int(np.count_nonzero(out["tp"][b, :nk]))
            seen["swallowed"] += int(np.count_nonzero((out["tp"][b, :nk] | out["fp"][b, :nk]) != ALL))
            pairs = set()
            for k in range(nk):
                pair = (int(case["labels"][b, k]), float(qs[b, k]))
                seen["score_tie"] += pair in pairs
                pairs.add(pair)
            seen["corner_tie"] += int(np.count_nonzero(np.mod(case["xyxy"][b, :nk].astype(np.float64) * 20.0, 2.0) == 1.0))
            # a duplicate: an FP at 0.5 whose best GT (by the oracle's overlap) is one that a TP at 0.5 holds
            held = {int(j) for j in out["gt_of"][b, :nk, 0] if j >= 0}
            im = cases.images(case)[b]
            for k in range(nk):
                if out["fp"][b, k] & 1 and held:
                    bb = [float(v) for v in voc.quantise(case["scores"][b, k], case["xyxy"][b, k])[1]]
                    ovs = [(oracle.overlap(bb, gt[1]), -g, g) for g, gt in enumerate(im["gts"]) if gt[0] == case["labels"][b, k]]
                    if ovs and max(ovs)[0] > 0.5 and max(ovs)[2] in held:
                        seen["duplicate"] += 1
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("name", [n for n in cases.names() if n.startswith("random") and "_G0_" not in n])
@pytest.mark.parametrize("year", [2007, 2012])
def test_evaluator_equals_oracle_summary(name, year):
    case = cases.get(name)
    # the oracle states the protocol for classes with a countable GT: score the leading classes that have one
    countable = {int(c) for b in range(len(case["n_gt"])) for c, d in zip(case["gt_label"][b, :case["n_gt"][b]], case["gt_difficult"][b]) if not d}
    n = next(c for c in range(case["n_classes"] + 1) if c not in countable)
    assert n >= 1 and (n == case["n_classes"] or case["gt_label"].shape[1] < case["n_classes"]), (name, sorted(countable))
    case = dict(case, n_classes=n)
    names = ["c%d" % i for i in range(case["n_classes"])]
    base, novel = names[:1], names[1:]
    got = evaluator_of(case, year=year, base_classes=base, novel_classes=novel).evaluate()["bbox"]
    want = oracle.voc_summary(cases.images(case), names, year, base, novel)
    assert set(got) == set(want)
    for k in want:
        print(name, year, k, got[k], want[k])
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])


# ---- hand-built cases with known answers

def test_quantisation_is_the_text_round_trip():
    qs, box = voc.quantise(np.float32([0.0625, 0.1875, 0.4996, 0.5004]), np.float32([[1.25, 0.75, 10.25, 10.75]] * 4))
    assert qs.tolist() == [0.062, 0.188, 0.5, 0.5]                      # 62.5 -> 62 and 187.5 -> 188: nearest even
    assert box[0].tolist() == [2.2, 1.8, 10.2, 10.8]                    # 22.5 -> 22, 17.5 -> 18, 102.5 -> 102, 107.5 -> 108
    assert [float(f"{np.float32(v):.3f}") for v in (0.0625, 0.1875)] == [0.062, 0.188]
    assert float(f"{np.float32(10.25):.1f}") == 10.2 and float(f"{np.float32(10.75):.1f}") == 10.8
    qs, box = voc.quantise(np.float32(0.9), np.float32([8388607.5, 0, 8388617, 10]))
    assert np.float32(8388607.5) + np.float32(1) == np.float32(8388608) and 8388607.5 + 1 != 8388608      # the add rounds in fp32
    assert box.tolist() == [8388608.0, 1.0, 8388617.0, 10.0]
    out = reference(cases.get("quantisation_ties"))
    assert out["qscore"][0].tolist() == [0.062, 0.188]
    out = reference(cases.get("fp32_plus_one"))
    assert oracle.overlap([8388608.0, 1.0, 8388617.0, 10.0], [8388608.0, 1.0, 8388617.0, 19.0]) == 100.0 / 190.0
    assert oracle.overlap([8388608.5, 1.0, 8388617.0, 10.0], [8388608.0, 1.0, 8388617.0, 19.0]) == 0.5
    assert out["tp"][0, 0] == bits(0) and out["fp"][0, 0] == ALL & ~bits(0)


def test_overlap_exactly_on_a_threshold_is_a_miss():
    out = reference(cases.get("on_threshold"))
    assert oracle.overlap([1.0, 1.0, 10.0, 10.0], [1.0, 1.0, 10.0, 5.0]) == 0.5
    assert out["tp"][0, 0] == 0 and out["fp"][0, 0] == ALL and (out["gt_of"] == -1).all()


def test_first_of_two_gts_of_equal_overlap_wins():
    out = reference(cases.get("twin_gts"))
    assert out["tp"][0, 0] == ALL and out["fp"][0, 0] == 0 and (out["gt_of"][0, 0] == 0).all()


def test_duplicate_on_a_taken_gt_is_a_false_positive():
    out = reference(cases.get("duplicate"))
    # row 1 (0.8; 10 x 9 of the GT's 10 x 10 = 0.9) goes first and takes the GT up to 0.85; row 0 (0.6; the GT's own box) is a
    # duplicate there, and the first to clear 0.9 and 0.95
    assert out["tp"][0, 1] == bits(*range(8)) and out["fp"][0, 1] == bits(8, 9)
    assert out["tp"][0, 0] == bits(8, 9) and out["fp"][0, 0] == bits(*range(8))
    assert out["gt_of"][0, 0].tolist() == [-1] * 8 + [0, 0]


def test_difficult_gt_swallows_its_detections():
    out = reference(cases.get("difficult"))
    assert out["tp"][0, 0] == 0 and out["fp"][0, 0] == 0                     # overlap 1: swallowed at every threshold
    assert out["tp"][0, 1] == 0 and out["fp"][0, 1] == bits(6, 7, 8, 9)      # overlap 0.8: swallowed below it, an FP from 0.8 up
    assert out["tp"][0, 2] == ALL and out["gt_of"][0, 2].tolist() == [1] * T
    res = evaluator_of(cases.get("difficult")).evaluate()["bbox"]
    assert res["AP50"] == pytest.approx(100.0, abs=1e-9)                     # one countable GT, found, no FP in front of it


def test_labels_without_gt_and_out_of_range():
    out = reference(cases.get("label_without_gt"))
    assert out["tp"][0].tolist() == [0, ALL] and out["fp"][0].tolist() == [ALL, 0]
    out = reference(cases.get("label_out_of_range"))
    assert out["tp"][0].tolist() == [0, 0, ALL] and out["fp"][0].tolist() == [0, 0, 0] and out["qscore"][0].tolist() == [0.9, 0.8, 0.7]
    assert out["gt_of"][0, 2].tolist() == [1] * T


def test_empty_rows_and_no_gt():
    out = reference(cases.get("image_without_detections"))
    assert out["qscore"][0, 0] == 0 and out["tp"][0, 0] == 0 and out["fp"][0, 0] == 0 and out["tp"][1, 0] == ALL
    # one of the class's two GTs found without a false positive: precision 1 up to recall 0.5 -> 6 of the 11 points
    assert evaluator_of(cases.get("image_without_detections")).evaluate()["bbox"]["AP"] == pytest.approx(100.0 * 6 / 11, abs=1e-9)
    assert evaluator_of(cases.get("image_without_detections"), year=2012).evaluate()["bbox"]["AP"] == pytest.approx(50.0, abs=1e-9)
    out = reference(cases.get("n_keep_zero"))
    assert not out["qscore"].any() and not out["tp"].any() and not out["fp"].any() and (out["gt_of"] == -1).all()
    assert evaluator_of(cases.get("n_keep_zero")).evaluate()["bbox"] == {"AP": 0.0, "AP50": 0.0, "AP75": 0.0}
    out = reference(cases.get("no_gt_at_all"))
    assert cases.get("no_gt_at_all")["gt_label"].shape == (1, 0)
    assert out["tp"][0].tolist() == [0, 0] and out["fp"][0].tolist() == [ALL, ALL]
    out = reference(cases.get("counts_out_of_range"))
    assert out["tp"][0].tolist() == [ALL, 0] and out["fp"][0].tolist() == [0, ALL] and not out["fp"][1].any()


def test_equal_quantised_scores_go_in_row_order():
    out = reference(cases.get("equal_quantised_scores"))
    assert out["qscore"][0].tolist() == [0.5, 0.5, 0.5]
    assert out["tp"][0].tolist() == [ALL, 0, 0] and out["fp"][0].tolist() == [0, ALL, ALL]


def test_accumulate_keeps_processing_order_among_equal_scores():
    """Two images, one class, one detection each with the same quantised score: the first processed comes first, so an FP in the
    first image costs precision and one in the second does not."""
    gts = [[(0, 1, 1, 10, 10, 0)], [(0, 1, 1, 10, 10, 0)]]
    hit, miss = (0.5004, 0, 0, 0, 10, 10), (0.4996, 0, 100, 100, 110, 110)
    ap = {}
    for what, dets in (("fp_first", [[miss], [hit]]), ("tp_first", [[hit], [miss]])):
        e = voc.PascalVOCBoxEvaluator(["c0"], year=2012)
        e.process_padded(*cases.tensors(cases._case(what, cases.pad(dets, gts))))
        ap[what] = e.evaluate()["bbox"]["AP50"]
    assert ap["tp_first"] == pytest.approx(50.0, abs=1e-9) and ap["fp_first"] == pytest.approx(25.0, abs=1e-9)


# ---- the evaluator's surface

def test_base_and_novel_keys_only_when_given():
    case = cases.get("random_B2_K65_G70_L3_v0")
    plain = evaluator_of(case).evaluate()["bbox"]
    assert set(plain) == {"AP", "AP50", "AP75"}
    both = evaluator_of(case, base_classes=["c0", "c1"], novel_classes=["c2"])
    res = both.evaluate()["bbox"]
    assert set(res) == {"AP", "AP50", "AP75", "bAP", "bAP50", "bAP75", "nAP", "nAP50", "nAP75"}
    assert res["nAP50"] == both.per_class_ap50["c2"] and {k: res[k] for k in plain} == plain
    assert res["bAP50"] == pytest.approx((both.per_class_ap50["c0"] + both.per_class_ap50["c1"]) / 2, abs=1e-12)
    assert set(evaluator_of(case, base_classes=["c0"]).evaluate()["bbox"]) == {"AP", "AP50", "AP75", "bAP", "bAP50", "bAP75"}
    assert set(evaluator_of(case, base_classes=["elsewhere"]).evaluate()["bbox"]) == {"AP", "AP50", "AP75"}
    with pytest.raises(ValueError, match="2007 or 2012"):
        voc.PascalVOCBoxEvaluator(["c0"], year=2010)


def test_merge_of_two_evaluators_equals_one_over_both():
    case = cases.get("random_B2_K65_G70_L3_v0")
    whole = evaluator_of(case).evaluate()
    t = cases.tensors(case)
    names = ["c0", "c1", "c2"]
    a, b = voc.PascalVOCBoxEvaluator(names), voc.PascalVOCBoxEvaluator(names)
    a.process_padded(*(x[:1].contiguous() for x in t))
    b.process_padded(*(x[1:].contiguous() for x in t))
    assert a.merge(b).evaluate() == whole and evaluator_of(case, chunks=2).evaluate() == whole
    with pytest.raises(ValueError, match="differ"):
        a.merge(voc.PascalVOCBoxEvaluator(names, year=2012))
    a.reset()
    assert a.evaluate()["bbox"] == {"AP": 0.0, "AP50": 0.0, "AP75": 0.0}


def instances_of(case):
    from ziragroundingdino_amd.structures import Boxes, Instances

    inputs, outputs = [], []
    for b in range(case["scores"].shape[0]):
        n, g = int(case["n_keep"][b]), int(case["n_gt"][b])
        outputs.append({"instances": Instances((400, 400), pred_boxes=Boxes(torch.from_numpy(case["xyxy"][b, :n])),
                                               scores=torch.from_numpy(case["scores"][b, :n]),
                                               pred_classes=torch.from_numpy(case["labels"][b, :n]))})
        inputs.append({"annotations": [{"bbox": case["gt_xyxy"][b, i].tolist(), "category_id": int(case["gt_label"][b, i]),
                                        "difficult": int(case["gt_difficult"][b, i])} for i in range(g)]})
    return inputs, outputs


def test_process_reads_instances_and_annotations_through_inference_on_dataset():
    from ziragroundingdino_amd.evaluation import inference_on_dataset

    case = cases.get("random_B2_K65_G70_L3_v0")
    inputs, outputs = instances_of(case)

    class Fixed(torch.nn.Module):
        def forward(self, batch):
            return [outputs[inputs.index(x)] for x in batch]

    model = Fixed().train()
    e = voc.PascalVOCBoxEvaluator(["c0", "c1", "c2"])
    e.process_padded(*cases.tensors(cases.get("twin_gts")))            # (reset by the loop)
    got = inference_on_dataset(model, [inputs[:1], inputs[1:]], e)
    assert model.training and got == evaluator_of(case).evaluate()


def test_match_declines_cpu_tensors_and_the_evaluator_takes_the_reference():
    case = cases.get("twin_gts")
    assert not voc.match_supported(*cases.tensors(case), 1)
    with pytest.raises(RuntimeError, match="does not serve"):
        voc.match(*cases.tensors(case), 1)
    with pytest.raises(ValueError, match="match_reference"):
        voc.match_reference(*cases.tensors(case)[:7], torch.zeros(3, dtype=torch.int32), 1)


# ---- the task chain's keyword

def test_run_task_evaluate_keyword_takes_the_voc_evaluator(tmp_path):
    from test_tasks import _SliceModel
    from test_train_step import build_slice_model, slice_inputs

    from ziragroundingdino_amd.evaluation import inference_on_dataset
    from ziragroundingdino_amd.tasks import TaskSpec, multistep_lr_multiplier, run_task

    g = torch.load(os.path.join(GOLDEN, "tasks_zira_slice.pt"), weights_only=False)
    data = slice_inputs({"inputs": g["tasks"][0]["inputs"]}, None, "cpu")
    spec = TaskSpec(name="voc_10_10", categories_names=["c0", "c1", "c2"], data=lambda start: itertools.repeat(data), max_iter=1,
                    output_dir=str(tmp_path / "voc"), lr_multiplier=multistep_lr_multiplier(1))
    case = cases.get("random_B2_K65_G70_L3_v0")
    inputs, outputs = instances_of(case)

    class Tail(torch.nn.Module):
        """The trained model's detections are not what this test is about: a fixed tail stands in for them."""

        def __init__(self, model):
            super().__init__()
            self.model = model

        def forward(self, batch):
            return outputs

    def evaluate(model, s):
        e = voc.PascalVOCBoxEvaluator(s.categories_names, base_classes=["c0", "c1"], novel_classes=["c2"])
        return inference_on_dataset(Tail(model), [inputs], e)

    path, result = run_task(spec, lambda: build_slice_model(g, "cpu", _SliceModel), None, evaluate=evaluate)
    assert os.path.exists(path)
    assert result == evaluator_of(case, base_classes=["c0", "c1"], novel_classes=["c2"]).evaluate()
