"""COCO box AP without a GPU: hand-worked cases with known answers, then ``evaluation.match_reference`` and
``CocoBoxEvaluator`` against the loop-for-loop restatement of COCOeval in cocoeval_oracle.py (two independent statements of the
rules), ``merge``, and the ``evaluate=`` keyword of the task chain.  The same cases, with the same oracle outputs, are what
test_evaluation_gpu.py holds the kernel to."""
import itertools
import os

import numpy as np
import pytest
import torch

import cocoeval_oracle as oracle
import evaluation_cases as cases
from conftest import GOLDEN

from ziragroundingdino_amd import evaluation as ev

T = len(cases.IOU_THRS)
ALL_BITS = np.uint64((1 << (4 * T)) - 1)


def reference(case):
    return cases.as_numpy(ev.match_reference(*cases.tensors(case), cases.IOU_THRS, cases.AREA_RNGS, case["max_det"]))


def summary(case, chunks=1, evaluator=None):
    e = evaluator or ev.CocoBoxEvaluator(["c%d" % i for i in range(case["n_classes"])])
    t = cases.tensors(case)
    B = t[0].shape[0]
    for lo in range(0, B, -(-B // chunks)):
        e.process_padded(*(x[lo:lo + -(-B // chunks)].contiguous() for x in t))
    return e


def bit(a, t):
    return np.uint64(1) << np.uint64(a * T + t)


# ---- hand-worked cases

def test_perfect_detections_score_100_everywhere():
    res = summary(cases.get("perfect")).evaluate()["bbox"]
    assert set(res) == {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "AP-c0", "AP-c1"}
    for k, v in res.items():
        assert v == pytest.approx(100.0, abs=1e-9), k


def test_false_positive_in_front_of_the_true_positive_halves_ap50():
    res = summary(cases.get("fp_then_tp")).evaluate()["bbox"]
    assert res["AP50"] == pytest.approx(50.0, abs=1e-9) and res["AR1"] == 0.0 and res["AR10"] == pytest.approx(100.0)


def test_crowd_takes_every_detection_and_its_class_leaves_the_mean():
    case = cases.get("crowd")
    out = reference(case)
    of_crowd = case["labels"][0] == 0
    assert (out["matched"][0][of_crowd] == ALL_BITS).all() and (out["ignored"][0][of_crowd] == ALL_BITS).all()
    assert (out["gt_of"][0][of_crowd] == 0).all()
    assert out["gt_ignored"][0, 0] == 0b1111
    res = summary(case).evaluate()["bbox"]
    assert res["AP-c0"] == -1.0 and res["AP-c1"] == pytest.approx(100.0) and res["AP"] == pytest.approx(100.0)


def test_equal_iou_goes_to_the_later_gt():
    out = reference(cases.get("twins"))
    m = out["matched"][0, 0]
    assert m != 0
    for p in range(4 * T):
        assert out["gt_of"][0, 0, p] == (1 if (m >> np.uint64(p)) & np.uint64(1) else -1)
    assert (out["gt_of"][0, 0, :T] == 1).all()


def test_iou_exactly_on_the_threshold_matches():
    out = reference(cases.get("on_threshold"))
    assert oracle.box_iou([0.0, 0.0, 2.0, 1.0], [0.0, 0.0, 1.0, 1.0], 0) == 0.5
    assert out["matched"][0, 0] & bit(0, 0) and not out["matched"][0, 0] & bit(0, 1)
    assert out["gt_of"][0, 0, 0] == 0 and out["gt_of"][0, 0, 1] == -1


def test_gt_area_range_ends_are_inclusive():
    out = reference(cases.get("area_edges"))
    assert out["gt_ignored"][0, 0] == 0b1000      # 32 x 32: all, small and medium; not large
    assert out["gt_ignored"][0, 1] == 0b0010      # 96 x 96: all, medium and large; not small


def test_max_det_cuts_the_101st_detection():
    case = cases.get("max_det_cut")
    out = reference(case)
    assert case["max_det"] == 100 and out["rank"][0, 100] == 100 and out["rank"][0, 99] == 99
    assert out["matched"][0, 100] == 0 and out["ignored"][0, 100] == 0 and (out["gt_of"][0] == -1).all()
    assert summary(case).evaluate()["bbox"]["AR100"] == 0.0


def test_empty_row_and_no_gt():
    out = reference(cases.get("empty_row"))
    rng_bits = lambda *a: sum(int(bit(i, t)) for i in a for t in range(T))
    assert (out["rank"][0] == -1).all() and out["matched"][0, 0] == 0 and out["ignored"][0, 0] == 0 and (out["gt_of"][0] == -1).all()
    # the other image's detection is its 10 x 10 GT: matched everywhere, ignored with the GT in "medium" and "large"
    assert out["rank"][1, 0] == 0 and out["matched"][1, 0] == ALL_BITS and int(out["ignored"][1, 0]) == rng_bits(2, 3)
    assert (out["gt_of"][1, 0] == 0).all() and (out["gt_ignored"] == 0b1100).all()
    # one of the class's two GTs found by a detection without a false positive: precision 1 up to recall 0.5, 51 of 101 samples
    assert summary(cases.get("empty_row")).evaluate()["bbox"]["AP"] == pytest.approx(100.0 * 51 / 101, abs=1e-9)
    case = cases.get("no_gt")
    out = reference(case)
    assert out["gt_ignored"].shape == (1, 0) and (out["matched"] == 0).all() and (out["gt_of"] == -1).all()
    # unmatched: ignored exactly where the detection's own area leaves the range (10 x 10: medium, large; 40 x 40: small, large)
    assert int(out["ignored"][0, 0]) == rng_bits(2, 3) and int(out["ignored"][0, 1]) == rng_bits(1, 3)
    assert set(summary(case).evaluate()["bbox"].values()) == {-1.0}


# ---- the two statements of the rules against each other

@pytest.mark.parametrize("name", cases.names())
def test_match_reference_equals_oracle(name):
    case = cases.get(name)
    got, want = reference(case), cases.expected(case)
    for k in cases.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %s" % (name, k, np.argwhere(got[k] != want[k])[:5].tolist())


def test_random_cases_contain_what_they_are_for():
    """Each shape holds every situation it is able to hold (evaluation_cases.RANDOM_SHAPES says which and why), and all three
    occur: a tie on IoU between two available GTs, a crowd matched again, a rank >= max_det cut."""
    seen = set()
    for case in cases.random_cases().values():
        found = oracle.probe(cases.images(case), cases.IOU_THRS, cases.AREA_RNGS, case["max_det"])
        print(case["name"], found)
        for what in case["expects"]:
            assert found[what] > 0, (case["name"], what)
        seen.update(k for k, v in found.items() if v)
    assert seen == {"tie", "crowd_rematch", "cut"}


@pytest.mark.parametrize("name", cases.names())
def test_evaluator_equals_oracle_summary(name):
    case = cases.get(name)
    class_names = ["c%d" % i for i in range(case["n_classes"])]
    got = summary(case).evaluate()["bbox"]
    want = oracle.coco_summary(cases.images(case), class_names)
    assert set(got) == set(want)
    for k in want:
        print(name, k, got[k], want[k])
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])


def test_unsorted_rows_are_put_in_score_order():
    case = cases.get("random_B3_K65_G65_L2_v0")
    t = cases.tensors(case)
    perm = torch.stack([torch.randperm(65, generator=torch.Generator().manual_seed(b)) for b in range(3)])
    valid = torch.arange(65)[None, :] < t[3][:, None]
    # shuffle inside the valid part only; the oracle sorts the shuffled rows itself (stable, by -score), as the evaluator must
    key = torch.where(valid, perm, perm + 1000)
    order = torch.sort(key, dim=1)[1]
    shuffled = [torch.gather(t[0], 1, order), torch.gather(t[1], 1, order), torch.gather(t[2], 1, order[:, :, None].expand(3, 65, 4))]
    e = ev.CocoBoxEvaluator(["a", "b"])
    e.process_padded(*shuffled, *t[3:])
    got = e.evaluate()["bbox"]
    imgs = oracle.images_from_padded(*(x.numpy() for x in shuffled), *(x.numpy() for x in t[3:]))
    want = oracle.coco_summary(imgs, ["a", "b"])
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, k


def test_merge_of_two_halves_equals_one_evaluator():
    case = cases.get("random_B3_K65_G65_L2_v0")
    whole = summary(case).evaluate()
    t = cases.tensors(case)
    a, b = ev.CocoBoxEvaluator(["c0", "c1"]), ev.CocoBoxEvaluator(["c0", "c1"])
    a.process_padded(*(x[:2].contiguous() for x in t))
    b.process_padded(*(x[2:].contiguous() for x in t))
    assert a.merge(b).evaluate() == whole
    with pytest.raises(ValueError, match="differ"):
        a.merge(ev.CocoBoxEvaluator(["c0", "c1"], max_dets=(1, 10)))


def test_process_reads_instances_and_annotations():
    from ziragroundingdino_amd.structures import Boxes, Instances

    case = cases.get("random_B3_K65_G65_L2_v0")
    inputs, outputs = [], []
    for b in range(3):
        n, g = int(case["n_keep"][b]), int(case["n_gt"][b])
        outputs.append({"instances": Instances((400, 400), pred_boxes=Boxes(torch.from_numpy(case["xyxy"][b, :n])),
                                               scores=torch.from_numpy(case["scores"][b, :n]),
                                               pred_classes=torch.from_numpy(case["labels"][b, :n]))})
        inputs.append({"annotations": [dict({"bbox": case["gt_xywh"][b, i].tolist(), "category_id": int(case["gt_label"][b, i]),
                                             "iscrowd": int(case["gt_crowd"][b, i])},
                                            **({"area": float(case["gt_area"][b, i])} if i % 2 else {})) for i in range(g)]})
    e = ev.CocoBoxEvaluator(["c0", "c1"])
    e.process(inputs, outputs)
    assert e.evaluate() == summary(case).evaluate()


def test_pycocotools_agrees_with_the_oracle(tmp_path):
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval

    for case in cases.random_cases().values():
        imgs = cases.images(case)
        class_names = ["c%d" % i for i in range(case["n_classes"])]
        gt = COCO()
        anns = [{"id": 1 + i, "image_id": b, "category_id": g["category_id"], "bbox": g["bbox"], "area": g["area"], "iscrowd": g["iscrowd"]}
                for i, (b, g) in enumerate((b, g) for b, im in enumerate(imgs) for g in im["gts"])]
        gt.dataset = {"images": [{"id": b} for b in range(len(imgs))], "annotations": anns,
                      "categories": [{"id": c, "name": n} for c, n in enumerate(class_names)]}
        gt.createIndex()
        dts = [{"image_id": b, "category_id": d["category_id"], "bbox": d["bbox"], "score": d["score"]}
               for b, im in enumerate(imgs) for d in im["dts"]]
        if not dts:
            continue
        e = COCOeval(gt, gt.loadRes(dts), "bbox")
        e.evaluate(), e.accumulate(), e.summarize()
        want = oracle.coco_summary(imgs, class_names)
        for k, s in zip(("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100"), e.stats):
            assert abs((s * 100 if s > -1 else -1.0) - want[k]) <= 1e-12, (case["name"], k)


# ---- the task chain's keyword

def test_run_task_evaluate_keyword(tmp_path):
    from test_tasks import _SliceModel
    from test_train_step import build_slice_model, slice_inputs

    from ziragroundingdino_amd.tasks import TaskSpec, multistep_lr_multiplier, run_task, run_tasks

    g = torch.load(os.path.join(GOLDEN, "tasks_zira_slice.pt"), weights_only=False)
    data = slice_inputs({"inputs": g["tasks"][0]["inputs"]}, None, "cpu")
    build = lambda: build_slice_model(g, "cpu", _SliceModel)
    spec = lambda out: TaskSpec(name="a", categories_names=["fish"], data=lambda start: itertools.repeat(data), max_iter=2,
                                output_dir=str(tmp_path / out), lr_multiplier=multistep_lr_multiplier(1))
    plain = run_task(spec("plain"), build, None)
    assert plain == os.path.join(str(tmp_path / "plain"), "model_final.pth") and os.path.exists(plain)
    calls = []

    def evaluate(model, s):
        calls.append((s.name, model.training, float(model.rep_linear_adapter.weight.detach().abs().max())))
        return {"bbox": {"AP": 12.5}}

    path, result = run_task(spec("scored"), build, None, evaluate=evaluate)
    assert path == os.path.join(str(tmp_path / "scored"), "model_final.pth") and result == {"bbox": {"AP": 12.5}}
    assert calls == [("a", True, pytest.approx(1e-8))]        # called once, after the merge reset the branches
    a, b = torch.load(plain, weights_only=False)["model"], torch.load(path, weights_only=False)["model"]
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert set(a) == set(b) and all(k.startswith("prompt_memory_pool.") for k in differ), differ    # (pool entries: drawn afresh)
    assert run_tasks([spec("chain")], build, evaluate=None) == [os.path.join(str(tmp_path / "chain"), "model_final.pth")]
    assert run_tasks([spec("chain2")], build, evaluate=evaluate) == [(os.path.join(str(tmp_path / "chain2"), "model_final.pth"),
                                                                      {"bbox": {"AP": 12.5}})]
