#!/usr/bin/env python3
"""Golden vectors for Pascal VOC box AP: the REFERENCE's own ``PascalVOCDetectionEvaluator.process`` / ``evaluate`` and
``voc_eval`` / ``voc_ap`` (groundingdino/evaluation/pascal_voc_evaluation.py) on a handful of tiny annotation XMLs and the
detection files the reference writes itself, for both metrics (VOC 2007's 11 points, the envelope area) and all ten thresholds.
detectron2 is not installed here, so the three things the module takes from it are stubs: the metadata (set on the object), the
single-process ``comm`` and the table printer.  Recorded: the inputs in ``voc_evaluation.match``'s layout, per
(metric, class, threshold) ``rec`` / ``prec`` / ``ap``, and the evaluator's result dicts.
      python tests/golden/gen_voc_golden.py
"""
import importlib
import logging
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

CLASSES = ["aeroplane", "bicycle", "bird", "boat"]     # what the evaluator scores
GHOST = "ghost"                                         # a fifth name with difficult GTs only (npos == 0): voc_eval alone
BASE, NOVEL = ["aeroplane", "bicycle", "bird"], ["boat"]
N_IMAGES, K = 5, 14
THRESHOLDS = list(range(50, 100, 5))


def reference_module():
    ref_import.load()
    if not hasattr(np, "bool"):
        np.bool = bool                                  # the reference predates numpy 1.24
    for name, attrs in (("detectron2.data", dict(MetadataCatalog=None)),
                        ("detectron2.utils", {}),
                        ("detectron2.utils.comm", dict(gather=lambda x, dst=0: [x], is_main_process=lambda: True)),
                        ("detectron2.utils.logger", dict(create_small_table=lambda d: str(dict(d))))):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    sys.modules["detectron2.utils"].comm = sys.modules["detectron2.utils.comm"]
    pkg = types.ModuleType("groundingdino.evaluation")   # the package without its __init__ (COCO / LVIS evaluators)
    pkg.__path__ = [os.path.join(ref_import.REF, "groundingdino", "evaluation")]
    sys.modules["groundingdino.evaluation"] = pkg
    return importlib.import_module("groundingdino.evaluation.pascal_voc_evaluation")


def build_dataset():
    """Integer GT corners (as an XML holds them), fp32 detections off the grid: GT boxes jittered on a 1/8 grid, a duplicate of
    a found GT, boxes that lie nowhere; scores with distinct three decimals within each class."""
    rng = np.random.default_rng(2012)
    names = CLASSES + [GHOST]
    gts = []                                            # per image: (label, x0, y0, x1, y1, difficult)
    for b in range(N_IMAGES):
        n = int(rng.integers(3, 8)) if b != 3 else 0    # image 3 has no object at all
        rows = []
        for _ in range(n):
            x0, y0 = (int(v) for v in rng.integers(1, 200, 2))
            w, h = (int(v) for v in rng.integers(8, 120, 2))
            rows.append([int(rng.integers(0, len(CLASSES))), x0, y0, x0 + w, y0 + h, int(rng.random() < 0.2)])
        if b in (0, 2):
            rows.append([len(CLASSES), 30 + b, 40, 90, 120 + b, 1])      # the ghost class: difficult only
        gts.append(rows)
    for c in range(len(CLASSES)):                       # every scored class keeps a non-difficult GT
        assert any(r[0] == c and not r[5] for rows in gts for r in rows), c
    scores = np.zeros((N_IMAGES, K), np.float32)
    labels = np.zeros((N_IMAGES, K), np.int64)
    xyxy = np.zeros((N_IMAGES, K, 4), np.float32)
    n_keep = np.zeros(N_IMAGES, np.int32)
    thousandths = {c: list(rng.permutation(np.arange(20, 990))) for c in range(len(names))}
    for b in range(N_IMAGES):
        n = int(rng.integers(K // 2, K + 1)) if b != 1 else 0           # image 1 has no detection
        n_keep[b] = n
        for k in range(n):
            rows = gts[b]
            if rows and rng.random() < 0.75:            # near a GT (0-based corners = the annotation's minus one on the top left)
                label, x0, y0, x1, y1, _ = rows[int(rng.integers(0, len(rows)))]
                jitter = rng.integers(-40, 41, 4) / 8.0 * (1.0 if rng.random() < 0.6 else 4.0)
                box = np.array([x0 - 1, y0 - 1, x1, y1], np.float64) + jitter
            else:
                label = int(rng.integers(0, len(names)))
                x0, y0 = rng.integers(0, 1600, 2) / 8.0
                box = np.array([x0, y0, x0 + rng.integers(40, 800) / 8.0, y0 + rng.integers(40, 800) / 8.0])
            box[2], box[3] = max(box[2], box[0] + 1), max(box[3], box[1] + 1)
            labels[b, k], xyxy[b, k] = label, box
            scores[b, k] = thousandths[label].pop() / 1000.0 + rng.integers(-3, 4) / 8192.0
    return names, gts, scores, labels, xyxy, n_keep


class _Boxes:
    def __init__(self, t):
        self.tensor = t


class _Instances:
    def __init__(self, boxes, scores, classes):
        self.pred_boxes, self.scores, self.pred_classes = _Boxes(boxes), scores, classes

    def to(self, device):
        return self


def main():
    mod = reference_module()
    names, gts, scores, labels, xyxy, n_keep = build_dataset()
    ids = ["%06d" % (b + 1) for b in range(N_IMAGES)]
    with tempfile.TemporaryDirectory(prefix="voc_golden_") as root:
        os.makedirs(os.path.join(root, "Annotations"))
        os.makedirs(os.path.join(root, "ImageSets", "Main"))
        for image_id, rows in zip(ids, gts):
            objs = "".join("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
                           "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
                           % (names[r[0]], r[5], r[1], r[2], r[3], r[4]) for r in rows)
            with open(os.path.join(root, "Annotations", image_id + ".xml"), "w") as f:
                f.write("<annotation><filename>%s.jpg</filename>%s</annotation>" % (image_id, objs))
        with open(os.path.join(root, "ImageSets", "Main", "test.txt"), "w") as f:
            f.write("\n".join(ids) + "\n")

        def evaluator(year, class_names, base, novel):
            e = mod.PascalVOCDetectionEvaluator.__new__(mod.PascalVOCDetectionEvaluator)
            e._dataset_name = "voc_golden"
            e._anno_file_template = os.path.join(root, "Annotations", "{}.xml")
            e._image_set_path = os.path.join(root, "ImageSets", "Main", "test.txt")
            e._class_names, e._base_classes, e._novel_classes = class_names, base, novel
            e._is_2007 = year == 2007
            e._cpu_device = torch.device("cpu")
            e._logger = logging.getLogger("gen_voc_golden")
            e.reset()
            for b in range(N_IMAGES):
                n = int(n_keep[b])
                e.process([{"image_id": ids[b]}], [{"instances": _Instances(torch.from_numpy(xyxy[b, :n].copy()),
                                                                            torch.from_numpy(scores[b, :n].copy()),
                                                                            torch.from_numpy(labels[b, :n].copy()))}])
            return e

        results = {}
        for year in (2007, 2012):
            results[year] = {k: float(v) for k, v in evaluator(year, CLASSES, BASE, NOVEL).evaluate()["bbox"].items()}
            results[(year, "plain")] = {k: float(v) for k, v in evaluator(year, CLASSES, None, None).evaluate()["bbox"].items()}
        # the detection files as the reference's evaluate() writes them, for voc_eval on every name (the ghost included)
        e = evaluator(2007, names, None, None)
        for c, name in enumerate(names):
            lines = e._predictions.get(c, [""])
            triples = [ln.split(" ")[1] for ln in lines if ln]
            assert len(set(triples)) == len(triples), "class %s: equal 3-decimal scores make the reference's order ambiguous" % name
            with open(os.path.join(root, name + ".txt"), "w") as f:
                f.write("\n".join(lines))
        curves = {}
        with np.errstate(divide="ignore", invalid="ignore"):
            for use07 in (True, False):
                for c, name in enumerate(names):
                    for thresh in THRESHOLDS:
                        rec, prec, ap = mod.voc_eval(os.path.join(root, "{}.txt"), e._anno_file_template, e._image_set_path, name,
                                                     ovthresh=thresh / 100.0, use_07_metric=use07)
                        curves[(use07, c, thresh)] = (np.asarray(rec, np.float64), np.asarray(prec, np.float64), float(ap))
        ap_checks = [(np.array(r), np.array(p), u, float(mod.voc_ap(np.array(r), np.array(p), u)))
                     for r, p in (([0.5, 0.5, 1.0], [1.0, 0.5, 2 / 3]), ([], []), ([0.25, 0.25, 0.5], [1.0, 0.5, 2 / 3]))
                     for u in (True, False)]

    G = max(len(r) for r in gts)
    gt_xyxy = np.zeros((N_IMAGES, G, 4), np.float64)
    gt_label = np.zeros((N_IMAGES, G), np.int64)
    gt_difficult = np.zeros((N_IMAGES, G), np.uint8)
    for b, rows in enumerate(gts):
        for g, r in enumerate(rows):
            gt_label[b, g], gt_xyxy[b, g], gt_difficult[b, g] = r[0], r[1:5], r[5]
    path = os.path.join(HERE, "voc_eval.pt")
    torch.save(dict(names=names, classes=CLASSES, base=BASE, novel=NOVEL, thresholds=THRESHOLDS,
                    inputs=dict(scores=scores, labels=labels, xyxy=xyxy, n_keep=n_keep, gt_xyxy=gt_xyxy, gt_label=gt_label,
                                gt_difficult=gt_difficult, n_gt=np.array([len(r) for r in gts], np.int32)),
                    curves=curves, results=results, ap_checks=ap_checks), path)
    ghost = len(CLASSES)
    print("voc_eval %.1f KiB; detections" % (os.path.getsize(path) / 1024), n_keep.tolist(), "GTs", [len(r) for r in gts])
    print("AP50 per class, 2007:", [round(curves[(True, c, 50)][2], 4) for c in range(len(names))])
    print("ghost class (npos == 0): 2007 ->", curves[(True, ghost, 50)][2], " 2012 ->", curves[(False, ghost, 50)][2],
          " detections", len(curves[(True, ghost, 50)][0]))
    print("results 2007:", results[2007])
    print("final recall at 0.5 / 0.75 / 0.95:", [round(float(curves[(True, c, t)][0][-1]), 3) if len(curves[(True, c, t)][0]) else None
                                                 for c in range(len(CLASSES)) for t in (50, 75, 95)])


if __name__ == "__main__":
    main()
