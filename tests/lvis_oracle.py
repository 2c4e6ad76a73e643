"""A helper, not a test: LVIS box AP matching (lvis-api's ``LVISResults.limit_dets_per_image``, ``LVISEval._prepare`` and
``LVISEval.evaluate_img``) restated loop for loop in Python floats, over lists of per-image dicts as the annotation files hold
them, with Python sets for an image's positive, negative and not-exhaustive categories.  It is written the way lvis-api walks the
problem -- one image cut, one (image, category, area range) at a time, explicit scans, explicit stable sorts -- and on purpose NOT
the way ``ziragroundingdino_amd.lvis_evaluation`` states it (bitsets, IoU matrices, all problems side by side), so that two
independent statements of the same rules check each other.

An image is ``{"dts": [...], "gts": [...], "neg": set, "nel": set}``;  a detection ``{"category_id", "bbox": [x, y, w, h],
"score", "pos"}`` (``pos``: its slot in the padded row, only used to lay results out);  a ground truth ``{"category_id", "bbox",
"area", "ignore", "idx"}``."""
import numpy as np

from cocoeval_oracle import AREA_RNGS, IOU_THRS  # noqa: F401  (LVISEval's Params hold the same two tables)

MAX_DETS = 300


def box_iou(d, g):
    """One detection box against one GT box, both xywh, in Python floats (IEEE doubles, every operation rounded on its own);
    LVIS has no crowd, so the union is always the plain one."""
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] + g[2] * g[3] - i
    return float(np.float64(i) / np.float64(u))


def limit_dets(dts, max_det):
    """LVISResults: the image's detections of all categories in stable descending score order, the first ``max_det`` of them."""
    order = np.argsort([-d["score"] for d in dts], kind="mergesort")
    return [dts[i] for i in order[:max_det]]


def prepare(image, num_classes, max_det):
    """-> (dts by category, gts by category): the cut, then only detections of a category of the dataset that is in the image's
    positive set (the categories of its GTs, ignored ones included) or in its negative set."""
    pos = {g["category_id"] for g in image["gts"]}
    dts, gts = {}, {}
    for d in limit_dets(image["dts"], max_det):
        c = d["category_id"]
        if not 0 <= c < num_classes:
            continue
        if c not in image["neg"] and c not in pos:
            continue
        dts.setdefault(c, []).append(d)
    for g in image["gts"]:
        if 0 <= g["category_id"] < num_classes:
            gts.setdefault(g["category_id"], []).append(g)
    return dts, gts


def evaluate_img(dts, gts, area_rng, iou_thrs, not_exhaustive):
    """One image, one category, one area range.  ``not_exhaustive``: the category is in the image's not-exhaustive set."""
    flag = [1 if (g["ignore"] or g["area"] < area_rng[0] or g["area"] > area_rng[1]) else 0 for g in gts]
    order = np.argsort(flag, kind="mergesort")
    gts = [gts[i] for i in order]
    flag = [flag[i] for i in order]
    dts = [dts[i] for i in np.argsort([-d["score"] for d in dts], kind="mergesort")]
    T, G, D = len(iou_thrs), len(gts), len(dts)
    gt_taken = np.zeros((T, G), bool)
    dt_gt = -np.ones((T, D), np.int64)          # position in the SORTED gt list
    dt_ig = np.zeros((T, D), bool)
    for ti, t in enumerate(iou_thrs):
        for di, d in enumerate(dts):
            best, m = min(t, 1 - 1e-10), -1
            for gi, g in enumerate(gts):
                if gt_taken[ti, gi]:
                    continue
                if m > -1 and flag[m] == 0 and flag[gi] == 1:
                    break
                iou = box_iou(d["bbox"], g["bbox"])
                if iou < best:
                    continue
                best, m = iou, gi
            if m == -1:
                continue
            dt_ig[ti, di] = bool(flag[m])
            dt_gt[ti, di] = m
            gt_taken[ti, m] = True
    for di, d in enumerate(dts):
        area = d["bbox"][2] * d["bbox"][3]
        if area < area_rng[0] or area > area_rng[1] or not_exhaustive:
            for ti in range(T):
                if dt_gt[ti, di] == -1:
                    dt_ig[ti, di] = True
    return {"dts": dts, "gts": gts, "dt_gt": dt_gt, "dt_ig": dt_ig, "gt_ig": flag}


def images_from_padded(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg, nel):
    """numpy arrays in ``lvis_evaluation.match``'s layout (counts clamped as the entry clamps them) plus per-image id lists ->
    the list of image dicts.  A detection's xywh is the reference's fp32 ``BoxMode.convert(XYXY_ABS -> XYWH_ABS)`` followed by
    ``.tolist()``: w = fl32(x1 - x0) as a Python float."""
    images = []
    K, G = scores.shape[1], gt_label.shape[1]
    for b in range(scores.shape[0]):
        dts = []
        for k in range(min(max(int(n_keep[b]), 0), K)):
            x0, y0, x1, y1 = (np.float32(v) for v in xyxy[b, k])
            dts.append({"category_id": int(labels[b, k]), "score": float(scores[b, k]), "pos": k,
                        "bbox": [float(x0), float(y0), float(np.float32(x1 - x0)), float(np.float32(y1 - y0))]})
        gts = [{"category_id": int(gt_label[b, g]), "bbox": [float(v) for v in gt_xywh[b, g]], "area": float(gt_area[b, g]),
                "ignore": int(gt_ignore[b, g] != 0), "idx": g} for g in range(min(max(int(n_gt[b]), 0), G) if G else 0)]
        images.append({"dts": dts, "gts": gts, "neg": set(int(c) for c in neg[b]), "nel": set(int(c) for c in nel[b])})
    return images


def match_outputs(images, K, G, num_classes, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, max_det=MAX_DETS):
    """The five arrays ``lvis_evaluation.match`` returns, from ``evaluate_img`` over every (image, category, area range)."""
    B, T, A = len(images), len(iou_thrs), len(area_rngs)
    rank = -np.ones((B, K), np.int32)
    matched = np.zeros((B, K), np.uint64)
    ignored = np.zeros((B, K), np.uint64)
    gt_ignored = np.zeros((B, G), np.uint8)
    gt_of = -np.ones((B, K, A * T), np.int32)
    for b, im in enumerate(images):
        dts, gts = prepare(im, num_classes, max_det)
        for c, ds in dts.items():
            for i, d in enumerate(sorted(ds, key=lambda d: d["pos"])):
                rank[b, d["pos"]] = i
        for a, rng in enumerate(area_rngs):         # a GT's flag is its own, whatever its category
            for g in im["gts"]:
                if g["ignore"] or g["area"] < rng[0] or g["area"] > rng[1]:
                    gt_ignored[b, g["idx"]] |= np.uint8(1 << a)
        for c in sorted(set(dts) | set(gts)):
            for a, rng in enumerate(area_rngs):
                e = evaluate_img(dts.get(c, []), gts.get(c, []), rng, iou_thrs, c in im["nel"])
                for di, d in enumerate(e["dts"]):
                    for t in range(T):
                        bit = np.uint64(1) << np.uint64(a * T + t)
                        if e["dt_gt"][t, di] >= 0:
                            matched[b, d["pos"]] |= bit
                            gt_of[b, d["pos"], a * T + t] = e["gts"][e["dt_gt"][t, di]]["idx"]
                        if e["dt_ig"][t, di]:
                            ignored[b, d["pos"]] |= bit
    return rank, matched, ignored, gt_ignored, gt_of
