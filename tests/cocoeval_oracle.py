"""A helper, not a test: COCOeval for boxes (``evaluateImg`` / ``accumulate`` / ``summarize``, ``useCats = 1``) restated loop
for loop in Python floats and numpy fp64, over lists of per-image dicts as the annotation files hold them.  It is written the
way pycocotools walks the problem -- one (image, category, area range) at a time, explicit scans, explicit sorts -- and on purpose
NOT the way ``ziragroundingdino_amd.evaluation`` states it (IoU matrices, all problems side by side, one global sort), so that
two independent statements of the same rules check each other.

An image is ``{"dts": [...], "gts": [...]}``;  a detection ``{"category_id", "bbox": [x, y, w, h], "score", "pos"}`` (``pos``: its
slot in the padded row, only used to lay results out);  a ground truth ``{"category_id", "bbox", "area", "iscrowd", "idx"}``."""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RNGS = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = [1, 10, 100]


def box_iou(d, g, crowd):
    """One detection box against one GT box, both xywh, in Python floats (IEEE doubles, every operation rounded on its own)."""
    da, ga = d[2] * d[3], g[2] * g[3]
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return float(np.float64(i) / np.float64(u))


def evaluate_img(dts, gts, area_rng, max_det, iou_thrs):
    """One image, one category, one area range.  None when both lists are empty."""
    if not dts and not gts:
        return None
    flag = [1 if (g["iscrowd"] or g["area"] < area_rng[0] or g["area"] > area_rng[1]) else 0 for g in gts]
    gts = [gts[i] for i in np.argsort(flag, kind="mergesort")]
    flag = sorted(flag)
    dts = [dts[i] for i in np.argsort([-d["score"] for d in dts], kind="mergesort")[:max_det]]
    T, G, D = len(iou_thrs), len(gts), len(dts)
    gt_taken = np.zeros((T, G), bool)
    dt_gt = -np.ones((T, D), np.int64)          # position in the SORTED gt list
    dt_ig = np.zeros((T, D), bool)
    for ti, t in enumerate(iou_thrs):
        for di, d in enumerate(dts):
            best, m = min(t, 1 - 1e-10), -1
            for gi, g in enumerate(gts):
                if gt_taken[ti, gi] and not g["iscrowd"]:
                    continue
                if m > -1 and flag[m] == 0 and flag[gi] == 1:
                    break
                iou = box_iou(d["bbox"], g["bbox"], g["iscrowd"])
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
        if area < area_rng[0] or area > area_rng[1]:
            for ti in range(T):
                if dt_gt[ti, di] == -1:
                    dt_ig[ti, di] = True
    return {"dts": dts, "gts": gts, "scores": [d["score"] for d in dts], "dt_gt": dt_gt, "dt_ig": dt_ig, "gt_ig": flag}


def evaluate(images, num_classes, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, max_det=MAX_DETS[-1]):
    """evalImgs[c][a][i], as COCOeval.evaluate lays them out."""
    return [[[evaluate_img([d for d in im["dts"] if d["category_id"] == c], [g for g in im["gts"] if g["category_id"] == c],
                           rng, max_det, iou_thrs) for im in images] for rng in area_rngs] for c in range(num_classes)]


def accumulate(eval_imgs, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS):
    C, A = len(eval_imgs), len(eval_imgs[0]) if eval_imgs else 0
    T, R, M = len(iou_thrs), len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, C, A, M))
    recall = -np.ones((T, C, A, M))
    for c in range(C):
        for a in range(A):
            for mi, max_det in enumerate(max_dets):
                E = [e for e in eval_imgs[c][a] if e is not None]
                if not E:
                    continue
                scores = np.concatenate([np.asarray(e["scores"][:max_det], np.float64) for e in E])
                order = np.argsort(-scores, kind="mergesort")
                dt_m = np.concatenate([e["dt_gt"][:, :max_det] >= 0 for e in E], axis=1)[:, order]
                dt_ig = np.concatenate([e["dt_ig"][:, :max_det] for e in E], axis=1)[:, order]
                gt_ig = np.concatenate([np.asarray(e["gt_ig"], np.int64) for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dt_m, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dt_m), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    q = [0.0] * R
                    recall[t, c, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side="left")):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, c, a, mi] = np.array(q)
    return precision, recall


def _stat(s):
    s = s[s > -1]
    return -1.0 if len(s) == 0 else float(np.mean(s))


def summarize(precision, recall, class_names, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """The twelve COCO numbers the evaluator reports plus per-class AP, in percent (-1 stays -1)."""
    iou_thrs = np.asarray(iou_thrs)

    def ap(thr=None, a=0):
        s = precision if thr is None else precision[np.where(np.isclose(iou_thrs, thr))[0]]
        return _stat(s[:, :, :, a, len(max_dets) - 1]) if a < precision.shape[3] else -1.0

    pct = lambda v: v * 100 if v > -1 else -1.0
    out = {"AP": pct(ap()), "AP50": pct(ap(0.5)), "AP75": pct(ap(0.75)), "APs": pct(ap(a=1)), "APm": pct(ap(a=2)),
           "APl": pct(ap(a=3))}
    for mi, m in enumerate(max_dets):
        out["AR%d" % m] = pct(_stat(recall[:, :, 0, mi]))
    for c, name in enumerate(class_names):
        out["AP-%s" % name] = pct(_stat(precision[:, :, c, 0, len(max_dets) - 1]))
    return out


def coco_summary(images, class_names, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, max_dets=MAX_DETS):
    ev = evaluate(images, len(class_names), iou_thrs, area_rngs, max_dets[-1])
    precision, recall = accumulate(ev, iou_thrs, REC_THRS, max_dets)
    return summarize(precision, recall, class_names, iou_thrs, max_dets)


# ---- between the padded tensors of ``evaluation.match`` and the per-image dicts

def images_from_padded(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_crowd, n_gt):
    """numpy arrays in ``match``'s layout -> the list of image dicts.  A detection's xywh is the reference's fp32
    ``BoxMode.convert(XYXY_ABS -> XYWH_ABS)`` followed by ``.tolist()``: w = fl32(x1 - x0) as a Python float."""
    images = []
    for b in range(scores.shape[0]):
        dts = []
        for k in range(int(n_keep[b])):
            x0, y0, x1, y1 = (np.float32(v) for v in xyxy[b, k])
            dts.append({"category_id": int(labels[b, k]), "score": float(scores[b, k]), "pos": k,
                        "bbox": [float(x0), float(y0), float(np.float32(x1 - x0)), float(np.float32(y1 - y0))]})
        gts = [{"category_id": int(gt_label[b, g]), "bbox": [float(v) for v in gt_xywh[b, g]], "area": float(gt_area[b, g]),
                "iscrowd": int(gt_crowd[b, g] != 0), "idx": g} for g in range(int(n_gt[b]))]
        images.append({"dts": dts, "gts": gts})
    return images


def match_outputs(images, K, G, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, max_det=100):
    """The five arrays ``evaluation.match`` returns, from ``evaluate_img`` over every (image, category, area range)."""
    B, T, A = len(images), len(iou_thrs), len(area_rngs)
    rank = -np.ones((B, K), np.int32)
    matched = np.zeros((B, K), np.uint64)
    ignored = np.zeros((B, K), np.uint64)
    gt_ignored = np.zeros((B, G), np.uint8)
    gt_of = -np.ones((B, K, A * T), np.int32)
    for b, im in enumerate(images):
        seen = {}
        for d in sorted(im["dts"], key=lambda d: d["pos"]):
            rank[b, d["pos"]] = seen.get(d["category_id"], 0)
            seen[d["category_id"]] = rank[b, d["pos"]] + 1
        for c in sorted({x["category_id"] for x in im["dts"] + im["gts"]}):
            for a, rng in enumerate(area_rngs):
                e = evaluate_img([d for d in im["dts"] if d["category_id"] == c],
                                 [g for g in im["gts"] if g["category_id"] == c], rng, max_det, iou_thrs)
                for g, ig in zip(e["gts"], e["gt_ig"]):
                    gt_ignored[b, g["idx"]] |= np.uint8(ig << a)
                for di, d in enumerate(e["dts"]):
                    for t in range(T):
                        bit = np.uint64(1) << np.uint64(a * T + t)
                        if e["dt_gt"][t, di] >= 0:
                            matched[b, d["pos"]] |= bit
                            gt_of[b, d["pos"], a * T + t] = e["gts"][e["dt_gt"][t, di]]["idx"]
                        if e["dt_ig"][t, di]:
                            ignored[b, d["pos"]] |= bit
    return rank, matched, ignored, gt_ignored, gt_of


def probe(images, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, max_det=100):
    """What a set of cases really exercises: {"tie": a detection whose winning IoU is shared by two available GTs of the same
    ignore class, "crowd_rematch": a crowd matched by a second detection at the same (a, t), "cut": a rank >= max_det}."""
    found = {"tie": 0, "crowd_rematch": 0, "cut": 0}
    for im in images:
        for c in sorted({x["category_id"] for x in im["dts"] + im["gts"]}):
            dts = [d for d in im["dts"] if d["category_id"] == c]
            gts = [g for g in im["gts"] if g["category_id"] == c]
            found["cut"] += max(0, len(dts) - max_det)
            for rng in area_rngs:
                e = evaluate_img(dts, gts, rng, max_det, iou_thrs)
                for t in range(len(iou_thrs)):
                    used = set()
                    for di, d in enumerate(e["dts"]):
                        m = int(e["dt_gt"][t, di])
                        if m < 0:
                            continue
                        won = box_iou(d["bbox"], e["gts"][m]["bbox"], e["gts"][m]["iscrowd"])
                        for gi, g in enumerate(e["gts"]):
                            free = g["iscrowd"] or gi not in used
                            if gi != m and free and e["gt_ig"][gi] == e["gt_ig"][m] and box_iou(d["bbox"], g["bbox"], g["iscrowd"]) == won:
                                found["tie"] += 1
                        if m in used and e["gts"][m]["iscrowd"]:
                            found["crowd_rematch"] += 1
                        used.add(m)
    return found
