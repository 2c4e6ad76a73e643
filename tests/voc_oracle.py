"""A helper, not a test: the Pascal VOC box AP protocol restated loop for loop in plain Python, from the rules alone -- the
second, independent statement that ``voc_evaluation`` (and through it the kernel) is held to.  It goes the long way round on
purpose: every detection becomes a line of text ("%.3f" score, "%.1f" corners after the fp32 ``+ 1`` on the top-left corner),
the lines are filed per class, parsed back with ``float()``, ordered by score (stable: equal scores stay in the order they
were filed), and walked one at a time against the class's GTs of the line's image with a ``det`` list per image.

An image is ``{"dts": [(score, label, (x0, y0, x1, y1)), ...], "gts": [(label, (x0, y0, x1, y1), difficult), ...]}`` with the
detections as np.float32 scalars in row order and the GT corners VOC's 1-based inclusive ones.
"""
import numpy as np

IOU_THRS = tuple(t / 100.0 for t in range(50, 100, 5))


def images_from_padded(scores, labels, xyxy, n_keep, gt_xyxy, gt_label, gt_difficult, n_gt):
    B, K = scores.shape
    G = gt_label.shape[1]
    images = []
    for b in range(B):
        nk, ng = min(max(int(n_keep[b]), 0), K), min(max(int(n_gt[b]), 0), G)
        dts = [(np.float32(scores[b, k]), int(labels[b, k]), tuple(np.float32(v) for v in xyxy[b, k])) for k in range(nk)]
        gts = [(int(gt_label[b, g]), tuple(float(v) for v in gt_xyxy[b, g]), bool(gt_difficult[b, g])) for g in range(ng)]
        images.append({"dts": dts, "gts": gts})
    return images


def line_of(image_id, row, score, box):
    """One line of a detection file; ``row`` rides along as a last column so that the verdict can be filed back."""
    xmin, ymin, xmax, ymax = (np.float32(v) for v in box)
    xmin = np.float32(xmin + np.float32(1))
    ymin = np.float32(ymin + np.float32(1))
    return f"{image_id} {np.float32(score):.3f} {xmin:.1f} {ymin:.1f} {xmax:.1f} {ymax:.1f} {row}"


def files(images, num_classes):
    """-> per class the list of lines, in processing order (image after image, row after row)."""
    out = [[] for _ in range(num_classes)]
    for image_id, im in enumerate(images):
        for row, (score, label, box) in enumerate(im["dts"]):
            if 0 <= label < num_classes:
                out[label].append(line_of(image_id, row, score, box))
    return out


def overlap(bb, gt):
    ixmin, iymin = max(gt[0], bb[0]), max(gt[1], bb[1])
    ixmax, iymax = min(gt[2], bb[2]), min(gt[3], bb[3])
    iw = max(ixmax - ixmin + 1.0, 0.0)
    ih = max(iymax - iymin + 1.0, 0.0)
    inters = iw * ih
    uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (gt[2] - gt[0] + 1.0) * (gt[3] - gt[1] + 1.0) - inters
    return inters / uni


def walk(lines, images, c, thr):
    """One class, one threshold.  -> per line, in FILE order: (image_id, row, confidence, "tp" | "fp" | "", gt index or -1),
    and the walk's order (indices into the file)."""
    recs = {}
    for image_id, im in enumerate(images):
        mine = [(g, gt) for g, gt in enumerate(im["gts"]) if gt[0] == c]
        recs[image_id] = {"index": [g for g, _ in mine], "bbox": [gt[1] for _, gt in mine],
                          "difficult": [gt[2] for _, gt in mine], "det": [False] * len(mine)}
    parsed = []
    for text in lines:
        cols = text.split(" ")
        parsed.append((int(cols[0]), int(cols[6]), float(cols[1]), [float(z) for z in cols[2:6]]))
    order = sorted(range(len(parsed)), key=lambda i: -parsed[i][2])
    verdict = [None] * len(parsed)
    for i in order:
        image_id, row, conf, bb = parsed[i]
        R = recs[image_id]
        ovmax, jmax = float("-inf"), -1
        for j, gt in enumerate(R["bbox"]):
            ov = overlap(bb, gt)
            if ov > ovmax:
                ovmax, jmax = ov, j
        what, which = "fp", -1
        if ovmax > thr:
            if R["difficult"][jmax]:
                what = ""
            elif not R["det"][jmax]:
                what, which = "tp", R["index"][jmax]
                R["det"][jmax] = True
        verdict[i] = (image_id, row, conf, what, which)
    return verdict, order


def ap_of(rec, prec, use_07_metric):
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            best = 0.0
            for r, p in zip(rec, prec):
                if r >= t and p > best:
                    best = p
            ap = ap + best / 11.0
        return ap
    mrec = [0.0] + list(rec) + [1.0]
    mpre = [0.0] + list(prec) + [0.0]
    for i in range(len(mpre) - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    ap = 0.0
    for i in range(len(mrec) - 1):
        if mrec[i + 1] != mrec[i]:
            ap += (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    return ap


def curve(verdict, order, npos):
    """rec, prec along the walk (npos > 0)."""
    rec, prec = [], []
    tp = fp = 0.0
    for i in order:
        tp += verdict[i][3] == "tp"
        fp += verdict[i][3] == "fp"
        rec.append(tp / float(npos))
        prec.append(tp / max(tp + fp, np.finfo(np.float64).eps))
    return rec, prec


def class_ap(images, lines, c, thr, use_07_metric):
    npos = sum(1 for im in images for gt in im["gts"] if gt[0] == c and not gt[2])
    verdict, order = walk(lines, images, c, thr)
    if npos == 0:
        raise ValueError("the oracle states the protocol for classes with a non-difficult GT only")
    rec, prec = curve(verdict, order, npos)
    return ap_of(rec, prec, use_07_metric), rec, prec


def match_outputs(images, K, num_classes, thrs=IOU_THRS):
    """The four arrays of ``voc_evaluation.match`` for a batch: qscore, tp, fp, gt_of."""
    B, T = len(images), len(thrs)
    qscore = np.zeros((B, K), np.float64)
    tp = np.zeros((B, K), np.uint32)
    fp = np.zeros((B, K), np.uint32)
    gt_of = np.full((B, K, T), -1, np.int32)
    for b, im in enumerate(images):
        for row, (score, _, _) in enumerate(im["dts"]):
            qscore[b, row] = float(f"{np.float32(score):.3f}")
    per_class = files(images, num_classes)
    for c in range(num_classes):
        for t, thr in enumerate(thrs):
            verdict, _ = walk(per_class[c], images, c, thr)
            for image_id, row, _, what, which in verdict:
                if what == "tp":
                    tp[image_id, row] |= np.uint32(1 << t)
                    gt_of[image_id, row, t] = which
                elif what == "fp":
                    fp[image_id, row] |= np.uint32(1 << t)
    return qscore, tp, fp, gt_of


def voc_summary(images, class_names, year=2007, base_classes=None, novel_classes=None, thrs=IOU_THRS):
    """The evaluator's result dict, percent, means taken as the reference takes them (per threshold over classes, then over
    thresholds).  Every class needs a non-difficult GT."""
    per_class = files(images, len(class_names))
    aps = {t: [] for t in range(len(thrs))}
    aps_base = {t: [] for t in range(len(thrs))}
    aps_novel = {t: [] for t in range(len(thrs))}
    for c, name in enumerate(class_names):
        for t, thr in enumerate(thrs):
            ap = class_ap(images, per_class[c], c, thr, year == 2007)[0] * 100
            aps[t].append(ap)
            if base_classes is not None and name in base_classes:
                aps_base[t].append(ap)
            if novel_classes is not None and name in novel_classes:
                aps_novel[t].append(ap)
    at = lambda v: [t for t, thr in enumerate(thrs) if abs(thr - v) < 1e-9][0]
    out = {}
    for prefix, table in (("", aps), ("b", aps_base), ("n", aps_novel)):
        if not table[0]:
            continue
        means = [float(np.mean(table[t])) for t in range(len(thrs))]
        out[prefix + "AP"] = float(np.mean(means))
        out[prefix + "AP50"], out[prefix + "AP75"] = means[at(0.5)], means[at(0.75)]
    return out
