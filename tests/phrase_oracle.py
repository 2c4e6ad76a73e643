"""The phrase-grounding matching as plain Python loops, one phrase at a time, written from the definition (include/zira_phrase.h,
the issue's rules) and sharing no code with ziragroundingdino_amd.phrase_evaluation.  fp32 steps are numpy float32 scalars, one
operation at a time; the IoU is Python floats (C doubles), one operation at a time."""
import math

import numpy as np

F = np.float32
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _fmax(a, b):            # C's fmax / fmaxf: the other operand where one is a NaN
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def phrase_tokens(words, T):
    """The tokens below T whose bit is set in the int32 mask words."""
    return [t for t in range(T) if (int(words[t // 32]) >> (t % 32)) & 1]


def score(row, tokens):
    """The maximum over the phrase's tokens; NaN where one of them is a NaN; one zero."""
    best = None
    for t in tokens:
        v = row[t]
        if v != v:
            return NAN32
        if best is None or v > best:
            best = v
    return F(0.0) if best == 0 else F(best)


def ranking(scores):
    """Stable descending order: NaN in front, then the values descending, equal values (-0.0 == 0.0) by ascending index."""
    nans = [q for q, s in enumerate(scores) if s != s]
    rest = [q for q, s in enumerate(scores) if s == s]
    rest.sort(key=lambda q: -float(scores[q]))            # Python's sort is stable
    return nans + rest


def pixel_box(box, img_h, img_w):
    """cxcywh in 0..1 -> clipped corners, the detections tail's chain at scale 1, every step rounded to fp32."""
    cx, cy, w, h = (F(v) for v in box)
    with np.errstate(all="ignore"):
        hw, hh = F(F(0.5) * w), F(F(0.5) * h)
        raw = (F(F(cx - hw) * img_w), F(F(cy - hh) * img_h), F(F(cx + hw) * img_w), F(F(cy + hh) * img_h))
    hi = (img_w, img_h, img_w, img_h)
    return tuple(_fmin(_fmax(v, F(0.0)), m) for v, m in zip(raw, hi))


def iou(a, g):
    x0, y0, x1, y1 = (float(v) for v in a)
    gx0, gy0, gx1, gy1 = (float(v) for v in g)
    area = (x1 - x0) * (y1 - y0)
    gt_area = (gx1 - gx0) * (gy1 - gy0)
    w = _fmin(x1, gx1) - _fmax(x0, gx0)
    h = _fmin(y1, gy1) - _fmax(y0, gy0)
    if not (w > 0.0 and h > 0.0):
        return 0.0
    inter = w * h
    union = area + gt_area - inter
    try:
        q = inter / union
    except ZeroDivisionError:
        q = math.inf if inter > 0 else math.nan
    return 0.0 if q != q else q


def union_box(boxes):
    u = list(boxes[0])
    for g in boxes[1:]:
        u = [_fmin(u[0], g[0]), _fmin(u[1], g[1]), _fmax(u[2], g[2]), _fmax(u[3], g[3])]
    return u


def match(prob, boxes, sizes, phrase_bits, gt_boxes, gt_count, k_max, iou_thrs, merged):
    """numpy arrays in (prob [B, Q, T] f32, boxes [B, Q, 4] f32, sizes [B, 2] f32, phrase_bits [B, P, W] i32, gt_boxes
    [B, P, G, 4] f32, gt_count [B, P] i32) -> dict of numpy arrays, the five outputs."""
    B, Q, T = prob.shape
    P, G = phrase_bits.shape[1], gt_boxes.shape[2]
    K, N = int(k_max), len(iou_thrs)
    out = dict(top_query=np.full((B, P, K), -1, np.int32), top_score=np.zeros((B, P, K), np.float32),
               top_iou=np.zeros((B, P, K), np.float64), first_hit=np.full((B, P, N), K, np.int32), valid=np.zeros((B, P), np.uint8))
    for b in range(B):
        img_h, img_w = F(sizes[b, 0]), F(sizes[b, 1])
        for p in range(P):
            tokens = phrase_tokens(phrase_bits[b, p], T)
            n_gt = min(max(int(gt_count[b, p]), 0), G)
            if not tokens or n_gt == 0:
                continue
            out["valid"][b, p] = 1
            scores = [score(prob[b, q], tokens) for q in range(Q)]
            gts = [list(gt_boxes[b, p, g]) for g in range(n_gt)]
            if merged:
                gts = [union_box(gts)]
            for r, q in enumerate(ranking(scores)[:K]):
                cand = pixel_box(boxes[b, q], img_h, img_w)
                best = 0.0
                for g in gts:
                    v = iou(cand, g)
                    if v > best:
                        best = v
                out["top_query"][b, p, r], out["top_score"][b, p, r], out["top_iou"][b, p, r] = q, scores[q], best
                for i, thr in enumerate(iou_thrs):
                    if best >= float(thr) and out["first_hit"][b, p, i] == K:
                        out["first_hit"][b, p, i] = r
    return out
