"""Pascal VOC box AP behind the detections tail: what the reference gets from ``PascalVOCDetectionEvaluator`` -> ``voc_eval``
(groundingdino/evaluation/pascal_voc_evaluation.py; the incremental-VOC splits of datasets/incremental_voc.py, coco_wo_voc.py
and meta_pascal_voc.py), without the text files, the XML tree or detectron2 in between: AP / AP50 / AP75 over the classes, and
the base / novel split (``bAP*`` / ``nAP*``) an incremental-learning run reports.

VOC matching is not COCO matching (``evaluation.match``): the overlap counts inclusive pixels (+1), a detection is compared with
the best-overlapping GT of its class whether or not that GT is taken, a second hit on a taken GT is a false positive, a
``difficult`` GT swallows its detection, and -- because the reference pushes every detection through a text file -- the scores
and boxes that are matched are the quantised ones ("%.3f", "%.1f" after ``xmin += 1``).  ``match`` runs all of that for a whole
batch, every label and every threshold in one launch (csrc/vocmatch.hip, the rules stated at ``zira_voc_match`` in
include/zira_msda.h); ``match_reference`` is the same function in numpy fp64 on any device, for what ``match_supported``
declines, for CPU tensors and for the tests.  ``PascalVOCBoxEvaluator`` keeps the per-batch results on the device and reads
them back once, in ``evaluate()``, which is the reference's cumulative sums and ``voc_ap`` in numpy fp64.  The padding of a
batch and the read-back of the kept state are ``box_eval``'s; the overlap and the walk here are VOC's own and share nothing.

``tp`` / ``fp`` are int32 tensors that hold the 32 bits of the entry's u32 words (bit ``t``).
"""
import ctypes
import sys

import numpy as np
import torch

from . import _lib, box_eval

MAX_B, MAX_K, MAX_G, MAX_THRS = 65535, 1024, 1024, _lib.VOC_MAX_THRS
FORCE_REFERENCE = False     # True: PascalVOCBoxEvaluator matches with match_reference wherever it runs (tests, A/B)

DEFAULT_IOU_THRS = tuple(t / 100.0 for t in range(50, 100, 5))      # the reference's `thresh / 100.0`, value for value
_DET_DTYPES = (torch.float32, torch.int64, torch.float32, torch.int32)
_GT_DTYPES = (torch.float64, torch.int64, torch.uint8, torch.int32)


def _shapes_ok(dets, gts) -> bool:
    scores = dets[0]
    if not all(torch.is_tensor(t) for t in tuple(dets) + tuple(gts)) or scores.dim() != 2:
        return False
    B, K = scores.shape
    G = gts[1].shape[1] if gts[1].dim() == 2 else -1
    want = ((B, K), (B, K), (B, K, 4), (B,), (B, G, 4), (B, G), (B, G), (B,))
    return all(tuple(t.shape) == s for t, s in zip(tuple(dets) + tuple(gts), want))


def match_supported(scores, labels, xyxy, n_keep, gt_xyxy, gt_label, gt_difficult, n_gt, num_classes,
                    iou_thrs=DEFAULT_IOU_THRS) -> bool:
    """True where ``match`` runs the kernel: contiguous tensors of the entry's dtypes on one GPU, inside its limits."""
    dets, gts = (scores, labels, xyxy, n_keep), (gt_xyxy, gt_label, gt_difficult, n_gt)
    if not _shapes_ok(dets, gts) or not scores.is_cuda:
        return False
    if not all(t.dtype == d and t.device == scores.device and t.is_contiguous()
               for t, d in zip(dets + gts, _DET_DTYPES + _GT_DTYPES)):
        return False
    (B, K), G = scores.shape, gt_label.shape[1]
    return (1 <= B <= MAX_B and 1 <= K <= MAX_K and 0 <= G <= MAX_G and 1 <= len(iou_thrs) <= MAX_THRS
            and 1 <= int(num_classes) < 2 ** 31)


def match(scores, labels, xyxy, n_keep, gt_xyxy, gt_label, gt_difficult, n_gt, num_classes, iou_thrs=DEFAULT_IOU_THRS,
          with_gt_of=True):
    """``zira_voc_match`` on the current stream (one launch, nothing uploaded, the host never waits; capturable).
    Detections in any row order, the first ``n_keep[b]`` of a row valid, boxes the model's 0-based xyxy; ground truth padded to G
    per image (VOC's 1-based inclusive xyxy fp64, label int64, difficult uint8, ``n_gt`` int32).  Returns
    (qscore [B, K] float64, tp [B, K] int32, fp [B, K] int32, gt_of [B, K, T] int32 or None)."""
    if not match_supported(scores, labels, xyxy, n_keep, gt_xyxy, gt_label, gt_difficult, n_gt, num_classes, iou_thrs):
        raise RuntimeError("zira_voc_match does not serve these inputs (see voc_evaluation.match_supported)")
    thrs = [float(t) for t in iou_thrs]
    (B, K), G, T = scores.shape, gt_label.shape[1], len(thrs)
    lib = _lib.load()
    dev = scores.device
    qscore = torch.empty((B, K), dtype=torch.float64, device=dev)
    tp = torch.empty((B, K), dtype=torch.int32, device=dev)
    fp = torch.empty((B, K), dtype=torch.int32, device=dev)
    gt_of = torch.empty((B, K, T), dtype=torch.int32, device=dev) if with_gt_of else None
    c_thrs = (ctypes.c_double * T)(*thrs)
    ptr = lambda t: t.data_ptr() if G > 0 else None
    with torch.cuda.device(dev):
        rc = lib.zira_voc_match(scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(), n_keep.data_ptr(), B, K, ptr(gt_xyxy),
                                ptr(gt_label), ptr(gt_difficult), ptr(n_gt), G, c_thrs, T, int(num_classes), qscore.data_ptr(),
                                tp.data_ptr(), fp.data_ptr(), gt_of.data_ptr() if with_gt_of else None,
                                torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_voc_match failed: hipError %d" % rc)
    return qscore, tp, fp, gt_of


def quantise(scores, xyxy):
    """The text round trip of the reference's detection files on fp32 arrays, in fp64: -> (qs [...], box' [..., 4])."""
    s, box = np.asarray(scores, np.float32), np.asarray(xyxy, np.float32)
    qs = np.rint(s.astype(np.float64) * 1000.0) / 1000.0
    shifted = box.copy()
    shifted[..., :2] = box[..., :2] + np.float32(1.0)
    return qs, np.rint(shifted.astype(np.float64) * 10.0) / 10.0


def match_reference(scores, labels, xyxy, n_keep, gt_xyxy, gt_label, gt_difficult, n_gt, num_classes,
                    iou_thrs=DEFAULT_IOU_THRS, with_gt_of=True):
    """What ``match`` returns, computed on the host in numpy fp64 (tensors on any device; the results go back to it).  Per image
    the overlap matrix is formed at once; what was taken before a detection is a prefix OR over the detections of its GT."""
    dets, gts = (scores, labels, xyxy, n_keep), (gt_xyxy, gt_label, gt_difficult, n_gt)
    if not _shapes_ok(dets, gts):
        raise ValueError("match_reference: scores / labels [B, K], xyxy [B, K, 4], n_keep [B], gt_xyxy [B, G, 4], "
                         "gt_label / gt_difficult [B, G], n_gt [B]")
    thrs = np.array([float(t) for t in iou_thrs], np.float64)
    (B, K), G, T, C = scores.shape, gt_label.shape[1], len(thrs), int(num_classes)
    if not 1 <= T <= 32 or C < 1:
        raise ValueError("match_reference: 1 <= T <= 32, num_classes >= 1")
    dev = scores.device
    host = lambda t, dt: t.detach().cpu().numpy().astype(dt, copy=False)
    lab, nk_all = host(labels, np.int64), np.clip(host(n_keep, np.int64), 0, K)
    qs_all, box_all = quantise(host(scores, np.float32), host(xyxy, np.float32))
    gbox, glab, gdiff = host(gt_xyxy, np.float64), host(gt_label, np.int64), host(gt_difficult, np.uint8) != 0
    ng_all = np.clip(host(n_gt, np.int64), 0, G)
    weight = np.uint32(1) << np.arange(T, dtype=np.uint32)
    every = np.uint32(weight.sum(dtype=np.uint64))

    qscore = np.zeros((B, K), np.float64)
    tp = np.zeros((B, K), np.uint32)
    fp = np.zeros((B, K), np.uint32)
    gt_of = np.full((B, K, T), -1, np.int32)
    for b in range(B):
        nk, ng = int(nk_all[b]), int(ng_all[b])
        qscore[b, :nk] = qs_all[b, :nk]
        l = lab[b, :nk]
        counts = (l >= 0) & (l < C)
        x0, y0, x1, y1 = (box_all[b, :nk, i][:, None] for i in range(4))
        gx0, gy0, gx1, gy1 = (gbox[b, :ng, i][None, :] for i in range(4))
        iw = np.maximum(np.minimum(gx1, x1) - np.maximum(gx0, x0) + 1.0, 0.0)
        ih = np.maximum(np.minimum(gy1, y1) - np.maximum(gy0, y0) + 1.0, 0.0)
        inter = iw * ih
        uni = (x1 - x0 + 1.0) * (y1 - y0 + 1.0) + (gx1 - gx0 + 1.0) * (gy1 - gy0 + 1.0) - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            ov = np.where((l[:, None] == glab[b, :ng][None, :]) & counts[:, None], inter / uni, -np.inf)      # [nk, ng]
        if ng:
            jmax = np.argmax(ov, 1)                        # the FIRST of the best
            ovmax = ov[np.arange(nk), jmax]
        else:
            jmax, ovmax = np.zeros(nk, np.int64), np.full(nk, -np.inf)
        hit = ovmax[:, None] > thrs[None, :]               # [nk, T]
        order = np.argsort(-qs_all[b, :nk], kind="stable")
        took = np.zeros((ng, T), bool)
        for k in order:
            if not counts[k]:
                continue
            if not hit[k].any():
                fp[b, k] = every
                continue
            j = jmax[k]
            if gdiff[b, j]:
                fp[b, k] = weight[~hit[k]].sum(dtype=np.uint32)
                continue
            won = hit[k] & ~took[j]
            took[j] |= hit[k]
            tp[b, k] = weight[won].sum(dtype=np.uint32)
            fp[b, k] = every & ~tp[b, k]
            gt_of[b, k, won] = j
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(qscore), t(tp.view(np.int32)), t(fp.view(np.int32)), t(gt_of) if with_gt_of else None


def voc_ap(rec, prec, use_07_metric=False):
    """The reference's ``voc_ap``: the 11-point rule of VOC 2007, or the area under the precision envelope."""
    rec, prec = np.asarray(rec, np.float64), np.asarray(prec, np.float64)
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            at = rec >= t
            p = np.max(prec[at]) if np.sum(at) != 0 else 0
            ap = ap + p / 11.0
        return float(ap)
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]          # the envelope: a running maximum from the right
    i = np.where(mrec[1:] != mrec[:-1])[0]
    with np.errstate(invalid="ignore"):
        return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def accumulate(qscore, labels, tp, fp, gt_label, gt_difficult, num_classes, iou_thrs, use_07_metric, with_curves=False):
    """The second half of the reference's ``voc_eval`` on flat host arrays: the kept detections of the data set in processing
    order (qscore fp64, labels, tp / fp bit words) and its GTs (label, difficult).  Per class and threshold the detections are
    ordered by ``-qscore`` (stable: equal scores stay in processing order), tp and fp are cumulative sums,
    rec = tp / npos with npos the class's non-difficult GTs, prec = tp / max(tp + fp, eps).
    -> ap [C, T] (fractions); with ``with_curves`` also curves[c][t] = (rec, prec).

    A class without detections scores 0.  A class with ``npos == 0`` does what the reference's arithmetic does: rec = 0 / 0 is
    NaN throughout, so the 11-point rule finds no recall >= t and gives 0.0, while the envelope area multiplies NaN recall
    steps by zero precision and gives NaN (which then makes the means NaN, as in the reference); without detections it is 0."""
    T = len(iou_thrs)
    tp, fp = np.asarray(tp).view(np.uint32), np.asarray(fp).view(np.uint32)
    order = np.argsort(-qscore, kind="stable")        # once for all classes: a stable sort commutes with taking a subset
    labels, tp, fp = labels[order], tp[order], fp[order]
    ap = np.zeros((num_classes, T), np.float64)
    curves = []
    eps = np.finfo(np.float64).eps
    for c in range(num_classes):
        of_c = labels == c
        npos = int(np.count_nonzero((gt_label == c) & (gt_difficult == 0)))
        tp_c, fp_c = tp[of_c], fp[of_c]
        row = []
        for t in range(T):
            ctp = np.cumsum(((tp_c >> np.uint32(t)) & np.uint32(1)).astype(np.float64))
            cfp = np.cumsum(((fp_c >> np.uint32(t)) & np.uint32(1)).astype(np.float64))
            with np.errstate(divide="ignore", invalid="ignore"):
                rec = ctp / float(npos)
            prec = ctp / np.maximum(ctp + cfp, eps)
            ap[c, t] = voc_ap(rec, prec, use_07_metric)
            row.append((rec, prec))
        curves.append(row)
    return (ap, curves) if with_curves else ap


_STATE = ("qscore", "labels", "tp", "fp", "gt_label", "gt_difficult")


class PascalVOCBoxEvaluator(box_eval.BoxEvaluator):
    """detectron2's ``DatasetEvaluator`` surface (``reset`` / ``process`` / ``evaluate``) for Pascal VOC box AP, with the
    reference's base / novel split.  ``process`` pads the batch, matches it in one launch and keeps the result where it is;
    nothing is read back before ``evaluate()``."""
    _STATE, _WORDS, _WORD_DTYPE = _STATE, ("tp", "fp"), np.uint32

    def __init__(self, class_names, year=2007, base_classes=None, novel_classes=None, iou_thrs=None):
        if year not in (2007, 2012):
            raise ValueError("PascalVOCBoxEvaluator: year is 2007 or 2012, got %r" % (year,))
        self.class_names = list(class_names)
        self.year = int(year)
        self.base_classes = None if base_classes is None else list(base_classes)
        self.novel_classes = None if novel_classes is None else list(novel_classes)
        self.iou_thrs = tuple(float(t) for t in (DEFAULT_IOU_THRS if iou_thrs is None else iou_thrs))
        self.reset()

    def process_padded(self, scores, labels, xyxy, n_keep, gt_xyxy, gt_label, gt_difficult, n_gt):
        """One batch from raw tensors (``match``'s inputs; rows in any order: the matching orders them itself)."""
        qscore, tp, fp, _ = box_eval.match_batch(sys.modules[__name__], scores, labels, xyxy, n_keep, gt_xyxy, gt_label, gt_difficult,
                                                 n_gt, len(self.class_names), self.iou_thrs)
        self._batches.append(dict(qscore=qscore, labels=box_eval.mask_behind(labels, n_keep), tp=tp, fp=fp,
                                  gt_label=box_eval.mask_behind(gt_label, n_gt), gt_difficult=gt_difficult))

    def process(self, inputs, outputs):
        """``inputs``: the batched_inputs dicts, each with ``"annotations"`` (dicts: ``bbox`` xyxy in VOC's 1-based inclusive
        pixels as the annotation file has them, ``category_id`` the contiguous index, ``difficult``); ``outputs``: what the model
        returns in eval mode, ``[{"instances": Instances}]``."""
        dets = box_eval.pad_instances(outputs)
        gt_xyxy, _, gt_label, gt_difficult, n_gt = box_eval.pad_annotations(inputs, dets[0].device, "difficult", with_area=False)
        self.process_padded(*dets, gt_xyxy, gt_label, gt_difficult, n_gt)

    def merge(self, other):
        """Append another evaluator's state (a data-parallel run gathers its ranks' evaluators with this, in rank order)."""
        if (other.iou_thrs, other.year, other.class_names) != (self.iou_thrs, self.year, self.class_names):
            raise ValueError("merge: the evaluators differ in thresholds, year or classes")
        self._batches.extend(other._batches)
        return self

    def evaluate(self):
        host = self._gather()
        cat = lambda k, dt: box_eval.concat_state(host, k, dt)
        labels, gt_label = cat("labels", np.int64), cat("gt_label", np.int64)
        det, gt = labels >= 0, gt_label >= 0
        ap = accumulate(cat("qscore", np.float64)[det], labels[det], cat("tp", np.uint32)[det], cat("fp", np.uint32)[det],
                        gt_label[gt], cat("gt_difficult", np.uint8)[gt], len(self.class_names), self.iou_thrs, self.year == 2007)
        self.ap = ap                                    # [C, T], fractions
        pct = ap * 100
        thrs = np.asarray(self.iou_thrs)

        def block(prefix, members):
            rows = [c for c, name in enumerate(self.class_names) if members is None or name in members]
            if not rows:
                return {}
            per_thr = [np.mean([pct[c, t] for c in rows]) for t in range(len(thrs))]       # the reference's order of means
            out = {prefix + "AP": float(np.mean(per_thr))}
            for name, v in (("AP50", 0.5), ("AP75", 0.75)):
                at = np.where(np.isclose(thrs, v))[0]
                if len(at):
                    out[prefix + name] = float(per_thr[at[0]])
            return out

        res = block("", None)
        if self.base_classes is not None:
            res.update(block("b", self.base_classes))
        if self.novel_classes is not None:
            res.update(block("n", self.novel_classes))
        at50 = np.where(np.isclose(thrs, 0.5))[0]
        self.per_class_ap50 = {n: float(pct[c, at50[0]]) for c, n in enumerate(self.class_names)} if len(at50) else {}
        return {"bbox": res}
