"""COCO box AP behind the detections tail: what the reference gets from ``COCOEvaluator`` -> ``pycocotools.COCOeval``
(groundingdino/evaluation/coco_evaluation.py:13, :207-268, :288, :312; every ODinW config's ``dataloader.evaluator``), without
pycocotools, detectron2 or a JSON file in between.

The hot part of COCOeval is ``evaluateImg``: per (image, category, area range, IoU threshold) a greedy, order-dependent matching
of up to 100 detections against the image's ground truth.  ``match`` runs it for a whole batch in one launch where the
detections already are (csrc/apmatch.hip, the rules stated at ``zira_ap_match`` in include/zira_msda.h); ``match_reference`` is
the same function in numpy fp64 on any device, for what ``match_supported`` declines, for CPU tensors and for the tests.
The padding of a batch, the score order, the kept state's read-back, the greedy walk of ``match_reference`` and the dataset
loop are ``box_eval``'s, shared with the LVIS, VOC and phrase evaluators; this module holds what is COCO's own.
``CocoBoxEvaluator`` keeps the per-batch results on the device until ``evaluate()``, which is pycocotools' ``accumulate`` +
``summarize``: ``accumulate_device`` fills the precision / recall tables where the state is (csrc/apaccum.hip, one launch, the
rules stated at ``zira_ap_accumulate``) and only the tables are read back; ``accumulate`` is the same function in numpy fp64 on
the host -- the same bits -- for what ``accumulate_supported`` declines; ``summarize`` works on the small tables.  The arithmetic is pycocotools' throughout -- IoU and areas in fp64
from the fp32 xyxy -> xywh conversion the reference's ``instances_to_coco_json`` does; the one deliberate difference from a
round trip through pycocotools is the input: tensors instead of files.

``matched`` / ``ignored`` are int64 tensors that hold the 64 bits of the entry's u64 words (bit ``a * T + t``).
"""
import ctypes
import sys

import numpy as np
import torch

from . import _lib, box_eval

MAX_B, MAX_K, MAX_G, MAX_BITS = 65535, 1024, 1024, 64
MAX_THRS, MAX_AREAS = _lib.AP_MAX_THRS, _lib.AP_MAX_AREAS
MAX_DETS, MAX_RECS, MAX_CLASSES, MAX_N = _lib.AP_MAX_DETS, _lib.AP_MAX_RECS, _lib.AP_MAX_CLASSES, 2 ** 31 - 1
FORCE_REFERENCE = False     # True: CocoBoxEvaluator matches with match_reference and accumulates on the host (tests, A/B)

DEFAULT_IOU_THRS = tuple(np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True).tolist())
DEFAULT_REC_THRS = tuple(np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True).tolist())
DEFAULT_AREA_RNGS = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))   # all, small, medium, large
_DET_DTYPES = (torch.float32, torch.int64, torch.float32, torch.int32)
_GT_DTYPES = (torch.float64, torch.float64, torch.int64, torch.uint8, torch.int32)


def _params(iou_thrs, area_rngs, max_det):
    thrs = [float(t) for t in iou_thrs]
    rngs = [(float(lo), float(hi)) for lo, hi in area_rngs]
    return thrs, rngs, int(max_det)


def _limits(B, K, G, T, A, max_det) -> bool:
    return (1 <= B <= MAX_B and 1 <= K <= MAX_K and 0 <= G <= MAX_G and 1 <= max_det <= K and 1 <= T <= MAX_THRS
            and 1 <= A <= MAX_AREAS and A * T <= MAX_BITS)


def _shapes_ok(dets, gts) -> bool:
    scores, labels, xyxy, n_keep = dets
    if not all(torch.is_tensor(t) for t in tuple(dets) + tuple(gts)) or scores.dim() != 2:
        return False
    B, K = scores.shape
    G = gts[2].shape[1] if gts[2].dim() == 2 else -1
    want = ((B, K), (B, K), (B, K, 4), (B,), (B, G, 4), (B, G), (B, G), (B, G), (B,))
    return all(tuple(t.shape) == s for t, s in zip(tuple(dets) + tuple(gts), want))


def match_supported(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_crowd, n_gt, iou_thrs=DEFAULT_IOU_THRS,
                    area_rngs=DEFAULT_AREA_RNGS, max_det=100) -> bool:
    """True where ``match`` runs the kernel: contiguous tensors of the entry's dtypes on one GPU, inside its limits."""
    dets, gts = (scores, labels, xyxy, n_keep), (gt_xywh, gt_area, gt_label, gt_crowd, n_gt)
    if not _shapes_ok(dets, gts) or not scores.is_cuda:
        return False
    if not all(t.dtype == d and t.device == scores.device and t.is_contiguous()
               for t, d in zip(dets + gts, _DET_DTYPES + _GT_DTYPES)):
        return False
    return _limits(scores.shape[0], scores.shape[1], gt_label.shape[1], len(iou_thrs), len(area_rngs), int(max_det))


def match(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_crowd, n_gt, iou_thrs=DEFAULT_IOU_THRS,
          area_rngs=DEFAULT_AREA_RNGS, max_det=100, with_gt_of=True):
    """``zira_ap_match`` on the current stream (one launch, nothing uploaded, the host never waits; capturable).
    Detections as ``topk.detections`` returns them -- rows in non-increasing score order, the first ``n_keep[b]`` valid --
    and ground truth padded to G per image (xywh and area fp64, label int64, crowd uint8, ``n_gt`` int32).  Returns
    (rank [B, K] int32, matched [B, K] int64, ignored [B, K] int64, gt_ignored [B, G] uint8, gt_of [B, K, A T] int32 or None)."""
    if not match_supported(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_crowd, n_gt, iou_thrs, area_rngs, max_det):
        raise RuntimeError("zira_ap_match does not serve these inputs (see evaluation.match_supported)")
    thrs, rngs, max_det = _params(iou_thrs, area_rngs, max_det)
    (B, K), G, T, A = scores.shape, gt_label.shape[1], len(thrs), len(rngs)
    lib = _lib.load()
    (rank, matched, ignored, gt_ignored, gt_of), c_thrs, c_rngs, ptr = box_eval.match_launch(scores, G, thrs, rngs, with_gt_of)
    with torch.cuda.device(scores.device):
        rc = lib.zira_ap_match(scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(), n_keep.data_ptr(), B, K, ptr(gt_xywh),
                               ptr(gt_area), ptr(gt_label), ptr(gt_crowd), ptr(n_gt), G, c_thrs, T, c_rngs, A, max_det,
                               rank.data_ptr(), matched.data_ptr(), ignored.data_ptr(), ptr(gt_ignored),
                               gt_of.data_ptr() if with_gt_of else None, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_ap_match failed: hipError %d" % rc)
    return rank, matched, ignored, gt_ignored, gt_of


def match_reference(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_crowd, n_gt, iou_thrs=DEFAULT_IOU_THRS,
                    area_rngs=DEFAULT_AREA_RNGS, max_det=100, with_gt_of=True):
    """What ``match`` returns, computed on the host in numpy fp64 (tensors on any device; the results go back to it): per image
    ``box_eval.match_image`` under COCO's rules -- a crowd GT may be taken again and its union is the detection's area -- for
    the detections inside the per-class ``max_det``."""
    dets, gts = (scores, labels, xyxy, n_keep), (gt_xywh, gt_area, gt_label, gt_crowd, n_gt)
    if not _shapes_ok(dets, gts):
        raise ValueError("match_reference: scores / labels [B, K], xyxy [B, K, 4], n_keep [B], gt_xywh [B, G, 4], "
                         "gt_area / gt_label / gt_crowd [B, G], n_gt [B]")
    thrs, rngs, max_det = _params(iou_thrs, area_rngs, max_det)
    (B, K), G, T, A = scores.shape, gt_label.shape[1], len(thrs), len(rngs)
    if not 1 <= max_det or A * T > MAX_BITS or A < 1 or T < 1:
        raise ValueError("match_reference: max_det >= 1, 1 <= A T <= 64")
    lab, box, nk_all, gbox, garea, glab, gcrowd, ng_all = box_eval.reference_inputs(*dets[1:], *gts)
    constants = box_eval.reference_constants(thrs, rngs)
    rank, matched, ignored, gt_ign, gt_of = box_eval.reference_outputs(B, K, G, A * T)
    for b in range(B):
        nk, ng = int(nk_all[b]), int(ng_all[b])
        l = lab[b, :nk]
        rank[b, :nk] = (np.tril(l[:, None] == l[None, :], -1)).sum(1)
        matched[b, :nk], ignored[b, :nk], gt_of[b, :nk], gt_ign[b, :ng] = box_eval.match_image(      # the per-class max_det cut
            l, rank[b, :nk] < max_det, box[b, :nk], gbox[b, :ng], garea[b, :ng], glab[b, :ng], gcrowd[b, :ng], constants,
            crowd_rules=True)
    return box_eval.reference_result(scores.device, rank, matched, ignored, gt_ign, gt_of, with_gt_of)


def accumulate(scores, labels, rank, matched, ignored, gt_label, gt_ignored, num_classes, iou_thrs, area_rngs, max_dets,
               rec_thrs=DEFAULT_REC_THRS):
    """pycocotools' ``accumulate`` on flat host arrays: detections (rank >= 0 only; in image order) and GTs (label >= 0 only).
    -> precision [T, R, C, A, M], recall [T, C, A, M], -1 where a cell has no not-ignored GT."""
    T, A, M, R = len(iou_thrs), len(area_rngs), len(max_dets), len(rec_thrs)
    rec_thrs = np.asarray(rec_thrs, np.float64)
    precision = -np.ones((T, R, num_classes, A, M))
    recall = -np.ones((T, num_classes, A, M))
    order = np.argsort(-scores, kind="mergesort")       # once for all cells: a stable sort commutes with taking a subset
    labels, rank, matched, ignored = labels[order], rank[order], matched[order], ignored[order]
    for c in range(num_classes):
        of_c = labels == c
        g_ign = gt_ignored[gt_label == c]
        for mi, max_det in enumerate(max_dets):
            sel = of_c & (rank < max_det)
            m_c, i_c = matched[sel], ignored[sel]
            for a in range(A):
                npig = int(np.count_nonzero(((g_ign >> a) & 1) == 0))
                if npig == 0:
                    continue
                for t in range(T):
                    bit = np.uint64(a * T + t)
                    keep = ((i_c >> bit) & np.uint64(1)) == 0
                    hit = ((m_c[keep] >> bit) & np.uint64(1)) != 0
                    tp = np.cumsum(hit).astype(np.float64)
                    fp = np.cumsum(~hit).astype(np.float64)
                    rc = tp / npig
                    pr = tp / (tp + fp + np.spacing(1))
                    recall[t, c, a, mi] = rc[-1] if len(rc) else 0.0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    at = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(R)
                    ok = at < len(pr)
                    q[ok] = pr[at[ok]]
                    precision[t, :, c, a, mi] = q
    return precision, recall


_STATE = ("scores", "labels", "rank", "matched", "ignored", "gt_label", "gt_ignored")
_STATE_DTYPES = (torch.float32, torch.int64, torch.int32, torch.int64, torch.int64, torch.int64, torch.uint8)


def accumulate_supported(state, num_classes, iou_thrs, area_rngs, max_dets, rec_thrs=DEFAULT_REC_THRS) -> bool:
    """True where ``accumulate_device`` runs the kernel: ``state`` is a non-empty list of per-batch dicts (what
    ``CocoBoxEvaluator`` keeps: ``scores`` / ``labels`` / ``rank`` / ``matched`` / ``ignored`` [B, K], ``gt_label`` /
    ``gt_ignored`` [B, G]) whose tensors all sit on ONE GPU in the evaluator's dtypes, the parameters are inside the entry's
    limits, ``rec_thrs`` ascends and the library is there."""
    if not isinstance(state, (list, tuple)) or not state:
        return False
    dev, n = None, 0
    for b in state:
        if not isinstance(b, dict) or not all(k in b and torch.is_tensor(b[k]) for k in _STATE):
            return False
        dev = b["scores"].device if dev is None else dev
        if not dev.type == "cuda" or not all(b[k].device == dev and b[k].dtype == d for k, d in zip(_STATE, _STATE_DTYPES)):
            return False
        if not all(b[k].shape == b["scores"].shape for k in _STATE[:5]) or b["gt_label"].shape != b["gt_ignored"].shape:
            return False
        n += b["scores"].numel()
    T, A, M, R = len(iou_thrs), len(area_rngs), len(max_dets), len(rec_thrs)
    if not (1 <= int(num_classes) <= MAX_CLASSES and 1 <= T <= MAX_THRS and 1 <= A <= MAX_AREAS and A * T <= MAX_BITS
            and 1 <= M <= MAX_DETS and 1 <= R <= MAX_RECS and n <= MAX_N):
        return False
    if not all(1 <= int(m) < 2 ** 31 for m in max_dets):
        return False
    rec = [float(r) for r in rec_thrs]
    if rec[0] != rec[0] or not all(b >= a for a, b in zip(rec, rec[1:])):
        return False
    try:
        _lib.load()
    except _lib.ExtensionMissingError:
        return False
    return True


def _ordered(state, C, A):
    """The flat state as ``zira_ap_accumulate`` takes it, by torch on the state's device and without a host wait:
    (rank, matched, ignored) in class-then-score order, seg_off [C + 1] i64, npig [C, A] i32."""
    cat = lambda k: torch.cat([b[k].reshape(-1) for b in state])
    scores, labels, rank, gt_label, gt_ignored = cat("scores"), cat("labels"), cat("rank"), cat("gt_label"), cat("gt_ignored")
    dev = scores.device
    key = torch.where((rank >= 0) & (labels >= 0) & (labels < C), labels, torch.full_like(labels, C))
    by_score = torch.sort(scores, descending=True, stable=True)[1]
    key, by_key = torch.sort(key[by_score], stable=True)
    order = by_score[by_key]
    seg_off = torch.searchsorted(key, torch.arange(C + 1, dtype=torch.int64, device=dev)).contiguous()
    gt_key = torch.where((gt_label >= 0) & (gt_label < C), gt_label, torch.full_like(gt_label, C))
    clear = ((gt_ignored.to(torch.int32)[:, None] >> torch.arange(A, dtype=torch.int32, device=dev)[None, :]) & 1) == 0
    npig = torch.zeros((C + 1, A), dtype=torch.int32, device=dev).index_add_(0, gt_key, clear.to(torch.int32))[:C].contiguous()
    return rank[order].contiguous(), cat("matched")[order].contiguous(), cat("ignored")[order].contiguous(), seg_off, npig


def accumulate_device(state, num_classes, iou_thrs, area_rngs, max_dets, rec_thrs=DEFAULT_REC_THRS):
    """``accumulate`` where the state is: ``zira_ap_accumulate`` on the current stream (one launch; the host never waits).
    ``state`` as ``accumulate_supported`` describes it.  torch puts the detections in order -- by class, inside a class by
    descending score, equal scores in state order (two stable sorts); entries with rank < 0 or a label outside [0, C) go behind
    the last class and take part in nothing -- and counts the not-ignored GTs per (class, area range).
    -> (precision [T, R, C, A, M], recall [T, C, A, M]), fp64 device tensors, bit for bit what ``accumulate`` returns."""
    if not accumulate_supported(state, num_classes, iou_thrs, area_rngs, max_dets, rec_thrs):
        raise RuntimeError("zira_ap_accumulate does not serve this state (see evaluation.accumulate_supported)")
    C, T, A, M, R = int(num_classes), len(iou_thrs), len(area_rngs), len(max_dets), len(rec_thrs)
    lib = _lib.load()
    dev = state[0]["scores"].device
    with torch.cuda.device(dev):
        rank, matched, ignored, seg_off, npig = _ordered(state, C, A)
        n = rank.numel()
        precision = torch.empty((T, R, C, A, M), dtype=torch.float64, device=dev)
        recall = torch.empty((T, C, A, M), dtype=torch.float64, device=dev)
        ptr = lambda t: t.data_ptr() if n > 0 else None
        rc = lib.zira_ap_accumulate(ptr(rank), ptr(matched), ptr(ignored), n, seg_off.data_ptr(), npig.data_ptr(), C, T, A,
                                    (ctypes.c_int32 * M)(*[int(m) for m in max_dets]), M,
                                    (ctypes.c_double * R)(*[float(r) for r in rec_thrs]), R, precision.data_ptr(),
                                    recall.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_ap_accumulate failed: hipError %d" % rc)
    return precision, recall


def _mean(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def summarize(precision, recall, class_names, iou_thrs, max_dets):
    """pycocotools' ``summarize`` and the reference's ``_derive_coco_results``: percent; -1 where nothing was populated."""
    thrs = np.asarray(iou_thrs)
    at = lambda v: np.where(np.isclose(thrs, v))[0]
    pct = lambda v: v * 100.0 if v > -1 else -1.0
    A = precision.shape[3]
    out = {"AP": pct(_mean(precision[:, :, :, 0, -1])),
           "AP50": pct(_mean(precision[at(0.5), :, :, 0, -1])),
           "AP75": pct(_mean(precision[at(0.75), :, :, 0, -1]))}
    for name, a in (("APs", 1), ("APm", 2), ("APl", 3)):
        out[name] = pct(_mean(precision[:, :, :, a, -1])) if a < A else -1.0
    for mi, m in enumerate(max_dets):
        out["AR%d" % m] = pct(_mean(recall[:, :, 0, mi]))
    for c, name in enumerate(class_names):
        out["AP-" + str(name)] = pct(_mean(precision[:, :, c, 0, -1]))
    return out


class CocoBoxEvaluator(box_eval.BoxEvaluator):
    """detectron2's ``DatasetEvaluator`` surface (``reset`` / ``process`` / ``evaluate``) for COCO box AP.  ``process`` pads the
    batch, matches it in one launch and keeps the result where it is; nothing is read back before ``evaluate()``, which
    accumulates where the state is (``accumulate_device``) and reads back the two tables, or -- CPU state, state on several
    devices after ``merge``, parameters outside the entry's limits, ``FORCE_REFERENCE`` -- reads back the state and accumulates
    on the host.  The tables are the same bits either way."""
    _STATE, _WORDS, _WORD_DTYPE = _STATE, ("matched", "ignored"), np.uint64

    def __init__(self, class_names, max_dets=(1, 10, 100), iou_thrs=None, area_rngs=None):
        self.class_names = list(class_names)
        self.max_dets = tuple(sorted(int(m) for m in max_dets))
        self.iou_thrs = tuple(float(t) for t in (DEFAULT_IOU_THRS if iou_thrs is None else iou_thrs))
        self.area_rngs = tuple((float(lo), float(hi)) for lo, hi in (DEFAULT_AREA_RNGS if area_rngs is None else area_rngs))
        self.reset()

    def process_padded(self, scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_crowd, n_gt):
        """One batch from raw tensors (``match``'s inputs; rows need not be sorted: a stable sort puts them in score order)."""
        scores, labels, xyxy = box_eval.sort_by_score(scores, labels, xyxy, n_keep)
        max_det = min(self.max_dets[-1], scores.shape[1])
        rank, matched, ignored, gt_ignored, _ = box_eval.match_batch(
            sys.modules[__name__], scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_crowd, n_gt, self.iou_thrs,
            self.area_rngs, max_det)
        self._batches.append(dict(scores=scores, labels=labels, rank=rank, matched=matched, ignored=ignored,
                                  gt_label=box_eval.mask_behind(gt_label, n_gt), gt_ignored=gt_ignored))

    def process(self, inputs, outputs):
        """``inputs``: the batched_inputs dicts, each with ``"annotations"`` (COCO dicts: ``bbox`` xywh in the output image's
        pixels, ``category_id`` the contiguous index, ``iscrowd``, optionally ``area``); ``outputs``: what the model returns in
        eval mode, ``[{"instances": Instances}]``."""
        dets = box_eval.pad_instances(outputs)
        self.process_padded(*dets, *box_eval.pad_annotations(inputs, dets[0].device, "iscrowd", with_area=True))

    def merge(self, other):
        """Append another evaluator's state (a data-parallel run gathers its ranks' evaluators with this)."""
        if (other.iou_thrs, other.area_rngs, other.max_dets) != (self.iou_thrs, self.area_rngs, self.max_dets):
            raise ValueError("merge: the evaluators differ in thresholds, area ranges or max_dets")
        self._batches.extend(other._batches)
        return self

    def evaluate(self):
        args = (len(self.class_names), self.iou_thrs, self.area_rngs, self.max_dets)
        if not FORCE_REFERENCE and accumulate_supported(self._batches, *args):
            precision, recall = box_eval.read_back(*accumulate_device(self._batches, *args))    # ONE device -> host copy
        else:
            precision, recall = accumulate(*box_eval.accumulate_inputs(self._gather()), *args)
        self.precision, self.recall = precision, recall
        return {"bbox": summarize(precision, recall, self.class_names, self.iou_thrs, self.max_dets)}


def inference_on_dataset(model, batches, evaluator):
    """The reference's evaluation loop (``box_eval.run_dataset``) over ``model(inputs)``."""
    return box_eval.run_dataset(model, batches, evaluator, lambda inputs: model(inputs))
