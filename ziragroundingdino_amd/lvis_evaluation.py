"""LVIS box AP behind the detections tail: what the reference gets from ``LVISEvaluator`` -> ``lvis.LVISResults`` /
``lvis.LVISEval`` (groundingdino/evaluation/lvis_evaluation.py:139-172; the ``lvis_v0.5`` metadata of datasets/builtin.py), without
the ``lvis`` package, detectron2 or a JSON file in between.  LVIS is a federated dataset: an image is annotated for the categories
of its positive set (those of its ground truth), checked and found empty for its negative set (``neg_category_ids``), and its
``not_exhaustive_category_ids`` may hold more instances than were drawn.  Two things therefore differ from COCO box AP
(``evaluation.py``):

- a detection of a category outside the image's positive and negative sets takes part in nothing -- it is not a false positive --
  and an unmatched detection of a not-exhaustively annotated category is ignored;
- detections are cut to the best ``max_dets`` (300) per IMAGE over all categories, not per class, and the summary adds APr / APc /
  APf over the rare / common / frequent classes.

``match`` runs the cut, the filter and ``LVISEval.evaluate_img`` for a whole batch in one launch where the detections already are
(csrc/lvismatch.hip, the rules stated in include/zira_lvis.h); ``match_reference`` is the same function in numpy fp64 on any device,
for what ``match_supported`` declines, for CPU tensors and for the tests.  Its outputs are laid out as ``evaluation.match``'s, so
``LVISBoxEvaluator`` keeps them on the device until ``evaluate()`` and accumulates them with ``evaluation.accumulate_device`` /
``accumulate`` as they are, ``max_dets = (300,)``; ``summarize`` works on the small tables.  Padding, score order, read-back and
the greedy walk itself are ``box_eval``'s: ``match_reference`` here states only the cut, the filter and the not-exhaustive flag.

``matched`` / ``ignored`` are int64 tensors that hold the 64 bits of the entry's u64 words (bit ``a * T + t``); the category bitsets
are int32 tensors that hold the 32 bits of the entry's u32 words (category ``c`` at bit ``c % 32`` of word ``c // 32``).
"""
import json
import sys

import numpy as np
import torch

from . import _lib, box_eval
from . import evaluation as ev

MAX_B, MAX_K, MAX_G, MAX_CLASSES = (_lib.LVIS_CONSTANTS[k] for k in ("ZIRA_LVIS_MAX_B", "ZIRA_LVIS_MAX_K", "ZIRA_LVIS_MAX_G",
                                                                     "ZIRA_LVIS_MAX_CLASSES"))
MAX_BITS, MAX_THRS, MAX_AREAS = ev.MAX_BITS, ev.MAX_THRS, ev.MAX_AREAS
FORCE_REFERENCE = False     # True: LVISBoxEvaluator matches with match_reference and accumulates on the host (tests, A/B)

DEFAULT_IOU_THRS, DEFAULT_REC_THRS, DEFAULT_AREA_RNGS = ev.DEFAULT_IOU_THRS, ev.DEFAULT_REC_THRS, ev.DEFAULT_AREA_RNGS
DEFAULT_MAX_DETS = 300
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf")     # what the reference's evaluator returns
_DTYPES = (torch.float32, torch.int64, torch.float32, torch.int32, torch.float64, torch.float64, torch.int64, torch.uint8,
           torch.int32, torch.int32, torch.int32)


def _shapes_ok(t, C) -> bool:
    if not all(torch.is_tensor(x) for x in t) or t[0].dim() != 2 or int(C) < 1:
        return False
    B, K = t[0].shape
    G = t[6].shape[1] if t[6].dim() == 2 else -1
    W = (int(C) + 31) // 32
    want = ((B, K), (B, K), (B, K, 4), (B,), (B, G, 4), (B, G), (B, G), (B, G), (B,), (B, W), (B, W))
    return all(tuple(x.shape) == s for x, s in zip(t, want))


def match_supported(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg_set, nel_set, num_classes,
                    iou_thrs=DEFAULT_IOU_THRS, area_rngs=DEFAULT_AREA_RNGS, max_det=DEFAULT_MAX_DETS) -> bool:
    """True where ``match`` runs the kernel: contiguous tensors of the entry's dtypes on one GPU, inside its limits."""
    t = (scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg_set, nel_set)
    if not _shapes_ok(t, num_classes) or not scores.is_cuda:
        return False
    if not all(x.dtype == d and x.device == scores.device and x.is_contiguous() for x, d in zip(t, _DTYPES)):
        return False
    (B, K), G, T, A = scores.shape, gt_label.shape[1], len(iou_thrs), len(area_rngs)
    return (1 <= B <= MAX_B and 1 <= K <= MAX_K and 0 <= G <= MAX_G and 1 <= int(num_classes) <= MAX_CLASSES
            and 1 <= int(max_det) <= K and 1 <= T <= MAX_THRS and 1 <= A <= MAX_AREAS and A * T <= MAX_BITS)


def match(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg_set, nel_set, num_classes,
          iou_thrs=DEFAULT_IOU_THRS, area_rngs=DEFAULT_AREA_RNGS, max_det=DEFAULT_MAX_DETS, with_gt_of=True):
    """``zira_lvis_match`` on the current stream (one launch, nothing uploaded, the host never waits; capturable).
    Detections as ``topk.detections`` / ``vocab.merge_detections`` return them -- rows in non-increasing score order, the first
    ``n_keep[b]`` valid -- ground truth padded to G per image (xywh and area fp64, label int64, ignore uint8, ``n_gt`` int32) and
    the two per-image bitsets of ``category_bitsets``.  Returns what ``evaluation.match`` returns:
    (rank [B, K] int32, matched [B, K] int64, ignored [B, K] int64, gt_ignored [B, G] uint8, gt_of [B, K, A T] int32 or None)."""
    args = (scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg_set, nel_set, num_classes)
    if not match_supported(*args, iou_thrs, area_rngs, max_det):
        raise RuntimeError("zira_lvis_match does not serve these inputs (see lvis_evaluation.match_supported)")
    thrs, rngs, max_det = ev._params(iou_thrs, area_rngs, max_det)
    (B, K), G, T, A = scores.shape, gt_label.shape[1], len(thrs), len(rngs)
    lib = _lib.load()
    (rank, matched, ignored, gt_ignored, gt_of), c_thrs, c_rngs, ptr = box_eval.match_launch(scores, G, thrs, rngs, with_gt_of)
    with torch.cuda.device(scores.device):
        rc = lib.zira_lvis_match(scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(), n_keep.data_ptr(), B, K, ptr(gt_xywh),
                                 ptr(gt_area), ptr(gt_label), ptr(gt_ignore), ptr(n_gt), G, neg_set.data_ptr(), nel_set.data_ptr(),
                                 int(num_classes), c_thrs, T, c_rngs, A, max_det, rank.data_ptr(), matched.data_ptr(),
                                 ignored.data_ptr(), ptr(gt_ignored), gt_of.data_ptr() if with_gt_of else None,
                                 torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_lvis_match failed: hipError %d" % rc)
    return rank, matched, ignored, gt_ignored, gt_of


def match_reference(scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg_set, nel_set, num_classes,
                    iou_thrs=DEFAULT_IOU_THRS, area_rngs=DEFAULT_AREA_RNGS, max_det=DEFAULT_MAX_DETS, with_gt_of=True):
    """What ``match`` returns, computed on the host in numpy fp64 (tensors on any device; the results go back to it): the
    definition.  Per image the cut and the category filter, then ``box_eval.match_image`` under LVIS's rules -- a taken GT stays
    taken, flagged or not, and an unmatched detection of a not-exhaustively annotated category is ignored."""
    t = (scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg_set, nel_set)
    if not _shapes_ok(t, num_classes):
        raise ValueError("match_reference: scores / labels [B, K], xyxy [B, K, 4], n_keep [B], gt_xywh [B, G, 4], gt_area / "
                         "gt_label / gt_ignore [B, G], n_gt [B], neg_set / nel_set [B, ceil(C / 32)], C >= 1")
    thrs, rngs, max_det = ev._params(iou_thrs, area_rngs, max_det)
    (B, K), G, T, A, C = scores.shape, gt_label.shape[1], len(thrs), len(rngs), int(num_classes)
    if not 1 <= max_det or A * T > MAX_BITS or A < 1 or T < 1:
        raise ValueError("match_reference: max_det >= 1, 1 <= A T <= 64")
    lab, box, nk_all, gbox, garea, glab, gflag, ng_all = box_eval.reference_inputs(*t[1:9])
    neg, nel = (x.detach().cpu().numpy().astype(np.int32, copy=False).view(np.uint32) for x in (neg_set, nel_set))
    constants = box_eval.reference_constants(thrs, rngs)
    in_set = lambda words, c: ((words[c >> 5] >> (c & 31).astype(np.uint32)) & np.uint32(1)) != 0
    rank, matched, ignored, gt_ign, gt_of = box_eval.reference_outputs(B, K, G, A * T)
    for b in range(B):
        nk, ng = min(int(nk_all[b]), max_det), int(ng_all[b])                       # the image cut
        gl = glab[b, :ng]
        l = lab[b, :nk]
        in_c = (l >= 0) & (l < C)
        c = np.where(in_c, l, 0)
        takes = in_c & (np.isin(l, gl) | in_set(neg[b], c))                         # the category filter
        l = np.where(takes, l, -1)
        rank[b, :nk] = np.where(takes, (np.tril(l[:, None] == l[None, :], -1)).sum(1), -1)
        matched[b, :nk], ignored[b, :nk], gt_of[b, :nk], gt_ign[b, :ng] = box_eval.match_image(
            l, takes, box[b, :nk], gbox[b, :ng], garea[b, :ng], gl, gflag[b, :ng], constants, crowd_rules=False,
            unmatched_ignored=in_c & in_set(nel[b], c))                             # not exhaustively annotated
    return box_eval.reference_result(scores.device, rank, matched, ignored, gt_ign, gt_of, with_gt_of)


def category_bitsets(lists, C, device="cpu"):
    """Per-image lists of contiguous 0-based category ids -> the [B, ceil(C / 32)] int32 tensor ``match`` takes (the 32 bits of a
    u32 word each: category c at bit c % 32 of word c // 32), packed on the host and moved to ``device`` in one copy."""
    C = int(C)
    if C < 1:
        raise ValueError("category_bitsets: C >= 1")
    words = np.zeros((len(lists), (C + 31) // 32), np.uint32)
    for b, ids in enumerate(lists):
        for c in ids:
            c = int(c)
            if not 0 <= c < C:
                raise ValueError("category_bitsets: id %d of image %d is outside 0..%d" % (c, b, C - 1))
            words[b, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return torch.from_numpy(words.view(np.int32)).to(device)


def load_categories(path):
    """The category fixture (tests/golden/lvis_v0_5_categories.json: name, 0-based index, frequency letter per class) ->
    (class names, frequency letters), both in index order."""
    with open(path) as f:
        rows = sorted(json.load(f)["categories"], key=lambda r: r["index"])
    if [r["index"] for r in rows] != list(range(len(rows))) or any(r["frequency"] not in ("r", "c", "f") for r in rows):
        raise ValueError("%s: indices 0..n-1 once each, frequencies r / c / f" % path)
    return [r["name"] for r in rows], [r["frequency"] for r in rows]


def load_frequencies(path):
    """The frequency letter ("r" rare, "c" common, "f" frequent) of every class of the category fixture, in index order."""
    return load_categories(path)[1]


def summarize(precision, recall, frequencies, iou_thrs, max_det=DEFAULT_MAX_DETS):
    """``LVISEval.summarize`` on the host: precision [T, R, C, A, M] and recall [T, C, A, M] as ``evaluation.accumulate`` returns
    them (the last max-det index is used) -> AP, AP50, AP75, APs, APm, APl, APr, APc, APf and AR@300, ARs@300, ARm@300, ARl@300
    in percent.  Each is the mean over the populated entries (> -1), -1 where there are none; APr / APc / APf take the classes
    whose frequency is "r" / "c" / "f"."""
    precision, recall = np.asarray(precision)[..., -1], np.asarray(recall)[..., -1]
    thrs = np.asarray(iou_thrs)
    at = lambda v: np.where(np.isclose(thrs, v))[0]
    pct = lambda v: v * 100.0 if v > -1 else -1.0
    A = precision.shape[3]
    freq = np.asarray(list(frequencies))
    if freq.shape != (precision.shape[2],):
        raise ValueError("summarize: one frequency letter per class")
    out = {"AP": pct(ev._mean(precision[:, :, :, 0])),
           "AP50": pct(ev._mean(precision[at(0.5), :, :, 0])),
           "AP75": pct(ev._mean(precision[at(0.75), :, :, 0]))}
    for name, a in (("APs", 1), ("APm", 2), ("APl", 3)):
        out[name] = pct(ev._mean(precision[:, :, :, a])) if a < A else -1.0
    for letter in "rcf":
        out["AP" + letter] = pct(ev._mean(precision[:, :, np.where(freq == letter)[0], 0]))
    for name, a in (("AR", 0), ("ARs", 1), ("ARm", 2), ("ARl", 3)):
        out["%s@%d" % (name, max_det)] = pct(ev._mean(recall[:, :, a])) if a < A else -1.0
    return out


class LVISBoxEvaluator(box_eval.BoxEvaluator):
    """detectron2's ``DatasetEvaluator`` surface (``reset`` / ``process`` / ``evaluate``) for LVIS box AP, with
    ``CocoBoxEvaluator``'s division of work: ``process`` pads the batch, matches it in one launch and keeps the result where it
    is; nothing is read back before ``evaluate()``, which accumulates where the state is (``evaluation.accumulate_device``) and
    reads back the two tables, or -- CPU state, state on several devices after ``merge``, parameters outside the entry's limits,
    ``FORCE_REFERENCE`` -- reads back the state and accumulates on the host.  The tables are the same bits either way."""
    _STATE, _WORDS, _WORD_DTYPE = ev._STATE, ("matched", "ignored"), np.uint64       # ``evaluation.match``'s layout

    def __init__(self, class_names, frequencies, max_dets=DEFAULT_MAX_DETS, iou_thrs=None, area_rngs=None):
        self.class_names = list(class_names)
        self.frequencies = list(frequencies)
        if len(self.frequencies) != len(self.class_names) or not set(self.frequencies) <= {"r", "c", "f"}:
            raise ValueError("LVISBoxEvaluator: one frequency letter (r / c / f) per class")
        self.max_dets = int(max_dets)
        self.iou_thrs = tuple(float(t) for t in (DEFAULT_IOU_THRS if iou_thrs is None else iou_thrs))
        self.area_rngs = tuple((float(lo), float(hi)) for lo, hi in (DEFAULT_AREA_RNGS if area_rngs is None else area_rngs))
        self.reset()

    def process_padded(self, scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg_set, nel_set):
        """One batch from raw tensors (``match``'s inputs; rows need not be sorted: a stable sort puts them in score order)."""
        scores, labels, xyxy = box_eval.sort_by_score(scores, labels, xyxy, n_keep)
        K = scores.shape[1]
        rank, matched, ignored, gt_ignored, _ = box_eval.match_batch(
            sys.modules[__name__], scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg_set, nel_set,
            len(self.class_names), self.iou_thrs, self.area_rngs, min(self.max_dets, K))
        self._batches.append(dict(scores=scores, labels=labels, rank=rank, matched=matched, ignored=ignored,
                                  gt_label=box_eval.mask_behind(gt_label, n_gt), gt_ignored=gt_ignored,
                                  n_pred=n_keep.clamp(0, K).sum(dtype=torch.int64)))

    def process(self, inputs, outputs):
        """``inputs``: the batched_inputs dicts, each with ``"annotations"`` (dicts: ``bbox`` xywh in the output image's pixels,
        ``category_id`` the contiguous index, optionally ``area`` and ``ignore``), ``"neg_category_ids"`` and
        ``"not_exhaustive_category_ids"`` (contiguous 0-based ids, i.e. after the metadata's mapping; a missing key is an empty
        list); ``outputs``: what the model returns in eval mode, ``[{"instances": Instances}]``."""
        dets = box_eval.pad_instances(outputs)
        dev, C = dets[0].device, len(self.class_names)
        self.process_padded(*dets, *box_eval.pad_annotations(inputs, dev, "ignore", with_area=True),
                            category_bitsets([x.get("neg_category_ids", ()) for x in inputs], C, dev),
                            category_bitsets([x.get("not_exhaustive_category_ids", ()) for x in inputs], C, dev))

    def merge(self, other):
        """Append another evaluator's state (a data-parallel run gathers its ranks' evaluators with this)."""
        mine = (self.iou_thrs, self.area_rngs, self.max_dets, self.frequencies)
        if (other.iou_thrs, other.area_rngs, other.max_dets, other.frequencies) != mine:
            raise ValueError("merge: the evaluators differ in thresholds, area ranges, max_dets or frequencies")
        self._batches.extend(other._batches)
        return self

    def _result(self, precision, recall, n_pred):
        self.precision, self.recall = precision, recall
        if n_pred == 0:                             # the reference: "No predictions from the model! Set scores to -1"
            return {"bbox": {k: -1.0 for k in summarize(precision, recall, self.frequencies, self.iou_thrs, self.max_dets)}}
        return {"bbox": summarize(precision, recall, self.frequencies, self.iou_thrs, self.max_dets)}

    def evaluate(self):
        args = (len(self.class_names), self.iou_thrs, self.area_rngs, (self.max_dets,))
        if not FORCE_REFERENCE and ev.accumulate_supported(self._batches, *args):
            p, r = ev.accumulate_device(self._batches, *args)
            n_pred = torch.stack([b["n_pred"] for b in self._batches]).sum().to(torch.float64)      # exact: far below 2^53
            precision, recall, n_pred = box_eval.read_back(p, r, n_pred)                           # ONE device -> host copy
            return self._result(precision, recall, int(n_pred))
        host = self._gather()
        n_pred = sum(int(b["n_pred"]) for b in self._batches)
        return self._result(*ev.accumulate(*box_eval.accumulate_inputs(host), *args), n_pred)
