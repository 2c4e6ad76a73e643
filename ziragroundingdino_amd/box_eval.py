"""What the device-side evaluators share (``evaluation``, ``lvis_evaluation``, ``voc_evaluation``, ``phrase_evaluation``): the
padding of a batch's detections and annotations, the stable score order, the -1 mask behind a row's count, the choice between
a module's kernel and its reference, the one-copy read-backs, the launcher pieces and the numpy fp64 definition of the greedy
COCO / LVIS matching (``match_image`` / ``greedy_walk``: ONE statement of the rule, with the places where the two data sets
differ as arguments), and the dataset loop.  Plain functions on tensors and arrays; nothing here knows a kernel's name."""
import ctypes

import numpy as np
import torch


# ---- padding a batch ---------------------------------------------------------------------------------------------------------
def pad_instances(outputs):
    """``[{"instances": Instances}]`` -> (scores [B, K] f32, labels [B, K] i64, xyxy [B, K, 4] f32, n_keep [B] i32) where the
    instances are, zero behind an image's count; K is the longest image's count, at least 1."""
    insts = [o["instances"] for o in outputs]
    dev = insts[0].scores.device
    lens = [len(i) for i in insts]
    B, K = len(insts), max(1, max(lens))
    scores = torch.zeros((B, K), dtype=torch.float32, device=dev)
    labels = torch.zeros((B, K), dtype=torch.int64, device=dev)
    xyxy = torch.zeros((B, K, 4), dtype=torch.float32, device=dev)
    for b, (inst, n) in enumerate(zip(insts, lens)):
        scores[b, :n], labels[b, :n], xyxy[b, :n] = inst.scores, inst.pred_classes, inst.pred_boxes.tensor
    return scores, labels, xyxy, torch.tensor(lens, dtype=torch.int32).to(dev)


def pad_annotations(inputs, device, flag_key, with_area):
    """The inputs' ``"annotations"`` (a missing key is an empty list) padded to the longest image's G -- 0 where no image has
    one -- and moved to ``device`` in one copy each: (bbox [B, G, 4] f64, the four numbers as they are; area [B, G] f64 or
    None without ``with_area``: the annotation's ``area``, else bbox[2] * bbox[3]; category_id [B, G] i64; the truth of
    ``flag_key`` [B, G] u8, 0 where the key is missing; n_gt [B] i32)."""
    annos = [list(x.get("annotations", ())) for x in inputs]
    B, G = len(annos), max(len(a) for a in annos)
    box, area = np.zeros((B, G, 4)), np.zeros((B, G))
    label, flag = np.zeros((B, G), np.int64), np.zeros((B, G), np.uint8)
    for b, anns in enumerate(annos):
        for g, ann in enumerate(anns):
            four = [float(v) for v in ann["bbox"]]
            box[b, g], label[b, g], flag[b, g] = four, int(ann["category_id"]), int(bool(ann.get(flag_key, 0)))
            if with_area:
                area[b, g] = float(ann["area"]) if "area" in ann else four[2] * four[3]
    up = lambda a: torch.from_numpy(a).to(device)
    return (up(box), up(area) if with_area else None, up(label), up(flag),
            torch.tensor([len(a) for a in annos], dtype=torch.int32).to(device))


def sort_by_score(scores, labels, xyxy, n_keep):
    """The three detection tensors with every row in non-increasing score order: a stable sort, equal scores keep their
    order, the rows at and behind ``n_keep[b]`` go last whatever they hold."""
    B, K = scores.shape
    valid = torch.arange(K, device=scores.device)[None, :] < n_keep[:, None]
    key = torch.where(valid, scores, torch.full_like(scores, float("-inf")))
    order = torch.sort(key, dim=1, descending=True, stable=True)[1]
    return (torch.gather(scores, 1, order).contiguous(), torch.gather(labels, 1, order).contiguous(),
            torch.gather(xyxy, 1, order[:, :, None].expand(B, K, 4)).contiguous())


def mask_behind(t, n):
    """``t`` [B, N] with -1 at and behind column ``n[b]`` of every row."""
    valid = torch.arange(t.shape[1], device=t.device)[None, :] < n[:, None]
    return torch.where(valid, t, torch.full_like(t, -1))


def match_batch(module, *args):
    """One batch through ``module.match`` where it serves ``args`` and ``module.FORCE_REFERENCE`` is off, else through
    ``module.match_reference``; without ``gt_of``.  The names are looked up per call: tests set them per module."""
    fn = module.match if not module.FORCE_REFERENCE and module.match_supported(*args) else module.match_reference
    return fn(*args, with_gt_of=False)


# ---- the kept state ----------------------------------------------------------------------------------------------------------
def gather_state(batches, keys, word_keys, word_dtype):
    """``batches``: per-batch dicts of tensors, a batch on the device of its ``keys[0]``.  -> per batch a dict of flat host
    arrays of ``keys``, through ONE device -> host copy per device that holds state; ``word_keys`` are reread as the unsigned
    ``word_dtype`` whose bits they hold."""
    host = [None] * len(batches)
    for dev in {b[keys[0]].device for b in batches}:
        idx = [i for i, b in enumerate(batches) if b[keys[0]].device == dev]
        blob = torch.cat([batches[i][k].contiguous().view(-1).view(torch.uint8) for i in idx for k in keys]).cpu().numpy()
        off = 0
        for i in idx:
            host[i] = {}
            for k in keys:
                t = batches[i][k]
                n = t.numel() * t.element_size()
                dt = word_dtype if k in word_keys else torch.empty(0, dtype=t.dtype).numpy().dtype
                host[i][k] = np.frombuffer(blob[off:off + n].tobytes(), dtype=dt)
                off += n
    return host


class BoxEvaluator:
    """What the three box evaluators keep: ``_batches``, a list of per-batch dicts of the tensors named by ``_STATE``, where
    the detections were; ``_WORDS`` of them hold the bits of ``_WORD_DTYPE`` words."""
    _STATE, _WORDS, _WORD_DTYPE = (), (), None

    def reset(self):
        self._batches = []

    def _gather(self):
        """Every kept tensor as a host array, through ONE device -> host copy per device that holds state."""
        return gather_state(self._batches, self._STATE, self._WORDS, self._WORD_DTYPE)


def read_back(*tensors):
    """Device tensors of one dtype -> host arrays of their shapes, through ONE device -> host copy."""
    flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
    ends = np.cumsum([t.numel() for t in tensors])
    return [flat[e - t.numel():e].reshape(tuple(t.shape)) for t, e in zip(tensors, ends)]


def concat_state(host, key, dtype):
    """``key`` of every batch of ``gather_state``'s result as one flat array, in batch order; empty of ``dtype`` without one."""
    return np.concatenate([h[key] for h in host]) if host else np.zeros(0, dtype)


def accumulate_inputs(host):
    """The gathered COCO-layout state (``evaluation._STATE``) -> the seven flat arrays ``evaluation.accumulate`` begins with:
    the detections with a rank, the GTs with a label."""
    cat = lambda k, dt: concat_state(host, k, dt)
    rank, gt_label = cat("rank", np.int32), cat("gt_label", np.int64)
    det, gt = rank >= 0, gt_label >= 0
    return (cat("scores", np.float32)[det].astype(np.float64), cat("labels", np.int64)[det], rank[det],
            cat("matched", np.uint64)[det], cat("ignored", np.uint64)[det], gt_label[gt], cat("gt_ignored", np.uint8)[gt])


# ---- launching a COCO-layout match -------------------------------------------------------------------------------------------
def match_launch(scores, G, thrs, rngs, with_gt_of):
    """What the ``zira_ap_match`` and ``zira_lvis_match`` launchers share: the outputs (rank [B, K] i32, matched / ignored
    [B, K] i64, gt_ignored [B, G] u8, gt_of [B, K, A T] i32 or None) beside ``scores``, the thresholds and the flattened area
    ranges as C doubles, and ``ptr``: a tensor's address, null for every [.., G, ..] tensor when G == 0."""
    (B, K), T, A, dev = scores.shape, len(thrs), len(rngs), scores.device
    out = (torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
           torch.empty((B, K), dtype=torch.int64, device=dev), torch.empty((B, G), dtype=torch.uint8, device=dev),
           torch.empty((B, K, A * T), dtype=torch.int32, device=dev) if with_gt_of else None)
    c_thrs = (ctypes.c_double * T)(*thrs)
    c_rngs = (ctypes.c_double * (2 * A))(*[v for r in rngs for v in r])
    return out, c_thrs, c_rngs, lambda t: t.data_ptr() if G > 0 else None


# ---- the definition of the greedy matching, numpy fp64 -----------------------------------------------------------------------
def reference_inputs(labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_flag, n_gt):
    """The tensors on the host as the definition reads them: (labels i64, xyxy f32, n_keep clamped to 0..K, gt_xywh f64,
    gt_area f64, gt_label i64, gt_flag bool, n_gt clamped to 0..G)."""
    host = lambda t, dt: t.detach().cpu().numpy().astype(dt, copy=False)
    K, G = labels.shape[1], gt_label.shape[1]
    return (host(labels, np.int64), host(xyxy, np.float32), np.clip(host(n_keep, np.int64), 0, K), host(gt_xywh, np.float64),
            host(gt_area, np.float64), host(gt_label, np.int64), host(gt_flag, np.uint8) != 0, np.clip(host(n_gt, np.int64), 0, G))


def reference_outputs(B, K, G, AT):
    """(rank, matched, ignored, gt_ignored, gt_of) as the definition fills them: nothing matched, no rank, no GT."""
    return (np.full((B, K), -1, np.int32), np.zeros((B, K), np.uint64), np.zeros((B, K), np.uint64), np.zeros((B, G), np.uint8),
            np.full((B, K, AT), -1, np.int32))


def reference_result(device, rank, matched, ignored, gt_ign, gt_of, with_gt_of):
    t = lambda a: torch.from_numpy(a).to(device)
    return t(rank), t(matched.view(np.int64)), t(ignored.view(np.int64)), t(gt_ign), t(gt_of) if with_gt_of else None


def reference_constants(thrs, rngs):
    """(lo [A, 1], hi [A, 1], floor [A T, 1]): the area ranges' ends and, for problem a T + t, the IoU a match needs."""
    lo = np.array([r[0] for r in rngs])[:, None]
    hi = np.array([r[1] for r in rngs])[:, None]
    return lo, hi, np.repeat(np.minimum(np.array(thrs), 1 - 1e-10)[None, :], len(rngs), 0).reshape(len(rngs) * len(thrs), 1)


def xywh_iou(box, gbox, crowd=None):
    """pycocotools' IoU in fp64, every operation rounded on its own: ``box`` [nk, 4] fp32 xyxy (its width and height are fp32
    differences), ``gbox`` [ng, 4] fp64 xywh.  Where ``crowd`` [ng] is set the union is the detection's area.
    -> (iou [nk, ng], the detections' areas [nk])."""
    dx, dy = box[:, 0].astype(np.float64), box[:, 1].astype(np.float64)
    dw = (box[:, 2] - box[:, 0]).astype(np.float64)
    dh = (box[:, 3] - box[:, 1]).astype(np.float64)
    da = dw * dh
    gx, gy, gw, gh = (gbox[:, i] for i in range(4))
    ga = gw * gh
    w = np.minimum((dx + dw)[:, None], (gx + gw)[None, :]) - np.maximum(dx[:, None], gx[None, :])
    h = np.minimum((dy + dh)[:, None], (gy + gh)[None, :]) - np.maximum(dy[:, None], gy[None, :])
    inter = w * h
    union = da[:, None] + ga[None, :] - inter
    if crowd is not None:
        union = np.where(crowd[None, :], da[:, None], union)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((w > 0) & (h > 0), inter / union, 0.0), da


def greedy_walk(iou, same, takes, ign, det_out, floor, retake=None):
    """The order-dependent part: the detections of one image in score order, all A T problems and all GTs of a step side by
    side.  ``iou`` [nk, ng]; ``same`` [nk, ng]: the pair shares a label; ``takes`` [nk]: the detection takes part (one that does
    not keeps zero words and takes no GT); ``ign`` [A T, ng]: the GT is ignored in the problem; ``det_out`` [A T, nk]: the
    detection's ignore flag where it stays unmatched; ``floor`` [A T, 1]; ``retake`` [ng] or None: GTs that may be taken again
    (COCO's crowds).  A detection takes, per problem, the free GT of its label with the highest IoU >= floor -- a not-ignored
    one before any ignored one, the LAST of equals -- and inherits that GT's ignore flag.
    -> (matched [nk] u64, ignored [nk] u64: bit a T + t;  gt_of [nk, A T] i32, -1 where unmatched)."""
    (nk, ng), AT = iou.shape, floor.shape[0]
    weight = np.uint64(1) << np.arange(AT, dtype=np.uint64)
    matched, ignored, gt_of = np.zeros(nk, np.uint64), np.zeros(nk, np.uint64), np.full((nk, AT), -1, np.int32)
    taken = np.zeros((AT, ng), bool)
    rows = np.arange(AT)
    for k in range(nk):
        if not takes[k]:
            continue
        m_bits, i_bits = np.zeros(AT, bool), det_out[:, k].copy()
        if ng and same[k].any():
            free = ~taken if retake is None else retake[None, :] | ~taken
            cand = same[k][None, :] & free & ~(iou[k][None, :] < floor)
            first = cand & ~ign
            pool = np.where(first.any(1)[:, None], first, cand)      # the not-ignored GTs shut the ignored ones out
            val = np.where(pool, iou[k][None, :], -np.inf)
            top = val.max(1)
            pick = ng - 1 - np.argmax((pool & (val == top[:, None]))[:, ::-1], 1)       # the LAST of the best
            got = pool.any(1)
            gt_of[k, got] = pick[got]
            taken[rows[got], pick[got]] = True
            m_bits = got
            i_bits = np.where(got, ign[rows, pick], i_bits)
        matched[k] = weight[m_bits].sum(dtype=np.uint64)
        ignored[k] = weight[i_bits].sum(dtype=np.uint64)
    return matched, ignored, gt_of


def match_image(labels, takes, box, gbox, garea, glabel, gflag, constants, crowd_rules, unmatched_ignored=None):
    """One image of the definition: ``labels`` [nk] / ``takes`` [nk] / ``box`` [nk, 4] in score order, the image's ng GTs,
    ``constants`` of ``reference_constants``.  A GT is ignored in area range a where it is flagged or its area lies outside
    the range; an unmatched detection where its own area does, or where ``unmatched_ignored`` [nk] says so (LVIS: a category
    not exhaustively annotated).  ``crowd_rules`` (COCO): a flagged GT is a crowd -- the union is the detection's area and it
    may be taken again.  -> ``greedy_walk``'s three and gt_ignored [ng] u8 (bit a)."""
    lo, hi, floor = constants
    A = lo.shape[0]
    T = floor.shape[0] // A
    ign_a = gflag[None, :] | (garea[None, :] < lo) | (garea[None, :] > hi)                                    # [A, ng]
    gt_ign = (ign_a.astype(np.uint8) << np.arange(A, dtype=np.uint8)[:, None]).sum(0, dtype=np.uint8)
    iou, da = xywh_iou(box, gbox, gflag if crowd_rules else None)
    det_out = np.repeat((da[None, :] < lo) | (da[None, :] > hi), T, 0)                                        # [A T, nk]
    if unmatched_ignored is not None:
        det_out = det_out | unmatched_ignored[None, :]
    same = labels[:, None] == glabel[None, :]
    return greedy_walk(iou, same, takes, np.repeat(ign_a, T, 0), det_out, floor, gflag if crowd_rules else None) + (gt_ign,)


# ---- the dataset loop --------------------------------------------------------------------------------------------------------
def run_dataset(model, batches, evaluator, forward):
    """The reference's evaluation loop (train_multidatasets.py:338-364): eval mode, no gradients, ``evaluator.process(inputs,
    forward(inputs))`` per batch, the model's mode put back."""
    was_training = model.training
    model.eval()
    evaluator.reset()
    try:
        with torch.no_grad():
            for inputs in batches:
                evaluator.process(inputs, forward(inputs))
    finally:
        model.train(was_training)
    return evaluator.evaluate()
