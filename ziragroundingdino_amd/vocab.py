"""Vocabularies longer than one caption: the category list split into chunks that fit ``max_text_len``, and the chunks'
detections merged on the device (csrc/vocab.hip).

``GroundingDINO.encode_text`` cuts a caption at ``max_text_len`` tokens, so the categories behind the cut can never be
detected.  The standard answer is to run the text side, the transformer and the heads once per chunk of the list and to keep
the global top-k.  ``split_categories`` is the host side of that; ``merge_detections`` is the device side: ONE launch for the
batch (``zira_det_merge_f32``) on the chunks' candidates, leaving the padded outputs of ``topk.detections``.

Why the two-level scheme is exact.  Per chunk j the caller has run ``topk.topk_rows(prob_j.view(B, Q * C_j), min(k, Q * C_j))``
and written values and flat indices into slice ``[chunk_start[j], chunk_start[j + 1])`` of the candidate row.  The merged result
equals the first k of a stable descending sort of the virtual row ``cat_j(prob_j[b].flatten())``: an element of the global
top-k has fewer than k elements before it in the virtual row, hence fewer than k before it in its own chunk, so it is among
that chunk's candidates; and the candidates stand in chunk-major order, inside a chunk in the order of the chunk's own stable
sort, so two equal scores meet in the candidate row in the order they have in the virtual row -- ties go to the lower chunk,
then to the lower index (tests/test_vocab_cpu.py holds this against the brute-force virtual row).

``detections_chunked_reference`` is the definition in torch ops, on any device; it also serves CPU tensors, other dtypes,
shapes outside the header's limits and ``FORCE_REFERENCE``."""
import ctypes

import torch

from . import _lib
from .box_ops import box_cxcywh_to_xyxy
from .structures import Boxes, Instances, detector_postprocess

MAX_CHUNKS, MAX_CANDIDATES = _lib.VOCAB_CONSTANTS["ZIRA_VOCAB_MAX_CHUNKS"], _lib.VOCAB_CONSTANTS["ZIRA_VOCAB_MAX_CANDIDATES"]
MAX_K, MAX_B = _lib.VOCAB_CONSTANTS["ZIRA_VOCAB_MAX_K"], _lib.VOCAB_CONSTANTS["ZIRA_VOCAB_MAX_B"]
FORCE_REFERENCE = False      # developer switch: every call takes detections_chunked_reference
_INT32_MAX = 2 ** 31 - 1


# ---- host side: the list in chunks ----------------------------------------------------------------------------------------------
def caption_of(names):
    """The caption of a chunk, as the task chain spells a category list."""
    return ".".join(names) + "."


def caption_tokens(caption, tokenizer):
    """How many tokens ``encode_text`` gets for ``caption``, special tokens included."""
    return int(tokenizer([caption], padding="longest", return_tensors="pt")["input_ids"].shape[1])


def split_categories(names, tokenizer, max_text_len, chunk_size=None):
    """``names`` in order, greedily, as chunks whose caption (``".".join(chunk) + "."``) tokenises to at most ``max_text_len``
    tokens and, with ``chunk_size``, which hold at most that many names.  A name that does not fit on its own raises
    ``ValueError``; a list that fits is one chunk."""
    names = list(names)
    if chunk_size is not None and int(chunk_size) < 1:
        raise ValueError("split_categories: chunk_size must be None or at least 1, not %r" % (chunk_size,))
    chunks, cur = [], []
    for name in names:
        if cur and (chunk_size is None or len(cur) < int(chunk_size)) \
                and caption_tokens(caption_of(cur + [name]), tokenizer) <= max_text_len:
            cur.append(name)
            continue
        if caption_tokens(caption_of([name]), tokenizer) > max_text_len:
            raise ValueError("split_categories: the category name %r alone tokenises to more than max_text_len = %d tokens"
                             % (name, max_text_len))
        if cur:
            chunks.append(cur)
        cur = [name]
    if cur:
        chunks.append(cur)
    return chunks


# ---- the merge --------------------------------------------------------------------------------------------------------------
def _table(chunk_start, chunk_classes, label_offset):
    start, classes, offset = [int(v) for v in chunk_start], [int(v) for v in chunk_classes], [int(v) for v in label_offset]
    J = len(classes)
    if not (J >= 1 and len(start) == J + 1 and len(offset) == J and start[0] == 0
            and all(a < b for a, b in zip(start, start[1:])) and min(classes) >= 1 and min(offset) >= 0):
        raise ValueError("merge_detections: chunk_start is 0 = s_0 < s_1 < ... < s_J, with J class counts >= 1 and J label offsets >= 0")
    return start, classes, offset


def _check(cand_scores, cand_index, start, boxes, k, sizes):
    J, N = len(start) - 1, start[-1]
    if not (torch.is_tensor(cand_scores) and cand_scores.dim() == 2 and cand_scores.shape[1] >= N and torch.is_tensor(cand_index)
            and tuple(cand_index.shape) == tuple(cand_scores.shape) and not cand_index.is_floating_point()):
        raise ValueError("merge_detections: cand_scores [B, >= chunk_start[J]] and integer cand_index of the same shape")
    B = cand_scores.shape[0]
    if not (torch.is_tensor(boxes) and boxes.dim() == 4 and tuple(boxes.shape[:2]) == (J, B) and boxes.shape[2] >= 1
            and boxes.shape[3] == 4):
        raise ValueError("merge_detections: boxes [J, B, Q, 4] (cxcywh)")
    if not (torch.is_tensor(sizes) and tuple(sizes.shape) == (B, 4)):
        raise ValueError("merge_detections: sizes [B, 4] = (img_h, img_w, out_h, out_w)")
    if int(k) < 1:
        raise ValueError("merge_detections: k >= 1")


def detections_chunked_reference(cand_scores, cand_index, chunk_start, chunk_classes, label_offset, boxes, k, sizes):
    """The definition.  cand_scores [B, N], cand_index [B, N] integers (flat indices into the chunks' [Q, C_j] tensors),
    chunk_start J + 1 host integers (chunk j owns positions ``chunk_start[j] .. chunk_start[j + 1] - 1``; N = chunk_start[J]),
    chunk_classes / label_offset J host integers, boxes [J, B, Q, 4] cxcywh in 0..1, sizes [B, 4] = (img_h, img_w, out_h,
    out_w) -> (scores [B, k], labels [B, k] int64, xyxy [B, k, 4], n_keep [B] int32) on the inputs' device, zero behind
    ``n_keep``.

    Per image: the first k positions of ``torch.sort(stable=True, descending=True)`` over the row (every position counts);
    position -> chunk, ``q = index // C_j``, ``label = label_offset[j] + index % C_j``, ``box = boxes[j, b, q]``; then the
    evaluation tail's own op chain -- ``dt_inference``'s boxes and ``structures.detector_postprocess``.  One host read, of the
    sizes."""
    start, classes, offset = _table(chunk_start, chunk_classes, label_offset)
    _check(cand_scores, cand_index, start, boxes, k, sizes)
    k, N, dev = int(k), start[-1], cand_scores.device
    B = cand_scores.shape[0]
    row = cand_scores[:, :N]
    pos = torch.sort(row, dim=1, descending=True, stable=True).indices[:, :k].contiguous()                 # [B, min(k, N)]
    top = torch.gather(row, 1, pos)
    flat = torch.gather(cand_index[:, :N].to(torch.int64), 1, pos)
    j = torch.bucketize(pos, torch.tensor(start[1:-1], dtype=torch.int64, device=dev), right=True)
    C = torch.tensor(classes, dtype=torch.int64, device=dev)[j]
    q = torch.div(flat, C, rounding_mode="floor")
    label = torch.tensor(offset, dtype=torch.int64, device=dev)[j] + flat % C
    picked = boxes[j, torch.arange(B, device=dev)[:, None], q]                                     # [B, min(k, N), 4]
    scores = torch.zeros((B, k), dtype=cand_scores.dtype, device=dev)
    labels = torch.zeros((B, k), dtype=torch.int64, device=dev)
    xyxy = torch.zeros((B, k, 4), dtype=boxes.dtype, device=dev)
    n_keep = torch.zeros((B,), dtype=torch.int32, device=dev)
    for b, (img_h, img_w, out_h, out_w) in enumerate(sizes.tolist()):
        r = Instances((img_h, img_w))                                                              # dt_inference, per image
        r.pred_boxes = Boxes(box_cxcywh_to_xyxy(picked[b]))
        r.pred_boxes.scale(scale_x=img_w, scale_y=img_h)
        r.scores, r.pred_classes = top[b], label[b]
        r = detector_postprocess(r, out_h, out_w)
        n = len(r)
        scores[b, :n], labels[b, :n], xyxy[b, :n], n_keep[b] = r.scores, r.pred_classes, r.pred_boxes.tensor, n
    return scores, labels, xyxy, n_keep


def supported(cand_scores, cand_index, chunk_start, chunk_classes, label_offset, boxes, k, sizes) -> bool:
    """True where ``merge_detections`` runs the kernel; everything else takes the definition."""
    try:
        start, classes, offset = _table(chunk_start, chunk_classes, label_offset)
        _check(cand_scores, cand_index, start, boxes, k, sizes)
    except ValueError:
        return False
    J, N, B, Q = len(classes), start[-1], cand_scores.shape[0], boxes.shape[2]
    dev = cand_scores.device
    return (cand_scores.is_cuda and cand_scores.dtype == torch.float32 and cand_index.dtype == torch.int64
            and boxes.dtype == torch.float32 and sizes.dtype == torch.float32
            and cand_index.device == dev and boxes.device == dev and sizes.device == dev
            and 1 <= J <= MAX_CHUNKS and 1 <= N <= MAX_CANDIDATES and 1 <= int(k) <= MAX_K and 1 <= B <= MAX_B
            and all(Q * c <= _INT32_MAX and o + c <= _INT32_MAX for c, o in zip(classes, offset)))


def pad_candidates_(cand_scores, cand_index, chunk_start, chunk_classes, Q, k):
    """The padding of short chunks, in place: chunk j has ``min(k, Q * C_j)`` candidates; the positions of its slice behind
    them get a score below every real candidate (-inf) and index 0."""
    for j, C in enumerate(chunk_classes):
        live, end = int(chunk_start[j]) + min(int(k), Q * int(C)), int(chunk_start[j + 1])
        if live < end:
            cand_scores[:, live:end] = float("-inf")
            cand_index[:, live:end] = 0


def merge_detections(cand_scores, cand_index, chunk_start, chunk_classes, label_offset, boxes, k, sizes):
    """``detections_chunked_reference``'s arguments and results as one launch on the current stream: no host
    synchronisation, the chunk table by value (nothing uploaded), no allocation inside the entry, capturable.  The padding
    positions of short chunks are first given a score below every real candidate, in place (``pad_candidates_``; nothing to
    do, and no launch, where every slice is exactly ``min(k, Q * C_j)`` wide).  ``FORCE_REFERENCE`` and the inputs the kernel
    does not serve (``supported``: CPU tensors, other dtypes, more than 64 chunks or 16384 candidate positions, k > 1024) take
    the definition."""
    start, classes, offset = _table(chunk_start, chunk_classes, label_offset)
    _check(cand_scores, cand_index, start, boxes, k, sizes)
    k, N = int(k), start[-1]
    pad_candidates_(cand_scores, cand_index, start, classes, boxes.shape[2], k)
    if FORCE_REFERENCE or not supported(cand_scores, cand_index, start, classes, offset, boxes, k, sizes):
        return detections_chunked_reference(cand_scores, cand_index, start, classes, offset, boxes, k, sizes)
    cand_scores, cand_index = cand_scores.detach()[:, :N].contiguous(), cand_index[:, :N].contiguous()
    boxes, sizes = boxes.detach().contiguous(), sizes.contiguous()
    J, B, Q = boxes.shape[:3]
    table = _lib.VocabChunks()
    table.J, table.n = J, N
    table.start[:J], table.classes[:J], table.label_offset[:J] = start[:J], classes, offset
    dev = cand_scores.device
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    labels = torch.empty((B, k), dtype=torch.int64, device=dev)
    xyxy = torch.empty((B, k, 4), dtype=torch.float32, device=dev)
    n_keep = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().zira_det_merge_f32(cand_scores.data_ptr(), cand_index.data_ptr(), ctypes.byref(table), boxes.data_ptr(),
                                            B, Q, k, sizes.data_ptr(), scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(),
                                            n_keep.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_det_merge_f32 failed: hipError %d" % rc)
    return scores, labels, xyxy, n_keep
