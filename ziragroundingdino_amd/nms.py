"""Box non-maximum suppression with torchvision's meaning (``torchvision.ops.nms`` and, with labels,
``_batched_nms_vanilla``) -- what the reference's model files import from torchvision, which this stack does not have.

Per image the candidates are visited in the stable descending order of their scores (ties to the lower index, topk.py's
order); a candidate is kept unless an earlier KEPT candidate has ``iou > iou_threshold`` with it (strict; a NaN IoU suppresses
nothing) and, with labels, carries the same label.  ``iou = inter / (area_i + area_j - inter)`` in fp32, every operation rounded
on its own.

``nms_reference`` is that definition in torch ops, on any device.  ``nms_padded`` is the same as ONE launch for the batch
(csrc/nms.hip) on padded inputs with a device count per image -- the outputs of ``topk.detections`` and ``grounding.ground`` as
they are -- without a host read, capturable, bit-identical to the definition.  ``nms`` and ``batched_nms`` are torchvision's
two functions on top of it."""
import torch

from . import _lib

MAX_K, MAX_B = _lib.NMS_MAX_K, _lib.NMS_MAX_B
FORCE_REFERENCE = False      # developer switch: every call takes nms_reference


def _check(boxes, scores, labels, n):
    if not (torch.is_tensor(boxes) and boxes.dim() == 3 and boxes.shape[2] == 4 and torch.is_tensor(scores)
            and tuple(scores.shape) == tuple(boxes.shape[:2])):
        raise ValueError("nms: boxes [B, K, 4] (xyxy) and scores [B, K]")
    if labels is not None and not (torch.is_tensor(labels) and tuple(labels.shape) == tuple(scores.shape)
                                   and not labels.is_floating_point()):
        raise ValueError("nms: labels is None or an integer tensor [B, K]")
    if n is not None and not (torch.is_tensor(n) and tuple(n.shape) == (boxes.shape[0],) and not n.is_floating_point()):
        raise ValueError("nms: n is None or an integer tensor [B]")


def nms_reference(boxes, scores, labels, n, iou_threshold):
    """The definition.  boxes [B, K, 4] xyxy, scores [B, K], labels [B, K] integers or None (class-agnostic), n [B] integers
    or None (every row counts) -> (keep [B, K] int32: the kept indices of each image by descending score, -1 behind them;
    n_keep [B] int32), on the inputs' device.  Rows at and behind ``n[b]`` are not looked at.  The arithmetic is fp32 whatever
    the inputs' dtype, and the threshold is rounded to fp32 first, as the kernel receives it.  The pairwise relation is formed on
    the tensors' device; the sweep over it is a host loop (one read per image)."""
    _check(boxes, scores, labels, n)
    B, K = scores.shape
    dev = boxes.device
    thr = torch.tensor(float(iou_threshold), dtype=torch.float32, device=dev)
    keep = torch.full((B, K), -1, dtype=torch.int32, device=dev)
    n_keep = torch.zeros((B,), dtype=torch.int32, device=dev)
    counts = [K] * B if n is None else [min(max(int(c), 0), K) for c in n.tolist()]
    for b, m in enumerate(counts):
        if m == 0:
            continue
        order = torch.sort(scores[b, :m].float(), descending=True, stable=True).indices
        x1, y1, x2, y2 = boxes[b, :m].float()[order].unbind(1)
        area = (x2 - x1) * (y2 - y1)
        w = (torch.minimum(x2[:, None], x2[None, :]) - torch.maximum(x1[:, None], x1[None, :])).clamp(min=0)
        h = (torch.minimum(y2[:, None], y2[None, :]) - torch.maximum(y1[:, None], y1[None, :])).clamp(min=0)
        inter = w * h
        iou = inter / (area[:, None] + area[None, :] - inter)
        hit = iou > thr                                           # [earlier, later] once cut to the upper triangle
        if labels is not None:
            lab = labels[b, :m][order]
            hit &= lab[:, None] == lab[None, :]
        hit = torch.triu(hit, diagonal=1).cpu()
        removed = torch.zeros(m, dtype=torch.bool)
        kept = []
        for i in range(m):
            if not removed[i]:
                kept.append(i)
                removed |= hit[i]
        keep[b, :len(kept)] = order[torch.tensor(kept, dtype=torch.int64, device=dev)].to(torch.int32)
        n_keep[b] = len(kept)
    return keep, n_keep


def supported(boxes, scores, labels=None, n=None) -> bool:
    """True where ``nms_padded`` runs the kernel; everything else takes the definition."""
    if not (torch.is_tensor(boxes) and boxes.is_cuda and boxes.dtype == torch.float32 and boxes.dim() == 3 and boxes.shape[2] == 4
            and torch.is_tensor(scores) and scores.device == boxes.device and scores.dtype == torch.float32
            and tuple(scores.shape) == tuple(boxes.shape[:2]) and 1 <= boxes.shape[0] <= MAX_B and 1 <= boxes.shape[1] <= MAX_K):
        return False
    if labels is not None and not (torch.is_tensor(labels) and labels.device == boxes.device and labels.dtype == torch.int64
                                   and tuple(labels.shape) == tuple(scores.shape)):
        return False
    return n is None or (torch.is_tensor(n) and n.device == boxes.device and n.dtype == torch.int32
                         and tuple(n.shape) == (boxes.shape[0],))


def nms_padded(boxes, scores, labels, n, iou_threshold):
    """``nms_reference``'s arguments and results as one launch on the current stream: no host synchronisation, no allocation
    inside the entry, capturable.  ``Switches.native_nms = False``, ``FORCE_REFERENCE`` and the inputs the kernel does not
    serve (``supported``: CPU tensors, other dtypes, K > 1024) take ``nms_reference``."""
    from .transformer import Switches

    _check(boxes, scores, labels, n)
    if FORCE_REFERENCE or not Switches.native_nms or not supported(boxes, scores, labels, n):
        return nms_reference(boxes, scores, labels, n, iou_threshold)
    boxes, scores = boxes.detach().contiguous(), scores.detach().contiguous()
    labels = None if labels is None else labels.contiguous()
    B, K = scores.shape
    dev = boxes.device
    n = torch.full((B,), K, dtype=torch.int32, device=dev) if n is None else n.contiguous()
    keep = torch.empty((B, K), dtype=torch.int32, device=dev)
    n_keep = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().zira_nms_f32(boxes.data_ptr(), scores.data_ptr(), None if labels is None else labels.data_ptr(),
                                      n.data_ptr(), B, K, float(iou_threshold), keep.data_ptr(), n_keep.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_nms_f32 failed: hipError %d" % rc)
    return keep, n_keep


def nms(boxes, scores, iou_threshold):
    """``torchvision.ops.nms``: boxes [N, 4] xyxy, scores [N] -> the int64 indices of the kept boxes by decreasing score.  One
    launch and one host read, for the length."""
    return batched_nms(boxes, scores, None, iou_threshold)


def batched_nms(boxes, scores, idxs, iou_threshold):
    """``torchvision.ops.batched_nms``: as ``nms``, boxes of different ``idxs`` [N] never suppressing each other (compared as
    labels, ``_batched_nms_vanilla``'s way, not through the coordinate offset)."""
    if not (torch.is_tensor(boxes) and boxes.dim() == 2 and boxes.shape[1] == 4 and torch.is_tensor(scores)
            and tuple(scores.shape) == (boxes.shape[0],)):
        raise ValueError("nms: boxes [N, 4] (xyxy) and scores [N]")
    if boxes.shape[0] == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    if idxs is not None and idxs.is_cuda and not idxs.is_floating_point():
        idxs = idxs.to(torch.int64)
    keep, n_keep = nms_padded(boxes[None], scores[None], None if idxs is None else idxs[None], None, iou_threshold)
    return keep[0, :int(n_keep[0])].to(torch.int64)
