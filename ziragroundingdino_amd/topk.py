"""Row-wise top-k with ONE meaning on every device (csrc/topk.hip): the first k entries of a stable descending sort of each
row -- values descending, equal values by ascending index, -0.0 == +0.0, NaN first -- so the selection depends on the input
alone.  ``torch.topk`` leaves the order of ties open and cannot be replayed from a hipGraph on this stack (graphs.py);
``torch.sort`` sorts 22 223 keys for a 900-element answer.  On the GPU this is one launch of one block per row, without host
synchronisation, global atomics or allocation inside the entry, so it can be captured and replayed.

``detections`` is the evaluation tail on top of it (``GroundingDINO.dt_inference`` + ``structures.detector_postprocess``) in
the same launch, bit-identical to the op chain."""
import torch

from . import _lib

MAX_K, MAX_N, MAX_ROWS = 1024, 1 << 20, 65535
_WS = {}


def _limits(rows, n, k) -> bool:
    return 1 <= k <= MAX_K and k <= n <= MAX_N and 1 <= rows <= MAX_ROWS


def supported(x, k) -> bool:
    """True where ``topk_rows`` runs the kernel; everything else takes the sort that defines it."""
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and _limits(x.shape[0], x.shape[1], int(k)))


def _workspace(dev, nbytes):
    """The entry's workspace, cached per (device, stream) like ``dense._scratch``; inside a capture it comes from the graph's pool."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def sorted_rows(x, k):
    """The definition: ``torch.sort(stable=True, descending=True)`` cut to k."""
    val, idx = torch.sort(x, dim=1, descending=True, stable=True)
    return val[:, :k], idx[:, :k]


def topk_rows(x, k):
    """(values [rows, k], indices [rows, k] int64) of ``x`` [rows, n]."""
    k = int(k)
    if not supported(x, k):
        return sorted_rows(x, k)
    x = x.detach().contiguous()
    rows, n = x.shape
    lib = _lib.load()
    nbytes = lib.zira_topk_rows_workspace_bytes(rows, n, k)
    if nbytes == 0:
        raise RuntimeError("zira_topk_rows_f32 does not serve rows=%d n=%d k=%d" % (rows, n, k))
    val = torch.empty((rows, k), dtype=torch.float32, device=x.device)
    idx = torch.empty((rows, k), dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        ws = _workspace(x.device, nbytes)
        rc = lib.zira_topk_rows_f32(x.data_ptr(), rows, n, k, val.data_ptr(), idx.data_ptr(), ws.data_ptr(), nbytes,
                                    torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_topk_rows_f32 failed: hipError %d" % rc)
    return val, idx


def detections_supported(prob, boxes, k) -> bool:
    return (torch.is_tensor(prob) and prob.is_cuda and prob.dtype == torch.float32 and prob.dim() == 3
            and torch.is_tensor(boxes) and boxes.device == prob.device and boxes.dtype == torch.float32
            and tuple(boxes.shape) == tuple(prob.shape[:2]) + (4,) and prob.shape[1] >= 1 and prob.shape[2] >= 1
            and _limits(prob.shape[0], prob.shape[1] * prob.shape[2], int(k)))


def detections(prob, boxes, k, sizes):
    """prob [B, Q, C], boxes [B, Q, 4] cxcywh in 0..1, sizes [B, 4] = (img_h, img_w, out_h, out_w) fp32 on the device ->
    (scores [B, k], labels [B, k] int64, xyxy [B, k, 4], n_keep [B] int32): per image the top-k (query, class) entries whose
    clipped box is not empty, in score order, ``n_keep[b]`` of them (the rest of a row is zero)."""
    k = int(k)
    if not detections_supported(prob, boxes, k):
        raise RuntimeError("zira_detections_f32 does not serve these inputs")
    prob, boxes = prob.detach().contiguous(), boxes.detach().contiguous()
    B, Q, C = prob.shape
    assert tuple(sizes.shape) == (B, 4) and sizes.dtype == torch.float32 and sizes.device == prob.device and sizes.is_contiguous()
    lib = _lib.load()
    nbytes = lib.zira_topk_rows_workspace_bytes(B, Q * C, k)
    dev = prob.device
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    labels = torch.empty((B, k), dtype=torch.int64, device=dev)
    xyxy = torch.empty((B, k, 4), dtype=torch.float32, device=dev)
    n_keep = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(dev, nbytes)
        rc = lib.zira_detections_f32(prob.data_ptr(), boxes.data_ptr(), B, Q, C, k, sizes.data_ptr(), scores.data_ptr(),
                                     labels.data_ptr(), xyxy.data_ptr(), n_keep.data_ptr(), ws.data_ptr(), nbytes,
                                     torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_detections_f32 failed: hipError %d" % rc)
    return scores, labels, xyxy, n_keep
