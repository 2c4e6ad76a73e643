"""The batched box NMS on the GPU (csrc/nms.hip): ``keep`` and ``n_keep`` bit for bit those of ``nms.nms_reference`` on the
host copy of the same batch -- every K at which the kernel takes another path (one word, a word boundary, the model's 300 and
900, the limit), counts 0 / 1 / K - 1 / K with NaN and inf behind them, boxes on an integer grid (pairs exactly on the
threshold), dense clusters, identical boxes, tied scores, 1 / 7 / 80 labels and none -- then capture and replay, and the two
tails with the suppression behind them against ``Switches.native_nms = False``."""
import functools
import os

import pytest
import torch

from conftest import GOLDEN
from test_train_step import build_slice_model

from ziragroundingdino_amd import _lib, grounding, nms, topk
from ziragroundingdino_amd import transformer as zt

pytestmark = pytest.mark.gpu

KS = [1, 2, 63, 64, 65, 300, 900, 1024]
BS = [1, 2, 8]
THRS = [0.0, 0.5, 1.0]
KINDS = ["grid", "clusters", "identical", "tied"]
LABELS = [None, 1, 7, 80]


@functools.lru_cache(maxsize=None)
def make(kind, B, K, n_labels, turn):
    """(boxes [B, K, 4], scores [B, K], labels [B, K] or None, n [B]) on the host.  ``turn`` rotates which image gets which of
    the counts K, K - 1, 1, 0 and a random one; the rows at and behind a count are NaN and inf."""
    g = torch.Generator().manual_seed(1000 * K + 10 * B + turn)
    side = max(3, int(K ** 0.5))
    xy = torch.randint(0, side, (B, K, 2), generator=g).float()
    boxes = torch.cat([xy, xy + torch.randint(1, 5, (B, K, 2), generator=g).float()], dim=2)   # integers: exact IoUs
    scores = torch.randint(0, 16, (B, K), generator=g).float() / 16                              # many ties
    if kind == "clusters":        # a box per 16 candidates, each with copies moved by a few percent of its side
        centres = boxes[:, torch.randint(0, K, (K,), generator=g) // 16 * 16 % K]
        boxes = centres + (torch.rand(B, K, 4, generator=g) - 0.5) * 0.3
        scores = torch.rand(B, K, generator=g)
    elif kind == "identical":
        boxes = torch.tensor([3.0, 2.0, 11.0, 7.0]).repeat(B, K, 1)
    elif kind == "tied":
        scores = torch.full((B, K), 0.5)
    labels = None if n_labels is None else torch.randint(0, n_labels, (B, K), generator=g)
    counts = [K, K - 1, 1, 0, int(torch.randint(0, K + 1, (1,), generator=g))]
    n = torch.tensor([min(max(counts[(b + turn) % 5], 0), K) for b in range(B)], dtype=torch.int32)
    for b in range(B):
        m = int(n[b])
        boxes[b, m::2] = float("nan")
        boxes[b, m + 1::2] = float("inf")
        scores[b, m::3] = float("nan")
        scores[b, m + 1::3] = float("inf")
        scores[b, m + 2::3] = 2.0                     # above every live score
    return boxes, scores, labels, n


@functools.lru_cache(maxsize=None)
def reference(kind, B, K, n_labels, turn, thr):
    return nms.nms_reference(*make(kind, B, K, n_labels, turn), thr)


def _cuda(case):
    return tuple(None if t is None else t.cuda() for t in case)


def _assert_equal(got, want, what):
    keep, n_keep = (t.cpu() for t in got)
    assert keep.dtype == want[0].dtype == torch.int32 and n_keep.dtype == want[1].dtype == torch.int32, what
    assert torch.equal(n_keep, want[1]), (what, n_keep.tolist(), want[1].tolist())
    assert torch.equal(keep, want[0]), what


def combos():
    """Every kind with every threshold; the label form and the counts' rotation move along with them, so that each (K, B)
    sees every label form and every count on every image."""
    return [(kind, LABELS[(i + j) % 4], (i + 2 * j) % 5, thr) for j, thr in enumerate(THRS) for i, kind in enumerate(KINDS)]


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("K", KS)
def test_kernel_equals_reference(K, B):
    assert zt.Switches.native_nms is True
    for kind, n_labels, turn, thr in combos():
        case = make(kind, B, K, n_labels, turn)
        assert nms.supported(*_cuda(case))
        got = nms.nms_padded(*_cuda(case), thr)
        _assert_equal(got, reference(kind, B, K, n_labels, turn, thr), (kind, n_labels, turn, thr))


def test_cases_hold_what_they_are_for():
    seen_labels, seen_counts = set(), set()
    for kind, n_labels, turn, thr in combos():
        seen_labels.add(n_labels)
        boxes, scores, labels, n = make(kind, 8, 300, n_labels, turn)
        seen_counts |= set(n.tolist())
        keep, n_keep = reference(kind, 8, 300, n_labels, turn, thr)
        full = [b for b in range(8) if int(n[b]) >= 299]
        assert full
        for b in full:
            m, k = int(n[b]), int(n_keep[b])
            if thr == 1.0:
                assert k == m                                    # nothing is above 1.0
            elif kind == "identical" and n_labels is None:
                assert k == 1
            elif kind == "identical":
                assert k == len(set(labels[b, :m].tolist()))     # one per label
            else:
                assert 1 < k < m, (kind, thr, k, m)              # some suppressed, some kept
    assert seen_labels == set(LABELS) and {0, 1, 299, 300} <= seen_counts
    # the grid puts pairs exactly on the threshold: IoU == 0.5 among the live rows, kept apart only by the strict comparison
    boxes, scores, labels, n = make("grid", 1, 300, None, 0)
    x1, y1, x2, y2 = boxes[0].unbind(1)
    area = (x2 - x1) * (y2 - y1)
    inter = ((torch.minimum(x2[:, None], x2[None]) - torch.maximum(x1[:, None], x1[None])).clamp(min=0)
             * (torch.minimum(y2[:, None], y2[None]) - torch.maximum(y1[:, None], y1[None])).clamp(min=0))
    iou = inter / (area[:, None] + area[None] - inter)
    assert int((iou == 0.5).sum()) >= 100
    loose = nms.nms_reference(boxes, scores, None, n, 0.49999997)[1]
    assert int(loose[0]) < int(reference("grid", 1, 300, None, 0, 0.5)[1][0])


def test_two_runs_give_the_same_bits_and_padding_does_not_matter():
    boxes, scores, labels, n = _cuda(make("clusters", 2, 900, 7, 1))
    first = nms.nms_padded(boxes, scores, labels, n, 0.5)
    again = nms.nms_padded(boxes, scores, labels, n, 0.5)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    for b in range(2):                                           # other garbage behind the counts
        boxes[b, int(n[b]):] = -7.0
        scores[b, int(n[b]):] = 9.0
        labels[b, int(n[b]):] = -1
    other = nms.nms_padded(boxes, scores, labels, n, 0.5)
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
    assert int(n.min()) < 900                                    # (there was padding)


@pytest.mark.parametrize("K,n_labels", [(300, 80), (1024, None)])
def test_capture_and_replay_on_three_inputs(K, n_labels):
    B, thr = 2, 0.5
    cases = [make(kind, B, K, n_labels, turn) for kind, turn in (("grid", 0), ("clusters", 1), ("tied", 3))]
    eager = [tuple(t.cpu() for t in nms.nms_padded(*_cuda(c), thr)) for c in cases]
    boxes_s, scores_s = torch.zeros(B, K, 4, device="cuda"), torch.zeros(B, K, device="cuda")
    labels_s = None if n_labels is None else torch.zeros(B, K, dtype=torch.int64, device="cuda")
    n_s = torch.zeros(B, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up off the default stream, as torch's capture asks
        nms.nms_padded(boxes_s, scores_s, labels_s, n_s, thr)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = nms.nms_padded(boxes_s, scores_s, labels_s, n_s, thr)
    for (boxes, scores, labels, n), want in zip(cases, eager):
        boxes_s.copy_(boxes)
        scores_s.copy_(scores)
        n_s.copy_(n)
        if labels is not None:
            labels_s.copy_(labels)
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(out, want, "replay")
    assert len({tuple(w[1].tolist()) for w in eager}) == 3       # three different answers


def test_c_entry_refuses_without_launching_and_python_declines():
    lib = _lib.load()
    boxes, scores, labels, n = _cuda(make("grid", 2, 64, 7, 0))
    keep = torch.full((2, 64), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    n_keep = torch.full((2,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")

    def call(B=2, K=64, boxes_ptr=None, n_ptr=n.data_ptr()):
        return lib.zira_nms_f32(boxes_ptr or boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), n_ptr, B, K, 0.5,
                                keep.data_ptr(), n_keep.data_ptr(), torch.cuda.current_stream().cuda_stream)

    for bad in (dict(B=0), dict(B=65536), dict(K=0), dict(K=1025), dict(boxes_ptr=boxes.data_ptr() + 4), dict(n_ptr=None)):
        assert call(**bad) == 1, bad                             # ZIRA_MSDA_EINVAL
    torch.cuda.synchronize()
    assert bool((keep == 0x7F7F7F7F).all()) and bool((n_keep == 0x7F7F7F7F).all())      # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    _assert_equal((keep, n_keep), reference("grid", 2, 64, 7, 0, 0.5), "after the refusals")
    # what the kernel does not serve takes the definition, on the device
    big = torch.rand(1, 1025, 4, device="cuda")
    assert not nms.supported(big, torch.rand(1, 1025, device="cuda"))
    assert not nms.supported(boxes.double(), scores.double()) and not nms.supported(boxes, scores, labels.int())
    got = nms.nms_padded(boxes.double(), scores.double(), labels.int(), n.long(), 0.5)
    _assert_equal(got, reference("grid", 2, 64, 7, 0, 0.5), "fp64 on the device")


def test_nms_and_batched_nms_on_the_device():
    boxes, scores, labels, _ = make("grid", 1, 300, 7, 0)
    want = nms.nms_reference(boxes, scores, None, None, 0.5)
    got = nms.nms(boxes[0].cuda(), scores[0].cuda(), 0.5)
    assert got.dtype == torch.int64 and got.is_cuda and got.tolist() == want[0][0, :int(want[1][0])].tolist()
    want = nms.nms_reference(boxes, scores, labels, None, 0.5)
    got = nms.batched_nms(boxes[0].cuda(), scores[0].cuda(), labels[0].cuda(), 0.5)
    assert got.dtype == torch.int64 and got.tolist() == want[0][0, :int(want[1][0])].tolist()


# ---- behind the tails ----------------------------------------------------------------------------------------------------------
SIZES = [((800, 1333), (800, 1333)), ((640, 1066), (480, 799))]


def _instances_equal(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = a["instances"], b["instances"]
        assert tuple(a.image_size) == tuple(b.image_size) and list(a.__dict__) == list(b.__dict__) and len(a) == len(b)
        assert a.scores.dtype == b.scores.dtype and a.pred_classes.dtype == b.pred_classes.dtype
        assert torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)
        assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)


def test_postprocess_with_nms_native_equals_reference(monkeypatch):
    g = torch.load(os.path.join(GOLDEN, "eval_zira_slice.pt"), weights_only=False)
    model = build_slice_model(g, "cuda").eval()
    model.select_box_nums_for_evaluation = 300
    gen = torch.Generator().manual_seed(17)
    Q, C = 900, 7
    logits = (torch.randn(2, Q, C, generator=gen) * 3).cuda()
    boxes = torch.rand(2, Q, 4, generator=gen)
    boxes[..., 2:] = boxes[..., 2:] * 0.3 + 0.05
    boxes[:, 300:] = boxes[:, :300].repeat(1, 2, 1) + (torch.rand(2, 600, 4, generator=gen) - 0.5) * 0.02   # near-duplicates
    boxes = boxes.cuda()
    batched = [{"height": o[0], "width": o[1]} for _, o in SIZES]
    sizes = [s for s, _ in SIZES]
    launches, reads = [], []
    real, real_ref = nms.nms_padded, nms.nms_reference
    monkeypatch.setattr(nms, "nms_padded", lambda *a: (launches.append(1), real(*a))[1])
    monkeypatch.setattr(nms, "nms_reference", lambda *a: (reads.append(1), real_ref(*a))[1])
    with torch.no_grad():
        plain = model.postprocess(logits, boxes, batched, sizes)
        assert launches == []
        model.nms_threshold_for_evaluation = 0.5
        got = model.postprocess(logits, boxes, batched, sizes)
        assert launches == [1] and reads == []                    # one call for the batch, on the kernel
        monkeypatch.setattr(zt.Switches, "native_nms", False)
        want = model.postprocess(logits, boxes, batched, sizes)
        assert launches == [1, 1] and reads == [1]
        _instances_equal(got, want)
        monkeypatch.setattr(zt.Switches, "native_detections", False)    # the op chain applies the definition per image
        monkeypatch.setattr(torch, "topk", lambda x, kk, dim=-1: topk.sorted_rows(x, kk))
        chain = model.postprocess(logits, boxes, batched, sizes)
        _instances_equal(got, chain)
    for a, p in zip(got, plain):
        assert 0 < len(a["instances"]) < len(p["instances"])     # some suppressed
        s = a["instances"].scores
        assert bool((s[:-1] >= s[1:]).all())


def test_predict_with_nms_native_equals_reference(monkeypatch):
    from test_model_gpu import small_model

    from ziragroundingdino_amd.train import synthetic_batch

    model = small_model().eval()
    a = synthetic_batch(1, 224, 320, n_categories=4, boxes_per_image=3, seed=1, device="cuda")[0]
    b = synthetic_batch(1, 200, 272, n_categories=2, boxes_per_image=1, seed=2, device="cuda")[0]
    a["captions"], b["captions"] = "Fish . Jellyfish . Penguin . Puffin", "a shark . starfish ."
    batch = [a, b]
    memo, real_forward = {}, model.forward_grounding

    def forward_once(inputs):                                    # the model runs once: the comparison is of the tails
        key = tuple(x["captions"] for x in inputs)
        if key not in memo:
            out = dict(real_forward(inputs))
            boxes = out["pred_boxes"].clone()                    # every odd query repeats its neighbour's box: duplicates,
            boxes[:, 1::2] = boxes[:, 0::2][:, :boxes.shape[1] // 2]      # which the untrained model does not give by itself
            memo[key] = dict(out, pred_boxes=boxes)
        return memo[key]

    monkeypatch.setattr(model, "forward_grounding", forward_once)
    with torch.no_grad():
        out = model.forward_grounding([dict(x, captions=grounding.preprocess_caption(x["captions"])) for x in batch])
    prob = out["pred_logits"].sigmoid().cpu()
    s = prob.max(dim=2).values
    box_thr = max(float(s[i].quantile(0.25)) for i in range(2))  # about three quarters of the queries pass
    text_thr = float(prob[prob > 0].quantile(0.5))
    plain = grounding.predict(model, batch, box_thr, text_thr)
    assert all(len(p[2]) > 1 for p in plain)
    for order, per_phrase in ((0, False), (1, False), (0, True)):
        monkeypatch.setattr(zt.Switches, "native_nms", True)
        got = grounding.predict(model, batch, box_thr, text_thr, order, nms_threshold=0.5, nms_per_phrase=per_phrase)
        monkeypatch.setattr(zt.Switches, "native_nms", False)
        want = grounding.predict(model, batch, box_thr, text_thr, order, nms_threshold=0.5, nms_per_phrase=per_phrase)
        for (gb, gl, gp), (wb, wl, wp), (pb, pl, pp) in zip(got, want, plain):
            assert torch.equal(gb, wb) and torch.equal(gl, wl) and gp == wp
            assert all(isinstance(p, str) for p in gp) and 0 < len(gp) <= len(pp) and len(gp) == gb.shape[0] == gl.shape[0]
            if order == 1:
                assert bool((gl[:-1] >= gl[1:]).all())
            if not per_phrase:
                assert len(gp) < len(pp)                         # of two kept queries with one box one is gone
    assert len(memo) == 1
