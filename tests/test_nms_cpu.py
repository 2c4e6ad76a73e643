"""The batched box NMS without a GPU: its C ABI is declared in include/zira_nms.h, typed from that header into tables of
its own and exported by the built library; argument errors are answered on the host; ``nms_reference`` on hand-worked cases;
CPU tensors never reach the library; the two tails are what they were while the new arguments stay at their defaults."""
import ctypes
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT
from test_train_step import build_slice_model

from ziragroundingdino_amd import _lib, grounding, nms
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd import transformer as zt
from ziragroundingdino_amd.structures import detector_postprocess

ENTRIES = ["zira_nms_lds_bytes", "zira_nms_f32"]
EINVAL = 1


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_typed_and_exported():
    text = open(os.path.join(ROOT, "include", "zira_nms.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(zira_[a-z0-9_]+)\s*\(", text)
    assert declared == ENTRIES == list(_lib.NMS_SYMBOLS) == list(_lib.NMS_PROTOTYPES)
    zbuild.build_extension()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ENTRIES:
        assert hasattr(raw, sym), "libzira_msda.so does not export %s" % sym
    vp, i, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    P = _lib.NMS_PROTOTYPES
    assert P["zira_nms_lds_bytes"] == (sz, [i])
    assert P["zira_nms_f32"] == (i, [vp, vp, vp, vp, i, i, f32, vp, vp, vp]) and P["zira_nms_f32"][1][6] is f32
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert _lib.NMS_CONSTANTS == {"ZIRA_NMS_MAX_K": 1024, "ZIRA_NMS_MAX_B": 65535}
    assert (nms.MAX_K, nms.MAX_B) == (1024, 65535)


def test_the_first_header_s_surface_is_what_it_was():
    assert len(_lib.SYMBOLS) == 100 and not set(ENTRIES) & set(_lib.SYMBOLS)
    assert not any("NMS" in name for name in _lib.CONSTANTS)
    assert os.path.join(ROOT, "include", "zira_nms.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "nms.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    assert "-ffp-contract=off" in zbuild.EXTRA_FLAGS["nms.hip"]


def test_argument_errors_are_answered_on_the_host():
    """Nothing is launched: there is no device here, and the host pointers are never looked at."""
    lib = _lib.load()

    def call(B=2, K=300, boxes=64, scores=64, labels=None, n=64, keep=64, n_keep=64):
        return lib.zira_nms_f32(boxes, scores, labels, n, B, K, 0.5, keep, n_keep, None)

    for B, K in ((0, 300), (-1, 300), (65536, 300), (2, 0), (2, -5), (2, 1025), (2, 1 << 30)):
        assert call(B=B, K=K) == EINVAL, (B, K)
        assert call(B=B, K=K, labels=64) == EINVAL, (B, K)
    for null in ("boxes", "scores", "n", "keep", "n_keep"):
        assert call(**{null: None}) == EINVAL, null
    assert call(boxes=72) == EINVAL                  # a box moves as 16 bytes
    assert call(labels=68) == EINVAL                 # int64 labels
    for name in ("scores", "n", "keep", "n_keep"):
        assert call(**{name: 66}) == EINVAL, name
    # the LDS the launch takes: the rows' 36 bytes, the sort's exchange buffer, the relation from the diagonal on
    assert lib.zira_nms_lds_bytes(1024) == 1024 * 36 + 1024 * 8 + 32 * 16 * 17 * 8 == 114688
    assert lib.zira_nms_lds_bytes(300) == 320 * 36 + 512 * 8 + 32 * 5 * 6 * 8
    assert lib.zira_nms_lds_bytes(1) == 64 * 36 + 8 + 32 * 2 * 8
    assert lib.zira_nms_lds_bytes(0) == lib.zira_nms_lds_bytes(1025) == lib.zira_nms_lds_bytes(-3) == 0
    assert lib.zira_nms_lds_bytes(1024) + 16 <= 160 * 1024


# ---- the definition on hand-worked cases ---------------------------------------------------------------------------------------
def _one(boxes, scores, thr, labels=None, n=None):
    boxes = torch.tensor(boxes, dtype=torch.float32)[None]
    scores = torch.tensor(scores, dtype=torch.float32)[None]
    labels = None if labels is None else torch.tensor(labels, dtype=torch.int64)[None]
    n = None if n is None else torch.tensor([n], dtype=torch.int32)
    keep, n_keep = nms.nms_reference(boxes, scores, labels, n, thr)
    assert keep.dtype == torch.int32 and n_keep.dtype == torch.int32 and tuple(keep.shape) == tuple(scores.shape)
    k = int(n_keep[0])
    assert bool((keep[0, k:] == -1).all())
    return keep[0, :k].tolist()


def test_iou_exactly_on_the_threshold_is_not_suppressed():
    # [0, 2] x [0, 3] and [0, 3] x [0, 2]: inter 4, union 6 + 6 - 4 = 8, IoU exactly 0.5 in fp32
    a, b = [0, 0, 2, 3], [0, 0, 3, 2]
    assert _one([a, b], [0.9, 0.8], 0.5) == [0, 1]
    assert _one([a, b], [0.9, 0.8], 0.49999997) == [0]          # the next fp32 below 0.5
    # [0, 4] x [0, 1] twice, one shifted by 2: inter 2, union 6, IoU 1 / 3 rounded to fp32; the same division is the threshold
    third = float(torch.tensor(2.0) / torch.tensor(6.0))
    assert _one([[0, 0, 4, 1], [2, 0, 6, 1]], [0.9, 0.8], third) == [0, 1]
    assert _one([[0, 0, 4, 1], [2, 0, 6, 1]], [0.9, 0.8], 0.3333) == [0]


def test_identical_boxes_leave_the_best():
    box = [1, 1, 5, 4]
    assert _one([box] * 4, [0.2, 0.9, 0.5, 0.7], 0.5) == [1]
    assert _one([box] * 4, [0.2, 0.9, 0.5, 0.7], 1.0) == [1, 3, 2, 0]      # IoU 1.0 is not above 1.0


def test_tied_scores_go_by_index():
    far = [[0, 0, 1, 1], [10, 10, 11, 11], [20, 20, 21, 21], [30, 30, 31, 31]]
    assert _one(far, [0.5, 0.5, 0.5, 0.5], 0.5) == [0, 1, 2, 3]
    assert _one(far, [0.5, 0.7, 0.5, 0.7], 0.5) == [1, 3, 0, 2]
    box = [1, 1, 5, 4]
    assert _one([box] * 3, [0.5, 0.5, 0.5], 0.5) == [0]
    assert _one([box] * 3, [0.0, -0.0, 0.0], 0.5) == [0]                    # -0.0 == +0.0


def test_two_zero_area_boxes_are_both_kept():
    point = [2, 2, 2, 2]
    assert _one([point, point], [0.9, 0.8], 0.5) == [0, 1]                 # 0 / 0: NaN compares false
    assert _one([point, point], [0.9, 0.8], 0.0) == [0, 1]


def test_a_suppressed_box_suppresses_nothing():
    # A-B and B-C overlap by 2 / 3 of a box (IoU 0.5), A-C by 1 / 3 (IoU 0.2)
    a, b, c = [0, 0, 6, 1], [2, 0, 8, 1], [4, 0, 10, 1]
    assert _one([a, b, c], [0.9, 0.8, 0.7], 0.4) == [0, 2]
    assert _one([a, b, c], [0.7, 0.9, 0.8], 0.4) == [1]                    # B in front: it removes both
    assert _one([a, b, c], [0.9, 0.8, 0.7], 0.1) == [0]


def test_labels_keep_equal_boxes_of_different_classes():
    box = [1, 1, 5, 4]
    assert _one([box] * 4, [0.9, 0.8, 0.7, 0.6], 0.5, labels=[3, 5, 3, 5]) == [0, 1]
    assert _one([box] * 4, [0.9, 0.8, 0.7, 0.6], 0.5, labels=[3, 3, 3, 3]) == [0]
    assert _one([box] * 4, [0.9, 0.8, 0.7, 0.6], 0.5) == [0]
    # far above any coordinate: compared as labels, not through an offset of the boxes
    assert _one([box] * 2, [0.9, 0.8], 0.5, labels=[1 << 40, (1 << 40) + 1]) == [0, 1]


def test_rows_behind_the_count_do_not_matter():
    box, nan = [1, 1, 5, 4], [float("nan")] * 4
    assert _one([box, [0, 0, 1, 1], nan, [float("inf")] * 4], [0.5, 0.6, float("nan"), float("inf")], 0.5, n=2) == [1, 0]
    assert _one([box, box], [0.5, 0.6], 0.5, n=0) == []
    assert _one([box, box], [0.5, 0.6], 0.5, n=1) == [0]
    assert _one([box, box], [0.5, 0.6], 0.5, n=7) == [1]                   # a count above K is K


def test_the_batch_is_image_by_image():
    g = torch.Generator().manual_seed(5)
    xy = torch.randint(0, 12, (3, 40, 2), generator=g).float()
    boxes = torch.cat([xy, xy + torch.randint(1, 6, (3, 40, 2), generator=g).float()], dim=2)
    scores = torch.randint(0, 8, (3, 40), generator=g).float() / 8
    labels = torch.randint(0, 3, (3, 40), generator=g)
    n = torch.tensor([40, 17, 0], dtype=torch.int32)
    keep, n_keep = nms.nms_reference(boxes, scores, labels, n, 0.3)
    for b in range(3):
        m = int(n[b])
        k1, n1 = nms.nms_reference(boxes[b:b + 1, :m], scores[b:b + 1, :m], labels[b:b + 1, :m], None, 0.3)
        assert int(n1[0]) == int(n_keep[b]) and torch.equal(k1[0, :int(n1[0])], keep[b, :int(n1[0])])
        assert bool((keep[b, int(n_keep[b]):] == -1).all())
    assert 0 < int(n_keep[0]) < 40 and int(n_keep[2]) == 0
    # other dtypes are served in fp32
    k64, n64 = nms.nms_reference(boxes.double(), scores.double(), labels.int(), n.long(), 0.3)
    assert torch.equal(k64, keep) and torch.equal(n64, n_keep)


# ---- the Python surface --------------------------------------------------------------------------------------------------------
def _refuse_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", refuse)


def test_cpu_tensors_and_force_reference_never_reach_the_library(monkeypatch):
    _refuse_library(monkeypatch)
    assert zt.Switches.native_nms is True and nms.FORCE_REFERENCE is False
    boxes = torch.tensor([[[0, 0, 2, 3], [0, 0, 3, 2], [0, 0, 2, 3]]], dtype=torch.float32)
    scores = torch.tensor([[0.5, 0.9, 0.7]])
    n = torch.tensor([3], dtype=torch.int32)
    assert not nms.supported(boxes, scores, None, n)
    keep, n_keep = nms.nms_padded(boxes, scores, None, n, 0.5)
    assert keep.tolist() == [[1, 2, -1]] and n_keep.tolist() == [2]
    meta = dict(device="meta")
    assert not nms.supported(torch.empty(1, 3, 4, **meta), torch.empty(1, 3, **meta))
    monkeypatch.setattr(nms, "FORCE_REFERENCE", True)
    keep, n_keep = nms.nms_padded(boxes, scores, None, None, 0.5)
    assert keep.tolist() == [[1, 2, -1]] and n_keep.tolist() == [2]
    with pytest.raises(ValueError):
        nms.nms_padded(boxes[0], scores, None, n, 0.5)
    with pytest.raises(ValueError):
        nms.nms_padded(boxes, scores, scores, n, 0.5)                      # floating-point labels


def test_nms_and_batched_nms_are_torchvision_s(monkeypatch):
    _refuse_library(monkeypatch)
    box = [1, 1, 5, 4]
    boxes = torch.tensor([box, [10, 10, 12, 12], box, box], dtype=torch.float32)
    scores = torch.tensor([0.3, 0.1, 0.8, 0.5])
    keep = nms.nms(boxes, scores, 0.5)
    assert keep.dtype == torch.int64 and keep.tolist() == [2, 1]
    keep = nms.batched_nms(boxes, scores, torch.tensor([0, 0, 1, 0]), 0.5)
    assert keep.dtype == torch.int64 and keep.tolist() == [2, 3, 1]
    empty = nms.nms(torch.zeros(0, 4), torch.zeros(0), 0.5)
    assert empty.dtype == torch.int64 and tuple(empty.shape) == (0,)
    with pytest.raises(ValueError):
        nms.nms(torch.zeros(3, 5), torch.zeros(3), 0.5)


# ---- behind the tails: nothing changes by default ----------------------------------------------------------------------------
def _postprocess_inputs():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 30, 5, generator=g) * 3
    boxes = torch.rand(2, 30, 4, generator=g)
    boxes[..., 2:] = boxes[..., 2:] * 0.5 + 0.05
    boxes[:, 10:20] = boxes[:, 0:10]                                       # the same query boxes again: duplicates to suppress
    return logits, boxes, [{"height": 90, "width": 120}, {"height": 50, "width": 70}], [(60, 80), (50, 70)]


def test_postprocess_is_what_it_was_by_default(monkeypatch):
    g = torch.load(os.path.join(GOLDEN, "eval_zira_slice.pt"), weights_only=False)
    model = build_slice_model(g, "cpu").eval()
    assert type(model).nms_threshold_for_evaluation is None and model.nms_threshold_for_evaluation is None
    model.select_box_nums_for_evaluation = 40
    logits, boxes, batched, sizes = _postprocess_inputs()
    monkeypatch.setattr(nms, "nms_reference", lambda *a: pytest.fail("NMS ran by default"))
    monkeypatch.setattr(nms, "nms_padded", lambda *a: pytest.fail("NMS ran by default"))
    got = model.postprocess(logits, boxes, batched, sizes)
    old = [detector_postprocess(r, inp["height"], inp["width"])                # the tail as it stood
           for r, inp in zip(model.dt_inference(logits, boxes, sizes), batched)]
    assert len(got) == 2
    for a, b in zip(got, old):
        a = a["instances"]
        assert tuple(a.image_size) == tuple(b.image_size) and len(a) == len(b) > 0
        assert torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)
        assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)


def test_postprocess_with_a_threshold_suppresses_per_class():
    g = torch.load(os.path.join(GOLDEN, "eval_zira_slice.pt"), weights_only=False)
    model = build_slice_model(g, "cpu").eval()
    model.select_box_nums_for_evaluation = 40
    logits, boxes, batched, sizes = _postprocess_inputs()
    plain = model.postprocess(logits, boxes, batched, sizes)
    model.nms_threshold_for_evaluation = 0.5
    got = model.postprocess(logits, boxes, batched, sizes)
    for a, p in zip(got, plain):
        a, p = a["instances"], p["instances"]
        keep = nms.batched_nms(p.pred_boxes.tensor, p.scores, p.pred_classes, 0.5)
        assert 0 < len(keep) < len(p) and len(a) == len(keep)
        assert torch.equal(a.scores, p.scores[keep]) and torch.equal(a.pred_classes, p.pred_classes[keep])
        assert torch.equal(a.pred_boxes.tensor, p.pred_boxes.tensor[keep])
        assert bool((a.scores[:-1] >= a.scores[1:]).all())


class _FakeGrounder:
    """What ``grounding.predict`` touches of a model: two images, six queries, one token per word."""
    training = False

    def __init__(self):
        from ziragroundingdino_amd.bert import SimpleTokenizer

        self.tokenizer = SimpleTokenizer()
        logit = torch.full((2, 6, 8), -20.0)
        # image 0: queries 0, 2 and 5 say "cat" (token 1), query 3 says "dog" (token 3); 0, 2 and 3 are one box
        for q, t, v in ((0, 1, 2.0), (2, 1, 3.0), (5, 1, 1.0), (3, 3, 2.5)):
            logit[0, q, t] = v
        logit[1, 4, 1] = 1.5                                               # image 1: one query
        box = torch.tensor([0.5, 0.5, 0.2, 0.2]).repeat(2, 6, 1)
        box[0, 5] = torch.tensor([0.2, 0.2, 0.1, 0.1])
        self.out = {"pred_logits": logit, "pred_boxes": box}

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def forward_grounding(self, inputs):
        return self.out

    def _captions(self, inputs):
        return [[x["captions"] for x in inputs]]


def test_predict_is_what_it_was_by_default_and_suppresses_on_request(monkeypatch):
    model = _FakeGrounder()
    batch = [{"captions": "cat . dog ."}, {"captions": "cat ."}]
    prob = model.out["pred_logits"].sigmoid()
    want = grounding.ground_reference(prob, model.out["pred_boxes"], 0.5, 0.5, 0)
    assert want.n_keep.tolist() == [4, 1] and want.query[0, :4].tolist() == [0, 2, 3, 5]
    real = nms.nms_padded
    monkeypatch.setattr(nms, "nms_padded", lambda *a: pytest.fail("NMS ran by default"))
    got = grounding.predict(model, batch, 0.5, 0.5)
    table = grounding.tokenize_caption(model.tokenizer, "cat . dog .")
    cat, dog = (grounding.phrases_from_bits(want.token_bits[0, r], table, "cat . dog .") for r in (0, 2))
    assert cat != dog and "cat" in cat
    for b, (boxes, logits, phrases) in enumerate(got):                      # the tail as it stood: the first n rows
        n = int(want.n_keep[b])
        assert torch.equal(boxes, want.box[b, :n]) and torch.equal(logits, want.score[b, :n])
    assert got[0][2] == [cat, cat, dog, cat] and len(got[1][2]) == 1
    monkeypatch.setattr(nms, "nms_padded", real)
    # class-agnostic: of the three equal boxes the best ("cat", query 2) stays; the survivors in the tail's order
    boxes, logits, phrases = grounding.predict(model, batch, 0.5, 0.5, nms_threshold=0.5)[0]
    assert phrases == [cat, cat] and torch.equal(logits, want.score[0, [1, 3]]) and torch.equal(boxes, want.box[0, [1, 3]])
    # per phrase: the "dog" on the same box stays too
    boxes, logits, phrases = grounding.predict(model, batch, 0.5, 0.5, nms_threshold=0.5, nms_per_phrase=True)[0]
    assert phrases == [cat, dog, cat] and torch.equal(logits, want.score[0, [1, 2, 3]])
    # descending-score order of the tail
    boxes, logits, phrases = grounding.predict(model, batch, 0.5, 0.5, 1, nms_threshold=0.5, nms_per_phrase=True)[0]
    assert phrases == [cat, dog, cat] and bool((logits[:-1] >= logits[1:]).all())
    assert len(grounding.predict(model, batch, 0.5, 0.5, nms_threshold=0.5)[1][2]) == 1
