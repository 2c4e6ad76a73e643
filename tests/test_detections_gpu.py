"""The native evaluation tail (``zira_detections_f32`` through ``GroundingDINO.postprocess`` with ``Switches.native_detections``)
against the chain it stands for on the same device -- ``dt_inference`` + ``structures.detector_postprocess`` -- with
``torch.equal`` on every field: with the chain's top-k replaced by the stable-sort definition where probabilities tie
(saturated logits, the -100 fill), with ``torch.topk`` itself where nothing ties, and on the reference's own detections
(tests/golden/eval_zira_slice.pt, read only)."""
import os

import pytest
import torch

from conftest import GOLDEN
from test_modules_golden import close
from test_train_step import build_slice_model, slice_inputs

from ziragroundingdino_amd import topk
from ziragroundingdino_amd import transformer as zt

pytestmark = pytest.mark.gpu

# (network input size, requested output size): the same size, a non-integer ratio, twice the size
SIZES = [((800, 1333), (800, 1333)), ((640, 1066), (480, 799)), ((600, 900), (1200, 1800))]


@pytest.fixture(scope="module")
def model():
    g = torch.load(os.path.join(GOLDEN, "eval_zira_slice.pt"), weights_only=False)
    return build_slice_model(g, "cuda").eval()


def _inputs(Q, C, tie_free, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(SIZES)
    if tie_free:   # distinct logits 1.3e-3 apart in [-4, 4]: the sigmoid's slope there keeps the probabilities > 2e-5 apart
        logits = torch.stack([torch.linspace(-4, 4, Q * C)[torch.randperm(Q * C, generator=g)] for _ in range(B)]).view(B, Q, C)
    else:
        logits = torch.randn(B, Q, C, generator=g) * 12          # |x| > 20 saturates: exact ties at 1.0 and near 0
        logits[:, :, C // 2:] = -100.0                           # recover_to_cls_logits' fill: one tied block
        logits[:, ::5] = logits[:, 1::5][:, :logits[:, ::5].shape[1]]   # whole rows repeated
    boxes = torch.rand(B, Q, 4, generator=g)
    boxes[..., 2:] *= 0.6
    boxes[:, ::7, 0] += 0.8                                      # leave the image on the right
    boxes[:, 3::11, 1] -= 0.7                                    # ... and at the top
    boxes[:, 2::9, 2] = 0.0                                      # no width
    boxes[:, 4::13, 3] = 0.0                                     # no height
    boxes[:, 5::17, :2] = 1.5                                    # wholly outside: clipped to nothing
    return logits.cuda(), boxes.cuda()


def _run(model, logits, boxes, native, monkeypatch, k):
    monkeypatch.setattr(zt.Switches, "native_detections", native)
    model.select_box_nums_for_evaluation = k
    batched = [{"height": o[0], "width": o[1]} for _, o in SIZES]
    with torch.no_grad():
        return model.postprocess(logits, boxes, batched, [s for s, _ in SIZES])


def _assert_equal(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = a["instances"], b["instances"]
        assert tuple(a.image_size) == tuple(b.image_size)
        assert list(a.__dict__) == list(b.__dict__)
        assert len(a) == len(b)
        assert a.scores.dtype == b.scores.dtype and a.pred_classes.dtype == b.pred_classes.dtype
        assert a.pred_boxes.tensor.dtype == b.pred_boxes.tensor.dtype and a.pred_boxes.tensor.shape == b.pred_boxes.tensor.shape
        assert torch.equal(a.scores, b.scores)
        assert torch.equal(a.pred_classes, b.pred_classes)
        assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)


@pytest.mark.parametrize("Q,C,k", [(900, 7, 300), (900, 96, 300), (900, 256, 300), (50, 4, 200), (900, 7, 1000)])
def test_native_tail_equals_the_chain_with_the_stable_sort(model, monkeypatch, Q, C, k):
    logits, boxes = _inputs(Q, C, False, Q + C)
    calls = []
    real = topk.detections
    monkeypatch.setattr(topk, "detections", lambda *a: (calls.append(1), real(*a))[1])
    got = _run(model, logits, boxes, True, monkeypatch, k)
    assert calls == [1]                                          # one call for the batch
    monkeypatch.setattr(torch, "topk", lambda x, kk, dim=-1: topk.sorted_rows(x, kk))
    want = _run(model, logits, boxes, False, monkeypatch, k)
    assert calls == [1]
    _assert_equal(got, want)
    assert 0 < min(len(r["instances"]) for r in got) and max(len(r["instances"]) for r in got) < k   # some kept, some dropped


@pytest.mark.parametrize("Q,C,k", [(900, 7, 300), (900, 96, 300)])
def test_native_tail_equals_the_unmodified_chain_where_nothing_ties(model, monkeypatch, Q, C, k):
    logits, boxes = _inputs(Q, C, True, Q * C)
    prob = logits.sigmoid().view(len(SIZES), -1)
    assert all(int(torch.unique(r).numel()) == Q * C for r in prob)
    got = _run(model, logits, boxes, True, monkeypatch, k)
    want = _run(model, logits, boxes, False, monkeypatch, k)     # torch.topk as it is
    _assert_equal(got, want)


def test_eval_branch_matches_reference_with_the_native_tail(model, monkeypatch):
    """tests/test_train_step.py::test_eval_branch_matches_reference, its assertions and tolerances, with the native tail on."""
    g = torch.load(os.path.join(GOLDEN, "eval_zira_slice.pt"), weights_only=False)
    monkeypatch.setattr(zt.Switches, "native_detections", True)
    calls = []
    real = topk.detections
    monkeypatch.setattr(topk, "detections", lambda *a: (calls.append(1), real(*a))[1])
    model.select_box_nums_for_evaluation = g["topk"]
    inp, feats, poss, am, pid, c2t = slice_inputs(g, model, "cuda")
    with torch.no_grad():
        text_dict, loss_lin = model.project_text(inp["bert_hidden"], torch.ones_like(inp["input_ids"]).bool(), pid, am)
        out = model.forward_features(feats, poss, inp["img_mask"], text_dict, c2t, loss_lin, None)
        close(out["pred_logits"], g["pred_logits"], 1e-4, "pred_logits")
        close(out["pred_boxes"], g["pred_boxes"], 1e-4, "pred_boxes")
        batched = [{"height": h, "width": w} for h, w in g["output_sizes"]]
        res = model.postprocess(out["pred_logits"], out["pred_boxes"], batched, g["image_sizes"])
    assert calls == [1]
    assert len(res) == len(g["results"])
    for r, want, osize in zip(res, g["results"], g["output_sizes"]):
        inst = r["instances"]
        assert tuple(inst.image_size) == tuple(osize)
        assert len(inst) == len(want["scores"])
        close(inst.scores, want["scores"], 1e-5, "scores")
        got = sorted(zip(inst.pred_classes.tolist(), [tuple(round(v, 1) for v in b) for b in inst.pred_boxes.tensor.tolist()]))
        ref = sorted(zip(want["pred_classes"].tolist(), [tuple(round(v, 1) for v in b) for b in want["pred_boxes"].tolist()]))
        assert [c for c, _ in got] == [c for c, _ in ref]
        for (_, a), (_, b) in zip(got, ref):
            assert max(abs(x - y) for x, y in zip(a, b)) <= 0.2, (a, b)
