"""``zira_lvis_match`` on the GPU (csrc/lvismatch.hip): every output element bit for bit that of ``match_reference`` on the host
copy of the same inputs (and so of lvis_oracle, which the CPU tests pin the reference to), nothing masked out; pinned to the
COCO kernel where the federated rules have nothing to say; run-to-run identity; capture and replay; the evaluator on device
state against the evaluator on CPU state; and the slice model with a chunked category list through ``inference_on_dataset``."""
import ctypes

import numpy as np
import pytest
import torch

import lvis_cases as cases
from test_lvis_cpu import EVAL_CASES, FREQ70, batch_of

pytestmark = pytest.mark.gpu

from ziragroundingdino_amd import _lib  # noqa: E402
from ziragroundingdino_amd import evaluation as ev  # noqa: E402
from ziragroundingdino_amd import lvis_evaluation as lv  # noqa: E402

DEV = "cuda"
EINVAL = 1


def raw_match(t, C, max_det, thrs=cases.IOU_THRS, rngs=cases.AREA_RNGS, fill=0xFF, **override):
    """The C entry on buffers pre-filled with ``fill`` (so an element the kernel leaves alone shows).  -> (rc, outputs)."""
    lib = _lib.load()
    scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_ignore, n_gt, neg, nel = t
    b, k = scores.shape
    g = gt_label.shape[1]
    T, A = len(thrs), len(rngs)
    byte = lambda shape, dt: torch.full((int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size(),), fill, dtype=torch.uint8,
                                        device=DEV).view(dt).view(shape)
    out = [byte((b, k), torch.int32), byte((b, k), torch.int64), byte((b, k), torch.int64), byte((b, g), torch.uint8),
           byte((b, k, min(A * T, 64)), torch.int32)]
    ptr = lambda x: x.data_ptr() if x.numel() else None
    o = lambda name, value: override.get(name, value)
    rc = lib.zira_lvis_match(scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(), n_keep.data_ptr(), o("B", b), o("K", k),
                             ptr(gt_xywh), ptr(gt_area), ptr(gt_label), ptr(gt_ignore), ptr(n_gt), o("G", g),
                             o("neg", neg.data_ptr()), nel.data_ptr(), o("C", C), (ctypes.c_double * T)(*thrs), T,
                             (ctypes.c_double * (2 * A))(*[v for r in rngs for v in r]), A, max_det,
                             out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ptr(out[3]), out[4].data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def assert_equal(got, want, what):
    for k in cases.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %s" % (what, k, np.argwhere(got[k] != want[k])[:5].tolist())


def reference(case, **kw):
    args = dict(thrs=cases.IOU_THRS, rngs=cases.AREA_RNGS, max_det=case["max_det"])
    args.update(kw)
    return cases.as_numpy(lv.match_reference(*cases.tensors(case), case["C"], args["thrs"], args["rngs"], args["max_det"]))


@pytest.mark.parametrize("name", cases.names())
def test_kernel_equals_the_definition_everywhere(name):
    """Through the raw entry on 0xFF-filled buffers (what the kernel writes behind the counts is part of the reference's arrays:
    -1 / 0) and through the wrapper; the oracle's arrays, which the reference equals on the CPU, beside them."""
    case = cases.get(name)
    t = cases.tensors(case, DEV)
    want = reference(case)
    rc, out = raw_match(t, case["C"], case["max_det"])
    assert rc == 0
    assert_equal(cases.as_numpy(out), want, name + " (raw entry)")
    assert lv.match_supported(*t, case["C"], cases.IOU_THRS, cases.AREA_RNGS, case["max_det"])
    got = lv.match(*t, case["C"], cases.IOU_THRS, cases.AREA_RNGS, case["max_det"])
    assert_equal(cases.as_numpy(got), want, name + " (wrapper)")
    assert_equal(cases.as_numpy(got), cases.expected(case), name + " (oracle)")


def test_other_parameters_and_the_optional_gt_of():
    """One threshold and one range (a single wave), 16 x 4 (64 problems on 16 waves), max_det inside a row, no gt_of."""
    case = cases.get("wide")
    t = cases.tensors(case, DEV)
    thr16 = tuple(0.5 + 0.03 * i for i in range(16))
    for thrs, rngs, max_det in ((cases.IOU_THRS[:1], cases.AREA_RNGS[:1], 65), (thr16, cases.AREA_RNGS, 65),
                                (cases.IOU_THRS, cases.AREA_RNGS[1:3], 33), (cases.IOU_THRS, cases.AREA_RNGS, 1)):
        want = reference(case, thrs=thrs, rngs=rngs, max_det=max_det)
        rc, out = raw_match(t, case["C"], max_det, thrs, rngs)
        assert rc == 0
        assert_equal(cases.as_numpy(out), want, (len(thrs), len(rngs), max_det))
    rank, matched, ignored, gt_ignored, gt_of = lv.match(*t, case["C"], cases.IOU_THRS, cases.AREA_RNGS, 65, with_gt_of=False)
    want = reference(case, max_det=65)
    assert gt_of is None
    assert_equal(cases.as_numpy([rank, matched, ignored, gt_ignored, torch.from_numpy(want["gt_of"].copy())]), want, "without gt_of")


def test_where_the_federated_rules_are_silent_it_is_the_coco_kernel():
    """Every detected label in the positive or the negative set, nothing not exhaustive, no ignore flag, n_keep <= max_det:
    ``evaluation.match`` with no crowd, on the same tensors."""
    labels = (5, 31, 32, 33, 63, 64, 69)
    for seed, (B, K, G) in enumerate(((2, 65, 70), (3, 40, 12), (1, 300, 40))):
        case = cases.random_case("silent%d" % seed, B, K, G, det_labels=labels, neg=labels, nel=(), ignore=0.0, seed=20 + seed)
        t = cases.tensors(case, DEV)
        assert not t[7].any() and not t[10].any() and int(t[3].max()) <= case["max_det"] == K
        got = lv.match(*t, case["C"], cases.IOU_THRS, cases.AREA_RNGS, case["max_det"])
        coco = ev.match(*t[:7], torch.zeros_like(t[7]), t[8], cases.IOU_THRS, cases.AREA_RNGS, case["max_det"])
        assert_equal(cases.as_numpy(got), cases.as_numpy(coco), case["name"])
        assert bool((got[1] != 0).any()) and bool((got[0] >= 0).any())


def test_two_runs_into_poisoned_outputs_are_identical():
    for name in ("mixed", "image_cut"):
        case = cases.get(name)
        t = cases.tensors(case, DEV)
        rc0, a = raw_match(t, case["C"], case["max_det"], fill=0xFF)
        rc1, b = raw_match(t, case["C"], case["max_det"], fill=0x5A)
        assert rc0 == rc1 == 0
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name


def test_unserved_arguments_return_einval_and_launch_nothing():
    case = cases.get("ignored_gt")
    t = cases.tensors(case, DEV)
    thr65 = tuple(0.5 + 0.005 * i for i in range(65))
    for what, kw in (("K = 1025", dict(K=1025)), ("G = 1025", dict(G=1025)), ("C = 0", dict(C=0)), ("C = 65536", dict(C=65536)),
                     ("A T = 65", dict(thrs=thr65, rngs=cases.AREA_RNGS[:1])), ("max_det = 0", dict(max_det=0)),
                     ("max_det > K", dict(max_det=5)), ("B = 0", dict(B=0)), ("B = 65536", dict(B=65536)), ("neg = null", dict(neg=None))):
        max_det = kw.pop("max_det", 1)
        rc, out = raw_match(t, kw.pop("C", case["C"]), max_det, **kw)
        assert rc == EINVAL, what
        assert all(bool((o.view(torch.uint8) == 0xFF).all()) for o in out), what + ": something was launched"
    assert not lv.match_supported(*t, case["C"], thr65, cases.AREA_RNGS[:1], 1)
    assert not lv.match_supported(*t, case["C"], cases.IOU_THRS, cases.AREA_RNGS, 0)
    assert not lv.match_supported(*t[:9], t[9].long(), t[10], case["C"])
    with pytest.raises(RuntimeError, match="does not serve"):
        lv.match(*t, case["C"], cases.IOU_THRS, cases.AREA_RNGS, 0)


def test_capture_and_replay_after_the_counts_and_the_bitsets_change():
    """The one kernel captured on one stream; n_keep, n_gt and both bitsets are rewritten in place between the replays."""
    first = cases.random_case("replay0", 3, 65, 70, seed=30)
    static = cases.tensors(first, DEV)
    args = (first["C"], cases.IOU_THRS, cases.AREA_RNGS, first["max_det"])
    lv.match(*static, *args)                      # (library load and first launch outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lv.match(*static, *args)
    changes = ((first["n_keep"] // 2, [[5, 31], [], [69, 33, 32]], [[], [64, 5], [63]]),
               (np.array([65, 0, 33], np.int32), [[], [33], [20, 40]], [[32], [31, 63], []]))
    seen = []
    for variant, (n_keep, neg, nel) in enumerate(changes):
        case = dict(first, name="replay%d" % (variant + 1), n_keep=n_keep.astype(np.int32), neg=neg, nel=nel)
        fresh = cases.tensors(case, DEV)
        for i in (3, 9, 10):
            static[i].copy_(fresh[i])
        graph.replay()
        torch.cuda.synchronize()
        got = cases.as_numpy(out)
        assert_equal(got, reference(case), "replay %d" % variant)
        seen.append(got["rank"].copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], reference(first)["rank"])


def test_largest_served_shape_stays_inside_its_buffers():
    """K = G = 1024, C = 65535 with all 40 problems: the launch with the largest LDS request (the opt-in above 48 KB), the
    widest bitsets (2048 words) and the longest loops; labels in the last word among them."""
    labels = (5, 31, 32, 65534, 65504, 40000, 65535, -7)
    case = cases.random_case("largest", 1, 1024, 1024, C=65535, det_labels=labels, gt_labels=labels[:5], neg=(40000, 65534),
                             nel=(65504, 40000), seed=40, max_det=1024, full=True)
    assert _lib.load().zira_lvis_match_lds_bytes(1024, 1024, 10, 4, 65535) > 48 * 1024
    rc, out = raw_match(cases.tensors(case, DEV), case["C"], case["max_det"])
    assert rc == 0
    assert_equal(cases.as_numpy(out), reference(case), "K = G = 1024, C = 65535")


def test_evaluator_on_device_state_equals_the_cpu_state_evaluator(monkeypatch):
    names = ["c%d" % c for c in range(70)]
    host, dev = lv.LVISBoxEvaluator(names, FREQ70), lv.LVISBoxEvaluator(names, FREQ70)
    calls = []
    real = lv.match
    monkeypatch.setattr(lv, "match", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for name in EVAL_CASES + ("image_cut",):
        inputs, outputs = batch_of(cases.get(name))
        host.process(inputs, outputs)
        for o in outputs:
            i = o["instances"]
            i.scores, i.pred_classes, i.pred_boxes.tensor = i.scores.to(DEV), i.pred_classes.to(DEV), i.pred_boxes.tensor.to(DEV)
        dev.process(inputs, outputs)
    assert len(calls) == len(EVAL_CASES) + 1                                   # every batch on the kernel, the CPU ones on none
    assert all(v.is_cuda for b in dev._batches for v in b.values()) and not any(v.is_cuda for b in host._batches for v in b.values())
    assert ev.accumulate_supported(dev._batches, 70, dev.iou_thrs, dev.area_rngs, (300,))
    want, got = host.evaluate(), dev.evaluate()
    assert got == want and np.array_equal(dev.precision, host.precision) and np.array_equal(dev.recall, host.recall)
    assert 0 < got["bbox"]["AP"] < 100 and len(got["bbox"]) == 13
    monkeypatch.setattr(lv, "FORCE_REFERENCE", True)
    forced = lv.LVISBoxEvaluator(names, FREQ70)
    for b in dev._batches:
        forced._batches.append(b)
    assert forced.evaluate() == want                                           # the host accumulation of the device state
    none = lv.LVISBoxEvaluator(names, FREQ70)
    inputs, outputs = batch_of(cases.get("mixed"))
    from test_lvis_cpu import _Inst
    none.process(inputs, [{"instances": _Inst(torch.zeros(0, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV),
                                              torch.zeros(0, 4, device=DEV))} for _ in outputs])
    monkeypatch.setattr(lv, "FORCE_REFERENCE", False)
    assert none.evaluate() == {"bbox": {k: -1.0 for k in want["bbox"]}}


def test_inference_on_dataset_with_a_chunked_category_list(monkeypatch):
    """The slice model with its seven names forced into three chunks: the merged tail leaves the padded outputs the evaluator
    takes.  Category 5 is annotated, 0 is annotated and not exhaustive, 3 was checked and is absent; the rest were not checked."""
    from test_vocab_cpu import SEVEN, chunk_model

    model, front = chunk_model("cuda", monkeypatch)
    model.category_chunk_size = 3
    batch = front.batch([".".join(SEVEN) + "."] * 2)
    for n, x in enumerate(batch):
        x["annotations"] = [{"bbox": [4.0 + n, 6.0, 30.0, 20.0], "category_id": 5},
                            {"bbox": [20.0, 10.0 + n, 25.0, 40.0], "category_id": 0, "ignore": n}]
        x["neg_category_ids"], x["not_exhaustive_category_ids"] = [3], [0]
    freq = ["c", "c", "r", "f", "c", "r", "f"]                                  # frequent: 3 and 6, neither annotated
    evaluator = lv.LVISBoxEvaluator(SEVEN, freq)
    assert model._category_chunks([SEVEN, SEVEN]) == [SEVEN[0:3], SEVEN[3:6], SEVEN[6:7]]
    got = ev.inference_on_dataset(model, [batch, batch], evaluator)
    assert set(got) == {"bbox"} and list(got["bbox"])[:9] == list(lv.METRICS) and len(got["bbox"]) == 13
    assert all(-1.0 <= v <= 100.0 for v in got["bbox"].values()) and got["bbox"]["AP"] > -1 and got["bbox"]["APf"] == -1.0
    assert len(evaluator._batches) == 2 and all(v.is_cuda for b in evaluator._batches for v in b.values())
    state = evaluator._batches[0]
    took = state["rank"] >= 0
    assert bool(took.any()) and set(state["labels"][took].tolist()) <= {0, 3, 5} and not bool(took.all())
    monkeypatch.setattr(lv, "FORCE_REFERENCE", True)
    assert ev.inference_on_dataset(model, [batch, batch], lv.LVISBoxEvaluator(SEVEN, freq)) == got
