"""``zira_ap_match`` on the GPU against cocoeval_oracle (the loop-for-loop COCOeval of the CPU tests, same cases, same expected
arrays): every output element compared for equality, nothing masked out; the entry's contract (fill behind the counts, limits,
graph capture); and the evaluator end to end behind the model's detections."""
import ctypes

import numpy as np
import pytest
import torch

import cocoeval_oracle as oracle
import evaluation_cases as cases

pytestmark = pytest.mark.gpu

from ziragroundingdino_amd import _lib  # noqa: E402
from ziragroundingdino_amd import evaluation as ev  # noqa: E402

DEV = "cuda"
EINVAL = 1


def raw_match(t, max_det, thrs=cases.IOU_THRS, rngs=cases.AREA_RNGS, B=None, K=None, G=None, fill=0xFF):
    """The C entry on buffers pre-filled with ``fill`` (so an element the kernel leaves alone shows).  -> (rc, outputs)."""
    lib = _lib.load()
    scores, labels, xyxy, n_keep, gt_xywh, gt_area, gt_label, gt_crowd, n_gt = t
    b, k = scores.shape
    g = gt_label.shape[1]
    T, A = len(thrs), len(rngs)
    byte = lambda shape, dt: torch.full((int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size(),), fill, dtype=torch.uint8,
                                        device=DEV).view(dt).view(shape)
    out = [byte((b, k), torch.int32), byte((b, k), torch.int64), byte((b, k), torch.int64), byte((b, g), torch.uint8),
           byte((b, k, min(A * T, 64)), torch.int32)]
    ptr = lambda x: x.data_ptr() if x.numel() else None
    rc = lib.zira_ap_match(scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(), n_keep.data_ptr(), b if B is None else B,
                           k if K is None else K, ptr(gt_xywh), ptr(gt_area), ptr(gt_label), ptr(gt_crowd), ptr(n_gt),
                           g if G is None else G, (ctypes.c_double * T)(*thrs), T,
                           (ctypes.c_double * (2 * A))(*[v for r in rngs for v in r]), A, max_det,
                           out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ptr(out[3]), out[4].data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def assert_equal(got, want, what):
    for k in cases.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %s" % (what, k, np.argwhere(got[k] != want[k])[:5].tolist())


@pytest.mark.parametrize("name", cases.names())
def test_match_equals_oracle_everywhere(name):
    """Hand-worked and random cases, through the raw entry on 0xFF-filled buffers (the documented fill behind n_keep / n_gt is
    part of the oracle's arrays: -1 / 0) and through the wrapper."""
    case = cases.get(name)
    t = cases.tensors(case, DEV)
    want = cases.expected(case)
    rc, out = raw_match(t, case["max_det"])
    assert rc == 0
    assert_equal(cases.as_numpy(out), want, name + " (raw entry)")
    assert_equal(cases.as_numpy(ev.match(*t, cases.IOU_THRS, cases.AREA_RNGS, case["max_det"])), want, name + " (wrapper)")


def test_fill_behind_the_counts():
    case = cases.get("random_B3_K65_G65_L2_v0")
    assert (case["n_keep"] == 0).any() and (case["n_gt"] == 0).any() and (case["n_keep"] == 65).any()
    rc, out = raw_match(cases.tensors(case, DEV), case["max_det"])
    got = cases.as_numpy(out)
    assert rc == 0
    for b in range(3):
        nk, ng = int(case["n_keep"][b]), int(case["n_gt"][b])
        assert (got["rank"][b, nk:] == -1).all() and (got["rank"][b, :nk] >= 0).all()
        assert (got["matched"][b, nk:] == 0).all() and (got["ignored"][b, nk:] == 0).all() and (got["gt_of"][b, nk:] == -1).all()
        assert (got["gt_ignored"][b, ng:] == 0).all()


def test_optional_gt_of_and_max_det_cut_flags():
    case = cases.get("random_B2_K128_G130_L3_v0")
    t = cases.tensors(case, DEV)
    want = cases.expected(case)
    rank, matched, ignored, gt_ignored, gt_of = ev.match(*t, cases.IOU_THRS, cases.AREA_RNGS, case["max_det"], with_gt_of=False)
    assert gt_of is None
    got = cases.as_numpy([rank, matched, ignored, gt_ignored, torch.from_numpy(want["gt_of"].copy())])
    assert_equal(got, want, "without gt_of")
    cut = got["rank"] >= case["max_det"]
    assert cut.any() and (got["matched"][cut] == 0).all() and (got["ignored"][cut] == 0).all()


def test_unserved_limits_return_einval():
    case = cases.get("twins")
    t = cases.tensors(case, DEV)
    before = raw_match(t, 1)[1]
    thr65 = tuple(0.5 + 0.005 * i for i in range(65))
    for what, kw in (("K = 1025", dict(K=1025)), ("G = 1025", dict(G=1025)), ("A T = 65", dict(thrs=thr65, rngs=cases.AREA_RNGS[:1])),
                     ("A T = 5 x 13", dict(thrs=thr65[:13], rngs=cases.AREA_RNGS + cases.AREA_RNGS[:1])),
                     ("max_det = 0", dict()), ("max_det > K", dict()), ("B = 0", dict(B=0)), ("B = 65536", dict(B=65536))):
        max_det = {"max_det = 0": 0, "max_det > K": 2}.get(what, 1)
        rc, out = raw_match(t, max_det, **kw)
        assert rc == EINVAL, what
        assert all(bool((o.view(torch.uint8) == 0xFF).all()) for o in out), what + ": something was launched"
    assert before[0].tolist() == [[0]]
    assert not ev.match_supported(*t, thr65, cases.AREA_RNGS[:1], 1) and not ev.match_supported(*t, cases.IOU_THRS, cases.AREA_RNGS, 0)
    with pytest.raises(RuntimeError, match="does not serve"):
        ev.match(*t, cases.IOU_THRS, cases.AREA_RNGS, 0)
    with pytest.raises(RuntimeError, match="does not serve"):
        ev.match(*cases.tensors(case, "cpu"), cases.IOU_THRS, cases.AREA_RNGS, 1)


def test_capture_and_replay_on_fresh_inputs():
    """The one kernel captured on one stream, replayed twice on new inputs of the same shape."""
    shape = next(s for s in cases.RANDOM_SHAPES if s[:3] == (3, 65, 65))
    first = cases.random_case(*shape, variant=0)
    static = cases.tensors(first, DEV)
    args = (cases.IOU_THRS, cases.AREA_RNGS, first["max_det"])
    ev.match(*static, *args)                      # (library load and first launch outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ev.match(*static, *args)
    for variant in (1, 2):
        case = cases.random_case(*shape, variant=variant)
        for dst, src in zip(static, cases.tensors(case, DEV)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        K, G = case["scores"].shape[1], case["gt_label"].shape[1]
        want = dict(zip(cases.OUTPUTS, oracle.match_outputs(cases.images(case), K, G, cases.IOU_THRS, cases.AREA_RNGS, case["max_det"])))
        assert_equal(cases.as_numpy(out), want, "replay %d" % variant)
    assert not np.array_equal(cases.random_case(*shape, variant=1)["xyxy"], cases.random_case(*shape, variant=2)["xyxy"])


def test_largest_served_shape_stays_inside_its_buffers():
    """K = G = 1024 with all 40 problems: the launch with the largest LDS request (the opt-in above 48 KB) and the longest
    loops, against ``match_reference`` (the oracle's Python loops would take minutes here)."""
    case = cases.random_case(1, 1024, 1024, 6, 100, 8, 77)
    t = cases.tensors(case, DEV)
    rc, out = raw_match(t, case["max_det"])
    assert rc == 0
    want = cases.as_numpy(ev.match_reference(*cases.tensors(case), cases.IOU_THRS, cases.AREA_RNGS, case["max_det"]))
    assert_equal(cases.as_numpy(out), want, "K = G = 1024")


def test_evaluator_end_to_end_behind_the_model(monkeypatch):
    from test_model_gpu import small_model

    from ziragroundingdino_amd.train import synthetic_batch

    model = small_model().eval()
    batches = []
    for seed in (0, 1):
        batch = synthetic_batch(2, 224, 320, n_categories=4, boxes_per_image=3, seed=seed, device=DEV)
        for x in batch:
            boxes, classes = x["instances"].gt_boxes.tensor.cpu().double(), x["instances"].gt_classes.cpu()
            x["annotations"] = [{"bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])],
                                 "category_id": int(c), "iscrowd": int(i == 2)} for i, (b, c) in enumerate(zip(boxes, classes))]
        batches.append(batch)
    names = ["fish", "jellyfish", "penguin", "puffin"]
    native = ev.CocoBoxEvaluator(names)
    got = ev.inference_on_dataset(model, batches, native)
    assert not model.training and len(native._batches) == 2 and all(v.is_cuda for b in native._batches for v in b.values())
    keys = {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100"} | {"AP-" + n for n in names}
    assert set(got) == {"bbox"} and set(got["bbox"]) == keys
    assert all(-1.0 <= v <= 100.0 for v in got["bbox"].values())
    monkeypatch.setattr(ev, "FORCE_REFERENCE", True)
    assert ev.inference_on_dataset(model, batches, ev.CocoBoxEvaluator(names)) == got
