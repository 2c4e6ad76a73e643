"""``zira_voc_match`` on the GPU against ``voc_evaluation.match_reference`` (which test_voc_evaluation.py holds to the reference's
``voc_eval`` and to voc_oracle on the same cases): every output element compared for equality, nothing masked out; the entry's
contract (fill behind the counts, clamped counts, limits, graph capture); and the evaluator on a stream of batches."""
import ctypes

import numpy as np
import pytest
import torch

import voc_cases as cases

pytestmark = pytest.mark.gpu

from ziragroundingdino_amd import _lib  # noqa: E402
from ziragroundingdino_amd import voc_evaluation as voc  # noqa: E402

DEV = "cuda"
EINVAL = 1
ONE_THR = (0.7,)


def raw_match(t, num_classes, thrs=cases.IOU_THRS, B=None, K=None, G=None, fill=0xFF):
    """The C entry on buffers pre-filled with ``fill`` (so an element the kernel leaves alone shows).  -> (rc, outputs)."""
    lib = _lib.load()
    scores, labels, xyxy, n_keep, gt_xyxy, gt_label, gt_difficult, n_gt = t
    b, k = scores.shape
    g = gt_label.shape[1]
    T = len(thrs)
    byte = lambda shape, dt: torch.full((int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size(),), fill, dtype=torch.uint8,
                                        device=DEV).view(dt).view(shape)
    out = [byte((b, k), torch.float64), byte((b, k), torch.int32), byte((b, k), torch.int32), byte((b, k, min(T, 16)), torch.int32)]
    ptr = lambda x: x.data_ptr() if x.numel() else None
    rc = lib.zira_voc_match(scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(), n_keep.data_ptr(), b if B is None else B,
                            k if K is None else K, ptr(gt_xyxy), ptr(gt_label), ptr(gt_difficult), ptr(n_gt),
                            g if G is None else G, (ctypes.c_double * T)(*thrs), T, num_classes, out[0].data_ptr(),
                            out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


_WANT = {}


def want_of(case, thrs=cases.IOU_THRS):
    """``match_reference``'s answer on the host, computed once per (case, thresholds) and left unchanged."""
    key = (case["name"], tuple(thrs))
    if key not in _WANT:
        _WANT[key] = cases.as_numpy(voc.match_reference(*cases.tensors(case), case["n_classes"], thrs))
        for a in _WANT[key].values():
            a.setflags(write=False)
    return _WANT[key]


def assert_equal(got, want, what):
    for k in cases.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        same = got[k].view(np.uint64) == want[k].view(np.uint64) if k == "qscore" else got[k] == want[k]     # qscore: bit for bit
        assert same.all(), "%s: %s differs at %s" % (what, k, np.argwhere(~same)[:5].tolist())


@pytest.mark.parametrize("thrs", [cases.IOU_THRS, ONE_THR], ids=["T10", "T1"])
@pytest.mark.parametrize("name", cases.names())
def test_match_equals_reference_everywhere(name, thrs):
    """Hand-built and random cases, through the raw entry on 0xFF-filled buffers (the documented fill behind n_keep is part of
    the expected arrays) and through the wrapper."""
    case = cases.get(name)
    t = cases.tensors(case, DEV)
    want = want_of(case, thrs)
    rc, out = raw_match(t, case["n_classes"], thrs)
    assert rc == 0
    assert_equal(cases.as_numpy(out), want, name + " (raw entry)")
    assert_equal(cases.as_numpy(voc.match(*t, case["n_classes"], thrs)), want, name + " (wrapper)")


def test_cases_equal_the_oracle_too():
    """The kernel against the loop-for-loop oracle directly, on the case with more GTs and detections than a wave."""
    case = cases.get("random_B2_K65_G70_L3_v0")
    assert_equal(cases.as_numpy(voc.match(*cases.tensors(case, DEV), case["n_classes"])), cases.expected(case), "oracle")


def test_largest_served_shape_stays_inside_its_buffers():
    """K = G = 1024 with 3 labels: the launch with the largest LDS request (the opt-in above 48 KB) and the longest loops."""
    case = cases.largest()
    assert case["scores"].shape == (1, 1024) and case["gt_label"].shape == (1, 1024) and case["n_classes"] == 3
    rc, out = raw_match(cases.tensors(case, DEV), 3)
    assert rc == 0
    assert_equal(cases.as_numpy(out), want_of(case), "K = G = 1024")


def test_fill_behind_the_counts_and_optional_gt_of():
    case = cases.get("random_B3_K7_G1_L2_v0")
    assert (case["n_keep"] == 0).any() and (case["n_keep"] == 7).any()
    t = cases.tensors(case, DEV)
    got = cases.as_numpy(raw_match(t, 2)[1])
    for b in range(3):
        nk = int(case["n_keep"][b])
        assert (got["qscore"][b, nk:] == 0).all() and (got["tp"][b, nk:] == 0).all() and (got["fp"][b, nk:] == 0).all()
        assert (got["gt_of"][b, nk:] == -1).all()
    qscore, tp, fp, gt_of = voc.match(*t, 2, with_gt_of=False)
    assert gt_of is None
    want = want_of(case)
    assert_equal(cases.as_numpy([qscore, tp, fp, torch.from_numpy(want["gt_of"].copy())]), want, "without gt_of")


def test_unserved_limits_return_einval():
    case = cases.get("twin_gts")
    t = cases.tensors(case, DEV)
    thr17 = tuple(0.5 + 0.02 * i for i in range(17))
    for what, kw in (("K = 1025", dict(K=1025)), ("K = 0", dict(K=0)), ("G = 1025", dict(G=1025)), ("G = -1", dict(G=-1)),
                     ("T = 17", dict(thrs=thr17)), ("B = 0", dict(B=0)), ("B = 65536", dict(B=65536)), ("no classes", dict())):
        rc, out = raw_match(t, 0 if what == "no classes" else 1, **kw)
        assert rc == EINVAL, what
        assert all(bool((o.view(torch.uint8) == 0xFF).all()) for o in out), what + ": something was launched"
    lib = _lib.load()
    assert lib.zira_voc_match(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 1, 1, None, None, None, None, 2,
                              (ctypes.c_double * 1)(0.5), 1, 1, t[0].data_ptr(), t[0].data_ptr(), t[0].data_ptr(), None,
                              None) == EINVAL                      # G > 0 without ground truth
    assert not voc.match_supported(*t, 1, thr17) and not voc.match_supported(*t, 0)
    assert not voc.match_supported(*t[:4], t[4].float(), *t[5:], 1)
    with pytest.raises(RuntimeError, match="does not serve"):
        voc.match(*t, 1, thr17)
    with pytest.raises(RuntimeError, match="does not serve"):
        voc.match(*cases.tensors(case, "cpu"), 1)


def test_capture_and_replay_equals_eager():
    """The one kernel captured on one stream; the replay on new inputs of the same shape equals the eager call on them."""
    shape = cases.RANDOM_SHAPES[2]
    first = cases.random_case(*shape, variant=0)
    static = cases.tensors(first, DEV)
    voc.match(*static, first["n_classes"])           # (library load and first launch outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = voc.match(*static, first["n_classes"])
    fresh = cases.random_case(*shape, variant=1)
    assert not np.array_equal(fresh["xyxy"], first["xyxy"])
    for dst, src in zip(static, cases.tensors(fresh, DEV)):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    eager = cases.as_numpy(voc.match(*cases.tensors(fresh, DEV), fresh["n_classes"]))
    assert_equal(cases.as_numpy(out), eager, "replay against eager")
    assert_equal(eager, want_of(fresh), "eager against the reference")


def test_evaluator_on_a_stream_of_batches_equals_the_reference_path(monkeypatch):
    names = ["c0", "c1", "c2"]
    stream = [cases.random_case(*cases.RANDOM_SHAPES[2], variant=v) for v in (0, 1, 2)]

    def run(**kw):
        e = voc.PascalVOCBoxEvaluator(names, base_classes=names[:2], novel_classes=names[2:], **kw)
        for case in stream:
            e.process_padded(*cases.tensors(case, DEV))
        assert len(e._batches) == 3 and all(v.is_cuda for b in e._batches for v in b.values())
        return e.evaluate(), e.per_class_ap50

    calls = []
    kernel = voc.match
    monkeypatch.setattr(voc, "match", lambda *a, **k: calls.append(1) or kernel(*a, **k))
    native = {year: run(year=year) for year in (2007, 2012)}
    assert len(calls) == 6                                     # the kernel served every batch
    monkeypatch.setattr(voc, "FORCE_REFERENCE", True)
    for year in (2007, 2012):
        assert run(year=year) == native[year]
    assert len(calls) == 6
    assert set(native[2007][0]["bbox"]) == {"AP", "AP50", "AP75", "bAP", "bAP50", "bAP75", "nAP", "nAP50", "nAP75"}
    assert 0.0 < native[2007][0]["bbox"]["AP50"] <= 100.0
