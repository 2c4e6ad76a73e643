"""``zira_ap_accumulate`` on the GPU against ``evaluation.accumulate`` (the host's numpy fp64; the small matched cases against
cocoeval_oracle.accumulate as well): every element of both tables compared for equality, the -1 cells included, no tolerance
anywhere.  States: the matching cases of evaluation_cases.py run through ``match``, the synthetic states of
ap_accumulate_cases.py (test_ap_accumulate_cpu.py shows on the reference's tables what each of them contains), the raw entry on
0xFF-filled tables, and the evaluator end to end."""
import ctypes

import numpy as np
import pytest
import torch

import ap_accumulate_cases as acc
import cocoeval_oracle as oracle
import evaluation_cases as cases

pytestmark = pytest.mark.gpu

from ziragroundingdino_amd import _lib  # noqa: E402
from ziragroundingdino_amd import evaluation as ev  # noqa: E402

DEV = "cuda"
EINVAL = 1
MAX_DETS = (1, 10, 100)


def assert_tables(got, want, what):
    for name, g, w in zip(("precision", "recall"), got, want):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == w.dtype == np.float64 and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), "%s: %s differs at %s" % (what, name, np.argwhere(g != w)[:5].tolist())


def host_state(state):
    return [{k: v.cpu().numpy() for k, v in b.items()} for b in state]


@pytest.mark.parametrize("name", cases.names())
def test_matched_cases_equal_the_host_and_the_oracle(name):
    """match -> accumulate_device with the default 10 thresholds x 4 areas x (1, 10, 100)."""
    case = cases.get(name)
    C = case["n_classes"]
    e = ev.CocoBoxEvaluator(["c%d" % i for i in range(C)])
    e.process_padded(*cases.tensors(case, DEV))
    args = (C, cases.IOU_THRS, cases.AREA_RNGS, MAX_DETS)
    assert ev.accumulate_supported(e._batches, *args)
    got = ev.accumulate_device(e._batches, *args)
    assert got[0].is_cuda and got[1].is_cuda
    assert_tables(got, acc.host_accumulate(host_state(e._batches), C, 10, 4, MAX_DETS, ev.DEFAULT_REC_THRS), name + " (host)")
    if case["scores"].shape[1] <= 65:
        assert_tables(got, oracle.accumulate(oracle.evaluate(cases.images(case), C)), name + " (oracle)")


@pytest.mark.parametrize("name", list(acc.CASES))
def test_synthetic_states_equal_the_host(name):
    """Segment lengths 0 / 1 / 63 / 64 / 65 / 129 / 4097 beside two other classes, 20 000 detections in one class, T A = 1,
    T A = 64, M = 1, three recall thresholds with both ends, labels outside [0, C)."""
    p = acc.params(name)
    state = acc.tensors(acc.state(name), DEV)
    args = (p["C"], [0.5] * p["T"], [(0.0, 1.0)] * p["A"], p["max_dets"], p["rec_thrs"])
    assert ev.accumulate_supported(state, *args)
    assert_tables(ev.accumulate_device(state, *args), acc.expected(name), name)


def raw(state, C, T, A, max_dets, rec_thrs, fill=0xFF, entry=None):
    """The C entry on tables pre-filled with ``fill``; ``entry`` replaces single arguments of the call.  -> (rc, precision, recall)."""
    rank, matched, ignored, seg_off, npig = ev._ordered(state, C, A)
    M, R = len(max_dets), len(rec_thrs)
    table = lambda *shape: torch.full((int(np.prod(shape)) * 8,), fill, dtype=torch.uint8, device=DEV).view(torch.float64).view(shape)
    shape = (min(T, 16), min(R, 256), min(C, 3), min(A, 4), min(M, 8))
    precision, recall = table(*shape), table(shape[0], *shape[2:])
    a = dict(rank=rank.data_ptr(), matched=matched.data_ptr(), ignored=ignored.data_ptr(), n=rank.numel(), seg_off=seg_off.data_ptr(),
             npig=npig.data_ptr(), C=C, T=T, A=A, M=M, R=R, precision=precision.data_ptr(), recall=recall.data_ptr())
    a.update(entry or {})
    rc = _lib.load().zira_ap_accumulate(a["rank"], a["matched"], a["ignored"], a["n"], a["seg_off"], a["npig"], a["C"], a["T"], a["A"],
                                        (ctypes.c_int32 * M)(*max_dets), a["M"], (ctypes.c_double * R)(*rec_thrs), a["R"],
                                        a["precision"], a["recall"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, precision, recall


def test_raw_entry_writes_every_element():
    name = "segment_65"
    p = acc.params(name)
    state = acc.tensors(acc.state(name), DEV)
    rc, precision, recall = raw(state, p["C"], p["T"], p["A"], p["max_dets"], p["rec_thrs"])
    assert rc == 0
    assert not torch.isnan(precision).any() and not torch.isnan(recall).any()        # 0xFF bytes are a NaN
    assert_tables((precision, recall), acc.expected(name), name + " (raw entry)")


def test_unserved_limits_return_einval_and_launch_nothing():
    name = "segment_65"
    p = acc.params(name)
    state = acc.tensors(acc.state(name), DEV)
    base = dict(C=p["C"], T=p["T"], A=p["A"], max_dets=p["max_dets"], rec_thrs=p["rec_thrs"])
    rec257 = tuple(i / 256 for i in range(257))
    for what, over, kw in (("T = 17", dict(T=17, A=1), {}), ("A = 5", dict(T=1, A=5), {}), ("T A = 65", dict(T=13, A=5), {}),
                           ("M = 9", dict(max_dets=tuple(range(1, 10))), {}), ("R = 257", dict(rec_thrs=rec257), {}),
                           ("max_det = 0", dict(max_dets=(0, 10, 100)), {}), ("rec_thrs descending", dict(rec_thrs=(1.0, 0.5, 0.0)), {}),
                           ("C = 0", {}, dict(C=0)), ("C = 65536", {}, dict(C=65536)), ("T = 0", {}, dict(T=0)), ("A = 0", {}, dict(A=0)),
                           ("M = 0", {}, dict(M=0)), ("R = 0", {}, dict(R=0)), ("n = -1", {}, dict(n=-1)), ("n = 2^31", {}, dict(n=2 ** 31)),
                           ("rank null", {}, dict(rank=None)), ("matched null", {}, dict(matched=None)),
                           ("ignored null", {}, dict(ignored=None)), ("seg_off null", {}, dict(seg_off=None)),
                           ("npig null", {}, dict(npig=None)), ("precision null", {}, dict(precision=None)),
                           ("recall null", {}, dict(recall=None))):
        rc, precision, recall = raw(state, **dict(base, **over), entry=kw)
        assert rc == EINVAL, what
        assert bool((precision.view(torch.uint8) == 0xFF).all()) and bool((recall.view(torch.uint8) == 0xFF).all()), what
    args = (p["C"], [0.5] * p["T"], [(0.0, 1.0)] * p["A"])
    assert not ev.accumulate_supported(state, *args, tuple(range(1, 10)), p["rec_thrs"])
    assert not ev.accumulate_supported(state, *args, p["max_dets"], rec257)
    assert not ev.accumulate_supported(state, *args, p["max_dets"], (1.0, 0.5, 0.0))
    assert not ev.accumulate_supported(state, *args, (0, 10, 100), p["rec_thrs"])
    assert not ev.accumulate_supported(state[:1] + acc.tensors(acc.state(name))[1:], *args, p["max_dets"], p["rec_thrs"])   # two devices
    with pytest.raises(RuntimeError, match="does not serve"):
        ev.accumulate_device(state, *args, p["max_dets"], rec257)


def test_evaluator_end_to_end(monkeypatch):
    """Two random batches of different K through ``process_padded``: the device accumulate and ``FORCE_REFERENCE`` give the same
    dictionary and the same tables, the device path is the one that ran, and ``accumulate_device`` never makes the host wait."""
    shapes = [s for s in cases.RANDOM_SHAPES if s[:3] in ((3, 65, 65), (2, 128, 130))]
    batches = [cases.tensors(cases.random_case(*s), DEV) for s in shapes]
    assert len(batches) == 2 and batches[0][0].shape[1] != batches[1][0].shape[1]
    names = ["c0", "c1", "c2"]

    def run():
        e = ev.CocoBoxEvaluator(names)
        for t in batches:
            e.process_padded(*t)
        return e, e.evaluate()

    calls = []
    real = ev.accumulate_device
    monkeypatch.setattr(ev, "accumulate_device", lambda *a, **k: calls.append(1) or real(*a, **k))
    native, got = run()
    assert calls == [1]
    monkeypatch.setattr(ev, "FORCE_REFERENCE", True)
    reference, want = run()
    assert calls == [1] and got == want
    assert isinstance(native.precision, np.ndarray) and isinstance(native.recall, np.ndarray)
    assert native.precision.dtype == reference.precision.dtype and native.recall.dtype == reference.recall.dtype
    assert native.precision.shape == reference.precision.shape == (10, 101, 3, 4, 3)
    assert native.recall.shape == reference.recall.shape == (10, 3, 4, 3)
    assert_tables((native.precision, native.recall), (reference.precision, reference.recall), "evaluator")
    assert ((native.precision > 0) & (native.precision < 1)).any()

    args = (3, native.iou_thrs, native.area_rngs, native.max_dets)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tables = real(native._batches, *args)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert_tables(tables, (reference.precision, reference.recall), "under sync debug mode")
