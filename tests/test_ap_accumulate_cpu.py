"""``zira_ap_accumulate`` and ``evaluation.accumulate_device`` without a GPU: the entry's argument checks (host arithmetic, in
front of any device call), ``accumulate_supported`` declining CPU state, the evaluator's unchanged host path, and the states of
ap_accumulate_cases.py examined on the HOST reference's tables -- what test_ap_accumulate_gpu.py then holds the kernel to is
not vacuous."""
import ctypes

import numpy as np
import pytest
import torch

import ap_accumulate_cases as acc
import cocoeval_oracle as oracle
import evaluation_cases as cases

from ziragroundingdino_amd import _lib
from ziragroundingdino_amd import evaluation as ev

EINVAL = 1


def entry(**kw):
    """The C entry on host buffers that a served call would never get: every check has to answer before any of them is used."""
    a = dict(rank=True, matched=True, ignored=True, n=8, seg_off=True, npig=True, C=2, T=10, A=4, max_dets=(1, 10, 100),
             rec_thrs=ev.DEFAULT_REC_THRS, precision=True, recall=True)
    a.update(kw)
    buf = ctypes.create_string_buffer(64)
    ptr = lambda on: ctypes.addressof(buf) if on else None
    M, R = len(a["max_dets"] or ()), len(a["rec_thrs"] or ())
    M, R = a.get("M", M), a.get("R", R)
    md = (ctypes.c_int32 * max(1, len(a["max_dets"] or ())))(*(a["max_dets"] or ())) if a["max_dets"] is not None else None
    rt = (ctypes.c_double * max(1, len(a["rec_thrs"] or ())))(*(a["rec_thrs"] or ())) if a["rec_thrs"] is not None else None
    return _lib.load().zira_ap_accumulate(ptr(a["rank"]), ptr(a["matched"]), ptr(a["ignored"]), a["n"], ptr(a["seg_off"]),
                                          ptr(a["npig"]), a["C"], a["T"], a["A"], md, M, rt, R, ptr(a["precision"]),
                                          ptr(a["recall"]), None)


@pytest.mark.parametrize("what, kw", [
    ("rank null", dict(rank=False)), ("matched null", dict(matched=False)), ("ignored null", dict(ignored=False)),
    ("seg_off null", dict(seg_off=False)), ("npig null", dict(npig=False)), ("precision null", dict(precision=False)),
    ("recall null", dict(recall=False)), ("max_dets null", dict(max_dets=None, M=3)), ("rec_thrs null", dict(rec_thrs=None, R=101)),
    ("T A = 65", dict(T=13, A=5)), ("T A = 17 x 4", dict(T=17, A=4)), ("A = 5", dict(T=1, A=5)), ("T = 17", dict(T=17, A=1)),
    ("C = 0", dict(C=0)), ("C = 65536", dict(C=65536)), ("T = 0", dict(T=0)), ("A = 0", dict(A=0)),
    ("M = 0", dict(M=0)), ("M = 9", dict(max_dets=tuple(range(1, 10)))), ("R = 0", dict(R=0)),
    ("R = 257", dict(rec_thrs=tuple(i / 256 for i in range(257)))), ("max_det = 0", dict(max_dets=(0, 10))),
    ("rec_thrs descending", dict(rec_thrs=(0.5, 0.25))), ("rec_thrs NaN", dict(rec_thrs=(float("nan"),))),
    ("n < 0", dict(n=-1)), ("n = 2^31", dict(n=2 ** 31)),
])
def test_entry_returns_einval_without_a_device(what, kw):
    assert entry(**kw) == EINVAL, what


def test_limits_are_the_header_s():
    assert (_lib.AP_MAX_DETS, _lib.AP_MAX_RECS, _lib.AP_MAX_CLASSES) == (8, 256, 65535)
    assert "zira_ap_accumulate" in _lib.SYMBOLS


def test_accumulate_supported_declines_cpu_state():
    p = acc.params("segment_65")
    state = acc.tensors(acc.state("segment_65"))
    args = (p["C"], [0.5] * p["T"], [(0.0, 1.0)] * p["A"], p["max_dets"], p["rec_thrs"])
    assert not ev.accumulate_supported(state, *args)
    assert not ev.accumulate_supported([], *args)
    with pytest.raises(RuntimeError, match="does not serve"):
        ev.accumulate_device(state, *args)


@pytest.mark.parametrize("name", ["perfect", "crowd", "empty_row", "no_gt", "random_B3_K65_G65_L2_v0"])
def test_evaluator_on_cpu_tensors_takes_the_host_path_as_before(name, monkeypatch):
    """CPU state: ``accumulate_device`` is not reached and the tables are the oracle's COCOeval.accumulate, element for element."""
    def no(*a, **k):
        raise AssertionError("accumulate_device reached with CPU state")

    monkeypatch.setattr(ev, "accumulate_device", no)
    case = cases.get(name)
    names = ["c%d" % i for i in range(case["n_classes"])]
    e = ev.CocoBoxEvaluator(names)
    e.process_padded(*cases.tensors(case))
    got = e.evaluate()
    want_p, want_r = oracle.accumulate(oracle.evaluate(cases.images(case), case["n_classes"]))
    assert e.precision.dtype == np.float64 and e.precision.shape == (10, 101, case["n_classes"], 4, 3)
    assert np.array_equal(e.precision, want_p) and np.array_equal(e.recall, want_r)
    assert got == {"bbox": ev.summarize(want_p, want_r, names, cases.IOU_THRS, (1, 10, 100))}
    assert ev.CocoBoxEvaluator(names).evaluate() == {"bbox": {k: -1.0 for k in got["bbox"]}}     # no batches: as before


@pytest.mark.parametrize("name", list(acc.CASES))
def test_cases_contain_what_they_are_for(name):
    p = acc.params(name)
    C, T, A, max_dets = p["C"], p["T"], p["A"], p["max_dets"]
    batches = acc.state(name)
    precision, recall = acc.expected(name)
    assert precision.shape == (T, len(p["rec_thrs"]), C, A, len(max_dets)) and recall.shape == (T, C, A, len(max_dets))
    cat = lambda k: np.concatenate([b[k].reshape(-1) for b in batches])
    scores, labels, rank, ignored, gt_label = cat("scores"), cat("labels"), cat("rank"), cat("ignored"), cat("gt_label")
    assert batches[0]["scores"].shape[1] != batches[1]["scores"].shape[1]
    # the count the case is named for
    n_target = acc.CASES[name][0]
    assert np.count_nonzero((labels == 0) & (rank >= 0) & (rank < max(max_dets))) == n_target
    # a -1 cell, and -1 only in whole cells
    empty = recall == -1
    assert empty.any() and not empty.all()
    assert np.array_equal((precision == -1).all(1), empty) and np.array_equal((precision == -1).any(1), empty)
    # GTs but no participating detection: recall 0.0 and precision 0.0 at every threshold
    assert ((recall[:, 2] == 0.0) & (precision[:, :, 2] == 0.0).all(1)).any()
    assert not ((labels == 2) & (rank >= 0) & (rank < max(max_dets))).any() and (gt_label == 2).any()
    # precision strictly inside (0, 1)
    assert ((precision > 0) & (precision < 1)).any()
    # ties inside a class and across classes, among the detections that take part
    live = (rank >= 0) & (rank < max(max_dets))
    s0, s1 = scores[live & (labels == 0)], scores[live & (labels == 1)]
    assert len(np.unique(s1)) < len(s1) and (n_target < 2 or len(np.unique(s0)) < len(s0))
    assert n_target == 0 or np.intersect1d(s0, s1).size
    # set ignore bits, ranks at or above the smallest max_det, padding on both sides
    assert (ignored[live] != 0).any() and (rank[(rank >= 0)] >= min(max_dets)).any()
    assert (rank == -1).any() and (gt_label == -1).any()
    assert ((rank == -1) & (labels == 0) & (ignored != (1 << (A * T)) - 1)).any()       # padding that would count if it took part
    if p["outside_labels"]:
        assert ((labels < 0) & live).any() and ((labels >= C) & live).any() and (gt_label >= C).any() and (gt_label < -1).any()


def test_reference_tables_do_not_depend_on_the_batch_cut():
    """The generator's two batches against the same entries as one flat batch: the reference sees state order only."""
    name = "segment_129"
    p = acc.params(name)
    batches = acc.state(name)
    flat = [{k: np.concatenate([b[k].reshape(-1) for b in batches])[None, :] for k in batches[0]}]
    got = acc.host_accumulate(flat, p["C"], p["T"], p["A"], p["max_dets"], p["rec_thrs"])
    assert all(np.array_equal(g, w) for g, w in zip(got, acc.expected(name)))
