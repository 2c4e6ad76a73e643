"""A helper, not a test: synthetic evaluator states for ``zira_ap_accumulate`` (test_ap_accumulate_cpu.py checks on the host
reference's tables that no case is vacuous; test_ap_accumulate_gpu.py holds the kernel to the same tables), in the layout
``CocoBoxEvaluator`` keeps: a list of per-batch dicts, ``scores`` f32 / ``labels`` i64 / ``rank`` i32 / ``matched`` / ``ignored``
i64 (the bits of a u64, bit ``a T + t``) of shape [B, K] and ``gt_label`` i64 / ``gt_ignored`` u8 of shape [B, G].

A state is drawn directly, not through ``match``, so that the counts are what a case says they are.  Classes:
  0  the target: exactly ``n_target`` detections with 0 <= rank < max(max_dets), and a few behind the cut;
  1  a filler with 37 such detections; with more than one area range all its GTs are ignored for the LAST range (a -1 cell);
  2  GTs, but only detections behind the cut: recall 0.0 and precision 0.0 everywhere the class has a not-ignored GT;
  3+ nothing at all (-1 cells).
Scores come from 8 values (ties inside and across classes), a fifth of the ignore bits is set, and both batches carry padding
(rank -1 with arbitrary labels and bits, gt_label -1) that must take part in nothing.  The entries are shuffled before they are
cut into two batches of different K, so the order the kernel needs is not the order it is handed.
The host reference's tables for a case are computed once per process (``expected``) and never modified."""
import functools

import numpy as np

from ziragroundingdino_amd import evaluation as ev

SCORES = np.array([0.95, 0.9, 0.8, 0.7, 0.5, 0.3, 0.2, 0.05], np.float32)
DEFAULT = dict(C=3, T=10, A=4, max_dets=(1, 10, 100), rec_thrs=ev.DEFAULT_REC_THRS, outside_labels=False)
REC3 = (0.0, 0.5, 1.0)

# name -> (n_target, seed, overrides of DEFAULT).  Seeds fixed here; test_ap_accumulate_cpu.py asserts what each case holds.
CASES = {}
for _n in (0, 1, 63, 64, 65, 129, 4097):
    CASES["segment_%d" % _n] = (_n, 10 + _n % 7, {})
CASES["one_class_20000"] = (20000, 3, {})
CASES["TA_1"] = (130, 4, dict(C=4, T=1, A=1))
CASES["TA_64"] = (130, 5, dict(T=16, A=4))
CASES["M_1"] = (130, 6, dict(max_dets=(10,)))
CASES["rec_thrs_3"] = (130, 7, dict(rec_thrs=REC3))
CASES["labels_outside"] = (130, 8, dict(outside_labels=True))


def params(name):
    p = dict(DEFAULT)
    p.update(CASES[name][2])
    return p


def _draw(rng, n, label, ranks, bits):
    """n detections of one label: (score, label, rank, matched, ignored) columns."""
    hit = np.zeros(n, np.uint64)
    ign = np.zeros(n, np.uint64)
    for b in range(bits):
        hit |= (rng.random(n) < 0.5).astype(np.uint64) << np.uint64(b)
        ign |= (rng.random(n) < 0.2).astype(np.uint64) << np.uint64(b)
    return (SCORES[rng.integers(0, len(SCORES), n)], np.full(n, label, np.int64), ranks.astype(np.int32), hit, ign)


@functools.lru_cache(maxsize=None)
def state(name):
    """-> the list of two per-batch dicts of numpy arrays (matched / ignored as uint64)."""
    n_target, seed, _ = CASES[name]
    p = params(name)
    C, T, A, max_dets = p["C"], p["T"], p["A"], p["max_dets"]
    rng = np.random.default_rng(seed)
    lo, top = min(max_dets), max(max_dets)
    inside = lambda n: np.where(rng.random(n) < 0.3, rng.integers(0, lo, n), rng.integers(0, top, n))     # 0 <= rank < top
    behind = lambda n: rng.integers(top, top + 20, n)
    parts = [_draw(rng, n_target, 0, inside(n_target), A * T), _draw(rng, 9, 0, behind(9), A * T),
             _draw(rng, 37, 1, inside(37), A * T), _draw(rng, 5, 1, behind(5), A * T), _draw(rng, 11, 2, behind(11), A * T)]
    if p["outside_labels"]:
        for label in (-3, -1, C, C + 5):
            parts.append(_draw(rng, 13, label, inside(13), A * T))
    n_pad = 23
    parts.append(_draw(rng, n_pad, 0, np.full(n_pad, -1), A * T))          # padding that looks like the target class
    parts[-1][1][:] = rng.integers(-1, C + 1, n_pad)
    cols = [np.concatenate([q[i] for q in parts]) for i in range(5)]
    order = rng.permutation(len(cols[0]))
    cols = [c[order] for c in cols]
    # ground truth: (label, ignore bits); class 1's GTs are all ignored for the last range where there is more than one
    gts = [(0, int(b)) for b in rng.integers(0, 1 << A, 40)] + [(0, 0)]
    last = 1 << (A - 1)
    gts += [(1, (int(b) | last) if A > 1 else int(b)) for b in rng.integers(0, 1 << A, 15)] + [(1, last if A > 1 else 0)]
    gts += [(2, 0), (2, (1 << A) - 1), (2, 1 if A > 1 else 0)]
    if p["outside_labels"]:
        gts += [(C, 0), (C + 5, 0), (-2, 0)]
    gts += [(-1, int(b)) for b in rng.integers(0, 1 << A, 6)]                # padding
    gts = [gts[i] for i in rng.permutation(len(gts))]
    g_lab, g_ign = np.array([g[0] for g in gts], np.int64), np.array([g[1] for g in gts], np.uint8)

    n = len(cols[0])
    cut, g_cut = n // 3, len(gts) // 2
    batches = []
    for (a, b), (ga, gb), B in (((0, cut), (0, g_cut), 3), ((cut, n), (g_cut, len(gts)), 2)):
        K, G = -(-(b - a) // B) + 1, -(-(gb - ga) // B) + 1

        def grid(x, size, fill):
            out = np.full(B * size, fill, x.dtype)
            out[:len(x)] = x
            return out.reshape(B, size)

        batches.append({"scores": grid(cols[0][a:b], K, 0), "labels": grid(cols[1][a:b], K, 0), "rank": grid(cols[2][a:b], K, -1),
                        "matched": grid(cols[3][a:b], K, 0), "ignored": grid(cols[4][a:b], K, 0),
                        "gt_label": grid(g_lab[ga:gb], G, -1), "gt_ignored": grid(g_ign[ga:gb], G, 0)})
    for batch in batches:
        for v in batch.values():
            v.setflags(write=False)
    return batches


def host_accumulate(batches, C, T, A, max_dets, rec_thrs):
    """``evaluation.accumulate`` on a state of numpy arrays, filtered as ``CocoBoxEvaluator.evaluate`` filters its host copy."""
    cat = lambda k: np.concatenate([np.asarray(b[k]).reshape(-1) for b in batches])
    rank, gt_label = cat("rank"), cat("gt_label")
    det, gt = rank >= 0, gt_label >= 0
    return ev.accumulate(cat("scores")[det].astype(np.float64), cat("labels")[det], rank[det],
                         cat("matched").view(np.uint64)[det], cat("ignored").view(np.uint64)[det], gt_label[gt],
                         cat("gt_ignored")[gt], C, [0.0] * T, [(0.0, 0.0)] * A, max_dets, rec_thrs)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(precision, recall) of the host reference for a case (computed once; read-only)."""
    p = params(name)
    out = host_accumulate(state(name), p["C"], p["T"], p["A"], p["max_dets"], p["rec_thrs"])
    for a in out:
        a.setflags(write=False)
    return out


def tensors(batches, device="cpu"):
    """The state as torch tensors in the evaluator's dtypes (the two bit fields as int64)."""
    import torch

    out = []
    for b in batches:
        d = {}
        for k, v in b.items():
            v = np.ascontiguousarray(v)
            d[k] = torch.from_numpy((v.view(np.int64) if v.dtype == np.uint64 else v).copy()).to(device)
        out.append(d)
    return out
