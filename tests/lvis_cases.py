"""A helper, not a test: the cases the LVIS evaluation tests share (CPU: ``match_reference`` and ``LVISBoxEvaluator`` against
lvis_oracle; GPU: ``match`` against ``match_reference``), as numpy arrays in ``lvis_evaluation.match``'s layout plus the per-image
id lists of the negative and the not-exhaustive set.  Boxes lie on an integer grid and scores come from eight values, so equal
IoUs and equal scores occur.  The oracle's answer for a case is computed once per process (``expected``) and never modified."""
import functools

import numpy as np

import lvis_oracle as oracle

IOU_THRS = tuple(oracle.IOU_THRS.tolist())
AREA_RNGS = tuple((float(lo), float(hi)) for lo, hi in oracle.AREA_RNGS)
INPUTS = ("scores", "labels", "xyxy", "n_keep", "gt_xywh", "gt_area", "gt_label", "gt_ignore", "n_gt")
OUTPUTS = ("rank", "matched", "ignored", "gt_ignored", "gt_of")
SCORES = np.array([0.95, 0.9, 0.8, 0.7, 0.5, 0.3, 0.2, 0.05], np.float32)

# C = 70: three bitset words, categories on both sides of bits 31 | 32 and 63 | 64.
C70 = 70
GT_LABELS = (5, 31, 32, 63, 64)                 # an image's positive set is drawn from these
#   5: in the positive set only;  33: in the negative set only;  40: in the not-exhaustive set only (filtered);  64: positive and
#   not exhaustive;  32: positive and negative;  69: negative and not exhaustive;  20: in none;  70, -1, 1000: outside 0..C-1
DET_LABELS = (5, 31, 32, 33, 40, 63, 64, 69, 20, 70, -1, 1000)
NEG, NEL = (33, 32, 69), (40, 64, 69)


def _case(name, arrays, neg, nel, C, max_det=300):
    K = arrays["scores"].shape[1]
    return dict(arrays, name=name, neg=[list(x) for x in neg], nel=[list(x) for x in nel], C=C, max_det=min(max_det, K))


def random_case(name, B, K, G, C=C70, det_labels=DET_LABELS, gt_labels=GT_LABELS, neg=NEG, nel=NEL, scale=8, seed=0, max_det=300,
                ignore=0.2, full=False):
    """Integer grid: corners 0..24, sides 1..12, times ``scale`` (8 reaches the medium class and the 96 x 96 edge of the large
    one); every fourth detection is a GT's box moved by a grid step, so matches and ties are common; ragged counts unless
    ``full``; ``ignore``: the share of GTs that carry the flag."""
    rng = np.random.default_rng(7000 + seed)

    def boxes(n):
        xy = rng.integers(0, 25, (B, n, 2))
        wh = rng.integers(1, 13, (B, n, 2))
        return (xy * scale).astype(np.float64), (wh * scale).astype(np.float64)

    n_keep = np.full(B, K, np.int32) if full else rng.integers((K + 1) // 2, K + 1, B).astype(np.int32)
    n_gt = np.full(B, G, np.int32) if full else rng.integers((G + 1) // 2, G + 1, B).astype(np.int32)
    dxy, dwh = boxes(K)
    gxy, gwh = boxes(G)
    labels = np.asarray(det_labels, np.int64)[rng.integers(0, len(det_labels), (B, K))]
    glab = np.asarray(gt_labels, np.int64)[rng.integers(0, len(gt_labels), (B, G))]
    if G:
        for b in range(B):
            for k in range(0, K, 4):
                g = int(rng.integers(0, G))
                dxy[b, k], dwh[b, k], labels[b, k] = gxy[b, g] + scale * rng.integers(-1, 2, 2), gwh[b, g], glab[b, g]
    a = {"scores": -np.sort(-SCORES[rng.integers(0, len(SCORES), (B, K))], axis=1), "labels": labels,
         "xyxy": np.concatenate([dxy, dxy + dwh], -1).astype(np.float32), "n_keep": n_keep,
         "gt_xywh": np.concatenate([gxy, gwh], -1), "gt_area": gwh[..., 0] * gwh[..., 1], "gt_label": glab,
         "gt_ignore": (rng.random((B, G)) < ignore).astype(np.uint8), "n_gt": n_gt}
    return _case(name, a, [neg] * B, [nel] * B, C, max_det)


def pad(dets, gts, K=None, G=None):
    """dets: per image a list of (score, label, x0, y0, x1, y1), in score order;  gts: per image a list of
    (label, x, y, w, h, ignore).  -> the nine input arrays (padding zero)."""
    B = len(dets)
    K = K or max(1, max(len(d) for d in dets))
    G = max(len(g) for g in gts) if G is None else G
    a = {"scores": np.zeros((B, K), np.float32), "labels": np.zeros((B, K), np.int64), "xyxy": np.zeros((B, K, 4), np.float32),
         "n_keep": np.array([len(d) for d in dets], np.int32), "gt_xywh": np.zeros((B, G, 4)), "gt_area": np.zeros((B, G)),
         "gt_label": np.zeros((B, G), np.int64), "gt_ignore": np.zeros((B, G), np.uint8),
         "n_gt": np.array([len(g) for g in gts], np.int32)}
    for b in range(B):
        for k, d in enumerate(dets[b]):
            a["scores"][b, k], a["labels"][b, k], a["xyxy"][b, k] = d[0], d[1], d[2:6]
        for g, t in enumerate(gts[b]):
            a["gt_label"][b, g], a["gt_xywh"][b, g], a["gt_ignore"][b, g], a["gt_area"][b, g] = t[0], t[1:5], t[5], t[3] * t[4]
    return a


@functools.lru_cache(maxsize=None)
def _all():
    cases = {}
    cases["mixed"] = random_case("mixed", 3, 40, 12, seed=1)
    # image 0: no GT and an empty negative set -- every detection is filtered; image 1 beside it is an ordinary one
    empty = random_case("empty_image", 2, 24, 6, seed=2)
    empty["n_gt"][0] = 0
    empty["neg"][0], empty["nel"][0] = [], [64]
    cases["empty_image"] = empty
    # G = 0: the GT pointers are null; what the negative set lets through is unmatched, and ignored where not exhaustive
    cases["no_gt_arrays"] = random_case("no_gt_arrays", 2, 16, 0, seed=3)
    # a flagged GT and a plain one of one label under three detections: the best IoU is the flagged GT's, the plain one is held
    # first; the second detection takes the flagged GT and is ignored; the third finds nothing and is a false positive
    cases["ignored_gt"] = _case("ignored_gt", pad(
        [[(0.9, 5, 0, 0, 10, 10), (0.8, 5, 0, 0, 10, 10), (0.7, 5, 0, 0, 10, 10), (0.6, 64, 50, 50, 60, 60)]],
        [[(5, 0, 0, 10, 10, 1), (5, 0, 0, 10, 12, 0), (64, 50, 50, 10, 10, 1)]]), [[]], [[]], C70)
    # a small detection (30 x 30) on a medium GT (34 x 34, IoU 900 / 1156): matched, so its own area does not ignore it where the
    # GT counts, and the GT's flag does where it does not; a second small detection apart from everything: unmatched, ignored
    # in medium and large by its area
    cases["area_ignore"] = _case("area_ignore", pad(
        [[(0.9, 5, 0, 0, 30, 30), (0.8, 5, 200, 200, 230, 230)]], [[(5, 0, 0, 34, 34, 0)]]), [[]], [[]], C70)
    # K = 1024, 700 valid rows, ONE score on both sides of row 300: the cut is by row order alone
    cut = random_case("image_cut", 1, 1024, 30, det_labels=(5, 31, 32, 33, 64, 20), seed=4, full=True)
    cut["n_keep"][0] = 700
    cut["scores"][0, 250:350] = cut["scores"][0, 250]
    assert (np.diff(cut["scores"][0]) <= 0).all()
    cases["image_cut"] = cut
    cases["image_cut_max_det_K"] = dict(cut, name="image_cut_max_det_K", max_det=1024)
    # counts outside their ranges: read as 0 and as K / G
    clamp = random_case("clamping", 3, 20, 6, seed=5)
    clamp["n_keep"][:] = (-3, 25, 20)
    clamp["n_gt"][:] = (10, -1, 6)
    cases["clamping"] = clamp
    # more than one wave's worth of GTs (G > 64) and K off the word size
    cases["wide"] = random_case("wide", 2, 65, 70, seed=6)
    return cases


def names():
    return list(_all())


def get(name):
    return _all()[name]


def images(case):
    return oracle.images_from_padded(*(case[k] for k in INPUTS), case["neg"], case["nel"])


_EXPECTED = {}


def expected(case):
    """The oracle's five output arrays for a case (computed once; callers must not write into them)."""
    key = case["name"]
    if key not in _EXPECTED:
        K, G = case["scores"].shape[1], case["gt_label"].shape[1]
        out = oracle.match_outputs(images(case), K, G, case["C"], IOU_THRS, AREA_RNGS, case["max_det"])
        for a in out:
            a.setflags(write=False)
        _EXPECTED[key] = dict(zip(OUTPUTS, out))
    return _EXPECTED[key]


def tensors(case, device="cpu"):
    """The eleven tensors ``match`` takes, the bitsets packed by ``category_bitsets``."""
    import torch

    from ziragroundingdino_amd import lvis_evaluation as lv

    t = [torch.from_numpy(np.ascontiguousarray(case[k])).to(device) for k in INPUTS]
    return t + [lv.category_bitsets(case["neg"], case["C"], device), lv.category_bitsets(case["nel"], case["C"], device)]


def as_numpy(outputs):
    """``match``'s five tensors -> numpy arrays, the two bit fields as uint64."""
    arrs = [t.detach().cpu().numpy() for t in outputs]
    arrs[1], arrs[2] = arrs[1].view(np.uint64), arrs[2].view(np.uint64)
    return dict(zip(OUTPUTS, arrs))
