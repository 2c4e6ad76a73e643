"""A helper, not a test: the cases the Pascal VOC evaluation tests share (CPU: ``match_reference`` and ``PascalVOCBoxEvaluator``
against voc_oracle; GPU: ``match`` against ``match_reference``), as numpy arrays in ``voc_evaluation.match``'s layout.
The oracle's answer for a case is computed once per process (``expected``) and never modified."""
import functools

import numpy as np

import voc_oracle as oracle

IOU_THRS = oracle.IOU_THRS
INPUTS = ("scores", "labels", "xyxy", "n_keep", "gt_xyxy", "gt_label", "gt_difficult", "n_gt")
OUTPUTS = ("qscore", "tp", "fp", "gt_of")


def pad(dets, gts, K=None, G=None):
    """dets: per image a list of (score, label, x0, y0, x1, y1) in the MODEL's 0-based corners (VOC's box (1, 1, 10, 10) is
    (0, 0, 10, 10) here);  gts: per image a list of (label, x0, y0, x1, y1, difficult), VOC's corners.  -> the eight inputs."""
    B = len(dets)
    K = K or max(1, max(len(d) for d in dets))
    G = max(len(g) for g in gts) if G is None else G
    a = {"scores": np.zeros((B, K), np.float32), "labels": np.zeros((B, K), np.int64), "xyxy": np.zeros((B, K, 4), np.float32),
         "n_keep": np.array([len(d) for d in dets], np.int32), "gt_xyxy": np.zeros((B, G, 4)),
         "gt_label": np.zeros((B, G), np.int64), "gt_difficult": np.zeros((B, G), np.uint8),
         "n_gt": np.array([len(g) for g in gts], np.int32)}
    for b in range(B):
        for k, d in enumerate(dets[b]):
            a["scores"][b, k], a["labels"][b, k], a["xyxy"][b, k] = d[0], d[1], d[2:6]
        for g, t in enumerate(gts[b]):
            a["gt_label"][b, g], a["gt_xyxy"][b, g], a["gt_difficult"][b, g] = t[0], t[1:5], t[5]
    return a


def _case(name, arrays, n_classes=None):
    n_classes = n_classes or int(max(arrays["labels"].max(initial=0), arrays["gt_label"].max(initial=0))) + 1
    return dict(arrays, name=name, n_classes=n_classes)


def hand_cases():
    c = {}
    # VOC (1, 1, 10, 10) against (1, 1, 10, 5): 50 / (100 + 50 - 50) = 0.5 exactly
    c["on_threshold"] = _case("on_threshold", pad([[(0.9, 0, 0, 0, 10, 10)]], [[(0, 1, 1, 10, 5, 0)]]))
    c["twin_gts"] = _case("twin_gts", pad([[(0.9, 0, 0, 0, 10, 10)]], [[(0, 1, 1, 10, 10, 0), (0, 1, 1, 10, 10, 0)]]))
    # the weaker detection comes first in the row; the stronger one takes the GT, the weaker one is the duplicate
    c["duplicate"] = _case("duplicate", pad([[(0.6, 0, 0, 0, 10, 10), (0.8, 0, 0, 0, 10, 9)]], [[(0, 1, 1, 10, 10, 0)]]))
    # a difficult GT under two detections, a plain one beside it
    c["difficult"] = _case("difficult", pad([[(0.9, 0, 0, 0, 10, 10), (0.8, 0, 0, 0, 10, 8), (0.7, 0, 50, 50, 60, 60)]],
                                            [[(0, 1, 1, 10, 10, 1), (0, 51, 51, 60, 60, 0)]]))
    c["label_without_gt"] = _case("label_without_gt", pad([[(0.9, 1, 0, 0, 10, 10), (0.8, 0, 0, 0, 10, 10)]], [[(0, 1, 1, 10, 10, 0)]]),
                                  n_classes=2)
    c["image_without_detections"] = _case("image_without_detections", pad(
        [[], [(0.9, 0, 0, 0, 10, 10)]], [[(0, 1, 1, 10, 10, 0)], [(0, 1, 1, 10, 10, 0)]]))
    a = pad([[(0.9, 0, 0, 0, 10, 10)], [(0.8, 0, 0, 0, 10, 10)]], [[(0, 1, 1, 10, 10, 0)], [(0, 1, 1, 10, 10, 0)]])
    a["n_keep"][:] = 0
    c["n_keep_zero"] = _case("n_keep_zero", a)
    c["no_gt_at_all"] = _case("no_gt_at_all", pad([[(0.9, 0, 0, 0, 10, 10), (0.8, 1, 0, 0, 40, 40)]], [[]]), n_classes=2)
    # 0.5004 and 0.4996 are one score in the file (0.500): the row order decides, and row 0 (the lower raw score) is first
    c["equal_quantised_scores"] = _case("equal_quantised_scores", pad(
        [[(0.4996, 0, 0, 0, 10, 10), (0.5004, 0, 0, 0, 10, 10), (0.5, 0, 0, 0, 10, 10)]], [[(0, 1, 1, 10, 10, 0)]]))
    # ties of the text round trip: 0.0625 -> 62.5 -> 0.062, 0.1875 -> 187.5 -> 0.188 (nearest even); m / 4 with odd m: 10.25 ->
    # 10.2, 10.75 -> 10.8, 2.25 (1.25 + 1) -> 2.2, 1.75 (0.75 + 1) -> 1.8
    c["quantisation_ties"] = _case("quantisation_ties", pad(
        [[(0.0625, 0, 1.25, 0.75, 10.25, 10.75), (0.1875, 0, 1.75, 1.25, 9.75, 9.25)]], [[(0, 2, 2, 10, 10, 0)]]))
    # x0 + 1 is an fp32 add: 8388607.5 + 1 = 8388608.5 is not an fp32 number and rounds (to even) to 8388608, so the box is 10
    # wide and covers 100 / 190 of the GT; an fp64 add would leave 9.5 x 10 = 95 / 190 = 0.5 exactly, a miss at 0.5
    c["fp32_plus_one"] = _case("fp32_plus_one", pad([[(0.9, 0, 8388607.5, 0, 8388617, 10)]], [[(0, 8388608, 1, 8388617, 19, 0)]]))
    a = pad([[(0.9, 0, 0, 0, 10, 10), (0.8, 0, 20, 20, 30, 30)], [(0.7, 0, 0, 0, 10, 10), (0.6, 0, 0, 0, 10, 10)]],
            [[(0, 1, 1, 10, 10, 0), (0, 21, 21, 30, 30, 0)], [(0, 1, 1, 10, 10, 0), (0, 1, 1, 10, 10, 0)]])
    a["n_keep"][:] = (7, -3)            # clamped to 2 and 0
    a["n_gt"][:] = (1, 11)              # image 0 loses its second GT, image 1 keeps both
    c["counts_out_of_range"] = _case("counts_out_of_range", a)
    c["label_out_of_range"] = _case("label_out_of_range", pad(
        [[(0.9, 2, 0, 0, 10, 10), (0.8, -1, 0, 0, 10, 10), (0.7, 1, 0, 0, 10, 10)]], [[(2, 1, 1, 10, 10, 0), (1, 1, 1, 10, 10, 0)]]),
        n_classes=2)
    return c


# (B, K, G, labels, seed)
RANDOM_SHAPES = ((1, 1, 0, 1, 1), (3, 7, 1, 2, 2), (2, 65, 70, 3, 3), (2, 300, 20, 20, 4))
LARGEST = (1, 1024, 1024, 3, 5)          # against match_reference only: the oracle's Python loops take too long here


def random_case(B, K, G, n_labels, seed, variant=0, distinct=False):
    """Integer GT corners in 1..100; detections half near a GT of the image (its corners moved on a 1/4 grid: odd quarters are
    ties of the "%.1f" round trip) and half anywhere; scores on a 1/4096 grid, so that quantised scores tie and the row order
    decides (``distinct``: three-decimal scores that differ within each label over the whole batch, as the reference's unstable
    argsort needs them); ragged counts; 25 % difficult; labels interleaved."""
    rng = np.random.default_rng(1000 * seed + variant)
    n_keep = rng.integers((K + 1) // 2, K + 1, B).astype(np.int32)
    n_gt = rng.integers((G + 1) // 2, G + 1, B).astype(np.int32)
    if B > 1:
        n_keep[(seed + variant) % B] = K
        if B > 2:
            n_keep[(seed + variant + 1) % B] = 0
    gxy = rng.integers(1, 60, (B, G, 2))
    gwh = rng.integers(3, 40, (B, G, 2))
    gt_xyxy = np.concatenate([gxy, gxy + gwh], -1).astype(np.float64)
    gt_label = rng.integers(0, n_labels, (B, G)).astype(np.int64)
    gt_difficult = (rng.random((B, G)) < 0.25).astype(np.uint8)
    if G >= n_labels:                       # every label has a GT that counts: image 0 opens with one of each
        n_gt[0], gt_label[0, :n_labels], gt_difficult[0, :n_labels] = G, np.arange(n_labels), 0
    elif G:
        gt_label[0, 0], gt_difficult[0, 0], n_gt[0] = 0, 0, G
    xy = rng.integers(0, 240, (B, K, 2)) / 4.0
    wh = rng.integers(8, 160, (B, K, 2)) / 4.0
    xyxy = np.concatenate([xy, xy + wh], -1)
    labels = rng.integers(0, n_labels, (B, K)).astype(np.int64)
    if G:
        near = rng.random((B, K)) < 0.6
        pick = rng.integers(0, G, (B, K))
        moved = np.take_along_axis(gt_xyxy, pick[:, :, None].repeat(4, 2), 1) - np.array([1.0, 1.0, 0.0, 0.0])
        moved = moved + rng.integers(-6, 7, (B, K, 4)) / 4.0
        moved[..., 2:] = np.maximum(moved[..., 2:], moved[..., :2] + 1.0)
        xyxy = np.where(near[:, :, None], moved, xyxy)
        labels = np.where(near, np.take_along_axis(gt_label, pick, 1), labels)
    if distinct:
        scores = np.zeros((B, K), np.float32)
        for c in range(n_labels):
            at = np.argwhere(labels == c)
            assert len(at) <= 970
            vals = rng.permutation(np.arange(20, 990))[:len(at)] / 1000.0 + rng.integers(-1, 2, len(at)) / 4096.0
            scores[at[:, 0], at[:, 1]] = vals
    else:
        scores = (rng.integers(0, 4097, (B, K)) / 4096.0).astype(np.float32)
    a = {"scores": scores.astype(np.float32), "labels": labels, "xyxy": xyxy.astype(np.float32), "n_keep": n_keep,
         "gt_xyxy": gt_xyxy, "gt_label": gt_label, "gt_difficult": gt_difficult, "n_gt": n_gt}
    return _case("random_B%d_K%d_G%d_L%d_v%d%s" % (B, K, G, n_labels, variant, "_distinct" if distinct else ""), a, n_labels)


def random_cases():
    out = {}
    for shape in RANDOM_SHAPES:
        for distinct in (False, True):
            case = random_case(*shape, distinct=distinct)
            out[case["name"]] = case
    return out


@functools.lru_cache(maxsize=None)
def _all():
    cases = hand_cases()
    cases.update(random_cases())
    return cases


def names():
    return list(_all())


def get(name):
    return _all()[name]


@functools.lru_cache(maxsize=None)
def largest():
    return random_case(*LARGEST)


def images(case):
    return oracle.images_from_padded(*(case[k] for k in INPUTS))


_EXPECTED = {}


def expected(case, thrs=IOU_THRS):
    """The oracle's four output arrays for a case (computed once; callers must not write into them)."""
    key = (case["name"], tuple(thrs))
    if key not in _EXPECTED:
        out = oracle.match_outputs(images(case), case["scores"].shape[1], case["n_classes"], thrs)
        for a in out:
            a.setflags(write=False)
        _EXPECTED[key] = dict(zip(OUTPUTS, out))
    return _EXPECTED[key]


def tensors(case, device="cpu"):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(case[k])).to(device) for k in INPUTS]


def as_numpy(outputs):
    """``match``'s four tensors -> numpy arrays, the two bit fields as uint32."""
    arrs = [t.detach().cpu().numpy() for t in outputs]
    arrs[1], arrs[2] = arrs[1].view(np.uint32), arrs[2].view(np.uint32)
    return dict(zip(OUTPUTS, arrs))
