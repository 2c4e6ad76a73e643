"""A helper, not a test: the cases the evaluation tests share (CPU: ``match_reference`` and ``CocoBoxEvaluator`` against
cocoeval_oracle; GPU: ``match`` against the same oracle outputs), as numpy arrays in ``evaluation.match``'s layout.
The oracle's answer for a case is computed once per process (``expected``) and never modified."""
import functools

import numpy as np

import cocoeval_oracle as oracle

IOU_THRS = tuple(oracle.IOU_THRS.tolist())
AREA_RNGS = tuple((float(lo), float(hi)) for lo, hi in oracle.AREA_RNGS)
INPUTS = ("scores", "labels", "xyxy", "n_keep", "gt_xywh", "gt_area", "gt_label", "gt_crowd", "n_gt")
OUTPUTS = ("rank", "matched", "ignored", "gt_ignored", "gt_of")


def pad(dets, gts, K=None, G=None):
    """dets: per image a list of (score, label, x0, y0, x1, y1), in score order;  gts: per image a list of
    (label, x, y, w, h, crowd[, area]).  -> the nine input arrays (padding zero)."""
    B = len(dets)
    K = K or max(1, max(len(d) for d in dets))
    G = max(len(g) for g in gts) if G is None else G
    a = {"scores": np.zeros((B, K), np.float32), "labels": np.zeros((B, K), np.int64), "xyxy": np.zeros((B, K, 4), np.float32),
         "n_keep": np.array([len(d) for d in dets], np.int32), "gt_xywh": np.zeros((B, G, 4)), "gt_area": np.zeros((B, G)),
         "gt_label": np.zeros((B, G), np.int64), "gt_crowd": np.zeros((B, G), np.uint8),
         "n_gt": np.array([len(g) for g in gts], np.int32)}
    for b in range(B):
        for k, d in enumerate(dets[b]):
            a["scores"][b, k], a["labels"][b, k], a["xyxy"][b, k] = d[0], d[1], d[2:6]
        for g, t in enumerate(gts[b]):
            a["gt_label"][b, g], a["gt_xywh"][b, g], a["gt_crowd"][b, g] = t[0], t[1:5], t[5]
            a["gt_area"][b, g] = t[6] if len(t) > 6 else t[3] * t[4]
    return a


def _case(name, arrays, max_det=100, n_classes=None):
    n_classes = n_classes or int(max(arrays["labels"].max(initial=0), arrays["gt_label"].max(initial=0))) + 1
    return dict(arrays, name=name, max_det=min(max_det, arrays["scores"].shape[1]), n_classes=n_classes)


def hand_cases():
    cases = {}
    # every (image, class) pair holds one GT and its exact detection; small, medium and large are populated
    box = lambda x, y, s: (x, y, x + s, y + s)
    cases["perfect"] = _case("perfect", pad(
        [[(0.9, 0) + box(0, 0, 10), (0.8, 1) + box(20, 20, 50)], [(0.7, 0) + box(5, 5, 200), (0.6, 1) + box(300, 0, 12)]],
        [[(0, 0, 0, 10, 10, 0), (1, 20, 20, 50, 50, 0)], [(0, 5, 5, 200, 200, 0), (1, 300, 0, 12, 12, 0)]]))
    cases["fp_then_tp"] = _case("fp_then_tp", pad([[(0.9, 0, 100, 100, 110, 110), (0.8, 0, 0, 0, 10, 10)]], [[(0, 0, 0, 10, 10, 0)]]))
    # class 0: one crowd under three detections; class 1: one plain GT with its detection
    cases["crowd"] = _case("crowd", pad(
        [[(0.9, 0, 0, 0, 10, 10), (0.8, 0, 10, 10, 20, 20), (0.7, 1, 50, 50, 60, 60), (0.6, 0, 5, 5, 25, 25)]],
        [[(0, 0, 0, 40, 40, 1), (1, 50, 50, 10, 10, 0)]]))
    cases["twins"] = _case("twins", pad([[(0.9, 0, 0, 0, 10, 10)]], [[(0, 0, 0, 10, 10, 0), (0, 0, 0, 10, 10, 0)]]))
    cases["on_threshold"] = _case("on_threshold", pad([[(0.9, 0, 0, 0, 2, 1)]], [[(0, 0, 0, 1, 1, 0)]]))
    cases["area_edges"] = _case("area_edges", pad([[(0.9, 0, 0, 0, 32, 32)]], [[(0, 0, 0, 32, 32, 0), (0, 100, 100, 96, 96, 0)]]))
    # 101 detections of one label: the first hundred lie apart from the GT, the 101st is the GT's box
    far = [(1.0 - 0.001 * i, 0, 500 + i, 500, 510 + i, 510) for i in range(100)]
    cases["max_det_cut"] = _case("max_det_cut", pad([far + [(0.5, 0, 0, 0, 10, 10)]], [[(0, 0, 0, 10, 10, 0)]]))
    cases["empty_row"] = _case("empty_row", pad([[], [(0.9, 0, 0, 0, 10, 10)]], [[(0, 0, 0, 10, 10, 0)], [(0, 0, 0, 10, 10, 0)]]),
                               n_classes=1)
    cases["no_gt"] = _case("no_gt", pad([[(0.9, 0, 0, 0, 10, 10), (0.8, 1, 0, 0, 40, 40)]], [[]]), n_classes=2)
    return cases


# (B, K, G, labels, max_det, grid scale, seed, what the shape is able to contain and must therefore contain):  a tie needs two GTs
# of one label in an image, a crowd re-match a crowd and two detections, a cut more than max_det detections of one label.
# The seeds are fixed; they were chosen by the ORACLE's verdict on the inputs (cocoeval_oracle.probe), never by the code under test.
RANDOM_SHAPES = (
    (1, 1, 1, 1, 100, 1, 11, ()),
    (2, 64, 1, 2, 100, 8, 62, ("crowd_rematch",)),
    (3, 65, 65, 2, 100, 1, 63, ("tie", "crowd_rematch")),
    (2, 128, 130, 3, 5, 8, 104, ("tie", "crowd_rematch", "cut")),
    (2, 128, 64, 40, 100, 1, 15, ()),        # 40 labels: most (image, label) pairs are empty on one side
    (4, 300, 0, 2, 5, 8, 16, ("cut",)),
)
SCORES = np.array([0.95, 0.9, 0.8, 0.7, 0.5, 0.3, 0.2, 0.05], np.float32)


def random_case(B, K, G, n_labels, max_det, scale, seed, expects=(), variant=0):
    """Integer grid: corners 0..24, sides 1..12, times ``scale`` (1 or 8: every value stays an exact integer, and 8 reaches the
    medium class and the 96 x 96 edge of the large one); scores from 8 values; ragged counts, zero among them; 20 % crowds."""
    rng = np.random.default_rng(1000 * seed + variant)

    def boxes(n):
        xy = rng.integers(0, 25, (B, n, 2))
        wh = rng.integers(1, 13, (B, n, 2))
        return (xy * scale).astype(np.float64), (wh * scale).astype(np.float64)

    n_keep = rng.integers((K + 1) // 2, K + 1, B).astype(np.int32)
    n_gt = rng.integers((G + 1) // 2, G + 1, B).astype(np.int32)
    if B > 1:
        n_keep[(seed + variant) % B] = K      # a full row, and an empty one beside it
        n_keep[(seed + variant + 1) % B] = 0 if B > 2 else n_keep[(seed + variant + 1) % B]
        if B > 2:
            n_gt[(seed + variant + 2) % B] = 0
    scores = -np.sort(-SCORES[rng.integers(0, len(SCORES), (B, K))], axis=1)
    dxy, dwh = boxes(K)
    gxy, gwh = boxes(G)
    a = {"scores": scores, "labels": rng.integers(0, n_labels, (B, K)).astype(np.int64),
         "xyxy": np.concatenate([dxy, dxy + dwh], -1).astype(np.float32), "n_keep": n_keep,
         "gt_xywh": np.concatenate([gxy, gwh], -1), "gt_area": gwh[..., 0] * gwh[..., 1],
         "gt_label": rng.integers(0, n_labels, (B, G)).astype(np.int64),
         "gt_crowd": (rng.random((B, G)) < 0.2).astype(np.uint8), "n_gt": n_gt}
    if G == 1 and "crowd_rematch" in expects:
        a["gt_crowd"][:] = 1                    # the shape's only GT: a crowd, or the shape cannot hold a re-match
    case = _case("random_B%d_K%d_G%d_L%d_v%d" % (B, K, G, n_labels, variant), a, max_det, n_labels)
    case["expects"] = tuple(expects)
    return case


def random_cases():
    return {c["name"]: c for c in (random_case(*shape) for shape in RANDOM_SHAPES)}


@functools.lru_cache(maxsize=None)
def _all():
    cases = hand_cases()
    cases.update(random_cases())
    return cases


def names():
    return list(_all())


def get(name):
    return _all()[name]


def images(case):
    return oracle.images_from_padded(*(case[k] for k in INPUTS))


_EXPECTED = {}


def expected(case):
    """The oracle's five output arrays for a case (computed once; callers must not write into them)."""
    key = case["name"]
    if key not in _EXPECTED:
        K, G = case["scores"].shape[1], case["gt_label"].shape[1]
        out = oracle.match_outputs(images(case), K, G, IOU_THRS, AREA_RNGS, case["max_det"])
        for a in out:
            a.setflags(write=False)
        _EXPECTED[key] = dict(zip(OUTPUTS, out))
    return _EXPECTED[key]


def tensors(case, device="cpu"):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(case[k])).to(device) for k in INPUTS]


def as_numpy(outputs):
    """``match``'s five tensors -> numpy arrays, the two bit fields as uint64."""
    arrs = [t.detach().cpu().numpy() for t in outputs]
    arrs[1], arrs[2] = arrs[1].view(np.uint64), arrs[2].view(np.uint64)
    return dict(zip(OUTPUTS, arrs))
