"""Inputs, hand-made matches and the float64 reference for the tests of the loss tail -- zira_match_cost_f32 (csrc/lsap.hip)
and zira_stacked_losses_{fwd,bwd}_f32 (csrc/criterion.hip) -- shared by the CPU test that proves them
(test_criterion_cases_cpu.py) and the GPU tests that call the C ABI on them (test_loss_tail_gpu.py).

The reference is the package's own op chain on CPU tensors in float64: criterion.sigmoid_focal_loss per prediction set (the
arithmetic of TwoStageCriterion._forward_stacked), F.l1_loss, box_ops.generalized_box_iou_aligned and
HungarianMatcher.cost_matrix; gradients are autograd's.  The float32 inputs are converted exactly.  The same functions in
float32 are the other arm of the GPU comparisons.

Layouts as in the C ABI: logits [S, B, Q, C], boxes [S, B, Q, 4] (cx, cy, w, h), q_idx / t_idx [S, M] int64 (t_idx indexes
the concatenated targets), image_of [M], labels_all [T], boxes_all [T, 4], num_boxes a float32 scalar, out / g_out [3, S] =
(class, L1, GIoU) per set."""
import functools
import types

import torch
import torch.nn.functional as F

from ziragroundingdino_amd import criterion
from ziragroundingdino_amd.box_ops import box_cxcywh_to_xyxy, generalized_box_iou_aligned
from ziragroundingdino_amd.matcher import HungarianMatcher

ROWS_PER_BLOCK = 4          # csrc/criterion.hip: a wave per (set, image, query) row, four rows per block
FILL = -100.0               # recover_to_cls_logits' fill for the categories an image does not have
SATURATED = (-88.0, -30.0, -17.0, -1e-3, 0.0, 17.0, 30.0, 88.0)

# (S, B, Q, C, targets per image, note): each the smallest shape that reaches what its note names
# (test_criterion_cases_cpu.py holds the notes to the cases).
SHAPES = [
    (2, 1, 5, 8, (3,), "two blocks | B Q = 5: the second block has one live wave; C < 64"),
    (3, 2, 7, 100, (4, 3), "second stride of 36 | C = 100; B Q = 14"),
    (1, 2, 70, 130, (64, 1), "second ballot round | M = 65: pairs at k = 63 and k = 64; C = 130: third stride of 2 lanes"),
    (2, 3, 50, 64, (20, 0, 44), "image without targets | M = 64 and C = 64 exactly"),
    (2, 1, 40, 32, (128,), "more targets than queries | M = 40 = Q: every row is matched"),
]
MODEL_SHAPE = (7, 2, 900, 256, (6, 4), "model size | the training step's own shape")

PARAMS = [(0.25, 2.0), (0.25, 1.5), (0.25, 1.0), (-1.0, 2.0), (-1.0, 1.5)]      # (alpha, gamma)
NUM_BOXES = (1.0, 3.5)      # 3.5: what an all-reduced average over ranks gives

# Box kinds: predictions (cx, cy, w, h) in units of 2^-6 against the target (32, 32, 16, 16) (corners 24 .. 40): every corner
# and every tie is exact in float32 and float64 alike.
DYADIC_TARGET = (32, 32, 16, 16)
KINDS = [
    ("identical", (32, 32, 16, 16)),
    ("contained and centred", (32, 32, 8, 8)),
    ("one x edge and both y edges shared", (28, 32, 8, 16)),
    ("disjoint in x", (48, 32, 8, 16)),
    ("touching: x0 == X1", (44, 34, 8, 12)),
    ("containing the target", (32, 32, 32, 32)),
    ("zero area at the centre", (32, 32, 0, 0)),
    ("zero area and disjoint", (52, 12, 0, 0)),
    ("general overlap", (36, 28, 16, 12)),
    ("same x extent, half the height", (32, 28, 16, 8)),
]
ORDINARY, FILLED, SATURATED_GROUP, FILLED_LABEL = 0, 1, 2, 3
LOGIT_GROUPS = {"ordinary": ORDINARY, "fill": FILLED, "saturated": SATURATED_GROUP, "label on a filled column": FILLED_LABEL}


def shape_id(shape):
    S, B, Q, C, sizes, note = shape
    return "S%d-B%d-Q%d-C%d-%s" % (S, B, Q, C, note.split(" | ")[0].replace(" ", "_"))


def scratch_bytes(S, B, Q, M):
    """zira_stacked_losses_scratch_bytes restated: a double per (set, block of four rows), two floats per (set, pair)."""
    if S <= 0 or B <= 0 or Q <= 0 or M < 0:
        return 0
    return S * (-(-B * Q // ROWS_PER_BLOCK)) * 8 + 2 * S * max(M, 1) * 4


def _dyadic(box):
    return torch.tensor(box, dtype=torch.float32) / 64.0


def kind_geometry(k):
    """(iw_raw, ih_raw, area of the prediction) of kind k against the dyadic target, in units of 2^-6 (and 2^-12)."""
    cx, cy, w, h = KINDS[k][1]
    X, Y, W, H = DYADIC_TARGET
    iw = min(cx + w / 2, X + W / 2) - max(cx - w / 2, X - W / 2)
    ih = min(cy + h / 2, Y + H / 2) - max(cy - h / 2, Y - H / 2)
    return iw, ih, w * h


def _random_pred_boxes(g, *lead):
    return torch.cat([torch.rand(*lead, 2, generator=g) * 0.6 + 0.2, torch.rand(*lead, 2, generator=g) * 0.3 + 0.05], -1)


def _random_target_boxes(g, n):
    return torch.cat([torch.rand(n, 2, generator=g) * 0.5 + 0.25, torch.rand(n, 2, generator=g) * 0.3 + 0.1], -1)


@functools.lru_cache(maxsize=None)
def make_case(shape, index=0):
    """The inputs of one shape.  ``index`` (the case's place in SHAPES) moves the saturated label column on.

    Matches: per set and image, min(Q, targets) distinct random queries in random order -- query 0 among those of image 0,
    query Q - 1 among those of the last image -- on distinct targets of the image in random order; the first ten targets (or
    M, if fewer), target 1 and the last target are matched in every set.
    Boxes: the first min(10, M) targets are the dyadic target; in the even sets the query matched to target j < 10 carries
    kind j, in the odd sets a random box.  Everything else is random as in test_criterion_gpu.py.
    Logits: randn * 2, FILL on the upper half of the columns.  Per set: the row matched to target 1 carries SATURATED with
    value number (set + index) mod 8 on its label column; one unmatched row (where every row is matched: the row matched to
    target 2) carries SATURATED on columns away from any label; the row matched to the last target has its label, C - 1, on
    a filled column."""
    S, B, Q, C, sizes, note = shape
    g = torch.Generator().manual_seed(((S * 131 + B) * 131 + Q) * 131 + C)
    per_image = [min(Q, n) for n in sizes]
    M, T = sum(per_image), sum(sizes)
    offs = [sum(sizes[:b]) for b in range(B)]
    last_image = max(b for b in range(B) if sizes[b] > 0)
    n_kinds = min(len(KINDS), M)
    must = sorted(set(range(n_kinds)) | {1, T - 1})
    image_of = torch.repeat_interleave(torch.arange(B), torch.tensor(per_image))

    def pick(n, m, required):
        """m distinct numbers below n in random order, ``required`` among them."""
        rest = [int(v) for v in torch.randperm(n, generator=g) if int(v) not in required][: m - len(required)]
        chosen = torch.tensor(list(required) + rest, dtype=torch.int64)
        return chosen[torch.randperm(m, generator=g)]

    q_idx, t_idx = torch.empty(S, M, dtype=torch.int64), torch.empty(S, M, dtype=torch.int64)
    for s in range(S):
        k = 0
        for b, m in enumerate(per_image):
            if m == 0:
                continue
            want_q = ([0] if b == 0 else []) + ([Q - 1] if b == last_image and not (b == 0 and Q == 1) else [])
            q_idx[s, k:k + m] = pick(Q, m, want_q)
            t_idx[s, k:k + m] = pick(sizes[b], m, [t - offs[b] for t in must if offs[b] <= t < offs[b] + sizes[b]]) + offs[b]
            k += m
    if M > 64:      # the second ballot round of find_pair: the pair at k = 64 is the last row of all, the one at k = 63 row 0
        assert per_image[0] == 64
        for s in range(S):
            at0 = int((q_idx[s, :64] == 0).nonzero()[0])
            q_idx[s, at0], q_idx[s, 63] = q_idx[s, 63].clone(), 0

    labels_all = torch.randint(0, C // 2, (T,), generator=g)
    labels_all[0], labels_all[T - 1] = 0, C - 1
    boxes_all = _random_target_boxes(g, T)
    boxes_all[:n_kinds] = _dyadic(DYADIC_TARGET)
    logits = torch.randn(S, B, Q, C, generator=g) * 2
    logits[..., C // 2:] = FILL
    group = torch.zeros(S, B, Q, C, dtype=torch.int8)
    group[..., C // 2:] = FILLED
    boxes = _random_pred_boxes(g, S, B, Q)
    kind = torch.full((S, M), -1, dtype=torch.int64)
    sat = torch.tensor(SATURATED)
    saturated_rows = []         # (s, b, q, label or -1, number of the value on the label column or -1)
    for s in range(S):
        pair_of = {int(t): k for k, t in enumerate(t_idx[s])}
        if s % 2 == 0:
            for j in range(n_kinds):
                k = pair_of[j]
                kind[s, k] = j
                boxes[s, image_of[k], q_idx[s, k]] = _dyadic(KINDS[j][1])
        # the matched saturated row
        k = pair_of[1]
        b, q, label, j = int(image_of[k]), int(q_idx[s, k]), int(labels_all[1]), (s + index) % 8
        cols = (label - j + torch.arange(8)) % C
        logits[s, b, q, cols], group[s, b, q, cols] = sat, SATURATED_GROUP
        saturated_rows.append((s, b, q, label, j))
        # the other one: unmatched where there is an unmatched row
        matched0 = set(int(v) for v in q_idx[s, :per_image[0]])
        free = [v for v in range(Q) if v not in matched0]
        if free:
            b, q, label = 0, free[len(free) // 2], -1
            cols = torch.arange(8)
        else:
            k = pair_of[2]
            b, q, label = int(image_of[k]), int(q_idx[s, k]), int(labels_all[2])
            cols = torch.arange(8) + (8 if label < 8 else 0)
        logits[s, b, q, cols], group[s, b, q, cols] = sat, SATURATED_GROUP
        saturated_rows.append((s, b, q, label, -1))
        # the label on a filled column
        k = pair_of[T - 1]
        group[s, image_of[k], q_idx[s, k], C - 1] = FILLED_LABEL
    g_out = (0.5 + torch.rand(3, S, generator=g)) * (torch.randint(0, 2, (3, S), generator=g).float() * 2 - 1)
    if S > 1:       # (a single set keeps its L1 weight: a zero there would switch the term off altogether)
        g_out[1, S - 1] = 0.0
    return types.SimpleNamespace(shape=shape, S=S, B=B, Q=Q, C=C, sizes=sizes, M=M, T=T, n_kinds=n_kinds, logits=logits, boxes=boxes,
                                 q_idx=q_idx, t_idx=t_idx, image_of=image_of, labels_all=labels_all, boxes_all=boxes_all, g_out=g_out,
                                 kind=kind, group=group, saturated_rows=saturated_rows)


def flat_index(case, device=None):
    """(set, image, query, target) of all S M pairs, set-major."""
    d = lambda t: t.to(device)
    s_i = torch.arange(case.S).repeat_interleave(case.M)
    return d(s_i), d(case.image_of.repeat(case.S)), d(case.q_idx.reshape(-1)), d(case.t_idx.reshape(-1))


def row_masks(case):
    """[S, B, Q] bool: rows of dyadic pairs, rows of the other pairs, unmatched rows."""
    s_i, b_i, q_i, _ = flat_index(case)
    dyadic = torch.zeros(case.S, case.B, case.Q, dtype=torch.bool)
    matched = torch.zeros_like(dyadic)
    matched[s_i, b_i, q_i] = True
    dyadic[s_i, b_i, q_i] = case.kind.reshape(-1) >= 0
    return dyadic, matched & ~dyadic, ~matched


def chain(case, alpha, gamma, num_boxes, dtype=torch.float64, device="cpu", g_out=None, want_logits=True, want_boxes=True):
    """The package's op chain on the case in ``dtype`` on ``device`` -> out [3, S], g_logits, g_boxes (autograd of
    sum(out * g_out); None where not wanted)."""
    to = lambda t: t.detach().to(device=device, dtype=dtype)
    S, Q, M = case.S, case.Q, case.M
    logits, boxes = to(case.logits).requires_grad_(want_logits), to(case.boxes).requires_grad_(want_boxes)
    boxes_all, labels_all = to(case.boxes_all), case.labels_all.to(device)
    nb = torch.tensor(num_boxes, dtype=torch.float32, device=device)
    s_i, b_i, q_i, t_i = flat_index(case, device)
    onehot = torch.zeros(case.logits.shape, dtype=dtype, device=device)
    onehot[s_i, b_i, q_i, labels_all[t_i]] = 1
    cls = torch.stack([criterion.sigmoid_focal_loss(logits[s], onehot[s], nb, alpha, gamma) * Q for s in range(S)])
    src, tgt = boxes[s_i, b_i, q_i], boxes_all[t_i]
    l1 = F.l1_loss(src, tgt, reduction="none").sum(-1)
    giou = 1 - generalized_box_iou_aligned(box_cxcywh_to_xyxy(src), box_cxcywh_to_xyxy(tgt))
    out = torch.stack([cls, l1.view(S, M).sum(1) / nb, giou.view(S, M).sum(1) / nb])
    leaves = [t for t, w in ((logits, want_logits), (boxes, want_boxes)) if w]
    grads = list(torch.autograd.grad((out * to(case.g_out if g_out is None else g_out)).sum(), leaves)) if leaves else []
    g_logits = grads.pop(0) if want_logits else None
    g_boxes = grads.pop(0) if want_boxes else None
    return out.detach(), g_logits, g_boxes


@functools.lru_cache(maxsize=None)
def reference_f64(shape, index, alpha, gamma, num_boxes):
    """chain() in float64 on the CPU, computed once per (case, parameters)."""
    return chain(make_case(shape, index), alpha, gamma, num_boxes)


def golden_case(g):
    """The sets of tests/golden/mod_criterion.pt (auxiliary layers, final layer, encoder output) with the golden's own
    assignments, in the layout of make_case."""
    out, idx = g["outputs"], g["indices"]
    sets = list(out["aux_outputs"]) + [out, out["enc_outputs"]]
    matches = list(idx["aux_outputs"]) + [idx["indices"]] + list(idx["enc_outputs"])
    sizes = tuple(len(t["labels"]) for t in g["targets"])
    offs = [sum(sizes[:b]) for b in range(len(sizes))]
    logits, boxes = torch.stack([o["pred_logits"] for o in sets]), torch.stack([o["pred_boxes"] for o in sets])
    S, B, Q, C = logits.shape
    q_idx = torch.stack([torch.cat([q for q, _ in m]) for m in matches])
    t_idx = torch.stack([torch.cat([t + offs[b] for b, (_, t) in enumerate(m)]) for m in matches])
    image_of = torch.repeat_interleave(torch.arange(B), torch.tensor([len(q) for q, _ in matches[0]]))
    return types.SimpleNamespace(S=S, B=B, Q=Q, C=C, sizes=sizes, M=q_idx.shape[1], T=sum(sizes), logits=logits.detach(), boxes=boxes.detach(),
                                 q_idx=q_idx, t_idx=t_idx, image_of=image_of, labels_all=torch.cat([t["labels"] for t in g["targets"]]),
                                 boxes_all=torch.cat([t["boxes"] for t in g["targets"]]), g_out=None, final_set=len(out["aux_outputs"]))


# ---- matching cost ------------------------------------------------------------------------------------------------------------

COST_SHAPES = [(5, 8, 1, "smallest"), (37, 100, 7, "N T = 259: a second block of 3 threads"), (300, 64, 64, "many targets"),
               (2700, 256, 23, "the step's size")]
COST_WEIGHTS = [(1.0, 1.0, 1.0), (2.0, 5.0, 2.0)]        # (class, bbox, giou)
COST_PARAMS = [(0.25, 2.0), (0.25, 1.5)]


@functools.lru_cache(maxsize=None)
def make_cost_case(shape):
    """Predictions 0 .. 9 (or N) are the ten kinds, target 0 the dyadic target, targets 1 .. 3 random boxes with corners on
    multiples of 2^-6; the rest is random.  Target ids hold 0, C - 1 and duplicates (T = 1: id 0).  Rows 10 .. 17 (N = 5:
    rows 0 .. 4) carry SATURATED on every gathered column."""
    N, C, T, note = shape
    g = torch.Generator().manual_seed((N * 131 + C) * 131 + T)
    ids = torch.randint(0, C, (T,), generator=g)
    ids[0] = 0
    if T > 1:
        ids[1] = C - 1
    if T > 3:
        ids[3] = ids[2]
    if T > 4:
        ids[T - 1] = 0
    logits = torch.randn(N, C, generator=g) * 3
    first = 10 if N >= 18 else 0
    sat_rows = torch.arange(first, min(first + 8, N))
    logits[sat_rows[:, None], ids[None, :]] = torch.tensor(SATURATED)[:len(sat_rows), None]
    boxes = _random_pred_boxes(g, N)
    n_kinds = min(len(KINDS), N)
    for j in range(n_kinds):
        boxes[j] = _dyadic(KINDS[j][1])
    tgt = _random_target_boxes(g, T)
    n_dyadic = min(4, T)
    for t in range(1, n_dyadic):
        x0, y0 = torch.randint(4, 30, (2,), generator=g)
        w, h = torch.randint(1, 16, (2,), generator=g) * 2
        tgt[t] = torch.stack([x0 + w / 2, y0 + h / 2, w, h]).float() / 64.0
    tgt[0] = _dyadic(DYADIC_TARGET)
    saturated = torch.zeros(N, T, dtype=torch.bool)
    saturated[sat_rows] = True
    return types.SimpleNamespace(shape=shape, N=N, C=C, T=T, logits=logits, boxes=boxes, ids=ids, tgt_boxes=tgt, n_kinds=n_kinds,
                                 n_dyadic=n_dyadic, saturated=saturated)


def cost_chain(case, weights, alpha, gamma, dtype=torch.float64, device="cpu"):
    """HungarianMatcher.cost_matrix on the case -> [N, T]."""
    to = lambda t: t.to(device=device, dtype=dtype)
    m = HungarianMatcher(cost_class=weights[0], cost_bbox=weights[1], cost_giou=weights[2], alpha=alpha, gamma=gamma)
    tgt = [{"labels": case.ids.to(device), "boxes": to(case.tgt_boxes)}]
    return m.cost_matrix({"pred_logits": to(case.logits)[None], "pred_boxes": to(case.boxes)[None]}, tgt)[0]


def group_err(a, ref64, mask=None):
    """Largest error of ``a`` relative to the float64 tensor's largest magnitude, both over ``mask``; None for an empty mask."""
    a, ref64 = a.detach().cpu().double(), ref64.detach().cpu()
    if mask is not None:
        a, ref64 = a[mask], ref64[mask]
    if ref64.numel() == 0:
        return None
    scale = float(ref64.abs().max())
    d = float((a - ref64).abs().max())
    return d / scale if scale > 0 else (0.0 if d == 0 else float("inf"))
