"""The inputs, the hand-made matches and the float64 reference of the loss tail's GPU tests (tests/criterion_cases.py), proven
where there is no GPU: the reference rounds to the float32 chain and reproduces the reference project's golden losses and
gradients, the matches are valid, every shape puts its pairs, rows and columns where its note says, the box kinds are the
kinks they are named after, and the float32 chain has its exact zeros where the float64 reference has them."""
import os

import pytest
import torch

import criterion_cases as cc

CASES = list(enumerate(cc.SHAPES)) + [(len(cc.SHAPES), cc.MODEL_SHAPE)]
IDS = [cc.shape_id(s) for _, s in CASES]
SMALL, SMALL_IDS = CASES[:-1], IDS[:-1]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mod_criterion.pt")


def _case(i, shape):
    return cc.make_case(shape, i)


@pytest.mark.parametrize("i,shape", CASES, ids=IDS)
def test_matches_are_valid_and_cover_the_corner_rows(i, shape):
    case = _case(i, shape)
    S, B, Q, C, sizes, _ = shape
    per_image = [min(Q, n) for n in sizes]
    assert case.M == sum(per_image) and case.T == sum(sizes)
    assert case.image_of.tolist() == [b for b, m in enumerate(per_image) for _ in range(m)]
    offs = [sum(sizes[:b]) for b in range(B)]
    last = max(b for b in range(B) if sizes[b])
    for s in range(S):
        rows = [(int(b), int(q)) for b, q in zip(case.image_of, case.q_idx[s])]
        assert len(set(rows)) == case.M                                  # every (set, image, query) at most once
        assert all(0 <= q < Q for _, q in rows)
        assert (0, 0) in rows and (last, Q - 1) in rows
        assert len(set(case.t_idx[s].tolist())) == case.M                # and every target at most once per set
        for k in range(case.M):
            b = int(case.image_of[k])
            assert offs[b] <= int(case.t_idx[s, k]) < offs[b] + sizes[b]
    assert int(case.labels_all.min()) == 0 and int(case.labels_all.max()) == C - 1
    assert float(case.logits.abs().max()) == 100.0 and bool(torch.isfinite(case.logits).all())
    assert cc.scratch_bytes(S, B, Q, case.M) == 8 * S * ((B * Q + 3) // 4) + 8 * S * case.M


def test_shapes_reach_what_their_notes_name():
    c = [_case(i, s) for i, s in CASES]
    # two blocks, the second with one live wave: rows 0 .. 3 and row 4, which is matched (query Q - 1 of the only image)
    assert c[0].B * c[0].Q == 5 and -(-5 // cc.ROWS_PER_BLOCK) == 2 and c[0].C < 64
    assert all(4 in c[0].q_idx[s].tolist() for s in range(c[0].S))
    # lane strides: 64 + 36, 64 + 64 + 2, exactly 64
    assert [c[1].C - 64, c[2].C - 128, c[3].C] == [36, 2, 64] and c[1].B * c[1].Q == 14
    # the ballot rounds of find_pair: M = 65, the pair in the last lane of round 0 is row 0, the pair in lane 0 of round 1 the last row
    assert c[2].M == 65 and c[3].M == 64
    assert (int(c[2].image_of[63]), int(c[2].q_idx[0, 63])) == (0, 0)
    assert (int(c[2].image_of[64]), int(c[2].q_idx[0, 64])) == (c[2].B - 1, c[2].Q - 1)
    assert int(c[2].t_idx[0, 64]) != int(c[2].t_idx[0, 0])              # (a lost k0 would hand the last row another target)
    assert not bool(torch.equal(c[2].boxes_all[c[2].t_idx[0, 64]], c[2].boxes_all[c[2].t_idx[0, 0]]))
    # an image without targets; every row matched
    assert c[3].sizes[1] == 0 and 1 not in c[3].image_of.tolist()
    assert c[4].M == c[4].Q * c[4].B and bool(cc.row_masks(c[4])[2].sum() == 0)
    assert (c[5].S, c[5].B, c[5].Q, c[5].C) == (7, 2, 900, 256)
    # the same query number is matched in two images somewhere (the image is part of the key)
    assert any(int(q) in c[1].q_idx[s, 4:].tolist() for s in range(c[1].S) for q in c[1].q_idx[s, :4])


@pytest.mark.parametrize("i,shape", CASES, ids=IDS)
def test_logit_groups_and_box_kinds_are_where_claimed(i, shape):
    case = _case(i, shape)
    S, B, Q, C, sizes, _ = shape
    assert case.n_kinds == min(10, case.M)
    sat = torch.tensor(cc.SATURATED)
    assert len(case.saturated_rows) == 2 * S
    for n, (s, b, q, label, j) in enumerate(case.saturated_rows):
        row, grp = case.logits[s, b, q], case.group[s, b, q]
        assert sorted(row[grp == cc.SATURATED_GROUP].tolist()) == sorted(sat.tolist())
        k = [k for k in range(case.M) if int(case.image_of[k]) == b and int(case.q_idx[s, k]) == q]
        if n % 2 == 0:      # the matched one: the label sits on value number (s + i) mod 8
            assert len(k) == 1 and int(case.labels_all[case.t_idx[s, k[0]]]) == label
            assert j == (s + i) % 8 and float(row[label]) == float(sat[j])
        elif k:             # every row matched: the label is off the eight
            assert int(grp[label]) != cc.SATURATED_GROUP
        else:
            assert bool(cc.row_masks(case)[2][s, b, q])
    # one label on a filled column per set; every pair's label column is ordinary, saturated or that one
    assert (case.group == cc.FILLED_LABEL).sum() == S
    s_i, b_i, q_i, t_i = cc.flat_index(case)
    on_label = case.group[s_i, b_i, q_i, case.labels_all[t_i]]
    assert int((on_label == cc.FILLED_LABEL).sum()) == S and int((on_label == cc.SATURATED_GROUP).sum()) >= S
    assert bool((case.logits[case.group == cc.FILLED_LABEL] == cc.FILL).all())
    assert bool((case.logits[case.group == cc.FILLED] == cc.FILL).all())
    for s in range(S):
        kinds = sorted(int(v) for v in case.kind[s] if v >= 0)
        assert kinds == (list(range(case.n_kinds)) if s % 2 == 0 else [])
        for k in range(case.M):
            j = int(case.kind[s, k])
            if j >= 0:
                assert torch.equal(case.boxes[s, case.image_of[k], case.q_idx[s, k]] * 64, torch.tensor(cc.KINDS[j][1]).float())
                assert torch.equal(case.boxes_all[case.t_idx[s, k]] * 64, torch.tensor(cc.DYADIC_TARGET).float())
    dyadic, other, unmatched = cc.row_masks(case)
    assert int(dyadic.sum()) == case.n_kinds * ((S + 1) // 2) and int(dyadic.sum() + other.sum()) == S * case.M


def test_saturated_label_cycles_over_all_eight_values():
    seen = {j for i, s in CASES for (_, _, _, _, j) in _case(i, s).saturated_rows if j >= 0}
    assert seen == set(range(8))


def test_box_kinds_are_the_kinks_they_name():
    geo = [cc.kind_geometry(k) for k in range(len(cc.KINDS))]
    names = [n for n, _ in cc.KINDS]
    assert geo[names.index("identical")] == (16, 16, 256)
    assert geo[names.index("disjoint in x")][0] < 0
    assert geo[names.index("touching: x0 == X1")][0] == 0 and geo[names.index("touching: x0 == X1")][1] > 0
    assert geo[names.index("zero area at the centre")] == (0, 0, 0)
    iw, ih, area = geo[names.index("zero area and disjoint")]
    assert iw < 0 and ih < 0 and area == 0
    cx, cy, w, h = cc.KINDS[names.index("containing the target")][1]
    assert cx - w / 2 < 24 and cx + w / 2 > 40 and cy - h / 2 < 24 and cy + h / 2 > 40
    cx, cy, w, h = cc.KINDS[names.index("contained and centred")][1]
    assert (cx, cy) == (32, 32) and w < 16 and h < 16
    cx, cy, w, h = cc.KINDS[names.index("one x edge and both y edges shared")][1]
    assert (cx - w / 2, cy - h / 2, cy + h / 2) == (24, 24, 40) and cx + w / 2 < 40
    cx, cy, w, h = cc.KINDS[names.index("same x extent, half the height")][1]
    assert (cx - w / 2, cx + w / 2, h) == (24, 40, 8)
    iw, ih, area = geo[names.index("general overlap")]
    assert 0 < iw < 16 and 0 < ih < 12
    for _, box in cc.KINDS:      # corners on multiples of 2^-6
        assert all(v % 2 == 0 for v in box[2:])


@pytest.mark.parametrize("num_boxes", cc.NUM_BOXES)
@pytest.mark.parametrize("alpha,gamma", cc.PARAMS)
@pytest.mark.parametrize("i,shape", SMALL, ids=SMALL_IDS)
def test_reference_rounds_to_the_float32_chain(i, shape, alpha, gamma, num_boxes):
    """Everything is finite in both precisions; the float64 reference agrees with the float32 chain to float32's rounding
    (per logit group and per kind of pair, relative to the group's largest magnitude); on the dyadic pairs the float32
    chain's box gradient is exactly zero where the float64 reference's is, and only there."""
    case = _case(i, shape)
    out64, gl64, gb64 = cc.reference_f64(shape, i, alpha, gamma, num_boxes)
    out32, gl32, gb32 = cc.chain(case, alpha, gamma, num_boxes, dtype=torch.float32)
    for t in (out64, gl64, gb64, out32, gl32, gb32):
        assert bool(torch.isfinite(t).all())
    for row in range(3):
        assert cc.group_err(out32[row], out64[row]) <= 2e-6
    for name, code in cc.LOGIT_GROUPS.items():
        if name == "fill":          # x = -100, t = 0: the float32 gradient underflows to 0 (float64: below 1e-80)
            assert float(gl64[case.group == code].abs().max()) < 1e-40 and float(gl32[case.group == code].abs().max()) < 1e-37
        else:
            assert cc.group_err(gl32, gl64, case.group == code) <= 1e-5, name
    dyadic, other, unmatched = cc.row_masks(case)
    for mask in (dyadic, other):
        e = cc.group_err(gb32, gb64, mask)
        assert e is None or e <= 1e-5
    assert bool((gb64[unmatched] == 0).all()) and bool((gb32[unmatched] == 0).all())
    assert torch.equal(gb32[dyadic] == 0, gb64[dyadic] == 0)
    assert bool((gb64[dyadic] == 0).any()) and bool((gb64[dyadic] != 0).any())


def test_model_size_reference_rounds_to_the_float32_chain():
    i, shape = CASES[-1]
    case = _case(i, shape)
    out64, gl64, gb64 = cc.reference_f64(shape, i, 0.25, 2.0, 3.5)
    out32, gl32, gb32 = cc.chain(case, 0.25, 2.0, 3.5, dtype=torch.float32)
    assert cc.group_err(out32, out64) <= 2e-6 and cc.group_err(gl32, gl64) <= 1e-5 and cc.group_err(gb32, gb64) <= 1e-5
    dyadic = cc.row_masks(case)[0]
    assert torch.equal(gb32[dyadic] == 0, gb64[dyadic] == 0)


def test_null_gradient_requests_of_the_chain():
    case = _case(1, cc.SHAPES[1])
    full = cc.chain(case, 0.25, 2.0, 3.5)
    only_boxes, only_logits = cc.chain(case, 0.25, 2.0, 3.5, want_logits=False), cc.chain(case, 0.25, 2.0, 3.5, want_boxes=False)
    assert only_boxes[1] is None and only_logits[2] is None
    assert torch.equal(only_boxes[2], full[2]) and torch.equal(only_logits[1], full[1])


def test_reference_reproduces_the_golden_losses_and_gradients():
    """tests/golden/mod_criterion.pt (the reference project's criterion on 4 prediction sets, 2 images, 30 queries, 16 columns,
    4 + 6 targets) with its own assignments: the 12 losses, and the gradients of the weighted total with respect to the
    final layer's logits and boxes."""
    g = torch.load(GOLDEN, weights_only=False)
    case = cc.golden_case(g)
    names = ["_%d" % n for n in range(case.final_set)] + ["", "_enc"]
    w = g["weight_dict"]
    g_out = torch.tensor([[float(w[k + suf]) for suf in names] for k in ("loss_class", "loss_bbox", "loss_giou")])
    num_boxes = float(max(case.T, 1))
    out, gl, gb = cc.chain(case, 0.25, 2.0, num_boxes, g_out=g_out)
    for row, k in enumerate(("loss_class", "loss_bbox", "loss_giou")):
        for s, suf in enumerate(names):
            want = float(g["losses"][k + suf])
            assert abs(float(out[row, s]) - want) <= 2e-6 * abs(want), (k + suf, float(out[row, s]), want)
    assert abs(float((out * g_out).sum()) - float(g["total"])) <= 2e-6 * float(g["total"])
    assert cc.group_err(g["grad_pred_logits"], gl[case.final_set]) <= 1e-5
    assert cc.group_err(g["grad_pred_boxes"], gb[case.final_set]) <= 1e-5


@pytest.mark.parametrize("shape", cc.COST_SHAPES, ids=[s[3].split(":")[0].replace(" ", "_") for s in cc.COST_SHAPES])
def test_matching_cost_cases(shape):
    case = cc.make_cost_case(shape)
    N, C, T, _ = shape
    ids = case.ids.tolist()
    assert 0 in ids and (T == 1 or C - 1 in ids) and (T <= 3 or len(set(ids)) < T)
    assert case.n_kinds == min(10, N) and torch.equal(case.tgt_boxes[0] * 64, torch.tensor(cc.DYADIC_TARGET).float())
    for j in range(case.n_kinds):
        assert torch.equal(case.boxes[j] * 64, torch.tensor(cc.KINDS[j][1]).float())
    corners = torch.cat([case.tgt_boxes[:case.n_dyadic, :2] - case.tgt_boxes[:case.n_dyadic, 2:] / 2,
                         case.tgt_boxes[:case.n_dyadic, :2] + case.tgt_boxes[:case.n_dyadic, 2:] / 2]) * 64
    assert torch.equal(corners, corners.round())
    rows = case.saturated.any(1).nonzero().flatten()
    assert len(rows) == min(8, N)
    for n, r in enumerate(rows):
        assert bool((case.logits[r, case.ids] == torch.tensor(cc.SATURATED)[n]).all())
    if N * T == 259:
        assert -(-259 // 256) == 2 and 259 - 256 == 3
    for weights in cc.COST_WEIGHTS:
        for alpha, gamma in cc.COST_PARAMS:
            c64 = cc.cost_chain(case, weights, alpha, gamma)
            c32 = cc.cost_chain(case, weights, alpha, gamma, dtype=torch.float32)
            assert bool(torch.isfinite(c64).all()) and bool(torch.isfinite(c32).all())
            # float32 forms 1 - p + 1e-8 from a p rounded to 2^-24: beyond |x| = 4 the logarithm's argument has lost digits
            # (1.5e-3 of the largest cost at |x| = 12), so the rounding claim is made where 1 - p >= 0.018
            moderate = (case.logits[:, case.ids].abs() <= 4) & ~case.saturated
            e = cc.group_err(c32, c64, moderate)
            assert e is None or e <= 1e-5
    # weights (0, 1, 0): the L1 distance alone, exact on the dyadic boxes
    l1 = cc.cost_chain(case, (0.0, 1.0, 0.0), 0.25, 2.0)[:case.n_kinds, :case.n_dyadic]
    assert torch.equal(l1 * 64, (l1 * 64).round())
