"""The loss tail through its C ABI -- zira_match_cost_f32 (csrc/lsap.hip) and zira_stacked_losses_{fwd,bwd}_f32
(csrc/criterion.hip) -- on hand-made matches: tests/criterion_cases.py holds the shapes, the inputs and the float64 reference
(proven on the CPU by test_criterion_cases_cpu.py).  Against float64 beside the float32 op chain, per logit group and per kind
of pair, for every (alpha, gamma) branch; exact zeros and full writes; null gradients; refusals; bitwise repeatability; the
matching cost's bad-box flag.  Every call writes into NaN-filled outputs with sentinels before and behind them and gets a
NaN-filled scratch of exactly the reported size."""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

pytestmark = pytest.mark.gpu

import criterion_cases as cc  # noqa: E402
from ziragroundingdino_amd import _lib  # noqa: E402

DEV = "cuda"
PAD = 64
EINVAL = 1      # hipErrorInvalidValue
CASES = list(enumerate(cc.SHAPES))
IDS = [cc.shape_id(s) for s in cc.SHAPES]
MODEL = (len(cc.SHAPES), cc.MODEL_SHAPE)

# Bars of the float64 comparisons: err(kernel) <= RATIO * err(float32 op chain on the same device) + FLOOR, both errors relative
# to the float64 tensor's largest magnitude within the group (criterion_cases.group_err).  RATIO is test_groupnorm_gpu.py's,
# FLOOR test_textside_gpu.py's; neither is fitted to these kernels.
# Measured on MI355X, the worst err over the five small shapes, the five (alpha, gamma) and both num_boxes -- kernel / chain
# (model-size run in brackets); the kernel's worst share of its bar is 0.50:
#   loss_class 1.06e-07 / 1.67e-07 (6.84e-08 / 1.47e-07)      loss_bbox 7.78e-08 / 7.78e-08 (7.52e-08 / 7.52e-08)
#   loss_giou  9.53e-08 / 9.53e-08 (5.50e-08 / 5.50e-08)
#   g_logits ordinary  8.20e-07 / 7.45e-07 (8.11e-07 / 8.88e-07)      saturated 1.34e-06 / 1.39e-06 (1.31e-06 / 1.31e-06)
#   g_logits label on a filled column 3.58e-08 / 1.03e-07 (3.29e-08 / 3.29e-08)
#   g_logits fill: 0 / 0 -- x = -100 with t = 0 gives an exact 0 in float64 too (1 - p rounds to 1)
#   g_boxes dyadic pairs 1.05e-07 / 1.64e-07 (9.90e-08 / 1.38e-07)    random pairs 1.67e-07 / 1.78e-07 (1.18e-07 / 1.16e-07)
# Matching cost (four shapes, two weightings, two (alpha, gamma)): rows with saturated logits 8.78e-02 / 8.78e-02, other rows
# 1.66e-03 / 1.66e-03 -- both arms form 1 - p + 1e-8 from a float32 p, which loses the logarithm's argument beyond |x| = 12
# and all of it at 17; the kernel follows the chain's roundings there (largest |kernel - chain| 2.9e-06 at a largest cost of
# 28, inside rtol = atol = 2e-6), which is what keeps the assignments the chain's.
RATIO = 2.0
FLOOR = 4 * 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pattern():
    return 1000.0 + torch.arange(PAD, device=DEV, dtype=torch.float32)          # the sentinel: no NaN in it


class _Guarded:
    """``n`` floats (NaN to begin with) with the sentinel pattern before and behind them."""

    def __init__(self, n, shape=None):
        self.raw = torch.full((PAD + n + PAD,), float("nan"), device=DEV)
        self.raw[:PAD], self.raw[-PAD:] = _pattern(), _pattern()
        self.body = self.raw[PAD:PAD + n]
        self.view = self.body.view(shape) if shape is not None else self.body

    def intact(self):
        return torch.equal(self.raw[:PAD], _pattern()) and torch.equal(self.raw[-PAD:], _pattern())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.body).all())


def _p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def _inputs(i, shape, num_boxes):
    case = cc.make_case(shape, i)
    d = {k: getattr(case, k).to(DEV).contiguous() for k in ("logits", "boxes", "q_idx", "t_idx", "image_of", "labels_all", "boxes_all", "g_out")}
    d["nb"] = torch.tensor([num_boxes], dtype=torch.float32, device=DEV)
    return case, d


def _buffers(case):
    lib = _lib.load()
    n = int(lib.zira_stacked_losses_scratch_bytes(case.S, case.B, case.Q, case.M))
    assert n == cc.scratch_bytes(case.S, case.B, case.Q, case.M) and n % 8 == 0
    return {"scratch": _Guarded(n // 4), "out": _Guarded(3 * case.S, (3, case.S)),
            "g_logits": _Guarded(case.logits.numel(), tuple(case.logits.shape)), "g_boxes": _Guarded(case.boxes.numel(), tuple(case.boxes.shape))}


def _fwd_args(case, d, buf, alpha, gamma):
    return [_p(d["logits"]), _p(d["boxes"]), _p(d["q_idx"]), _p(d["t_idx"]), _p(d["image_of"]), _p(d["labels_all"]), _p(d["boxes_all"]),
            _p(d["nb"]), case.S, case.B, case.Q, case.C, case.M, alpha, gamma, _p(buf["scratch"].body), _p(buf["out"].body), _stream()]


def _bwd_args(case, d, buf, alpha, gamma, want_logits=True, want_boxes=True):
    return [_p(d["logits"]), _p(d["boxes"]), _p(d["q_idx"]), _p(d["t_idx"]), _p(d["image_of"]), _p(d["labels_all"]), _p(d["boxes_all"]),
            _p(d["nb"]), _p(d["g_out"]), case.S, case.B, case.Q, case.C, case.M, alpha, gamma,
            _p(buf["g_logits"].body) if want_logits else None, _p(buf["g_boxes"].body) if want_boxes else None, _stream()]


def run(i, shape, alpha, gamma, num_boxes, want_logits=True, want_boxes=True):
    """Forward and backward on a case -> (out, g_logits, g_boxes, buffers): the sentinels round the scratch and round every
    output are checked here, and that an output that was not asked for is still all NaN."""
    lib = _lib.load()
    case, d = _inputs(i, shape, num_boxes)
    buf = _buffers(case)
    assert lib.zira_stacked_losses_fwd_f32(*_fwd_args(case, d, buf, alpha, gamma)) == 0
    assert lib.zira_stacked_losses_bwd_f32(*_bwd_args(case, d, buf, alpha, gamma, want_logits, want_boxes)) == 0
    torch.cuda.synchronize()
    for name, g in buf.items():
        assert g.intact(), "written outside %s" % name
    assert want_logits or buf["g_logits"].untouched()
    assert want_boxes or buf["g_boxes"].untouched()
    return buf["out"].view, buf["g_logits"].view, buf["g_boxes"].view, buf


def _figures(tag, case, got, chain32, ref64):
    """[(group, err(kernel), err(chain))] of the losses (per quantity), g_logits (per logit group) and g_boxes (dyadic pairs,
    the other pairs), each printed."""
    figs = []
    for row, name in enumerate(("loss_class", "loss_bbox", "loss_giou")):
        figs.append((name, cc.group_err(got[0][row], ref64[0][row]), cc.group_err(chain32[0][row], ref64[0][row])))
    for name, code in cc.LOGIT_GROUPS.items():
        mask = case.group == code
        figs.append(("g_logits " + name, cc.group_err(got[1], ref64[1], mask), cc.group_err(chain32[1], ref64[1], mask)))
    dyadic, other, _ = cc.row_masks(case)
    for name, mask in (("dyadic pairs", dyadic), ("random pairs", other)):
        figs.append(("g_boxes " + name, cc.group_err(got[2], ref64[2], mask), cc.group_err(chain32[2], ref64[2], mask)))
    figs = [f for f in figs if f[1] is not None]
    for name, ek, ec in figs:
        print("LOSSFIG %s | %s | kernel %.3e chain %.3e" % (tag, name, ek, ec))
    return figs


def _check(i, shape, alpha, gamma, num_boxes):
    case = cc.make_case(shape, i)
    out, gl, gb, _ = run(i, shape, alpha, gamma, num_boxes)
    for t in (out, gl, gb):
        assert not bool(torch.isnan(t).any()), "an element was left unwritten"
    ref64 = cc.reference_f64(shape, i, alpha, gamma, num_boxes)
    chain32 = cc.chain(case, alpha, gamma, num_boxes, dtype=torch.float32, device=DEV)
    tag = "%s alpha %g gamma %g num_boxes %g" % (cc.shape_id(shape), alpha, gamma, num_boxes)
    figs = _figures(tag, case, (out, gl, gb), chain32, ref64)
    dyadic, other, unmatched = cc.row_masks(case)
    gb_cpu = gb.cpu()
    assert bool((gb_cpu[unmatched] == 0).all())
    assert torch.equal(gb_cpu[dyadic] == 0, ref64[2][dyadic] == 0)
    for name, ek, ec in figs:
        assert ek <= RATIO * ec + FLOOR, "%s %s: kernel %.3e, chain %.3e, bar %.3e" % (tag, name, ek, ec, RATIO * ec + FLOOR)


@pytest.mark.parametrize("num_boxes", cc.NUM_BOXES)
@pytest.mark.parametrize("alpha,gamma", cc.PARAMS)
@pytest.mark.parametrize("i,shape", CASES, ids=IDS)
def test_matches_float64_beside_the_chain(i, shape, alpha, gamma, num_boxes):
    """Losses and both gradients against the float64 reference with the float32 chain's own error as the yardstick; g_boxes
    exactly zero on unmatched rows and, on the dyadic pairs, exactly where the float64 reference is; no NaN left."""
    _check(i, shape, alpha, gamma, num_boxes)


def test_model_size_matches_float64_beside_the_chain():
    _check(MODEL[0], MODEL[1], 0.25, 2.0, 3.5)


@pytest.mark.parametrize("alpha,gamma", [(0.25, 2.0), (-1.0, 1.5)])
@pytest.mark.parametrize("i,shape", CASES, ids=IDS)
def test_null_gradients(i, shape, alpha, gamma):
    """With g_logits null, g_boxes is bit for bit that of the call with both and the logits' buffer is untouched (run()
    checks it); the converse; with both null the call is refused and nothing is written."""
    lib = _lib.load()
    _, gl, gb, _ = run(i, shape, alpha, gamma, 3.5)
    _, _, gb_only, _ = run(i, shape, alpha, gamma, 3.5, want_logits=False)
    _, gl_only, _, _ = run(i, shape, alpha, gamma, 3.5, want_boxes=False)
    assert torch.equal(gb_only, gb) and torch.equal(gl_only, gl)
    case, d = _inputs(i, shape, 3.5)
    buf = _buffers(case)
    assert lib.zira_stacked_losses_bwd_f32(*_bwd_args(case, d, buf, alpha, gamma, False, False)) == EINVAL
    torch.cuda.synchronize()
    assert all(g.untouched() for g in buf.values())


def test_refusals_launch_nothing():
    """Each null pointer, each of S, B, Q, C, M at 0, S = 65536, boxes / boxes_all / scratch off by 4 bytes: both entry points
    return hipErrorInvalidValue and every NaN-filled output and the scratch stay untouched."""
    lib = _lib.load()
    i, shape = CASES[1]
    case, d = _inputs(i, shape, 3.5)
    buf = _buffers(case)
    fwd, bwd = _fwd_args(case, d, buf, 0.25, 2.0), _bwd_args(case, d, buf, 0.25, 2.0)
    shifted = {}
    for k in ("boxes", "boxes_all"):     # the same numbers 4 bytes further on, inside a buffer of their own
        room = torch.zeros(d[k].numel() + 4, device=DEV)
        room[1:1 + d[k].numel()] = d[k].reshape(-1)
        shifted[k] = room
    tried = 0
    for name, fn, args, pointers, dims, aligned in (("fwd", lib.zira_stacked_losses_fwd_f32, fwd, list(range(8)) + [15, 16], range(8, 13), (1, 6, 15)),
                                                   ("bwd", lib.zira_stacked_losses_bwd_f32, bwd, list(range(9)), range(9, 14), (1, 6))):
        def refused(k, value, what):
            a = list(args)
            a[k] = value
            assert fn(*a) == EINVAL, (name, what, k)
            return 1
        for k in pointers:
            tried += refused(k, None, "null")
        for k in dims:
            tried += refused(k, 0, "zero")
        tried += refused(dims[0], 65536, "S = 65536")
        for k in aligned:
            at = shifted["boxes"].data_ptr() if k == 1 else shifted["boxes_all"].data_ptr() if k == 6 else args[k]
            tried += refused(k, at + 4, "off by 4 bytes")
    # both gradients null
    a = list(bwd)
    a[16] = a[17] = None
    assert lib.zira_stacked_losses_bwd_f32(*a) == EINVAL
    torch.cuda.synchronize()
    assert tried == (10 + 5 + 1 + 3) + (9 + 5 + 1 + 2)
    assert all(g.untouched() for g in buf.values())
    assert int(lib.zira_stacked_losses_scratch_bytes(0, 1, 1, 1)) == 0 == cc.scratch_bytes(0, 1, 1, 1)


@pytest.mark.parametrize("i,shape", CASES + [MODEL], ids=IDS + [cc.shape_id(cc.MODEL_SHAPE)])
def test_two_runs_are_bit_identical(i, shape):
    """No atomics, a fixed order of the partial sums."""
    one, two = run(i, shape, 0.25, 1.5, 3.5), run(i, shape, 0.25, 1.5, 3.5)
    for a, b in zip(one[:3], two[:3]):
        assert torch.equal(a, b)


# ---- the matching cost ---------------------------------------------------------------------------------------------------------

COST_IDS = ["N%d-C%d-T%d" % s[:3] for s in cc.COST_SHAPES]


@functools.lru_cache(maxsize=None)
def _cost_inputs(shape):
    case = cc.make_cost_case(shape)
    return case, {k: getattr(case, k).to(DEV).contiguous() for k in ("logits", "boxes", "ids", "tgt_boxes")}


def match_cost(case, d, weights, alpha, gamma, status="own"):
    """zira_match_cost_f32 into a guarded NaN-filled [N, T] -> (cost, the status word or None)."""
    lib = _lib.load()
    cost = _Guarded(case.N * case.T, (case.N, case.T))
    st = torch.zeros(1, dtype=torch.int32, device=DEV) if status == "own" else None
    rc = lib.zira_match_cost_f32(_p(d["logits"]), _p(d["boxes"]), _p(d["ids"]), _p(d["tgt_boxes"]), case.N, case.C, case.T, weights[0], weights[1],
                                 weights[2], alpha, gamma, _p(cost.body), _p(st), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert cost.intact() and not bool(torch.isnan(cost.body).any())
    return cost.view, None if st is None else int(st.item())


@pytest.mark.parametrize("alpha,gamma", cc.COST_PARAMS)
@pytest.mark.parametrize("weights", cc.COST_WEIGHTS, ids=["w111", "w252"])
@pytest.mark.parametrize("shape", cc.COST_SHAPES, ids=COST_IDS)
def test_matching_cost_matches_float64_beside_the_chain(shape, weights, alpha, gamma):
    """The bar of the losses, on the rows with saturated logits and on the rest separately; the float32 chain's numbers to
    2e-6 as in test_lsap_gpu.py; the bad-box flag stays clear on proper boxes."""
    case, d = _cost_inputs(shape)
    got, status = match_cost(case, d, weights, alpha, gamma)
    assert status == 0
    ref64 = cc.cost_chain(case, weights, alpha, gamma)
    chain32 = cc.cost_chain(case, weights, alpha, gamma, dtype=torch.float32, device=DEV)
    tag = "cost N %d C %d T %d w %s alpha %g gamma %g" % (shape[:3] + (weights, alpha, gamma))
    figs = []
    for name, mask in (("saturated rows", case.saturated), ("other rows", ~case.saturated)):
        ek, ec = cc.group_err(got, ref64, mask), cc.group_err(chain32, ref64, mask)
        if ek is not None:
            figs.append((name, ek, ec))
            print("LOSSFIG %s | %s | kernel %.3e chain %.3e" % (tag, name, ek, ec))
    print("LOSSFIG %s | kernel - chain | %.3e" % (tag, float((got - chain32).abs().max())))
    for name, ek, ec in figs:
        assert ek <= RATIO * ec + FLOOR, "%s %s: kernel %.3e, chain %.3e" % (tag, name, ek, ec)
    torch.testing.assert_close(got, chain32, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("shape", cc.COST_SHAPES, ids=COST_IDS)
def test_matching_cost_of_weights_0_1_0_is_the_exact_l1_distance(shape):
    """Exactly the float64 L1 distance on the dyadic boxes; float32's rounding of it and torch.cdist's bits on the rest."""
    case, d = _cost_inputs(shape)
    got, _ = match_cost(case, d, (0.0, 1.0, 0.0), 0.25, 2.0)
    want = cc.cost_chain(case, (0.0, 1.0, 0.0), 0.25, 2.0)
    assert torch.equal(got[:case.n_kinds, :case.n_dyadic].cpu().double(), want[:case.n_kinds, :case.n_dyadic])
    # elsewhere four differences and a tree of three sums, each rounded once: three units of 2^-24 of the entry at most
    assert cc.group_err(got, want) <= FLOOR
    # and on every input the bits of torch.cdist (the pairing of its reduction), as csrc/lsap.hip claims
    assert torch.equal(got, torch.cdist(d["boxes"], d["tgt_boxes"], p=1))


def test_assignments_from_the_kernel_cost_are_the_chain_s():
    shape = cc.COST_SHAPES[3]
    case, d = _cost_inputs(shape)
    got, _ = match_cost(case, d, (2.0, 5.0, 2.0), 0.25, 2.0)
    chain32 = cc.cost_chain(case, (2.0, 5.0, 2.0), 0.25, 2.0, dtype=torch.float32, device=DEV)
    for a, b in zip(got.view(3, 900, case.T).cpu().numpy(), chain32.view(3, 900, case.T).cpu().numpy()):
        for x, y in zip(linear_sum_assignment(a), linear_sum_assignment(b)):
            assert np.array_equal(x, y)


def test_bad_box_flag():
    """Set (bit 1 of the status word) by a prediction of negative width, by a target of negative height and by a NaN
    coordinate, not otherwise; a null status is accepted; lsap.bad_boxes reads and resets the package's own word."""
    from ziragroundingdino_amd import lsap

    shape = cc.COST_SHAPES[1]
    case, d = _cost_inputs(shape)
    w = (1.0, 1.0, 1.0)
    clean, status = match_cost(case, d, w, 0.25, 2.0)
    assert status == 0
    none, status = match_cost(case, d, w, 0.25, 2.0, status=None)
    assert status is None and torch.equal(none, clean)
    for key, row, col, value in (("boxes", case.N - 1, 2, -0.125), ("tgt_boxes", case.T - 1, 3, -0.125), ("boxes", 3, 0, float("nan")),
                                 ("tgt_boxes", 0, 1, float("nan"))):
        bad = dict(d)
        bad[key] = d[key].clone()
        bad[key][row, col] = value
        lib = _lib.load()
        cost = _Guarded(case.N * case.T)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert lib.zira_match_cost_f32(_p(bad["logits"]), _p(bad["boxes"]), _p(bad["ids"]), _p(bad["tgt_boxes"]), case.N, case.C, case.T, *w, 0.25, 2.0,
                                       _p(cost.body), _p(st), _stream()) == 0
        torch.cuda.synchronize()
        assert int(st.item()) == 2 and cost.intact(), (key, row, col, value)
    dev = torch.device("cuda", torch.cuda.current_device())
    lsap.bad_boxes(dev, reset=True)
    lsap.matching_cost(d["logits"], d["boxes"], d["ids"], d["tgt_boxes"])
    assert not lsap.bad_boxes(dev)
    boxes = d["boxes"].clone()
    boxes[5, 2] = -0.125
    lsap.matching_cost(d["logits"], boxes, d["ids"], d["tgt_boxes"])
    assert lsap.bad_boxes(dev, reset=True) and not lsap.bad_boxes(dev)
