"""The fused bi-softmax (csrc/bisoftmax.hip) through its C ABI, zira_bisoftmax_{fwd,bwd}_f32, on every branch of its launchers:
tests/bisoftmax_cases.py holds the shapes, the inputs and the float64 reference (proven on the CPU by
test_bisoftmax_cases_cpu.py).  Exact on one-hot inputs; against float64 beside the fp32 composition at N(0, 1) and at peaked
scores; the clamps where they bind; fully masked images; the scratch contract with sentinels behind every output; bitwise
repeatability.  Every call here gets a workspace of exactly the reported size, filled with NaN before the forward and again
before the backward, and checks the sentinels behind the workspace and the seven outputs."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bisoftmax_cases as bc  # noqa: E402
from ziragroundingdino_amd import _lib  # noqa: E402

DEV = "cuda"
PAD = 64
IDS = [bc.shape_id(s) for s in bc.SHAPES]
FWD_SHAPES = {"pv": "xm", "e": "xm", "colsum": "c", "colmax": "c", "gmax": None, "g_xm": "xm", "g_c": "c"}


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


def _input(t, offset=0):
    """A tensor on the GPU, ``offset`` floats into its buffer (torch's allocations are 512-byte aligned: 1 = misaligned)."""
    if not offset:
        return t.to(DEV).contiguous()
    buf = torch.full((t.numel() + offset,), -7.0, device=DEV)
    buf[offset:] = t.to(DEV).flatten()
    return buf[offset:].view(t.shape)


def _mask(m):
    return None if m is None else m.to(DEV, torch.uint8).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def run(case, workspace="exact", offset=None):
    """Forward and backward of a case -> the seven outputs on the GPU.  ``workspace``: "exact" = the reported size, NaN-filled
    before each of the two calls, or "large" = twice that and 1024 floats more, zeroed.  ``offset``: xm and g_pv that many
    floats into their buffers (default: 1 for the shape whose note says misaligned)."""
    lib = _lib.load()
    B, N, H, T = case.B, case.N, case.H, case.T
    HT = H * T
    offset = int(bc.misaligned(case.shape)) if offset is None else offset
    xm, g_pv = _input(case.xm, offset), _input(case.g_pv, offset)
    assert not offset or xm.data_ptr() % 16 != 0
    c, g_e, g_colsum = _input(case.c), _input(case.g_e), _input(case.g_colsum)
    ml, mv = _mask(case.mask_l), _mask(case.mask_v)
    n = int(lib.zira_bisoftmax_workspace_floats(B, N, H, T))
    assert n == bc.dispatch(N, H, T).workspace_floats(B)
    ws = _Guarded(n) if workspace == "exact" else _Guarded(2 * n + 1024)
    if workspace != "exact":
        ws.body.zero_()
    out = {name: _Guarded({"xm": B * N * HT, "c": B * HT, None: 1}[like], {"xm": (B, N, HT), "c": (B, HT), None: (1,)}[like])
           for name, like in FWD_SHAPES.items()}
    o = {name: g.view for name, g in out.items()}
    flags = (int(case.stable), int(case.clamp_lo), int(case.clamp_hi))
    rc = lib.zira_bisoftmax_fwd_f32(_p(xm), _p(c), _p(ml), _p(mv), B, N, H, T, *flags, _p(o["pv"]), _p(o["e"]), _p(o["colsum"]),
                                    _p(o["colmax"]), _p(o["gmax"]), _p(ws.body), _stream())
    assert rc == 0
    if workspace == "exact":
        ws.body.fill_(float("nan"))
    rc = lib.zira_bisoftmax_bwd_f32(_p(xm), _p(c), _p(ml), B, N, H, T, *flags, _p(o["pv"]), _p(o["e"]), _p(o["colmax"]), _p(o["gmax"]),
                                    _p(g_pv), _p(g_e), _p(g_colsum), _p(o["g_xm"]), _p(o["g_c"]), _p(ws.body), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert ws.intact(), "written outside the workspace of the reported size"
    for name, g in out.items():
        assert g.intact(), "%s: written outside the tensor" % name
    return o


def err(a, b64):
    """Largest error relative to the float64 tensor's own largest magnitude."""
    return float((a.double() - b64).abs().max() / b64.abs().max())


# Bars of the float64 comparisons: err(kernel) <= RATIO * err(fp32 composition on the same device) + FLOOR, both errors relative
# to the float64 tensor's largest magnitude.  FLOOR: four units of 2^-24 of that magnitude (a few fp32 ulps of the output's
# scale), for the figures on which the composition happens to be exact or nearly so.
# RATIO: measured on MI355X as the worst err(kernel) / err(composition) over the 24 shapes of bisoftmax_cases.SHAPES at gains
# 1 and 8 (MEASURED_RATIO; 48 figures per output), doubled and rounded up to one digit.  e, colmax and gmax came out bit for
# bit the composition's on all 48 (the same fp32 additions and the same expf), g_xm on most.  The two largest:
#   colsum 3.86 at N = 40000, T = 1 (4.96e-7 against 1.28e-7; 1.74 at most elsewhere): a column's 40000 terms are added 64 in a
#     row per tile, two tiles per block, then 16 partials in a row per fold phase and the 32 phases in a row -- 8 units of
#     2^-24 of the sum after ~110 dependent additions, where ATen's sum is a tree;
#   pv 2.50 at H*T = 2048 (the walk, gain 8: 1.32e-6 against 5.28e-7): one thread adds a group's 125 exponentials in a row.
# The other cases of this file (clamps, fully masked images; 14 figures per output) stay below these ratios but for pv in the
# walk at T = 129, 5.7 and 5.3 x the composition -- 4.9e-7 and 3.0e-7, eight and five units of 2^-24 after ~120 additions in
# a row, beside a composition that is within 1.4 units there: the FLOOR carries that (bar 6.7e-7 and 5.2e-7).
FLOOR = 4 * 2.0 ** -24
MEASURED_RATIO = {"pv": 2.50, "e": 1.00, "colsum": 3.86, "colmax": 1.00, "gmax": 1.00, "g_xm": 1.09, "g_c": 1.83}
RATIO = {"pv": 5.0, "e": 2.0, "colsum": 8.0, "colmax": 2.0, "gmax": 2.0, "g_xm": 3.0, "g_c": 4.0}


def check_against_f64(tag, case, got):
    """Print every figure, then assert the bar for each of the seven outputs."""
    want, comp = bc.reference_all(case, DEV), bc.composition_all(case, DEV)
    figs = []
    for name in bc.OUTPUTS:
        figs.append((name, err(got[name], getattr(want, name)), err(getattr(comp, name), getattr(want, name))))
        print("BISFIG %s %s kernel %.3e composition %.3e" % (tag, name, figs[-1][1], figs[-1][2]))
    for name, ek, ec in figs:
        assert ek <= RATIO[name] * ec + FLOOR, "%s %s: kernel %.3e, composition %.3e, bar %.3e" % (tag, name, ek, ec, RATIO[name] * ec + FLOOR)


@functools.lru_cache(maxsize=None)
def _randn(i, gain=1.0):
    return bc.randn_case(bc.SHAPES[i], seed=300 + i, gain=gain)


@pytest.mark.parametrize("i", range(len(bc.SHAPES)), ids=IDS)
def test_exact_inputs_give_exact_results(i):
    """bisoftmax_cases.exact_case: pv one-hot, e in {0, 1}, colsum a count, g_xm and g_c small integers -- every output is
    bit-exact whatever the order of the sums.  A wrong column <-> head or row <-> column map, a skipped or doubled row tile, an
    ignored mask or a lost partial sum changes integers."""
    case = bc.exact_case(bc.SHAPES[i], seed=100 + i)
    got = run(case)
    for name in bc.OUTPUTS:
        assert torch.equal(got[name].cpu(), getattr(case.want, name)), name


@pytest.mark.parametrize("gain", [1.0, 8.0])
@pytest.mark.parametrize("i", range(len(bc.SHAPES)), ids=IDS)
def test_matches_float64_beside_the_composition(i, gain):
    """N(0, 1) scores and scores of deviation 8 (peaked softmaxes): the seven outputs against float64, with the error of the
    fp32 composition on the same inputs and device as the yardstick (RATIO, FLOOR above)."""
    case = _randn(i, gain)
    check_against_f64("%s gain %g" % (IDS[i], gain), case, run(case))


@pytest.mark.parametrize("shape", bc.CLAMP_SHAPES, ids=[bc.shape_id(s) for s in bc.CLAMP_SHAPES])
def test_clamps_where_they_bind(shape):
    """bisoftmax_cases.clamp_case: groups that lie wholly beyond a clamp are EXACTLY uniform over their live tokens, g_xm is
    exactly 0 wherever the first clamp clipped and nonzero on the entries exactly on +-50000; the rest against float64."""
    case = bc.clamp_case(shape, seed=5)
    B, N, H, T = shape[:4]
    got = run(case)
    pv = got["pv"].cpu().view(B, N, H, T)
    dead = torch.zeros(B, 1, 1, T, dtype=torch.bool) if case.mask_l is None else case.mask_l.view(B, 1, 1, T)
    spread = pv.masked_fill(dead, -1.0).amax(-1) - pv.masked_fill(dead, 2.0).amin(-1)
    assert float(spread[case.uniform].max()) == 0.0
    assert float(pv.masked_fill(~dead, 0.0).abs().max()) == 0.0
    g_xm = got["g_xm"].cpu()
    assert float(g_xm[case.clipped].abs().max()) == 0.0
    assert float(g_xm[case.edge].abs().min()) > 0.0
    check_against_f64("clamp %s" % bc.shape_id(shape), case, got)


@pytest.mark.parametrize("shape", bc.CONVENTION_SHAPES, ids=[bc.shape_id(s) for s in bc.CONVENTION_SHAPES])
def test_image_with_every_text_token_masked(shape):
    """pv = 0 for that image on every forward branch, no NaN in any output; the other image bit for bit what it is without."""
    case = bc.randn_case(shape, seed=11)
    plain, got = run(case), run(bc.fully_masked(case, text_image=0))
    for name in bc.OUTPUTS:
        assert bool(torch.isfinite(got[name]).all()), name
        if name != "gmax":
            assert torch.equal(got[name][1], plain[name][1]), name
    assert float(got["pv"][0].abs().max()) == 0.0
    assert torch.equal(got["e"], plain["e"]) and torch.equal(got["colsum"], plain["colsum"])
    check_against_f64("textmasked %s" % bc.shape_id(shape), bc.fully_masked(case, text_image=0), got)


@pytest.mark.parametrize("shape", bc.CONVENTION_SHAPES, ids=[bc.shape_id(s) for s in bc.CONVENTION_SHAPES])
def test_image_with_every_image_token_masked(shape):
    """e = 0 and colsum = 0 for that image, no NaN; pv, the maxima and the other image bit for bit what they are without."""
    case = bc.randn_case(shape, seed=12)
    plain, got = run(case), run(bc.fully_masked(case, rows_image=0))
    for name in bc.OUTPUTS:
        assert bool(torch.isfinite(got[name]).all()), name
        if name != "gmax":
            assert torch.equal(got[name][1], plain[name][1]), name
    assert float(got["e"][0].abs().max()) == 0.0 and float(got["colsum"][0].abs().max()) == 0.0
    for name in ("pv", "colmax", "gmax"):
        assert torch.equal(got[name], plain[name]), name
    check_against_f64("rowsmasked %s" % bc.shape_id(shape), bc.fully_masked(case, rows_image=0), got)


@pytest.mark.parametrize("i", range(len(bc.SHAPES)), ids=IDS)
def test_workspace_needs_no_initialisation_and_no_more_than_reported(i):
    """A NaN-filled workspace of exactly zira_bisoftmax_workspace_floats (run() checks the sentinels round it and round the
    outputs) gives bit for bit what a zeroed workspace of more than twice the size gives."""
    case = _randn(i)
    exact, large = run(case, "exact"), run(case, "large")
    for name in bc.OUTPUTS:
        assert bool(torch.isfinite(exact[name]).all()), name
        assert torch.equal(exact[name], large[name]), name


@pytest.mark.parametrize("i", range(len(bc.SHAPES)), ids=IDS)
def test_two_runs_are_bit_identical(i):
    """No atomics, a fixed order of the partial sums."""
    case = _randn(i, 8.0)
    one, two = run(case), run(case)
    for name in bc.OUTPUTS:
        assert torch.equal(one[name], two[name]), name


@pytest.mark.parametrize("shape", bc.CONVENTION_SHAPES, ids=[bc.shape_id(s) for s in bc.CONVENTION_SHAPES])
def test_null_masks_are_all_zero_masks(shape):
    case = bc.randn_case(shape, seed=13)
    case.mask_l = case.mask_v = None
    zeros = bc.types.SimpleNamespace(**case.__dict__)
    zeros.mask_l, zeros.mask_v = torch.zeros(case.B, case.T, dtype=torch.bool), torch.zeros(case.B, case.N, dtype=torch.bool)
    null, zero = run(case), run(zeros)
    for name in bc.OUTPUTS:
        assert torch.equal(null[name], zero[name]), name


def test_more_than_2048_columns_are_refused():
    """H*T = 2049: ZIRA_MSDA_EINVAL from both entry points, nothing launched (every buffer keeps what it held)."""
    lib = _lib.load()
    B, N, H, T = 1, 2, 1, 2049
    big = [torch.full((B * N * H * T,), 3.0, device=DEV) for _ in range(6)]         # xm, g_pv, g_e, pv, e, g_xm
    small = [torch.full((B * H * T,), 3.0, device=DEV) for _ in range(5)]           # c, g_colsum, colsum, colmax, g_c
    gmax, ws = torch.full((1,), 3.0, device=DEV), torch.full((65536,), 3.0, device=DEV)
    xm, g_pv, g_e, pv, e, g_xm = big
    c, g_colsum, colsum, colmax, g_c = small
    assert lib.zira_bisoftmax_fwd_f32(_p(xm), _p(c), None, None, B, N, H, T, 1, 1, 1, _p(pv), _p(e), _p(colsum), _p(colmax), _p(gmax),
                                      _p(ws), _stream()) == 1
    assert lib.zira_bisoftmax_bwd_f32(_p(xm), _p(c), None, B, N, H, T, 1, 1, 1, _p(pv), _p(e), _p(colmax), _p(gmax), _p(g_pv), _p(g_e),
                                      _p(g_colsum), _p(g_xm), _p(g_c), _p(ws), _stream()) == 1
    torch.cuda.synchronize()
    for t in big + small + [gmax, ws]:
        assert bool((t == 3.0).all())
    # 2048 columns are served (bisoftmax_cases.SHAPES has the shape)
    assert lib.zira_bisoftmax_workspace_floats(1, 515, 16, 128) > 0
