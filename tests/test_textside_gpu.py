"""The fused text side (csrc/textside.hip) through its C ABI -- zira_text_prep_{fwd,bwd}_f32, zira_text_out_{fwd,bwd}_f32 -- on
every class of K chunk and every edge of its tiles: tests/textside_cases.py holds the shapes, the inputs and the float64
reference (proven on the CPU by test_textside_cases_cpu.py).  Exact on gather weights and on small integers; against float64
beside the fp32 composition; null gradients; stochastic depth; an image with colsum = 0; refusals; the scratch contract;
bitwise repeatability.  Every call here writes into NaN-filled outputs with sentinels before and behind them, and gets a
scratch of exactly the reported size, NaN-filled again before each of the two calls that use it, with sentinels behind it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import textside_cases as tc  # noqa: E402
from ziragroundingdino_amd import _lib  # noqa: E402

DEV = "cuda"
PAD = 64
EINVAL = 1      # hipErrorInvalidValue
IDS = [tc.shape_id(s) for s in tc.SHAPES]
N = len(tc.SHAPES)
# the shapes with a mixed chunk that holds columns of a
WITH_A = [i for i, s in enumerate(tc.SHAPES) if s[:5] in ((3, 9, 3, 32, 96), (2, 5, 3, 85, 100), (5, 13, 8, 20, 256))]
SEVERAL_IMAGES = [i for i, s in enumerate(tc.SHAPES) if s[0] > 1]


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


def _dev(t):
    return None if t is None else t.to(DEV, torch.float32).contiguous()


def _outputs(case):
    B, T, H, Dv, Dl = case.B, case.T, case.H, case.Dv, case.Dl
    shapes = {"l_ln": (B, T, Dl), "a": (B, Dv, H * T), "c": (B, H * T), "z": (B, H * T, Dv), "stats": (B * T, 2), "g_l_in": (B, T, Dl),
              "out": (B, T, Dl), "g_u": (B, H * T, Dv), "g_colsum": (B, H * T)}
    return {name: _Guarded(int(torch.Size(s).numel()), s) for name, s in shapes.items()}


def run(case, scratch="exact"):
    """The four entry points on a case (a None among g_a, g_c, g_z, g_l_ln, keep goes in as a null pointer) -> the nine
    outputs on the GPU.  ``scratch``: "exact" = the reported size, NaN-filled before each of the two calls that use it, or
    "large" = twice that and 1024 floats more, zeroed."""
    lib = _lib.load()
    dims = (case.B, case.T, case.H, case.Dv, case.Dl)
    n = int(lib.zira_text_side_scratch_floats(*dims))
    assert n == tc.geometry(*dims).scratch_floats
    ws = _Guarded(n) if scratch == "exact" else _Guarded(2 * n + 1024)
    if scratch != "exact":
        ws.body.zero_()
    i = {k: _dev(getattr(case, k)) for k in ("l_in", "ln_w", "ln_b", "W1", "b1", "O", "o0", "gamma", "keep", "u", "colsum", "g_a", "g_c",
                                             "g_z", "g_l_ln", "g")}
    W1T, OT = i["W1"].t().contiguous(), i["O"].t().contiguous()
    out = _outputs(case)
    o = {name: g.view for name, g in out.items()}
    rc = lib.zira_text_prep_fwd_f32(_p(i["l_in"]), _p(i["ln_w"]), _p(i["ln_b"]), case.eps, _p(i["W1"]), _p(i["b1"]), *dims, _p(o["l_ln"]),
                                    _p(o["a"]), _p(o["c"]), _p(o["z"]), _p(o["stats"]), _stream())
    assert rc == 0
    rc = lib.zira_text_prep_bwd_f32(_p(i["g_a"]), _p(i["g_c"]), _p(i["g_z"]), _p(i["g_l_ln"]), _p(i["l_in"]), _p(i["ln_w"]), _p(o["stats"]),
                                    _p(W1T), *dims, _p(ws.body), _p(o["g_l_in"]), _stream())
    assert rc == 0
    if scratch == "exact":
        ws.body.fill_(float("nan"))
    rc = lib.zira_text_out_fwd_f32(_p(i["u"]), _p(i["colsum"]), _p(o["l_ln"]), _p(i["O"]), _p(i["o0"]), _p(i["gamma"]), _p(i["keep"]), *dims,
                                   _p(ws.body), _p(o["out"]), _stream())
    assert rc == 0
    rc = lib.zira_text_out_bwd_f32(_p(i["g"]), _p(i["u"]), _p(i["colsum"]), _p(OT), _p(i["gamma"]), _p(i["keep"]), *dims, _p(o["g_u"]),
                                   _p(o["g_colsum"]), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert ws.intact(), "written outside the scratch of the reported size"
    for name, g in out.items():
        assert g.intact(), "%s: written outside the tensor" % name
    return o


def err(a, b64):
    """Largest error relative to the float64 tensor's own largest magnitude."""
    return float((a.double() - b64).abs().max() / b64.abs().max())


# Bars of the float64 comparisons: err(kernel) <= RATIO * err(fp32 composition on the same device) + FLOOR, both errors relative
# to the float64 tensor's largest magnitude.  FLOOR: four units of 2^-24 of that magnitude, for the figures on which the
# composition happens to be exact or nearly so.
# RATIO: measured on MI355X as the worst err(kernel) / err(composition) over the 9 shapes of textside_cases.SHAPES and the two
# draws (MEASURED_RATIO; 18 figures per output), doubled and rounded up to one digit.  No output is the composition's bits
# throughout (stats and g_u on 2 of 18, a and c on 1), and every error of the kernel stays below 8.2e-7 -- 14 units of 2^-24.
# The two largest:
#   c 1.97 at H Dv = 255, Dl = 100 with l_in x 8 (2.0e-7 against 1.0e-7, three units of 2^-24 against two; 1.28 at most on the
#     other shapes): a column's 100 products are one chain of fmaf in the order of k, beside a library GEMM that splits K;
#   a 1.90 on the degenerate shape (one row, Dl = 4; 5.0e-8 against 2.7e-8: both below one unit of 2^-24, the rounding of the
#     one l_ln value the single entry of a reads); 1.65 at most elsewhere (H Dv = 255 again: 3.6e-7 against 2.2e-7).
FLOOR = 4 * 2.0 ** -24
MEASURED_RATIO = {"l_ln": 1.65, "a": 1.90, "c": 1.97, "z": 1.55, "stats": 1.23, "g_l_in": 1.07, "out": 1.50, "g_u": 1.47, "g_colsum": 1.65}
RATIO = {"l_ln": 4.0, "a": 4.0, "c": 4.0, "z": 4.0, "stats": 3.0, "g_l_in": 3.0, "out": 4.0, "g_u": 3.0, "g_colsum": 4.0}


def check_against_f64(tag, case, got):
    """Print every figure, then assert the bar for each of the nine outputs."""
    want, comp = tc.reference_f64(case, DEV), tc.composition_all(case, DEV, torch.float32)
    figs = []
    for name in tc.OUTPUTS:
        figs.append((name, err(got[name], getattr(want, name)), err(getattr(comp, name), getattr(want, name)),
                     torch.equal(got[name], getattr(comp, name))))
        print("TXTFIG %s %s kernel %.3e composition %.3e same-bits %d" % ((tag,) + figs[-1]))
    for name, ek, ec, same in figs:
        assert ek <= RATIO[name] * ec + FLOOR, "%s %s: kernel %.3e, composition %.3e, bar %.3e" % (tag, name, ek, ec, RATIO[name] * ec + FLOOR)


@functools.lru_cache(maxsize=None)
def _random(i, gain=1.0):
    return tc.random_case(tc.SHAPES[i], gain=gain)


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_gather_weights_copy_l_ln_into_a_c_z(i):
    """textside_cases.exact_gather_case: one 1.0 per column of W1, b1 = 0 -- every entry of a, c, z is the kernel's own
    l_ln[m, (7 n + 3) mod Dl], bit for bit.  A wrong (b, t) or (h, d) map, a K chunk or a column tile lost or doubled, a lane
    of the LayerNorm beyond Dl let in: the copy is of another element."""
    case = tc.exact_gather_case(tc.SHAPES[i])
    got = run(case)
    assert bool(torch.isfinite(got["l_ln"]).all())
    for name, want in zip(("a", "c", "z"), tc.gathered(got["l_ln"], case)):
        assert torch.equal(got[name], want), name


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_integer_inputs_give_exact_results(i):
    """textside_cases.exact_integer_case: l_ln, a, c, z, out, g_u, g_colsum are float64's bit for bit whatever the order of
    the sums (keep in {0, 2} differs inside a row tile wherever a tile spans images)."""
    case = tc.exact_integer_case(tc.SHAPES[i])
    got, want = run(case), tc.reference_f64(case)
    for name in ("l_ln", "a", "c", "z", "out", "g_u", "g_colsum"):
        assert torch.equal(got[name].cpu().double(), getattr(want, name)), name


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_prep_backward_sums_integer_gradients_exactly(i):
    """Integer g_a / g_c / g_z with g_l_ln null, against the three null with g_l_ln = the exact integer product G W1^T: the
    finish kernel sees the same exact sums either way, so the two g_l_in are bit-identical -- unless a column of G was read
    from the wrong place, dropped or counted twice.  (ln_w from the random case: with the integer case's ln_w = 0 the
    gradient is 0.)"""
    case = tc.with_(tc.exact_integer_case(tc.SHAPES[i]), ln_w=_random(i).ln_w)
    gathered = run(tc.with_(case, g_l_ln=None))
    direct = run(tc.with_(case, g_a=None, g_c=None, g_z=None, g_l_ln=tc.integer_g_ln(case)))
    assert torch.equal(gathered["g_l_in"], direct["g_l_in"])
    want = tc.reference_f64(tc.with_(case, g_l_ln=None)).g_l_in              # (and neither is garbage)
    assert float(want.abs().max()) > 0 and err(gathered["g_l_in"].cpu(), want) < 1e-4
    # each of the three on its own as well: a column routed into another tensor's sum would cancel in the total only
    for name in ("g_a", "g_c", "g_z"):
        only = tc.with_(case, **{k: (getattr(case, k) if k == name else None) for k in tc.NULLABLE})
        assert torch.equal(run(only)["g_l_in"], run(tc.with_(only, **{name: None}, g_l_ln=tc.integer_g_ln(only)))["g_l_in"]), name


@pytest.mark.parametrize("gain", [1.0, 8.0])
@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_matches_float64_beside_the_composition(i, gain):
    """The random case, and a second draw with l_in and the gradients times 8: the nine outputs against float64, with the
    error of the fp32 composition on the same inputs and device as the yardstick (RATIO, FLOOR above)."""
    case = _random(i, gain)
    check_against_f64("%s gain %g" % (IDS[i], gain), case, run(case))


@pytest.mark.parametrize("i", WITH_A, ids=[IDS[i] for i in WITH_A])
def test_null_gradients_are_zero_gradients(i):
    """Each of g_a, g_c, g_z, g_l_ln null, singly and all but one, on the shapes whose mixed chunk holds columns of a: bit
    for bit the call with zero tensors in their place (the mixed chunk loads from a dummy address and discards the value)."""
    case = _random(i)
    sets = [(k,) for k in tc.NULLABLE] + [tuple(x for x in tc.NULLABLE if x != k) for k in tc.NULLABLE]
    full = run(case)["g_l_in"]
    for null in sets:
        got = run(tc.with_(case, **{k: None for k in null}))["g_l_in"]
        zero = run(tc.with_(case, **{k: torch.zeros_like(getattr(case, k)) for k in null}))["g_l_in"]
        assert bool(torch.isfinite(got).all()) and torch.equal(got, zero), null
        assert not torch.equal(got, full), null


def _keeps(B):
    if B == 1:
        return [[2.0], [0.0]]
    pattern = [2.0, 0.0, 4.0, 0.5, 2.0][:B]
    return [pattern, pattern[::-1]]


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_keep_scales_each_image(i):
    """keep null is keep = 1, bit for bit.  An image with keep[b] = 0 has out = l_ln, g_u = 0 and g_colsum = 0 exactly; an
    image with a power of two f has the bits of the run without stochastic depth on gamma f (scale = gamma[n] keep[b] is then
    the same fp32 number), also where one row tile spans images with different factors."""
    case = _random(i)
    B = case.B
    null, ones = run(tc.with_(case, keep=None)), run(tc.with_(case, keep=torch.ones(B)))
    for name in ("out", "g_u", "g_colsum"):
        assert torch.equal(null[name], ones[name]), name
    for keep in _keeps(B):
        got = run(tc.with_(case, keep=torch.tensor(keep)))
        for f in sorted(set(keep)):
            images = [b for b in range(B) if keep[b] == f]
            if f == 0.0:
                assert torch.equal(got["out"][images], got["l_ln"][images])
                assert bool((got["g_u"][images] == 0).all()) and bool((got["g_colsum"][images] == 0).all())
                continue
            plain = null if f == 1.0 else run(tc.with_(case, keep=None, gamma=case.gamma * f))
            for name in ("out", "g_u", "g_colsum"):
                assert torch.equal(got[name][images], plain[name][images]), (name, keep, f)


@pytest.mark.parametrize("i", SEVERAL_IMAGES, ids=[IDS[i] for i in SEVERAL_IMAGES])
def test_image_with_colsum_zero(i):
    """What the bi-softmax hands over for a fully padded image: colsum = 0 and u = 0 for the whole image.  The other images
    are bit for bit what they are with that image's colsum = 1 (its rows share row tiles with theirs); the empty image
    itself is 0 / 0: out and g_colsum are NaN on all of it and g_u is nowhere finite (stated in include/zira_msda.h)."""
    case = _random(i)
    B, empty = case.B, 1
    others = [b for b in range(B) if b != empty]
    u, colsum, one = case.u.clone(), case.colsum.clone(), case.colsum.clone()
    u[empty], colsum[empty], one[empty] = 0.0, 0.0, 1.0
    got, ref = run(tc.with_(case, u=u, colsum=colsum, keep=None)), run(tc.with_(case, u=u, colsum=one, keep=None))
    for name in ("out", "g_u", "g_colsum"):
        assert bool(torch.isfinite(got[name][others]).all()), name
        assert torch.equal(got[name][others], ref[name][others]), name
    assert bool(torch.isnan(got["out"][empty]).all()) and bool(torch.isnan(got["g_colsum"][empty]).all())
    assert not bool(torch.isfinite(got["g_u"][empty]).any())


def _calls(case, o, ws, dims, i, W1T, OT):
    """The four calls as (name, function, arguments, indices of the required pointers, outputs it writes)."""
    lib = _lib.load()
    s = _stream()
    return [
        ("prep_fwd", lib.zira_text_prep_fwd_f32,
         [_p(i["l_in"]), _p(i["ln_w"]), _p(i["ln_b"]), case.eps, _p(i["W1"]), _p(i["b1"]), *dims, _p(o["l_ln"]), _p(o["a"]), _p(o["c"]),
          _p(o["z"]), _p(o["stats"]), s], [0, 1, 2, 4, 5, 11, 12, 13, 14, 15]),
        ("prep_bwd", lib.zira_text_prep_bwd_f32,
         [_p(i["g_a"]), _p(i["g_c"]), _p(i["g_z"]), _p(i["g_l_ln"]), _p(i["l_in"]), _p(i["ln_w"]), _p(i["stats"]), _p(W1T), *dims,
          _p(ws.body), _p(o["g_l_in"]), s], [4, 5, 6, 7, 13, 14]),
        ("out_fwd", lib.zira_text_out_fwd_f32,
         [_p(i["u"]), _p(i["colsum"]), _p(i["l_ln"]), _p(i["O"]), _p(i["o0"]), _p(i["gamma"]), _p(i["keep"]), *dims, _p(ws.body),
          _p(o["out"]), s], [0, 1, 2, 3, 4, 5, 12, 13]),
        ("out_bwd", lib.zira_text_out_bwd_f32,
         [_p(i["g"]), _p(i["u"]), _p(i["colsum"]), _p(OT), _p(i["gamma"]), _p(i["keep"]), *dims, _p(o["g_u"]), _p(o["g_colsum"]), s],
         [0, 1, 2, 3, 4, 11, 12]),
    ]


def test_refusals_launch_nothing():
    """Dl = 257, B = 0 and a null pointer in the place of each required one: hipErrorInvalidValue from all four entry points,
    every NaN-filled output and the NaN-filled scratch untouched; zira_text_side_scratch_floats is 0 for the bad dimensions.
    (The buffers are those of Dl = 257 throughout, so that a call let through would still stay inside them.)"""
    lib = _lib.load()
    shape = (2, 16, 2, 64, 257, "refused")
    case = tc.random_case(shape)
    i = {k: _dev(getattr(case, k)) for k in ("l_in", "ln_w", "ln_b", "W1", "b1", "O", "o0", "gamma", "keep", "u", "colsum", "g_a", "g_c", "g_z",
                                             "g_l_ln", "g")}
    i["stats"], i["l_ln"] = torch.ones(case.B * case.T, 2, device=DEV), i["l_in"].clone()
    W1T, OT = i["W1"].t().contiguous(), i["O"].t().contiguous()
    out = _outputs(case)
    o = {name: g.view for name, g in out.items()}
    ws = _Guarded(17 * case.B * case.T * 257)
    tried = 0
    for label, dims in (("Dl = 257", (2, 16, 2, 64, 257)), ("B = 0", (0, 16, 2, 64, 256)), ("null", (2, 16, 2, 64, 256))):
        assert int(lib.zira_text_side_scratch_floats(*dims)) == (0 if label != "null" else tc.geometry(*dims).scratch_floats)
        for name, fn, args, required in _calls(case, o, ws, dims, i, W1T, OT):
            for k in (required if label == "null" else [None]):
                a = list(args)
                if k is not None:
                    a[k] = None
                assert fn(*a) == EINVAL, (label, name, k)
                tried += 1
    torch.cuda.synchronize()
    assert tried == 2 * 4 + 10 + 6 + 8 + 7
    assert ws.untouched()
    for name, g in out.items():
        assert g.untouched(), name


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_two_runs_are_bit_identical(i):
    """No atomics, a fixed order of the partial sums."""
    case = _random(i, 8.0)
    one, two = run(case), run(case)
    for name in tc.OUTPUTS:
        assert torch.equal(one[name], two[name]), name


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_scratch_needs_no_initialisation_and_no_more_than_reported(i):
    """A NaN-filled scratch of exactly zira_text_side_scratch_floats for both calls that use it (run() checks the sentinels
    round it and round the outputs) gives bit for bit what a zeroed one of twice the size and 1024 floats more gives."""
    case = _random(i)
    exact, large = run(case, "exact"), run(case, "large")
    for name in tc.OUTPUTS:
        assert bool(torch.isfinite(exact[name]).all()), name
        assert torch.equal(exact[name], large[name]), name
