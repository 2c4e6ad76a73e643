"""The inputs of the fused bi-softmax's GPU tests (tests/bisoftmax_cases.py), proven where there is no GPU: the exact cases give
their claimed results in float64 and in fp32 torch, bit for bit; the gradient with both maxima held constant is the full
gradient wherever e and colsum are used as e / colsum; the clamp cases are observable; the fully-masked conventions hold
in the reference; and every shape reaches the branch of the launcher that its note names."""
import functools

import pytest
import torch

import bisoftmax_cases as bc

IDS = [bc.shape_id(s) for s in bc.SHAPES]
CLAMP_IDS = [bc.shape_id(s) for s in bc.CLAMP_SHAPES]


@functools.lru_cache(maxsize=None)
def _exact(i):
    return bc.exact_case(bc.SHAPES[i], seed=100 + i)


@pytest.mark.parametrize("i", range(len(bc.SHAPES)), ids=IDS)
def test_exact_case_is_exact_in_float64_and_in_fp32(i):
    case = _exact(i)
    ref, comp = bc.reference_all(case), bc.composition_all(case)
    for name in bc.OUTPUTS:
        want = getattr(case.want, name)
        assert torch.equal(getattr(ref, name).float(), want), name     # float64, rounded to fp32 (exp(-122) = 1e-53 -> 0)
        assert torch.equal(getattr(comp, name), want), name            # the fp32 chain + autograd (-0.0 == 0.0)
    assert float(case.want.gmax) == 3.0
    ones = case.want.pv.view(case.B, case.N, case.H, case.T).sum(-1)
    assert bool((ones == 1).all()) and bool(((case.want.pv == 0) | (case.want.pv == 1)).all())
    if case.mask_l is not None:                                        # nobody selects a masked text token
        assert float(case.want.pv.view(case.B, case.N, case.H, case.T)[case.mask_l[:, None, None, :].expand(-1, case.N, case.H, -1)].sum()) == 0


def test_exact_cases_hold_what_they_are_meant_to_catch():
    """Some column is selected by masked rows only (colmax counts them, colsum = 0); some column by nobody (e = 1 on every
    live row); the selection depends on each of b, n, h; g_c reaches past 2^11 at N = 40000 and stays an integer below 2^24."""
    case = _exact(next(i for i, s in enumerate(bc.SHAPES) if s[:4] == (2, 9, 4, 194)))
    col_selected = case.want.colmax == case.c
    assert bool((col_selected & (case.want.colsum == 0)).any())
    assert bool((~col_selected & (case.want.colsum == (case.N - case.mask_v.sum(1))[:, None])).any())
    pv = _exact(0).want.pv.view(2, 117, 4, 9)
    assert not torch.equal(pv[0], pv[1]) and not torch.equal(pv[:, 0], pv[:, 1]) and not torch.equal(pv[:, :, 0], pv[:, :, 1])
    big = _exact(next(i for i, s in enumerate(bc.SHAPES) if s[1] == 40000))
    assert 2.0 ** 11 < float(big.want.g_c.abs().max()) < 2.0 ** 24 and float(big.want.colsum.max()) == 40000 - 1234


@pytest.mark.parametrize("gain", [1.0, 8.0])
@pytest.mark.parametrize("i", range(len(bc.SHAPES)), ids=IDS)
def test_gradient_with_constant_maxima_is_the_full_gradient(i, gain):
    """Full float64 autograd through pv and p_l = e / colsum with the maxima NOT detached, against reference_f64 (maxima
    constant) fed with the gradients that e / colsum hands back: the paths through the maxima vanish."""
    case = bc.randn_case(bc.SHAPES[i], seed=200 + i, gain=gain)
    xm, c = case.xm.double().requires_grad_(), case.c.double().requires_grad_()
    pv, e, colsum, colmax, gmax = bc.composition(xm, c, case.mask_l, case.mask_v, case.H, case.T, case.stable, case.clamp_lo,
                                                 case.clamp_hi, detach_maxima=False)
    assert float(colsum.detach().min()) > 0
    g_pv, g_pl = case.g_pv.double(), case.g_e.double()
    want_xm, want_c = torch.autograd.grad((pv * g_pv).sum() + (e / colsum[:, None] * g_pl).sum(), [xm, c])
    e, colsum = e.detach(), colsum.detach()
    ref = bc.reference_f64(case.xm, case.c, case.mask_l, case.mask_v, case.H, case.T, case.stable, case.clamp_lo, case.clamp_hi,
                           g_pv, g_pl / colsum[:, None], -(g_pl * e).sum(1) / colsum ** 2)
    # (g_c is the column sum of g_xm, to which p_l adds nothing -- at T = 1 it is identically 0: both on the scale of g_xm)
    scale = want_xm.abs().max()
    for name, got, want in (("g_xm", ref.g_xm, want_xm), ("g_c", ref.g_c, want_c)):
        err = float((got - want).abs().max() / scale)
        assert err < 1e-12, (name, err)
    for name, got in (("pv", pv), ("e", e), ("colsum", colsum), ("colmax", colmax), ("gmax", gmax)):
        assert float((getattr(ref, name) - got.detach()).abs().max()) < 1e-12, name


def _spread(pv, case):
    """[B, N, H]: largest minus smallest pv over the live text tokens of a group."""
    p = pv.view(case.B, case.N, case.H, case.T)
    dead = torch.zeros(case.B, 1, 1, case.T, dtype=torch.bool) if case.mask_l is None else case.mask_l.view(case.B, 1, 1, case.T)
    return p.masked_fill(dead, -1.0).amax(-1) - p.masked_fill(dead, 2.0).amin(-1)


@pytest.mark.parametrize("shape", bc.CLAMP_SHAPES, ids=CLAMP_IDS)
def test_clamp_case_is_observable(shape):
    """With the clamp: the designated groups are exactly uniform, g_xm is exactly 0 where the clamp clipped and nonzero on the
    entries exactly on a bound -- in float64 and in the fp32 chain.  With the flag switched off the same groups are not
    uniform (some pv moves by half a uniform share or more) and the clipped entries carry gradient: a kernel that drops the
    clamp or its gradient mask cannot pass."""
    case = bc.clamp_case(shape, seed=5)
    B, N, H, T, stable = shape[:5]
    assert bool(case.uniform.any()) and bool(case.clipped.any()) and bool(case.edge.any())
    groups = case.clipped.view(B, N, H, T)
    assert bool((groups.any(-1) & ~groups.all(-1) & ~case.uniform).any()) == bool(stable)      # groups that straddle the clamp
    for res in (bc.reference_all(case), bc.composition_all(case)):
        assert float(_spread(res.pv, case)[case.uniform].max()) == 0.0
        assert float(res.g_xm[case.clipped].abs().max()) == 0.0
        assert float(res.g_xm[case.edge].abs().min()) > 0.0
        assert bool(torch.isfinite(res.g_xm).all())
    off = bc.reference_f64(case.xm, case.c, case.mask_l, case.mask_v, H, T, stable, 0 if stable else 1, 1 if stable else 0,
                           case.g_pv, case.g_e, case.g_colsum)
    clipped_high = case.clipped & (case.xm > 0)
    watched = case.uniform if stable else clipped_high.view(B, N, H, T).any(-1)
    on = bc.reference_all(case)
    moved = (off.pv - on.pv).abs().view(B, N, H, T).amax(-1)            # a uniform pv is 1 / live >= 1 / T
    assert float(moved[watched].min()) >= 0.5 / T and float(_spread(off.pv, case)[watched].min()) >= 0.5 / T
    assert float(off.g_xm[case.clipped if stable else clipped_high].abs().max()) > 1e-3


def test_reference_f64_fully_masked_conventions():
    shape = bc.SHAPES[0]
    case = bc.randn_case(shape, seed=3)
    B, N, H, T = shape[:4]
    plain = bc.reference_all(case)
    # every text token of image 0 masked: pv = 0 there, nothing through g_pv, no NaN; image 1 as before
    text = bc.fully_masked(case, text_image=0)
    r = bc.reference_all(text)
    for name in bc.OUTPUTS:
        assert bool(torch.isfinite(getattr(r, name)).all()), name
    assert float(r.pv[0].abs().max()) == 0.0
    no_gpv = bc.types.SimpleNamespace(**text.__dict__)
    no_gpv.g_pv = text.g_pv.clone()
    no_gpv.g_pv[0] = 0
    assert torch.equal(r.g_xm, bc.reference_all(no_gpv).g_xm)
    for name in bc.OUTPUTS:
        if name != "gmax":
            assert torch.equal(getattr(r, name)[1], getattr(plain, name)[1]), name
    assert torch.equal(r.e, plain.e) and torch.equal(r.colsum, plain.colsum)               # (the text mask does not touch e)
    comp = bc.composition_all(text)
    assert float(comp.pv[0].abs().max()) == 0.0 and bool(torch.isfinite(comp.g_xm).all())
    # every image token of image 0 masked: e = 0, colsum = 0 there; image 1 as before (the maxima count masked rows)
    r = bc.reference_all(bc.fully_masked(case, rows_image=0))
    assert float(r.e[0].abs().max()) == 0.0 and float(r.colsum[0].abs().max()) == 0.0
    for name in bc.OUTPUTS:
        assert bool(torch.isfinite(getattr(r, name)).all()), name
        if name != "gmax":
            assert torch.equal(getattr(r, name)[1], getattr(plain, name)[1]), name
    assert torch.equal(r.pv, plain.pv) and torch.equal(r.colmax, plain.colmax) and torch.equal(r.gmax, plain.gmax)


def test_torch_clamp_passes_the_gradient_on_its_bounds():
    x = torch.tensor([-50000.5, -50000.0, 0.0, 50000.0, 50000.5], dtype=torch.float64, requires_grad=True)
    torch.clamp(x, min=-bc.CLAMP, max=bc.CLAMP).sum().backward()
    assert x.grad.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]


@pytest.mark.parametrize("shape", bc.SHAPES + bc.CLAMP_SHAPES + bc.CONVENTION_SHAPES,
                         ids=IDS + ["clamp-" + i for i in CLAMP_IDS] + ["convention-" + bc.shape_id(s) for s in bc.CONVENTION_SHAPES])
def test_note_names_the_branch_the_shape_reaches(shape):
    """The note's first part is what the launcher's predicates (restated in bisoftmax_cases.dispatch) give for the shape, and
    the library's own workspace size -- rows per tile, the block caps, the wave form's switch -- agrees with the restatement."""
    from ziragroundingdino_amd import _lib

    B, N, H, T = shape[:4]
    assert shape[9].split(" | ")[0] == bc.branch_name(shape)
    assert int(_lib.load().zira_bisoftmax_workspace_floats(B, N, H, T)) == bc.dispatch(N, H, T).workspace_floats(B)


def test_shapes_cover_every_branch():
    names = [s[9].split(" | ")[0] for s in bc.SHAPES]
    for wanted in ("tile G=1 vec strided colmax-rows=79", "tile G=8 scalar", "tile G=16 vec", "tile G=16 scalar misaligned", "tile G=32 vec",
                   "tile G=64 vec", "t32<1>", "t32<2>", "t32<4>", "wave KPL=4", "wave KPL=4 strided", "wave KPL=8", "wave KPL=12",
                   "wave KPL=13", "wave KPL=16", "walk vec", "walk vec strided"):
        assert wanted in names, wanted
    flags = {s[4:7] for s in bc.SHAPES}
    assert {(1, 1, 1), (0, 1, 1), (1, 0, 0)} <= flags
    for flag in ((0, 1, 1), (1, 0, 0)):                      # each flag setting in the lane-group and in the wave form
        assert {bc.dispatch(*s[1:4]).fwd for s in bc.SHAPES if s[4:7] == flag} == {"tile", "wave"}
    assert any(s[7] is None for s in bc.SHAPES) and any(s[8] is None for s in bc.SHAPES)        # null mask pointers
    # the figures the notes quote, and both sides of every threshold of the launcher
    d = bc.dispatch(117, 4, 9)
    assert (d.rows_per_tile, d.tiles, 117 - 2 * 56) == (56, 3, 5)
    d = bc.dispatch(40000, 4, 1)
    assert (d.rows_per_tile, d.tiles, d.row_blocks, d.colmax_chunks, d.colmax_rows, d.strided) == (64, 625, 512, 512, 79, True)
    assert bc.dispatch(32768, 4, 1).colmax_rows == 64 and bc.dispatch(32769, 4, 1).colmax_rows == 65
    assert [bc.dispatch(9, 1, ht).kpl for ht in (65, 256, 257, 512, 513, 768, 769, 832, 833, 1024)] == [4, 4, 8, 8, 12, 12, 13, 13, 16, 16]
    assert bc.dispatch(9, 4, 209).kpl == 16 and bc.dispatch(9, 4, 208).kpl == 13
    assert bc.dispatch(9, 4, 256).fwd == "wave" and bc.dispatch(6, 8, 129).fwd == "tile" and bc.dispatch(6, 8, 129).G == 0
    assert bc.dispatch(20, 2, 64).G == 64 and bc.dispatch(20, 1, 65).fwd == "wave"
    assert bc.dispatch(2048, 1, 65).strided is False and bc.dispatch(2049, 1, 65).strided is True
    assert bc.dispatch(512, 16, 128).strided is False and bc.dispatch(513, 16, 128).strided is True
    assert bc.dispatch(1, 16, 128) is not None and bc.dispatch(1, 1, 2049) is None
