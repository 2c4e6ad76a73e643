"""The inputs and the float64 reference of the fused text side's GPU tests (tests/textside_cases.py), proven where there is no
GPU: the closed-form backwards are autograd's, the layout maps are the permutes of the ATen block, every shape reaches the
chunk classes and edges its note names (by the launcher's arithmetic restated in textside_cases.geometry, which the
library's own scratch size is held to), and the exact-integer inputs are exact."""
import functools

import pytest
import torch

import textside_cases as tc

IDS = [tc.shape_id(s) for s in tc.SHAPES]


def _geo(shape):
    return tc.geometry(*shape[:5])


@functools.lru_cache(maxsize=None)
def _random(i, gain=1.0):
    return tc.random_case(tc.SHAPES[i], gain=gain)


@pytest.mark.parametrize("gain", [1.0, 8.0])
@pytest.mark.parametrize("i", range(len(tc.SHAPES)), ids=IDS)
def test_reference_backward_is_autograd_of_the_float64_composition(i, gain):
    """reference_f64 (closed forms) against composition_all in float64 (F.layer_norm, addmm, permutes + autograd): all nine
    outputs to 1e-12 of the tensor's largest magnitude."""
    case = _random(i, gain)
    ref, comp = tc.reference_f64(case), tc.composition_all(case, dtype=torch.float64)
    for name in tc.OUTPUTS:
        want, got = getattr(comp, name), getattr(ref, name)
        assert got.shape == want.shape, name
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name


@pytest.mark.parametrize("i", [2, 3, 5], ids=[IDS[i] for i in (2, 3, 5)])
def test_reference_with_null_gradients_and_without_keep(i):
    """A None gradient is a zero gradient, keep = None is keep = 1, in the reference and in the composition."""
    case = _random(i)
    for null in tc.NULLABLE:
        none = tc.reference_f64(tc.with_(case, **{null: None}))
        zero = tc.reference_f64(tc.with_(case, **{null: torch.zeros_like(getattr(case, null))}))
        comp = tc.composition_all(tc.with_(case, **{null: None}), dtype=torch.float64)
        assert torch.equal(none.g_l_in, zero.g_l_in) and not torch.equal(none.g_l_in, tc.reference_f64(case).g_l_in), null
        assert float((none.g_l_in - comp.g_l_in).abs().max()) <= 1e-12 * float(comp.g_l_in.abs().max()), null
    none, ones = tc.reference_f64(tc.with_(case, keep=None)), tc.reference_f64(tc.with_(case, keep=torch.ones(case.B)))
    comp = tc.composition_all(tc.with_(case, keep=None), dtype=torch.float64)
    for name in ("out", "g_u", "g_colsum"):
        assert torch.equal(getattr(none, name), getattr(ones, name)), name
        assert float((getattr(none, name) - getattr(comp, name)).abs().max()) <= 1e-12 * float(getattr(comp, name).abs().max()), name


@pytest.mark.parametrize("i", range(len(tc.SHAPES)), ids=IDS)
def test_layout_maps_are_the_permutes_of_the_dense_product(i):
    """scatter_acz / gather_acz / rows_of_u / u_of_rows (index arithmetic from the header) against permute / view of a dense
    [M, N1] product whose entries name their own (row, column)."""
    B, T, H, Dv, Dl, note = tc.SHAPES[i]
    M, HD = B * T, H * Dv
    N1 = 2 * HD + H
    P = (torch.arange(M, dtype=torch.float64)[:, None] * 4096 + torch.arange(N1, dtype=torch.float64)[None, :])
    a, c, z = tc.scatter_acz(P, B, T, H, Dv)
    P3 = P.view(B, T, N1)
    assert torch.equal(a, P3[..., :HD].reshape(B, T, H, Dv).permute(0, 3, 2, 1).reshape(B, Dv, H * T))
    assert torch.equal(c, P3[..., HD:HD + H].permute(0, 2, 1).reshape(B, H * T))
    assert torch.equal(z, P3[..., HD + H:].reshape(B, T, H, Dv).permute(0, 2, 1, 3).reshape(B, H * T, Dv))
    assert torch.equal(tc.gather_acz(a, c, z, B, T, H, Dv, P), P)
    assert torch.equal(tc.gather_acz(None, c, None, B, T, H, Dv, P)[:, HD:HD + H], P[:, HD:HD + H])
    U = P[:, :HD].contiguous()
    u = tc.u_of_rows(U, B, T, H, Dv)
    assert torch.equal(u, U.view(B, T, H, Dv).permute(0, 2, 1, 3).reshape(B, H * T, Dv))
    assert torch.equal(tc.rows_of_u(u, B, T, H, Dv), U)


def test_exact_gather_selects_one_row_per_column():
    for shape in tc.SHAPES:
        case = tc.exact_gather_case(shape)
        assert bool((case.W1.sum(0) == 1).all()) and bool(((case.W1 == 0) | (case.W1 == 1)).all()) and float(case.b1.abs().max()) == 0
        ref = tc.reference_f64(case)
        a, c, z = tc.gathered(ref.l_ln, case)
        assert torch.equal(a, ref.a) and torch.equal(c, ref.c) and torch.equal(z, ref.z)
    # neighbouring columns read different rows, and the rows of one head's columns are not those of the next head's
    case = tc.exact_gather_case(tc.SHAPES[2])
    k = tc.gather_row(torch.arange(case.W1.shape[1]), case.Dl)
    assert bool((k[1:] != k[:-1]).all()) and not torch.equal(k[:case.Dv], k[case.Dv:2 * case.Dv])


@pytest.mark.parametrize("i", range(len(tc.SHAPES)), ids=IDS)
def test_exact_integer_case_is_exact(i):
    """Every accumulation stays below 2^22 units of its terms' step -- a quarter of what fp32 holds exactly --, the float64
    results are fp32 numbers, and the fp32 composition gives the same bits."""
    case = tc.exact_integer_case(tc.SHAPES[i])
    assert tc.exact_integer_bound(case) < 2.0 ** 22
    ref, comp = tc.reference_f64(case), tc.composition_all(case)
    for name in ("l_ln", "a", "c", "z", "out", "g_u", "g_colsum"):
        r = getattr(ref, name)
        assert torch.equal(r.float().double(), r), name
        assert torch.equal(getattr(comp, name).double(), r), name
    assert torch.equal(ref.l_ln, case.ln_b.double().expand_as(ref.l_ln))
    g_ln = tc.integer_g_ln(case)
    assert torch.equal(g_ln.double().frac(), torch.zeros_like(g_ln, dtype=torch.float64)) and float(g_ln.abs().max()) < 2.0 ** 22
    assert set(case.keep.tolist()) <= {0.0, 2.0} and (case.B == 1 or set(case.keep.tolist()) == {0.0, 2.0})
    assert set(case.colsum.unique().tolist()) <= {0.5, 1.0, 2.0, 4.0} and set(case.gamma.abs().unique().tolist()) <= {0.5, 1.0, 2.0, 4.0}


def test_random_case_is_what_the_docstring_says():
    for shape in tc.SHAPES:
        case = tc.random_case(shape)
        assert 0.5 <= float(case.colsum.min()) and float(case.colsum.max()) <= 50.0
        assert 0.5 <= float(case.gamma.abs().min()) and float(case.gamma.abs().max()) <= 1.5
        assert 0.5 <= float(case.ln_w.min()) and float(case.ln_w.max()) <= 1.5
        keep = set(round(k, 6) for k in case.keep.tolist())
        assert keep <= {0.0, round(1 / 0.7, 6)} and (case.B == 1 or len(keep) == 2)
        eight = tc.random_case(shape, gain=8.0)
        assert torch.equal(eight.l_in, case.l_in * 8) and torch.equal(eight.g_z, case.g_z * 8) and torch.equal(eight.u, case.u)


@pytest.mark.parametrize("i", range(len(tc.SHAPES)), ids=IDS)
def test_library_reports_the_restated_scratch_size(i):
    from ziragroundingdino_amd import _lib

    assert int(_lib.load().zira_text_side_scratch_floats(*tc.SHAPES[i][:5])) == _geo(tc.SHAPES[i]).scratch_floats


def test_refused_dimensions():
    from ziragroundingdino_amd import _lib

    lib = _lib.load()
    for dims in ((2, 16, 2, 64, 257), (0, 16, 2, 64, 128), (2, 0, 2, 64, 128), (2, 16, 0, 64, 128), (2, 16, 2, 0, 128), (2, 16, 2, 64, 0)):
        assert tc.geometry(*dims) is None and int(lib.zira_text_side_scratch_floats(*dims)) == 0, dims
    assert tc.geometry(2, 16, 2, 64, 256) is not None and int(lib.zira_text_side_scratch_floats(2, 16, 2, 64, 256)) > 0


def _kinds(g):
    """Chunk classes of a shape: a, z, mixed+a (a mixed chunk that holds columns of a), mixed-a."""
    return [kind if kind != "mixed" else ("mixed+a" if has_a else "mixed-a") for k0, kn, kind, has_a, has_c, has_z in g.prep_chunks]


def test_each_shape_reaches_what_its_note_names():
    geo = {s[:5]: _geo(s) for s in tc.SHAPES}
    g = geo[(2, 32, 4, 256, 256)]
    assert (g.prep_parts, g.N1, g.HD) == (17, 2052, 1024) and _kinds(g) == ["a"] * 8 + ["mixed-a"] + ["z"] * 8
    assert g.prep_chunks[8][:2] == (1024, 128) and g.prep_chunks[8][3:] == (False, True, True) and g.prep_chunks[-1][1] == 4
    assert g.fwd_chunks == [128, 128] and g.out_kn == [128] * 8
    g = geo[(1, 195, 4, 256, 256)]
    assert g.M == 195 and len(g.row_tiles) == 7 and g.row_tiles[-1] == (192, 3)
    g = geo[(3, 9, 3, 32, 96)]
    assert (g.HD, g.N1) == (96, 195) and _kinds(g) == ["mixed+a", "z"] and g.prep_chunks[0][3:] == (True, True, True)
    assert g.prep_chunks[1][:2] == (128, 67) and g.fwd_chunks == [96] and g.row_tiles == [(0, 27)] and g.images_per_tile == [3]
    g = geo[(2, 5, 3, 85, 100)]
    assert (g.HD, g.N1) == (255, 513) and _kinds(g) == ["a", "mixed+a", "mixed-a", "z", "z"]
    assert g.prep_chunks[1][3:] == (True, True, False) and g.prep_chunks[2][3:] == (False, True, True)     # c: 255 | 256, 257
    assert g.prep_chunks[-1][1] == 1 and g.dl_overhang == 28 and g.fwd_chunks == [100] and g.head_split_in_tile
    g = geo[(2, 33, 2, 40, 200)]
    assert g.M == 66 and g.row_tiles[-1] == (64, 2) and g.fwd_chunks == [128, 72] and g.out_kn == [80] and g.head_split_in_tile
    g = geo[(5, 13, 8, 20, 256)]
    assert g.M == 65 and g.HD == 160 and _kinds(g) == ["a", "mixed+a", "z"] and g.prep_chunks[1][3:] == (True, True, True)
    assert g.prep_chunks[2][:2] == (256, 72) and max(g.images_per_tile) >= 3 and g.out_kn == [128, 32]
    g = geo[(2, 16, 2, 64, 128)]
    assert g.fwd_chunks == [128] and _kinds(g) == ["a", "mixed-a", "z"] and g.prep_chunks[2][1] == 2
    g = geo[(2, 16, 2, 64, 129)]
    assert g.fwd_chunks == [128, 1] and g.dl_overhang == 31
    g = geo[(1, 1, 1, 1, 4)]
    assert (g.M, g.N1, g.prep_parts, g.out_kn) == (1, 3, 1, [1]) and _kinds(g) == ["mixed+a"]


def test_shapes_cover_every_chunk_class_and_edge():
    geos = [_geo(s) for s in tc.SHAPES]
    kinds = [_kinds(g) for g in geos]
    for wanted in ("a", "z", "mixed+a", "mixed-a"):
        assert any(wanted in k for k in kinds), wanted
    assert any(sum(x.startswith("mixed") for x in k) == 2 for k in kinds)                 # two mixed chunks in one call
    assert any(g.prep_chunks[-1][1] < tc.KC for g in geos) and any(g.out_kn[-1] < tc.KC for g in geos)
    dls = [s[4] for s in tc.SHAPES]
    assert any(d < 128 for d in dls) and 128 in dls and any(128 < d < 256 for d in dls) and 256 in dls
    assert any(d % 32 for d in dls) and any(d % 4 for d in dls)
    assert any(g.M % 32 for g in geos) and any(g.M > 32 and g.M % 32 for g in geos)
    assert any(max(g.images_per_tile) > 1 for g in geos)
    assert any(s[3] % 32 and s[3] % 4 for s in tc.SHAPES) and any(s[3] < 64 for s in tc.SHAPES)     # Dv: odd, and below a wave
    # a keep of both kinds inside ONE row tile, in the cases the GPU tests run, wherever a tile spans images
    for shape in tc.SHAPES:
        B, T = shape[:2]
        if max(_geo(shape).images_per_tile) > 1:
            for case in (tc.random_case(shape), tc.exact_integer_case(shape)):
                rows = case.keep.repeat_interleave(T)
                assert any(len(set(rows[m0:m0 + n].tolist())) == 2 for m0, n in _geo(shape).row_tiles), shape
